// Per-frame depth export: the inverse of frame_ingest.hip's geometry.  A batch of SLAM-resolution disparity maps
// [H,W] (rows of GraphBuffer.disps_up) goes back through the crop and the resize of `StandardResize` to the frame's
// native size [H0,W0] and leaves as depth, in ONE pass:
//
//   disp [R,H,W] f32 --replicate-pad to (h1,w1) by (top,left)--> bilinear (H0,W0) --> depth_scale / d --> out [N,H0,W0]
//
// The padded map is never built: per axis, with n_res = h1 | w1, n_out = H0 | W0, off = top | left, n_in = H | W,
//   scale = float(n_res) / float(n_out),  src = max(fma(scale, dst + 0.5, -0.5), 0)   (F.interpolate, align_corners=False;
//                                                ONE fused multiply-add, as make_tap of frame_ingest.hip and for its reason)
//   src   = clamp(src - off, 0, n_in - 1)       (exact: off is a small integer; the clamp IS the replicate padding - the
//                                                band the centre crop removed takes the edge row / column of the cropped map)
//   i0 = int(src), i1 = min(i0 + 1, n_in - 1), l1 = src - i0, l0 = 1 - l1
//   d     = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * e)     (ingest's `blend`; the library is built with
//                                                                      -ffp-contract=off: six products and three sums)
//   depth = d > 0 ? depth_scale / d : 0                               (one correctly rounded division)
// Interpolation is in the disparity domain on purpose: disparity is linear in the image, depth is not.  f16 output is the
// round-to-nearest-even of the f32 value.  tests/depth_export_reference.py restates this in float64 and derives the
// error bound from this operation count.
//
// Layout (frame_ingest_kernel's): one output pixel per thread, 64 x 4 pixel tiles, the batch index in blockIdx.z.  A
// wave owns 64 x-adjacent pixels of one output row: its store is 128 (f16) / 256 (f32) contiguous bytes, its four taps
// walk two source rows front to back and come out of L1 / L2 (upsampling 384 x 512 -> 1080 x 1920, 64 output pixels
// span 18 source pixels).  Memory bound: H*W*4 B read once, H0*W0*(2|4) B written.
#include "export_taps.cuh"

namespace {

using namespace export_geom;  // TILE_W x TILE_H tiles, Tap, make_tap, blend: shared with depth_consistency.hip

struct ExportArgs {
  const float* disp;    // [R,H,W]
  const int64_t* rows;  // [N] or null
  void* out;            // [N,H0,W0]
  int R, H, W, H0, W0, top, left;
  float scale_y, scale_x;  // float(h1) / float(H0), float(w1) / float(W0)
  float depth_scale;
};

__device__ __forceinline__ void put(float* p, float v) { *p = v; }
__device__ __forceinline__ void put(half_t* p, float v) { *p = f2h(v); }

template <typename T>
__global__ __launch_bounds__(TILE_W* TILE_H) void depth_export_kernel(ExportArgs a) {
  const int x = blockIdx.x * TILE_W + (threadIdx.x & (TILE_W - 1));
  const int y = blockIdx.y * TILE_H + (threadIdx.x / TILE_W);
  if (x >= a.W0 || y >= a.H0) return;
  const int64_t n = blockIdx.z;
  const int64_t r = a.rows ? a.rows[n] : n;
  if (r < 0 || r >= a.R) return;  // out[n] stays as it is
  const Tap ty = make_tap(y, a.scale_y, a.top, a.H), tx = make_tap(x, a.scale_x, a.left, a.W);
  const float* m = a.disp + r * ((int64_t)a.H * a.W);
  const float* r0 = m + (int64_t)ty.i0 * a.W;
  const float* r1 = m + (int64_t)ty.i1 * a.W;
  const float d = blend(ty, tx, r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1]);
  const float depth = d > 0.0f ? __fdiv_rn(a.depth_scale, d) : 0.0f;
  put((T*)a.out + (n * a.H0 + y) * (int64_t)a.W0 + x, depth);
}

}  // namespace

VIPE_EXPORT int vipe_depth_export(const float* d_disp, const int64_t* d_rows, void* d_out, int out_dtype, int N, int R,
                                  int H, int W, int h1, int w1, int top, int left, int H0, int W0, float depth_scale,
                                  void* stream) {
  VIPE_CHECK_ARG(N >= 0 && R >= 0);
  VIPE_CHECK_ARG(geometry_ok(H, W, h1, w1, top, left, H0, W0));
  VIPE_CHECK_ARG(out_dtype == VIPE_F16 || out_dtype == VIPE_F32);
  VIPE_CHECK_ARG(d_rows || N <= R);
  const int by = (H0 + TILE_H - 1) / TILE_H;
  VIPE_CHECK_ARG(by <= 65535 && N <= 65535);  // grid.y / grid.z: an error, not a silent truncation
  if (N == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_disp && d_out);
  ExportArgs a;
  a.disp = d_disp; a.rows = d_rows; a.out = d_out;
  a.R = R; a.H = H; a.W = W; a.H0 = H0; a.W0 = W0; a.top = top; a.left = left;
  a.scale_y = (float)h1 / (float)H0;
  a.scale_x = (float)w1 / (float)W0;
  a.depth_scale = depth_scale;
  const dim3 grid((W0 + TILE_W - 1) / TILE_W, by, N);
  hipStream_t s = as_stream(stream);
  if (out_dtype == VIPE_F32) depth_export_kernel<float><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  else depth_export_kernel<half_t><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  return vipe_launch_status();
}
