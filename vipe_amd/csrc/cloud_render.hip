// Fused cloud -> camera images: a z-buffered splat of world points into B target cameras on the export grid.
//
// vipe_cloud_render, per point m (index index_base + m) and image b, with (R, t) = cams[b] as matrix and translation
// (the row's quaternion is normalised on load, as every pose row is) and I = intrinsics[b] (panorama: the grid):
//
//   Xc      = R X + t                        per row ((R0 X0 + R1 X1) + R2 X2) + t: three products, three sums
//   finite  = every component of Xc is finite;  not finite: the pair counts as OUTSIDE
//   valid   = cam::valid_point<CAM>(Xc)      Z > 0.1 (pinhole, MEI); range and pole rule (panorama);  else INVALID
//   z       = Xc.z (pinhole, MEI),  sqrtf((X X + Z Z) + Y Y) (panorama: a range, frame_depths' convention)
//   (x, y)  = cam::proj<CAM>(I, Xc)          SLAM-grid coordinates
//   p       = floorf(((x + off) + 0.5f) / scale) per axis, off = left | top, scale = float(w1) / float(W0) |
//             float(h1) / float(H0): the forward form of export_taps.cuh's mapping; the crop band is part of the image
//   unless -max_radius - 1 <= p <= n_out + max_radius on both axes (as floats; a NaN fails): OUTSIDE
//   q       = (0.5f * point_size) * foc / z, foc = fx / scale_x (pinhole, MEI; one division per image),
//             float(W0) / (2 pi) (panorama);   r = q >= max_radius ? max_radius : (int)q
//   pixels  = [px - r, px + r] x [py - r, py + r], rows clipped to [0, H0), columns clipped to [0, W0) - panorama: taken
//             modulo W0 instead;  none left: OUTSIDE
//   value   = (uint64)float_as_uint(z) << 32 | (uint32)(index_base + m);  atomicMin(&zbuf[b][y][x], value) per pixel
//
// z > 0, so its bit pattern orders as the number does; equal depths go to the lower index.  Minima are idempotent and
// commutative and no thread waits for another: the buffer depends only on the set of (point, index) pairs drawn - not
// on their order, on how the cloud is split over launches, on calling twice, or on the run.
//
// Layout: one thread per point, 256 per workgroup, the image in blockIdx.y.  Thread 0 builds the image's matrix, its
// intrinsics and foc once in LDS; every lane reads them back as wave-uniform values.  The three counters are summed per
// wave (ballot + popcount), per workgroup in LDS, and leave as at most three global atomics per workgroup.
//
// Two forms from this source.  VIPE_CLOUD_RENDER_PRELOAD = 0 issues the atomic always; = 1 (the library's) first does a
// plain 64-bit load of the pixel and skips the atomic when the stored value is already <= the candidate.  Values only
// decrease, so a stale read can only cost an atomic that was not needed: both forms leave the same buffer bit for bit
// (scratch/cloud_render_time.py builds both and checks; DESIGN.md section 19 has the times).
//
// vipe_cloud_resolve: one thread per pixel, no atomics: depth = the upper word as a float (0 where empty), the winner's
// index = the lower word (-1 where empty), its colour gathered from the point colours.
#include "export_taps.cuh"
#include "term_geom.cuh"

#ifndef VIPE_CLOUD_RENDER_PRELOAD
#define VIPE_CLOUD_RENDER_PRELOAD 1
#endif

namespace {

using export_geom::geometry_ok;
using u64 = unsigned long long;

constexpr int THREADS = 256;
constexpr int MAX_RADIUS = 4;
constexpr u64 EMPTY = ~0ull;

struct RenderArgs {
  const float *xyz, *cams, *intr;  // [M,3], [B,7], [B,idim]
  u64* zbuf;                       // [B,H0,W0]
  u64* stats;                      // [3]
  int64_t M;
  int index_base, idim, H, W, H0, W0, max_radius;
  float off_x, off_y, scale_x, scale_y, half_size;
};

enum { ST_DRAWN = 0, ST_INVALID = 1, ST_OUTSIDE = 2 };

struct Image {
  Rigid T;
  cam::Intr I;
  float foc;
};

template <int CAM>
__global__ __launch_bounds__(THREADS) void cloud_render_kernel(RenderArgs a) {
  __shared__ Image img;
  __shared__ unsigned wg_stats[3];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    img.T = to_rigid(lie::SE3<float>(a.cams + 7 * b));
    img.I = cam::load<CAM>(a.intr + (int64_t)b * a.idim, a.idim - 4, 1.0f, a.H, a.W);
    img.foc = CAM == VIPE_CAM_PANORAMA ? (float)a.W0 / (2.0f * cam::PI_F) : img.I.fx / a.scale_x;
  }
  if (threadIdx.x < 3) wg_stats[threadIdx.x] = 0;
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  int what = -1;  // lanes past the last point count nowhere
  if (m < a.M) {
    what = ST_OUTSIDE;
    const float X0 = a.xyz[3 * m], X1 = a.xyz[3 * m + 1], X2 = a.xyz[3 * m + 2];
    const Rigid& T = img.T;
    const float X = T.R[0] * X0 + T.R[1] * X1 + T.R[2] * X2 + T.t[0];
    const float Y = T.R[3] * X0 + T.R[4] * X1 + T.R[5] * X2 + T.t[1];
    const float Z = T.R[6] * X0 + T.R[7] * X1 + T.R[8] * X2 + T.t[2];
    const float big = __builtin_inff();
    const bool finite = fabsf(X) < big && fabsf(Y) < big && fabsf(Z) < big;  // false for a NaN
    if (finite && !cam::valid_point<CAM>(X, Y, Z)) what = ST_INVALID;
    if (finite && what != ST_INVALID) {
      const float z = CAM == VIPE_CAM_PANORAMA ? sqrtf((X * X + Z * Z) + Y * Y) : Z;
      float x, y, Jp[2][3], Jf[2][1];
      cam::proj<CAM, false, 0>(img.I, X, Y, Z, x, y, Jp, Jf);
      const float pxf = floorf(((x + a.off_x) + 0.5f) / a.scale_x);
      const float pyf = floorf(((y + a.off_y) + 0.5f) / a.scale_y);
      const float lo = (float)(-a.max_radius - 1);
      const bool in_band = pxf >= lo && pxf <= (float)(a.W0 + a.max_radius) && pyf >= lo && pyf <= (float)(a.H0 + a.max_radius);
      if (in_band) {  // only now do the positions become integers: |p| <= 2^24 + 5 by the entry point's size limits
        const int px = (int)pxf, py = (int)pyf;
        const float q = a.half_size * img.foc / z;
        const int r = q >= (float)a.max_radius ? a.max_radius : (int)q;  // q >= 0 and not a NaN: z > 0 is finite
        const int y0 = max(py - r, 0), y1 = min(py + r, a.H0 - 1);
        int x0 = px - r, x1 = px + r;
        if constexpr (CAM != VIPE_CAM_PANORAMA) x0 = max(x0, 0), x1 = min(x1, a.W0 - 1);
        if (y0 <= y1 && x0 <= x1) {
          what = ST_DRAWN;
          const u64 value = ((u64)__float_as_uint(z) << 32) | (u64)(unsigned)(a.index_base + (int)m);
          u64* plane = a.zbuf + (int64_t)b * a.H0 * a.W0;
          for (int yy = y0; yy <= y1; ++yy) {
            u64* row = plane + (int64_t)yy * a.W0;
            for (int xx = x0; xx <= x1; ++xx) {
              int col = xx;
              if constexpr (CAM == VIPE_CAM_PANORAMA) col = ((xx % a.W0) + a.W0) % a.W0;
              u64* p = row + col;
#if VIPE_CLOUD_RENDER_PRELOAD
              if (*p <= value) continue;
#endif
              atomicMin(p, value);
            }
          }
        }
      }
    }
  }
  const int lane = lane_id();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const u64 mask = __ballot(what == k);
    if (mask != 0 && lane == 0) atomicAdd(wg_stats + k, (unsigned)__popcll(mask));
  }
  __syncthreads();
  if (threadIdx.x < 3 && wg_stats[threadIdx.x]) atomicAdd(a.stats + threadIdx.x, (u64)wg_stats[threadIdx.x]);
}

struct ResolveArgs {
  const u64* zbuf;           // [B,H0,W0]
  void* depth;               // [B,H0,W0]
  const unsigned char* rgb;  // [M_total,3] or null
  unsigned char* rgb_out;    // [B,H0,W0,3] or null
  int* index;                // [B,H0,W0] or null
  int64_t total, M_total;
};

__device__ __forceinline__ void put(float* p, float v) { *p = v; }
__device__ __forceinline__ void put(half_t* p, float v) { *p = f2h(v); }

template <typename T>
__global__ __launch_bounds__(THREADS) void cloud_resolve_kernel(ResolveArgs a) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.total) return;
  const u64 v = a.zbuf[i];
  const bool empty = v == EMPTY;
  const int idx = empty ? -1 : (int)(unsigned)(v & 0xffffffffull);
  put((T*)a.depth + i, empty ? 0.0f : __uint_as_float((unsigned)(v >> 32)));
  if (a.index) a.index[i] = idx;
  if (a.rgb_out) {
    const bool ok = idx >= 0 && idx < a.M_total;  // an index past the colours is a caller error: 0, never a fault
#pragma unroll
    for (int c = 0; c < 3; ++c) a.rgb_out[i * 3 + c] = ok ? a.rgb[(int64_t)idx * 3 + c] : (unsigned char)0;
  }
}

}  // namespace

VIPE_EXPORT int vipe_cloud_render(const float* d_xyz, int64_t M, int index_base, const float* d_cams,
                                  const float* d_intrinsics, int intr_dim, int camera, int B, int H, int W, int h1, int w1,
                                  int top, int left, int H0, int W0, float point_size, int max_radius, int64_t* d_zbuf,
                                  int64_t* d_stats, void* stream) {
  VIPE_CHECK_ARG(M >= 0 && B >= 0);
  VIPE_CHECK_ARG(index_base >= 0 && M <= (int64_t)0x7fffffff - index_base);
  VIPE_CHECK_ARG(geometry_ok(H, W, h1, w1, top, left, H0, W0));
  VIPE_CHECK_ARG(H0 <= (1 << 24) && W0 <= (1 << 24));  // pixel positions stay exact as floats
  VIPE_CHECK_ARG(camera == VIPE_CAM_PINHOLE || camera == VIPE_CAM_MEI || camera == VIPE_CAM_PANORAMA);
  VIPE_CHECK_ARG(intr_dim == (camera == VIPE_CAM_MEI ? 5 : 4));
  if (camera == VIPE_CAM_PANORAMA) VIPE_CHECK_ARG(top == 0 && left == 0 && h1 == H && w1 == W);  // a crop breaks the sphere
  VIPE_CHECK_ARG(point_size >= 0.0f && point_size <= 3.0e38f);  // finite; false for a NaN
  VIPE_CHECK_ARG(max_radius >= 0 && max_radius <= MAX_RADIUS);
  const int64_t bx = (M + THREADS - 1) / THREADS;
  VIPE_CHECK_ARG(bx <= 0x7fffffff && B <= 65535);  // grid.x / grid.y: an error, not a silent truncation
  if (M == 0 || B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_xyz && d_cams && d_intrinsics && d_zbuf && d_stats);
  RenderArgs a;
  a.xyz = d_xyz; a.cams = d_cams; a.intr = d_intrinsics;
  a.zbuf = (u64*)d_zbuf; a.stats = (u64*)d_stats;
  a.M = M; a.index_base = index_base; a.idim = intr_dim;
  a.H = H; a.W = W; a.H0 = H0; a.W0 = W0; a.max_radius = max_radius;
  a.off_x = (float)left; a.off_y = (float)top;
  a.scale_x = (float)w1 / (float)W0;
  a.scale_y = (float)h1 / (float)H0;
  a.half_size = 0.5f * point_size;
  const dim3 grid((unsigned)bx, B);
  hipStream_t s = as_stream(stream);
  if (camera == VIPE_CAM_PINHOLE) cloud_render_kernel<VIPE_CAM_PINHOLE><<<grid, THREADS, 0, s>>>(a);
  else if (camera == VIPE_CAM_MEI) cloud_render_kernel<VIPE_CAM_MEI><<<grid, THREADS, 0, s>>>(a);
  else cloud_render_kernel<VIPE_CAM_PANORAMA><<<grid, THREADS, 0, s>>>(a);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_cloud_resolve(const int64_t* d_zbuf, int B, int H0, int W0, void* d_depth, int depth_dtype,
                                   const unsigned char* d_rgb_points, int64_t M_total, unsigned char* d_rgb_out,
                                   int* d_index, void* stream) {
  VIPE_CHECK_ARG(B >= 0 && H0 > 0 && W0 > 0 && M_total >= 0);
  VIPE_CHECK_ARG(depth_dtype == VIPE_F16 || depth_dtype == VIPE_F32);
  const int64_t total = (int64_t)B * H0 * W0;
  const int64_t bx = (total + THREADS - 1) / THREADS;
  VIPE_CHECK_ARG(bx <= 0x7fffffff);
  if (B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_zbuf && d_depth);
  VIPE_CHECK_ARG(!d_rgb_out || d_rgb_points || M_total == 0);
  ResolveArgs a;
  a.zbuf = (const u64*)d_zbuf; a.depth = d_depth; a.rgb = d_rgb_points; a.rgb_out = d_rgb_out; a.index = d_index;
  a.total = total; a.M_total = d_rgb_points ? M_total : 0;
  hipStream_t s = as_stream(stream);
  if (depth_dtype == VIPE_F32) cloud_resolve_kernel<float><<<(unsigned)bx, THREADS, 0, s>>>(a);
  else cloud_resolve_kernel<half_t><<<(unsigned)bx, THREADS, 0, s>>>(a);
  return vipe_launch_status();
}
