// Per-frame depth confidence: how many of K neighbour maps confirm each pixel of an exported depth map.
//
// For every pixel of the native-size grid of depth_export.hip (same tiles, same taps, same blended disparity d) the
// kernel back-projects the pixel's place in the SLAM-resolution grid, carries the point into each neighbour row q of the
// same `disps_up` buffer, and compares the disparity it would have there with the four taps around its projection:
//
//   (u, v)  = (tx.i0 + tx.l1, ty.i0 + ty.l1)           the clamped source coordinate of the export's taps: a pixel of
//                                                       the replicate-padded band repeats its edge pixel's test
//   ray     = cam::iproj<CAM>(I[view of r], u, v)
//   T       = (rig[vq]^-1 G[pq]) (rig[vr]^-1 G[pr])^-1  term_transforms of term_geom.cuh, as reproject.hip builds it
//   X1      = transform_ray<CAM>(T, ray, d);  valid = cam::valid_point<CAM>(X1);  (x', y') = cam::proj<CAM>(I[vq], X1)
//   d'      = d / X1.z (pinhole, MEI),  d / |X1| (panorama: inverse range)
//   visible = valid and 0 <= floor(y') <= H - 2 and (0 <= floor(x') <= W - 2 or, panorama, the columns wrap at the seam)
//   agree   = visible and one of the four taps t of disp[q] at (y0 | y0 + 1, x0 | x0 + 1) has t > 0, |d' - t| <= tol d'
//   out     = agree_count | visible_count << 4          (K <= 8: a nibble each)
//
// The test is relative in disparity, hence relative in depth and free of the clip's scale: no per-view mean, no host
// sync.  tests/depth_consistency_reference.py restates this in float64 and bounds the float32 error of every compared
// quantity from the operation counts below.
//
// Layout: one output pixel per thread, 64 x 4 tiles, the map index in blockIdx.z; a wave's store is 64 contiguous
// bytes.  The K relative transforms and the neighbour views' intrinsics are built once per workgroup in LDS by the first
// K lanes (depth_filter_kernel's scheme for its six) and read back as wave-uniform values; the row r and with it every
// skip of a neighbour are workgroup-uniform, so the only divergent exit is the pixel-bounds test behind the barrier.
// No atomics: a thread owns its byte.
#include "export_taps.cuh"
#include "term_geom.cuh"

namespace {

using namespace export_geom;

constexpr int MAX_K = 8, MAX_VIEWS = 8;

struct ConsistencyArgs {
  const float *disp, *poses, *rig, *intr;  // [R,H,W], [R/V,7], [V,7], [V,idim]
  const int64_t *rows, *nbr;               // [N] or null, [N,K]
  unsigned char* out;                      // [N,H0,W0]
  int K, R, V, idim, H, W, H0, W0, top, left;
  float scale_y, scale_x, tol;
};

struct Neighbour {
  Rigid T;
  cam::Intr I;
  int q;  // row of disp, -1: no test
};

// the two columns of the taps; pinhole / MEI end at the image border, the panorama's wrap at the seam
template <int CAM>
__device__ __forceinline__ bool columns(float xf, int W, int& c0, int& c1) {
  if constexpr (CAM == VIPE_CAM_PANORAMA) {  // x' lies in [-0.5, W - 0.5): xf in [-1, W - 1]
    const int x0 = (int)xf;
    c0 = ((x0 % W) + W) % W;
    c1 = (c0 + 1) % W;
    return true;
  } else {
    if (!(xf >= 0.0f && xf <= (float)(W - 2))) return false;  // also any x' that is not a number
    c0 = (int)xf;
    c1 = c0 + 1;
    return true;
  }
}

template <int CAM>
__global__ __launch_bounds__(TILE_W* TILE_H) void depth_consistency_kernel(ConsistencyArgs a) {
  __shared__ Neighbour nb[MAX_K];
  __shared__ cam::Intr Ii;
  const int64_t n = blockIdx.z;
  const int64_t r = a.rows ? a.rows[n] : n;
  const bool row_ok = r >= 0 && r < a.R;  // workgroup-uniform
  const int D = a.idim - 4;
  if (row_ok && threadIdx.x < a.K) {
    const int k = threadIdx.x;
    const int64_t q = a.nbr[n * a.K + k];
    Neighbour& B = nb[k];
    B.q = -1;
    if (q >= 0 && q < a.R && q != r) {
      const int pr = (int)(r / a.V), vr = (int)(r % a.V), pq = (int)(q / a.V), vq = (int)(q % a.V);
      Rigid G, Rr;
      term_transforms(a.poses, a.rig, pr, vr, pq, vq, B.T, G, Rr);
      B.I = cam::load<CAM>(a.intr + vq * a.idim, D, 1.0f, a.H, a.W);
      B.q = (int)q;
    }
    if (k == 0) Ii = cam::load<CAM>(a.intr + (int)(r % a.V) * a.idim, D, 1.0f, a.H, a.W);
  }
  __syncthreads();
  if (!row_ok) return;  // out[n] stays as it is
  const int x = blockIdx.x * TILE_W + (threadIdx.x & (TILE_W - 1));
  const int y = blockIdx.y * TILE_H + (threadIdx.x / TILE_W);
  if (x >= a.W0 || y >= a.H0) return;
  const Tap ty = make_tap(y, a.scale_y, a.top, a.H), tx = make_tap(x, a.scale_x, a.left, a.W);
  const int64_t P = (int64_t)a.H * a.W;
  const float* m = a.disp + r * P;
  const float* r0 = m + (int64_t)ty.i0 * a.W;
  const float* r1 = m + (int64_t)ty.i1 * a.W;
  const float d = blend(ty, tx, r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1]);
  unsigned agree = 0, visible = 0;
  if (d > 0.0f) {
    const float u = (float)tx.i0 + tx.l1, v = (float)ty.i0 + ty.l1;  // exact: the clamped source coordinate
    float X0, Y0, Z0 = 1.0f, dX[1], dY[1];
    cam::iproj<CAM, 0>(Ii, u, v, X0, Y0, Z0, dX, dY);
    for (int k = 0; k < a.K; ++k) {
      const Neighbour& B = nb[k];
      if (B.q < 0) continue;  // uniform
      float X, Y, Z, xp, yp, Jp[2][3], Jf[2][1];
      transform_ray<CAM>(B.T, X0, Y0, Z0, d, X, Y, Z);
      if (!cam::valid_point<CAM>(X, Y, Z)) continue;
      cam::proj<CAM, false, 0>(B.I, X, Y, Z, xp, yp, Jp, Jf);
      const float dq = CAM == VIPE_CAM_PANORAMA ? d / sqrtf(X * X + Y * Y + Z * Z) : d / Z;
      const float yf = floorf(yp);
      int c0, c1;
      if (!(yf >= 0.0f && yf <= (float)(a.H - 2)) || !columns<CAM>(floorf(xp), a.W, c0, c1)) continue;
      ++visible;
      const float* t0 = a.disp + B.q * P + (int64_t)(int)yf * a.W;
      const float* t1 = t0 + a.W;
      const float t[4] = {t0[c0], t0[c1], t1[c0], t1[c1]};
      const float lim = a.tol * dq;
      bool ok = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) ok = ok || (t[i] > 0.0f && fabsf(dq - t[i]) <= lim);
      agree += ok ? 1u : 0u;
    }
  }
  a.out[(n * a.H0 + y) * (int64_t)a.W0 + x] = (unsigned char)(agree | (visible << 4));
}

}  // namespace

VIPE_EXPORT int vipe_depth_consistency(const float* d_disp, const float* d_poses, const float* d_rig,
                                       const float* d_intrinsics, int intr_dim, int camera, const int64_t* d_rows,
                                       const int64_t* d_nbr, unsigned char* d_out, int N, int K, int R, int n_views, int H,
                                       int W, int h1, int w1, int top, int left, int H0, int W0, float tol, void* stream) {
  VIPE_CHECK_ARG(N >= 0 && R >= 0);
  VIPE_CHECK_ARG(geometry_ok(H, W, h1, w1, top, left, H0, W0));
  VIPE_CHECK_ARG(K >= 1 && K <= MAX_K);
  VIPE_CHECK_ARG(n_views >= 1 && n_views <= MAX_VIEWS && R % n_views == 0);
  VIPE_CHECK_ARG(camera == VIPE_CAM_PINHOLE || camera == VIPE_CAM_MEI || camera == VIPE_CAM_PANORAMA);
  VIPE_CHECK_ARG(intr_dim == (camera == VIPE_CAM_MEI ? 5 : 4));
  if (camera == VIPE_CAM_PANORAMA) VIPE_CHECK_ARG(top == 0 && left == 0 && h1 == H && w1 == W);  // a crop breaks the sphere
  VIPE_CHECK_ARG(tol > 0.0f);
  VIPE_CHECK_ARG(d_rows || N <= R);
  const int by = (H0 + TILE_H - 1) / TILE_H;
  VIPE_CHECK_ARG(by <= 65535 && N <= 65535);  // grid.y / grid.z: an error, not a silent truncation
  if (N == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_disp && d_poses && d_rig && d_intrinsics && d_nbr && d_out);
  ConsistencyArgs a;
  a.disp = d_disp; a.poses = d_poses; a.rig = d_rig; a.intr = d_intrinsics;
  a.rows = d_rows; a.nbr = d_nbr; a.out = d_out;
  a.K = K; a.R = R; a.V = n_views; a.idim = intr_dim;
  a.H = H; a.W = W; a.H0 = H0; a.W0 = W0; a.top = top; a.left = left;
  a.scale_y = (float)h1 / (float)H0;
  a.scale_x = (float)w1 / (float)W0;
  a.tol = tol;
  const dim3 grid((W0 + TILE_W - 1) / TILE_W, by, N);
  hipStream_t s = as_stream(stream);
  if (camera == VIPE_CAM_PINHOLE) depth_consistency_kernel<VIPE_CAM_PINHOLE><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  else if (camera == VIPE_CAM_MEI) depth_consistency_kernel<VIPE_CAM_MEI><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  else depth_consistency_kernel<VIPE_CAM_PANORAMA><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  return vipe_launch_status();
}
