// The geometry kernels the SLAM host code calls between update iterations, for the 360-degree panorama camera:
// frame distance (edge proposal), depth filter (map extraction) and back-projection to world points.  The pinhole
// kernels of geom_ops.hip are pinned bit for bit to the reference's and stay as they are; these restate the same three
// operations (vipe/slam/components/buffer.py:550-593, geom_kernels.cu:678-793, :795-861) on the sphere, with the camera
// of camera.cuh (ray, projection, validity, seam) and the group operations of lie_math.h.  Disparity is inverse RANGE.
#include "term_geom.cuh"

namespace {

constexpr int CAM = VIPE_CAM_PANORAMA;

// pixel p of the grid -> unit ray
__device__ __forceinline__ void pixel_ray(const cam::Intr& I, int p, int wd, float& u, float& v, float (&b)[3]) {
  u = (float)(p % wd);
  v = (float)(p / wd);
  float dX[1], dY[1];
  cam::iproj<CAM, 0>(I, u, v, b[0], b[1], b[2], dX, dY);
}

// length of the flow of (b, d) under T, in pixels of the grid, with the seam wrapped; ok: the target-side validity
__device__ __forceinline__ float flow_length(const cam::Intr& I, const Rigid& T, const float (&b)[3], float d, float u, float v,
                                             bool& ok) {
  float X, Y, Z, x, y, Jp[2][3], Jf[2][1];
  transform_ray<CAM>(T, b[0], b[1], b[2], d, X, Y, Z);
  cam::proj<CAM, false, 0>(I, X, Y, Z, x, y, Jp, Jf);
  ok = cam::valid_point<CAM>(X, Y, Z);
  const float du = cam::wrap_dx<CAM>(x - u, I.cx), dv = y - v;
  return sqrtf(du * du + dv * dv);
}

// the distance of one ordered pair (buffer.py:550-593 -> geom_kernels.cu:560-676): beta-weighted mean of the full and
// the translation-only flow over the valid pixels, 1000 when fewer than 75 % are valid.  Lanes stride over the pixels;
// the result is valid in thread 0.
__device__ __forceinline__ float pair_distance(const cam::Intr& I, const Rigid& T, const float* __restrict__ d, int P, int wd,
                                               float beta, float (*red)[4]) {
  Rigid Tt = T;  // translation only
#pragma unroll
  for (int i = 0; i < 9; ++i) Tt.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
  float accum = 0.f, valid = 0.f, total = 0.f;
  for (int k = threadIdx.x; k < P; k += blockDim.x) {
    float u, v, b[3];
    pixel_ray(I, k, wd, u, v, b);
    bool ok;
    float dd = flow_length(I, T, b, d[k], u, v, ok);
    total += beta;
    if (ok) {
      accum += beta * dd;
      valid += beta;
    }
    dd = flow_length(I, Tt, b, d[k], u, v, ok);
    total += (1 - beta);
    if (ok) {
      accum += (1 - beta) * dd;
      valid += (1 - beta);
    }
  }
  accum = wave_sum(accum);
  valid = wave_sum(valid);
  total = wave_sum(total);
  __syncthreads();  // red may still be read by thread 0 of an earlier call
  if (lane_id() == 0) {
    red[0][wave_id()] = accum;
    red[1][wave_id()] = valid;
    red[2][wave_id()] = total;
  }
  __syncthreads();
  const float a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const float vv = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  const float tt = red[2][0] + red[2][1] + red[2][2] + red[2][3];
  return (vv / (tt + 1e-8f) < 0.75f) ? 1000.0f : a / vv;
}

// one workgroup per candidate (keyframe pi, view qi) -> (pj, qj)
__global__ __launch_bounds__(256) void frame_distance_sphere_kernel(const float* __restrict__ poses, const float* __restrict__ rig,
                                                                    const float* __restrict__ disps,
                                                                    const int64_t* __restrict__ pi, const int64_t* __restrict__ qi,
                                                                    const int64_t* __restrict__ pj, const int64_t* __restrict__ qj,
                                                                    float* __restrict__ dist, int V, int ht, int wd, float beta,
                                                                    int bidir) {
  const int b = blockIdx.x;
  __shared__ Rigid Tij, Tji;
  __shared__ float red[3][4];
  if (threadIdx.x == 0) {
    Rigid G, Rr;
    term_transforms(poses, rig, (int)pi[b], (int)qi[b], (int)pj[b], (int)qj[b], Tij, G, Rr);
    term_transforms(poses, rig, (int)pj[b], (int)qj[b], (int)pi[b], (int)qi[b], Tji, G, Rr);
  }
  __syncthreads();
  const cam::Intr I = cam::load<CAM>(nullptr, 0, 1.0f, ht, wd);
  const int P = ht * wd;
  float r = pair_distance(I, Tij, disps + (pi[b] * V + qi[b]) * (int64_t)P, P, wd, beta, red);
  if (bidir) {
    const float r2 = pair_distance(I, Tji, disps + (pj[b] * V + qj[b]) * (int64_t)P, P, wd, beta, red);
    r = 0.5f * (r + r2);
  }
  if (threadIdx.x == 0) dist[b] = r;
}

// one lane per (keyframe slot, pixel): walks the 6 temporal neighbours itself, so the count needs no atomics
__global__ __launch_bounds__(256) void depth_filter_sphere_kernel(const float* __restrict__ poses, const float* __restrict__ disps,
                                                                  const int64_t* __restrict__ inds,
                                                                  const float* __restrict__ thresh, float* __restrict__ counter,
                                                                  int n, int ht, int wd) {
  const int b = blockIdx.y;
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  const int ix = (int)inds[b];
  const float t = thresh[b];
  __shared__ Rigid T[6];
  __shared__ int jxs[6];
  if (threadIdx.x < 6) {
    const int nb = threadIdx.x;
    const int jx = (nb < 3) ? ix - nb - 1 : ix + nb - 2;  // geom_kernels.cu:709
    jxs[nb] = jx;
    if (jx >= 0 && jx < n) T[nb] = to_rigid(lie::SE3<float>(poses + 7 * jx) * lie::SE3<float>(poses + 7 * ix).inv());
  }
  __syncthreads();
  if (index >= ht * wd) return;
  const cam::Intr I = cam::load<CAM>(nullptr, 0, 1.0f, ht, wd);
  float u, v, ray[3];
  pixel_ray(I, index, wd, u, v, ray);
  const float di = disps[(int64_t)ix * ht * wd + index];
  float cnt = 0.0f;
  for (int nb = 0; nb < 6; ++nb) {
    const int jx = jxs[nb];
    if (jx < 0 || jx >= n) continue;
    float X, Y, Z, x, y, Jp[2][3], Jf[2][1];
    transform_ray<CAM>(T[nb], ray[0], ray[1], ray[2], di, X, Y, Z);
    if (!cam::valid_point<CAM>(X, Y, Z)) continue;
    cam::proj<CAM, false, 0>(I, X, Y, Z, x, y, Jp, Jf);
    const float dj = di / sqrtf(X * X + Y * Y + Z * Z);  // inverse range in the neighbour
    const int u0 = (int)floorf(x), v0 = (int)floorf(y);
    if (v0 >= 0 && v0 < ht - 1) {  // the columns wrap at the seam, the rows end at the poles
      const int c0 = (u0 + wd) % wd, c1 = (u0 + 1 + wd) % wd;
      const float* dn = disps + (int64_t)jx * ht * wd;
      const float d00 = dn[v0 * wd + c0], d01 = dn[v0 * wd + c1];
      const float d10 = dn[(v0 + 1) * wd + c0], d11 = dn[(v0 + 1) * wd + c1];
      const double inv = 1.0 / (double)dj, tt = (double)t;  // as the pinhole kernel: double expressions
      if (fabs(inv - 1.0 / (double)d00) < tt) cnt += 1.0f;
      else if (fabs(inv - 1.0 / (double)d01) < tt) cnt += 1.0f;
      else if (fabs(inv - 1.0 / (double)d10) < tt) cnt += 1.0f;
      else if (fabs(inv - 1.0 / (double)d11) < tt) cnt += 1.0f;
    }
  }
  counter[(int64_t)b * ht * wd + index] = cnt;
}

// world points act(pose, (b, d)) / d, with the pose applied as handed in (iproj_kernel does the same)
__global__ __launch_bounds__(256) void iproj_sphere_kernel(const float* __restrict__ poses, const float* __restrict__ disps,
                                                           float* __restrict__ points, int ht, int wd) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ Rigid T;
  if (threadIdx.x == 0) T = to_rigid(lie::SE3<float>(poses + 7 * b));
  __syncthreads();
  if (k >= ht * wd) return;
  const cam::Intr I = cam::load<CAM>(nullptr, 0, 1.0f, ht, wd);
  float u, v, ray[3], X, Y, Z;
  pixel_ray(I, k, wd, u, v, ray);
  const float d = disps[(int64_t)b * ht * wd + k];
  transform_ray<CAM>(T, ray[0], ray[1], ray[2], d, X, Y, Z);
  float* p = points + ((int64_t)b * ht * wd + k) * 3;
  p[0] = X / d;
  p[1] = Y / d;
  p[2] = Z / d;
}

}  // namespace

VIPE_EXPORT int vipe_frame_distance_sphere(const float* d_poses, const float* d_rig, const float* d_disps, const int64_t* d_pi,
                                           const int64_t* d_qi, const int64_t* d_pj, const int64_t* d_qj, float* d_dist, int M,
                                           int n_views, int ht, int wd, float beta, int bidirectional, void* stream) {
  VIPE_CHECK_ARG(M >= 0 && ht > 0 && wd > 0 && n_views > 0);
  if (M == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_rig && d_disps && d_pi && d_pj && d_qi && d_qj && d_dist);
  frame_distance_sphere_kernel<<<M, 256, 0, as_stream(stream)>>>(d_poses, d_rig, d_disps, d_pi, d_qi, d_pj, d_qj, d_dist, n_views,
                                                                 ht, wd, beta, bidirectional);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_depth_filter_sphere(const float* d_poses, const float* d_disps, const int64_t* d_inds, const float* d_thresh,
                                         float* d_counter, int n, int num, int ht, int wd, void* stream) {
  VIPE_CHECK_ARG(n >= 0 && num >= 0 && ht > 0 && wd > 0 && num <= 65535);
  if (num == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_disps && d_inds && d_thresh && d_counter);
  depth_filter_sphere_kernel<<<dim3((ht * wd + 255) / 256, num), 256, 0, as_stream(stream)>>>(d_poses, d_disps, d_inds, d_thresh,
                                                                                              d_counter, n, ht, wd);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_iproj_sphere(const float* d_poses, const float* d_disps, float* d_points, int n, int ht, int wd,
                                  void* stream) {
  VIPE_CHECK_ARG(n >= 0 && ht > 0 && wd > 0 && n <= 65535);
  if (n == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_disps && d_points);
  iproj_sphere_kernel<<<dim3((ht * wd + 255) / 256, n), 256, 0, as_stream(stream)>>>(d_poses, d_disps, d_points, ht, wd);
  return vipe_launch_status();
}
