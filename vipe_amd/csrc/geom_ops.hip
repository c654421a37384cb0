// slam_ext geometry kernels that the SLAM host code calls between update iterations:
//   frame_distance (edge proposal, LIVE: vipe/slam/maths/geom.py:343), depth_filter (map extraction, LIVE:
//   vipe/slam/components/buffer.py:625), projmap and iproj (bound but dormant).
// Replaces csrc/slam_ext/geom_kernels.cu:434-861.  Each walk over the pixels - the pair distance, the six-neighbour depth
// filter, the back-projection - is written once, for a camera FAMILY that supplies only what differs:
//   Pinhole (pinhole, and MEI through its pinhole-equivalent row): the reference's arithmetic - relative pose from raw
//     quaternions without re-normalisation (relSE3, :145-156), quaternion point action (actSO3, :106-116),
//     MIN_DEPTH = 0.25 (:33), float math except where the reference's double literals promote (the 75 % rule, :674;
//     depth_filter's 1.0 / d terms, :783-790).  Pinned bit for bit to the reference's kernels.
//   Sphere (the 360-degree panorama): the same operations with the camera of camera.cuh (ray, projection, validity,
//     seam) and the group operations of lie_math.h.  Disparity is inverse RANGE.
#include "common.cuh"
#include "lie_math.h"
#include "term_geom.cuh"

#pragma clang fp contract(off)

namespace {

constexpr float GEOM_MIN_DEPTH = 0.25f;

struct Rel {
  float t[3], q[4];
};

__device__ __forceinline__ void act_so3(const float* q, const float* X, float* Y) {
  float uv[3];
  uv[0] = 2.0f * (q[1] * X[2] - q[2] * X[1]);
  uv[1] = 2.0f * (q[2] * X[0] - q[0] * X[2]);
  uv[2] = 2.0f * (q[0] * X[1] - q[1] * X[0]);
  Y[0] = X[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
  Y[1] = X[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
  Y[2] = X[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}

__device__ __forceinline__ void act_se3(const Rel& T, const float* X, float* Y) {
  act_so3(T.q, X, Y);
  Y[3] = X[3];
  Y[0] += X[3] * T.t[0];
  Y[1] += X[3] * T.t[1];
  Y[2] += X[3] * T.t[2];
}

__device__ __forceinline__ Rel rel_se3(const float* pi, const float* pj) {
  const float *ti = pi, *qi = pi + 3, *tj = pj, *qj = pj + 3;
  Rel r;
  r.q[0] = -qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1];
  r.q[1] = -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2];
  r.q[2] = -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0];
  r.q[3] = qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2];
  float tmp[3];
  act_so3(r.q, ti, tmp);
  r.t[0] = tj[0] - tmp[0];
  r.t[1] = tj[1] - tmp[1];
  r.t[2] = tj[2] - tmp[2];
  return r;
}

// what thread 0 of a candidate's workgroup prepares for its lanes: both directions' transforms and the two views'
// intrinsics rows (zero where a view is the grid, which every lane knows)
template <class F>
struct RigPair {
  typename F::Xf Tij, Tji;
  float rows[2][4];
};

struct Pinhole {
  static constexpr bool ROWS = true;  // a view is an intrinsics row
  using Xf = Rel;
  struct View {
    float fx, fy, cx, cy;
  };
  struct Point {
    float X[4];  // (x, y, 1, d)
  };
  static __device__ __forceinline__ Xf relative(const float* pi, const float* pj) { return rel_se3(pi, pj); }
  static __device__ __forceinline__ Xf absolute(const float* p) {  // the pose as handed in: no normalisation
    Xf T;
    for (int q = 0; q < 3; ++q) T.t[q] = p[q];
    for (int q = 0; q < 4; ++q) T.q[q] = p[3 + q];
    return T;
  }
  // [fused] what thread 0 prepares for one candidate (keyframe pi, view qi) -> (pj, qj): the per-view poses R_q^-1 G_p
  // (geom.py:338: the reference expands them for ALL frames on the host side) and the pinhole rows at 1 / factor scale
  // (geom.py:335; MEI through its pinhole equivalent, cameras.py:338-343).  The group operations are lie_math.h's, applied
  // exactly as the lietorch calls of the unfused path apply them (every operand re-normalised when it is loaded), so
  // both paths give the same bits.
  static __device__ __forceinline__ RigPair<Pinhole> rig_pair(const float* poses, const float* rig, const float* intr_full,
                                                              int idim, float factor, int64_t pi, int64_t qi, int64_t pj,
                                                              int64_t qj) {
    RigPair<Pinhole> S;
    float e[2][7];
    const int64_t pp[2] = {pi, pj}, qq[2] = {qi, qj};
    for (int s = 0; s < 2; ++s) {
      float tmp[7];
      lie::SE3<float>(rig + 7 * qq[s]).inv().store(tmp);  // lietorch inv, stored ...
      (lie::SE3<float>(tmp) * lie::SE3<float>(poses + 7 * pp[s])).store(e[s]);  // ... and loaded again by the product
      const float* k = intr_full + (int64_t)idim * qq[s];
      for (int c = 0; c < 4; ++c) S.rows[s][c] = k[c] / factor;
      if (idim == 5) {  // MEI: f / (1 + k1)
        S.rows[s][0] = S.rows[s][0] / (1 + k[4]);
        S.rows[s][1] = S.rows[s][1] / (1 + k[4]);
      }
    }
    S.Tij = rel_se3(e[0], e[1]);
    S.Tji = rel_se3(e[1], e[0]);
    return S;
  }
  static __device__ __forceinline__ View view(const float* row, int, int) { return {row[0], row[1], row[2], row[3]}; }
  static __device__ __forceinline__ Point point(const View& I, float u, float v, float d) {
    return {{(u - I.cx) / I.fx, (v - I.cy) / I.fy, 1.0f, d}};
  }
  static __device__ __forceinline__ void act(const Xf& T, const Point& P, float (&X)[3]) {
    float Y[4];
    act_se3(T, P.X, Y);
    X[0] = Y[0], X[1] = Y[1], X[2] = Y[2];
  }
  // the translation added to the untransformed point: no identity rotation, whose operations would stay
  static __device__ __forceinline__ void act_translation(const Xf& T, const Point& P, float (&X)[3]) {
    for (int c = 0; c < 3; ++c) X[c] = P.X[c] + P.X[3] * T.t[c];
  }
  // -> target-side validity
  static __device__ __forceinline__ bool project(const View& J, const float (&X)[3], float& x, float& y) {
    x = J.fx * (X[0] / X[2]) + J.cx;
    y = J.fy * (X[1] / X[2]) + J.cy;
    return X[2] > GEOM_MIN_DEPTH;
  }
  static __device__ __forceinline__ float wrap(const View&, float dx) { return dx; }
  static __device__ __forceinline__ bool too_few(float vv, float tt) { return vv / (tt + 1e-8) < 0.75; }  // in double, :674
  // depth filter: the reference has no depth test before it projects
  static __device__ __forceinline__ bool usable(bool) { return true; }
  static __device__ __forceinline__ float disparity(const Point& P, const float (&X)[3]) { return P.X[3] / X[2]; }
  static __device__ __forceinline__ bool columns(int u0, int wd, int& c0, int& c1) {
    c0 = u0, c1 = u0 + 1;
    return u0 >= 0 && u0 < wd - 1;
  }
};

struct Sphere {
  static constexpr bool ROWS = false;  // a view is the grid
  static constexpr int CAM = VIPE_CAM_PANORAMA;
  using Xf = Rigid;
  using View = cam::Intr;
  struct Point {
    float b[3], d;  // unit ray, inverse range
  };
  static __device__ __forceinline__ Xf relative(const float* pi, const float* pj) {
    return to_rigid(lie::SE3<float>(pj) * lie::SE3<float>(pi).inv());
  }
  static __device__ __forceinline__ Xf absolute(const float* p) { return to_rigid(lie::SE3<float>(p)); }
  static __device__ __forceinline__ RigPair<Sphere> rig_pair(const float* poses, const float* rig, const float*, int, float,
                                                             int64_t pi, int64_t qi, int64_t pj, int64_t qj) {
    RigPair<Sphere> S = {};
    Rigid G, Rr;
    term_transforms(poses, rig, (int)pi, (int)qi, (int)pj, (int)qj, S.Tij, G, Rr);
    term_transforms(poses, rig, (int)pj, (int)qj, (int)pi, (int)qi, S.Tji, G, Rr);
    return S;
  }
  static __device__ __forceinline__ View view(const float*, int ht, int wd) { return cam::load<CAM>(nullptr, 0, 1.0f, ht, wd); }
  static __device__ __forceinline__ Point point(const View& I, float u, float v, float d) {
    Point P;
    float dX[1], dY[1];
    cam::iproj<CAM, 0>(I, u, v, P.b[0], P.b[1], P.b[2], dX, dY);
    P.d = d;
    return P;
  }
  static __device__ __forceinline__ void act(const Xf& T, const Point& P, float (&X)[3]) {
    transform_ray<CAM>(T, P.b[0], P.b[1], P.b[2], P.d, X[0], X[1], X[2]);
  }
  static __device__ __forceinline__ void act_translation(const Xf& T, const Point& P, float (&X)[3]) {
    Rigid Tt = T;
#pragma unroll
    for (int i = 0; i < 9; ++i) Tt.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    act(Tt, P, X);
  }
  static __device__ __forceinline__ bool project(const View& J, const float (&X)[3], float& x, float& y) {
    float Jp[2][3], Jf[2][1];
    cam::proj<CAM, false, 0>(J, X[0], X[1], X[2], x, y, Jp, Jf);
    return cam::valid_point<CAM>(X[0], X[1], X[2]);
  }
  static __device__ __forceinline__ float wrap(const View& J, float dx) { return cam::wrap_dx<CAM>(dx, J.cx); }  // the seam
  static __device__ __forceinline__ bool too_few(float vv, float tt) { return vv / (tt + 1e-8f) < 0.75f; }
  static __device__ __forceinline__ bool usable(bool valid) { return valid; }
  static __device__ __forceinline__ float disparity(const Point& P, const float (&X)[3]) {
    return P.d / sqrtf(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);  // inverse range in the neighbour
  }
  static __device__ __forceinline__ bool columns(int u0, int wd, int& c0, int& c1) {  // the columns wrap at the seam
    c0 = (u0 + wd) % wd, c1 = (u0 + 1 + wd) % wd;
    return true;
  }
};

// length of the flow of pixel (u, v) to the point X of view J, in pixels; ok: the target-side validity
template <class F>
__device__ __forceinline__ float flow_length(const typename F::View& J, const float (&X)[3], float u, float v, bool& ok) {
  float x, y;
  ok = F::project(J, X, x, y);
  const float du = F::wrap(J, x - u), dv = y - v;
  return sqrtf(du * du + dv * dv);
}

// the distance of one ordered pair (buffer.py:550-593 -> geom_kernels.cu:560-676): beta-weighted mean of the full and
// the translation-only flow over the valid pixels, 1000 when fewer than 75 % are valid.  Lanes stride over the pixels,
// wave-shuffle + LDS reduction; the result is valid in thread 0.
template <class F>
__device__ __forceinline__ float pair_distance(const typename F::Xf& T, const typename F::View& Vi, const typename F::View& Vj,
                                               const float* __restrict__ d, int ht, int wd, float beta, float (*red)[4]) {
  float accum = 0.f, valid = 0.f, total = 0.f;
  for (int k = threadIdx.x; k < ht * wd; k += blockDim.x) {
    const float u = (float)(k % wd), v = (float)(k / wd);
    const typename F::Point P = F::point(Vi, u, v, d[k]);
    float X[3];
    bool ok;
    F::act(T, P, X);
    float dd = flow_length<F>(Vj, X, u, v, ok);
    total += beta;
    if (ok) {
      accum += beta * dd;
      valid += beta;
    }
    F::act_translation(T, P, X);
    dd = flow_length<F>(Vj, X, u, v, ok);
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
  return F::too_few(vv, tt) ? 1000.0f : a / vv;
}

// one workgroup per candidate pair; the reference's unfused operator, pinhole only
__global__ __launch_bounds__(256) void frame_distance_kernel(const float* __restrict__ poses,
                                                             const float* __restrict__ disps,
                                                             const float* __restrict__ intr,
                                                             const int64_t* __restrict__ pi,
                                                             const int64_t* __restrict__ pj,
                                                             const int64_t* __restrict__ ri,
                                                             const int64_t* __restrict__ rj,
                                                             const int64_t* __restrict__ di, float* __restrict__ dist,
                                                             int ht, int wd, float beta) {
  const int b = blockIdx.x;
  __shared__ Rel T;
  __shared__ float red[3][4];
  if (threadIdx.x == 0) T = rel_se3(poses + 7 * pi[b], poses + 7 * pj[b]);
  __syncthreads();
  const float r = pair_distance<Pinhole>(T, Pinhole::view(intr + 4 * ri[b], ht, wd), Pinhole::view(intr + 4 * rj[b], ht, wd),
                                         disps + (int64_t)di[b] * ht * wd, ht, wd, beta, red);
  if (threadIdx.x == 0) dist[b] = r;
}

// [fused] GraphBuffer.frame_distance_dense_disp (buffer.py:550-593), one workgroup per candidate (keyframe pi, view qi) ->
// (pj, qj): the distance and - `bidir` - the reverse one, averaged
template <class F>
__global__ __launch_bounds__(256) void frame_distance_rig_kernel(const float* __restrict__ poses, const float* __restrict__ rig,
                                                                 const float* __restrict__ disps,
                                                                 const float* __restrict__ intr_full, int idim, float factor,
                                                                 const int64_t* __restrict__ pi, const int64_t* __restrict__ qi,
                                                                 const int64_t* __restrict__ pj, const int64_t* __restrict__ qj,
                                                                 float* __restrict__ dist, int V, int ht, int wd, float beta,
                                                                 int bidir) {
  const int b = blockIdx.x;
  __shared__ RigPair<F> S;
  __shared__ float red[3][4];
  if (threadIdx.x == 0) S = F::rig_pair(poses, rig, intr_full, idim, factor, pi[b], qi[b], pj[b], qj[b]);
  __syncthreads();
  const int64_t P = (int64_t)ht * wd;
  float r = pair_distance<F>(S.Tij, F::view(S.rows[0], ht, wd), F::view(S.rows[1], ht, wd), disps + (pi[b] * V + qi[b]) * P, ht,
                             wd, beta, red);
  if (bidir) {
    const float r2 = pair_distance<F>(S.Tji, F::view(S.rows[1], ht, wd), F::view(S.rows[0], ht, wd),
                                      disps + (pj[b] * V + qj[b]) * P, ht, wd, beta, red);
    r = 0.5f * (r + r2);
  }
  if (threadIdx.x == 0) dist[b] = r;
}

// one lane per (keyframe slot, pixel): walks the 6 temporal neighbours itself, so the count needs no atomics
template <class F>
__global__ __launch_bounds__(256) void depth_filter_kernel(const float* __restrict__ poses,
                                                           const float* __restrict__ disps,
                                                           const float* __restrict__ intr,
                                                           const int64_t* __restrict__ inds,
                                                           const float* __restrict__ thresh, float* __restrict__ counter,
                                                           int num, int ht, int wd) {
  const int b = blockIdx.y;
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  const int ix = (int)inds[b];
  const float t = thresh[b];
  __shared__ typename F::Xf T[6];
  __shared__ int jxs[6];
  if (threadIdx.x < 6) {
    const int nb = threadIdx.x;
    const int jx = (nb < 3) ? ix - nb - 1 : ix + nb - 2;  // geom_kernels.cu:709
    jxs[nb] = jx;
    if (jx >= 0 && jx < num) T[nb] = F::relative(poses + 7 * ix, poses + 7 * jx);
  }
  __syncthreads();
  if (index >= ht * wd) return;
  const typename F::View I = F::view(intr, ht, wd);
  const typename F::Point P = F::point(I, (float)(index % wd), (float)(index / wd), disps[(int64_t)ix * ht * wd + index]);
  float cnt = 0.0f;
  for (int nb = 0; nb < 6; ++nb) {
    const int jx = jxs[nb];
    if (jx < 0 || jx >= num) continue;
    float X[3], x, y;
    F::act(T[nb], P, X);
    if (!F::usable(F::project(I, X, x, y))) continue;
    const float dj = F::disparity(P, X);
    const int u0 = (int)floorf(x), v0 = (int)floorf(y);
    int c0, c1;
    if (F::columns(u0, wd, c0, c1) && v0 >= 0 && v0 < ht - 1) {  // the rows end at the image border / the poles
      const float* dn = disps + (int64_t)jx * ht * wd;
      const float d00 = dn[v0 * wd + c0], d01 = dn[v0 * wd + c1];
      const float d10 = dn[(v0 + 1) * wd + c0], d11 = dn[(v0 + 1) * wd + c1];
      const double inv = 1.0 / (double)dj, tt = (double)t;  // the reference's `1.0 / dj` is a double expression
      if (fabs(inv - 1.0 / (double)d00) < tt) cnt += 1.0f;
      else if (fabs(inv - 1.0 / (double)d01) < tt) cnt += 1.0f;
      else if (fabs(inv - 1.0 / (double)d10) < tt) cnt += 1.0f;
      else if (fabs(inv - 1.0 / (double)d11) < tt) cnt += 1.0f;
    }
  }
  counter[(int64_t)b * ht * wd + index] = cnt;
}

__global__ __launch_bounds__(256) void projmap_kernel(const float* __restrict__ poses, const float* __restrict__ disps,
                                                      const float* __restrict__ intr, const int64_t* __restrict__ ii,
                                                      const int64_t* __restrict__ jj, float* __restrict__ coords,
                                                      float* __restrict__ valid, int ht, int wd) {
  const int b = blockIdx.y;
  __shared__ Rel T;
  if (threadIdx.x == 0) T = rel_se3(poses + 7 * ii[b], poses + 7 * jj[b]);
  __syncthreads();
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ht * wd) return;
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const float u = (float)(k % wd), v = (float)(k / wd);
  float Xi[4] = {(u - cx) / fx, (v - cy) / fy, 1.0f, disps[(int64_t)ii[b] * ht * wd + k]}, Xj[4];
  act_se3(T, Xi, Xj);
  float* c = coords + ((int64_t)b * ht * wd + k) * 3;
  c[0] = u;
  c[1] = v;
  if (Xj[2] > 0.01f) {
    c[0] = fx * (Xj[0] / Xj[2]) + cx;
    c[1] = fy * (Xj[1] / Xj[2]) + cy;
  }
  valid[(int64_t)b * ht * wd + k] = (Xj[2] > GEOM_MIN_DEPTH) ? 1.0f : 0.0f;
}

// world points act(pose, point) / d, with the pose applied as the family takes an absolute pose
template <class F>
__global__ __launch_bounds__(256) void iproj_kernel(const float* __restrict__ poses, const float* __restrict__ disps,
                                                    const float* __restrict__ intr, float* __restrict__ points, int ht,
                                                    int wd) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ typename F::Xf T;
  if (threadIdx.x == 0) T = F::absolute(poses + 7 * b);
  __syncthreads();
  if (k >= ht * wd) return;
  const float d = disps[(int64_t)b * ht * wd + k];
  float X[3];
  F::act(T, F::point(F::view(intr, ht, wd), (float)(k % wd), (float)(k / wd), d), X);
  float* p = points + ((int64_t)b * ht * wd + k) * 3;
  p[0] = X[0] / d;
  p[1] = X[1] / d;
  p[2] = X[2] / d;
}

// the launches of a family's three operations, behind the argument checks both families' entry points share
template <class F>
int launch_frame_distance_rig(const float* d_poses, const float* d_rig, const float* d_disps, const float* d_intrinsics,
                              int intr_dim, float intr_factor, const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj,
                              const int64_t* d_qj, float* d_dist, int M, int n_views, int ht, int wd, float beta,
                              int bidirectional, void* stream) {
  VIPE_CHECK_ARG(M >= 0 && ht > 0 && wd > 0 && n_views > 0);
  if (M == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_rig && d_disps && (d_intrinsics || !F::ROWS) && d_pi && d_pj && d_qi && d_qj && d_dist);
  frame_distance_rig_kernel<F><<<M, 256, 0, as_stream(stream)>>>(d_poses, d_rig, d_disps, d_intrinsics, intr_dim, intr_factor,
                                                                 d_pi, d_qi, d_pj, d_qj, d_dist, n_views, ht, wd, beta,
                                                                 bidirectional);
  return vipe_launch_status();
}

template <class F>
int launch_depth_filter(const float* d_poses, const float* d_disps, const float* d_intrinsics, const int64_t* d_inds,
                        const float* d_thresh, float* d_counter, int n, int num, int ht, int wd, void* stream) {
  VIPE_CHECK_ARG(n >= 0 && num >= 0 && ht > 0 && wd > 0 && num <= 65535);
  if (num == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_disps && (d_intrinsics || !F::ROWS) && d_inds && d_thresh && d_counter);
  depth_filter_kernel<F><<<dim3((ht * wd + 255) / 256, num), 256, 0, as_stream(stream)>>>(
      d_poses, d_disps, d_intrinsics, d_inds, d_thresh, d_counter, n, ht, wd);
  return vipe_launch_status();
}

template <class F>
int launch_iproj(const float* d_poses, const float* d_disps, const float* d_intrinsics, float* d_points, int n, int ht, int wd,
                 void* stream) {
  VIPE_CHECK_ARG(n >= 0 && ht > 0 && wd > 0 && n <= 65535);
  if (n == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_disps && (d_intrinsics || !F::ROWS) && d_points);
  iproj_kernel<F><<<dim3((ht * wd + 255) / 256, n), 256, 0, as_stream(stream)>>>(d_poses, d_disps, d_intrinsics, d_points, ht,
                                                                               wd);
  return vipe_launch_status();
}

}  // namespace

VIPE_EXPORT int vipe_frame_distance(const float* d_poses, const float* d_disps, const float* d_intrinsics,
                                    const int64_t* d_pi, const int64_t* d_pj, const int64_t* d_qi, const int64_t* d_qj,
                                    const int64_t* d_di, float* d_dist, int M, int ht, int wd, float beta, void* stream) {
  VIPE_CHECK_ARG(M >= 0 && ht > 0 && wd > 0);
  if (M == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_disps && d_intrinsics && d_pi && d_pj && d_qi && d_qj && d_di && d_dist);
  frame_distance_kernel<<<M, 256, 0, as_stream(stream)>>>(d_poses, d_disps, d_intrinsics, d_pi, d_pj, d_qi, d_qj, d_di,
                                                          d_dist, ht, wd, beta);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_frame_distance_rig(const float* d_poses, const float* d_rig, const float* d_disps, const float* d_intrinsics,
                                        int intr_dim, float intr_factor, const int64_t* d_pi, const int64_t* d_qi,
                                        const int64_t* d_pj, const int64_t* d_qj, float* d_dist, int M, int n_views, int ht,
                                        int wd, float beta, int bidirectional, void* stream) {
  VIPE_CHECK_ARG((intr_dim == 4 || intr_dim == 5) && intr_factor > 0);
  return launch_frame_distance_rig<Pinhole>(d_poses, d_rig, d_disps, d_intrinsics, intr_dim, intr_factor, d_pi, d_qi, d_pj, d_qj,
                                            d_dist, M, n_views, ht, wd, beta, bidirectional, stream);
}

VIPE_EXPORT int vipe_frame_distance_sphere(const float* d_poses, const float* d_rig, const float* d_disps, const int64_t* d_pi,
                                           const int64_t* d_qi, const int64_t* d_pj, const int64_t* d_qj, float* d_dist, int M,
                                           int n_views, int ht, int wd, float beta, int bidirectional, void* stream) {
  return launch_frame_distance_rig<Sphere>(d_poses, d_rig, d_disps, nullptr, 0, 0.0f, d_pi, d_qi, d_pj, d_qj, d_dist, M, n_views,
                                           ht, wd, beta, bidirectional, stream);
}

VIPE_EXPORT int vipe_depth_filter(const float* d_poses, const float* d_disps, const float* d_intrinsics,
                                  const int64_t* d_inds, const float* d_thresh, float* d_counter, int n, int num,
                                  int ht, int wd, void* stream) {
  return launch_depth_filter<Pinhole>(d_poses, d_disps, d_intrinsics, d_inds, d_thresh, d_counter, n, num, ht, wd, stream);
}

VIPE_EXPORT int vipe_depth_filter_sphere(const float* d_poses, const float* d_disps, const int64_t* d_inds, const float* d_thresh,
                                         float* d_counter, int n, int num, int ht, int wd, void* stream) {
  return launch_depth_filter<Sphere>(d_poses, d_disps, nullptr, d_inds, d_thresh, d_counter, n, num, ht, wd, stream);
}

VIPE_EXPORT int vipe_projmap(const float* d_poses, const float* d_disps, const float* d_intrinsics,
                             const int64_t* d_ii, const int64_t* d_jj, float* d_coords, float* d_valid, int E, int ht,
                             int wd, void* stream) {
  VIPE_CHECK_ARG(E >= 0 && ht > 0 && wd > 0 && E <= 65535);
  if (E == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_poses && d_disps && d_intrinsics && d_ii && d_jj && d_coords && d_valid);
  projmap_kernel<<<dim3((ht * wd + 255) / 256, E), 256, 0, as_stream(stream)>>>(d_poses, d_disps, d_intrinsics, d_ii,
                                                                                d_jj, d_coords, d_valid, ht, wd);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_iproj(const float* d_poses, const float* d_disps, const float* d_intrinsics, float* d_points,
                           int n, int ht, int wd, void* stream) {
  return launch_iproj<Pinhole>(d_poses, d_disps, d_intrinsics, d_points, n, ht, wd, stream);
}

VIPE_EXPORT int vipe_iproj_sphere(const float* d_poses, const float* d_disps, float* d_points, int n, int ht, int wd,
                                  void* stream) {
  return launch_iproj<Sphere>(d_poses, d_disps, nullptr, d_points, n, ht, wd, stream);
}
