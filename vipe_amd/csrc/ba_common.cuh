// Bundle adjustment: constants, workspace layout and the device helpers every stage shares.
// Included by ba.hip inside its anonymous namespace (one translation unit); not a stand-alone header.

constexpr int TILE = 256;   // lanes per workgroup = pixels per tile
constexpr int NWAVE = TILE / WAVE;
constexpr int TCHUNK = 8;   // terms whose transforms are staged in LDS at a time
constexpr int AM_DMAX = 6;  // largest source-frame degree the matrix-core accumulate kernel handles

// Slots of BAWs::info, copied to the caller's d_info (include/vipe_amd.h; ext/slam_ext.py reads two of them by number)
enum InfoSlot {
  INFO_FREE_POSES = 0,   // plan: free poses = 6x6 blocks of the reduced system
  INFO_FREE_DISP = 1,    // plan: free disparity frames
  INFO_FAILURES = 2,     // failed factorisations of this call (their step is zero)
  INFO_UNKNOWNS = 3,     // plan: n = 6 free poses + tail unknowns
  INFO_BAND_BLOCKS = 4,  // plan: band width of the pose part in 6x6 blocks
  INFO_SOLVER = 5,       // a Solver: who solved the last iteration.  A report for the caller; no kernel reads it
  INFO_MAX_DEGREE = 6,   // plan: largest number of terms of one source frame
  INFO_TILED_FAIL = 7,   // tiled factorisation: a pivot of the current one failed (chol_potrf -> chol_backsub)
};
// Values of INFO_SOLVER; part of the ABI (vipe_ba_params.path_hint is learnt from them)
enum Solver { SOLVER_GLOBAL = 0, SOLVER_BAND = 1, SOLVER_DENSE = 2 };

struct BAWs {
  int* rowptr;      // [nF+1] CSR over source disparity frames
  int* order;       // [M] term ids sorted by source frame (stable)
  int* pose_slot;   // [nP] slot in the reduced system or -1
  int* slot_pose;   // [nP] inverse map
  int* fflags;      // [nF] bit0 source, bit1 disparity free (the sensor-prior test is NOT part of the plan: finish_disp reads sens_sum, refreshed every call)
  int* scratch;     // [2*nP + nF]
  int* info;        // [8] by InfoSlot
  float* sens_sum;  // [nF]
  float* C;         // [nF,P] damped disparity diagonal
  float* wv;        // [nF,P]
  float* Ekk;       // [nF,6,P]
  float* Ef;        // [nF,2,P]
  float* Et;        // [nF,ntail,P] multi-view rigs: rows of the tail unknowns (per-view intrinsics, rig rotations)
  float* Ej;        // [M,6,P]
  double* S;        // [(nmax+1),(nmax+1)] lower triangle + rhs row
  double* Hd;       // [nmax] undamped diagonal of H (for lambda * diag)
  float* dx;        // [nmax]
  double* Wi;       // [ceil(nmax / 64)][64][64] inverses of the diagonal factor tiles (tiled Cholesky)
  int* krow;        // [nF] DROID mode: row of frame k in the sorted unique set arange(t0,t1) U ii (eta / dz row)
  int* mslot;       // [M] marginals: slot of the target pose of the term at each CSR position, or -1 (ba_term_slot_kernel)
  int ld;           // nmax + 1
};

struct BAArgs {
  vipe_ba_params p;
  float *poses, *disps, *intr, *rig;
  const float *sens, *target, *weight, *eta;
  const int64_t *pi, *qi, *pj, *qj, *di;
  BAWs w;
  int P, nF, D;
  // multi-view rigs (n_views > 1): the tail of the reduced system holds one intrinsics block
  // per view (nintr = V (1 + D) unknowns when optimize_intrinsics) and one rotation block per view >= 1 (6 (V - 1) when
  // optimize_rig_rotation; view 0 is the gauge, buffer.py:506); ntail = both.  Mono: the F <= 2 shared intrinsics.
  int mv, nintr, ntail;
  int force_general; // vipe_ba_params.solver_options & VIPE_BA_OPT_GENERAL_ACCUMULATE
  int band2;         // two-chain band solve for long pose-only chains (off: VIPE_BA_OPT_ONE_CHAIN)
  // DROID semantics of slam_ext.ba (geom_kernels.cu:178-432, 1273-1404; see oracle/droid_ba.py for the list):
  // target / weight [M,2,P], eta [K,P] by krow, per-pixel depth prior, reduced-diagonal damping, poses free iff in
  // [t0,t1), stereo terms, MIN_DEPTH 0.25, pose t0 left out of the disparity back-substitution, dz written to dz_out
  int droid;
  float* dz_out;
};

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

constexpr int RG_VMAX = 8;  // views of a rig the multi-view kernels handle: the per-view tail rows of a pixel live in registers
                            // (instantiations for <= 4 and <= 8 views; the reference's Solver is generic in V, buffer.py:404-506)
inline bool is_multiview(const vipe_ba_params& p) { return p.n_views > 1; }  // a mono rig has no rig unknowns (view 0 is the gauge)
inline int tail_intr(const vipe_ba_params& p) {
  const int F = 1 + (p.camera == VIPE_CAM_MEI ? 1 : 0);
  return p.optimize_intrinsics ? (is_multiview(p) ? p.n_views * F : F) : 0;
}
inline int tail_rig(const vipe_ba_params& p) { return p.optimize_rig_rotation ? 6 * (p.n_views - 1) : 0; }

size_t carve(const vipe_ba_params& p, char* base, BAWs* out) {
  const size_t nP = p.n_poses, nF = (size_t)p.n_poses * p.n_views, P = (size_t)p.ht * p.wd, M = p.M;
  const size_t ntail_max = is_multiview(p) ? (size_t)p.n_views * 2 + 6 * (size_t)(p.n_views - 1) : 2;
  const size_t nmax = 6 * nP + ntail_max;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* ptr = base ? base + off : nullptr;
    off += align_up(bytes);
    return ptr;
  };
  BAWs w;
  w.rowptr = (int*)take(4 * (nF + 1));
  w.order = (int*)take(4 * (M + 1));
  w.pose_slot = (int*)take(4 * nP);
  w.slot_pose = (int*)take(4 * nP);
  w.fflags = (int*)take(4 * nF);
  w.scratch = (int*)take(4 * (2 * nP + nF));
  w.info = (int*)take(4 * 8);
  w.sens_sum = (float*)take(4 * nF);
  w.C = (float*)take(4 * nF * P);
  w.wv = (float*)take(4 * nF * P);
  w.Ekk = (float*)take(4 * nF * 6 * P);
  w.Ef = (float*)take(4 * nF * 2 * P);
  w.Et = (float*)take(is_multiview(p) ? 4 * nF * ntail_max * P : 0);
  w.Ej = (float*)take(4 * (M + 1) * 6 * P);
  w.S = (double*)take(8 * (nmax + 1) * (nmax + 1));
  w.Hd = (double*)take(8 * (nmax + 16));  // + 16 debug stamp slots
  w.dx = (float*)take(4 * nmax);
  w.Wi = (double*)take(8 * 64 * 64 * ((nmax + 63) / 64));
  w.krow = (int*)take(4 * (nF + 1));
  w.mslot = (int*)take(4 * (M + 1));
  w.ld = (int)(nmax + 1);
  if (out) *out = w;
  return off;
}

// target / weight of term e at pixel p: live layout [M,P,2], DROID layout [M,2,P] (geom_kernels.cu:304-309)
__device__ __forceinline__ void load_tw(const BAArgs& a, int e, int p, int P, float2& tgt, float2& wg) {
  if (a.droid) {
    const int64_t o = (int64_t)e * 2 * P + p;
    tgt = make_float2(a.target[o], a.target[o + P]);
    wg = make_float2(a.weight[o], a.weight[o + P]);
  } else {
    const int64_t o2 = ((int64_t)e * P + p) * 2;
    tgt = *reinterpret_cast<const float2*>(a.target + o2);
    wg = *reinterpret_cast<const float2*>(a.weight + o2);
  }
}
// validity weight: live z0... target-side z > 0.1 (geom.py:263; the panorama's range and pole test, camera.cuh); DROID
// !(z < 0.25) (geom_kernels.cu:33,304)
template <int CAM>
__device__ __forceinline__ float valid_weight(const BAArgs& a, const float (&X1)[3], bool inb) {
  const bool ok = a.droid ? !(X1[2] < 0.25f) : cam::valid_point<CAM>(X1[0], X1[1], X1[2]);
  return (inb && ok) ? a.p.weight_scale : 0.0f;
}
// per-term transforms incl. the DROID stereo term (ii == jj: fixed baseline, no pose blocks; geom_kernels.cu:222-233)
template <int CAM>
__device__ __forceinline__ void term_setup(const BAArgs& a, int e, TermGeom& g) {
  const int pi = (int)a.pi[e], pj = (int)a.pj[e], qj = (int)a.qj[e];
  term_transforms(a.poses, a.rig, pi, (int)a.qi[e], pj, qj, g.T, g.G, g.Rr);
  g.Ij = cam::load<CAM>(a.intr + qj * (4 + a.D), a.D, 1.0f / a.p.intr_factor, a.p.ht, a.p.wd);
  g.e = e;
  g.merge = (pi == pj);
  if (a.droid && pi == pj) {
    g.merge = 2;  // stereo
    for (int i = 0; i < 9; ++i) g.T.R[i] = g.G.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    g.T.t[0] = g.G.t[0] = -0.1f;
    g.T.t[1] = g.T.t[2] = g.G.t[1] = g.G.t[2] = 0.0f;
  }
  g.rig_adj = !(g.Rr.t[0] == 0.f && g.Rr.t[1] == 0.f && g.Rr.t[2] == 0.f && g.Rr.R[0] == 1.f &&
                g.Rr.R[4] == 1.f && g.Rr.R[8] == 1.f);
  g.sj = g.merge ? -1 : a.w.pose_slot[pj];
}
// sensor-depth prior and damping of one pixel's disparity block.  Live: frame-level flag, C += alpha, then the
// damping 1e-7 + (0.2 eta + 1e-7) (terms.py:258-268, buffer.py:482-489).  DROID: per-pixel mask m = sens > 0,
// C += m ? alpha : eta, w -= m alpha (d - sens) (geom_kernels.cu:1359-1369).
__device__ __forceinline__ void finish_disp(const BAArgs& a, int k, int p, int P, int flags, float d, float& C, float& wz) {
  const int64_t kp = (int64_t)k * P + p;
  if (a.droid) {
    const float sv = a.sens[kp];
    if (sv > 0.0f) { C += a.p.alpha; wz -= a.p.alpha * (d - sv); }
    else C += a.eta[(int64_t)a.w.krow[k] * P + p];
  } else {
    if (a.w.sens_sum[k] > 0.0f) {  // frames with sensor depth (buffer.py:470-471); read per call, not part of the plan
      C += a.p.alpha;
      wz -= a.p.alpha * (d - a.sens[kp]);
    }
    C += 1e-7f + (0.2f * a.eta[kp] + 1e-7f);
  }
}

__device__ __forceinline__ void s_add(const BAWs& w, int row, int col, double v) {
  // lower triangle storage: (row, col) with row >= col
  if (row < col) { int tmp = row; row = col; col = tmp; }
  atomicAdd(&w.S[(int64_t)row * w.ld + col], v);
}

// 1/sqrt(x) in fp64: hardware estimate + 2 Newton steps (avoids the long sqrt / divide sequences on the
// factorisation's critical path)
__device__ __forceinline__ double rsqrt_nr(double x) {
  double r = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
  r = r * __builtin_fma(-hx * r, r, 1.5);
  r = r * __builtin_fma(-hx * r, r, 1.5);
  return r;
}

// ---- shared by the four solvers (LDS band, LDS dense, global memory, tiled)

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)u, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// (i, j), j <= i, of the lower-triangle entry with linear index q = i (i + 1) / 2 + j
__device__ __forceinline__ void tri_index(int q, int& i, int& j) {
  i = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
  while ((i + 1) * (i + 2) / 2 <= q) ++i;
  while (i * (i + 1) / 2 > q) --i;
  j = q - i * (i + 1) / 2;
}

// LM damping of the diagonal entry v of row r (matrix.py:179-186): v + ep + lambda * diag(H).  Pose rows (r < npr): the
// caller's (lambda, ep); intrinsics rows 1e-6 / 1e-6; rig-rotation rows 1e-4 / 1e-4 (buffer.py:466,498,503).  hd = Hd[r],
// loaded by the caller (the LDS solvers preload it with the matrix entries); DROID damps with the reduced diagonal itself
// (geom_kernels.cu:1176) and does not read it.
__device__ __forceinline__ double damped_diag(const BAArgs& a, int r, int npr, double v, double hd) {
  const bool pose = r < npr, rigrow = a.mv && r >= npr + a.nintr;
  const double ep = pose ? (double)a.p.pose_ep : (rigrow ? 1e-4 : 1e-6);
  const double lam = pose ? (double)a.p.pose_damping : (rigrow ? 1e-4 : 1e-6);
  return v + (ep + lam * (a.droid ? v : hd));
}

// the step of unknown dd as float; zero after a failed pivot (`bad`) and for a NaN
__device__ __forceinline__ void store_step(const BAWs& w, int dd, double x, bool bad) {
  if (bad || !(x == x)) x = 0.0;
  w.dx[dd] = (float)x;
}

// Retraction shared by the four solvers: poses X <- Exp(dx) X (retractor.py:27-29), intrinsics (retractor.py:50-62)
__device__ __forceinline__ void apply_retraction(const BAArgs& a, int t, int nthreads, int n_free) {
  const BAWs& w = a.w;
  for (int sl = t; sl < n_free; sl += nthreads) {
    const int pidx = w.slot_pose[sl];
    float xi[6];
    for (int q = 0; q < 6; ++q) xi[q] = w.dx[6 * sl + q];
    lie::SE3<float> X(a.poses + 7 * pidx);
    (lie::SE3<float>::exp(xi) * X).store(a.poses + 7 * pidx);
  }
  if (a.mv) {
    // one intrinsics block per view (retractor.py:50-62 with len(dx) == V) and one rotation-only step per view >= 1
    // (retractor.py:32-37: the translation part of the tangent is zeroed, X <- Exp([0, phi]) X)
    const int F = 1 + a.D, V = a.p.n_views;
    if (a.p.optimize_intrinsics && t < V) {
      float* I = a.intr + t * (4 + a.D);
      const float df = w.dx[6 * n_free + t * F];
      I[0] += df; I[1] += df;
      if (F > 1) I[4] += 0.01f * w.dx[6 * n_free + t * F + 1];
    }
    if (a.p.optimize_rig_rotation && t >= 1 && t < V) {
      float xi[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int q = 3; q < 6; ++q) xi[q] = w.dx[6 * n_free + a.nintr + 6 * (t - 1) + q];
      lie::SE3<float> X(a.rig + 7 * t);
      (lie::SE3<float>::exp(xi) * X).store(a.rig + 7 * t);
    }
  } else if (a.p.optimize_intrinsics && t == 0) {
    const int F = 1 + a.D;
    const float df = w.dx[6 * n_free];
    for (int vq = 0; vq < a.p.n_views; ++vq) {
      float* I = a.intr + vq * (4 + a.D);
      if (I[0] > 0) { I[0] += df; I[1] += df; if (F > 1) I[4] += 0.01f * w.dx[6 * n_free + 1]; }
    }
  }
}
