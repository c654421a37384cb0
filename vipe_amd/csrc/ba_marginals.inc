// ------------------------------------------------------------------------------------------------ marginals
//
// Marginal covariances of the damped Gauss-Newton system H = [[B, E], [E^T, C]], C diagonal, S = B - E C^-1 E^T:
//   disparity of pixel p of a free frame k:  var = 1 / C_p + (e_p^T S^-1 e_p) / C_p^2
//   free pose:                               the 6 x 6 diagonal block of S^-1 at its slot
// e_p is the column of E of that pixel: E_kk at the slot of the frame's own pose, E_j[e] at the slot of pj[e] for every
// term of the frame's CSR row, and the tail rows E_f (mono) / E_t (rig) - the blocks ba_retract_kernel multiplies with dx.
// vipe_dense_ba_linearize leaves them in the workspace; S^-1 comes from the caller (fp64, full symmetric).

// slot of the target pose of every term in CSR order, -1 for pi == pj and for fixed targets (the marginals read the
// workspace alone: the caller's index arrays are gone by then)
__global__ void ba_term_slot_kernel(BAArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.p.M) return;
  const int e = a.w.order[c];
  const int pj = (int)a.pj[e];
  a.w.mslot[c] = ((int)a.pi[e] == pj) ? -1 : a.w.pose_slot[pj];
}

// the reduced system as the solvers see it: symmetric, LM damping on the diagonal (damped_diag), n = info[INFO_UNKNOWNS] rows
__global__ void ba_export_reduced_kernel(BAArgs a, double* __restrict__ out, int ld_out) {
  const BAWs& w = a.w;
  const int n = min(w.info[INFO_UNKNOWNS], ld_out), npr = 6 * w.info[INFO_FREE_POSES];
  const int64_t nn = (int64_t)n * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / n), c = (int)(i % n);
    double v = w.S[(int64_t)max(r, c) * w.ld + min(r, c)];
    if (r == c) v = damped_diag(a, r, npr, v, w.Hd[r]);
    out[(int64_t)r * ld_out + c] = v;
  }
}

constexpr int MG_CH = 24;  // rows of e_p per chunk: four pose blocks; a chunk pair is a 24 x 24 sub-block of S^-1 in LDS.
                           // (48 rows - a frame of <= 7 targets in ONE pair - took 232 VGPRs and was slower, 41 us against
                           // 28 us on the 48-keyframe graph: the kernel is bound by the LDS broadcast reads, not by latency)

struct MargRow {
  const float* e;  // row of E over the pixels of the frame, nullptr: no unknown of the reduced system behind it
  int gcol;
};

// row r of e_p for frame k: 6 rows per member (own pose, then the terms of the CSR row), then the tail
__device__ __forceinline__ MargRow marg_row(const BAArgs& a, int k, int beg, int deg, int si, int foff, int r) {
  const BAWs& w = a.w;
  const int64_t P = a.P;
  MargRow m{nullptr, -1};
  if (r < 6 * (deg + 1)) {
    const int mm = r / 6, q = r % 6;
    if (mm == 0) {
      if (si >= 0) { m.gcol = 6 * si + q; m.e = w.Ekk + ((int64_t)k * 6 + q) * P; }
    } else {
      const int c = beg + mm - 1, sj = w.mslot[c];
      if (sj >= 0) { m.gcol = 6 * sj + q; m.e = w.Ej + ((int64_t)w.order[c] * 6 + q) * P; }
    }
  } else if (r < 6 * (deg + 1) + a.ntail) {
    const int f = r - 6 * (deg + 1);
    m.gcol = foff + f;
    m.e = a.mv ? w.Et + ((int64_t)k * a.ntail + f) * P : w.Ef + ((int64_t)k * 2 + f) * P;
  }
  return m;
}

// grid (pixel tiles, source frames).  q = e^T S^-1 e is summed over chunk pairs (A, B <= A) of MG_CH rows: the sub-block
// of S^-1 at the two chunks' slots is gathered once per workgroup into LDS as f32 and read as broadcasts, the lanes' own
// E rows are coalesced loads.  A frame of any degree takes the same loop (three pairs for 6 targets, 153 for 64 targets).
// f32 accumulation in a fixed order, plain stores: repeated calls are bitwise equal.
struct MargLds {
  float M[MG_CH][MG_CH];
  const float* erow[2][MG_CH];
  int gcol[2][MG_CH];
};

// rows [c * MG_CH, (c + 1) * MG_CH) of e_p into side `side` of the descriptors (lanes 0 .. MG_CH - 1)
__device__ __forceinline__ void marg_chunk(const BAArgs& a, MargLds& sh, int side, int c, int k, int beg, int deg, int si,
                                           int foff, int n) {
  if (threadIdx.x < MG_CH) {
    const MargRow m = marg_row(a, k, beg, deg, si, foff, c * MG_CH + threadIdx.x);
    const bool on = m.e && m.gcol < n;
    sh.erow[side][threadIdx.x] = on ? m.e : nullptr;
    sh.gcol[side][threadIdx.x] = on ? m.gcol : -1;
  }
}
// sub-block of S^-1 at (rows of side 0, rows of side sb), zero where either row stands for no unknown
__device__ __forceinline__ void marg_gather(MargLds& sh, int sb, const double* __restrict__ Sinv, int ld) {
  for (int i = threadIdx.x; i < MG_CH * MG_CH; i += TILE) {
    const int gi = sh.gcol[0][i / MG_CH], gj = sh.gcol[sb][i % MG_CH];
    sh.M[i / MG_CH][i % MG_CH] = (gi >= 0 && gj >= 0) ? (float)Sinv[(int64_t)gi * ld + gj] : 0.0f;
  }
}
__device__ __forceinline__ void marg_load(const MargLds& sh, int side, int pc, float (&e)[MG_CH]) {
#pragma unroll
  for (int i = 0; i < MG_CH; ++i) e[i] = sh.erow[side][i] ? sh.erow[side][i][pc] : 0.0f;
}
// ea^T M eb; DIAG: ea and eb are the same chunk and M is symmetric - the strict lower triangle counts twice, half the reads
template <bool DIAG>
__device__ __forceinline__ float marg_form(const MargLds& sh, const float (&ea)[MG_CH], const float (&eb)[MG_CH]) {
  float t = 0.0f;
#pragma unroll
  for (int i = 0; i < MG_CH; ++i) {
    float r = 0.0f;
#pragma unroll
    for (int j = 0; j < (DIAG ? i : MG_CH); ++j) r += sh.M[i][j] * eb[j];
    t += ea[i] * (DIAG ? 2.0f * r + sh.M[i][i] * ea[i] : r);
  }
  return t;
}

__global__ __launch_bounds__(TILE) void ba_disp_variance_kernel(BAArgs a, const double* __restrict__ Sinv, int ld,
                                                                float* __restrict__ var) {
  const BAWs& w = a.w;
  const int k = blockIdx.y;
  if (!(w.fflags[k] & 2)) return;
  const int P = a.P;
  const int p = blockIdx.x * TILE + threadIdx.x;
  const int pc = min(p, P - 1);
  const int beg = w.rowptr[k], deg = w.rowptr[k + 1] - beg;
  const int si = w.pose_slot[k / a.p.n_views];
  const int foff = 6 * w.info[INFO_FREE_POSES], n = min(w.info[INFO_UNKNOWNS], ld);
  const int R = 6 * (deg + 1) + a.ntail, nch = (R + MG_CH - 1) / MG_CH;
  __shared__ MargLds sh;

  float q = 0.0f;
  for (int A = 0; A < nch; ++A) {
    __syncthreads();  // the previous pair has read M and the descriptors
    marg_chunk(a, sh, 0, A, k, beg, deg, si, foff, n);
    __syncthreads();
    float eA[MG_CH];
    marg_load(sh, 0, pc, eA);
    marg_gather(sh, 0, Sinv, ld);
    __syncthreads();
    q += marg_form<true>(sh, eA, eA);
    for (int B = 0; B < A; ++B) {
      __syncthreads();
      marg_chunk(a, sh, 1, B, k, beg, deg, si, foff, n);
      __syncthreads();
      float eB[MG_CH];
      marg_load(sh, 1, pc, eB);
      marg_gather(sh, 1, Sinv, ld);
      __syncthreads();
      q += 2.0f * marg_form<false>(sh, eA, eB);  // S^-1 is symmetric: the pair (B, A) is the pair (A, B)
    }
  }
  if (p < P) {
    const int64_t kp = (int64_t)k * P + p;
    const float ic = 1.0f / w.C[kp];
    var[kp] = ic + fmaxf(q, 0.0f) * ic * ic;  // both summands are >= 0; a rounding-negative form is clamped
  }
}

// pose blocks of S^-1, and S / Hd zeroed again as ba_retract_kernel leaves them (a later call that reuses the plan in this
// workspace starts its accumulation from zero)
__global__ void ba_marginals_finish_kernel(BAArgs a, const double* __restrict__ Sinv, int ld, double* __restrict__ pose_cov) {
  const BAWs& w = a.w;
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ns = (int64_t)w.ld * w.ld;
  for (int64_t i = gid; i < ns; i += nthr) w.S[i] = 0.0;
  for (int64_t i = gid; i < (int64_t)w.ld - 1; i += nthr) w.Hd[i] = 0.0;
  if (!Sinv || !pose_cov) return;
  const int n = min(w.info[INFO_UNKNOWNS], ld);
  for (int64_t i = gid; i < (int64_t)a.p.n_poses * 36; i += nthr) {
    const int sl = w.pose_slot[i / 36], r = (int)(i % 36) / 6, c = (int)(i % 36) % 6;
    if (sl >= 0 && 6 * sl + 5 < n) pose_cov[i] = Sinv[(int64_t)(6 * sl + r) * ld + 6 * sl + c];
  }
}
