// ------------------------------------------------------------------------------------------------ retract

template <int F>
__global__ __launch_bounds__(TILE) void ba_retract_kernel(BAArgs a) {
  const BAWs& w = a.w;
  {
    // The reduced system has been solved (this kernel only reads dx): clear S and Hd for the next accumulation here,
    // spread over the whole grid, instead of two memset launches per Gauss-Newton iteration.
    const int64_t nthr = (int64_t)gridDim.x * gridDim.y * TILE;
    const int64_t gid = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * TILE + threadIdx.x;
    const int64_t ns = (int64_t)w.ld * w.ld;
    for (int64_t i = gid; i < ns; i += nthr) w.S[i] = 0.0;
    for (int64_t i = gid; i < (int64_t)w.ld - 1; i += nthr) w.Hd[i] = 0.0;
  }
  const int k = blockIdx.y;
  const int flags = w.fflags[k];
  if (!(flags & 2)) return;
  const int P = a.P, V = a.p.n_views;
  const int p = blockIdx.x * TILE + threadIdx.x;
  if (p >= P) return;
  const int64_t kp = (int64_t)k * P + p;
  if (flags & 8) {
    // DROID: frame of [t0, t1) without terms - only the depth prior acts on it (geom_kernels.cu:1359-1369)
    float C = 0.f, wz = 0.f;
    finish_disp(a, k, p, P, flags, a.disps[kp], C, wz);
    const float dz = wz / C;
    a.disps[kp] += dz;
    if (a.dz_out) a.dz_out[(int64_t)w.krow[k] * P + p] = dz;
    return;
  }
  const int beg = w.rowptr[k], end = w.rowptr[k + 1];
  float rhs = w.wv[kp];
  const int si = w.pose_slot[k / V];
  const int n_free = w.info[INFO_FREE_POSES];
  // DROID leaves pose slot 0 out of the back-substitution (EvT6x1_kernel: idx <= 0 returns, geom_kernels.cu:1085)
  const int smin = a.droid ? 1 : 0;
  if (si >= smin) {
#pragma unroll
    for (int q = 0; q < 6; ++q) rhs -= w.Ekk[((int64_t)k * 6 + q) * P + p] * w.dx[6 * si + q];
  }
  for (int c = beg; c < end; ++c) {
    const int e = w.order[c];
    const int pj = (int)a.pj[e];
    const int sj = ((int)a.pi[e] == pj) ? -1 : w.pose_slot[pj];
    if (sj < smin) continue;
#pragma unroll
    for (int q = 0; q < 6; ++q) rhs -= w.Ej[((int64_t)e * 6 + q) * P + p] * w.dx[6 * sj + q];
  }
  if constexpr (F > 0) {
#pragma unroll
    for (int f = 0; f < F; ++f) rhs -= w.Ef[((int64_t)k * 2 + f) * P + p] * w.dx[6 * n_free + f];
  }
  if (a.mv) {
    for (int f = 0; f < a.ntail; ++f) rhs -= w.Et[((int64_t)k * a.ntail + f) * P + p] * w.dx[6 * n_free + f];
  }
  float dz = rhs / w.C[kp];
  if (!a.droid && dz > 10.0f) dz = 0.0f;  // retractor.py:41
  a.disps[kp] += dz;
  if (a.dz_out) a.dz_out[(int64_t)w.krow[k] * P + p] = dz;
}

__global__ void clamp_min_kernel(float* __restrict__ x, int64_t n, float lo) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    x[i] = fmaxf(x[i], lo);  // fmaxf(NaN, lo) = lo where torch.clamp keeps the NaN: on purpose, a NaN disparity leaves as lo (DESIGN.md section 2)
}
