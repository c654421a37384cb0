// ------------------------------------------------------------------------------------------------ plan

__global__ __launch_bounds__(256) void ba_sens_kernel(const float* __restrict__ sens, float* __restrict__ out, int P,
                                                      int* __restrict__ info) {
  // buffer.py:470-471: frames whose sensor disparity sums to > 0
  const int k = blockIdx.x;
  if (k == 0 && threadIdx.x == 0) {
    info[INFO_FAILURES] = 0;  // Cholesky failure count of this call (also when the plan is reused)
    info[INFO_SOLVER] = SOLVER_GLOBAL;  // what a call in which nothing solved reports
  }
  float s = 0.f;
  for (int p = threadIdx.x; p < P; p += blockDim.x) s += sens[(int64_t)k * P + p];
  s = wave_sum(s);
  __shared__ float red[NWAVE];
  if (lane_id() == 0) red[wave_id()] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[k] = red[0] + red[1] + red[2] + red[3];
}

// exclusive scan of v[0..n) in place with 1024 threads; returns the total (all threads)
__device__ int block_scan_excl(int* v, int n, int* lds /* [1024] */) {
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int b = t * per;
  int s = 0;
  for (int i = b; i < b + per && i < n; ++i) s += v[i];
  lds[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    int x = t >= o ? lds[t - o] : 0;
    __syncthreads();
    lds[t] += x;
    __syncthreads();
  }
  int run = t > 0 ? lds[t - 1] : 0;
  const int total = lds[1023];
  for (int i = b; i < b + per && i < n; ++i) {
    int c = v[i];
    v[i] = run;
    run += c;
  }
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(1024) void ba_plan_kernel(BAArgs a) {
  const vipe_ba_params& p = a.p;
  const int t = threadIdx.x;
  const int nP = p.n_poses, nF = a.nF, M = p.M, V = p.n_views;
  int* cnt = a.w.scratch;           // [nF]
  int* is_src = cnt + nF;           // [nP]
  int* used = is_src + nP;          // [nP]
  __shared__ int lds[1024];
  __shared__ int stage[4096];
  for (int i = t; i < nF; i += 1024) cnt[i] = 0;
  for (int i = t; i < nP; i += 1024) { is_src[i] = 0; used[i] = 0; }
  __syncthreads();
  for (int e = t; e < M; e += 1024) {
    atomicAdd(&cnt[(int)a.di[e]], 1);
    is_src[(int)a.pi[e]] = 1;
    used[(int)a.pi[e]] = 1;
    used[(int)a.pj[e]] = 1;
  }
  __syncthreads();
  // frame flags before cnt is turned into offsets
  const bool all_fixed = !(p.t0 < p.t1);
  int nfd_local = 0;
  for (int k = t; k < nF; k += 1024) {
    const int pose = k / V;
    int f = cnt[k] > 0 ? 1 : 0;
    if (a.droid) {
      // disparity frames = unique(arange(t0,t1) U ii) (geom_kernels.cu:1297-1303); bit 3: in the set without terms
      const bool inkx = f || (k >= p.t0 && k < p.t1);
      a.w.krow[k] = inkx ? 1 : 0;
      if (inkx && !p.motion_only) { f |= 2; ++nfd_local; if (!(f & 1)) f |= 8; }
    } else {
      bool dfree = f && !p.motion_only && !(p.limited_disp && (pose < p.t0 || pose >= p.t1));  // buffer.py:490-493
      if (dfree) { f |= 2; ++nfd_local; }
    }
    a.w.fflags[k] = f;
  }
  if (a.droid) {
    __syncthreads();
    block_scan_excl(a.w.krow, nF, lds);
  }
  // rowptr = exclusive scan of counts
  for (int i = t; i < nF; i += 1024) a.w.rowptr[i] = cnt[i];
  __syncthreads();
  const int total = block_scan_excl(a.w.rowptr, nF, lds);
  if (t == 0) a.w.rowptr[nF] = total;
  // pose slots (buffer.py:462-465: fixed iff it is a source pose outside [t0,t1); t0 == t1 fixes all)
  for (int i = t; i < nP; i += 1024) {
    const bool fixed = all_fixed || (is_src[i] && (i < p.t0 || i >= p.t1));
    // DROID: the system has one block per pose of [t0, t1), used or not (SparseBlock(t1 - t0, 6))
    a.w.pose_slot[i] = a.droid ? ((i >= p.t0 && i < p.t1) ? 1 : 0) : ((used[i] && !fixed) ? 1 : 0);
  }
  __syncthreads();
  for (int i = t; i < nP; i += 1024) is_src[i] = a.w.pose_slot[i];  // keep the 0/1 flags
  __syncthreads();
  const int n_free = block_scan_excl(a.w.pose_slot, nP, lds);
  for (int i = t; i < nP; i += 1024) {
    if (is_src[i]) a.w.slot_pose[a.w.pose_slot[i]] = i;
    else a.w.pose_slot[i] = -1;
  }
  // count free disparity frames
  lds[t] = nfd_local;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) lds[t] += lds[t + o];
    __syncthreads();
  }
  if (t == 0) {
    a.w.info[INFO_FREE_POSES] = n_free;
    a.w.info[INFO_FREE_DISP] = lds[0];
    a.w.info[INFO_FAILURES] = 0;
    a.w.info[INFO_UNKNOWNS] = 6 * n_free + a.ntail;
    a.w.info[INFO_BAND_BLOCKS] = 0;  // band width of the reduced pose system in 6x6 blocks (filled below)
    a.w.info[INFO_MAX_DEGREE] = 0;  // largest number of terms of one source frame (selects the accumulate kernel)
  }
  // stable counting sort of the terms by source frame: frame k's owner scans the term list in order
  // (cursor kept in cnt[]: reuse cnt as the running write position)
  __syncthreads();
  for (int k = t; k < nF; k += 1024) cnt[k] = a.w.rowptr[k];
  for (int c0 = 0; c0 < M; c0 += 4096) {
    const int nc = min(4096, M - c0);
    __syncthreads();
    for (int i = t; i < nc; i += 1024) stage[i] = (int)a.di[c0 + i];
    __syncthreads();
    for (int k = t; k < nF; k += 1024) {
      if (!(a.w.fflags[k] & 1)) continue;
      int pos = cnt[k];
      for (int i = 0; i < nc; ++i)
        if (stage[i] == k) a.w.order[pos++] = c0 + i;
      cnt[k] = pos;
    }
  }
  // Band of the reduced system: two poses couple (directly through H_ij or through the Schur complement of a
  // source frame) only if they are members {pose of k} + {targets of k's terms} of the same frame k.
  __syncthreads();
  for (int k = t; k < nF; k += 1024) {
    if (!(a.w.fflags[k] & 1)) continue;
    int lo = 1 << 30, hi = -1;
    const int si = a.w.pose_slot[k / V];
    if (si >= 0) { lo = si; hi = si; }
    for (int q = a.w.rowptr[k]; q < a.w.rowptr[k + 1]; ++q) {
      const int sj = a.w.pose_slot[(int)a.pj[a.w.order[q]]];
      if (sj >= 0) { lo = min(lo, sj); hi = max(hi, sj); }
    }
    if (hi >= 0) atomicMax(&a.w.info[INFO_BAND_BLOCKS], hi - lo);
    atomicMax(&a.w.info[INFO_MAX_DEGREE], a.w.rowptr[k + 1] - a.w.rowptr[k]);
  }
}
