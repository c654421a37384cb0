// ------------------------------------------------------------------------------------------------ solve

// Cholesky solve of the reduced system in global memory by ONE workgroup of 8 waves, fp64: the systems of up to
// CT_MIN_N unknowns that neither LDS solver takes (global_form, ba_route.cuh; multi-view rigs among them).
//   S: lower triangle, row-major, ld; row n holds the rhs, so the forward substitution y = L^-1 g falls out of
//   the factorisation as the last panel row.  Right-looking, NB = 12 columns per step:
//     1. diagonal block: wave 0, one matrix row per lane in registers, column by column with the finished columns
//        published to LDS;
//     2. panel: one row per thread - only the rows that can be nonzero in these columns, i.e. the pose rows inside
//        the band and the dense tail rows - X Lkk^T = A by forward substitution against Lkk in LDS; the solved panel
//        is also kept TRANSPOSED in LDS (PT[j][panel row]), where the update reads its operands;
//     3. trailing update A22 -= P P^T on the fp64 matrix cores: 16 x 16 tiles of the panel rows' lower triangle, one
//        tile per wave at a time, S read-modify-write.
//   Then the diagonal blocks are inverted in place (upper triangle of S, Hd), the backward substitution L^T x = y
//   runs block by block, and the poses / intrinsics / rig are retracted.  Reports SOLVER_GLOBAL in info[INFO_SOLVER].
// The panel always fits its LDS buffer: n <= CT_MIN_N here, and run_iters (ba.hip) checks CT_MIN_N + 1 <= panel_cap.
constexpr int NB = 12;
constexpr int SOLVE_T = 512;  // 8 waves: up to 256 VGPRs per lane, no spills in the register-resident phases

struct SolveLds {
  double Lkk[NB][NB + 1];
  double rdiag[NB];  // 1 / L[j][j]
  double xk[NB];
  int fail;
};

__global__ __launch_bounds__(SOLVE_T) void ba_solve_kernel(BAArgs a, int panel_cap) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  SolveLds& sh = *reinterpret_cast<SolveLds*>(smem_raw);
  double* PT = reinterpret_cast<double*>(smem_raw + ((sizeof(SolveLds) + 15) / 16) * 16);  // [NB][panel_cap]
  const BAWs& w = a.w;
  const int t = threadIdx.x;
  const int n = w.info[INFO_UNKNOWNS], n_free = w.info[INFO_FREE_POSES];
  const int ld = w.ld;
  double* S = w.S;
  if (t == 0) sh.fail = 0;
  if (global_form(route_in(a)) != GLOBAL_ONE_WORKGROUP) return;
  // LM damping on the diagonal
  for (int dd = t; dd < n; dd += SOLVE_T) {
    double& sdd = S[(int64_t)dd * ld + dd];
    sdd = damped_diag(a, dd, 6 * n_free, sdd, a.droid ? 0.0 : w.Hd[dd]);
  }
  __syncthreads();
  const int npose_rows = 6 * n_free;
  const int bandblk = w.info[INFO_BAND_BLOCKS];  // band of the pose part in 6x6 blocks (plan kernel)

  for (int k0 = 0; k0 < n; k0 += NB) {
    const int bw = min(NB, n - k0);
    // ---- 1. diagonal block (wave 0)
    if (t < WAVE) {
      double row[NB];
      const int r = t;
      if (r < bw) {
#pragma unroll
        for (int c = 0; c < NB; ++c) row[c] = (c <= r && c < bw) ? S[(int64_t)(k0 + r) * ld + k0 + c] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j < bw) {
          double sacc = 0.0;
          if (r >= j && r < bw) {
            sacc = row[j];
#pragma unroll
            for (int m = 0; m < NB; ++m)
              if (m < j) sacc -= row[m] * sh.Lkk[j][m];
          }
          // pivot from lane j
          double piv = __shfl(sacc, j, WAVE);
          if (!(piv > 0.0)) {
            if (r == 0) sh.fail = 1;
            piv = 1.0;
          }
          const double rl = rsqrt_nr(piv);
          if (r >= j && r < bw) {
            row[j] = (r == j) ? piv * rl : sacc * rl;
            sh.Lkk[r][j] = row[j];
            if (r == j) sh.rdiag[j] = rl;
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
      }
      if (r < bw) {
#pragma unroll
        for (int c = 0; c < NB; ++c)
          if (c <= r) S[(int64_t)(k0 + r) * ld + k0 + c] = row[c];
      }
    }
    __syncthreads();
    // ---- 2. panel rows r0..n (row n = rhs)
    // Rows below the block that can be nonzero in these columns: the band [r0, e1) of pose rows plus the dense
    // tail [t0, n] (intrinsics rows and the rhs row).  Compact panel index pr -> global row prow(pr).
    const int r0 = k0 + bw;
    const int e1 = r0 < npose_rows ? min(npose_rows, 6 * ((k0 + bw - 1) / 6 + bandblk + 1)) : r0;
    const int t0 = max(r0, npose_rows);
    const int nb1 = max(e1 - r0, 0);
    const int m = nb1 + (n - t0 + 1);
    auto prow = [&](int pr) { return pr < nb1 ? r0 + pr : t0 + (pr - nb1); };
    for (int pr = t; pr < m; pr += SOLVE_T) {
      double x[NB];
      double* grow = S + (int64_t)prow(pr) * ld + k0;
#pragma unroll
      for (int j = 0; j < NB; ++j) x[j] = j < bw ? grow[j] : 0.0;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j < bw) {
          double sacc = x[j];
#pragma unroll
          for (int q = 0; q < NB; ++q)
            if (q < j) sacc -= x[q] * sh.Lkk[j][q];
          x[j] = sacc * sh.rdiag[j];
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j < bw) grow[j] = x[j];
        PT[j * panel_cap + pr] = j < bw ? x[j] : 0.0;
      }
    }
    __syncthreads();
    // ---- 3. trailing update A22 -= P P^T on the fp64 matrix cores (v_mfma_f64_16x16x4_f64): 16x16 tiles of the
    //         lower triangle, one tile per wave at a time, K = NB = 3 MFMAs; operands straight from the
    //         transposed panel in LDS (lane l: A[row l&15][k l>>4], B[k l>>4][col l&15]).
    {
      typedef double double4v __attribute__((ext_vector_type(4)));
      const int wv = t >> 6, ln = t & 63;
      const int nt = (m + 15) >> 4;
      const int ntiles = nt * (nt + 1) / 2;
      for (int q = wv; q < ntiles; q += SOLVE_T / 64) {
        int ti, tj;
        tri_index(q, ti, tj);
        double4v c = {0.0, 0.0, 0.0, 0.0};
        const int ar = 16 * ti + (ln & 15), bc = 16 * tj + (ln & 15), kq = ln >> 4;
#pragma unroll
        for (int s4 = 0; s4 < NB / 4; ++s4) {
          const double av = PT[(4 * s4 + kq) * panel_cap + ar];
          const double bv = PT[(4 * s4 + kq) * panel_cap + bc];
          c = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
        }
        const int cc = 16 * tj + (ln & 15);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int rr = 16 * ti + (ln >> 4) + 4 * r4;
          if (rr < m && cc <= rr && cc <= m - 2) S[(int64_t)prow(rr) * ld + prow(cc)] -= c[r4];
        }
      }
    }
    __syncthreads();
  }

  // ---- backward substitution L^T x = y (y = row n).
  // (i) invert every diagonal block Lkk (lower triangular) in parallel, one wave per block, lane c = column c of
  //     the inverse by forward substitution; the inverse overwrites the STRICT UPPER part + a side array is not
  //     needed: it is written to the (unused) upper triangle of S at the block's position, transposed, i.e.
  //     S[k0+c][k0+j] (j > c) := Linv[j][c], and the inverse's diagonal to Hd (no longer needed).
  {
    const int nblk = (n + NB - 1) / NB;
    const int wv = t >> 6, ln = t & 63;
    for (int blk = wv; blk < nblk; blk += SOLVE_T / 64) {
      const int k0 = blk * NB, bw = min(NB, n - k0);
      if (ln < bw) {
        const int c = ln;
        double z[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if (j < bw && j >= c) {
            double sacc = (j == c) ? 1.0 : 0.0;
#pragma unroll
            for (int q = 0; q < NB; ++q)
              if (q < j) sacc -= S[(int64_t)(k0 + j) * ld + k0 + q] * z[q];  // z[q] == 0 for q < c
            z[j] = sacc / S[(int64_t)(k0 + j) * ld + k0 + j];
          } else {
            z[j] = 0.0;
          }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if (j < bw && j > c) S[(int64_t)(k0 + c) * ld + k0 + j] = z[j];  // upper triangle: Linv[j][c]
          if (j == c) w.Hd[k0 + c] = z[j];
        }
      }
    }
  }
  __syncthreads();
  // (ii) blocks from the last to the first: x_k = Lkk^-T y_k (an NB x NB mat-vec, lane j: sum_m Linv[m][j] y[m]),
  //      then y_c -= sum_m L[k0+m][c] x_k[m] for every earlier column c (coalesced row reads).
  double* yrow = S + (int64_t)n * ld;
  for (int k0 = ((n - 1) / NB) * NB; k0 >= 0; k0 -= NB) {
    const int bw = min(NB, n - k0);
    if (t < WAVE) {
      if (t < bw) sh.xk[t] = yrow[k0 + t];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      double xj = 0.0;
      if (t < bw) {
        // Linv[m][j] for m > j is stored at S[k0+j][k0+m]; Linv[j][j] in Hd
        xj = w.Hd[k0 + t] * sh.xk[t];
        for (int mq = t + 1; mq < bw; ++mq) xj += S[(int64_t)(k0 + t) * ld + k0 + mq] * sh.xk[mq];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      if (t < bw) {
        sh.xk[t] = xj;
        yrow[k0 + t] = xj;
      }
    }
    __syncthreads();
    // rows of this block are zero left of the band (pose rows only; tail rows are dense)
    const int c_lo = (k0 + bw <= npose_rows) ? max(0, 6 * (k0 / 6 - bandblk)) : 0;
    for (int c = c_lo + t; c < k0; c += SOLVE_T) {
      double sacc = 0.0;
      for (int q = 0; q < bw; ++q) sacc += S[(int64_t)(k0 + q) * ld + c] * sh.xk[q];
      yrow[c] -= sacc;
    }
    __syncthreads();
  }
  const bool bad = sh.fail != 0;
  if (t == 0) {
    if (bad) w.info[INFO_FAILURES] += 1;
    w.info[INFO_SOLVER] = SOLVER_GLOBAL;
  }
  for (int dd = t; dd < n; dd += SOLVE_T) store_step(w, dd, yrow[dd], bad);
  __syncthreads();
  apply_retraction(a, t, SOLVE_T, n_free);
}

// ------------------------------------------------------------------------------------------------ solve (tiled, chip wide)
//
// The global BA's reduced systems (n = 600 ... 1200+ unknowns, dense: every keyframe pair may couple) are bound in the
// single-workgroup kernel above by ~n/12 block steps of dependent fp64 chains and L2 round trips on ONE CU (2.1 ms at
// n = 1200).  Here the factorisation is tiled 64 x 64 and spread over the chip, three launches per tile column k:
//   chol_potrf_kernel  one workgroup: wave 0 factors the diagonal tile in registers (lane = row, right-looking: pivot
//                      by readlane, rsqrt from an fp32 seed + one fp64 Newton step, rank-1 update with the column
//                      broadcast lane by lane), then the workgroup inverts the factor (16 x 16 diagonal blocks by
//                      substitution, off-diagonal blocks level by level) and leaves L^-1 in the workspace;
//   chol_trsm_kernel   one workgroup per tile row below: X = A L^-T as a 64^3 product on the fp64 matrix cores;
//   chol_syrk_kernel   one workgroup per tile pair (i >= j > k): A_ij -= X_i X_j^T, same tiles, same cores.
// Row n (the rhs) rides along as a row of the last tile row, so the forward substitution is part of the factorisation;
// chol_backsub_kernel (one workgroup) then solves L^T x = y tile column by tile column with the stored inverses and
// retracts.  LM damping is added by potrf when it loads its tile (the trailing updates only subtract from later tiles,
// so the order is immaterial).  A dependent fp64 operation costs ~40 cycles on this part: the pivot chain alone is
// ~0.15 us per column - the floor of any Cholesky here - which is why the diagonal tile stays in one wave's registers.
constexpr int CT = 64;

__device__ __forceinline__ double rsqrt_seeded(double x) {
  // branch free (the callers are long fully unrolled blocks): pivots of a damped normal matrix are far inside the float
  // range; should one not be, the seed is clamped and the two Newton steps still converge from within a factor 2^64
  const float xf = fminf(fmaxf((float)x, 1e-30f), 1e30f);
  double r = (double)__builtin_amdgcn_rsqf(xf);  // 23 bits
  const double hx = 0.5 * x;
  r = r * __builtin_fma(-hx * r, r, 1.5);          // ~45 bits
  r = r * __builtin_fma(-hx * r, r, 1.5);          // full fp64
  return r;
}

__device__ __forceinline__ bool chol_active(const BAArgs& a, int& n) {
  n = a.w.info[INFO_UNKNOWNS];
  return global_form(route_in(a)) == GLOBAL_TILED;
}

__global__ __launch_bounds__(256) void chol_potrf_kernel(BAArgs a, int k) {
  int n;
  if (!chol_active(a, n)) return;
  const int c0 = CT * k;
  if (c0 >= n) return;
  const int bw = min(CT, n - c0);
  const BAWs& w = a.w;
  const int ld = w.ld, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* S = w.S;
  __shared__ double Ls[CT][CT + 1];   // the factor tile (lower), identity beyond bw
  __shared__ double Li[CT][CT + 1];   // its inverse (lower)
  __shared__ int fail;
  if (t == 0) fail = 0;
  if (k == 0 && t == 0) w.info[INFO_TILED_FAIL] = 0;  // failure flag of this factorisation
  __syncthreads();
  // the tile travels global <-> LDS with all 256 threads (row segments, coalesced), LM damping (damped_diag) added on the
  // way in.  The last tile column of a system with
  // n % 64 != 0 shares its tile row with the rhs (row n = c0 + bw): row bw of the tile carries it through the
  // factorisation as one more row below the diagonal (its own "diagonal" entry is a dummy 1).
  const bool has_rhs = bw < CT && c0 + bw == n;
  {
    const int n_free = w.info[INFO_FREE_POSES];
    double v[16], hd[16];  // all loads of the thread in flight before the first LDS store
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = t + 256 * q, r = i >> 6, c = i & 63;
      v[q] = (r < bw && c <= r) ? S[(int64_t)(c0 + r) * ld + c0 + c] : (c == r ? 1.0 : 0.0);
      if (has_rhs && r == bw && c < bw) v[q] = S[(int64_t)n * ld + c0 + c];
      hd[q] = (r < bw && c == r && !a.droid) ? w.Hd[c0 + r] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = t + 256 * q, r = i >> 6, c = i & 63;
      if (r < bw && c == r) v[q] = damped_diag(a, c0 + r, 6 * n_free, v[q], hd[q]);
      Ls[r][c] = v[q];
    }
  }
  __syncthreads();
  // Blocked right-looking factorisation, four panels of 16 columns.  Panel: wave 0, one tile row per lane, the 16 panel
  // entries of the row in registers; per column the pivot by readlane (compile-time lane), rsqrt from an fp32 seed + two
  // fp64 Newton steps, the finished column published to LDS and read back as BROADCAST reads for the rank-1 update of
  // the remaining panel columns only (<= 14 fused multiply-adds per lane instead of <= 62 over the whole tile row: the
  // dependent pivot chain, ~0.15 us per column, is what is left).  Trailing update: all four waves, 16 x 16 tiles of the
  // lower triangle, A_ij -= P_i P_j^T on the fp64 matrix cores straight in LDS.
  {
    double* colb = &Li[0][0];  // scratch: two column buffers of 64 doubles (Li is not in use yet)
    bool bad = false;
    const int l16 = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int pnl = 0; pnl < 4; ++pnl) {
      const int p0 = 16 * pnl;
      if (wave == 0) {
        const int r = lane;
        double ar[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) ar[c] = Ls[r][p0 + c];
        double d = readlane_f64(ar[0], p0);
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const int j = p0 + jj;
          const bool okp = d > 0.0;
          bad |= (j < bw) & !okp;
          d = okp ? d : 1.0;
          const double rl = rsqrt_seeded(d);
          const double lj = r == j ? d * rl : (r > j ? ar[jj] * rl : 0.0);
          ar[jj] = lj;
          // the NEXT pivot only needs lane j + 1's own entry of this column: form it ahead of the LDS round trip
          if (jj + 1 < 16) {
            ar[jj + 1] = __builtin_fma(-lj, readlane_f64(lj, j + 1), ar[jj + 1]);
            d = readlane_f64(ar[jj + 1], j + 1);
          }
          if (jj + 2 < 16) {
            double* cb = colb + (jj & 1) * CT;
            cb[r] = lj;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int c = jj + 2; c < 16; ++c) ar[c] = __builtin_fma(-lj, cb[p0 + c], ar[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) Ls[r][p0 + c] = ar[c];  // rows above the diagonal hold zeros in finished columns
      }
      __syncthreads();
      if (pnl < 3) {
        // tiles (ti, tj), pnl < tj <= ti <= 3, numbered ti (ti + 1) / 2 + tj relative to pnl + 1
        const int nt = (3 - pnl) * (4 - pnl) / 2;
        for (int e = wave; e < nt; e += 4) {
          int ti = 0;
          while ((ti + 1) * (ti + 2) / 2 <= e) ++ti;
          const int tj = e - ti * (ti + 1) / 2;
          const int R = 16 * (pnl + 1 + ti), C = 16 * (pnl + 1 + tj);
          double4c acc;
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) acc[r4] = Ls[R + kq + 4 * r4][C + l16];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Ls[R + l16][p0 + 4 * s4 + kq], Ls[C + l16][p0 + 4 * s4 + kq], acc, 0, 0, 0);
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) Ls[R + kq + 4 * r4][C + l16] = acc[r4];
        }
        __syncthreads();
      }
    }
    if (wave == 0 && bad) fail = 1;
    // the rhs row leaves for the workspace; the tile itself keeps the factor only (identity beyond bw, zeros above the
    // diagonal - the trailing updates of the diagonal 16 x 16 tiles wrote there)
    if (has_rhs && t < bw) S[(int64_t)n * ld + c0 + t] = Ls[bw][t];
    __syncthreads();
    for (int i = t; i < CT * CT; i += 256) {
      const int r = i >> 6, c = i & 63;
      if (r >= bw || c > r) Ls[r][c] = c == r ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  for (int i = t; i < CT * CT; i += 256) {
    const int r = i >> 6, c = i & 63;
    if (r < bw && c <= r) S[(int64_t)(c0 + r) * ld + c0 + c] = Ls[r][c];
  }
  // ---- inverse of the factor tile.  (1) the four 16 x 16 diagonal blocks, one thread per column: forward substitution,
  //      column oriented - as soon as x[i] is known every later row's partial sum takes its term, so the dependent chain
  //      per step is one multiply and one fused multiply-add (a row-oriented sum is a chain of i of them)
  __syncthreads();  // (the tile store above read Ls; Li's first rows served as column buffers)
  if (t < 64) {
    const int b = t >> 4, cc = t & 15, o = 16 * b;
    double sv[16], x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) sv[i] = i == cc ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      x[i] = i >= cc ? sv[i] / Ls[o + i][o + i] : 0.0;
#pragma unroll
      for (int m = i + 1; m < 16; ++m) sv[m] = __builtin_fma(-Ls[o + m][o + i], x[i], sv[m]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) Li[o + i][o + cc] = x[i];
  }
  for (int i = t; i < CT * CT; i += 256) {  // zero the strictly upper part and the off-diagonal blocks (filled below)
    const int r = i >> 6, c = i & 63;
    if ((r >> 4) != (c >> 4)) Li[r][c] = 0.0;
  }
  __syncthreads();
  // (2) off-diagonal blocks by distance d = 1..3: Linv(i,j) = -Dinv_i * sum_{m=j}^{i-1} L(i,m) Linv(m,j), one wave per
  //     block, both products on the fp64 matrix cores (T travels through LDS between them: D layout -> B operand)
  __shared__ double Tm[3][16][17];
  {
    const int l16 = lane & 15, kq = lane >> 4;
    for (int d = 1; d < 4; ++d) {
      const int bj = wave, bi = bj + d;  // blocks (bi, bj), bj = 0 .. 3 - d
      if (bi < 4) {
        double4c acc = {0.0, 0.0, 0.0, 0.0};
        for (int m = bj; m < bi; ++m)
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ls[16 * bi + l16][16 * m + 4 * s4 + kq], Li[16 * m + 4 * s4 + kq][16 * bj + l16], acc, 0, 0, 0);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) Tm[bj][kq + 4 * r4][l16] = acc[r4];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double4c acc2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
          acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-Li[16 * bi + l16][16 * bi + 4 * s4 + kq], Tm[bj][4 * s4 + kq][l16], acc2, 0, 0, 0);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) Li[16 * bi + kq + 4 * r4][16 * bj + l16] = acc2[r4];
      }
      __syncthreads();
    }
  }
  double* Wk = w.Wi + (int64_t)k * CT * CT;
  for (int i = t; i < CT * CT; i += 256) Wk[i] = Li[i >> 6][i & 63];
  if (t == 0 && fail) w.info[INFO_TILED_FAIL] = 1;
}

// X = A L^-T for the tile rows below tile k; grid = tile rows (exits beyond the matrix)
__global__ __launch_bounds__(256) void chol_trsm_kernel(BAArgs a, int k) {
  int n;
  if (!chol_active(a, n)) return;
  const int c0 = CT * k, R0 = CT * (k + 1 + blockIdx.x);
  if (c0 >= n || R0 > n) return;
  const BAWs& w = a.w;
  const int ld = w.ld, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int bw = min(CT, n - c0), nr = min(CT, n + 1 - R0);  // rows R0 .. R0 + nr - 1 (row n = rhs)
  __shared__ double As[CT][CT + 2];  // pitch 66 doubles: the 16 x 4 operand fragments of a wave spread over all banks
  __shared__ double Ls[CT][CT + 2];
  const double* Wk = w.Wi + (int64_t)k * CT * CT;
  {
    // all 32 loads of a thread in flight before the first LDS store (a load -> store loop is one L2 round trip per
    // iteration: most of this kernel's 10 us)
    double va[16], vl[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = t + 256 * q, r = i >> 6, c = i & 63;
      va[q] = (r < nr && c < bw) ? w.S[(int64_t)(R0 + r) * ld + c0 + c] : 0.0;
      vl[q] = Wk[i];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = t + 256 * q, r = i >> 6, c = i & 63;
      As[r][c] = va[q];
      Ls[r][c] = vl[q];
    }
  }
  __syncthreads();
  // wave w: rows 16 w .. 16 w + 15; X[r][c] = sum_m A[r][m] Linv[c][m]
  const int l16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int tc = 0; tc < 4; ++tc) {
    double4c acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s4 = 0; s4 < 16; ++s4)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[16 * wave + l16][4 * s4 + kq], Ls[16 * tc + l16][4 * s4 + kq], acc, 0, 0, 0);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int rr = 16 * wave + kq + 4 * r4, cc = 16 * tc + l16;
      if (rr < nr && cc < bw) w.S[(int64_t)(R0 + rr) * ld + c0 + cc] = acc[r4];
    }
  }
}

// A_ij -= X_i X_j^T for all tile pairs k < j <= i; grid.x = pairs of the largest possible matrix (extra blocks exit)
__global__ __launch_bounds__(256) void chol_syrk_kernel(BAArgs a, int k) {
  int n;
  if (!chol_active(a, n)) return;
  const int c0 = CT * k;
  if (c0 >= n) return;
  int ti, tj;
  tri_index((int)blockIdx.x, ti, tj);
  const int Ri = CT * (k + 1 + ti), Rj = CT * (k + 1 + tj);
  if (Ri > n || Rj >= n) return;  // row tile must hold a row <= n, column tile a column < n
  const BAWs& w = a.w;
  const int ld = w.ld, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int bw = min(CT, n - c0), nri = min(CT, n + 1 - Ri), ncj = min(CT, n - Rj);
  __shared__ double Xi[CT][CT + 2];
  __shared__ double Xj[CT][CT + 2];
  const int l16 = lane & 15, kq = lane >> 4;
  // every load of the thread - the two operand tiles and the 16 entries of A_ij it will update - is in flight before
  // the first dependent instruction (load -> LDS store loops and the read-modify-write at the end were one L2 round
  // trip per iteration each)
  double aold[4][4];
  {
    double vi[16], vj[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = t + 256 * q, r = i >> 6, c = i & 63;
      vi[q] = (r < nri && c < bw) ? w.S[(int64_t)(Ri + r) * ld + c0 + c] : 0.0;
      vj[q] = (r < ncj && c < bw) ? w.S[(int64_t)(Rj + r) * ld + c0 + c] : 0.0;
    }
#pragma unroll
    for (int tc = 0; tc < 4; ++tc)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int rr = 16 * wave + kq + 4 * r4, cc = 16 * tc + l16;
        aold[tc][r4] = (rr < nri && cc < ncj && Rj + cc <= Ri + rr) ? w.S[(int64_t)(Ri + rr) * ld + Rj + cc] : 0.0;
      }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = t + 256 * q, r = i >> 6, c = i & 63;
      Xi[r][c] = vi[q];
      Xj[r][c] = vj[q];
    }
  }
  __syncthreads();
#pragma unroll
  for (int tc = 0; tc < 4; ++tc) {
    double4c acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s4 = 0; s4 < 16; ++s4)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Xi[16 * wave + l16][4 * s4 + kq], Xj[16 * tc + l16][4 * s4 + kq], acc, 0, 0, 0);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int rr = 16 * wave + kq + 4 * r4, cc = 16 * tc + l16;
      if (rr < nri && cc < ncj && Rj + cc <= Ri + rr) w.S[(int64_t)(Ri + rr) * ld + Rj + cc] = aold[tc][r4] - acc[r4];
    }
  }
}

__global__ __launch_bounds__(512) void chol_backsub_kernel(BAArgs a) {
  int n;
  if (!chol_active(a, n)) return;
  const BAWs& w = a.w;
  const int ld = w.ld, t = threadIdx.x, n_free = w.info[INFO_FREE_POSES];
  __shared__ double Li[2][CT][CT + 1];
  __shared__ double xk[CT];
  extern __shared__ __align__(16) double ys[];  // [n]: the running right-hand side stays in LDS
  for (int i = t; i < n; i += 512) ys[i] = w.S[(int64_t)n * ld + i];
  const int Tc = (n + CT - 1) / CT;
  auto load_tile = [&](int k, int b) {
    const double* Wk = w.Wi + (int64_t)k * CT * CT;
    double v[8];  // all eight loads in flight before the first LDS store
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = Wk[t + 512 * q];
#pragma unroll
    for (int q = 0; q < 8; ++q) Li[b][(t + 512 * q) >> 6][(t + 512 * q) & 63] = v[q];
  };
  load_tile(Tc - 1, (Tc - 1) & 1);
  __syncthreads();
  for (int k = Tc - 1; k >= 0; --k) {
    const int c0 = CT * k, bw = min(CT, n - c0), b = k & 1;
    // x = L^-T y: x[c] = sum_{m >= c} Linv[m][c] y[m]; 8 lanes per column, combined by DPP-free shuffles
    {
      const int c = t >> 3, part = t & 7;
      double sacc = 0.0;
      if (c < bw)
        for (int m = c + part; m < bw; m += 8) sacc = __builtin_fma(Li[b][m][c], ys[c0 + m], sacc);
      sacc += __shfl_xor(sacc, 1, 8);
      sacc += __shfl_xor(sacc, 2, 8);
      sacc += __shfl_xor(sacc, 4, 8);
      if (part == 0 && c < bw) xk[c] = sacc;
    }
    if (k > 0) load_tile(k - 1, b ^ 1);  // next tile's inverse: independent of x
    __syncthreads();
    if (t < bw) ys[c0 + t] = xk[t];
    for (int c = t; c < c0; c += 512) {  // y[c] -= sum_r L[c0 + r][c] x[r]
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      const double* col = w.S + (int64_t)c0 * ld + c;
      int r = 0;
      for (; r + 15 < bw; r += 16) {  // sixteen rows of the column in flight per pass (each is its own cache line)
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = col[(int64_t)(r + q) * ld];
#pragma unroll
        for (int q = 0; q < 16; q += 4) {
          s0 = __builtin_fma(v[q], xk[r + q], s0);
          s1 = __builtin_fma(v[q + 1], xk[r + q + 1], s1);
          s2 = __builtin_fma(v[q + 2], xk[r + q + 2], s2);
          s3 = __builtin_fma(v[q + 3], xk[r + q + 3], s3);
        }
      }
      for (; r < bw; ++r) s0 = __builtin_fma(col[(int64_t)r * ld], xk[r], s0);
      ys[c] -= (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
  }
  const bool bad = w.info[INFO_TILED_FAIL] != 0;
  if (t == 0) {
    if (bad) w.info[INFO_FAILURES] += 1;
    w.info[INFO_SOLVER] = SOLVER_GLOBAL;
  }
  for (int dd = t; dd < n; dd += 512) store_step(w, dd, ys[dd], bad);
  __syncthreads();
  apply_retraction(a, t, 512, n_free);
}

// host side: the launches of one tiled solve, sized for the largest system the workspace can hold (blocks beyond the
// actual n exit at once; n itself lives on the device)
inline void launch_tiled_cholesky(const BAArgs& a, hipStream_t s) {
  const int nmax = a.w.ld - 1;
  if (nmax <= CT_MIN_N || nmax > 8000) return;  // (the back substitution keeps the rhs, up to 8000 doubles, in LDS)
  const int T = (nmax + 1 + CT - 1) / CT;  // tile rows incl. the rhs row
  const int Tc = (nmax + CT - 1) / CT;
  for (int k = 0; k < Tc; ++k) {
    chol_potrf_kernel<<<1, 256, 0, s>>>(a, k);
    const int m = T - 1 - k;
    if (m > 0) {
      chol_trsm_kernel<<<m, 256, 0, s>>>(a, k);
      chol_syrk_kernel<<<m * (m + 1) / 2, 256, 0, s>>>(a, k);
    }
  }
  chol_backsub_kernel<<<1, 512, sizeof(double) * (size_t)(nmax + 8), s>>>(a);
}
