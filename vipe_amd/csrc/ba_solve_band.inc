// ------------------------------------------------------------------------------------------------ solve (LDS band)

// When the reduced system is banded (sliding-window / neighbourhood graphs: two poses couple only through a shared
// source frame) and its band fits the 160 KB of LDS, the whole factorisation runs out of LDS: every dependent step
// then costs an LDS round trip (~100 cycles) instead of an L2 round trip (~2000), which is what bounds this
// latency-critical kernel.  Storage: pose row r keeps columns [6 (r/6 - bandblk), 6 (r/6) + 5] at pitch WB + 1
// doubles (so the LDS address of (row j0 + 6 + i, column j0 + m) advances by a constant per block step and every
// thread's operand addresses are computed once); the dense tail rows (intrinsics, then the rhs) are kept full
// length.  Block size 6 = one pose.  Per block step: panel (one row per lane), barrier, trailing update (one
// (row, row) pair per lane, descriptors fixed over the steps) while lane 0 of wave 0 - whose wave owns the 21
// entries of the NEXT diagonal block - already factors that block (look-ahead), barrier.  The back substitution is
// run by wave 0 alone: 8 lanes per column, DPP reductions, the 6x6 triangular solve replicated in every lane with
// stored reciprocal pivots - no workgroup barrier and no division on the dependent chain.
// Takes the systems band_form (ba_route.cuh) gives it, in the form it names, and reports SOLVER_BAND in info[INFO_SOLVER].
//
// The pieces of a block step are written once, over one LDS band image (BandImage), and called by the one-chain body
// (one image) and the two-chain body (one image per chain).  The workgroup barriers are the bodies', not the pieces'.
// (BAND_T threads per image, BAND_UPT, band_npair and the LDS sizes of the carves: ba_route.cuh)

struct BandImage {
  double* L;      // band rows [npr][WBP]; the offsets below and in BandPairs count doubles from here
  int tl0, tp;    // dense tail rows (intrinsics rows, then the rhs row; two chains: the rhs row alone): the first at L + tl0, pitch tp
  double* y;      // the rhs row: forward-substituted by the factorisation (a tail row), solved in place by the back substitution
  double* rdall;  // 1 / L[r][r] of the pose rows
  double* blk;    // 6x7: the current diagonal factor block
  double* rd;     // its reciprocal pivots
  int* failp;     // set by a non-positive pivot
  int PB, WBP, KS, npr;  // 6 bandblk; row pitch PB + 7; 6 WBP = what one block step adds to a band offset; pose rows
};

__device__ __forceinline__ int band_ofs(const BandImage& b, int r, int c) { return r * b.WBP + c - 6 * (r / 6) + b.PB; }

// 6x6 diagonal block of pose kb: factor in registers, publish L (band), blk, rd, rdall
__device__ __forceinline__ void band_factor_diag(const BandImage& b, int kb) {
  const int j0 = 6 * kb, WBP = b.WBP;
  double* Dk = b.L + band_ofs(b, j0, j0);  // row i of the block at Dk + i * WBP
  double A[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) A[i][j] = Dk[i * WBP + j];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int m = 0; m < j; ++m) d = __builtin_fma(-(A[j][m]), A[j][m], d);
    if (!(d > 0.0)) { *b.failp = 1; d = 1.0; }
    const double rl = rsqrt_nr(d);
    A[j][j] = d * rl;
    b.rd[j] = rl;
    b.rdall[j0 + j] = rl;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double sacc = A[i][j];
#pragma unroll
      for (int m = 0; m < j; ++m) sacc = __builtin_fma(-(A[i][m]), A[j][m], sacc);
      A[i][j] = sacc * rl;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) { Dk[i * WBP + j] = A[i][j]; b.blk[i * 7 + j] = A[i][j]; }
}

// Band rows of S -> image, with LM damping on the diagonal (matrix.py:179-186).  One band row (WB <= 64 NC doubles,
// contiguous in S) per wave and iteration, CH rows per pass with every load of the pass - matrix entries AND the damping
// diagonal - issued from clamped addresses before the first use: as `load; if (diagonal) load Hd; store` the loop was one
// memory round trip per row (the second load depends on a branch on the first; stamps: 34.7k cycles to load the
// headline's two images).  NO per-entry index arithmetic: the row is wave-uniform, its block arithmetic runs on the scalar
// unit, and what depends on the lane is a constant of the lane (as per-entry divisions it was the loop's bulk: four waves
// per SIMD, 14k .. 38k cycles by wave in the stamps).
template <int CH, int NC>
__device__ __forceinline__ void band_load_rows(const BandImage& b, const BAArgs& a, int tl) {
  const BAWs& w = a.w;
  const double* S = w.S;
  const int ld = w.ld, PB = b.PB, WBP = b.WBP, WB = WBP - 1, npr = b.npr;
  const int wv = __builtin_amdgcn_readfirstlane(tl >> 6), ln = tl & 63;
  const bool dr = a.droid;
  for (int r0 = wv; r0 < npr; r0 += CH * (BAND_T / 64)) {
    double sv[CH][NC], hv[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int r = min(r0 + i * (BAND_T / 64), npr - 1), rb6 = 6 * (r / 6);
      hv[i] = dr ? 0.0 : w.Hd[r];
#pragma unroll
      for (int h = 0; h < NC; ++h) sv[i][h] = S[(int64_t)r * ld + min(max(rb6 - PB + ln + 64 * h, 0), r)];
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int r = r0 + i * (BAND_T / 64);
      if (r < npr) {
        const int rb6 = 6 * (r / 6), rm = r - rb6;
#pragma unroll
        for (int h = 0; h < NC; ++h) {
          const int l2 = ln + 64 * h;
          double v = (l2 < WB && rb6 + l2 >= PB && l2 <= rm + PB) ? sv[i][h] : 0.0;
          if (l2 == rm + PB) v = damped_diag(a, r, npr, v, hv[i]);
          if (l2 < WBP) b.L[r * WBP + l2] = v;
        }
      }
    }
  }
}

// Per-thread operand descriptors, fixed over the block steps: offset from L at step 0 + stride per step
template <int UPT>
struct BandPairs {
  // panel: thread pr < PB + ntail owns one row below the diagonal block
  int prow_off, prow_str, prow_ia;  // prow_ia >= 0: pose row offset (valid while 6 kb + 6 + ia < npr)
  bool has_prow;
  // update: pair index -> one (a, b) pair, b <= a (operands uA, uB, target uD): pose-pose, tail-pose, tail-tail
  int uA[UPT], uB[UPT], uD[UPT], sA[UPT], sB[UPT], sD[UPT], u_ia[UPT], u_ib[UPT];
  bool has_pair[UPT];
};

// tl: the thread's index in its image; ntail: tail rows (intrinsics rows + the rhs row)
template <int UPT>
__device__ __forceinline__ void band_pairs_setup(const BandImage& b, int tl, int ntail, BandPairs<UPT>& d) {
  const int PB = b.PB, WBP = b.WBP, KS = b.KS, F = ntail - 1;
  const int npp = PB * (PB + 1) / 2, ntp = ntail * PB, npair = band_npair(PB, ntail);
  d.prow_off = 0; d.prow_str = 0; d.prow_ia = -1;
  d.has_prow = tl < PB + ntail;
  if (d.has_prow) {
    if (tl < PB) { d.prow_ia = tl; d.prow_off = (6 + tl) * WBP - 6 - 6 * (tl / 6) + PB; d.prow_str = KS; }
    else { d.prow_off = b.tl0 + (tl - PB) * b.tp; d.prow_str = 6; }
  }
#pragma unroll
  for (int sl = 0; sl < UPT; ++sl) {
    // pairs 0..20 (the next diagonal block) are lanes 0..20 of wave 0 and nothing else runs there: that wave goes
    // straight on to factor the next block; the other pairs are spread over waves 1..7
    const int pid = tl < 64 ? (sl == 0 && tl < 21 ? tl : npair) : 21 + (tl - 64) + (BAND_T - 64) * sl;
    d.has_pair[sl] = pid < npair;
    d.uA[sl] = d.uB[sl] = d.uD[sl] = d.sA[sl] = d.sB[sl] = d.sD[sl] = 0;
    d.u_ia[sl] = d.u_ib[sl] = -1;
    if (!d.has_pair[sl]) continue;
    if (pid < npp) {
      int ia, ib;
      tri_index(pid, ia, ib);
      d.u_ia[sl] = ia; d.u_ib[sl] = ib;
      d.uA[sl] = (6 + ia) * WBP - 6 - 6 * (ia / 6) + PB; d.sA[sl] = KS;
      d.uB[sl] = (6 + ib) * WBP - 6 - 6 * (ib / 6) + PB; d.sB[sl] = KS;
      d.uD[sl] = (6 + ia) * WBP + ib - 6 * (ia / 6) + PB; d.sD[sl] = KS;
    } else if (pid < npp + ntp) {
      const int u = pid - npp, q = u / PB, ib = u % PB;
      d.u_ib[sl] = ib;
      d.uA[sl] = b.tl0 + q * b.tp; d.sA[sl] = 6;
      d.uB[sl] = (6 + ib) * WBP - 6 - 6 * (ib / 6) + PB; d.sB[sl] = KS;
      d.uD[sl] = b.tl0 + q * b.tp + 6 + ib; d.sD[sl] = 6;
    } else {
      // (q, q2), q2 <= q, q2 < ntail - 1 (the rhs row has no column): F = 1: (0,0) (1,0); F = 2: (0,0) (1,0) (1,1) (2,0) (2,1)
      const int v = pid - npp - ntp;
      int q, q2;
      if (F == 1) { q = v; q2 = 0; }
      else { q = v == 0 ? 0 : (v <= 2 ? 1 : 2); q2 = v == 0 ? 0 : (v <= 2 ? v - 1 : v - 3); }
      d.uA[sl] = b.tl0 + q * b.tp; d.sA[sl] = 6;
      d.uB[sl] = b.tl0 + q2 * b.tp; d.sB[sl] = 6;
      d.uD[sl] = b.tl0 + q * b.tp + b.npr + q2; d.sD[sl] = 0;
    }
  }
}

// One block step of an image (the barrier between and after the two halves is the caller's).
// panel: x = a Lkk^-T for every row below the block (pose rows inside the band, all tail rows)
template <int UPT>
__device__ __forceinline__ void band_panel(const BandImage& b, const BandPairs<UPT>& d, int kb) {
  const int j0 = 6 * kb;
  if (d.has_prow && (d.prow_ia < 0 || j0 + 6 + d.prow_ia < b.npr)) {
    double* row = b.L + d.prow_off + kb * d.prow_str;
    double x[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double sacc = row[j];
#pragma unroll
      for (int m = 0; m < j; ++m) sacc = __builtin_fma(-(x[m]), b.blk[j * 7 + m], sacc);
      x[j] = sacc * b.rd[j];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) row[j] = x[j];
  }
}

// trailing update, one (a, b) pair per thread and slot; then the look-ahead: the 21 entries of the next diagonal block
// are pairs 0..20, all in wave 0 of the image, whose lane 0 factors block kb + 1 (if there is one before kend)
template <int UPT>
__device__ __forceinline__ void band_trailing(const BandImage& b, const BandPairs<UPT>& d, int tl, int kb, int kend) {
  const int j0 = 6 * kb, npr = b.npr;
  double* const L = b.L;
#pragma unroll
  for (int sl = 0; sl < UPT; ++sl) {
    if (d.has_pair[sl] && (d.u_ia[sl] < 0 || j0 + 6 + d.u_ia[sl] < npr) && (d.u_ib[sl] < 0 || j0 + 6 + d.u_ib[sl] < npr)) {
      const double* pa = L + d.uA[sl] + kb * d.sA[sl];
      const double* pb = L + d.uB[sl] + kb * d.sB[sl];
      double sacc = 0.0;
#pragma unroll
      for (int m = 0; m < 6; ++m) sacc = __builtin_fma(pa[m], pb[m], sacc);
      L[d.uD[sl] + kb * d.sD[sl]] -= sacc;
    }
  }
  if (tl < 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (tl == 0 && kb + 1 < kend) band_factor_diag(b, kb + 1);
  }
}

// One block of the back substitution L^T x = y, run by wave 0 of the image (tl < 64).  Column-oriented: once x of block
// kb is known (6x6 triangular solve, replicated in every lane from broadcast LDS reads, reciprocal pivots - or `known`:
// already in y), lane c subtracts its contribution from y of band row 6 kb - PB + c (columns < colmax) right away, so no
// reduction and no cross-lane traffic sits on the dependent chain.  TWO: a second column per lane for bands wider than
// one wave (PB > 64).
template <bool TWO>
__device__ __forceinline__ void band_backsub_block(const BandImage& b, int tl, int kb, bool known, int colmax) {
  const int j0 = 6 * kb, PB = b.PB, WBP = b.WBP;
  double* const L = b.L;
  double* const y = b.y;
  const double* Dk = L + band_ofs(b, j0, j0);
  // operands that do not depend on the running y: block factor, reciprocal pivots, this lane's column of the
  // six block rows (entries L[j0 + j][6 kb - PB + tl])
  double Lk[6][6], rp[6], lc[6], lc2[6];
  const int rt = j0 - PB + tl, rt2 = rt + 64;
  const bool upd = tl < PB && rt >= 0 && rt < colmax;
  const bool upd2 = TWO && tl + 64 < PB && rt2 >= 0 && rt2 < colmax;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    rp[i] = b.rdall[j0 + i];
    lc[i] = upd ? L[(j0 + i) * WBP + tl] : 0.0;
    if constexpr (TWO) lc2[i] = upd2 ? L[(j0 + i) * WBP + tl + 64] : 0.0;
    else lc2[i] = 0.0;
#pragma unroll
    for (int j = 0; j < i; ++j) Lk[i][j] = Dk[i * WBP + j];
  }
  double x[6];
  if (known) {
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = y[j0 + j];
  } else {
#pragma unroll
    for (int j = 5; j >= 0; --j) {
      double sacc = y[j0 + j];
#pragma unroll
      for (int m = 5; m > j; --m) sacc = __builtin_fma(-(Lk[m][j]), x[m], sacc);
      x[j] = sacc * rp[j];
    }
    if (tl < 6) {
      double xo = x[0];
#pragma unroll
      for (int j = 1; j < 6; ++j) xo = tl == j ? x[j] : xo;
      y[j0 + tl] = xo;
    }
  }
  if (upd) {
    double sacc = lc[0] * x[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) sacc = __builtin_fma(lc[j], x[j], sacc);
    y[rt] -= sacc;
  }
  if (TWO && upd2) {
    double sacc = lc2[0] * x[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) sacc = __builtin_fma(lc2[j], x[j], sacc);
    y[rt2] -= sacc;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One chain.  UPT: trailing-update pair slots per thread, TWO: two band columns per lane (bands wider than one wave).
// Short neighbourhood graphs and those with intrinsics columns run the <2, false> instantiation (fewer slots to walk per
// step, one pipelined load pass); the frontend's dense windows the <BAND_UPT, true> one.
template <int UPT, bool TWO>
__device__ __forceinline__ void band_solve_body(const BAArgs& a, const RouteIn& r, unsigned char* smem_raw) {
  const int t = threadIdx.x;
  double* const L = reinterpret_cast<double*>(smem_raw);
  const BAWs& w = a.w;
  const int n = r.n, n_free = r.n_free, bandblk = r.bandblk;
  const int ld = w.ld;
  const int npr = 6 * n_free, ntail = n - npr + 1;  // tail rows: intrinsics rows, then the rhs row
  const int F = ntail - 1;
  const int PB = 6 * bandblk, WB = PB + 6, WBP = WB + 1;
  // band_form let the system in, so its limits hold; the optimiser does not see that through the form's value, and
  // this one shapes the tail loops below
  __builtin_assume(F <= LDS_TAIL_MAX);
  // LDS carve: band [npr][WBP], tail [ntail][n + 1], rdall [npr], blk[6][7], rd[6], flags (band_need doubles)
  const int TL0 = band_tail0(npr, WBP);
  const int RD0 = band_rd0(n, npr, ntail, WBP);
  double* const Tl = L + TL0;
  BandImage b;
  b.L = L; b.tl0 = TL0; b.tp = n + 1; b.y = Tl + F * (n + 1);
  b.rdall = L + RD0; b.blk = b.rdall + npr; b.rd = b.blk + 42;
  b.failp = reinterpret_cast<int*>(b.rd + 6);
  b.PB = PB; b.WBP = WBP; b.KS = 6 * WBP; b.npr = npr;
  const double* S = w.S;
  auto tref = [&](int q, int c) -> double& { return Tl[q * (n + 1) + c]; };

  // ---- load.  Sixteen rows per pass: a dozen row loads in flight per wave (unpipelined, the loop is one L2 round trip
  // per row)
  if (t == 0) *b.failp = 0;
  band_load_rows<16, TWO ? 2 : 1>(b, a, t);
  for (int idx = t; idx < ntail * (n + 1); idx += BAND_T) {
    const int q = idx / (n + 1), c = idx % (n + 1), r = npr + q;
    double v = 0.0;
    if (c <= r && c < n) {
      v = S[(int64_t)r * ld + c];
      if (c == r) v = damped_diag(a, r, npr, v, w.Hd[r]);
    }
    Tl[idx] = v;
  }
  BandPairs<UPT> d;
  band_pairs_setup(b, t, ntail, d);
  __syncthreads();
  if (t == 0 && n_free > 0) band_factor_diag(b, 0);
  __syncthreads();

  // ---- factorisation, one pose block (6 columns) per step
  for (int kb = 0; kb < n_free; ++kb) {
    band_panel(b, d, kb);
    __syncthreads();
    band_trailing(b, d, t, kb, n_free);
    __syncthreads();
  }
  // ---- tail columns (intrinsics unknowns), unblocked
  for (int f = 0; f < F; ++f) {
    const int cf = npr + f;
    if (t == 0) {
      double dg = tref(f, cf);
      if (!(dg > 0.0)) { *b.failp = 1; dg = 1.0; }
      const double rl = rsqrt_nr(dg);
      tref(f, cf) = dg * rl;
      for (int q = f + 1; q < ntail; ++q) tref(q, cf) *= rl;
      for (int q = f + 1; q < ntail; ++q)
        for (int q2 = f + 1; q2 <= q && q2 < ntail - 1; ++q2) tref(q, npr + q2) -= tref(q, cf) * tref(q2, cf);
    }
    __syncthreads();
  }
  // ---- back substitution L^T x = y; y = rhs row (tail row F), solved in place by wave 0
  double* const y = b.y;
  if (t < 64) {
    if (t == 0) {
      for (int f = F - 1; f >= 0; --f) {
        double sacc = y[npr + f];
        for (int q = f + 1; q < F; ++q) sacc -= tref(q, npr + f) * y[npr + q];
        y[npr + f] = sacc / tref(f, npr + f);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (F > 0) {
      for (int r = t; r < npr; r += 64) {
        double sacc = y[r];
        for (int f = 0; f < F; ++f) sacc -= tref(f, r) * y[npr + f];
        y[r] = sacc;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    for (int kb = n_free - 1; kb >= 0; --kb) band_backsub_block<TWO>(b, t, kb, false, npr);
  }
  __syncthreads();
  const bool bad = *b.failp != 0;
  if (t == 0) {
    if (bad) w.info[INFO_FAILURES] += 1;
    w.info[INFO_SOLVER] = SOLVER_BAND;
  }
  for (int dd = t; dd < n; dd += BAND_T) store_step(w, dd, y[dd], bad);
  __syncthreads();
  apply_retraction(a, t, BAND_T, n_free);
}

// Two-chain ("burn at both ends") form of the band solve for pose-only systems (no intrinsics columns): the sequential
// pivot chain, not arithmetic, bounds the kernel (47 dependent block steps at N = 48), and a block-banded SPD matrix can be
// eliminated from BOTH ends at once.  Blocks 0..a-1 (chain A, natural order) and blocks nb-1..a+bandblk (chain B,
// REVERSED order - the mirrored matrix is banded too, its lower triangle being the transposed upper one) are factorised
// concurrently by the two halves of the workgroup, each on its own LDS band image with the pieces above (one tail row =
// the right-hand side, two pair slots per thread, one band column per lane); the bandblk separator blocks in the middle
// are ordinary band rows at the end of both images, so both eliminations leave their Schur contributions in them.  Chain
// B's are then added to chain A's image, chain A factors the separator (bandblk more steps), and the back substitution
// runs separator first, then both chains at once.  Dependent block steps: max(a, b) + bandblk forward,
// bandblk + max(a, b) back, instead of nb + nb.
// The kernel is launched with 2 * BAND_T threads: BAND_T per chain; the one-chain forms use the first BAND_T.
__device__ __forceinline__ void band2_solve_body(const BAArgs& a, const RouteIn& r, unsigned char* smem_raw) {
  const BAWs& w = a.w;
  // image B's threads are rotated by one wave: its critical wave (tl < 64: diagonal pairs, look-ahead factor, back
  // substitution) is then hardware wave 9 - another SIMD than image A's wave 0 (waves go to SIMDs round robin); with both
  // chains' critical waves on one SIMD each ran at the pace of two
  const int t = threadIdx.x, g = t >= BAND_T ? 1 : 0, tl = g ? ((t - 64) & (BAND_T - 1)) : t;
  const int n = r.n, nb = r.n_free, bandblk = r.bandblk;
  const int ld = w.ld;
  const int PB = 6 * bandblk, WB = PB + 6, WBP = WB + 1;
  const int ca = (nb - bandblk) / 2, cb = nb - bandblk - ca;  // chain lengths in blocks (cb >= ca)
  const int nf = (g ? cb : ca) + bandblk, chain = g ? cb : ca;  // blocks of this image, of its chain
  const int npr = 6 * nf, nprmax = band2_rows_max(nb, bandblk);  // 6 (cb + bandblk)
  // LDS carve per image: band [nprmax][WBP], rhs row [nprmax + 1], rdall [nprmax], blk 42, rd 6; then one flag
  const int IMG = band2_image(nprmax, WBP);
  double* const LA = reinterpret_cast<double*>(smem_raw);
  double* const LB = LA + IMG;
  BandImage b;
  // tp = 0: with one tail row band_pairs_setup only ever forms q * tp with q == 0, and the constant folds those products
  // away.  A form with more tail rows per image has to set the real pitch (nprmax + 1) here.
  b.L = g ? LB : LA; b.tl0 = nprmax * WBP; b.tp = 0;
  b.y = b.L + nprmax * WBP;  // the image's right-hand side (the one tail row of the factorisation)
  b.rdall = b.y + nprmax + 1; b.blk = b.rdall + nprmax; b.rd = b.blk + 42;
  b.failp = reinterpret_cast<int*>(LA + 2 * IMG);
  b.PB = PB; b.WBP = WBP; b.KS = 6 * WBP; b.npr = npr;
  double* const L = b.L;
  double* const y = b.y;
  const double* S = w.S;
  auto gblk = [&](int l) { return g ? nb - 1 - l : l; };  // local block -> global block
  // @bstamp 0
  // @bwave 100
  if (t == 0) *b.failp = 0;

  // ---- load both images.  Image B: mirrored; its separator square and separator right-hand side start from zero (they
  // only collect chain B's contributions)
  {
    // Image A reads its band rows as they lie in S.  Image B is the MIRRORED matrix (its band row is a column of S): it
    // walks the rows of S as well, in the same passes, and scatters every entry to its mirrored position (zero-filled first).
    constexpr int CH = 20;  // the headline's images: 19 rows per wave, one pass = one memory round trip
    if (g)
      for (int idx = tl; idx < npr * WBP; idx += BAND_T) L[idx] = 0.0;
    __syncthreads();
    if (!g) {
      band_load_rows<CH, 1>(b, a, tl);
    } else {
      const int wv = __builtin_amdgcn_readfirstlane(tl >> 6), ln = tl & 63;
      const int lq = ln / 6, lm = ln - 6 * lq;
      const bool dr = a.droid;
      const int G0 = 6 * (nb - nf);  // first global row of image B's blocks
      // target offset of lane ln's entry of global row Cg (block bcl = nb - 1 - Cg / 6 locally, cm = Cg % 6):
      //   own block (ln >= PB): (6 bcl + cm) WBP + lm + PB - inside a diagonal block the mirrored matrix keeps the row /
      //   column order, so the entry goes to the transposed position; left of it: local row block bcl + bandblk - lq
      const bool own = ln >= PB;
      const int K1 = 6 * (bandblk - lq);
      const int lconst = own ? lm : (K1 + lm) * WBP - K1;
      for (int r0 = wv; r0 < npr; r0 += CH * (BAND_T / 64)) {
        double sv[CH], hv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int Cg = G0 + min(r0 + i * (BAND_T / 64), npr - 1), cb6 = 6 * (Cg / 6);
          sv[i] = S[(int64_t)Cg * ld + min(max(cb6 - PB + ln, G0), Cg)];
          hv[i] = dr ? 0.0 : w.Hd[Cg];
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int rr = r0 + i * (BAND_T / 64);
          const int Cg = G0 + rr, cq = Cg / 6, cb6 = 6 * cq, cm = Cg - cb6, bcl = nb - 1 - cq;
          // rows of the separator: their own square starts from zero (the zero fill), their chain columns are loaded
          if (rr < npr && ln < WB && cb6 - PB + ln >= G0 && ln <= cm + PB) {
            const bool sepsq = bcl >= chain && (own || bcl + bandblk - lq >= chain);
            const int A1 = 6 * bcl * WBP + PB;
            double v = sepsq ? 0.0 : sv[i];
            if (ln == cm + PB && !sepsq) v = damped_diag(a, rr, npr, v, hv[i]);  // every row of an image is a pose row
            L[(own ? A1 + cm * WBP : A1 + cm) + lconst] = v;
          }
        }
      }
    }
    // @bwave 120
    // @bstamp 8
    for (int c = tl; c <= npr; c += BAND_T) {
      double v = 0.0;
      if (c < npr && !(g && c / 6 >= chain)) v = S[(int64_t)n * ld + 6 * gblk(c / 6) + c % 6];
      y[c] = v;
    }
  }
  // @bstamp 9
  BandPairs<2> d;
  band_pairs_setup(b, tl, 1, d);
  // @bstamp 10
  // @bwave 140
  __syncthreads();
  // @bstamp 1
  if (tl == 0) band_factor_diag(b, 0);
  __syncthreads();
  // @bstamp 2
  // ---- both chains, one block per step
  for (int kb = 0; kb < cb; ++kb) {
    const bool mine = kb < chain;
    if (mine) band_panel(b, d, kb);
    __syncthreads();
    if (mine) band_trailing(b, d, tl, kb, chain);  // the look-ahead stops at the chain's end: the separator is not final yet
    __syncthreads();
  }
  // @bstamp 3
  // ---- chain B's contributions to the separator square and right-hand side go to image A (mirrored back)
  for (int idx = t; idx < PB * PB + PB; idx += 2 * BAND_T) {
    if (idx < PB * PB) {
      const int rB = idx / PB, cB = idx % PB;  // separator-local row / column in image B's order, rB >= cB
      if (rB >= cB) {
        const int sr = rB / 6, sc = cB / 6, i = rB % 6, j = cB % 6;
        const double v = LB[band_ofs(b, 6 * cb + rB, 6 * cb + cB)];
        const int br = bandblk - 1 - sr, bc = bandblk - 1 - sc;  // separator blocks in image A's order (br <= bc)
        if (sr == sc) LA[band_ofs(b, 6 * (ca + br) + i, 6 * (ca + br) + j)] += v;
        else LA[band_ofs(b, 6 * (ca + bc) + j, 6 * (ca + br) + i)] += v;  // the transposed position
      }
    } else {
      const int q = idx - PB * PB, sq = q / 6, i = q % 6;
      LA[nprmax * WBP + 6 * (ca + bandblk - 1 - sq) + i] += LB[nprmax * WBP + 6 * cb + q];
    }
  }
  __syncthreads();
  // ---- chain A goes on through the separator
  if (g == 0 && tl == 0) band_factor_diag(b, ca);
  __syncthreads();
  for (int kb = ca; kb < ca + bandblk; ++kb) {
    if (g == 0) band_panel(b, d, kb);
    __syncthreads();
    if (g == 0) band_trailing(b, d, tl, kb, ca + bandblk);
    __syncthreads();
  }
  // @bstamp 4
  // ---- back substitution (one wave per image): separator first (image A) ...
  if (g == 0 && tl < 64)
    for (int kb = ca + bandblk - 1; kb >= ca; --kb) band_backsub_block<false>(b, tl, kb, false, npr);
  __syncthreads();
  // @bstamp 5
  if (t < PB) LB[nprmax * WBP + 6 * (cb + bandblk - 1 - t / 6) + t % 6] = LA[nprmax * WBP + 6 * ca + t];  // x of the separator, mirrored
  __syncthreads();
  // ... then both chains at once; in image B the separator rows only hand their (known) x down to the chain's columns
  if (tl < 64) {
    if (g)
      for (int kb = cb + bandblk - 1; kb >= cb; --kb) band_backsub_block<false>(b, tl, kb, true, 6 * cb);
    for (int kb = chain - 1; kb >= 0; --kb) band_backsub_block<false>(b, tl, kb, false, npr);
  }
  __syncthreads();
  // @bstamp 6
  const bool bad = *b.failp != 0;
  if (t == 0) {
    if (bad) w.info[INFO_FAILURES] += 1;
    w.info[INFO_SOLVER] = SOLVER_BAND;
  }
  // image A: chain + separator, image B: its chain
  for (int r = tl; r < (g ? 6 * cb : npr); r += BAND_T) store_step(w, 6 * gblk(r / 6) + r % 6, y[r], bad);
  __syncthreads();
  apply_retraction(a, t, 2 * BAND_T, nb);
  // @bstamp 7
}

__global__ __launch_bounds__(2 * BAND_T) void ba_solve_band_kernel(BAArgs a, int lds_doubles) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  // a uniform decision made before any barrier (the caller's VIPE_BA_OPT_ONE_CHAIN keeps the one-chain forms for A/B -
  // BAArgs::band2)
  const RouteIn r = route_in(a, lds_doubles);
  const int form = band_form(r);
  if (form == BAND_TWO_CHAIN) { band2_solve_body(a, r, smem_raw); return; }
  if (form == BAND_DECLINES || threadIdx.x >= BAND_T) return;  // the one-chain forms are written for BAND_T threads
  if (form == BAND_WIDE) band_solve_body<BAND_UPT, true>(a, r, smem_raw);
  else band_solve_body<2, false>(a, r, smem_raw);
}
