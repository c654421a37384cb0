// ------------------------------------------------------------------------------------------------ solve (LDS band)

// Retraction shared by both solve kernels: poses X <- Exp(dx) X (retractor.py:27-29), intrinsics (retractor.py:50-62)
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
// Sets info[5] = 1 when it solved the system (the global-memory kernel launched after it then exits).
constexpr int BAND_T = 512;
constexpr int BAND_UPT = 6;  // trailing-update pairs per thread: dense 12-pose windows (PB = 66: 2277 pairs) still fit

#define VIPE_DPP_F64(v, ctrl)                                                                                    \
  __builtin_bit_cast(double, ((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(                         \
                                  0, (int)(__builtin_bit_cast(unsigned long long, v) >> 32), ctrl, 0xf, 0xf, true) \
                              << 32) |                                                                           \
                                 (unsigned)__builtin_amdgcn_update_dpp(                                          \
                                     0, (int)__builtin_bit_cast(unsigned long long, v), ctrl, 0xf, 0xf, true))

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)u, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// UPT_: trailing-update pair slots per thread, TWO: two band columns per lane (bands wider than one wave).  The
// neighbourhood graphs of the headline configuration run the <2, false> instantiation (fewer slots to walk per step, one
// pipelined load pass); the frontend's dense windows the <BAND_UPT, true> one.
template <int UPT_, bool TWO>
__device__ __forceinline__ void band_solve_body(const BAArgs& a, int lds_doubles, unsigned char* smem_raw) {
  const int t = threadIdx.x;
  double* const L = reinterpret_cast<double*>(smem_raw);
  const vipe_ba_params& prm = a.p;
  const BAWs& w = a.w;
  const int n = w.info[3], n_free = w.info[0], bandblk = w.info[4];
  const int ld = w.ld;
  const int npr = 6 * n_free, ntail = n - npr + 1;  // tail rows: intrinsics rows, then the rhs row
  const int F = ntail - 1;
  const int PB = 6 * bandblk, WB = PB + 6, WBP = WB + 1, KS = 6 * WBP;
  const int npp = PB * (PB + 1) / 2, ntp = ntail * PB, ntt = F == 0 ? 0 : (F == 1 ? 2 : 5);
  const int npair = npp + ntp + ntt;
  // LDS carve: band [npr][WBP], tail [ntail][n + 1], rdall [npr], blk[6][7], rd[6], flags
  const int TL0 = npr * WBP;
  const int RD0 = TL0 + ntail * (n + 1);
  const int need = RD0 + npr + 64;
  if (t == 0) w.info[5] = 0;
  if (n == 0 || need > lds_doubles || npair > 21 + UPT_ * (BAND_T - 64) || PB + ntail > BAND_T || WBP > (TWO ? 128 : 64) || F > 2) {
    return;
  }
  double* const Tl = L + TL0;
  double* const rdall = L + RD0;          // 1 / L[r][r] of the pose rows
  double* const blk = rdall + npr;        // 6x7: the current diagonal factor block
  double* const rd = blk + 42;            // its reciprocal pivots
  int* const failp = reinterpret_cast<int*>(rd + 6);
  const double* S = w.S;
  auto bofs = [&](int r, int c) { return r * WBP + c - 6 * (r / 6) + PB; };
  auto tref = [&](int q, int c) -> double& { return Tl[q * (n + 1) + c]; };

  // ---- load (with LM damping on the diagonal, matrix.py:179-186)
  if (t == 0) *failp = 0;
  {
    // one band row (WB <= 64 doubles, contiguous in S) per wave and iteration; unrolled so that a dozen row loads are
    // in flight per wave (the loop is otherwise one L2 round trip per row)
    // Sixteen rows per pass with every load of the pass - matrix entries AND the damping diagonal - issued from clamped
    // addresses before the first use: as `load; if (diagonal) load Hd; store` the loop was one memory round trip per row
    // (the second load depends on a branch on the first; stamps: 34.7k cycles to load the headline's two images).
    // The row is wave-uniform: its block arithmetic runs on the scalar unit (as per-entry divisions it was the loop's bulk).
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
    constexpr int CH = 16, NC = TWO ? 2 : 1;
    const bool dr = a.droid;
    const double dep = (double)prm.pose_ep, ddm = (double)prm.pose_damping;
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
            if (l2 == rm + PB) v += dep + ddm * (dr ? v : hv[i]);  // DROID: geom_kernels.cu:1176
            if (l2 < WBP) L[r * WBP + l2] = v;
          }
        }
      }
    }
  }
  for (int idx = t; idx < ntail * (n + 1); idx += BAND_T) {
    const int q = idx / (n + 1), c = idx % (n + 1), r = npr + q;
    double v = 0.0;
    if (c <= r && c < n) {
      v = S[(int64_t)r * ld + c];
      if (c == r) v += 1e-6 + 1e-6 * w.Hd[r];
    }
    Tl[idx] = v;
  }

  // ---- per-thread operand descriptors, fixed over the block steps (offsets in doubles from L at step 0 + stride)
  // panel: thread pr < PB + ntail owns one row below the diagonal block
  int prow_off = 0, prow_str = 0, prow_ia = -1;  // prow_ia >= 0: pose row offset (valid while 6 kb + 6 + ia < npr)
  const bool has_prow = t < PB + ntail;
  if (has_prow) {
    if (t < PB) { prow_ia = t; prow_off = (6 + t) * WBP - 6 - 6 * (t / 6) + PB; prow_str = KS; }
    else { prow_off = TL0 + (t - PB) * (n + 1); prow_str = 6; }
  }
  // update: pair index t + BAND_T * slot (slot < UPT) -> one (a, b) pair, b <= a: pose-pose, tail-pose, tail-tail
  constexpr int UPT = UPT_;
  int uA[UPT], uB[UPT], uD[UPT], sA[UPT], sB[UPT], sD[UPT], u_ia[UPT], u_ib[UPT];
  bool has_pair[UPT];
#pragma unroll
  for (int sl = 0; sl < UPT; ++sl) {
    // pairs 0..20 (the next diagonal block) are lanes 0..20 of wave 0 and nothing else runs there: that wave goes
    // straight on to factor the next block; the other pairs are spread over waves 1..7
    const int pid = t < 64 ? (sl == 0 && t < 21 ? t : npair) : 21 + (t - 64) + (BAND_T - 64) * sl;
    has_pair[sl] = pid < npair;
    uA[sl] = uB[sl] = uD[sl] = sA[sl] = sB[sl] = sD[sl] = 0;
    u_ia[sl] = u_ib[sl] = -1;
    if (!has_pair[sl]) continue;
    if (pid < npp) {
      int ia = (int)((sqrtf(8.0f * (float)pid + 1.0f) - 1.0f) * 0.5f);
      while ((ia + 1) * (ia + 2) / 2 <= pid) ++ia;
      while (ia * (ia + 1) / 2 > pid) --ia;
      const int ib = pid - ia * (ia + 1) / 2;
      u_ia[sl] = ia; u_ib[sl] = ib;
      uA[sl] = (6 + ia) * WBP - 6 - 6 * (ia / 6) + PB; sA[sl] = KS;
      uB[sl] = (6 + ib) * WBP - 6 - 6 * (ib / 6) + PB; sB[sl] = KS;
      uD[sl] = (6 + ia) * WBP + ib - 6 * (ia / 6) + PB; sD[sl] = KS;
    } else if (pid < npp + ntp) {
      const int u = pid - npp, q = u / PB, ib = u % PB;
      u_ib[sl] = ib;
      uA[sl] = TL0 + q * (n + 1); sA[sl] = 6;
      uB[sl] = (6 + ib) * WBP - 6 - 6 * (ib / 6) + PB; sB[sl] = KS;
      uD[sl] = TL0 + q * (n + 1) + 6 + ib; sD[sl] = 6;
    } else {
      // (q, q2), q2 <= q, q2 < ntail - 1 (the rhs row has no column): F = 1: (0,0) (1,0); F = 2: (0,0) (1,0) (1,1) (2,0) (2,1)
      const int v = pid - npp - ntp;
      int q, q2;
      if (F == 1) { q = v; q2 = 0; }
      else { q = v == 0 ? 0 : (v <= 2 ? 1 : 2); q2 = v == 0 ? 0 : (v <= 2 ? v - 1 : v - 3); }
      uA[sl] = TL0 + q * (n + 1); sA[sl] = 6;
      uB[sl] = TL0 + q2 * (n + 1); sB[sl] = 6;
      uD[sl] = TL0 + q * (n + 1) + npr + q2; sD[sl] = 0;
    }
  }
  // 6x6 diagonal block of pose kb: factor in registers, publish L (band), blk, rd, rdall
  auto factor_diag = [&](int kb) {
    const int j0 = 6 * kb;
    double* Dk = L + bofs(j0, j0);  // row i of the block at Dk + i * WBP
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
      if (!(d > 0.0)) { *failp = 1; d = 1.0; }
      const double rl = rsqrt_nr(d);
      A[j][j] = d * rl;
      rd[j] = rl;
      rdall[j0 + j] = rl;
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
      for (int j = 0; j <= i; ++j) { Dk[i * WBP + j] = A[i][j]; blk[i * 7 + j] = A[i][j]; }
  };
  __syncthreads();
  if (t == 0 && n_free > 0) factor_diag(0);
  __syncthreads();

  // ---- factorisation, one pose block (6 columns) per step
  for (int kb = 0; kb < n_free; ++kb) {
    const int j0 = 6 * kb;
    // panel: x = a Lkk^-T for every row below the block (pose rows inside the band, all tail rows)
    if (has_prow && (prow_ia < 0 || j0 + 6 + prow_ia < npr)) {
      double* row = L + prow_off + kb * prow_str;
      double x[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double sacc = row[j];
#pragma unroll
        for (int m = 0; m < j; ++m) sacc = __builtin_fma(-(x[m]), blk[j * 7 + m], sacc);
        x[j] = sacc * rd[j];
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) row[j] = x[j];
    }
    __syncthreads();
    // trailing update, one (a, b) pair per thread
#pragma unroll
    for (int sl = 0; sl < UPT; ++sl) {
      if (has_pair[sl] && (u_ia[sl] < 0 || j0 + 6 + u_ia[sl] < npr) && (u_ib[sl] < 0 || j0 + 6 + u_ib[sl] < npr)) {
        const double* pa = L + uA[sl] + kb * sA[sl];
        const double* pb = L + uB[sl] + kb * sB[sl];
        double sacc = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) sacc = __builtin_fma(pa[m], pb[m], sacc);
        L[uD[sl] + kb * sD[sl]] -= sacc;
      }
    }
    // look-ahead: the 21 entries of the next diagonal block are pairs 0..20, all in wave 0
    if (t < 64) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (t == 0 && kb + 1 < n_free) factor_diag(kb + 1);
    }
    __syncthreads();
  }
  // ---- tail columns (intrinsics unknowns), unblocked
  for (int f = 0; f < F; ++f) {
    const int cf = npr + f;
    if (t == 0) {
      double d = tref(f, cf);
      if (!(d > 0.0)) { *failp = 1; d = 1.0; }
      const double rl = rsqrt_nr(d);
      tref(f, cf) = d * rl;
      for (int q = f + 1; q < ntail; ++q) tref(q, cf) *= rl;
      for (int q = f + 1; q < ntail; ++q)
        for (int q2 = f + 1; q2 <= q && q2 < ntail - 1; ++q2) tref(q, npr + q2) -= tref(q, cf) * tref(q2, cf);
    }
    __syncthreads();
  }
  // ---- back substitution L^T x = y; y = rhs row (tail row F), solved in place by wave 0
  double* y = &tref(F, 0);
  if (t < 64) {
    // column-oriented: once x of block kb is known (6x6 triangular solve, replicated in every lane from broadcast
    // LDS reads, reciprocal pivots), lane c subtracts its contribution from y of band row 6 kb - PB + c right away,
    // so no reduction and no cross-lane traffic sits on the dependent chain
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
    for (int kb = n_free - 1; kb >= 0; --kb) {
      const int j0 = 6 * kb;
      const double* Dk = L + bofs(j0, j0);
      // operands that do not depend on the running y: block factor, reciprocal pivots, this lane's column of the
      // six block rows (entries L[j0 + j][6 kb - PB + t])
      double Lk[6][6], rp[6], lc[6], lc2[6];
      const int rt = j0 - PB + t, rt2 = rt + 64;  // second column for bands wider than one wave (PB > 64)
      const bool upd = t < PB && rt >= 0;
      const bool upd2 = TWO && t + 64 < PB && rt2 >= 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        rp[i] = rdall[j0 + i];
        lc[i] = upd ? L[(j0 + i) * WBP + t] : 0.0;
        if constexpr (TWO) lc2[i] = upd2 ? L[(j0 + i) * WBP + t + 64] : 0.0;
        else lc2[i] = 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) Lk[i][j] = Dk[i * WBP + j];
      }
      double x[6];
#pragma unroll
      for (int j = 5; j >= 0; --j) {
        double sacc = y[j0 + j];
#pragma unroll
        for (int m = 5; m > j; --m) sacc = __builtin_fma(-(Lk[m][j]), x[m], sacc);
        x[j] = sacc * rp[j];
      }
      if (t < 6) {
        double xo = x[0];
#pragma unroll
        for (int j = 1; j < 6; ++j) xo = t == j ? x[j] : xo;
        y[j0 + t] = xo;
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
  }
  __syncthreads();
  const bool bad = *failp != 0;
  if (t == 0) {
    if (bad) w.info[2] += 1;
    w.info[5] = 1;
  }
  for (int dd = t; dd < n; dd += BAND_T) {
    double x = y[dd];
    if (bad || !(x == x)) x = 0.0;
    w.dx[dd] = (float)x;
  }
  __syncthreads();
  apply_retraction(a, t, BAND_T, n_free);
}

// Two-chain ("burn at both ends") form of the band solve for pose-only systems (no intrinsics columns): the sequential
// pivot chain, not arithmetic, bounds the kernel (47 dependent block steps at N = 48), and a block-banded SPD matrix can be
// eliminated from BOTH ends at once.  Blocks 0..a-1 (chain A, natural order) and blocks nb-1..a+bandblk (chain B,
// REVERSED order - the mirrored matrix is banded too, its lower triangle being the transposed upper one) are factorised
// concurrently by the two halves of the workgroup, each on its own LDS band image with the same code as above; the
// bandblk separator blocks in the middle are ordinary band rows at the end of both images, so both eliminations leave
// their Schur contributions in them.  Chain B's are then added to chain A's image, chain A factors the separator (bandblk
// more steps), and the back substitution runs separator first, then both chains at once.  Dependent block steps:
// max(a, b) + bandblk forward, bandblk + max(a, b) back, instead of nb + nb.
constexpr int B2_T = BAND_T;  // threads per chain: the kernel is launched with 2 * BAND_T threads, the one-chain forms use the first BAND_T

__device__ __forceinline__ bool band2_solve_body(const BAArgs& a, int lds_doubles, unsigned char* smem_raw) {
  const vipe_ba_params& prm = a.p;
  const BAWs& w = a.w;
  // image B's threads are rotated by one wave: its critical wave (tl < 64: diagonal pairs, look-ahead factor, back
  // substitution) is then hardware wave 9 - another SIMD than image A's wave 0 (waves go to SIMDs round robin); with both
  // chains' critical waves on one SIMD each ran at the pace of two
  const int t = threadIdx.x, g = t >= B2_T ? 1 : 0, tl = g ? ((t - 64) & (B2_T - 1)) : t;
  const int n = w.info[3], nb = w.info[0], bandblk = w.info[4];
  const int ld = w.ld;
  if (n != 6 * nb || bandblk < 1 || nb < 4 * bandblk + 4) return false;
  const int PB = 6 * bandblk, WB = PB + 6, WBP = WB + 1, KS = 6 * WBP;
  if (PB + 7 > 64) return false;
  const int ca = (nb - bandblk) / 2, cb = nb - bandblk - ca;  // chain lengths in blocks (cb >= ca)
  const int nf = (g ? cb : ca) + bandblk, chain = g ? cb : ca;  // blocks of this image, of its chain
  const int nfmax = cb + bandblk;
  const int npr = 6 * nf, nprmax = 6 * nfmax;
  const int npp = PB * (PB + 1) / 2, npair = npp + PB;
  if (npair > 21 + 2 * (B2_T - 64)) return false;
  // LDS carve per image: band [nprmax][WBP], rhs row [nprmax + 1], rdall [nprmax], blk 42, rd 6; then one flag
  const int IMG = nprmax * WBP + (nprmax + 1) + nprmax + 48;
  if (2 * IMG + 8 > lds_doubles) return false;
  double* const L = reinterpret_cast<double*>(smem_raw) + g * IMG;
  double* const y = L + nprmax * WBP;  // the image's right-hand side (a tail row of the factorisation)
  double* const rdall = y + nprmax + 1;
  double* const blk = rdall + nprmax;
  double* const rd = blk + 42;
  int* const failp = reinterpret_cast<int*>(reinterpret_cast<double*>(smem_raw) + 2 * IMG);
  double* const LA = reinterpret_cast<double*>(smem_raw);
  double* const LB = LA + IMG;
  const double* S = w.S;
  auto gblk = [&](int l) { return g ? nb - 1 - l : l; };  // local block -> global block
  // @bstamp 0
  // @bwave 100
  if (t == 0) { *failp = 0; w.info[5] = 0; }

  // ---- load both images (LM damping on the diagonal, matrix.py:179-186).  Image B: mirrored; its separator square and
  // separator right-hand side start from zero (they only collect chain B's contributions)
  {
    // Sixteen rows per pass, every load of the pass in flight before the first use (see band_solve_body), and NO per-entry
    // index arithmetic: the row is wave-uniform (scalar unit), what depends on the lane is a constant of the lane.  The
    // first form of this loop spent its time issuing integer divisions - four waves per SIMD, 14k .. 38k cycles by wave
    // (stamps).  Image A reads its band rows as they lie in S.  Image B is the MIRRORED matrix (its band row is a column
    // of S): it walks the rows of S as well and scatters every entry to its mirrored position (zero-filled first).
    const int wv = __builtin_amdgcn_readfirstlane(tl >> 6), ln = tl & 63;
    const int lq = ln / 6, lm = ln - 6 * lq;
    constexpr int CH = 20;  // the headline's images: 19 rows per wave, one pass = one memory round trip
    const bool dr = a.droid;
    const double dep = (double)prm.pose_ep, ddm = (double)prm.pose_damping;
    if (g)
      for (int idx = tl; idx < npr * WBP; idx += B2_T) L[idx] = 0.0;
    __syncthreads();
    if (!g) {
      for (int r0 = wv; r0 < npr; r0 += CH * (B2_T / 64)) {
        double sv[CH], hv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int r = min(r0 + i * (B2_T / 64), npr - 1), rb6 = 6 * (r / 6);
          sv[i] = S[(int64_t)r * ld + min(max(rb6 - PB + ln, 0), r)];
          hv[i] = dr ? 0.0 : w.Hd[r];
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int r = r0 + i * (B2_T / 64);
          if (r < npr) {
            const int rb6 = 6 * (r / 6), rm = r - rb6;
            double v = (ln < WB && rb6 + ln >= PB && ln <= rm + PB) ? sv[i] : 0.0;
            if (ln == rm + PB) v += dep + ddm * (dr ? v : hv[i]);
            if (ln < WBP) L[r * WBP + ln] = v;
          }
        }
      }
    } else {
      const int G0 = 6 * (nb - nf);  // first global row of image B's blocks
      // target offset of lane ln's entry of global row Cg (block bcl = nb - 1 - Cg / 6 locally, cm = Cg % 6):
      //   own block (ln >= PB): (6 bcl + cm) WBP + lm + PB - inside a diagonal block the mirrored matrix keeps the row /
      //   column order, so the entry goes to the transposed position; left of it: local row block bcl + bandblk - lq
      const bool own = ln >= PB;
      const int K1 = 6 * (bandblk - lq);
      const int lconst = own ? lm : (K1 + lm) * WBP - K1;
      for (int r0 = wv; r0 < npr; r0 += CH * (B2_T / 64)) {
        double sv[CH], hv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int Cg = G0 + min(r0 + i * (B2_T / 64), npr - 1), cb6 = 6 * (Cg / 6);
          sv[i] = S[(int64_t)Cg * ld + min(max(cb6 - PB + ln, G0), Cg)];
          hv[i] = dr ? 0.0 : w.Hd[Cg];
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int rr = r0 + i * (B2_T / 64);
          const int Cg = G0 + rr, cq = Cg / 6, cb6 = 6 * cq, cm = Cg - cb6, bcl = nb - 1 - cq;
          // rows of the separator: their own square starts from zero (the zero fill), their chain columns are loaded
          if (rr < npr && ln < WB && cb6 - PB + ln >= G0 && ln <= cm + PB) {
            const bool sepsq = bcl >= chain && (own || bcl + bandblk - lq >= chain);
            const int A1 = 6 * bcl * WBP + PB;
            double v = sepsq ? 0.0 : sv[i];
            if (ln == cm + PB && !sepsq) v += dep + ddm * (dr ? v : hv[i]);
            L[(own ? A1 + cm * WBP : A1 + cm) + lconst] = v;
          }
        }
      }
    }
    // @bwave 120
    // @bstamp 8
    for (int c = tl; c <= npr; c += B2_T) {
      double v = 0.0;
      if (c < npr && !(g && c / 6 >= chain)) v = S[(int64_t)n * ld + 6 * gblk(c / 6) + c % 6];
      y[c] = v;
    }
  }
  // @bstamp 9
  // ---- per-thread operand descriptors (as in band_solve_body, one tail row = the right-hand side)
  int prow_off = 0, prow_str = 0, prow_ia = -1;
  const bool has_prow = tl < PB + 1;
  if (has_prow) {
    if (tl < PB) { prow_ia = tl; prow_off = (6 + tl) * WBP - 6 - 6 * (tl / 6) + PB; prow_str = KS; }
    else { prow_off = nprmax * WBP; prow_str = 6; }
  }
  constexpr int UPT = 2;
  int uA[UPT], uB[UPT], uD[UPT], sA[UPT], sB[UPT], sD[UPT], u_ia[UPT], u_ib[UPT];
  bool has_pair[UPT];
#pragma unroll
  for (int sl = 0; sl < UPT; ++sl) {
    const int pid = tl < 64 ? (sl == 0 && tl < 21 ? tl : npair) : 21 + (tl - 64) + (B2_T - 64) * sl;
    has_pair[sl] = pid < npair;
    uA[sl] = uB[sl] = uD[sl] = sA[sl] = sB[sl] = sD[sl] = 0;
    u_ia[sl] = u_ib[sl] = -1;
    if (!has_pair[sl]) continue;
    if (pid < npp) {
      int ia = (int)((sqrtf(8.0f * (float)pid + 1.0f) - 1.0f) * 0.5f);
      while ((ia + 1) * (ia + 2) / 2 <= pid) ++ia;
      while (ia * (ia + 1) / 2 > pid) --ia;
      const int ib = pid - ia * (ia + 1) / 2;
      u_ia[sl] = ia; u_ib[sl] = ib;
      uA[sl] = (6 + ia) * WBP - 6 - 6 * (ia / 6) + PB; sA[sl] = KS;
      uB[sl] = (6 + ib) * WBP - 6 - 6 * (ib / 6) + PB; sB[sl] = KS;
      uD[sl] = (6 + ia) * WBP + ib - 6 * (ia / 6) + PB; sD[sl] = KS;
    } else {
      const int ib = pid - npp;
      u_ib[sl] = ib;
      uA[sl] = nprmax * WBP; sA[sl] = 6;
      uB[sl] = (6 + ib) * WBP - 6 - 6 * (ib / 6) + PB; sB[sl] = KS;
      uD[sl] = nprmax * WBP + 6 + ib; sD[sl] = 6;
    }
  }
  // @bstamp 10
  // @bwave 140
  auto bofs = [&](int r, int c) { return r * WBP + c - 6 * (r / 6) + PB; };
  auto factor_diag = [&](int kb) {
    const int j0 = 6 * kb;
    double* Dk = L + bofs(j0, j0);
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
      if (!(d > 0.0)) { *failp = 1; d = 1.0; }
      const double rl = rsqrt_nr(d);
      A[j][j] = d * rl;
      rd[j] = rl;
      rdall[j0 + j] = rl;
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
      for (int j = 0; j <= i; ++j) { Dk[i * WBP + j] = A[i][j]; blk[i * 7 + j] = A[i][j]; }
  };
  // one block step of this image (the barriers are the caller's): panel, then trailing update + look-ahead
  auto panel = [&](int kb) {
    const int j0 = 6 * kb;
    if (has_prow && (prow_ia < 0 || j0 + 6 + prow_ia < npr)) {
      double* row = L + prow_off + kb * prow_str;
      double x[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double sacc = row[j];
#pragma unroll
        for (int m = 0; m < j; ++m) sacc = __builtin_fma(-(x[m]), blk[j * 7 + m], sacc);
        x[j] = sacc * rd[j];
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) row[j] = x[j];
    }
  };
  auto trailing = [&](int kb, int kend) {
    const int j0 = 6 * kb;
#pragma unroll
    for (int sl = 0; sl < UPT; ++sl) {
      if (has_pair[sl] && (u_ia[sl] < 0 || j0 + 6 + u_ia[sl] < npr) && (u_ib[sl] < 0 || j0 + 6 + u_ib[sl] < npr)) {
        const double* pa = L + uA[sl] + kb * sA[sl];
        const double* pb = L + uB[sl] + kb * sB[sl];
        double sacc = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) sacc = __builtin_fma(pa[m], pb[m], sacc);
        L[uD[sl] + kb * sD[sl]] -= sacc;
      }
    }
    if (tl < 64) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (tl == 0 && kb + 1 < kend) factor_diag(kb + 1);
    }
  };
  __syncthreads();
  // @bstamp 1
  if (tl == 0) factor_diag(0);
  __syncthreads();
  // @bstamp 2
  // ---- both chains, one block per step
  for (int kb = 0; kb < cb; ++kb) {
    const bool mine = kb < chain;
    if (mine) panel(kb);
    __syncthreads();
    if (mine) trailing(kb, chain);  // the look-ahead stops at the chain's end: the separator is not final yet
    __syncthreads();
  }
  // @bstamp 3
  // ---- chain B's contributions to the separator square and right-hand side go to image A (mirrored back)
  for (int idx = t; idx < PB * PB + PB; idx += 2 * B2_T) {
    if (idx < PB * PB) {
      const int rB = idx / PB, cB = idx % PB;  // separator-local row / column in image B's order, rB >= cB
      if (rB >= cB) {
        const int sr = rB / 6, sc = cB / 6, i = rB % 6, j = cB % 6;
        const double v = LB[bofs(6 * cb + rB, 6 * cb + cB)];
        const int br = bandblk - 1 - sr, bc = bandblk - 1 - sc;  // separator blocks in image A's order (br <= bc)
        if (sr == sc) LA[bofs(6 * (ca + br) + i, 6 * (ca + br) + j)] += v;
        else LA[bofs(6 * (ca + bc) + j, 6 * (ca + br) + i)] += v;  // the transposed position
      }
    } else {
      const int q = idx - PB * PB, sq = q / 6, i = q % 6;
      LA[nprmax * WBP + 6 * (ca + bandblk - 1 - sq) + i] += LB[nprmax * WBP + 6 * cb + q];
    }
  }
  __syncthreads();
  // ---- chain A goes on through the separator
  if (g == 0 && tl == 0) factor_diag(ca);
  __syncthreads();
  for (int kb = ca; kb < ca + bandblk; ++kb) {
    if (g == 0) panel(kb);
    __syncthreads();
    if (g == 0) trailing(kb, ca + bandblk);
    __syncthreads();
  }
  // @bstamp 4
  // ---- back substitution, column oriented as in band_solve_body (one wave per image): separator first (image A) ...
  auto backsub_block = [&](int kb, bool known, int colmax) {
    // x of block kb (solved here, or `known`: already in y), then y[band columns < colmax] -= L[block rows][column] x
    const int j0 = 6 * kb;
    const double* Dk = L + bofs(j0, j0);
    double Lk[6][6], rp[6], lc[6];
    const int rt = j0 - PB + tl;
    const bool upd = tl < PB && rt >= 0 && rt < colmax;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      rp[i] = rdall[j0 + i];
      lc[i] = upd ? L[(j0 + i) * WBP + tl] : 0.0;
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
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  if (g == 0 && tl < 64)
    for (int kb = ca + bandblk - 1; kb >= ca; --kb) backsub_block(kb, false, npr);
  __syncthreads();
  // @bstamp 5
  if (t < PB) LB[nprmax * WBP + 6 * (cb + bandblk - 1 - t / 6) + t % 6] = LA[nprmax * WBP + 6 * ca + t];  // x of the separator, mirrored
  __syncthreads();
  // ... then both chains at once; in image B the separator rows only hand their (known) x down to the chain's columns
  if (tl < 64) {
    if (g)
      for (int kb = cb + bandblk - 1; kb >= cb; --kb) backsub_block(kb, true, 6 * cb);
    for (int kb = chain - 1; kb >= 0; --kb) backsub_block(kb, false, npr);
  }
  __syncthreads();
  // @bstamp 6
  const bool bad = *failp != 0;
  if (t == 0) {
    if (bad) w.info[2] += 1;
    w.info[5] = 1;
  }
  for (int r = tl; r < (g ? 6 * cb : npr); r += B2_T) {  // image A: chain + separator, image B: its chain
    double x = y[r];
    if (bad || !(x == x)) x = 0.0;
    w.dx[6 * gblk(r / 6) + r % 6] = (float)x;
  }
  __syncthreads();
  apply_retraction(a, t, 2 * B2_T, nb);
  // @bstamp 7
  return true;
}

__global__ __launch_bounds__(2 * BAND_T) void ba_solve_band_kernel(BAArgs a, int lds_doubles) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const BAWs& w = a.w;
  const int n = w.info[3], n_free = w.info[0], bandblk = w.info[4];
  const int ntail = n - 6 * n_free + 1, F = ntail - 1;
  const int PB = 6 * bandblk;
  const int npair = PB * (PB + 1) / 2 + ntail * PB + (F == 0 ? 0 : (F == 1 ? 2 : 5));
  const bool wide = PB + 7 > 64 || npair > 21 + 2 * (BAND_T - 64);
  // long pose-only chains: both ends at once, one chain per half of the workgroup (a uniform decision made before any
  // barrier; VIPE_BA_BAND2=0 in the environment keeps the one-chain form for A/B - passed down as a flag)
  if (!wide && F == 0 && a.band2 && band2_solve_body(a, lds_doubles, smem_raw)) return;
  if (threadIdx.x >= BAND_T) return;  // the one-chain forms are written for BAND_T threads
  if (wide) band_solve_body<BAND_UPT, true>(a, lds_doubles, smem_raw);
  else band_solve_body<2, false>(a, lds_doubles, smem_raw);
}
