// ------------------------------------------------------------------------------------------------ solve (LDS dense)
//
// Dense windows that the band solver cannot hold (the keyframe frontend: up to ~25 free poses, every pair coupled through
// proximity and inactive edges), n + 1 <= 160 rows (26 free poses).  One workgroup of 8 waves, fp64, 6-column block steps; row n of the
// matrix is the right-hand side, so the forward substitution falls out of the factorisation.
//   * The trailing matrix lives in REGISTERS of waves 1..7: 16 x 16 tiles of the lower triangle in the accumulator
//     layout of v_mfma_f64_16x16x4_f64 (negated, so that the update is a plain multiply-accumulate); the update of a
//     block step is two matrix instructions per live tile whose operand fragments come from a panel buffer at addresses
//     that never change (no index arithmetic in the loop).
//   * Wave 0 is the CHAIN wave: it owns the dependent chain and nothing else - factor the 6 x 6 diagonal block in
//     registers (row per lane, pivots by v_readlane), solve the six panel rows of the NEXT diagonal block itself,
//     subtract their product from a preview of that block which the tile waves extracted one step earlier, factor it.
//     The tile waves' panel / update / extract run beside it; two workgroup barriers per step.  The wave that shares
//     the chain wave's SIMD (read from HW_ID) stays idle: fp64 matrix instructions and the chain's fp64 arithmetic use
//     the same pipe, and with a tile wave next to it the chain ran 2.5 times slower (stamps).
//   * LDS holds what has left the registers: the factor (packed rows, for the back substitution), the panel buffer
//     (two parities, rows of 8 doubles: 6 panel columns + 2 zeros = the K = 8 of two matrix instructions), previews.
// A single wave issues at most one instruction every ~4 cycles and a dependent fp64 operation takes ~35: the phases were
// sized by in-kernel cycle stamps (scratch/make_ba_stamps.py) - before this form the chain (2 850 cycles per block) ran
// in sequence with the panel, the update and the extraction (7 700 per step).
// Takes the systems dense_takes (ba_route.cuh, with DN_T, DN_PP, DN_SLOTS and the LDS sizes) gives it and reports
// SOLVER_DENSE in info[INFO_SOLVER].
typedef double double4c __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(DN_T) void ba_solve_dense_kernel(BAArgs a, int lds_doubles) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* const L = reinterpret_cast<double*>(smem_raw);
  const BAWs& w = a.w;
  const int t = threadIdx.x;
  if (!dense_takes(route_in(a, lds_doubles))) return;
  const int n = w.info[INFO_UNKNOWNS], n_free = w.info[INFO_FREE_POSES];
  const int npr = 6 * n_free, F = n - npr;
  const int NP = dense_packed(n);  // packed size incl. the rhs row
  const int NTR = dense_tile_rows(n), NTL = dense_tiles(n);  // tile rows covering rows 0..n; tiles of the triangle
  double* const blk = L + NP;      // 6x7: the current diagonal factor block
  double* const rd = blk + 42;     // its reciprocal pivots
  int* const failp = reinterpret_cast<int*>(rd + 6);
  double* const dnext = rd + 8;    // [2][36] previews of the next diagonal block (entries (i, j), j <= i)
  double* const xbuf = dnext + 72; // [6][6] the chain wave's own panel rows
  double* const rdall = xbuf + 36; // [n] reciprocal pivots of every column (back substitution)
  double* const Linv = rdall + ((n + 8) & ~1);  // [blocks][6][6] inverses of the diagonal factor blocks, zero above the diagonal
  double* const Pbuf = Linv + 6 * (n + 6);      // [16 NTR rows][DN_PP]: panel rows (raw, then solved), parity p at column 8 p
  auto off = [](int r) { return r * (r + 1) / 2; };
  const double* S = w.S;
  const int ld = w.ld;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), l16 = lane & 15, kq = lane >> 4;
  const int nblk = n_free + (F > 0 ? 1 : 0);
  // @stamp 0
  if (t == 0) *failp = 0;
  // roles: wave 0 = chain; waves on its SIMD = idle (barriers only); the others = tile waves, ranked.  Should the
  // hardware place fewer than six waves on the other SIMDs, the idle ones become tile waves after all (slower, correct).
  int* const simd_of = reinterpret_cast<int*>(xbuf);  // 8 ints, before xbuf's first use
  if (lane == 0) simd_of[wave] = (int)(__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4) & 3);  // HW_ID.SIMD_ID
  __syncthreads();
  int twave = -1, ntw = 0;  // this wave's rank among the tile waves; their number
  {
    int others = 0;
    for (int v = 1; v < DN_T / 64; ++v) others += simd_of[v] != simd_of[0];
    const bool use_partners = others < 6;
    for (int v = 1; v < DN_T / 64; ++v) {
      const bool tw = use_partners || simd_of[v] != simd_of[0];
      if (v == wave && tw) twave = ntw;
      ntw += tw;
    }
    if (twave >= 6) twave = -1;  // six tile waves carry all the slots
  }
  twave = __builtin_amdgcn_readfirstlane(twave);
  __syncthreads();
  for (int i = t; i < DN_PP * 16 * NTR; i += DN_T) Pbuf[i] = 0.0;  // columns 6, 7 stay zero; rows beyond n too

  // ---- tile waves: tile tau = I (I + 1) / 2 + J of the lower triangle -> tile wave tau % 6, slot tau / 6.  Per slot and
  //      lane: T (four entries: rows 16 I + kq + 4 r4, column 16 J + l16, NEGATED), the row / column this lane extracts
  //      and the LDS byte addresses of its two operand fragments in the panel buffer
  double4c T[DN_SLOTS];
  int colv[DN_SLOTS], rowv[DN_SLOTS];
#pragma unroll
  for (int sl = 0; sl < DN_SLOTS; ++sl) {
    T[sl] = double4c{0.0, 0.0, 0.0, 0.0};
    colv[sl] = rowv[sl] = -(1 << 20);
  }
  if (twave >= 0) {
#pragma unroll
    for (int sl = 0; sl < DN_SLOTS; ++sl) {
      const int tau = twave + 6 * sl;
      int ti, tj;
      tri_index(tau, ti, tj);
      const bool ok = tau < NTL;
      colv[sl] = ok ? 16 * tj + l16 : -(1 << 20);  // an absent tile is never live and never intersects a column block
      rowv[sl] = ok ? 16 * ti + kq : -(1 << 20);
      // unconditional loads from clamped positions (all of a lane's loads in flight at once: a load under a branch
      // whose condition needs the previous load costs a memory round trip each), selected afterwards
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int row = 16 * ti + kq + 4 * r4, col = 16 * tj + l16;
        const int rr = min(row, n), cc = min(col, min(rr, n - 1));
        T[sl][r4] = S[(int64_t)rr * ld + cc];
      }
    }
    const bool dr = a.droid;
#pragma unroll
    for (int sl = 0; sl < DN_SLOTS; ++sl) {
      double hd[4];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) hd[r4] = dr ? 0.0 : w.Hd[min(max(rowv[sl] + 4 * r4, 0), n - 1)];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int row = rowv[sl] + 4 * r4, col = colv[sl];
        double v = T[sl][r4];
        if (col == row) v = damped_diag(a, row, npr, v, hd[r4]);  // LM damping on the diagonal
        T[sl][r4] = (row <= n && col < n && col <= row && col >= 0) ? -v : 0.0;
      }
    }
  }
  // which of this wave's slots hold tile column J / tile row I: bit masks, lane J < 16 holds the column mask of J and
  // lane 16 + I the row mask of I (a block step finds the two or three slots that meet its columns with two v_readlane
  // instead of testing every slot); nsl = slots in use (the unrolled slot loops leave at the first unused one)
  int maskv = 0, nsl = 0;
#pragma unroll
  for (int sl = 0; sl < DN_SLOTS; ++sl) {
    const int tj = __builtin_amdgcn_readfirstlane(colv[sl]) >> 4, ti = __builtin_amdgcn_readfirstlane(rowv[sl]) >> 4;
    if (tj >= 0) {
      maskv |= ((lane == tj) || (lane == 16 + ti)) ? (1 << sl) : 0;
      nsl = sl + 1;
    }
  }
  // the chain wave's diagonal block: lane i = row i (lanes >= 6 run along on row 5 and store nothing)
  const int ic = lane < 6 ? lane : 5;
  double A[6];
  if (wave == 0) {
    const int bw0 = min(6, n);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double v = (c == ic) ? 1.0 : 0.0;
      if (ic < bw0 && c <= ic) {
        v = S[(int64_t)ic * ld + c];
        if (c == ic) {
          // LM damping, summed as (v + ep) + lambda * d: damped_diag adds v + (ep + lambda * d), one rounding apart,
          // and this block's factor is the head of the dependent chain - its bits stay what they were
          const bool pose = ic < npr;
          v = v + (pose ? (double)a.p.pose_ep : 1e-6) +
              (pose ? (double)a.p.pose_damping : 1e-6) * (a.droid ? v : w.Hd[ic]);
        }
      }
      A[c] = v;
    }
  }
  // factor the block held in A (bw columns; identity beyond); publish L, blk, rd, rdall.
  // DIVISION-FREE elimination: a pivot step multiplies the remaining rows by the pivot p instead of dividing the pivot
  // column by it, a_im <- (a_im p - a_ic a_mc) 2^-e with 2^e the binade of p (an exact rescale that keeps the running
  // scale s in (2^-6, 1]): the dependent chain per pivot is v_readlane -> fused multiply-add -> ldexp instead of
  // reciprocal square root + two Newton steps + multiply + fused multiply-add (9 dependent fp64 operations of ~35 cycles
  // each: 2 850 cycles per block by the stamps).  The factor follows at the end, all six columns at once:
  // L_ic = a_ic / sqrt(p_c s_c), 1 / L_cc = s_c / sqrt(p_c s_c), one reciprocal square root per LANE.  Same stability as
  // the Cholesky recurrence (it is the LDL^T elimination with exactly rescaled rows).
  auto factor_diag = [&](int kb) {
    const int j0 = 6 * kb, bw = min(6, n - j0);
    double sc = 1.0, p_own = 1.0, s_own = 1.0;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      // a non-positive pivot marks the solve as failed (its step is then zero) and the arithmetic just runs on
      const double pv = readlane_f64(A[c], c);
      bad |= (c < bw) & !(pv > 0.0);
      p_own = (ic == c) ? pv : p_own;
      s_own = (ic == c) ? sc : s_own;
      if (c + 1 < 6) {
        // pv = ps 2^e with ps in [0.5, 1): rows are multiplied by ps and the pivot column is scaled by 2^-e ONCE, so that
        // an entry's update is one multiply and one fused multiply-add
        const unsigned long long pb = __builtin_bit_cast(unsigned long long, pv);
        const int e = (int)((pb >> 52) & 0x7ff) - 1022;
        const double ps = __builtin_bit_cast(double, (pb & 0x800fffffffffffffull) | (1022ull << 52));
        const double own_sq = A[c] * A[c];              // ready before the pivot arrives
        const double colc = __builtin_ldexp(A[c], -e);  // this lane's entry of the pivot column, scaled
#pragma unroll
        for (int m = c + 1; m < 6; ++m) {
          // lane c + 1 forms its next pivot from its own entry: no lane hand-off on the dependent chain
          const double prod = (m == c + 1 && ic == c + 1) ? __builtin_ldexp(own_sq, -e) : A[c] * readlane_f64(colc, m);
          A[m] = __builtin_fma(A[m], ps, -prod);
        }
        sc = sc * ps;
      }
    }
    const double rho = rsqrt_nr(p_own * s_own);  // lane c: 1 / sqrt(p_c s_c)
    const double rdv = s_own * rho;              // 1 / L_cc
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double rc = readlane_f64(rho, c);
      A[c] = ic == c ? p_own * rho : (ic > c ? A[c] * rc : 0.0);
    }
    if (lane == 0 && bad) *failp = 1;
    if (lane < 6) {
      rd[lane] = rdv;
      if (lane < bw) rdall[j0 + lane] = rdv;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        if (c <= lane) {
          if (lane < bw) L[off(j0 + lane) + j0 + c] = A[c];
          blk[lane * 7 + c] = A[c];
        }
      }
    }
  };
  // forward substitution of one panel row against the published factor block
  auto solve_row = [&](const double (&raw)[6], int bw, double (&x)[6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double sacc = j < bw ? raw[j] : 0.0;
#pragma unroll
      for (int m = 0; m < j; ++m) sacc = __builtin_fma(-x[m], blk[j * 7 + m], sacc);
      x[j] = sacc * rd[j];
    }
  };
  // tile waves: columns [c0, c0 + cw) of the trailing matrix -> panel buffer Pb (= Pbuf + 8 parity; every row of the
  // tiles that hold them: rows that are not panel rows any more only ever meet finished entries); the block
  // [p0, p0 + pw)^2 that follows -> preview buffer pv
  auto extract = [&](double* Pb, int c0, int cw, int p0, int pw, double* pv) {
    const int cm = __builtin_amdgcn_readlane(maskv, c0 >> 4) | __builtin_amdgcn_readlane(maskv, (c0 + cw - 1) >> 4);
    int pm = 0;
    if (pw > 0) {
      const int ja = p0 >> 4, jb = (p0 + pw - 1) >> 4;
      pm = (__builtin_amdgcn_readlane(maskv, ja) | __builtin_amdgcn_readlane(maskv, jb)) &
           (__builtin_amdgcn_readlane(maskv, 16 + ja) | __builtin_amdgcn_readlane(maskv, 16 + jb));
    }
    if ((cm | pm) == 0) return;
#pragma unroll
    for (int sl = 0; sl < DN_SLOTS; ++sl) {
      if ((cm >> sl) & 1) {
        if ((unsigned)(colv[sl] - c0) < (unsigned)cw) {
          double* dst = Pb + rowv[sl] * DN_PP + (colv[sl] - c0);
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) dst[r4 * 4 * DN_PP] = -T[sl][r4];
        }
      }
      if ((pm >> sl) & 1) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int pr = rowv[sl] + 4 * r4 - p0, pc = colv[sl] - p0;
          if ((unsigned)pr < (unsigned)pw && pc >= 0 && pc <= pr) pv[pr * 6 + pc] = -T[sl][r4];
        }
      }
    }
  };

  if (twave >= 0) extract(Pbuf, 0, min(6, n), min(6, n), min(6, n - min(6, n)), dnext + 36);
  if (wave == 0) factor_diag(0);
  __syncthreads();
  // @stamp 1
  // one block step of each role; the panel buffer's parity is kb & 1.  Two workgroup barriers per step in BOTH loops (the
  // hardware barrier counts arrivals, whatever the code address): separate loops keep the tile registers out of the
  // chain wave's code and the chain's out of the tile waves'
  if (wave == 0) {
    for (int kb = 0; kb < nblk; ++kb) {
      double* const Pb = Pbuf + 8 * (kb & 1);
      const int j0 = 6 * kb, bw = min(6, n - j0), R0 = j0 + bw, nbw = min(6, n - R0);
      double x[6];
      // @stampk 0
      // the rows of the next diagonal block: solved here, kept in registers, published for the update
      if (nbw > 0) {
        const int r = min(R0 + ic, n);
        const double* src = Pb + r * DN_PP;
        double raw[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) raw[j] = src[j];
        solve_row(raw, bw, x);
        if (lane < nbw) {
          double* dst = Pb + r * DN_PP;
          double* lrow = L + off(r) + j0;
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            dst[j] = j < bw ? x[j] : 0.0;
            if (j < bw) lrow[j] = x[j];
            xbuf[lane * 6 + j] = j < bw ? x[j] : 0.0;
          }
        }
      }
      // @stampk 1
      __syncthreads();
      // @stampk 2
      if (nbw > 0) {
        // next diagonal block = its preview (state before this step) - P P^T of its six panel rows, then its factor
        const double* pv = dnext + ((kb + 1) & 1) * 36;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double v = (c == ic) ? 1.0 : 0.0;
          if (ic < nbw && c <= ic) {
            double s0 = pv[ic * 6 + c], s1 = 0.0;
#pragma unroll
            for (int m = 0; m < 6; m += 2) {
              s0 = __builtin_fma(-x[m], xbuf[c * 6 + m], s0);
              s1 = __builtin_fma(-x[m + 1], xbuf[c * 6 + m + 1], s1);
            }
            v = s0 + s1;
          }
          A[c] = v;
        }
        // @stampk 3
        factor_diag(kb + 1);
      }
      // @stampk 4
      __syncthreads();
      // @stampk 5
    }
  } else {
    for (int kb = 0; kb < nblk; ++kb) {
      double* const Pb = Pbuf + 8 * (kb & 1);
      const int j0 = 6 * kb, bw = min(6, n - j0), R0 = j0 + bw, nbw = min(6, n - R0), R1 = R0 + nbw;
      // @wstampk 0
      if (twave >= 0) {
        const int r = R1 + 64 * twave + lane;
        if (r <= n) {
          double* row = Pb + r * DN_PP;
          double raw[6], x[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) raw[j] = row[j];
          solve_row(raw, bw, x);
          double* lrow = L + off(r) + j0;
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            row[j] = j < bw ? x[j] : 0.0;
            if (j < bw) lrow[j] = x[j];
          }
        }
      }
      // @wstampk 1
      __syncthreads();
      // @wstampk 2
      // trailing update T' += P P^T (live tiles: some column >= R0), then the next column block and the preview after it.
      // One inline-asm block per slot - skip test, the four operand reads, both matrix instructions - so that the
      // compiler sees T[sl] modified IN PLACE on every path: through the builtin under a branch it kept the skipped and
      // the updated accumulator in two register sets (four 64-bit moves per slot and step, twice the registers).
      const unsigned pb_u = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const unsigned char*)(Pb + kq);
      const bool upd = twave >= 0 && R0 < n;
#pragma unroll
      for (int sl = 0; sl < DN_SLOTS; ++sl) {
        const int live = __builtin_amdgcn_readfirstlane((int)(upd && sl < nsl && (colv[sl] | 15) >= R0));
        const unsigned aa = pb_u + (unsigned)(((rowv[sl] & ~15) + l16) * (DN_PP * 8));
        const unsigned ba = pb_u + (unsigned)(((colv[sl] & ~15) + l16) * (DN_PP * 8));
        double fa0, fa1, fb0, fb1;
        asm volatile(
            "s_cmp_eq_u32 %7, 0\n\t"
            "s_cbranch_scc1 1f\n\t"
            "ds_read_b64 %1, %5\n\t"
            "ds_read_b64 %3, %6\n\t"
            "ds_read_b64 %2, %5 offset:32\n\t"
            "ds_read_b64 %4, %6 offset:32\n\t"
            "s_waitcnt lgkmcnt(2)\n\t"
            "v_mfma_f64_16x16x4_f64 %0, %1, %3, %0\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "v_mfma_f64_16x16x4_f64 %0, %2, %4, %0\n"
            "1:"
            : "+v"(T[sl]), "=&v"(fa0), "=&v"(fa1), "=&v"(fb0), "=&v"(fb1)
            : "v"(aa), "v"(ba), "s"(live)
            : "scc", "memory");
      }
      // the compiler does not see matrix instructions inside inline asm: cover the result hazard of the last one (the
      // extraction below reads T with vector instructions) by hand
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
      // @wstampk 3
      if (upd) extract(Pbuf + 8 * ((kb + 1) & 1), R0, nbw, R1, min(6, n - R1), dnext + (kb & 1) * 36);
      // @wstampk 4
      __syncthreads();
      // @wstampk 5
    }
  }
  // @stamp 2
  // ---- back substitution L^T x = y (y = row n).  First every diagonal block is replaced by its INVERSE (thread = one
  //      column of one block; all blocks at once), so that a block's six unknowns are six independent dot products
  //      instead of a twelve-step substitution chain.  Then wave 0 alone, y in REGISTERS (lane c holds y[c], y[c + 64],
  //      y[c + 128]): per block the six y entries come by v_readlane, every lane forms all six x (uniform values, the
  //      inverse block by broadcast reads) and subtracts its columns' contributions; the next block's operands are
  //      fetched while the current one is on the chain.  The version that kept y in LDS spent 2 570 cycles per block
  //      (LDS round trip of y behind the 39 in-order prefetch reads) where the dependent chain is ~500.
  const double* y = L + off(n);
  __syncthreads();
  {
    const int kb = t / 6, q = t - 6 * kb;
    if (kb < nblk) {
      const int j0 = 6 * kb, bw = min(6, n - j0);
      double z[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        // column q of the inverse: z_q = 1 / L_qq, z_i = -(sum_{q <= m < i} L_im z_m) / L_ii; zero rows beyond the matrix
        double sacc = 0.0;
#pragma unroll
        for (int m = 0; m < i; ++m) sacc = __builtin_fma((i < bw) ? L[off(j0 + i) + j0 + m] : 0.0, (m >= q) ? z[m] : 0.0, sacc);
        const double ri = (i < bw) ? rdall[j0 + i] : 0.0;
        z[i] = (q < bw) ? ((i == q) ? ri : ((i > q) ? -sacc * ri : 0.0)) : 0.0;
        Linv[kb * 36 + 6 * i + q] = z[i];
      }
    }
  }
  __syncthreads();
  // @stamp 3
  const bool bad = *failp != 0;
  if (t < 64) {
    // y in registers: column c = 48 q + lane (lanes 0..47; 48 = 8 blocks, so a block never straddles two registers).
    // Per block: its six y entries by v_readlane, x_q in the block's own lanes (lane 6 kbl + q holds column q of the
    // inverse), x back to every lane by v_readlane, then each lane subtracts its columns' contributions.  Operands are
    // fetched a block ahead with UNCONDITIONAL loads (what lies right of the block in a packed row is discarded by a
    // select on the result): a predicated load costs a branch, and a spilled operand a scratch round trip.
    constexpr int YR = 4;
    double yv[YR];
#pragma unroll
    for (int q = 0; q < YR; ++q) yv[q] = (t < 48 && 48 * q + t < n) ? y[48 * q + t] : 0.0;
    const int qmax = (nblk - 1) >> 3;
    auto run_reg = [&](auto QC, int kb_hi) {  // blocks kb_hi .. 8 Q, register Q
      constexpr int Q = decltype(QC)::value;
      double col[2][6], lc[2][Q + 1][6];
      auto fetch = [&](int kb, double (&cv)[6], double (&lv)[Q + 1][6]) {
        const int j0 = 6 * kb;
        const double* ci = Linv + kb * 36 + (t - 6 * (kb - 8 * Q));  // column (lane - first lane of the block)
#pragma unroll
        for (int m = 0; m < 6; ++m) {
          cv[m] = ci[6 * m];
          const double* row = L + off(j0 + m) + t;
#pragma unroll
          for (int q = 0; q <= Q; ++q) lv[q][m] = row[48 * q];
        }
      };
      auto solve = [&](int kb, const double (&cv)[6], const double (&lv)[Q + 1][6]) {
        const int kbl = kb - 8 * Q, j0 = 6 * kb, l0 = 6 * kbl;
        double v[6], x[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) v[m] = readlane_f64(yv[Q], l0 + m);
        double s0 = cv[0] * v[0], s1 = cv[1] * v[1];
        s0 = __builtin_fma(cv[2], v[2], s0);
        s1 = __builtin_fma(cv[3], v[3], s1);
        s0 = __builtin_fma(cv[4], v[4], s0);
        s1 = __builtin_fma(cv[5], v[5], s1);
        const double xq = s0 + s1;  // x of column (lane - l0) in the block's lanes
#pragma unroll
        for (int m = 0; m < 6; ++m) x[m] = readlane_f64(xq, l0 + m);
#pragma unroll
        for (int q = 0; q <= Q; ++q) {
          double d0 = lv[q][0] * x[0], d1 = lv[q][1] * x[1];
          d0 = __builtin_fma(lv[q][2], x[2], d0);
          d1 = __builtin_fma(lv[q][3], x[3], d1);
          d0 = __builtin_fma(lv[q][4], x[4], d0);
          d1 = __builtin_fma(lv[q][5], x[5], d1);
          const double nv = yv[q] - (d0 + d1);
          yv[q] = (t < 48 && 48 * q + t < j0) ? nv : yv[q];  // columns left of the block
        }
        yv[Q] = (t >= l0 && t < l0 + 6) ? xq : yv[Q];  // the block's own entries become x
      };
      int kb = kb_hi;
      fetch(kb, col[0], lc[0]);
      while (true) {  // two blocks per trip: the operand buffers are named at compile time
        if (kb > 8 * Q) fetch(kb - 1, col[1], lc[1]);
        solve(kb, col[0], lc[0]);
        if (--kb < 8 * Q) break;
        if (kb > 8 * Q) fetch(kb - 1, col[0], lc[0]);
        solve(kb, col[1], lc[1]);
        if (--kb < 8 * Q) break;
      }
    };
    if (qmax >= 3) run_reg(std::integral_constant<int, 3>{}, nblk - 1);
    if (qmax >= 2) run_reg(std::integral_constant<int, 2>{}, qmax == 2 ? nblk - 1 : 23);
    if (qmax >= 1) run_reg(std::integral_constant<int, 1>{}, qmax == 1 ? nblk - 1 : 15);
    run_reg(std::integral_constant<int, 0>{}, qmax == 0 ? nblk - 1 : 7);
    if (t < 48) {
#pragma unroll
      for (int q = 0; q < YR; ++q) {
        const int dd = 48 * q + t;
        if (dd < n) store_step(w, dd, yv[q], bad);
      }
    }
    if (t == 0) {
      if (bad) w.info[INFO_FAILURES] += 1;
      w.info[INFO_SOLVER] = SOLVER_DENSE;
    }
  }
  // @stamp 4
  __syncthreads();
  apply_retraction(a, t, DN_T, n_free);
  // @stamp 5
}
