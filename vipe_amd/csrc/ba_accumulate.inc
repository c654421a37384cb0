// ------------------------------------------------------------------------------------------------ accumulate (MFMA)
//
// Every reduction over pixels runs on the matrix cores instead of DPP + LDS
// trees (the shuffle version spends ~9.5k DPP adds and ~70 workgroup barriers per tile on 1,281 reduced values):
//   * R1, per term: the lane (= pixel) writes the rows sqrt(w_c) * [Jj_c(6); r_c; Jf_c(F)] of its pixel for both
//     residual components c into a wave-private LDS tile [16 rows][2 x 64 pixels]; one chain of 32
//     v_mfma_f32_16x16x4_f32 (A = B = the tile) yields the Gram matrix = H_jj, -v_j, H_jf, H_ff, -v_f of the term
//     over the wave's 64 pixels.  Only the TARGET-side blocks are reduced: J_i = M J_j per term (M = -Adj(G_ij)^T,
//     or I - Adj^T when both ends are views of one pose), so H_ii += M H_jj M^T, H_ij = M H_jj, v_i += M v_j and
//     H_if += M H_jf are formed from the 6x6 sums by a few lanes afterwards.
//   * R2, per source frame: rows sqrt(Q) * [E_i; E_j(terms); E_f; w] (Q = 1/C per pixel) go to the same LDS region
//     [<= 48 rows][64 pixels]; the Schur complement E Q E^T and the reduced rhs E Q w are the lower-triangle tiles of
//     its Gram matrix (16 MFMAs per 16x16 tile pair).
// Waves never wait for each other inside the walk: wave-private LDS, LDS float atomics into workgroup accumulators,
// three workgroup barriers in total.  Exact fp32 products and sums (the f32 MFMA is an fmaf chain).
// Handles source frames with at most AM_DMAX terms (the radius-3 neighbourhood graph: 6); ba_plan_kernel publishes
// the largest degree in info[INFO_MAX_DEGREE] and exactly one of the two accumulate kernels runs.
constexpr int AM_ROWS = 48;             // R2 row capacity: 6 (AM_DMAX + 1) + F + 1 <= 48
constexpr int AM_P1 = 130;              // float pitch of the R1 tile [16][128]   (= 2 mod 32: conflict-free b32 reads)
constexpr int AM_P2 = 66;               // float pitch of the R2 image [48][64]
constexpr int AM_P2H = 34;              // float pitch of HALF the R2 image [48][32]: the fused kernel reduces the wave's
                                        // 64 pixels in two passes of 32 (34 = 2 + 32 mod 64: lanes (row l16, pixel kq) of an
                                        // MFMA operand read hit 64 distinct banks)
constexpr int AM_WBUF = 16 * AM_P1;     // 2080 floats per wave: the R1 tile (R2 half image: 48 * 34 = 1632)
static_assert(AM_ROWS * AM_P2H <= AM_WBUF, "R2 half image must fit the wave buffer");
constexpr int AM_SP = AM_ROWS + 1;

struct TermGeomM {
  TermGeom g;
  float Mi[36];  // J_i = Mi J_j
};

constexpr size_t accum_mfma_lds() {
  return sizeof(float) * (NWAVE * AM_WBUF + AM_ROWS * AM_SP + AM_DMAX * 256 + 64) + AM_DMAX * sizeof(TermGeomM);
}

typedef float float4m __attribute__((ext_vector_type(4)));

// ---- the term walk, written once.  Everything below inlines into the three accumulate kernels, which keep what only
// they have: the fused kernel its R2 image and Schur scatter, the walk kernel its chunk loop, the rig kernel its local
// map Lm / gcol, its own R1 rows and its tail rows.

// term_setup plus the map of the mono kernels: column c of Mi = [pi == pj: e_c] - Adj(G_ij)^T e_c
template <int CAM>
__device__ __forceinline__ void term_setup_m(const BAArgs& a, int e, TermGeomM& m) {
  TermGeom& g = m.g;
  term_setup<CAM>(a, e, g);
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float ec[6] = {0, 0, 0, 0, 0, 0}, col[6];
    ec[c] = 1.0f;
    adjT_apply(g.G, ec, col);
#pragma unroll
    for (int r = 0; r < 6; ++r) m.Mi[r * 6 + c] = (g.merge == 1 && r == c ? 1.0f : 0.0f) - col[r];
  }
}

// The lane's pixel p of source frame k: its back-projected ray with the derivatives by the source view's intrinsics,
// and the running sums of its disparity block, final when the last term has been walked
template <int F>
struct WalkPixel {
  static constexpr int FF = F > 0 ? F : 1;
  int p;     // clamped to P - 1 ...
  bool inb;  // ... for the lanes past the image, whose weights are 0 and which store nothing
  float d, X0, Y0, Z0, dX0[FF], dY0[FF];  // Z0: the panorama's; pinhole / MEI rays have the constant 1 (transform_ray)
  float C, wz, Ei[6], Efr[FF];  // C_k, w_k, E_kk, E_f (rigs: the intrinsics of the source view)
};

template <int CAM, int F>
__device__ __forceinline__ WalkPixel<F> walk_pixel(const BAArgs& a, int k, int qi) {
  WalkPixel<F> px;
  const int p_raw = blockIdx.x * TILE + threadIdx.x;
  px.inb = p_raw < a.P;
  px.p = px.inb ? p_raw : a.P - 1;
  const cam::Intr Ii = cam::load<CAM>(a.intr + qi * (4 + a.D), a.D, 1.0f / a.p.intr_factor, a.p.ht, a.p.wd);
  const float u = (float)(px.p % a.p.wd), v = (float)(px.p / a.p.wd);
  px.d = a.disps[(int64_t)k * a.P + px.p];
  px.Z0 = 1.0f;
  cam::iproj<CAM, F>(Ii, u, v, px.X0, px.Y0, px.Z0, px.dX0, px.dY0);
  px.C = px.wz = 0.f;
#pragma unroll
  for (int q = 0; q < 6; ++q) px.Ei[q] = 0.f;
#pragma unroll
  for (int f = 0; f < px.FF; ++f) px.Efr[f] = 0.f;
  return px;
}

// Pixel px seen through term G: the point X1 in the target view, projection (x, y) with its Jacobians by the point (Jp) and
// by the target view's intrinsics (Jfj), and Ja = d point / d pose_j (with the rig adjoint where R_qj is not the identity)
template <int CAM, int F>
__device__ __forceinline__ void term_point_jacobians(const TermGeom& G, const WalkPixel<F>& px, float (&X1)[3], float& x,
                                                     float& y, float (&Jp)[2][3], float (&Jfj)[2][WalkPixel<F>::FF],
                                                     float (&Ja)[3][6]) {
  const float d = px.d;
  transform_ray<CAM>(G.T, px.X0, px.Y0, px.Z0, d, X1[0], X1[1], X1[2]);
  const float X = X1[0], Y = X1[1], Z = X1[2];
  cam::proj<CAM, true, F>(G.Ij, X, Y, Z, x, y, Jp, Jfj);
  const float J0[3][6] = {{d, 0, 0, 0, Z, -Y}, {0, d, 0, -Z, 0, X}, {0, 0, d, Y, -X, 0}};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int q = 0; q < 6; ++q) Ja[r][q] = J0[r][q];
  }
  if (G.rig_adj) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float tmp[6];
      adjT_apply(G.Rr, Ja[r], tmp);
#pragma unroll
      for (int q = 0; q < 6; ++q) Ja[r][q] = tmp[q];
    }
  }
}

// Residual component c: Jj = d r_c / d pose_j and Jz = d r_c / d disparity
__device__ __forceinline__ void term_row_jacobians(const float (&Jpc)[3], const float (&Ja)[3][6], const Rigid& T,
                                                   float (&Jj)[6], float& Jz) {
#pragma unroll
  for (int q = 0; q < 6; ++q) Jj[q] = Jpc[0] * Ja[0][q] + Jpc[1] * Ja[1][q] + Jpc[2] * Ja[2][q];
  Jz = Jpc[0] * T.t[0] + Jpc[1] * T.t[1] + Jpc[2] * T.t[2];
}

// ... and by one intrinsic of the SOURCE view through the ray: Jp_c . (R_T d(X0, Y0) / df) (geom.py:286-288), unscaled
__device__ __forceinline__ float term_row_src_intr(const float (&Jpc)[3], const Rigid& T, float dX0, float dY0) {
  const float ax = T.R[0] * dX0 + T.R[1] * dY0;
  const float ay = T.R[3] * dX0 + T.R[4] * dY0;
  const float az = T.R[6] * dX0 + T.R[7] * dY0;
  return Jpc[0] * ax + Jpc[1] * ay + Jpc[2] * az;
}

// Gram matrix of the wave's R1 tile [16 rows][2 x 64 pixels] on the matrix cores: lane (l16, kq) receives
// D[row = 4 kq + r][col = l16], r = 0..3.  The caller scatters them and then meets the wave again before the tile is rewritten.
__device__ __forceinline__ float4m gram_r1(const float* wbuf, int l16, int kq) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float4m g4 = {0.f, 0.f, 0.f, 0.f};
  const float* arow = wbuf + l16 * AM_P1 + kq;
#pragma unroll 8
  for (int s = 0; s < 32; ++s) {
    const float av = arow[4 * s];
    g4 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, av, g4, 0, 0, 0);
  }
  return g4;
}

// The walk of the mono kernels over the `deg` terms staged in tg: R1 rows, Gram sums into acc1[term][16][16], the
// pixel's disparity sums, and the E_j rows left in the workspace
template <int CAM, int F>
__device__ __forceinline__ void walk_tile(const BAArgs& a, const TermGeomM* tg, int deg, bool dfree, float* wbuf,
                                          float* acc1, WalkPixel<F>& px) {
  constexpr int FF = F > 0 ? F : 1;
  constexpr int RPT = F > 0 ? 16 : 8;  // R1 rows per term: 6 J, r, F Jf (padded)
  constexpr int TPT = 16 / RPT;        // terms per R1 tile
  const BAWs& w = a.w;
  const int P = a.P, p = px.p, lane = threadIdx.x & 63, l16 = lane & 15, kq = lane >> 4;
  const bool inb = px.inb;
  // target / weight of the next tile's terms are fetched while the current tile is computed (the walk is otherwise
  // a chain of dependent global-load latencies: measured 5 us per tile)
  float2 nx_t[TPT], nx_w[TPT];
  auto prefetch = [&](int t0) {
#pragma unroll
    for (int uu = 0; uu < TPT; ++uu) {
      const int t = min(t0 + uu, deg - 1);
      load_tw(a, tg[t].g.e, p, P, nx_t[uu], nx_w[uu]);
    }
  };
  prefetch(0);
  for (int t0 = 0; t0 < deg; t0 += TPT) {
    float2 cur_t[TPT], cur_w[TPT];
#pragma unroll
    for (int uu = 0; uu < TPT; ++uu) { cur_t[uu] = nx_t[uu]; cur_w[uu] = nx_w[uu]; }
    if (t0 + TPT < deg) prefetch(t0 + TPT);
#pragma unroll
    for (int uu = 0; uu < TPT; ++uu) {
      const int t = t0 + uu;
      if (t >= deg) break;  // workgroup-uniform
      const TermGeom& G = tg[t].g;
      const int e = G.e;
      float X1[3], x, y, Jp[2][3], Jfj[2][FF], Ja[3][6];
      term_point_jacobians<CAM, F>(G, px, X1, x, y, Jp, Jfj, Ja);
      const float2 tgt = cur_t[uu], wg = cur_w[uu];
      const float val = valid_weight<CAM>(a, X1, inb);  // geom.py:263, buffer.py:413
      const float wd2[2] = {val * wg.x, val * wg.y};                     // weights of the disparity system
      const float wc[2] = {G.merge == 2 ? 0.0f : wd2[0], G.merge == 2 ? 0.0f : wd2[1]};  // ... of the pose blocks
      const float rc[2] = {cam::wrap_dx<CAM>(x - tgt.x, G.Ij.cx), y - tgt.y};
      const bool fj = G.sj >= 0;
      float Ejv[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float Jj[6], Ji[6], Jf[FF], Jz;
        term_row_jacobians(Jp[c], Ja, G.T, Jj, Jz);
        if constexpr (F > 0) {
#pragma unroll
          for (int f = 0; f < F; ++f)
            Jf[f] = (term_row_src_intr(Jp[c], G.T, px.dX0[f], px.dY0[f]) + Jfj[c][f]) * (1.0f / a.p.intr_factor);
        }
        // R1 rows of this term and component
        const float sw = __builtin_amdgcn_sqrtf(wc[c]);  // v_sqrt_f32 (1 ulp): only splits w between the Gram factors
        float* col = wbuf + (uu * RPT) * AM_P1 + c * 64 + lane;
#pragma unroll
        for (int q = 0; q < 6; ++q) col[q * AM_P1] = Jj[q] * sw;
        col[6 * AM_P1] = rc[c] * sw;
        if constexpr (F > 0) {
#pragma unroll
          for (int f = 0; f < F; ++f) col[(7 + f) * AM_P1] = Jf[f] * sw;
        }
        // per-pixel disparity quantities
        if (dfree) {
          const float wJz = wc[c] * Jz;
          px.C += wd2[c] * Jz * Jz;
          px.wz -= wd2[c] * Jz * rc[c];
          float tmp[6];
          adjT_apply(G.G, Jj, tmp);
#pragma unroll
          for (int q = 0; q < 6; ++q) {
            Ji[q] = (G.merge == 1 ? Jj[q] : 0.0f) - tmp[q];
            px.Ei[q] += Ji[q] * wJz;
          }
          if constexpr (F > 0) {
#pragma unroll
            for (int f = 0; f < F; ++f) px.Efr[f] += Jf[f] * wJz;
          }
#pragma unroll
          for (int q = 0; q < 6; ++q) Ejv[q] += Jj[q] * wJz;
        }
      }
      if (dfree && fj && inb) {
#pragma unroll
        for (int q = 0; q < 6; ++q) w.Ej[((int64_t)e * 6 + q) * P + p] = Ejv[q];
      }
    }
    // ---- Gram matrix of the tile over this wave's 64 pixels x 2 components
    const float4m g4 = gram_r1(wbuf, l16, kq);
    // keep the diagonal RPT x RPT blocks
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kq + r;
      const int tb = row / RPT;
      if (l16 / RPT == tb && t0 + tb < deg) atomicAdd(&acc1[(t0 + tb) * 256 + (row % RPT) * 16 + (l16 % RPT)], g4[r]);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// Per-term blocks of the reduced system from the Gram sums of the mono kernels (one wave per term): H_jj, H_ij, v_j,
// H_jf go to S; the shares of the frame-level blocks H_ii, v_i, H_if, H_ff, v_f to accI.  T1 is wave-private scratch.
template <int F>
__device__ __forceinline__ void flush_term_blocks(const BAWs& w, const TermGeomM* tg, int deg, const float* acc1, float* accI,
                                                  float* T1 /* [6][6 + F]: Mi Hjj | Mi Hjf */, int si, int nrow, int foff) {
  constexpr int FF = F > 0 ? F : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool fi = si >= 0;
  for (int t = wave; t < deg; t += NWAVE) {
    const TermGeomM& TG = tg[t];
    const float* Gm = acc1 + t * 256;  // [16][16]: rows/cols 0..5 J, 6 r, 7.. Jf
    const float* Mi = TG.Mi;
    const int sj = TG.g.sj;
    const bool fj = sj >= 0;
    const int bj = 6 * sj, bi = 6 * si;
    if (lane < 36) {
      const int r = lane / 6, c = lane % 6;
      const float hjj = Gm[r * 16 + c];
      if (fj && r >= c) {
        s_add(w, bj + r, bj + c, (double)hjj);
        if (r == c) atomicAdd(&w.Hd[bj + r], (double)hjj);
      }
      float t1 = 0.f;
#pragma unroll
      for (int q = 0; q < 6; ++q) t1 += Mi[r * 6 + q] * Gm[q * 16 + c];
      T1[r * 8 + c] = t1;
      if (fi && fj) s_add(w, bi + r, bj + c, (double)t1);  // H_ij = Mi H_jj
    } else if (lane < 42) {
      const int q = lane - 36;
      const float vjn = Gm[q * 16 + 6];  // sum w J_q r  (v_j = -that)
      if (fj) atomicAdd(&w.S[(int64_t)nrow * w.ld + bj + q], -(double)vjn);
      if (fi) {
        float vin = 0.f;
#pragma unroll
        for (int c = 0; c < 6; ++c) vin += Mi[q * 6 + c] * Gm[c * 16 + 6];
        atomicAdd(&accI[36 + q], -vin);
      }
    } else if (F > 0 && lane < 42 + 6 * F) {
      const int q = (lane - 42) / FF, f = (lane - 42) % FF;
      const float hjf = Gm[q * 16 + 7 + f];
      if (fj) s_add(w, foff + f, bj + q, (double)hjf);
      if (fi) {
        float hif = 0.f;
#pragma unroll
        for (int c = 0; c < 6; ++c) hif += Mi[q * 6 + c] * Gm[c * 16 + 7 + f];
        atomicAdd(&accI[42 + q * FF + f], hif);
      }
    } else if (F > 0 && lane < 42 + 6 * F + F * F) {
      const int i2 = lane - 42 - 6 * F, f = i2 / FF, f2 = i2 % FF;
      if (f >= f2) atomicAdd(&accI[42 + 6 * FF + f * FF + f2], Gm[(7 + f) * 16 + 7 + f2]);
    } else if (F > 0 && lane < 42 + 6 * F + F * F + F) {
      const int f = lane - 42 - 6 * F - F * F;
      atomicAdd(&accI[42 + 6 * FF + FF * FF + f], -Gm[(7 + f) * 16 + 6]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (fi && lane < 36) {
      const int r = lane / 6, c = lane % 6;
      float hii = 0.f;
#pragma unroll
      for (int q = 0; q < 6; ++q) hii += T1[r * 8 + q] * Mi[c * 6 + q];
      atomicAdd(&accI[r * 6 + c], hii);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// Frame level of the mono kernels, from accI [64]: H_ii 36, v_i 6, H_if 6F, H_ff F F, v_f F
template <int F>
__device__ __forceinline__ void flush_frame_blocks(const BAWs& w, const float* accI, int si, int nrow, int foff) {
  constexpr int FF = F > 0 ? F : 1;
  const int tid = threadIdx.x;
  const bool fi = si >= 0;
  const int bi = 6 * si;
  if (tid < 36) {
    const int r = tid / 6, c = tid % 6;
    if (fi && r >= c) {
      const double s = (double)accI[r * 6 + c];
      s_add(w, bi + r, bi + c, s);
      if (r == c) atomicAdd(&w.Hd[bi + r], s);
    }
  } else if (tid < 42) {
    if (fi) atomicAdd(&w.S[(int64_t)nrow * w.ld + bi + (tid - 36)], (double)accI[tid]);
  } else if (F > 0 && tid < 42 + 6 * F) {
    const int q = (tid - 42) / FF, f = (tid - 42) % FF;
    if (fi) s_add(w, foff + f, bi + q, (double)accI[tid]);
  } else if (F > 0 && tid < 42 + 6 * F + F * F) {
    const int i2 = tid - 42 - 6 * F, f = i2 / FF, f2 = i2 % FF;
    if (f >= f2) {
      const double s = (double)accI[tid];
      s_add(w, foff + f, foff + f2, s);
      if (f == f2) atomicAdd(&w.Hd[foff + f], s);
    }
  } else if (F > 0 && tid < 42 + 6 * F + F * F + F) {
    atomicAdd(&w.S[(int64_t)nrow * w.ld + foff + (tid - 42 - 6 * F - F * F)], (double)accI[tid]);
  }
}

// Finish the disparity block of a pixel with a free disparity (sensor prior, damping: terms.py:258-268,
// buffer.py:482-489) and leave C, w, E_kk and the NF shared-intrinsics rows E_f in the workspace
template <int NF, int F>
__device__ __forceinline__ void store_disp_block(const BAArgs& a, int k, int flags, WalkPixel<F>& px) {
  static_assert(NF <= WalkPixel<F>::FF, "E_f rows come from px.Efr");
  const BAWs& w = a.w;
  const int P = a.P, p = px.p;
  const int64_t kp = (int64_t)k * P + p;
  finish_disp(a, k, p, P, flags, px.d, px.C, px.wz);
  if (px.inb) {
    w.C[kp] = px.C;
    w.wv[kp] = px.wz;
#pragma unroll
    for (int q = 0; q < 6; ++q) w.Ekk[((int64_t)k * 6 + q) * P + p] = px.Ei[q];
#pragma unroll
    for (int f = 0; f < NF; ++f) w.Ef[((int64_t)k * 2 + f) * P + p] = px.Efr[f];
  }
}

template <int CAM, int F>
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(3, 3))) void ba_accum_mfma_kernel(BAArgs a) {
  const vipe_ba_params& prm = a.p;
  const BAWs& w = a.w;
  if (a.force_general || w.info[INFO_MAX_DEGREE] > AM_DMAX) return;  // force_general: the walk + Schur pair takes every graph (vipe_ba_params.solver_options)
  const int k = blockIdx.y;
  const int beg = w.rowptr[k], end = w.rowptr[k + 1];
  if (beg == end) return;
  const int deg = end - beg;
  const int P = a.P, V = prm.n_views, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int flags = w.fflags[k];
  const bool dfree = flags & 2;
  const int pose_i = k / V, qi = k % V;
  const int si = w.pose_slot[pose_i];
  const bool fi = si >= 0;
  const int n_free = w.info[INFO_FREE_POSES], nrow = w.info[INFO_UNKNOWNS];
  const int foff = 6 * n_free;

  // @astamp 0
  extern __shared__ __align__(16) float am_smem[];
  float* wbuf = am_smem + wave * AM_WBUF;       // wave-private
  float* accS = am_smem + NWAVE * AM_WBUF;      // [48][49] Schur Gram accumulators
  float* acc1 = accS + AM_ROWS * AM_SP;         // [AM_DMAX][16][16] per-term Gram accumulators
  float* accI = acc1 + AM_DMAX * 256;           // [64] frame level: H_ii 36, v_i 6, H_if 6F, H_ff 3, v_f F
  TermGeomM* tg = reinterpret_cast<TermGeomM*>(accI + 64);

  for (int i = tid; i < AM_ROWS * AM_SP + AM_DMAX * 256 + 64; i += TILE) accS[i] = 0.0f;
  if (tid < deg) {
    TermGeomM m;
    term_setup_m<CAM>(a, w.order[beg + tid], m);
    tg[tid] = m;
  }
  __syncthreads();
  // @astamp 1

  WalkPixel<F> px = walk_pixel<CAM, F>(a, k, qi);
  const int l16 = lane & 15, kq = lane >> 4;
  walk_tile<CAM, F>(a, tg, deg, dfree, wbuf, acc1, px);

  // @astamp 2
  const int NR = 6 * (deg + 1) + F + 1;  // R2 rows: pose i, targets, intrinsics, w
  if (dfree) {
    store_disp_block<F>(a, k, flags, px);
    const float sq = px.inb ? __builtin_amdgcn_rsqf(px.C) : 0.0f;  // sqrt(Q), Q = 1 / C
    // R2 rows, scaled by sqrt(Q).  The wave's 64 pixels are reduced in two passes of 32 (lanes 0-31, then 32-63, put
    // their rows into the [48][32] image; the Gram chains continue across the passes): the wave buffer then is the
    // 8 KiB of the R1 tile instead of 12.4 KiB, three workgroups instead of two fit a CU and the 576 workgroups of the
    // 48-keyframe graph are resident at once instead of in two rounds.
    // all E_j rows of this pixel in flight at once (a per-term loop serialises one L2 round trip per term)
    float ej[AM_DMAX][6];
#pragma unroll
    for (int t = 0; t < AM_DMAX; ++t) {
      const bool on = t < deg && tg[min(t, deg - 1)].g.sj >= 0 && px.inb;
      const int64_t eb = (int64_t)tg[min(t, deg - 1)].g.e * 6 * P + px.p;
#pragma unroll
      for (int q = 0; q < 6; ++q) ej[t][q] = on ? w.Ej[eb + (int64_t)q * P] : 0.0f;
    }
    constexpr int NPAIR = 6;  // lower-triangle 16 x 16 tile pairs of up to 48 rows
    float4m g4[NPAIR];
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) g4[i] = float4m{0.f, 0.f, 0.f, 0.f};
    const int RT = (NR + 15) >> 4;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if ((lane >> 5) == half) {
        float* col = wbuf + (lane & 31);
#pragma unroll
        for (int q = 0; q < 6; ++q) col[q * AM_P2H] = fi ? px.Ei[q] * sq : 0.0f;
#pragma unroll
        for (int t = 0; t < AM_DMAX; ++t) {
          if (t < deg) {
#pragma unroll
            for (int q = 0; q < 6; ++q) col[(6 * (t + 1) + q) * AM_P2H] = ej[t][q] * sq;
          }
        }
        if constexpr (F > 0) {
#pragma unroll
          for (int f = 0; f < F; ++f) col[(6 * (deg + 1) + f) * AM_P2H] = px.Efr[f] * sq;
        }
        col[(NR - 1) * AM_P2H] = px.wz * sq;
        for (int r = NR; r < ((NR + 15) & ~15); ++r) col[r * AM_P2H] = 0.0f;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int ta = 0; ta < 3; ++ta)
#pragma unroll
        for (int tb = 0; tb <= ta; ++tb) {
          if (ta < RT) {  // wave-uniform
            const float* ar = wbuf + (16 * ta + l16) * AM_P2H + kq;
            const float* br = wbuf + (16 * tb + l16) * AM_P2H + kq;
            float4m acc = g4[ta * (ta + 1) / 2 + tb];
#pragma unroll
            for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[4 * s], br[4 * s], acc, 0, 0, 0);
            g4[ta * (ta + 1) / 2 + tb] = acc;
          }
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the second half overwrites the image the chains above have read
    }
#pragma unroll
    for (int ta = 0; ta < 3; ++ta)
#pragma unroll
      for (int tb = 0; tb <= ta; ++tb) {
        if (ta < RT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * ta + 4 * kq + r, cc = 16 * tb + l16;
            if (row < NR && cc <= row) atomicAdd(&accS[row * AM_SP + cc], g4[ta * (ta + 1) / 2 + tb][r]);
          }
        }
      }
  }
  // @astamp 3
  __syncthreads();
  // @astamp 4

  flush_term_blocks<F>(w, tg, deg, acc1, accI, wbuf, si, nrow, foff);
  __syncthreads();
  // @astamp 5

  flush_frame_blocks<F>(w, accI, si, nrow, foff);
  // @astamp 6
  // ---- Schur complement of frame k: S -= E Q E^T, g -= E Q w   (solver.py:176-178)
  if (dfree) {
    auto gmap = [&](int row) -> int {
      if (row >= 6 * (deg + 1)) return foff + (row - 6 * (deg + 1));
      const int m = row / 6, q = row % 6;
      const int sl = m == 0 ? si : tg[m - 1].g.sj;
      return sl >= 0 ? 6 * sl + q : -1;
    };
    for (int i = tid; i < NR * NR; i += TILE) {
      const int row = i / NR, cc = i % NR;
      if (cc > row || cc == NR - 1) continue;
      const int gc = gmap(cc);
      if (gc < 0) continue;
      const float val = accS[row * AM_SP + cc];
      if (row == NR - 1) {
        atomicAdd(&w.S[(int64_t)nrow * w.ld + gc], -(double)val);
      } else {
        const int gr = gmap(row);
        // two terms with the same target (a duplicated edge) put two local rows on one unknown: their cross product
        // belongs to the diagonal entry twice, (r1, r2) and (r2, r1), and the local lower triangle holds it once
        if (gr >= 0) s_add(w, gr, gc, (gr == gc && row != cc) ? -2.0 * (double)val : -(double)val);
      }
    }
  }
  // @astamp 7
}

// ---- general accumulate (any number of terms per source frame): the same walk with matrix-core Gram reductions, the
// terms staged 8 at a time, WITHOUT the Schur complement - that is formed afterwards by ba_schur_kernel from the E rows
// this kernel leaves in the workspace (E_kk, E_j, E_f, w, C).  LDS per workgroup is independent of the degree (42 KB).
constexpr int WK_CH = 8;    // rig walk: terms per chunk
constexpr int WK_CH1 = 12;  // mono walk: the keyframe frontend's source frames have 6-12 terms - with 8 per chunk a 9-term
                            // frame paid a second chunk's set-up (10k cycles of dependent loads, stamps) for one term: 17k of 66k
constexpr size_t walk_lds() {
  return sizeof(float) * (NWAVE * 16 * AM_P1 + WK_CH1 * 256 + 64) + WK_CH1 * sizeof(TermGeomM);
}

template <int CAM, int F>
__global__ __launch_bounds__(TILE) void ba_walk_kernel(BAArgs a) {
  constexpr int WBUF = 16 * AM_P1;
  const vipe_ba_params& prm = a.p;
  const BAWs& w = a.w;
  if (!a.force_general && w.info[INFO_MAX_DEGREE] <= AM_DMAX) return;  // low-degree graphs: the fused kernel
  const int k = blockIdx.y;
  const int beg = w.rowptr[k], end = w.rowptr[k + 1];
  if (beg == end) return;
  const int deg_all = end - beg;
  const int V = prm.n_views, tid = threadIdx.x, wave = tid >> 6;
  const int flags = w.fflags[k];
  const bool dfree = flags & 2;
  const int pose_i = k / V, qi = k % V;
  const int si = w.pose_slot[pose_i];
  const int n_free = w.info[INFO_FREE_POSES], nrow = w.info[INFO_UNKNOWNS];
  const int foff = 6 * n_free;

  extern __shared__ __align__(16) float am_smem[];
  float* wbuf = am_smem + wave * WBUF;        // wave-private R1 tile
  float* acc1 = am_smem + NWAVE * WBUF;       // [WK_CH1][16][16] per-term Gram accumulators of the current chunk
  float* accI = acc1 + WK_CH1 * 256;          // [64] frame level: H_ii 36, v_i 6, H_if 6F, H_ff 3, v_f F
  TermGeomM* tg = reinterpret_cast<TermGeomM*>(accI + 64);
  // @kstamp 0
  if (tid < 64) accI[tid] = 0.0f;

  WalkPixel<F> px = walk_pixel<CAM, F>(a, k, qi);

  for (int cb = 0; cb < deg_all; cb += WK_CH1) {
    const int deg = min(WK_CH1, deg_all - cb);  // terms of this chunk
    // @kstampc 1
    __syncthreads();                            // the previous chunk's flush is done with acc1 / tg
    for (int i = tid; i < WK_CH1 * 256; i += TILE) acc1[i] = 0.0f;
    if (tid < deg) {
      TermGeomM m;
      term_setup_m<CAM>(a, w.order[beg + cb + tid], m);
      tg[tid] = m;
    }
    __syncthreads();
    // @kstampc 2

    walk_tile<CAM, F>(a, tg, deg, dfree, wbuf, acc1, px);
    // @kstampc 3

    __syncthreads();
    // @kstampc 4
    flush_term_blocks<F>(w, tg, deg, acc1, accI, wbuf, si, nrow, foff);
    // @kstampc 5

  }
  __syncthreads();
  // @kstamp 20

  flush_frame_blocks<F>(w, accI, si, nrow, foff);
  if (dfree) store_disp_block<F>(a, k, flags, px);
  // @kstamp 21
}

// ---- multi-view rigs (n_views > 1, optionally the rig-rotation group): the general walk with per-term LOCAL variable
// blocks.  Every Jacobian of a term is a linear image of 6 + 2F "base" rows the walk forms per pixel:
//     base = [Jj (6: d r / d pose_j), JfA (F: intrinsics of the source view qi, plus the target's when qj == qi),
//             JfB (F: intrinsics of the target view qj when qj != qi)]
//     pose_i = Mi0 Jj   (Mi0 = -Adj(G_ij)^T, geom.py:277)      pose_j = Jj
//     rig_qi = -pose_i, rig_qj = -pose_j (geom.py:292-294)       intr_qi = JfA, intr_qj = JfB (terms.py:224-227)
// so ONE Gram matrix of [base; r] per term (matrix cores, as in ba_walk_kernel) gives every block of J^T W J through a
// small map Lm [28 local columns x 10 base rows] and a table gcol[28] of reduced-system columns (-1: fixed).  Local
// columns that land on the same unknown (cross-view self edges: pose_i = pose_j; qi == qj: one rig block) are summed by
// adding ALL ordered pairs (a, b) with gcol[a] >= gcol[b] - exactly (Ja + Jb)^T W (Ja + Jb), what the reference's block
// coalescing produces (matrix.py:124-177).  The E rows of the tail unknowns are accumulated per pixel in registers and
// left in the workspace (Et) for ba_schur_kernel / ba_retract_kernel.
constexpr int RG_NB = 10;  // base rows: Jj 0..5, JfA 6..7, JfB 8..9  (Gram tile rows 0..5, 7..8, 9..10; tile row 6 = r)
constexpr int RG_NL = 28;  // local columns: pose_i 0..5, pose_j 6..11, intr A 12..13, intr B 14..15, rig A 16..21, rig B 22..27
struct TermGeomR {
  TermGeom g;
  int qj, same_view;
  int gcol[RG_NL];
  float Lm[RG_NL][RG_NB];
};
constexpr size_t walk_rig_lds() {
  return sizeof(float) * (NWAVE * 16 * AM_P1 + WK_CH * 256) + WK_CH * sizeof(TermGeomR);
}
__device__ __forceinline__ int rg_tile_row(int b) { return b < 6 ? b : b + 1; }

template <int CAM, int VM>
__global__ __launch_bounds__(TILE) void ba_walk_rig_kernel(BAArgs a) {
  constexpr int WBUF = 16 * AM_P1;
  constexpr int F = CAM == VIPE_CAM_MEI ? 2 : 1;
  const vipe_ba_params& prm = a.p;
  const BAWs& w = a.w;
  const int k = blockIdx.y;
  const int beg = w.rowptr[k], end = w.rowptr[k + 1];
  if (beg == end) return;
  const int deg_all = end - beg;
  const int P = a.P, V = prm.n_views, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int flags = w.fflags[k];
  const bool dfree = flags & 2;
  const int pose_i = k / V, qi = k % V;
  const int si = w.pose_slot[pose_i];
  const int n_free = w.info[INFO_FREE_POSES], nrow = w.info[INFO_UNKNOWNS];
  const int foff = 6 * n_free, roff = foff + a.nintr;
  const bool oi = prm.optimize_intrinsics, orr = prm.optimize_rig_rotation;

  extern __shared__ __align__(16) float am_smem[];
  float* wbuf = am_smem + wave * WBUF;   // wave-private R1 tile; reused as scratch by the flush
  float* acc1 = am_smem + NWAVE * WBUF;  // [WK_CH][16][16] per-term Gram accumulators of the current chunk
  TermGeomR* tg = reinterpret_cast<TermGeomR*>(acc1 + WK_CH * 256);

  WalkPixel<F> px = walk_pixel<CAM, F>(a, k, qi);      // px.Efr: the intrinsics rows of the source view qi
  const int p = px.p;
  const bool inb = px.inb;
  float ErA[6] = {0, 0, 0, 0, 0, 0};                   // rig rows of the source view qi
  float Efv[VM][F] = {}, Erv[VM][6] = {};              // ... of the target views (selected by predicate)
  const int l16 = lane & 15, kq = lane >> 4;

  for (int cb = 0; cb < deg_all; cb += WK_CH) {
    const int deg = min(WK_CH, deg_all - cb);
    __syncthreads();  // the previous chunk's flush is done with acc1 / tg
    for (int i = tid; i < WK_CH * 256; i += TILE) acc1[i] = 0.0f;
    if (tid < deg) {
      TermGeomR& m = tg[tid];
      const int e = w.order[beg + cb + tid];
      const int pi = (int)a.pi[e], pj = (int)a.pj[e], qj = (int)a.qj[e];
      term_transforms(a.poses, a.rig, pi, qi, pj, qj, m.g.T, m.g.G, m.g.Rr);
      m.g.Ij = cam::load<CAM>(a.intr + qj * (4 + a.D), a.D, 1.0f / prm.intr_factor, prm.ht, prm.wd);
      m.g.e = e;
      m.g.merge = (pi == pj);
      m.g.rig_adj = !(m.g.Rr.t[0] == 0.f && m.g.Rr.t[1] == 0.f && m.g.Rr.t[2] == 0.f && m.g.Rr.R[0] == 1.f &&
                      m.g.Rr.R[4] == 1.f && m.g.Rr.R[8] == 1.f);
      m.g.sj = m.g.merge ? -1 : w.pose_slot[pj];  // E_j row of the Schur stack: absent when merged into pose i
      m.qj = qj;
      m.same_view = (qj == qi);
      const int sjj = w.pose_slot[pj];
      for (int c = 0; c < RG_NL; ++c)
        for (int b = 0; b < RG_NB; ++b) m.Lm[c][b] = 0.0f;
      for (int c = 0; c < 6; ++c) {
        float ec[6] = {0, 0, 0, 0, 0, 0}, col[6];
        ec[c] = 1.0f;
        adjT_apply(m.g.G, ec, col);
        for (int r = 0; r < 6; ++r) {
          m.Lm[r][c] = -col[r];       // pose_i = Mi0 Jj
          m.Lm[16 + r][c] = col[r];   // rig of view qi = -pose_i
        }
        m.Lm[6 + c][c] = 1.0f;        // pose_j
        m.Lm[22 + c][c] = -1.0f;      // rig of view qj = -pose_j
      }
      for (int f = 0; f < 2; ++f) {
        m.Lm[12 + f][6 + f] = 1.0f;
        m.Lm[14 + f][8 + f] = 1.0f;
      }
      for (int q = 0; q < 6; ++q) {
        m.gcol[q] = si >= 0 ? 6 * si + q : -1;
        m.gcol[6 + q] = sjj >= 0 ? 6 * sjj + q : -1;
        m.gcol[16 + q] = (orr && qi >= 1) ? roff + 6 * (qi - 1) + q : -1;
        m.gcol[22 + q] = (orr && qj >= 1) ? roff + 6 * (qj - 1) + q : -1;
      }
      for (int f = 0; f < 2; ++f) {
        m.gcol[12 + f] = (oi && f < F) ? foff + qi * F + f : -1;
        m.gcol[14 + f] = (oi && f < F && qj != qi) ? foff + qj * F + f : -1;
      }
    }
    __syncthreads();

    for (int t = 0; t < deg; ++t) {
      const TermGeom& G = tg[t].g;
      const int e = G.e, qj = tg[t].qj;
      const bool same = tg[t].same_view;
      float X1[3], x, y, Jp[2][3], Jfj[2][F], Ja[3][6];
      term_point_jacobians<CAM, F>(G, px, X1, x, y, Jp, Jfj, Ja);
      float2 tgt, wg;
      load_tw(a, e, p, P, tgt, wg);
      const float val = valid_weight<CAM>(a, X1, inb);  // geom.py:263, buffer.py:413
      const float wc[2] = {val * wg.x, val * wg.y};
      const float rc[2] = {cam::wrap_dx<CAM>(x - tgt.x, G.Ij.cx), y - tgt.y};
      float Ejv[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float Jj[6], JfA[F], JfB[F], Jz;
        term_row_jacobians(Jp[c], Ja, G.T, Jj, Jz);
#pragma unroll
        for (int f = 0; f < F; ++f) {
          // Jfi = Jp . (R_T dX0/df) (geom.py:286-288), Jfj from the target camera; J_scale 1/8 (terms.py:224-227)
          const float ji = term_row_src_intr(Jp[c], G.T, px.dX0[f], px.dY0[f]) * (1.0f / prm.intr_factor);
          const float jj = Jfj[c][f] * (1.0f / prm.intr_factor);
          JfA[f] = same ? ji + jj : ji;
          JfB[f] = same ? 0.0f : jj;
        }
        const float sw = __builtin_amdgcn_sqrtf(wc[c]);
        float* col = wbuf + c * 64 + lane;
#pragma unroll
        for (int q = 0; q < 6; ++q) col[q * AM_P1] = Jj[q] * sw;
        col[6 * AM_P1] = rc[c] * sw;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          col[(7 + f) * AM_P1] = f < F ? JfA[f < F ? f : 0] * sw : 0.0f;
          col[(9 + f) * AM_P1] = f < F ? JfB[f < F ? f : 0] * sw : 0.0f;
        }
#pragma unroll
        for (int r = 11; r < 16; ++r) col[r * AM_P1] = 0.0f;
        if (dfree) {
          const float wJz = wc[c] * Jz;
          px.C += wc[c] * Jz * Jz;
          px.wz -= wc[c] * Jz * rc[c];
          float tmp[6];
          adjT_apply(G.G, Jj, tmp);  // pose_i Jacobian before merging: -tmp
#pragma unroll
          for (int q = 0; q < 6; ++q) {
            px.Ei[q] += ((G.merge ? Jj[q] : 0.0f) - tmp[q]) * wJz;
            ErA[q] += tmp[q] * wJz;          // rig of view qi: -(pose_i Jacobian)
            Ejv[q] += Jj[q] * wJz;
          }
#pragma unroll
          for (int f = 0; f < F; ++f) px.Efr[f] += JfA[f] * wJz;
#pragma unroll
          for (int vv = 0; vv < VM; ++vv) {
            if (vv == qj) {
#pragma unroll
              for (int f = 0; f < F; ++f) Efv[vv][f] += JfB[f] * wJz;
#pragma unroll
              for (int q = 0; q < 6; ++q) Erv[vv][q] -= Jj[q] * wJz;  // rig of view qj: -(pose_j Jacobian)
            }
          }
        }
      }
      if (dfree && G.sj >= 0 && inb) {
#pragma unroll
        for (int q = 0; q < 6; ++q) w.Ej[((int64_t)e * 6 + q) * P + p] = Ejv[q];
      }
      // ---- Gram matrix of [base; r] over this wave's 64 pixels x 2 components
      const float4m g4 = gram_r1(wbuf, l16, kq);
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(&acc1[t * 256 + (4 * kq + r) * 16 + l16], g4[r]);
      __builtin_amdgcn_wave_barrier();
    }

    __syncthreads();
    // ---- per-term blocks from the Gram sums (one wave per term): T1 = Lm Gb, H = T1 Lm^T, v = -Lm g
    for (int t = wave; t < deg; t += NWAVE) {
      const TermGeomR& TG = tg[t];
      const float* Gm = acc1 + t * 256;
      float* T1 = wbuf;  // [RG_NL][RG_NB]
      for (int i = lane; i < RG_NL * RG_NB; i += 64) {
        const int c = i / RG_NB, b = i % RG_NB;
        float acc = 0.f;
#pragma unroll
        for (int b2 = 0; b2 < RG_NB; ++b2) acc += TG.Lm[c][b2] * Gm[rg_tile_row(b2) * 16 + rg_tile_row(b)];
        T1[i] = acc;
      }
      if (lane < RG_NL && TG.gcol[lane] >= 0) {
        float acc = 0.f;
#pragma unroll
        for (int b2 = 0; b2 < RG_NB; ++b2) acc += TG.Lm[lane][b2] * Gm[rg_tile_row(b2) * 16 + 6];
        atomicAdd(&w.S[(int64_t)nrow * w.ld + TG.gcol[lane]], -(double)acc);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int i = lane; i < RG_NL * RG_NL; i += 64) {
        const int ca = i / RG_NL, cb2 = i % RG_NL;
        const int ga = TG.gcol[ca], gb = TG.gcol[cb2];
        if (ga < 0 || gb < 0 || ga < gb) continue;
        float acc = 0.f;
#pragma unroll
        for (int b = 0; b < RG_NB; ++b) acc += T1[ca * RG_NB + b] * TG.Lm[cb2][b];
        atomicAdd(&w.S[(int64_t)ga * w.ld + gb], (double)acc);
        if (ga == gb) atomicAdd(&w.Hd[ga], (double)acc);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }

  // ---- finish the disparity block of this pixel and leave the E rows for the Schur / back-substitution kernels
  if (dfree) {
    store_disp_block<0>(a, k, flags, px);  // the intrinsics rows of a rig are tail rows
    if (inb) {
      float* et = w.Et + (int64_t)k * a.ntail * P + p;
      if (oi) {
#pragma unroll
        for (int vv = 0; vv < VM; ++vv) {
          if (vv < V) {
#pragma unroll
            for (int f = 0; f < F; ++f) et[(int64_t)(vv * F + f) * P] = Efv[vv][f] + (vv == qi ? px.Efr[f] : 0.0f);
          }
        }
      }
      if (orr) {
#pragma unroll
        for (int vv = 1; vv < VM; ++vv) {
          if (vv < V) {
#pragma unroll
            for (int q = 0; q < 6; ++q)
              et[(int64_t)(a.nintr + 6 * (vv - 1) + q) * P] = Erv[vv][q] + (vv == qi ? ErA[q] : 0.0f);
          }
        }
      }
    }
  }
}

// Schur complement of one source frame from the E rows in the workspace (general path, after ba_walk_kernel):
// rows = sqrt(Q) * [E_kk (pose i); E_j of every term; E_f; w], Gram over all P pixels, one workgroup per 16 x 16 tile
// pair of the lower triangle.  Each wave takes every fourth 64-pixel chunk: the two row tiles are staged in LDS
// (coalesced 256-byte row segments), 16 v_mfma_f32_16x16x4_f32 per chunk, partial tiles summed through LDS.
constexpr int SC_GRID = 96;  // tile pairs processed in parallel per frame (the kernel strides over the rest; idle blocks exit)

template <int F>
__global__ __launch_bounds__(TILE) void ba_schur_kernel(BAArgs a) {
  const BAWs& w = a.w;
  if (!a.mv && !a.force_general && w.info[INFO_MAX_DEGREE] <= AM_DMAX) return;
  const int k = blockIdx.y;
  const int flags = w.fflags[k];
  const int beg = w.rowptr[k], end = w.rowptr[k + 1];
  if (!(flags & 2) || beg == end) return;
  const int deg = end - beg, P = a.P, V = a.p.n_views;
  const int NT = a.mv ? a.ntail : F;  // tail rows: per-view intrinsics + rig rotations (Et), or the shared intrinsics (Ef)
  const int NR = 6 * (deg + 1) + NT + 1, RT = (NR + 15) >> 4, npairs = RT * (RT + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  const int si = w.pose_slot[k / V];
  const int n_free = w.info[INFO_FREE_POSES], nrow = w.info[INFO_UNKNOWNS], foff = 6 * n_free;
  __shared__ float tile[NWAVE][2][16 * AM_P2];
  __shared__ float red[NWAVE][256];
  __shared__ const float* rowp[32];
  __shared__ float rowm[32];  // 1 for a live row, 0 for an absent one (its pointer then aims at valid memory: loads stay unconditional)
  __shared__ int rowg[32];
  // source row r of the stacked E matrix: pointer to its P values (or null) and its index in the reduced system
  auto resolve = [&](int r, const float*& ptr, int& g) {
    ptr = nullptr; g = -1;
    if (r >= NR) return;
    if (r == NR - 1) { ptr = w.wv + (int64_t)k * P; g = -2; return; }
    if (r >= 6 * (deg + 1)) {
      const int f = r - 6 * (deg + 1);
      ptr = a.mv ? w.Et + ((int64_t)k * NT + f) * P : w.Ef + ((int64_t)k * 2 + f) * P;
      g = foff + f;
      return;
    }
    const int m = r / 6, q = r % 6;
    if (m == 0) {
      if (si >= 0) { ptr = w.Ekk + ((int64_t)k * 6 + q) * P; g = 6 * si + q; }
    } else {
      const int e = w.order[beg + m - 1];
      const int pj = (int)a.pj[e];
      const int sj = ((int)a.pi[e] == pj) ? -1 : w.pose_slot[pj];
      if (sj >= 0) { ptr = w.Ej + (int64_t)e * 6 * P + (int64_t)q * P; g = 6 * sj + q; }
    }
  };
  const float* Ck = w.C + (int64_t)k * P;
  const int nchunks = (P + 63) / 64;
  // A frame with few tile pairs (the keyframe frontend: <= 28) leaves most of the grid's blocks without one: the pixel
  // range of every pair is then cut into `slices` pieces, one workgroup each (the partial Grams meet in the fp64 atomics
  // below) - a workgroup's 12 dependent chunk iterations per wave were the kernel's whole duration (42 us)
  const int slices = max(1, min((int)gridDim.x / npairs, nchunks / NWAVE));
  for (int item = blockIdx.x; item < npairs * slices; item += gridDim.x) {
    const int pid = item / slices, slc = item % slices;
    const int ch0 = (int)((int64_t)nchunks * slc / slices), ch1 = (int)((int64_t)nchunks * (slc + 1) / slices);
    int ta = 0;
    while ((ta + 1) * (ta + 2) / 2 <= pid) ++ta;
    const int tb = pid - ta * (ta + 1) / 2;
    __syncthreads();
    if (tid < 32) {
      const float* ptr; int g;
      resolve(16 * (tid < 16 ? ta : tb) + (tid & 15), ptr, g);
      rowp[tid] = ptr ? ptr : (w.C + (int64_t)k * P); rowm[tid] = ptr ? 1.0f : 0.0f; rowg[tid] = g;
    }
    __syncthreads();
    float4m g4 = {0.f, 0.f, 0.f, 0.f};
    // the rows of the next chunk are fetched while the current chunk's MFMAs run
    float va[16], vb[16], na[16], nb[16];
    auto fetch = [&](int ch, float (&da)[16], float (&db)[16]) {
      const int px = ch * 64 + lane;
      const bool ok = px < P;
      const int pxc = ok ? px : 0;
      const float sq = ok ? __builtin_amdgcn_rsqf(Ck[pxc]) : 0.0f;
      // all 32 row loads are unconditional (absent rows read a valid dummy row and are scaled by 0), so they are in
      // flight together instead of one L2 round trip per guarded load
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        da[r] = rowp[r][pxc];
        db[r] = rowp[16 + r][pxc];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        da[r] *= sq * rowm[r];
        db[r] *= sq * rowm[16 + r];
      }
    };
    if (ch0 + wave < ch1) fetch(ch0 + wave, na, nb);
    for (int ch = ch0 + wave; ch < ch1; ch += NWAVE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { va[r] = na[r]; vb[r] = nb[r]; }
      if (ch + NWAVE < ch1) fetch(ch + NWAVE, na, nb);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        tile[wave][0][r * AM_P2 + lane] = va[r];
        tile[wave][1][r * AM_P2 + lane] = vb[r];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const float* ar = &tile[wave][0][l16 * AM_P2 + kq];
      const float* br = &tile[wave][1][l16 * AM_P2 + kq];
#pragma unroll 8
      for (int s2 = 0; s2 < 16; ++s2) g4 = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[4 * s2], br[4 * s2], g4, 0, 0, 0);
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(4 * kq + r) * 16 + l16] = g4[r];
    __syncthreads();
    {
      const float val = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      const int ra = tid >> 4, cb = tid & 15;
      const int row = 16 * ta + ra, cc = 16 * tb + cb;
      const int gr = rowg[ra], gc = rowg[16 + cb];
      if (row < NR && cc <= row && cc != NR - 1 && gc >= 0) {
        if (row == NR - 1) atomicAdd(&w.S[(int64_t)nrow * w.ld + gc], -(double)val);
        else if (gr >= 0) s_add(w, gr, gc, (gr == gc && row != cc) ? -2.0 * (double)val : -(double)val);  // duplicated edge: see ba_accum_mfma_kernel
      }
    }
  }
}
