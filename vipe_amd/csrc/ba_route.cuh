// ------------------------------------------------------------------------------------------------ route
//
// Which of the four solvers takes the reduced system: the LDS band solver (three forms), the LDS dense solver, the
// single-workgroup global-memory Cholesky or the tiled one.  Written once, as pure integer functions of the plan's facts
// and launch constants - nothing here changes between the iterations of a call or between calls that reuse a plan.  Every
// solver kernel evaluates the route at entry and returns unless the system is its own; the solver that solves reports its
// Solver id in info[INFO_SOLVER] for the caller (vipe_ba_params.path_hint).  Order of preference: band two-chain, band
// one-chain (narrow or wide), dense, global.  Multi-view rigs always take the global solver (dense tail rows).
//
// The limits are LDS sizes and slot counts of the solvers' carves: each size expression below is used by the gate here
// and by the carve it guards in ba_solve_band.inc / ba_solve_dense.inc, which is why their constants live in this file.
constexpr int SOLVER_LDS_DOUBLES = 158 * 1024 / 8;  // dynamic LDS the band and dense solvers are launched with (run_iters)
constexpr int BAND_T = 512;   // band solver: threads per image
constexpr int BAND_UPT = 6;   // trailing-update pairs per thread: dense 12-pose windows (PB = 66: 2277 pairs) still fit
constexpr int DN_T = 512;
constexpr int DN_PP = 20;     // panel buffer: doubles per row = 2 parities x 8 + 4 (20 l16 mod 32 takes 8 values 4 apart: with kq the 64
                              // lanes of an operand-fragment read cover the 32 8-byte slots of the bank window twice - a pitch of 16 is 8-way conflicted)
constexpr int DN_SLOTS = 10;  // 6 tile waves x 10 >= 55 tiles (n + 1 <= 160 rows: 10 tile rows; 11 slots spill)
constexpr int LDS_TAIL_MAX = 2;  // tail unknowns the LDS solvers carry: the shared intrinsics of a mono system
constexpr int CT_MIN_N = 256;  // larger systems take the tiled, chip-wide factorisation

// ---- band solver.  PB = 6 bandblk, WBP = PB + 7 (row pitch), npr = 6 n_free pose rows, rows = tail rows (intrinsics rows
// + the rhs row)

// trailing-update pairs of a block step: pose-pose (lower triangle of the PB rows below the block), tail-pose, tail-tail
__device__ __forceinline__ int band_npair(int PB, int rows) {
  const int F = rows - 1;
  return PB * (PB + 1) / 2 + rows * PB + (F == 0 ? 0 : (F == 1 ? 2 : 5));
}
// pairs that UPT slots per thread hold: 21 (the next diagonal block, wave 0) + UPT per thread of waves 1..7
constexpr int band_pair_cap(int UPT) { return 21 + UPT * (BAND_T - 64); }
// one chain, LDS carve: band [npr][WBP], tail [rows][n + 1] at band_tail0, rdall [npr] at band_rd0, blk[6][7], rd[6], flags
__device__ __forceinline__ int band_tail0(int npr, int WBP) { return npr * WBP; }
__device__ __forceinline__ int band_rd0(int n, int npr, int rows, int WBP) { return band_tail0(npr, WBP) + rows * (n + 1); }
__device__ __forceinline__ int band_need(int n, int npr, int rows, int WBP) { return band_rd0(n, npr, rows, WBP) + npr + 64; }
// two chains over nb blocks: chain A takes ca = (nb - bandblk) / 2 blocks, chain B the cb >= ca others, and both images
// end in the bandblk separator blocks.  Rows of the longer image; LDS carve per image: band [nprmax][WBP], rhs row
// [nprmax + 1], rdall [nprmax], blk 42, rd 6; one flag after both images
__device__ __forceinline__ int band2_rows_max(int nb, int bandblk) { return 6 * (nb - (nb - bandblk) / 2); }
__device__ __forceinline__ int band2_image(int nprmax, int WBP) { return nprmax * WBP + (nprmax + 1) + nprmax + 48; }

// What the route depends on: info[INFO_UNKNOWNS], info[INFO_FREE_POSES], info[INFO_BAND_BLOCKS] of the plan; BAArgs::ntail
// (tail unknowns, n = 6 n_free + ntail), mv, band2; the LDS the band and dense solvers are launched with
struct RouteIn { int n, n_free, bandblk, ntail, mv, band2, lds_doubles; };

enum BandForm { BAND_DECLINES = 0, BAND_NARROW, BAND_WIDE, BAND_TWO_CHAIN };  // narrow: <2, false>, wide: <BAND_UPT, true>

__device__ __forceinline__ int band_form(const RouteIn& r) {
  if (r.mv || r.n == 0) return BAND_DECLINES;
  const int npr = 6 * r.n_free, rows = r.ntail + 1, PB = 6 * r.bandblk, WBP = PB + 7;
  const bool wide = WBP > 64 || band_npair(PB, rows) > band_pair_cap(2);
  // long pose-only chains: both ends at once, tried first.  Not wide: one band column per lane and two pair slots do
  if (!wide && r.ntail == 0 && r.band2 && r.bandblk >= 1 && r.n_free >= 4 * r.bandblk + 4 &&
      2 * band2_image(band2_rows_max(r.n_free, r.bandblk), WBP) + 8 <= r.lds_doubles)
    return BAND_TWO_CHAIN;
  if (band_need(r.n, npr, rows, WBP) > r.lds_doubles || band_npair(PB, rows) > band_pair_cap(wide ? BAND_UPT : 2) ||
      PB + rows > BAND_T || WBP > (wide ? 128 : 64) || r.ntail > LDS_TAIL_MAX)
    return BAND_DECLINES;
  return wide ? BAND_WIDE : BAND_NARROW;
}

// ---- dense solver.  LDS carve: packed factor incl. the rhs row, blk / rd / flags, previews, the chain wave's panel rows,
// rdall, inverse diagonal blocks, panel buffer [16 tile rows][DN_PP]; one register slot per 16 x 16 tile and tile wave
__device__ __forceinline__ int dense_packed(int n) { return ((n + 1) * (n + 2) / 2 + 1) & ~1; }  // even: what follows is 16-byte aligned
__device__ __forceinline__ int dense_tile_rows(int n) { return (n + 16) >> 4; }  // tile rows covering rows 0..n
__device__ __forceinline__ int dense_tiles(int n) { return dense_tile_rows(n) * (dense_tile_rows(n) + 1) / 2; }
__device__ __forceinline__ int dense_need(int n) {
  return dense_packed(n) + 64 + 2 * 36 + 36 + (n + 8) + 6 * (n + 6) + DN_PP * 16 * dense_tile_rows(n);
}
__device__ __forceinline__ bool dense_takes(const RouteIn& r) {
  return r.n != 0 && !r.mv && band_form(r) == BAND_DECLINES && dense_need(r.n) <= r.lds_doubles && r.ntail <= LDS_TAIL_MAX &&
         dense_tiles(r.n) <= 6 * DN_SLOTS;
}

// ---- global-memory solvers: what is left
enum GlobalForm { GLOBAL_DECLINES = 0, GLOBAL_ONE_WORKGROUP, GLOBAL_TILED };

__device__ __forceinline__ int global_form(const RouteIn& r) {
  if (r.n == 0 || band_form(r) != BAND_DECLINES || dense_takes(r)) return GLOBAL_DECLINES;
  return r.n <= CT_MIN_N ? GLOBAL_ONE_WORKGROUP : GLOBAL_TILED;
}

// the inputs of the system the plan left in the workspace.  lds_doubles: the band and dense kernels pass what they were
// launched with, the global-memory ones have no such argument and count on the constant
__device__ __forceinline__ RouteIn route_in(const BAArgs& a, int lds_doubles = SOLVER_LDS_DOUBLES) {
  const int* info = a.w.info;
  return {info[INFO_UNKNOWNS], info[INFO_FREE_POSES], info[INFO_BAND_BLOCKS], a.ntail, a.mv, a.band2, lds_doubles};
}
