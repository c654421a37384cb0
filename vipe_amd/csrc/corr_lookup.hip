// Windowed bilinear lookup into the all-pairs correlation pyramid (droid_net_ext.corr_index_*).
//
// Replaces csrc/droid_net_ext/correlation_kernels.cu:22-159 of the reference.  One lane owns one
// source pixel (b,y,x): it reads the (2r+2)^2 integer taps around floor(coords) from that pixel's
// [h2,w2] slab and keeps the (2r+1)^2 outputs in registers, so every output is written exactly once,
// coalesced along x (the reference does 4 global read-modify-writes per tap).
//
// Numerics (bit-parity contract): per output the four contributions are added in the reference's tap
// order (i = x offset outer, j = y offset inner).  For half, every product and every sum is rounded
// to half (c10::Half operators) and the bilinear weight is rounded to half first.  For float/double the
// update `corr += s * w` is one fused multiply-add (the contraction nvcc applies to that statement).
// Out-of-bounds taps are skipped in the reference; adding their +-0 products instead is bit-identical
// because an accumulator that starts at +0 can never hold -0.
#include <algorithm>
#include <type_traits>

#include "common.cuh"
#include "corr_layout.cuh"

namespace {

template <typename T>
struct Acc;  // arithmetic in the storage type's rounding

template <>
struct Acc<half_t> {
  using reg = float;  // holds a half-representable value
  static __device__ __forceinline__ reg load(const half_t* p) { return (float)*p; }
  static __device__ __forceinline__ reg weight(float w) {
    // the f32 product must be ROUNDED TO f32 before the half conversion (scalar_t(dx * dy) in the reference);
    // without the barrier hipcc fuses mul + cvt into v_fma_mixlo_f16, which rounds the exact product once
    asm volatile("" : "+v"(w));
    return (float)(half_t)w;
  }
  static __device__ __forceinline__ reg madd(reg acc, reg s, reg w) {
    float prod = (float)(half_t)(s * w);  // exact product of two halves, rounded once to half
    return (float)(half_t)(acc + prod);
  }
  static __device__ __forceinline__ half_t store(reg v) { return (half_t)v; }
};
template <>
struct Acc<float> {
  using reg = float;
  static __device__ __forceinline__ reg load(const float* p) { return *p; }
  static __device__ __forceinline__ reg weight(float w) { return w; }
  static __device__ __forceinline__ reg madd(reg acc, reg s, reg w) { return __builtin_fmaf(s, w, acc); }
  static __device__ __forceinline__ float store(reg v) { return v; }
};
template <>
struct Acc<double> {
  using reg = double;
  static __device__ __forceinline__ reg load(const double* p) { return *p; }
  static __device__ __forceinline__ reg weight(float w) { return (double)w; }
  static __device__ __forceinline__ reg madd(reg acc, reg s, reg w) { return __builtin_fma(s, w, acc); }
  static __device__ __forceinline__ double store(reg v) { return v; }
};

// Tap setup of one pixel at pyramid level l (0 for a plain volume): the (2R+2)^2 integer taps (bx + i, by + j) around
// floor(coords / 2**l) and the four bilinear weights.  The weights are a separate step because their rounding barrier
// is not dead code to the compiler: a caller that only needs the window origin does not ask for them.
template <typename T, int R>
struct Taps {
  using A = Acc<T>;
  using reg = typename A::reg;
  struct Weights { reg w00, w01, w10, w11; };
  float dx, dy;
  int bx, by;  // window origin
  __device__ __forceinline__ Taps(float cx, float cy, int l) {
    const float sc = 1.0f / (float)(1 << l);  // coords / 2**l is exact (droid_net.py:78)
    const float x0 = cx * sc, y0 = cy * sc;
    const float fx = floorf(x0), fy = floorf(y0);
    dx = x0 - fx, dy = y0 - fy;
    bx = (int)fx - R, by = (int)fy - R;
  }
  __device__ __forceinline__ int sh() const { return bx & 7; }  // tap column bx within its 8-column chunk bx >> 3
  __device__ __forceinline__ Weights weights() const {
    Weights w;
    w.w11 = A::weight(dx * dy);                    // tap (i,j) -> out[i-1][j-1]
    w.w10 = A::weight(dx * (1.0f - dy));           // tap (i,j) -> out[i-1][j]
    w.w01 = A::weight((1.0f - dx) * dy);           // tap (i,j) -> out[i][j-1]
    w.w00 = A::weight((1.0f - dx) * (1.0f - dy));  // tap (i,j) -> out[i][j]
    return w;
  }
};

// zero channels [from, to) of one pixel's channel row (the padding behind the looked-up channels), split among `lanes`
// lanes of which this is number `lane`
template <typename T>
__device__ __forceinline__ void zero_channels(T* px, int from, int to, int lane = 0, int lanes = 1) {
  for (int q = from + lane; q < to; q += lanes) px[q] = (T)0;
}

// One pixel, one level.  R = radius (compile-time for full unrolling), RD = 2R+1.
template <typename T, int R>
__device__ __forceinline__ void lookup_pixel(const T* __restrict__ slab, int h2, int w2, float cx, float cy, int l,
                                             T* __restrict__ out, int64_t out_stride) {
  constexpr int RD = 2 * R + 1;
  using A = Acc<T>;
  using reg = typename A::reg;
  const Taps<T, R> t(cx, cy, l);
  const auto [w00, w01, w10, w11] = t.weights();

  // taps: s[i][j] = slab[t.by + j][t.bx + i]   (i <-> x, j <-> y), zero outside the map
  reg s[RD + 1][RD + 1];
#pragma unroll
  for (int j = 0; j <= RD; ++j) {
    const int y1 = t.by + j;
    const bool yin = (y1 >= 0) & (y1 < h2);
    const T* row = slab + (int64_t)(yin ? y1 : 0) * w2;
#pragma unroll
    for (int i = 0; i <= RD; ++i) {
      const int x1 = t.bx + i;
      const bool in = yin & (x1 >= 0) & (x1 < w2);
      s[i][j] = in ? A::load(row + x1) : (reg)0;
    }
  }
#pragma unroll
  for (int a = 0; a < RD; ++a) {
#pragma unroll
    for (int b = 0; b < RD; ++b) {
      reg acc = (reg)0;
      acc = A::madd(acc, s[a][b], w00);          // visited at (i=a,   j=b)
      acc = A::madd(acc, s[a][b + 1], w01);      //            (i=a,   j=b+1)
      acc = A::madd(acc, s[a + 1][b], w10);      //            (i=a+1, j=b)
      acc = A::madd(acc, s[a + 1][b + 1], w11);  //            (i=a+1, j=b+1)
      out[(int64_t)(a * RD + b) * out_stride] = A::store(acc);
    }
  }
}

// grid: (ceil(P/256), B); coords [B,2,h1,w1]
template <typename T, int R>
__global__ __launch_bounds__(256) void corr_index_forward_kernel(const T* __restrict__ volume,
                                                                  const float* __restrict__ coords,
                                                                  T* __restrict__ corr, int h1, int w1, int h2,
                                                                  int w2) {
  const int P = h1 * w1;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (p >= P) return;
  const float x0 = coords[((int64_t)n * 2 + 0) * P + p];
  const float y0 = coords[((int64_t)n * 2 + 1) * P + p];
  constexpr int RD = 2 * R + 1;
  const T* slab = volume + ((int64_t)n * P + p) * ((int64_t)h2 * w2);
  T* out = corr + (int64_t)n * RD * RD * P + p;
  lookup_pixel<T, R>(slab, h2, w2, x0, y0, 0, out, P);
}

struct LevelPtrs {
  const void* p[8];
};

// grid: (ceil(P/256), B, levels); coords [B,h1,w1,2]; out [B, L*RD*RD, h1, w1], or with nhwc_stride > 0
// out [B,h1,w1,nhwc_stride] (channel = level*RD*RD + a*RD + b; channels >= L*RD*RD are zero filled)
template <typename T, int R>
__global__ __launch_bounds__(256) void corr_pyramid_lookup_kernel(LevelPtrs lv, const float* __restrict__ coords,
                                                                   T* __restrict__ out, int h1, int w1, int h2,
                                                                   int w2, int L, int nhwc_stride) {
  const int P = h1 * w1;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  const int l = blockIdx.z;
  if (p >= P) return;
  const float2 c = reinterpret_cast<const float2*>(coords)[(int64_t)n * P + p];
  const int h2l = h2 >> l, w2l = w2 >> l;
  constexpr int RD = 2 * R + 1;
  const T* slab = reinterpret_cast<const T*>(lv.p[l]) + ((int64_t)n * P + p) * ((int64_t)h2l * w2l);
  if (nhwc_stride > 0) {
    T* px = out + ((int64_t)n * P + p) * nhwc_stride;
    lookup_pixel<T, R>(slab, h2l, w2l, c.x, c.y, l, px + l * (RD * RD), 1);
    if (l == L - 1) zero_channels(px, L * RD * RD, nhwc_stride);
  } else {
    T* o = out + ((int64_t)n * L + l) * (RD * RD) * P + p;
    lookup_pixel<T, R>(slab, h2l, w2l, c.x, c.y, l, o, P);
  }
}

// ---- fp16 fast path (radius 3, level widths multiples of 8): 8 lanes per (pixel, level), lane j owns tap row j.
// Each lane fetches its 8 taps with TWO aligned 16-byte loads (the row's 16-byte chunks around floor(x) - 3) instead
// of eight 2-byte loads, extracts them with a funnel shift, gets row j+1 from its neighbour lane by shuffle and
// produces the 7 outputs out[a][j], a = 0..6, with exactly the reference's per-output addition chain.  A wave-level
// load instruction now covers 8 pixels x 8 rows x 16 B, i.e. 4x fewer cache-line visits per pixel than the
// lane-per-pixel kernel.
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// ---- the two aligned 16-byte chunks of tap row y1 that cover columns [8 c0, 8 c0 + 16) of source pixel pc's level-l slab
// in `slot` of the level buffer `base`, zero outside the map.  The layout decides where a chunk lives and how many a row has.
template <bool BLK>  // BLK: VIPE_PYRAMID_BLOCKED (source grid == target grid, padded: d), else level l = [slot][P][h2 >> l][w2 >> l]
struct PyrLayout {
  int P, h2, w2;
  BlockedDims d;
  __device__ __forceinline__ PyrLayout(int P_, int h2_, int w2_) : P(P_), h2(h2_), w2(w2_), d(h2_, w2_) {}
};

struct RowPair { uint4v lo, hi; };

// Where those two chunks live and whether each is inside the map.  The address of a chunk outside the map is that of the
// nearest chunk inside it (nearest row, nearest chunk of the row): always readable, and in a line that the other chunk
// of the pair or a neighbouring lane's row fetches anyway, unless the whole window is outside.
struct RowChunks {
  const uint4v* p[2];
  bool ok[2];
};

template <bool BLK>
__device__ __forceinline__ RowChunks row_chunks(const void* base, const PyrLayout<BLK>& lay, int l, int64_t slot, int pc,
                                                int y1, int c0) {
  const half_t* lvl = reinterpret_cast<const half_t*>(base);
  const int h2l = lay.h2 >> l, w2l = lay.w2 >> l;
  // 8-column pieces of a row: whole ones in the reference layout; in the blocked layout the last one may be partial
  // (columns >= w2l stored as zero by the build kernel)
  const int nchunks = BLK ? (w2l + 7) >> 3 : w2l >> 3;
  const bool rowok = (y1 >= 0) & (y1 < h2l);
  const int yr = min(max(y1, 0), h2l - 1);
  // one slab per source pixel (reference layout; levels 2 / 3 of the blocked layout, padded): the row's chunks are
  // contiguous.  Levels 0 / 1 of the blocked layout are tiled
  const bool tiled = BLK && l < 2;
  const uint4v* rowp = nullptr;
  if (!tiled) {
    const BlockedDims::Slab s = BLK ? lay.d.slab23(l, slot, pc) : BlockedDims::Slab{(slot * lay.P + pc) * ((int64_t)h2l * w2l), h2l, w2l};
    rowp = reinterpret_cast<const uint4v*>(lvl + s.base + (int64_t)yr * s.pitch);
  }
  RowChunks ch;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    ch.ok[k] = rowok & (c0 + k >= 0) & (c0 + k < nchunks);
    const int c = min(max(c0 + k, 0), nchunks - 1);
    ch.p[k] = tiled ? reinterpret_cast<const uint4v*>(lvl + lay.d.piece01(l, slot, pc, yr, c)) : rowp + c;
  }
  return ch;
}

template <bool BLK>
__device__ __forceinline__ RowPair gather_row(const void* base, const PyrLayout<BLK>& lay, int l, int64_t slot, int pc,
                                              int y1, int c0) {
  const RowChunks ch = row_chunks(base, lay, l, slot, pc, y1, c0);
  RowPair r = {uint4v{0, 0, 0, 0}, uint4v{0, 0, 0, 0}};
  if (ch.ok[0]) r.lo = *ch.p[0];
  if (ch.ok[1]) r.hi = *ch.p[1];
  return r;
}

// The 7 outputs out[a][j], a = 0..6, of ONE tap row j of one level, in packed fp16 arithmetic.  d[0..7]: the two aligned
// 16-byte chunks of row y = by + j (zero outside the map), sh = (bx & 7): taps t[i] = halves d[sh + i], i = 0..7; the taps
// nb[i] of row y + 1 come from lane + 1 of the 8-lane group.  out[a] = ((t[a] w00 + nb[a] w01) + t[a+1] w10) + nb[a+1] w11
// with every product and every sum rounded to half - c10::Half's operators compute in float and round to half, which
// for two half operands is the correctly rounded half product / sum (the float product of two halves is exact; the
// float sum is exact unless the exponents differ by > 12, when both roundings return the larger operand), i.e. exactly
// v_pk_mul_f16 / v_pk_add_f16.  -ffp-contract=off keeps the compiler from fusing them into v_pk_fma_f16.
// Results: o[k] = (out[2k], out[2k+1]) as packed pairs, k = 0..3 (out[7] is a by-product that no one reads).
__device__ __forceinline__ void row_outputs_pk(const unsigned (&d)[8], int sh, float w00, float w01, float w10, float w11,
                                               half2v (&o)[4]) {
  // funnel: e[k] = halves (sh + 2k, sh + 2k + 1) of the 16-half window.  Dword stages as bit-selects (v_bfi_b32; written
  // as ternaries the compiler turns the stages into a dynamically indexed scratch array), then one v_alignbit by 0 / 16
  const unsigned m1 = 0u - ((unsigned)(sh >> 1) & 1u), m2 = 0u - ((unsigned)(sh >> 2) & 1u);
  unsigned a1[7], f[5];
#pragma unroll
  for (int k = 0; k < 7; ++k) a1[k] = (d[k + 1] & m1) | (d[k] & ~m1);
#pragma unroll
  for (int k = 0; k < 5; ++k) f[k] = (a1[k + 2] & m2) | (a1[k] & ~m2);
  const unsigned hs = ((unsigned)sh & 1u) << 4;
  unsigned e[5];  // e[k] = (t[2k], t[2k+1]); e[4] = (t[8], .) only feeds the unused out[7]
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = __builtin_amdgcn_alignbit(f[k + 1], f[k], hs);
  e[4] = 0;
  const half_t h00 = (half_t)w00, h01 = (half_t)w01, h10 = (half_t)w10, h11 = (half_t)w11;
  const half2v v00 = {h00, h00}, v01 = {h01, h01}, v10 = {h10, h10}, v11 = {h11, h11};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned se = __builtin_amdgcn_alignbyte(e[k + 1], e[k], 2);  // (t[2k+1], t[2k+2])
    const unsigned ne = __shfl_down(e[k], 1, 8), nse = __shfl_down(se, 1, 8);
    half2v acc = __builtin_bit_cast(half2v, e[k]) * v00;   // (half)(0 + p) == p
    acc = acc + __builtin_bit_cast(half2v, ne) * v01;
    acc = acc + __builtin_bit_cast(half2v, se) * v10;
    acc = acc + __builtin_bit_cast(half2v, nse) * v11;
    o[k] = acc;
  }
}

__global__ __launch_bounds__(256) void corr_pyramid_lookup_rows_kernel(LevelPtrs lv, const float* __restrict__ coords,
                                                                       half_t* __restrict__ out, int h1, int w1, int h2,
                                                                       int w2, int L, int nhwc_stride) {
  constexpr int R = 3, RD = 7;
  const int P = h1 * w1;
  const int j = threadIdx.x & 7;                         // tap row
  const int p = blockIdx.x * 32 + (threadIdx.x >> 3);    // pixel
  const int n = blockIdx.y, l = blockIdx.z;
  const bool pok = p < P;
  const int pc = pok ? p : P - 1;
  const float2 c = reinterpret_cast<const float2*>(coords)[(int64_t)n * P + pc];
  const Taps<half_t, R> t(c.x, c.y, l);
  const auto [w00, w01, w10, w11] = t.weights();
  const RowPair r = gather_row(lv.p[l], PyrLayout<false>(P, h2, w2), l, n, pc, t.by + j, t.bx >> 3);
  const unsigned d[8] = {r.lo[0], r.lo[1], r.lo[2], r.lo[3], r.hi[0], r.hi[1], r.hi[2], r.hi[3]};
  half2v o[4];
  row_outputs_pk(d, t.sh(), w00, w01, w10, w11, o);
  if (!pok || j >= RD) return;
#pragma unroll
  for (int a = 0; a < RD; ++a) {
    const int ch = l * (RD * RD) + a * RD + j;
    const half_t v = o[a >> 1][a & 1];
    if (nhwc_stride > 0) out[((int64_t)n * P + p) * nhwc_stride + ch] = v;
    else out[((int64_t)n * L * (RD * RD) + ch) * P + p] = v;
  }
  if (nhwc_stride > 0 && l == L - 1 && j == 0) zero_channels(out + ((int64_t)n * P + p) * nhwc_stride, L * RD * RD, nhwc_stride);
}

// ---- channels-last, 4 levels in one workgroup: the 8 loads of a lane (2 per level) are issued back to back (4x the
// memory-level parallelism of the per-level launch) and the pixel's 196 + 4 channels are staged in LDS so that the
// output leaves as full 16-byte stores, 400 contiguous bytes per pixel (the per-level kernel writes 2-byte pieces:
// 437 MB of HBM writes for 339 MB of output at E = 276).  Same taps, weights and addition chains as above.
constexpr int LK4_PITCH = 208;  // halves per staged pixel (16-byte aligned rows)

// Tap row j of level l of one source pixel, its two chunks in r (zero outside the map) -> channels 49 l .. 49 l + 48 of row
// pl of `stage` (PITCH halves per pixel)
template <int PITCH>
__device__ __forceinline__ void level_to_lds(const RowPair& r, const Taps<half_t, 3>& t, int l, int j, half_t* __restrict__ stage,
                                             int pl) {
  constexpr int RD = 7;
  const auto [w00, w01, w10, w11] = t.weights();
  const unsigned d[8] = {r.lo[0], r.lo[1], r.lo[2], r.lo[3], r.hi[0], r.hi[1], r.hi[2], r.hi[3]};
  half2v o[4];
  row_outputs_pk(d, t.sh(), w00, w01, w10, w11, o);
  if (j < RD) {
#pragma unroll
    for (int a = 0; a < RD; ++a) stage[pl * PITCH + l * (RD * RD) + a * RD + j] = o[a >> 1][a & 1];
  }
}

// Tap row j of all 4 levels of source pixel pc (coords c) -> channels 0..195 of row pl of `stage`.  Two phases: first all 8
// loads of the lane, then the arithmetic - interleaved, each level's loads would wait behind the previous level's
// arithmetic.
template <int PITCH, bool BLK>
__device__ __forceinline__ void lookup4_to_lds(const LevelPtrs& lv, const PyrLayout<BLK>& lay, int64_t slot, int pc, float2 c,
                                               int j, half_t* __restrict__ stage, int pl) {
  constexpr int R = 3, L = 4;
  RowPair r[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const Taps<half_t, R> t(c.x, c.y, l);
    r[l] = gather_row(lv.p[l], lay, l, slot, pc, t.by + j, t.bx >> 3);
  }
#pragma unroll
  for (int l = 0; l < L; ++l) level_to_lds<PITCH>(r[l], Taps<half_t, R>(c.x, c.y, l), l, j, stage, pl);
}

__global__ __launch_bounds__(256) void corr_pyramid_lookup_rows4_kernel(LevelPtrs lv, const float* __restrict__ coords,
                                                                        half_t* __restrict__ out, int h1, int w1, int h2,
                                                                        int w2, int nhwc_stride) {
  constexpr int RD = 7, L = 4;
  __shared__ __align__(16) half_t stage[32 * LK4_PITCH];
  const int P = h1 * w1;
  const int j = threadIdx.x & 7;       // tap row
  const int pl = threadIdx.x >> 3;     // pixel of the workgroup
  const int p = blockIdx.x * 32 + pl;
  const int n = blockIdx.y;
  const bool pok = p < P;
  const int pc = pok ? p : P - 1;
  const float2 c = reinterpret_cast<const float2*>(coords)[(int64_t)n * P + pc];
  lookup4_to_lds<LK4_PITCH>(lv, PyrLayout<false>(P, h2, w2), n, pc, c, j, stage, pl);
  zero_channels(stage + pl * LK4_PITCH, L * RD * RD, L * RD * RD + 4, j, 8);
  __syncthreads();
  // 16-byte pieces of the staged pixels: nhwc_stride / 8 per pixel
  const int cpp = nhwc_stride >> 3;
  for (int i = threadIdx.x; i < 32 * cpp; i += 256) {
    const int pq = i / cpp, ck = i % cpp;
    const int pg = blockIdx.x * 32 + pq;
    if (pg < P)
      *reinterpret_cast<uint4v*>(out + ((int64_t)n * P + pg) * nhwc_stride + ck * 8) =
          *reinterpret_cast<const uint4v*>(stage + pq * LK4_PITCH + ck * 8);
  }
}

// ---- lookup fused with the correlation encoder's 1x1 convolution (droid_net.py:436-437 first layer, 196 -> Cout,
// + bias + activation): the 196 looked-up channels of 64 pixels are staged in LDS as above and consumed right there
// as the B operand of v_mfma_f32_16x16x32_f16; the [E,h,w,200] intermediate (339 MB written and read back per update
// at E = 276) never exists.  Persistent 512-thread workgroups: each wave keeps its 16 output channels x 224 k of the
// packed weights in registers (loaded once), so only the gather and the 256-byte output rows touch memory.
//
// The kernel is bound by the gather (HBM), so what it must do is keep loads in flight, and what it must not do is hold
// more of a CU than that takes: one workgroup is 2 waves per SIMD at <= 128 VGPRs and 47 KB of LDS, i.e. half a CU, and
// the other half is free for a neighbour on another stream (the flow encoder in vipe_update_operator).  A lane's two
// 16-byte row loads of level l of group g + 1 are issued as soon as the arithmetic of level l of group g has freed their
// registers, and stay in flight through the other levels' arithmetic, the barriers, the MFMAs and the stores: each level
// is waited for with a counted vmcnt that leaves the three younger levels out (48 to 64 KiB per workgroup in flight at
// any time, in one register set).  The coordinate and slot loads that head the address chain of group g + 2 are issued
// one pass earlier still.  Prefetches past the last group are clamped to it: no out-of-range address, and the loop
// condition is uniform, so no wave leaves before a barrier.
constexpr int LKC_PITCH = 232;   // halves per staged pixel: 224 k + 8 (row stride 464 B spreads the 16-lane b128 reads)
constexpr int LKC_OPITCH = 136;  // halves per staged output pixel (128 couts + 8)
constexpr int LKC_PX = 64;       // pixels per pass: 8 lanes each
constexpr int LKC_THREADS = 8 * LKC_PX;
constexpr int LKC_LDS = LKC_PX * (LKC_PITCH + LKC_OPITCH) * (int)sizeof(half_t);  // staged rows + staged outputs: 47,104 B
// Asked for instead of LKC_LDS when the CU is to be shared: more than half of the 160 KiB, so a second workgroup of this
// kernel never becomes resident on the CU, and the 76 KiB left hold a tile-convolution workgroup (76,800 B)
constexpr int LKC_LDS_SHARED_CU = 84 * 1024;

typedef _Float16 half8v __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

template <bool BLK>  // BLK: levels in VIPE_PYRAMID_BLOCKED (padded grid), else the reference layout
__global__ __launch_bounds__(LKC_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void corr_lookup_conv_kernel(
    LevelPtrs lv, const float* __restrict__ coords, const half_t* __restrict__ wpk, const float* __restrict__ bias,
    half_t* __restrict__ out, int out_ctot, int out_coff, int h1, int w1, int h2, int w2, int B, int cout_pad, int act,
    const int* __restrict__ slots) {
  constexpr int RD = 7, L = 4;
  extern __shared__ __align__(16) unsigned char lkc_lds[];
  half_t* const stage = reinterpret_cast<half_t*>(lkc_lds);
  half_t* const ostage = stage + LKC_PX * LKC_PITCH;
  const int P = h1 * w1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = tid & 7, pl = tid >> 3;
  const int l16 = lane & 15, kg = lane >> 4;
  const int gpp = (P + LKC_PX - 1) / LKC_PX;
  const int ngroups = B * gpp;
  const PyrLayout<BLK> lay(P, h2, w2);
  // this wave's weights: couts 16 wave + l16, k = 32 s + 8 kg .. + 7  (packed [k / 64][cout_pad][64])
  half8v af[7];
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int k = 32 * s + 8 * kg, r = 16 * wave + l16;
    af[s] = *reinterpret_cast<const half8v*>(wpk + ((int64_t)(k >> 6) * cout_pad + r) * 64 + (k & 63));
  }
  const float4 bv = *reinterpret_cast<const float4*>(bias + 16 * wave + 4 * kg);
  // zero the k padding of the staged rows once (columns 196..231 are never written by the lookup)
  zero_channels(stage + pl * LKC_PITCH, L * RD * RD, LKC_PITCH, j, 8);

  // head of a group's address chain, for this lane's pixel: coordinates and pyramid slot.  Groups past the last one
  // read the last one's
  struct Head { float2 c; int ns, pc; };
  auto head = [&](int grp) {
    grp = min(grp, ngroups - 1);
    const int n = grp / gpp;
    Head hd;
    hd.pc = min((grp % gpp) * LKC_PX + pl, P - 1);
    hd.c = reinterpret_cast<const float2*>(coords)[(int64_t)n * P + hd.pc];
    hd.ns = slots ? slots[n] : n;  // pooled pyramids: edge n lives in slot slots[n] of the level buffers
    return hd;
  };
  const int step = gridDim.x;
  Head hd0 = head(blockIdx.x), hd1 = head(blockIdx.x + step);
  // this lane's two chunks of level l for a group, as loaded (what lies outside the map is dropped when they are used):
  // loads under no branch, so that the waits below are counted ones and leave the younger loads in flight
  auto issue = [&](const Head& hd, int l) {
    const Taps<half_t, 3> t(hd.c.x, hd.c.y, l);
    const RowChunks ch = row_chunks(lv.p[l], lay, l, hd.ns, hd.pc, t.by + j, t.bx >> 3);
    return RowPair{*ch.p[0], *ch.p[1]};
  };
  RowPair rows[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    rows[l] = issue(hd0, l);
    // in the order in which the loop issues them: where the two orders differ, the loop's first wait (for level 0, with
    // the other levels left in flight) is counted for the worse of them and drains every level
    __builtin_amdgcn_sched_barrier(0);
  }

  for (int grp = blockIdx.x; grp < ngroups; grp += step) {
    const Head hd2 = head(grp + 2 * step);
    // level by level: this group's arithmetic, then the next group's loads into the registers it has just freed
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const Taps<half_t, 3> t(hd0.c.x, hd0.c.y, l);
      const RowChunks ch = row_chunks(lv.p[l], lay, l, hd0.ns, hd0.pc, t.by + j, t.bx >> 3);  // for ok[] only
      const uint4v zero = {0, 0, 0, 0};
      level_to_lds<LKC_PITCH>(RowPair{ch.ok[0] ? rows[l].lo : zero, ch.ok[1] ? rows[l].hi : zero}, t, l, j, stage, pl);
      rows[l] = issue(hd1, l);
    }
    __syncthreads();
    // ---- 1x1 convolution of the 64 staged pixels: D[cout, pixel], four 16-pixel tiles per wave
    float4v acc[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) acc[jj] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 7; ++s)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const half8v xf = *reinterpret_cast<const half8v*>(stage + (16 * jj + l16) * LKC_PITCH + 32 * s + 8 * kg);
        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s], xf, acc[jj], 0, 0, 0);
      }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      half4v hv;
      const float v0 = acc[jj][0] + bv.x, v1 = acc[jj][1] + bv.y, v2 = acc[jj][2] + bv.z, v3 = acc[jj][3] + bv.w;
      hv[0] = (half_t)(act == VIPE_ACT_RELU ? fmaxf(v0, 0.0f) : v0);
      hv[1] = (half_t)(act == VIPE_ACT_RELU ? fmaxf(v1, 0.0f) : v1);
      hv[2] = (half_t)(act == VIPE_ACT_RELU ? fmaxf(v2, 0.0f) : v2);
      hv[3] = (half_t)(act == VIPE_ACT_RELU ? fmaxf(v3, 0.0f) : v3);
      *reinterpret_cast<half4v*>(ostage + (16 * jj + l16) * LKC_OPITCH + 16 * wave + 4 * kg) = hv;
    }
    __syncthreads();
    // 256 contiguous bytes per pixel: 2 x 16 B per thread.  The next pass writes `stage` behind this barrier and `ostage`
    // behind its own first one
    {
      const int n = grp / gpp, ck = tid & 7;
      const int pg = (grp % gpp) * LKC_PX + pl;
      if (pg < P) {
        half_t* dst = out + ((int64_t)n * P + pg) * out_ctot + out_coff;
        *reinterpret_cast<uint4v*>(dst + ck * 8) = *reinterpret_cast<const uint4v*>(ostage + pl * LKC_OPITCH + ck * 8);
        *reinterpret_cast<uint4v*>(dst + 64 + ck * 8) = *reinterpret_cast<const uint4v*>(ostage + pl * LKC_OPITCH + 64 + ck * 8);
      }
    }
    hd0 = hd1, hd1 = hd2;
  }
}

// adjoint: each lane owns its pixel's slab, so plain stores into a zero-filled gradient are race free.
template <typename T, int R>
__global__ __launch_bounds__(256) void corr_index_backward_kernel(const float* __restrict__ coords,
                                                                   const T* __restrict__ corr_grad,
                                                                   T* __restrict__ volume_grad, int h1, int w1,
                                                                   int h2, int w2) {
  constexpr int RD = 2 * R + 1;
  using A = Acc<T>;
  using reg = typename A::reg;
  const int P = h1 * w1;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (p >= P) return;
  const float x0 = coords[((int64_t)n * 2 + 0) * P + p];
  const float y0 = coords[((int64_t)n * 2 + 1) * P + p];
  const Taps<T, R> t(x0, y0, 0);
  const auto [w00, w01, w10, w11] = t.weights();
  const T* g = corr_grad + (int64_t)n * RD * RD * P + p;
  T* slab = volume_grad + ((int64_t)n * P + p) * ((int64_t)h2 * w2);
  reg cg[RD][RD];
#pragma unroll
  for (int a = 0; a < RD; ++a)
#pragma unroll
    for (int b = 0; b < RD; ++b) cg[a][b] = A::load(g + (int64_t)(a * RD + b) * P);
#pragma unroll
  for (int i = 0; i <= RD; ++i) {
#pragma unroll
    for (int j = 0; j <= RD; ++j) {
      const int x1 = t.bx + i, y1 = t.by + j;
      if ((y1 >= 0) & (y1 < h2) & (x1 >= 0) & (x1 < w2)) {
        reg acc = (reg)0;  // correlation_kernels.cu:100-107 order
        if (i > 0 && j > 0) acc = A::madd(acc, cg[i - 1][j - 1], w11);
        if (i > 0 && j < RD) acc = A::madd(acc, cg[i - 1][j], w10);
        if (i < RD && j > 0) acc = A::madd(acc, cg[i][j - 1], w01);
        if (i < RD && j < RD) acc = A::madd(acc, cg[i][j], w00);
        slab[(int64_t)y1 * w2 + x1] = A::store(acc);
      }
    }
  }
}

// launch(std::integral_constant<int, r>) if r is one of the radii Rs (the instantiated ones), then the launch status
template <int... Rs, typename F>
int for_radius(int r, F&& launch) {
  const bool hit = ((r == Rs && (launch(std::integral_constant<int, Rs>{}), true)) || ...);
  return hit ? vipe_launch_status() : VIPE_EUNSUPPORTED;
}

// f(T{}) for the storage type T of a VIPE_F* code
template <bool WITH_F64, typename F>
int for_dtype(int dtype, F&& f) {
  if (dtype == VIPE_F16) return f(half_t{});
  if (dtype == VIPE_F32) return f(float{});
  if constexpr (WITH_F64)
    if (dtype == VIPE_F64) return f(double{});
  return VIPE_EINVAL;
}

}  // namespace

VIPE_EXPORT int vipe_corr_index_forward(const void* d_volume, const float* d_coords, void* d_corr, int B, int h1,
                                        int w1, int h2, int w2, int radius, int dtype, void* stream) {
  VIPE_CHECK_ARG(B >= 0 && h1 > 0 && w1 > 0 && h2 > 0 && w2 > 0 && B <= 65535);
  if (B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_volume && d_coords && d_corr);
  const dim3 grid((h1 * w1 + 255) / 256, B);
  return for_dtype<true>(dtype, [&](auto t) {
    using T = decltype(t);
    return for_radius<1, 2, 3, 4>(radius, [&](auto r) {
      corr_index_forward_kernel<T, decltype(r)::value><<<grid, 256, 0, as_stream(stream)>>>(
          (const T*)d_volume, d_coords, (T*)d_corr, h1, w1, h2, w2);
    });
  });
}

VIPE_EXPORT int vipe_corr_index_backward(const float* d_coords, const void* d_corr_grad, void* d_volume_grad, int B,
                                         int h1, int w1, int h2, int w2, int radius, int dtype, void* stream) {
  VIPE_CHECK_ARG(B >= 0 && h1 > 0 && w1 > 0 && h2 > 0 && w2 > 0 && B <= 65535);
  if (B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_coords && d_corr_grad && d_volume_grad);
  hipStream_t s = as_stream(stream);
  const dim3 grid((h1 * w1 + 255) / 256, B);
  return for_dtype<true>(dtype, [&](auto t) {
    using T = decltype(t);
    hipError_t e = hipMemsetAsync(d_volume_grad, 0, sizeof(T) * (size_t)B * h1 * w1 * h2 * w2, s);
    if (e != hipSuccess) return (int)e;
    return for_radius<1, 2, 3, 4>(radius, [&](auto r) {
      corr_index_backward_kernel<T, decltype(r)::value><<<grid, 256, 0, s>>>(d_coords, (const T*)d_corr_grad,
                                                                             (T*)d_volume_grad, h1, w1, h2, w2);
    });
  });
}

static int pyramid_lookup_impl(const void* const* h_levels, const float* d_coords, void* d_out, int B, int h1, int w1,
                               int h2, int w2, int num_levels, int radius, int dtype, int nhwc_stride, void* stream) {
  VIPE_CHECK_ARG(num_levels >= 1 && num_levels <= 8 && B >= 0 && B <= 65535);
  VIPE_CHECK_ARG((h2 >> (num_levels - 1)) >= 1 && (w2 >> (num_levels - 1)) >= 1);
  if (B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(h_levels && d_coords && d_out);
  LevelPtrs lv;
  for (int i = 0; i < num_levels; ++i) {
    VIPE_CHECK_ARG(h_levels[i]);
    lv.p[i] = h_levels[i];
  }
  hipStream_t s = as_stream(stream);
  if (dtype == VIPE_F16 && radius == 3 && ((w2 >> (num_levels - 1)) & 7) == 0) {
    if (num_levels == 4 && nhwc_stride == 200) {
      corr_pyramid_lookup_rows4_kernel<<<dim3((h1 * w1 + 31) / 32, B), 256, 0, s>>>(lv, d_coords, (half_t*)d_out, h1, w1,
                                                                                   h2, w2, nhwc_stride);
      return vipe_launch_status();
    }
    corr_pyramid_lookup_rows_kernel<<<dim3((h1 * w1 + 31) / 32, B, num_levels), 256, 0, s>>>(
        lv, d_coords, (half_t*)d_out, h1, w1, h2, w2, num_levels, nhwc_stride);
    return vipe_launch_status();
  }
  const dim3 grid((h1 * w1 + 255) / 256, B, num_levels);
  return for_dtype<false>(dtype, [&](auto t) {
    using T = decltype(t);
    return for_radius<3, 4>(radius, [&](auto r) {
      corr_pyramid_lookup_kernel<T, decltype(r)::value><<<grid, 256, 0, s>>>(lv, d_coords, (T*)d_out, h1, w1, h2, w2,
                                                                             num_levels, nhwc_stride);
    });
  });
}

VIPE_EXPORT int vipe_corr_pyramid_lookup(const void* const* h_levels, const float* d_coords, void* d_out, int B,
                                         int h1, int w1, int h2, int w2, int num_levels, int radius, int dtype,
                                         void* stream) {
  return pyramid_lookup_impl(h_levels, d_coords, d_out, B, h1, w1, h2, w2, num_levels, radius, dtype, 0, stream);
}

VIPE_EXPORT int vipe_corr_pyramid_lookup_nhwc(const void* const* h_levels, const float* d_coords, void* d_out, int B,
                                              int h1, int w1, int h2, int w2, int num_levels, int radius, int dtype,
                                              int channel_stride, void* stream) {
  const int rd = 2 * radius + 1;
  VIPE_CHECK_ARG(channel_stride >= num_levels * rd * rd);
  return pyramid_lookup_impl(h_levels, d_coords, d_out, B, h1, w1, h2, w2, num_levels, radius, dtype, channel_stride,
                             stream);
}

// compute units of the current device (0: the query failed), asked once per device
static int device_compute_units() {
  static std::atomic<int> cus[64];
  int d = 0;
  (void)hipGetDevice(&d);
  int n = cus[d & 63].load(std::memory_order_relaxed);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) return 0;
  cus[d & 63].store(n, std::memory_order_relaxed);
  return n;
}

VIPE_EXPORT int vipe_corr_lookup_conv1x1(const void* const* h_levels, const float* d_coords, const void* d_w_packed,
                                         const float* d_bias, void* d_out, int out_ctot, int out_coff, int B, int h1,
                                         int w1, int h2, int w2, int Cout, int act, const int* d_slots, int layout,
                                         void* stream) {
  return vipe_corr_lookup_conv1x1_ex(h_levels, d_coords, d_w_packed, d_bias, d_out, out_ctot, out_coff, B, h1, w1, h2, w2,
                                     Cout, act, d_slots, layout, stream, 0, 0);
}

VIPE_EXPORT int vipe_corr_lookup_conv1x1_ex(const void* const* h_levels, const float* d_coords, const void* d_w_packed,
                                            const float* d_bias, void* d_out, int out_ctot, int out_coff, int B, int h1,
                                            int w1, int h2, int w2, int Cout, int act, const int* d_slots, int layout,
                                            void* stream, int max_workgroups, int share_cu) {
  VIPE_CHECK_ARG(B >= 0 && h1 > 0 && w1 > 0 && h2 > 0 && w2 > 0 && max_workgroups >= 0);
  if (B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(h_levels && d_coords && d_w_packed && d_bias && d_out);
  VIPE_CHECK_ARG(act == VIPE_ACT_NONE || act == VIPE_ACT_RELU);
  VIPE_CHECK_ARG(out_ctot % 8 == 0 && out_coff % 8 == 0 && out_coff + Cout <= out_ctot);
  VIPE_CHECK_ARG(layout == VIPE_PYRAMID_REFERENCE || layout == VIPE_PYRAMID_BLOCKED);
  // 4 levels, radius 3, fp16 volume, 128 output channels.  Reference layout: the coarsest level must still have
  // 8-element row chunks (16-byte loads); the blocked layout pads its rows itself: any grid with a non-empty level 3
  if (Cout != 128 || (h2 >> 3) < 1 || (w2 >> 3) < 1) return VIPE_EUNSUPPORTED;
  if (layout == VIPE_PYRAMID_REFERENCE && ((w2 >> 3) & 7) != 0) return VIPE_EUNSUPPORTED;
  if (layout == VIPE_PYRAMID_BLOCKED) VIPE_CHECK_ARG(h1 == h2 && w1 == w2);
  LevelPtrs lv;
  for (int i = 0; i < 4; ++i) {
    VIPE_CHECK_ARG(h_levels[i]);
    lv.p[i] = h_levels[i];
  }
  const int64_t ngroups = (int64_t)B * ((h1 * w1 + LKC_PX - 1) / LKC_PX);
  VIPE_CHECK_ARG(ngroups < (1 << 30));  // the kernel indexes groups, and two prefetch steps past them, in int
  // persistent workgroups, each half a CU (see the kernel): two per CU when the kernel has the device to itself, one -
  // enforced by the LDS request, which grid size alone would not - when a neighbour on another stream is to run beside it
  const int cus = device_compute_units();
  if (cus <= 0) return VIPE_EINVAL;
  int64_t blocks = std::min<int64_t>(ngroups, share_cu ? cus : 2 * cus);
  if (max_workgroups > 0) blocks = std::min<int64_t>(blocks, max_workgroups);
  const size_t lds = share_cu ? LKC_LDS_SHARED_CU : LKC_LDS;
  auto launch = [&](auto blk) {
    auto* kernel = corr_lookup_conv_kernel<decltype(blk)::value>;
    static std::atomic<uint64_t> seen{0};  // one per layout: each call of the generic lambda instantiates its own
    vipe_once_per_device(seen, [&] { (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LKC_LDS_SHARED_CU); });
    kernel<<<(int)blocks, LKC_THREADS, lds, as_stream(stream)>>>(lv, d_coords, (const half_t*)d_w_packed, d_bias, (half_t*)d_out,
                                                                 out_ctot, out_coff, h1, w1, h2, w2, B, 128, act, d_slots);
  };
  if (layout == VIPE_PYRAMID_BLOCKED) launch(std::true_type{});
  else launch(std::false_type{});
  return vipe_launch_status();
}
