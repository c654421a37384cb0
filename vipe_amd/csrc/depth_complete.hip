// Hole-free depth maps: grid kNN scale / shift completion.  A sparse map (the fused surface drawn into a camera: values
// at some pixels, 0 elsewhere) and a dense prediction of the same size; every pixel without a sparse value takes the
// prediction there, aligned to the K nearest pixels that have both by an inverse-distance-weighted least-squares fit of
// scale and shift in the disparity domain.  The rule is stated in include/vipe_amd.h; tests/depth_complete_reference.py
// restates it in float64 by brute force and derives the float32 bounds from the operation count below.
//
// vipe_depth_anchor_bits: anchor(y, x) = sparse and pred both finite and > 0, packed 64 columns to a word:
//   bits [B,H,ceil(W/64)] uint64, bit (x & 63) of word (x >> 6); columns past W are zero.  One wave per word: a ballot.
//
// vipe_depth_complete: one thread per pixel, 64 x 4 pixel tiles (a wave owns 64 x-adjacent pixels of one row), the image
// in blockIdx.y.
//   window   the workgroup stages the bits of its rows y0 - R .. y0 + 3 + R and columns x0 - 64 .. x0 + 127 in LDS:
//            (4 + 2R) x 3 words, 3168 bytes at R = 64.  Rows outside the image are zero; columns outside are zero or,
//            with wrap_x, taken modulo W (a word is put together from pieces of the circular row; W >= 2R + 1 makes every
//            column appear once among the 2R + 1 a target looks at).  Bits at columns >= W are masked off on the way in, so
//            even a stale bit buffer can only name pixels of the image.
//   scan     a target walks rows dy = 0, -1, +1, -2, +2, ... and stops when dy^2 exceeds its K-th best d^2 (R^2 while it
//            holds fewer than K).  In a row it takes the three window words, funnel-shifts them so that bit 64 + dx of
//            (lo, hi) is offset dx, masks |dx| <= floor(sqrt(kth - dy^2)) and walks the set bits with find-first-set.
//   list     K packed keys d^2 << 16 | (dy + R) << 8 | (dx + R) in registers, ascending; unsigned order is the rule's
//            lexicographic order of (d^2, dy, dx).  Insertion is K unrolled min / max pairs: nothing is indexed dynamically.
//   gather   only the final k' neighbours' two values are read from global memory.
//   fit      f32, every product and sum rounded on its own (the library is built with -ffp-contract=off), neighbours in
//            key order:  w = 1 / float(d^2);  S = sum w;  pm = (sum w p) / S;  dm = (sum w d) / S;  e = p - pm;  f = d - dm;
//            var = sum (w e) e;  cov = sum (w e) f;  thr = ((2^-10 pm) (2^-10 pm)) S;
//            affine if k' >= 2, var > thr and s = cov / var > 0: t = dm - s pm;  else s = dm / pm, t = 0;  r = s p + t.
//   stats    affine / scale-only / unreached / rejected, one per target: ballot + popcount per wave, LDS per workgroup, at
//            most four global atomics per workgroup.  Nothing else is atomic.
#include "common.cuh"

namespace {

using u64 = unsigned long long;

constexpr int TILE_W = 64, TILE_H = 4, THREADS = TILE_W * TILE_H;
constexpr int MAX_R = 64, MAX_K = 8, WIN_WORDS = 3;
constexpr unsigned EMPTY_KEY = 0xffffffffu;

enum { ST_AFFINE = 0, ST_SCALE = 1, ST_UNREACHED = 2, ST_REJECTED = 3 };

__device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ld(const half_t* p, int64_t i) { return h2f(p[i]); }
__device__ __forceinline__ void put(float* p, float v) { *p = v; }
__device__ __forceinline__ void put(half_t* p, float v) { *p = f2h(v); }
__device__ __forceinline__ bool pos_finite(float v) { return v > 0.0f && v < __builtin_inff(); }  // false for a NaN

template <typename T>
__global__ __launch_bounds__(THREADS) void anchor_bits_kernel(const T* sparse, const T* pred, u64* bits, int H, int W, int nw) {
  const int word = blockIdx.x % nw;
  const int y = (blockIdx.x / nw) * TILE_H + (threadIdx.x >> 6);
  const int x = word * 64 + lane_id();
  const int64_t b = blockIdx.y;
  bool anchor = false;
  if (y < H && x < W) {
    const int64_t i = (b * H + y) * (int64_t)W + x;
    anchor = pos_finite(ld(sparse, i)) && pos_finite(ld(pred, i));
  }
  const u64 m = __ballot(anchor);
  if (lane_id() == 0 && y < H) bits[(b * H + y) * (int64_t)nw + word] = m;
}

struct CompleteArgs {
  const void *sparse, *pred;  // [B,H,W]
  const unsigned char* mask;  // [B,H,W] or null
  const u64* bits;            // [B,H,nw]
  void* out;                  // [B,H,W]
  float *scale, *shift;       // [B,H,W] or null
  int* nbr;                   // [B,H,W,K] or null
  u64* stats;                 // [4]
  int H, W, nw, R, tiles_x, depth_domain, wrap;
};

// 64 bits of the circular row of W bits, from column `start` (any sign) on
__device__ u64 circular_word(const u64* row, int W, int start) {
  int c = start % W;
  if (c < 0) c += W;
  u64 out = 0;
  int filled = 0;
  while (filled < 64) {
    int n = min(64 - filled, W - c);
    n = min(n, 64 - (c & 63));  // stay inside one source word
    u64 src = row[c >> 6] >> (c & 63);
    if (n < 64) src &= (1ull << n) - 1;
    out |= src << filled;
    filled += n;
    c += n;
    if (c == W) c = 0;
  }
  return out;
}

__device__ __forceinline__ int isqrt_small(int n) {  // floor(sqrt(n)), 0 <= n <= 4096
  int r = (int)sqrtf((float)n);
  if (r * r > n) --r;
  if ((r + 1) * (r + 1) <= n) ++r;
  return r;
}

template <int K>
__device__ __forceinline__ void insert(unsigned (&k)[K], unsigned key) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const unsigned lo = min(key, k[i]), hi = max(key, k[i]);
    k[i] = lo;
    key = hi;
  }
}

template <typename T, int K>
__global__ __launch_bounds__(THREADS) void depth_complete_kernel(CompleteArgs a) {
  __shared__ u64 win[(TILE_H + 2 * MAX_R) * WIN_WORDS];
  __shared__ unsigned wg_stats[4];
  const int64_t b = blockIdx.y;
  const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
  const int x0 = tx * TILE_W, y0 = ty * TILE_H;
  const int R = a.R, H = a.H, W = a.W;
  if (threadIdx.x < 4) wg_stats[threadIdx.x] = 0;
  {
    const u64* img = a.bits + b * H * (int64_t)a.nw;
    const int tail = W & 63;
    for (int i = threadIdx.x; i < (TILE_H + 2 * R) * WIN_WORDS; i += THREADS) {
      const int wr = i / WIN_WORDS, ww = i - wr * WIN_WORDS;
      const int yy = y0 - R + wr;
      u64 v = 0;
      if (yy >= 0 && yy < H) {
        const u64* row = img + (int64_t)yy * a.nw;
        if (a.wrap) {
          v = circular_word(row, W, x0 - 64 + 64 * ww);
        } else {
          const int gw = tx - 1 + ww;
          if (gw >= 0 && gw < a.nw) v = row[gw];
          if (gw == a.nw - 1 && tail) v &= (1ull << tail) - 1;
        }
      }
      win[i] = v;
    }
  }
  __syncthreads();
  const int lx = threadIdx.x & (TILE_W - 1), ly = threadIdx.x / TILE_W;
  const int x = x0 + lx, y = y0 + ly;
  int what = -1;  // lanes outside the image and pixels that are no target count nowhere
  if (x < W && y < H) {
    const T* sparse = (const T*)a.sparse + b * H * (int64_t)W;
    const T* pred = (const T*)a.pred + b * H * (int64_t)W;
    const int64_t pix = (int64_t)y * W + x, gpix = b * H * (int64_t)W + pix;
    const float vs = ld(sparse, pix), vp = ld(pred, pix);
    const bool anchor = pos_finite(vs) && pos_finite(vp);
    const bool target = !anchor && pos_finite(vp) && (!a.mask || a.mask[gpix] != 0);
    unsigned k[K];
#pragma unroll
    for (int i = 0; i < K; ++i) k[i] = EMPTY_KEY;
    float s = anchor ? 1.0f : 0.0f, t = 0.0f, result = 0.0f;
    if (target) {
      const int R2 = R * R;
      for (int ady = 0; ady <= R; ++ady) {
        bool done = false;
#pragma unroll
        for (int sgn = 0; sgn < 2; ++sgn) {
          if (sgn == 1 && ady == 0) continue;
          const int lim = k[K - 1] == EMPTY_KEY ? R2 : (int)(k[K - 1] >> 16);
          if (ady * ady > lim) { done = true; break; }
          const int dy = sgn ? ady : -ady;
          if (y + dy < 0 || y + dy >= H) continue;
          const int rx = isqrt_small(lim - ady * ady);
          const u64* wrow = win + (ly + R + dy) * WIN_WORDS;
          const u64 w0 = wrow[0], w1 = wrow[1], w2 = wrow[2];
          u64 lo = lx ? (w0 >> lx) | (w1 << (64 - lx)) : w0;  // bit j: dx = j - 64
          u64 hi = lx ? (w1 >> lx) | (w2 << (64 - lx)) : w1;  // bit j: dx = j
          const bool ex = rx >= 64 && ((w2 >> lx) & 1);       // dx = 64
          lo &= rx >= 64 ? ~0ull : (rx == 0 ? 0ull : ~0ull << (64 - rx));
          hi &= rx >= 63 ? ~0ull : (1ull << (rx + 1)) - 1;
          const unsigned base = ((unsigned)(ady * ady) << 16) | ((unsigned)(dy + R) << 8);
          while (lo) {
            const int dx = __ffsll((long long)lo) - 1 - 64;
            lo &= lo - 1;
            insert<K>(k, base + ((unsigned)(dx * dx) << 16) + (unsigned)(dx + R));
          }
          while (hi) {
            const int dx = __ffsll((long long)hi) - 1;
            hi &= hi - 1;
            insert<K>(k, base + ((unsigned)(dx * dx) << 16) + (unsigned)(dx + R));
          }
          if (ex) insert<K>(k, base + (4096u << 16) + (unsigned)(64 + R));
        }
        if (done) break;
      }
      // the final neighbours' values, as disparities, in key order
      float w[K], p[K], d[K];
      int kp = 0;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        w[i] = p[i] = d[i] = 0.0f;
        if (k[i] != EMPTY_KEY) {
          ++kp;
          const int d2 = (int)(k[i] >> 16), dy = (int)((k[i] >> 8) & 255) - R, dx = (int)(k[i] & 255) - R;
          int xx = x + dx;
          if (a.wrap) xx = xx < 0 ? xx + W : (xx >= W ? xx - W : xx);
          const int64_t j = (int64_t)(y + dy) * W + xx;
          k[i] = (unsigned)j;  // from here on the list holds pixel indices (H W < 2^31; EMPTY_KEY stays what it is)
          float pv = ld(pred, j), dv = ld(sparse, j);
          if (a.depth_domain) pv = __fdiv_rn(1.0f, pv), dv = __fdiv_rn(1.0f, dv);
          w[i] = __fdiv_rn(1.0f, (float)d2);
          p[i] = pv;
          d[i] = dv;
        }
      }
      if (kp == 0) {
        what = ST_UNREACHED;
      } else {
        float S = 0.0f, Sp = 0.0f, Sd = 0.0f;
#pragma unroll
        for (int i = 0; i < K; ++i)
          if (i < kp) S += w[i], Sp += w[i] * p[i], Sd += w[i] * d[i];
        const float pm = __fdiv_rn(Sp, S), dm = __fdiv_rn(Sd, S);
        float var = 0.0f, cov = 0.0f;
#pragma unroll
        for (int i = 0; i < K; ++i)
          if (i < kp) {
            const float e = p[i] - pm, f = d[i] - dm, we = w[i] * e;
            var += we * e;
            cov += we * f;
          }
        const float e0 = 0.0009765625f * pm;
        const float thr = (e0 * e0) * S;
        bool affine = kp >= 2 && var > thr;
        if (affine) {
          s = __fdiv_rn(cov, var);
          affine = s > 0.0f;
        }
        if (affine) t = dm - s * pm;
        else s = __fdiv_rn(dm, pm), t = 0.0f;
        const float pt = a.depth_domain ? __fdiv_rn(1.0f, vp) : vp;
        const float r = s * pt + t;
        if (pos_finite(r)) {
          what = affine ? ST_AFFINE : ST_SCALE;
          result = a.depth_domain ? __fdiv_rn(1.0f, r) : r;
        } else {
          what = ST_REJECTED;
        }
      }
      if (what == ST_UNREACHED || what == ST_REJECTED) s = t = 0.0f;
    }
    T* out = (T*)a.out + gpix;
    if (anchor) *out = sparse[pix];  // the stored value as it is, not through a float
    else put(out, result);
    if (a.scale) a.scale[gpix] = s;
    if (a.shift) a.shift[gpix] = t;
    if (a.nbr) {
      int* nb = a.nbr + gpix * K;
#pragma unroll
      for (int i = 0; i < K; ++i) nb[i] = (int)k[i];  // EMPTY_KEY is -1
    }
  }
  const int lane = lane_id();
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const u64 m = __ballot(what == c);
    if (m != 0 && lane == 0) atomicAdd(wg_stats + c, (unsigned)__popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < 4 && wg_stats[threadIdx.x]) atomicAdd(a.stats + threadIdx.x, (u64)wg_stats[threadIdx.x]);
}

template <typename T>
void launch_complete(int K, dim3 grid, hipStream_t s, const CompleteArgs& a) {
  switch (K) {
    case 1: depth_complete_kernel<T, 1><<<grid, THREADS, 0, s>>>(a); break;
    case 2: depth_complete_kernel<T, 2><<<grid, THREADS, 0, s>>>(a); break;
    case 3: depth_complete_kernel<T, 3><<<grid, THREADS, 0, s>>>(a); break;
    case 4: depth_complete_kernel<T, 4><<<grid, THREADS, 0, s>>>(a); break;
    case 5: depth_complete_kernel<T, 5><<<grid, THREADS, 0, s>>>(a); break;
    case 6: depth_complete_kernel<T, 6><<<grid, THREADS, 0, s>>>(a); break;
    case 7: depth_complete_kernel<T, 7><<<grid, THREADS, 0, s>>>(a); break;
    default: depth_complete_kernel<T, 8><<<grid, THREADS, 0, s>>>(a); break;
  }
}

// the size conditions both entry points share -> tiles per image, or -1
int64_t tiles_of(int B, int H, int W) {
  if (B < 0 || B > 65535 || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24)) return -1;
  if ((int64_t)H * W > 0x7fffffff) return -1;  // neighbour indices are int32
  return (int64_t)((W + TILE_W - 1) / TILE_W) * ((H + TILE_H - 1) / TILE_H);
}

}  // namespace

VIPE_EXPORT int vipe_depth_anchor_bits(const void* d_sparse, const void* d_pred, int dtype, int B, int H, int W,
                                       int64_t* d_bits, void* stream) {
  VIPE_CHECK_ARG(dtype == VIPE_F16 || dtype == VIPE_F32);
  const int64_t tiles = tiles_of(B, H, W);
  VIPE_CHECK_ARG(tiles > 0 && tiles <= 0x7fffffff);
  if (B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_sparse && d_pred && d_bits);
  const int nw = (W + 63) / 64;
  const dim3 grid((unsigned)tiles, B);  // a tile is 64 columns x 4 rows here as well: one word per wave
  hipStream_t s = as_stream(stream);
  if (dtype == VIPE_F32) anchor_bits_kernel<float><<<grid, THREADS, 0, s>>>((const float*)d_sparse, (const float*)d_pred, (u64*)d_bits, H, W, nw);
  else anchor_bits_kernel<half_t><<<grid, THREADS, 0, s>>>((const half_t*)d_sparse, (const half_t*)d_pred, (u64*)d_bits, H, W, nw);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_depth_complete(const void* d_sparse, const void* d_pred, int dtype, const unsigned char* d_mask,
                                    const int64_t* d_bits, int B, int H, int W, int domain, int K, int radius, int wrap_x,
                                    void* d_out, float* d_scale, float* d_shift, int* d_nbr, int64_t* d_stats, void* stream) {
  VIPE_CHECK_ARG(dtype == VIPE_F16 || dtype == VIPE_F32);
  VIPE_CHECK_ARG(domain == VIPE_COMPLETE_DISP || domain == VIPE_COMPLETE_DEPTH);
  VIPE_CHECK_ARG(K >= 1 && K <= MAX_K);
  VIPE_CHECK_ARG(radius >= 1 && radius <= MAX_R);
  VIPE_CHECK_ARG(wrap_x == 0 || wrap_x == 1);
  const int64_t tiles = tiles_of(B, H, W);
  VIPE_CHECK_ARG(tiles > 0 && tiles <= 0x7fffffff);
  VIPE_CHECK_ARG(!wrap_x || W >= 2 * radius + 1);
  if (B == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_sparse && d_pred && d_bits && d_out && d_stats);
  CompleteArgs a;
  a.sparse = d_sparse; a.pred = d_pred; a.mask = d_mask; a.bits = (const u64*)d_bits; a.out = d_out;
  a.scale = d_scale; a.shift = d_shift; a.nbr = d_nbr; a.stats = (u64*)d_stats;
  a.H = H; a.W = W; a.nw = (W + 63) / 64; a.R = radius; a.tiles_x = (W + TILE_W - 1) / TILE_W;
  a.depth_domain = domain == VIPE_COMPLETE_DEPTH; a.wrap = wrap_x;
  const dim3 grid((unsigned)tiles, B);
  hipStream_t s = as_stream(stream);
  if (dtype == VIPE_F32) launch_complete<float>(K, grid, s, a);
  else launch_complete<half_t>(K, grid, s, a);
  return vipe_launch_status();
}
