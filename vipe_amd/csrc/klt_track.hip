// Sparse keypoint tracker: gray pyramid, min-eigenvalue corner detection per cell, pyramidal Lucas-Kanade in the
// inverse-compositional form.  include/vipe_amd.h states the arithmetic operation by operation (tests/klt_reference.py
// restates it in float64); this file keeps to it: f32 throughout, no contraction (the library is built with
// -ffp-contract=off), border replication through clamped indices on EVERY read - a position that is NaN or far outside
// the image still reads inside it.
//
// The work is small and latency bound (a frame is L + 3 launches of this file, about a thousand waves of tracking):
//   pyramid  level 0 is the one pass over the frame: four pixels per thread, 12 B (u8) / 48 B (f32) in as 4- / 16-byte
//            loads, one 16-byte store.  A further level is a quarter of the one before: one output pixel per thread, its
//            5 x 5 taps come out of L1 / L2.
//   detect   one workgroup per cell.  The gradient products of the cell and its 2-pixel apron go to LDS once (each is read
//            by up to 25 box sums), every thread then forms the box sums of its pixels in a fixed order and keeps its
//            best; the cell's best is an order-fixed (response, then lowest pixel index) wave + LDS reduction.
//   track    one wave per point, four points per workgroup, all levels in one launch.  The (2r+1)^2 window pixels are
//            dealt over the 64 lanes (r = 4: 81 -> two per lane, r = 7: 225 -> four), template and gradients stay in
//            registers for the iterations of a level, the sums go through xor butterflies, which leave the same bits in
//            every lane: the iteration count and every decision are wave-uniform.  No LDS.
#include "common.cuh"

namespace {

constexpr int KLT_MAX_LEVELS = 6;
constexpr int KLT_THREADS = 256;

struct KltLevels {
  int h[KLT_MAX_LEVELS], w[KLT_MAX_LEVELS];
  int64_t off[KLT_MAX_LEVELS];
};

KltLevels klt_levels(int H, int W, int L) {
  KltLevels lv = {};
  int64_t off = 0;
  for (int l = 0; l < L; ++l) {
    lv.h[l] = H, lv.w[l] = W, lv.off[l] = off;
    off += (int64_t)H * W;
    H = (H + 1) / 2, W = (W + 1) / 2;
  }
  return lv;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ float lambda_min(float a, float b, float c) {
  const float hd = 0.5f * (a - c);
  return 0.5f * (a + c) - sqrtf(hd * hd + b * b);
}

// ---------------------------------------------------------------------------------------------------------- pyramid
typedef float klt_float4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gray_of(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }

// four pixels (12 channel values) starting at pixel i, on the scale of the input
__device__ __forceinline__ void load12(const unsigned char* rgb, int64_t i, float* v) {
  const uint32_t* p = (const uint32_t*)(rgb + i * 3);  // i % 4 == 0: 12-byte steps from a 16-byte aligned base
  const uint32_t q[3] = {p[0], p[1], p[2]};
#pragma unroll
  for (int k = 0; k < 12; ++k) v[k] = (float)((q[k >> 2] >> (8 * (k & 3))) & 0xffu);
}
__device__ __forceinline__ void load12(const float* rgb, int64_t i, float* v) {
  const klt_float4* p = (const klt_float4*)(rgb + i * 3);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const klt_float4 q = p[k];
    v[4 * k] = q[0], v[4 * k + 1] = q[1], v[4 * k + 2] = q[2], v[4 * k + 3] = q[3];
  }
}
__device__ __forceinline__ float to255(unsigned char, float g) { return g; }
__device__ __forceinline__ float to255(float, float g) { return g * 255.0f; }

template <typename T>
__global__ __launch_bounds__(KLT_THREADS) void klt_gray_kernel(const T* rgb, float* out, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * KLT_THREADS + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n) {
    float v[12];
    load12(rgb, i, v);
    klt_float4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = to255(T{}, gray_of(v[3 * k], v[3 * k + 1], v[3 * k + 2]));
    *(klt_float4*)(out + i) = o;
  } else {
    for (int64_t j = i; j < n; ++j)
      out[j] = to255(T{}, gray_of((float)rgb[3 * j], (float)rgb[3 * j + 1], (float)rgb[3 * j + 2]));
  }
}

__device__ __forceinline__ float binom5(float p0, float p1, float p2, float p3, float p4) {
  return (((p0 + p4) + 4.0f * (p1 + p3)) + 6.0f * p2) * 0.0625f;
}

__global__ __launch_bounds__(KLT_THREADS) void klt_down_kernel(const float* src, int h, int w, float* dst, int h2, int w2) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w2 || y >= h2) return;
  int xs[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) xs[k] = clampi(2 * x + k - 2, 0, w - 1);
  float t[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float* r = src + (int64_t)clampi(2 * y + k - 2, 0, h - 1) * w;
    t[k] = binom5(r[xs[0]], r[xs[1]], r[xs[2]], r[xs[3]], r[xs[4]]);
  }
  dst[(int64_t)y * w2 + x] = binom5(t[0], t[1], t[2], t[3], t[4]);
}

// ----------------------------------------------------------------------------------------------------------- detect
constexpr int DET_MAX_CELL = 32;
constexpr int DET_TILE = DET_MAX_CELL + 4;

// (response, pixel index) pairs: larger response wins, then the lower index; index < 0 = nothing yet
__device__ __forceinline__ void take_better(float& r, int& i, float r2, int i2) {
  if (i2 >= 0 && (i < 0 || r2 > r || (r2 == r && i2 < i))) r = r2, i = i2;
}

__global__ __launch_bounds__(KLT_THREADS) void klt_detect_kernel(const float* __restrict__ img, int H, int W,
                                                                 const unsigned char* __restrict__ mask,
                                                                 const unsigned char* __restrict__ busy, int cell, int ncx,
                                                                 int border, float min_eig, float* __restrict__ out) {
  __shared__ float sa[DET_TILE * DET_TILE], sb[DET_TILE * DET_TILE], sc[DET_TILE * DET_TILE];
  __shared__ float wr[KLT_THREADS / WAVE];
  __shared__ int wi[KLT_THREADS / WAVE];
  const int t = threadIdx.x, cid = blockIdx.x;
  float* o = out + (int64_t)cid * 3;
  if (busy && busy[cid]) {  // uniform over the workgroup
    if (t == 0) o[0] = -1.0f, o[1] = -1.0f, o[2] = 0.0f;
    return;
  }
  const int x0 = (cid % ncx) * cell, y0 = (cid / ncx) * cell;
  const int cw = min(cell, W - x0), ch = min(cell, H - y0);
  const int tw = cw + 4, th = ch + 4;
  for (int i = t; i < tw * th; i += KLT_THREADS) {
    const int ty = i / tw, tx = i - ty * tw;
    const int x = x0 - 2 + tx, y = y0 - 2 + ty;
    float a = 0.0f, b = 0.0f, c = 0.0f;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const float* r = img + (int64_t)y * W;
      const float gx = 0.5f * (r[min(x + 1, W - 1)] - r[max(x - 1, 0)]);
      const float gy = 0.5f * (img[(int64_t)min(y + 1, H - 1) * W + x] - img[(int64_t)max(y - 1, 0) * W + x]);
      a = gx * gx, b = gx * gy, c = gy * gy;
    }
    sa[ty * DET_TILE + tx] = a, sb[ty * DET_TILE + tx] = b, sc[ty * DET_TILE + tx] = c;
  }
  __syncthreads();
  float best = 0.0f;
  int bidx = -1;
  for (int i = t; i < cw * ch; i += KLT_THREADS) {  // ascending pixel index per thread: `>` keeps the lowest of a tie
    const int py = i / cw, px = i - py * cw;
    const int x = x0 + px, y = y0 + py;
    if (x < border || x > W - 1 - border || y < border || y > H - 1 - border) continue;
    if (mask && !mask[(int64_t)y * W + x]) continue;
    float a = 0.0f, b = 0.0f, c = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int k = (py + dy) * DET_TILE + px + dx;
        a += sa[k], b += sb[k], c += sc[k];
      }
    }
    const float resp = lambda_min(a, b, c);
    if (resp / 25.0f >= min_eig && (bidx < 0 || resp > best)) best = resp, bidx = y * W + x;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const float r2 = __shfl_xor(best, s, WAVE);
    const int i2 = __shfl_xor(bidx, s, WAVE);
    take_better(best, bidx, r2, i2);
  }
  if (lane_id() == 0) wr[wave_id()] = best, wi[wave_id()] = bidx;
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < KLT_THREADS / WAVE; ++k) take_better(best, bidx, wr[k], wi[k]);
    if (bidx >= 0) o[0] = (float)(bidx % W), o[1] = (float)(bidx / W), o[2] = best;
    else o[0] = -1.0f, o[1] = -1.0f, o[2] = 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------------ track
constexpr int KLT_PER_LANE = 4;  // ceil(15 * 15 / 64)
constexpr int KLT_POINTS = KLT_THREADS / WAVE;

// bilinear sample with border replication; a NaN or far-away position still reads inside the image
__device__ __forceinline__ float klt_sample(const float* img, int h, int w, float x, float y) {
  const float flx = floorf(x), fly = floorf(y);
  const float fx = x - flx, fy = y - fly;
  const int xi = (int)fminf(fmaxf(flx, -1.0f), (float)w), yi = (int)fminf(fmaxf(fly, -1.0f), (float)h);
  const int xa = clampi(xi, 0, w - 1), xb = clampi(xi + 1, 0, w - 1);
  const float* r0 = img + (int64_t)clampi(yi, 0, h - 1) * w;
  const float* r1 = img + (int64_t)clampi(yi + 1, 0, h - 1) * w;
  const float v00 = r0[xa], v01 = r0[xb], v10 = r1[xa], v11 = r1[xb];
  const float top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10);
  return top + fy * (bot - top);
}

struct KltTrackArgs {
  const float *pyr_a, *pyr_b, *pts, *fb_ref;
  const unsigned char* mask;
  float *out, *resid;
  unsigned char *status, *busy;
  KltLevels lv;
  int H, W, L, N, r, n_iters, border, cell;
  float eps, min_eig, max_residual, fb_thresh, max_flow;
};

__device__ __forceinline__ bool inside(float x, float y, float b, int w, int h) {  // false for NaN
  return x >= b && x <= (float)(w - 1) - b && y >= b && y <= (float)(h - 1) - b;
}

__global__ __launch_bounds__(KLT_THREADS) void klt_track_kernel(const KltTrackArgs a) {
  const int n = blockIdx.x * KLT_POINTS + wave_id();
  if (n >= a.N) return;  // whole waves leave
  const int lane = lane_id();
  const int side = 2 * a.r + 1, nwin = side * side;
  const float px = a.pts[2 * n], py = a.pts[2 * n + 1];
  float ox[KLT_PER_LANE], oy[KLT_PER_LANE];
  bool on[KLT_PER_LANE];
#pragma unroll
  for (int k = 0; k < KLT_PER_LANE; ++k) {
    const int i = k * WAVE + lane;
    on[k] = i < nwin;
    ox[k] = (float)(i % side - a.r), oy[k] = (float)(i / side - a.r);
  }
  float tI[KLT_PER_LANE], tx[KLT_PER_LANE], ty[KLT_PER_LANE];
  float dx = 0.0f, dy = 0.0f, ga = 0.0f, gb = 0.0f, gc = 0.0f;
  bool oob = false;
  for (int l = a.L - 1; l >= 0; --l) {
    const float scale = 1.0f / (float)(1 << l);
    const float cx = px * scale, cy = py * scale;
    const int h = a.lv.h[l], w = a.lv.w[l];
    const float* A = a.pyr_a + a.lv.off[l];
    const float* B = a.pyr_b + a.lv.off[l];
    ga = gb = gc = 0.0f;
#pragma unroll
    for (int k = 0; k < KLT_PER_LANE; ++k) {
      tI[k] = tx[k] = ty[k] = 0.0f;
      if (on[k]) {
        const float sx = cx + ox[k], sy = cy + oy[k];
        tI[k] = klt_sample(A, h, w, sx, sy);
        tx[k] = 0.5f * (klt_sample(A, h, w, sx + 1.0f, sy) - klt_sample(A, h, w, sx - 1.0f, sy));
        ty[k] = 0.5f * (klt_sample(A, h, w, sx, sy + 1.0f) - klt_sample(A, h, w, sx, sy - 1.0f));
        ga += tx[k] * tx[k], gb += tx[k] * ty[k], gc += ty[k] * ty[k];
      }
    }
    ga = wave_sum(ga), gb = wave_sum(gb), gc = wave_sum(gc);
    const float det = ga * gc - gb * gb;
    for (int it = 0; it < a.n_iters; ++it) {
      const float qx = cx + dx, qy = cy + dy;
      float bx = 0.0f, by = 0.0f;
#pragma unroll
      for (int k = 0; k < KLT_PER_LANE; ++k) {
        if (on[k]) {
          const float e = tI[k] - klt_sample(B, h, w, qx + ox[k], qy + oy[k]);
          bx += e * tx[k], by += e * ty[k];
        }
      }
      bx = wave_sum(bx), by = wave_sum(by);
      float ux = 0.0f, uy = 0.0f;
      if (det > 0.0f) ux = (gc * bx - gb * by) / det, uy = (ga * by - gb * bx) / det;
      dx += ux, dy += uy;
      if (a.eps > 0.0f && ux * ux + uy * uy < a.eps * a.eps) break;
    }
    const float bl = (float)a.border * scale;
    if (!inside(cx, cy, bl, w, h) || !inside(cx + dx, cy + dy, bl, w, h)) oob = true;
    if (l > 0) dx *= 2.0f, dy *= 2.0f;
  }
  const float qx = px + dx, qy = py + dy;
  float res = 0.0f;
#pragma unroll
  for (int k = 0; k < KLT_PER_LANE; ++k)
    if (on[k]) res += fabsf(tI[k] - klt_sample(a.pyr_b, a.H, a.W, qx + ox[k], qy + oy[k]));
  res = wave_sum(res) / (float)nwin;
  if (lane != 0) return;

  a.out[2 * n] = qx, a.out[2 * n + 1] = qy;
  a.resid[n] = res;
  if (!a.fb_ref) {
    int st = oob ? VIPE_KLT_OOB : 0;
    if (lambda_min(ga, gb, gc) / (float)nwin < a.min_eig) st |= VIPE_KLT_LOW_TEXTURE;
    if (res > a.max_residual) st |= VIPE_KLT_RESIDUAL;
    if (!(isfinite(dx) && isfinite(dy)) || dx * dx + dy * dy > a.max_flow * a.max_flow) st |= VIPE_KLT_DIVERGED;
    if (a.mask) {
      const float rx = floorf(qx + 0.5f), ry = floorf(qy + 0.5f);
      if (rx >= 0.0f && rx <= (float)(a.W - 1) && ry >= 0.0f && ry <= (float)(a.H - 1) &&
          !a.mask[(int64_t)ry * a.W + (int64_t)rx])
        st |= VIPE_KLT_MASKED;
    }
    a.status[n] = (unsigned char)st;
  } else {
    const float ex = qx - a.fb_ref[2 * n], ey = qy - a.fb_ref[2 * n + 1];
    int st = a.status[n];
    if (!(ex * ex + ey * ey <= a.fb_thresh * a.fb_thresh)) st |= VIPE_KLT_FB;
    a.status[n] = (unsigned char)st;
    if (st == 0 && a.busy) {  // status 0: the forward position lies inside the border, so inside the image
      const int ix = clampi((int)floorf(px + 0.5f), 0, a.W - 1), iy = clampi((int)floorf(py + 0.5f), 0, a.H - 1);
      a.busy[(iy / a.cell) * ((a.W + a.cell - 1) / a.cell) + ix / a.cell] = 1;
    }
  }
}

}  // namespace

VIPE_EXPORT int vipe_klt_pyramid(const void* d_rgb, int rgb_dtype, int H, int W, int L, float* d_pyr, void* stream) {
  VIPE_CHECK_ARG(d_rgb && d_pyr && H > 0 && W > 0 && L >= 1 && L <= KLT_MAX_LEVELS);
  VIPE_CHECK_ARG(rgb_dtype == VIPE_U8 || rgb_dtype == VIPE_F32);
  VIPE_CHECK_ARG((int64_t)H * W <= (1 << 28));
  VIPE_CHECK_ARG((((uintptr_t)d_rgb | (uintptr_t)d_pyr) & 15) == 0);  // vector loads / stores of level 0
  hipStream_t s = as_stream(stream);
  const KltLevels lv = klt_levels(H, W, L);
  const int64_t n = (int64_t)H * W;
  const unsigned grid = (unsigned)((n + 4 * KLT_THREADS - 1) / (4 * KLT_THREADS));
  if (rgb_dtype == VIPE_U8) klt_gray_kernel<unsigned char><<<grid, KLT_THREADS, 0, s>>>((const unsigned char*)d_rgb, d_pyr, n);
  else klt_gray_kernel<float><<<grid, KLT_THREADS, 0, s>>>((const float*)d_rgb, d_pyr, n);
  for (int l = 1; l < L; ++l) {
    const dim3 g((lv.w[l] + 63) / 64, (lv.h[l] + 3) / 4);
    klt_down_kernel<<<g, KLT_THREADS, 0, s>>>(d_pyr + lv.off[l - 1], lv.h[l - 1], lv.w[l - 1], d_pyr + lv.off[l], lv.h[l],
                                              lv.w[l]);
  }
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_klt_detect(const float* d_img, int H, int W, const unsigned char* d_mask,
                                const unsigned char* d_cell_busy, int cell, int border, float min_eig, float* d_out,
                                void* stream) {
  VIPE_CHECK_ARG(d_img && d_out && H > 0 && W > 0 && border >= 0);
  VIPE_CHECK_ARG(cell >= 4 && cell <= DET_MAX_CELL);
  VIPE_CHECK_ARG((int64_t)H * W <= (1 << 28));  // pixel indices are ints
  const int ncx = (W + cell - 1) / cell, ncy = (H + cell - 1) / cell;
  klt_detect_kernel<<<ncx * ncy, KLT_THREADS, 0, as_stream(stream)>>>(d_img, H, W, d_mask, d_cell_busy, cell, ncx, border,
                                                                      min_eig, d_out);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_klt_track(const float* d_pyr_a, const float* d_pyr_b, int H, int W, int L, const float* d_pts, int N,
                               const float* d_fb_ref, const unsigned char* d_mask, int win_radius, int n_iters, float eps,
                               int border, float min_eig, float max_residual, float fb_thresh, float max_flow, int cell,
                               float* d_out, unsigned char* d_status, float* d_resid, unsigned char* d_cell_busy,
                               void* stream) {
  VIPE_CHECK_ARG(N >= 0 && H > 0 && W > 0 && L >= 1 && L <= KLT_MAX_LEVELS);
  VIPE_CHECK_ARG(win_radius >= 2 && win_radius <= 7 && n_iters >= 1 && n_iters <= 100);
  VIPE_CHECK_ARG(border >= 0 && eps >= 0.0f && (int64_t)H * W <= (1 << 28));
  VIPE_CHECK_ARG(!(d_fb_ref && d_cell_busy) || cell >= 4);
  if (N == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_pyr_a && d_pyr_b && d_pts && d_out && d_status && d_resid);
  KltTrackArgs a;
  a.pyr_a = d_pyr_a, a.pyr_b = d_pyr_b, a.pts = d_pts, a.fb_ref = d_fb_ref;
  a.mask = d_mask, a.out = d_out, a.resid = d_resid, a.status = d_status, a.busy = d_cell_busy;
  a.lv = klt_levels(H, W, L);
  a.H = H, a.W = W, a.L = L, a.N = N, a.r = win_radius, a.n_iters = n_iters, a.border = border, a.cell = cell;
  a.eps = eps, a.min_eig = min_eig, a.max_residual = max_residual, a.fb_thresh = fb_thresh, a.max_flow = max_flow;
  klt_track_kernel<<<(N + KLT_POINTS - 1) / KLT_POINTS, KLT_THREADS, 0, as_stream(stream)>>>(a);
  return vipe_launch_status();
}
