// Learned convex upsampling of a 1/8-resolution map (DROID-SLAM's cvx_upsample, the consumer of GraphAgg.upmask):
//
//   out[r, 8y+dy, 8x+dx, c] = sum_k softmax_k(mask[s, y, x, k*64 + dy*8 + dx]) * data[r, y+ky-1, x+kx-1, c]
//
// with k = ky*3 + kx, data read as zero outside the grid, r = rows[s] (or s).  The softmax runs in f32 with the maximum
// subtracted: nine expf (1 ulp), the numerator as one chain of fused multiply-adds over the taps, the denominator as a
// chain of additions, ONE correctly rounded division per output value - tests/cvx_reference.py derives the error bound
// from exactly this operation count.
//
// The kernel is memory bound: per coarse pixel 1152 B of fp16 mask in, 256 * C B out.  Layout: the mask rows of
// consecutive coarse pixels (s, y, x) are contiguous in memory, so the grid is flat over N*h*w coarse pixels, 16 per
// workgroup of 256 threads, 4 per wave.  A thread owns 4 x-adjacent sub-pixels (dy, 4*dxg .. 4*dxg+3) of one coarse
// pixel:
//   - mask: per tap it reads its 4 logits as one 8-byte (fp16) or 16-byte (f32) load; the 16 threads of a coarse pixel
//     cover that tap's 64 logits = one whole 128-byte line (fp16), a wave-instruction reads four such lines and the nine
//     tap loads are independent (all in flight before the first use).  A lane-per-sub-pixel mapping would read the same
//     lines 2 bytes per lane.
//   - out: 4*C contiguous floats per thread, stored as C 16-byte vectors; within a wave the lanes (dxg, coarse pixel)
//     of one dy are x-adjacent, so a store wave-instruction writes 8 output rows x 128*C contiguous bytes (whole lines)
//     instead of the 32*C bytes one coarse pixel contributes to a row.
//   - data: the 3 x 3 x C neighbourhood is the same address for the 16 threads of a coarse pixel (broadcast loads that
//     hit in L1; 36*C B per coarse pixel against 1152 B of mask).
// Rows that `rows` does not name are not touched; a row index outside [0, R) skips its mask row (bounded writes).
#include "common.cuh"

namespace {

constexpr int CVX_THREADS = 256;
constexpr int CVX_PIXELS = CVX_THREADS / 16;  // coarse pixels per workgroup

typedef half_t cvx_half4 __attribute__((ext_vector_type(4)));
typedef float cvx_float4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ cvx_float4 load4(const float* p) { return *(const cvx_float4*)p; }
__device__ __forceinline__ cvx_float4 load4(const half_t* p) {
  const cvx_half4 v = *(const cvx_half4*)p;
  cvx_float4 o;
  o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2]; o[3] = (float)v[3];
  return o;
}

template <typename MT, int C>
__global__ __launch_bounds__(CVX_THREADS) void convex_upsample_kernel(const MT* __restrict__ mask,
                                                                      const float* __restrict__ data,
                                                                      float* __restrict__ out,
                                                                      const int64_t* __restrict__ rows, int64_t total,
                                                                      int R, int h, int w) {
  const int t = threadIdx.x;
  const int dxg = t & 1, dy = (t >> 1) & 7;
  const int64_t g = (int64_t)blockIdx.x * CVX_PIXELS + (t >> 4);  // coarse pixel (s, y, x), flat
  if (g >= total) return;
  const int hw = h * w;
  const int64_t s = g / hw;
  const int rem = (int)(g - s * hw);
  const int y = rem / w, x = rem - y * w;
  const int64_t r = rows ? rows[s] : s;
  if (r < 0 || r >= R) return;

  // the nine taps' logits of this thread's four sub-pixels
  const MT* m = mask + g * 576 + dy * 8 + dxg * 4;
  cvx_float4 l[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) l[k] = load4(m + k * 64);

  // the neighbourhood, zero outside the grid
  const float* dr = data + r * (int64_t)hw * C;
  float d[9][C];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int yy = y + ky - 1, xx = x + kx - 1;
      const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
      const float* p = dr + ((int64_t)(in ? yy : y) * w + (in ? xx : x)) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) d[ky * 3 + kx][c] = in ? p[c] : 0.0f;
    }
  }

  float res[4][C];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float mx = l[0][j];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, l[k][j]);
    float den = 0.0f, num[C];
#pragma unroll
    for (int c = 0; c < C; ++c) num[c] = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float e = expf(l[k][j] - mx);
      den = k == 0 ? e : den + e;
#pragma unroll
      for (int c = 0; c < C; ++c) num[c] = __fmaf_rn(e, d[k][c], num[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) res[j][c] = num[c] / den;
  }

  // 4*C contiguous floats at out[r, 8y+dy, 8x+4dxg, 0]
  const int64_t W8 = (int64_t)w * 8;
  float* o = out + ((r * ((int64_t)h * 8) + (y * 8 + dy)) * W8 + (x * 8 + dxg * 4)) * C;
  const float* flat = &res[0][0];
#pragma unroll
  for (int v = 0; v < C; ++v) {
    cvx_float4 q;
    q[0] = flat[4 * v]; q[1] = flat[4 * v + 1]; q[2] = flat[4 * v + 2]; q[3] = flat[4 * v + 3];
    *(cvx_float4*)(o + 4 * v) = q;
  }
}

template <typename MT>
void launch(const void* mask, const float* data, float* out, const int64_t* rows, int64_t total, int R, int h, int w,
            int C, hipStream_t s) {
  const unsigned grid = (unsigned)((total + CVX_PIXELS - 1) / CVX_PIXELS);
  const MT* m = (const MT*)mask;
  switch (C) {
    case 1: convex_upsample_kernel<MT, 1><<<grid, CVX_THREADS, 0, s>>>(m, data, out, rows, total, R, h, w); break;
    case 2: convex_upsample_kernel<MT, 2><<<grid, CVX_THREADS, 0, s>>>(m, data, out, rows, total, R, h, w); break;
    case 3: convex_upsample_kernel<MT, 3><<<grid, CVX_THREADS, 0, s>>>(m, data, out, rows, total, R, h, w); break;
    default: convex_upsample_kernel<MT, 4><<<grid, CVX_THREADS, 0, s>>>(m, data, out, rows, total, R, h, w); break;
  }
}

}  // namespace

VIPE_EXPORT int vipe_convex_upsample(const void* d_mask, int mask_dtype, const float* d_data, float* d_out,
                                     const int64_t* d_rows, int N, int R, int h, int w, int C, void* stream) {
  VIPE_CHECK_ARG(N >= 0 && R >= 0 && h > 0 && w > 0 && C >= 1);
  VIPE_CHECK_ARG(mask_dtype == VIPE_F16 || mask_dtype == VIPE_F32);
  if (C > 4) return VIPE_EUNSUPPORTED;
  if (N == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_mask && d_data && d_out);
  VIPE_CHECK_ARG((((uintptr_t)d_mask | (uintptr_t)d_out) & 15) == 0);  // vector loads / stores
  VIPE_CHECK_ARG(d_rows || N <= R);
  VIPE_CHECK_ARG((int64_t)h * w <= (1 << 28));  // 8h * 8w output pixels per row of `out` stay below 2^34: int64 offsets
  const int64_t total = (int64_t)N * h * w;
  VIPE_CHECK_ARG((total + CVX_PIXELS - 1) / CVX_PIXELS <= 0x7fffffffLL);
  hipStream_t s = as_stream(stream);
  if (mask_dtype == VIPE_F16) launch<half_t>(d_mask, d_data, d_out, d_rows, total, R, h, w, C, s);
  else launch<float>(d_mask, d_data, d_out, d_rows, total, R, h, w, C, s);
  return vipe_launch_status();
}
