// Multi-scale deformable attention (grounding_dino_ext: csrc/grounding_dino_ext/vision.cpp:9-33,
// ms_deform_attn_cuda.cu), written from the maths of multi_scale_deformable_attn_pytorch (ms_deform_attn.py:92-134):
//
//   out[b,q,h,c] = sum_{l,p} a[b,q,h,l,p] * bilinear(value[b, start_l : start_l + H_l*W_l, h, c] as H_l x W_l,
//                                                   x = loc_x * W_l - 0.5, y = loc_y * H_l - 0.5)
//
// with corners outside the level counting as zero (grid_sample, padding_mode="zeros", align_corners=False, on 2 loc - 1).
//
// Layout: one (b, q, h) group per G lanes of a wave, G = next power of two of min(C, 64), lanes over channels.  At the
// GroundingDINO shape (C = 32) a wave owns two heads of one query.  The group's L*P locations and weights are loaded
// once, one point per lane, and handed to the other lanes of the group by a lane shuffle; the level metadata (H, W,
// start) sits in LDS.  Every corner read of a wave-instruction is then one contiguous C-element row segment per group
// (two 128-B segments at C = 32, fp32), and the output is written by coalesced vector stores.
//
// Backward: grad_attn_weight and grad_sampling_loc sum over the C lanes of a group - a fixed xor-butterfly of lane
// shuffles, so these two are bitwise reproducible - and are written by plain stores, one point per lane.  grad_value
// is accumulated with float atomics (global_atomic_add_f32 / _f64, no compare-and-swap loop) in the same lane layout;
// its last bits depend on arrival order, as in the reference.
//
// Safety: a corner is read only if it lies inside its level AND inside [0, Lv) - levels whose (H, W, start) do not
// fit are treated as empty - so an inconsistent level_start_index cannot make the kernel read or write outside value.
// Offsets are 64-bit.
#include <limits.h>

#include "common.cuh"

namespace {

constexpr int MSDA_BLOCK = 256;
constexpr int MSDA_MAX_LEVELS = 1024;  // 16 B of LDS per level
constexpr int64_t MSDA_MAX_BLOCKS = 1 << 20;  // the kernels loop over waves beyond that
constexpr int64_t MSDA_MAX_SIDE = 1 << 30;    // larger H or W: the level is empty (corner arithmetic stays in int)

struct LevelMeta {
  int h, w;
  int64_t start;
};

__device__ __forceinline__ void msda_load_levels(LevelMeta* lv, const int64_t* __restrict__ shapes,
                                                 const int64_t* __restrict__ starts, int L, int64_t Lv) {
  for (int i = threadIdx.x; i < L; i += blockDim.x) {
    const int64_t h = shapes[2 * i], w = shapes[2 * i + 1], s = starts[i];
    const bool ok = h > 0 && w > 0 && h <= MSDA_MAX_SIDE && w <= MSDA_MAX_SIDE && s >= 0 && s <= Lv;
    LevelMeta m;
    m.h = ok ? (int)h : 0;
    m.w = ok ? (int)w : 0;
    m.start = ok ? s : 0;
    lv[i] = m;
  }
  __syncthreads();
}

// The four bilinear corners of pixel position (x, y) in level m: row index into value's [Lv] axis, or -1 when the corner
// lies outside the level or outside value.  Returns false when no corner can be inside (the reference's
// "h_im > -1 && w_im > -1 && h_im < H && w_im < W" test; also false for NaN).  Corner order: (y0,x0) (y0,x1) (y1,x0) (y1,x1).
template <typename T>
__device__ __forceinline__ bool msda_corners(T x, T y, const LevelMeta& m, int64_t Lv, int64_t (&p)[4], T& lx, T& ly) {
  if (!(x > T(-1) && y > T(-1) && x < T(m.w) && y < T(m.h))) return false;
  const T xf = floor(x), yf = floor(y);
  const int x0 = (int)xf, y0 = (int)yf;
  lx = x - xf;
  ly = y - yf;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
    const int64_t r = m.start + (int64_t)yy * m.w + xx;
    p[k] = (xx >= 0 && xx < m.w && yy >= 0 && yy < m.h && r < Lv) ? r : -1;
  }
  return true;
}

template <typename T>
__device__ __forceinline__ T msda_group_sum(T v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// value [bs, Lv, heads, C]; loc [bs, Lq, heads, L, P, 2]; attn [bs, Lq, heads, L, P]; out [bs, Lq, heads * C]
template <typename T>
__global__ __launch_bounds__(MSDA_BLOCK) void msda_forward_kernel(
    const T* __restrict__ value, const int64_t* __restrict__ shapes, const int64_t* __restrict__ starts,
    const T* __restrict__ loc, const T* __restrict__ attn, T* __restrict__ out, int64_t bs, int64_t Lv, int heads,
    int C, int L, int64_t Lq, int P, int lg) {
  extern __shared__ __align__(16) unsigned char msda_smem[];
  LevelMeta* lv = reinterpret_cast<LevelMeta*>(msda_smem);
  msda_load_levels(lv, shapes, starts, L, Lv);

  const int G = 1 << lg, lane = lane_id();
  const int gl = lane & (G - 1), gbase = lane & ~(G - 1), gpw = WAVE >> lg;
  const int LP = L * P;
  const int64_t ngroups = bs * Lq * heads, row = (int64_t)heads * C;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // the loop and every shuffle below are wave-uniform: groups past the end only mask their loads and stores
  for (int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv * gpw < ngroups; wv += nwaves) {
    const int64_t g = wv * gpw + (lane >> lg);
    const bool gv = g < ngroups;
    const int64_t b = g / (Lq * heads);
    const int h = (int)(g % heads);
    const T* vb = value + b * Lv * row + (int64_t)h * C;  // row r, channel c: vb[r * row + c]
    const T* gloc = loc + g * LP * 2;
    const T* gatt = attn + g * LP;
    for (int c0 = 0; c0 < C; c0 += G) {
      const int c = c0 + gl;
      const bool cv = gv && c < C;
      T acc = T(0);
      for (int k0 = 0; k0 < LP; k0 += G) {
        const int kk = k0 + gl;
        T mx = T(0), my = T(0), ma = T(0);
        if (gv && kk < LP) {
          mx = gloc[2 * kk];
          my = gloc[2 * kk + 1];
          ma = gatt[kk];
        }
        const int n = min(G, LP - k0);
        for (int j = 0; j < n; ++j) {
          const LevelMeta m = lv[(k0 + j) / P];
          const T x = __shfl(mx, gbase + j, WAVE) * T(m.w) - T(0.5);
          const T y = __shfl(my, gbase + j, WAVE) * T(m.h) - T(0.5);
          const T a = __shfl(ma, gbase + j, WAVE);
          int64_t p[4];
          T lx, ly;
          if (cv && msda_corners(x, y, m, Lv, p, lx, ly)) {
            const T hx = T(1) - lx, hy = T(1) - ly;
            const T v0 = p[0] >= 0 ? vb[p[0] * row + c] : T(0);
            const T v1 = p[1] >= 0 ? vb[p[1] * row + c] : T(0);
            const T v2 = p[2] >= 0 ? vb[p[2] * row + c] : T(0);
            const T v3 = p[3] >= 0 ? vb[p[3] * row + c] : T(0);
            const T val = hy * hx * v0 + hy * lx * v1 + ly * hx * v2 + ly * lx * v3;
            acc += a * val;
          }
        }
      }
      if (cv) out[g * C + c] = acc;
    }
  }
}

// grad_output [bs, Lq, heads * C] -> grad_value [bs, Lv, heads, C] (accumulated: zero it first), grad_loc
// [bs, Lq, heads, L, P, 2], grad_attn [bs, Lq, heads, L, P] (written)
template <typename T>
__global__ __launch_bounds__(MSDA_BLOCK) void msda_backward_kernel(
    const T* __restrict__ value, const int64_t* __restrict__ shapes, const int64_t* __restrict__ starts,
    const T* __restrict__ loc, const T* __restrict__ attn, const T* __restrict__ gout, T* __restrict__ gval,
    T* __restrict__ gloc_out, T* __restrict__ gatt_out, int64_t bs, int64_t Lv, int heads, int C, int L, int64_t Lq,
    int P, int lg) {
  extern __shared__ __align__(16) unsigned char msda_smem[];
  LevelMeta* lv = reinterpret_cast<LevelMeta*>(msda_smem);
  msda_load_levels(lv, shapes, starts, L, Lv);

  const int G = 1 << lg, lane = lane_id();
  const int gl = lane & (G - 1), gbase = lane & ~(G - 1), gpw = WAVE >> lg;
  const int LP = L * P;
  const int64_t ngroups = bs * Lq * heads, row = (int64_t)heads * C;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv * gpw < ngroups; wv += nwaves) {
    const int64_t g = wv * gpw + (lane >> lg);
    const bool gv = g < ngroups;
    const int64_t b = g / (Lq * heads);
    const int h = (int)(g % heads);
    const int64_t vofs = b * Lv * row + (int64_t)h * C;
    const T* vb = value + vofs;
    T* gvb = gval + vofs;
    const T* gloc = loc + g * LP * 2;
    const T* gatt = attn + g * LP;
    const T* gtop = gout + g * C;
    const T top0 = (gv && gl < C) ? gtop[gl] : T(0);  // channel chunk 0 (the only one for C <= 64)
    for (int k0 = 0; k0 < LP; k0 += G) {
      const int kk = k0 + gl;
      T mx = T(0), my = T(0), ma = T(0);
      if (gv && kk < LP) {
        mx = gloc[2 * kk];
        my = gloc[2 * kk + 1];
        ma = gatt[kk];
      }
      T keep_a = T(0), keep_x = T(0), keep_y = T(0);
      const int n = min(G, LP - k0);
      for (int j = 0; j < n; ++j) {
        const LevelMeta m = lv[(k0 + j) / P];
        const T x = __shfl(mx, gbase + j, WAVE) * T(m.w) - T(0.5);
        const T y = __shfl(my, gbase + j, WAVE) * T(m.h) - T(0.5);
        const T a = __shfl(ma, gbase + j, WAVE);
        int64_t p[4];
        T lx = T(0), ly = T(0);
        T sa = T(0), sx = T(0), sy = T(0);
        if (gv && msda_corners(x, y, m, Lv, p, lx, ly)) {
          const T hx = T(1) - lx, hy = T(1) - ly;
          const T w0 = hy * hx, w1 = hy * lx, w2 = ly * hx, w3 = ly * lx;
          for (int c0 = 0; c0 < C; c0 += G) {
            const int c = c0 + gl;
            if (c < C) {
              const T top = c0 == 0 ? top0 : gtop[c];
              const T v0 = p[0] >= 0 ? vb[p[0] * row + c] : T(0);
              const T v1 = p[1] >= 0 ? vb[p[1] * row + c] : T(0);
              const T v2 = p[2] >= 0 ? vb[p[2] * row + c] : T(0);
              const T v3 = p[3] >= 0 ? vb[p[3] * row + c] : T(0);
              sa += top * (w0 * v0 + w1 * v1 + w2 * v2 + w3 * v3);
              sx += top * (hy * (v1 - v0) + ly * (v3 - v2));  // d bilinear / dx
              sy += top * (hx * (v2 - v0) + lx * (v3 - v1));  // d bilinear / dy
              const T ta = top * a;
              if (p[0] >= 0) atomicAdd(gvb + p[0] * row + c, w0 * ta);
              if (p[1] >= 0) atomicAdd(gvb + p[1] * row + c, w1 * ta);
              if (p[2] >= 0) atomicAdd(gvb + p[2] * row + c, w2 * ta);
              if (p[3] >= 0) atomicAdd(gvb + p[3] * row + c, w3 * ta);
            }
          }
        }
        // every lane of the wave takes part in the butterflies (a group whose point is outside sums zeros)
        sa = msda_group_sum(sa, G);
        sx = msda_group_sum(sx, G);
        sy = msda_group_sum(sy, G);
        if (gl == j) {
          keep_a = sa;
          keep_x = sx * a * T(m.w);
          keep_y = sy * a * T(m.h);
        }
      }
      if (gv && kk < LP) {
        gatt_out[g * LP + kk] = keep_a;
        gloc_out[(g * LP + kk) * 2] = keep_x;
        gloc_out[(g * LP + kk) * 2 + 1] = keep_y;
      }
    }
  }
}

static int msda_lg(int C) {
  int lg = 0;
  while ((1 << lg) < C && lg < 6) ++lg;
  return lg;
}

static int msda_check(int64_t bs, int64_t Lv, int heads, int C, int L, int64_t Lq, int P, int dtype) {
  VIPE_CHECK_ARG(bs >= 0 && Lv >= 0 && Lq >= 0 && heads >= 1 && C >= 1 && L >= 1 && P >= 1);
  VIPE_CHECK_ARG(dtype == VIPE_F32 || dtype == VIPE_F64);
  return VIPE_OK;
}

static int msda_supported(int L, int P) {
  if (L > MSDA_MAX_LEVELS || (int64_t)L * P > INT_MAX / 2) return VIPE_EUNSUPPORTED;
  return VIPE_OK;
}

static dim3 msda_grid(int64_t bs, int64_t Lq, int heads, int lg) {
  const int64_t groups = bs * Lq * heads, gpw = WAVE >> lg;
  const int64_t waves = (groups + gpw - 1) / gpw, per_block = MSDA_BLOCK / WAVE;
  const int64_t blocks = (waves + per_block - 1) / per_block;
  return dim3((unsigned)(blocks < MSDA_MAX_BLOCKS ? blocks : MSDA_MAX_BLOCKS));
}

}  // namespace

VIPE_EXPORT int vipe_ms_deform_attn_forward(const void* d_value, const int64_t* d_spatial_shapes,
                                            const int64_t* d_level_start_index, const void* d_sampling_loc,
                                            const void* d_attn_weight, void* d_output, int64_t bs, int64_t Lv, int heads,
                                            int C, int L, int64_t Lq, int P, int dtype, void* stream) {
  int e = msda_check(bs, Lv, heads, C, L, Lq, P, dtype);
  if (e != VIPE_OK) return e;
  if (bs == 0 || Lq == 0) return VIPE_OK;
  VIPE_CHECK_ARG((d_value || Lv == 0) && d_spatial_shapes && d_level_start_index && d_sampling_loc && d_attn_weight &&
                 d_output);
  if ((e = msda_supported(L, P)) != VIPE_OK) return e;
  const int lg = msda_lg(C);
  const size_t lds = (size_t)L * sizeof(LevelMeta);
  const dim3 grid = msda_grid(bs, Lq, heads, lg);
  if (dtype == VIPE_F32)
    msda_forward_kernel<float><<<grid, MSDA_BLOCK, lds, as_stream(stream)>>>(
        (const float*)d_value, d_spatial_shapes, d_level_start_index, (const float*)d_sampling_loc,
        (const float*)d_attn_weight, (float*)d_output, bs, Lv, heads, C, L, Lq, P, lg);
  else
    msda_forward_kernel<double><<<grid, MSDA_BLOCK, lds, as_stream(stream)>>>(
        (const double*)d_value, d_spatial_shapes, d_level_start_index, (const double*)d_sampling_loc,
        (const double*)d_attn_weight, (double*)d_output, bs, Lv, heads, C, L, Lq, P, lg);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_ms_deform_attn_backward(const void* d_value, const int64_t* d_spatial_shapes,
                                             const int64_t* d_level_start_index, const void* d_sampling_loc,
                                             const void* d_attn_weight, const void* d_grad_output, void* d_grad_value,
                                             void* d_grad_sampling_loc, void* d_grad_attn_weight, int64_t bs,
                                             int64_t Lv, int heads, int C, int L, int64_t Lq, int P, int dtype,
                                             void* stream) {
  int e = msda_check(bs, Lv, heads, C, L, Lq, P, dtype);
  if (e != VIPE_OK) return e;
  if (bs == 0 || Lq == 0) return VIPE_OK;
  VIPE_CHECK_ARG((d_value || Lv == 0) && (d_grad_value || Lv == 0) && d_spatial_shapes && d_level_start_index &&
                 d_sampling_loc && d_attn_weight && d_grad_output && d_grad_sampling_loc && d_grad_attn_weight);
  if ((e = msda_supported(L, P)) != VIPE_OK) return e;
  const int lg = msda_lg(C);
  const size_t lds = (size_t)L * sizeof(LevelMeta);
  const dim3 grid = msda_grid(bs, Lq, heads, lg);
  if (dtype == VIPE_F32)
    msda_backward_kernel<float><<<grid, MSDA_BLOCK, lds, as_stream(stream)>>>(
        (const float*)d_value, d_spatial_shapes, d_level_start_index, (const float*)d_sampling_loc,
        (const float*)d_attn_weight, (const float*)d_grad_output, (float*)d_grad_value, (float*)d_grad_sampling_loc,
        (float*)d_grad_attn_weight, bs, Lv, heads, C, L, Lq, P, lg);
  else
    msda_backward_kernel<double><<<grid, MSDA_BLOCK, lds, as_stream(stream)>>>(
        (const double*)d_value, d_spatial_shapes, d_level_start_index, (const double*)d_sampling_loc,
        (const double*)d_attn_weight, (const double*)d_grad_output, (double*)d_grad_value,
        (double*)d_grad_sampling_loc, (double*)d_grad_attn_weight, bs, Lv, heads, C, L, Lq, P, lg);
  return vipe_launch_status();
}
