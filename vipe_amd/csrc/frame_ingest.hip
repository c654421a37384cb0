// Native-resolution frame ingest (vipe/slam/system.py:42-77, 183-205 and vipe/streams/base.py:164-254 of the reference):
// what `StandardResizeStreamProcessor` + `_precompute_features` + `_add_keyframe` make of one decoded frame, in ONE pass
// over it.  Per view
//
//   rgb [H0,W0,3] (u8 / f16 / f32) --bilinear (h1,w1)--> crop (top,left,H,W) --> images [3,H,W] f32   (buffer.images)
//                                                                           \--> x4 [H,W,4] f16       (enc_prep's output)
//   mask [H0,W0] bytes --bilinear (h1,w1) > 0.9--> crop --bilinear 1/8 > 0.9, inverted--> mask8 [H/8,W/8]  (True = invalid)
//   depth [H0,W0] f32 --bilinear (h1,w1)--> crop --[3::8,3::8]--> d > 0 ? 1/d : d --> disps_sens [H/8,W/8]
//
// The resample is F.interpolate(mode="bilinear", size=...) of torch: align_corners=False, no antialiasing,
//   scale = float(in) / float(out),  src = max(fma(scale, dst + 0.5, -0.5), 0),  i0 = int(src),  i1 = min(i0 + 1, in - 1),
//   l1 = src - i0, l0 = 1 - l1,      out = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
// `src` is ONE fused multiply-add, written as the intrinsic so that it is one whatever the flags (the library is built
// with -ffp-contract=off, so every other product and sum is rounded on its own): that is how torch's device kernel
// evaluates area_pixel_compute_source_index (device code is compiled with contraction on), and at coordinate 1900 one
// ulp of src is 1.2e-4 of lambda.  Measured on a 1080 x 1920 frame against F.interpolate on the same GPU: max |d| of
// the images 1.2e-7 with the fused src, 2.8e-5 with product and difference rounded separately (the latter by
// scratch/ingest_time.py --unfused-src, which resamples with that form in torch).  Against torch's host kernel (the
// fixture) the choice is invisible at the fixture's sizes: one ulp of src at coordinate 64 is 7.6e-6.
//
// Layout: one output pixel per thread, 64 x 4 pixel tiles (one wave per output row segment: a wave's taps walk two
// source rows front to back, its three plane stores are 256 contiguous bytes each and its x4 store 512).  The 1/8
// outputs come from the thread that owns cropped pixel (8i+3, 8j+3): the second mask stage samples at 8i+3.5 with
// lambda 0.5 in both directions, i.e. the mean of the 2 x 2 thresholded pixels at rows 8i+3, 8i+4 and columns 8j+3,
// 8j+4 - above 0.9 only when all four are valid - so that thread resamples those four mask pixels and one depth
// pixel; neither the resized mask nor the resized depth exists at full resolution anywhere.
#include "common.cuh"

namespace {

typedef half_t half4 __attribute__((ext_vector_type(4)));

constexpr int TILE_W = 64, TILE_H = 4;

struct IngestArgs {
  const void* rgb;             // [H0,W0,3]
  const unsigned char* mask;   // [H0,W0] or null
  const float* depth;          // [H0,W0] or null
  float* images;               // [3,H,W]
  half_t* x4;                  // [H,W,4]
  unsigned char* mask8;        // [H/8,W/8]
  float* disps_sens;           // [H/8,W/8]
  int H0, W0, top, left, H, W;
  float scale_y, scale_x;      // float(H0) / float(h1), float(W0) / float(w1)
};

struct Tap {
  int i0, i1;
  float l0, l1;
};

// area_pixel_compute_source_index + the index / lambda lines of upsample_bilinear2d (align_corners = false)
__device__ __forceinline__ Tap make_tap(int dst, float scale, int in) {
  float src = __fmaf_rn(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  Tap t;
  t.i0 = min((int)src, in - 1);
  t.i1 = min(t.i0 + 1, in - 1);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}

__device__ __forceinline__ float blend(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
  return ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * c + tx.l1 * d);
}

__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(half_t v) { return (float)v; }
__device__ __forceinline__ float to_float(unsigned char v) { return (float)v / 255.0f; }

// one plane [in_h, in_w] of floats / bytes-as-0-or-1 at the taps
__device__ __forceinline__ float sample_depth(const float* p, int W0, const Tap& ty, const Tap& tx) {
  const float* r0 = p + (int64_t)ty.i0 * W0;
  const float* r1 = p + (int64_t)ty.i1 * W0;
  return blend(ty, tx, r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1]);
}

__device__ __forceinline__ bool sample_mask_valid(const IngestArgs& a, int y, int x) {  // resized, cropped pixel (y, x)
  const Tap ty = make_tap(a.top + y, a.scale_y, a.H0), tx = make_tap(a.left + x, a.scale_x, a.W0);
  const unsigned char* r0 = a.mask + (int64_t)ty.i0 * a.W0;
  const unsigned char* r1 = a.mask + (int64_t)ty.i1 * a.W0;
  const float v = blend(ty, tx, r0[tx.i0] ? 1.0f : 0.0f, r0[tx.i1] ? 1.0f : 0.0f, r1[tx.i0] ? 1.0f : 0.0f,
                        r1[tx.i1] ? 1.0f : 0.0f);
  return v > 0.9f;
}

template <typename T>
__global__ __launch_bounds__(TILE_W* TILE_H) void frame_ingest_kernel(IngestArgs a) {
  const int x = blockIdx.x * TILE_W + (threadIdx.x & (TILE_W - 1));
  const int y = blockIdx.y * TILE_H + (threadIdx.x / TILE_W);
  if (x >= a.W || y >= a.H) return;
  const Tap ty = make_tap(a.top + y, a.scale_y, a.H0), tx = make_tap(a.left + x, a.scale_x, a.W0);
  const T* rgb = (const T*)a.rgb;
  const T* p00 = rgb + ((int64_t)ty.i0 * a.W0 + tx.i0) * 3;
  const T* p01 = rgb + ((int64_t)ty.i0 * a.W0 + tx.i1) * 3;
  const T* p10 = rgb + ((int64_t)ty.i1 * a.W0 + tx.i0) * 3;
  const T* p11 = rgb + ((int64_t)ty.i1 * a.W0 + tx.i1) * 3;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};  // enc_prep_kernel's
  const int64_t HW = (int64_t)a.H * a.W, p = (int64_t)y * a.W + x;
  half4 o;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = blend(ty, tx, to_float(p00[c]), to_float(p01[c]), to_float(p10[c]), to_float(p11[c]));
    a.images[c * HW + p] = v;
    o[c] = f2h((v - mean[c]) / stdv[c]);
  }
  o[3] = (half_t)0;
  *(half4*)(a.x4 + p * 4) = o;

  if ((y & 7) == 3 && (x & 7) == 3) {  // H, W are multiples of 8: (y + 1, x + 1) are inside the crop
    const int64_t q = (int64_t)(y >> 3) * (a.W >> 3) + (x >> 3);
    if (a.mask) {
      const bool valid = sample_mask_valid(a, y, x) && sample_mask_valid(a, y, x + 1) &&
                         sample_mask_valid(a, y + 1, x) && sample_mask_valid(a, y + 1, x + 1);
      a.mask8[q] = valid ? 0 : 1;
    }
    if (a.depth) {
      const float d = sample_depth(a.depth, a.W0, ty, tx);
      a.disps_sens[q] = d > 0.0f ? 1.0f / d : d;
    }
  }
}

}  // namespace

VIPE_EXPORT int vipe_frame_ingest(const void* d_rgb, int rgb_dtype, const unsigned char* d_mask, const float* d_depth,
                                  int H0, int W0, int h1, int w1, int top, int left, int H, int W, float* d_images,
                                  void* d_x4, unsigned char* d_mask8, float* d_disps_sens, void* stream) {
  VIPE_CHECK_ARG(d_rgb && d_images && d_x4);
  VIPE_CHECK_ARG(rgb_dtype == VIPE_F16 || rgb_dtype == VIPE_F32 || rgb_dtype == VIPE_U8);
  VIPE_CHECK_ARG(H0 > 0 && W0 > 0 && h1 > 0 && w1 > 0 && H > 0 && W > 0);
  VIPE_CHECK_ARG(H % 8 == 0 && W % 8 == 0 && top >= 0 && left >= 0);
  VIPE_CHECK_ARG((int64_t)top + H <= h1 && (int64_t)left + W <= w1);
  VIPE_CHECK_ARG((!d_mask || d_mask8) && (!d_depth || d_disps_sens));
  const int by = (H + TILE_H - 1) / TILE_H;
  VIPE_CHECK_ARG(by <= 65535);
  IngestArgs a;
  a.rgb = d_rgb; a.mask = d_mask; a.depth = d_depth;
  a.images = d_images; a.x4 = (half_t*)d_x4; a.mask8 = d_mask8; a.disps_sens = d_disps_sens;
  a.H0 = H0; a.W0 = W0; a.top = top; a.left = left; a.H = H; a.W = W;
  a.scale_y = (float)H0 / (float)h1;
  a.scale_x = (float)W0 / (float)w1;
  const dim3 grid((W + TILE_W - 1) / TILE_W, by);
  hipStream_t s = as_stream(stream);
  if (rgb_dtype == VIPE_F32) frame_ingest_kernel<float><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  else if (rgb_dtype == VIPE_F16) frame_ingest_kernel<half_t><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  else frame_ingest_kernel<unsigned char><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  return vipe_launch_status();
}
