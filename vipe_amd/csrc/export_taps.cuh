// The per-axis taps and the blend of the export geometry (the inverse of frame_ingest.hip's crop and resize), shared by
// depth_export.hip and depth_consistency.hip: both walk the native-size grid in 64 x 4 tiles, one output pixel per
// thread, and read a SLAM-resolution map through the same four taps.  The arithmetic is stated in depth_export.hip.
#pragma once
#include "common.cuh"

namespace export_geom {

constexpr int TILE_W = 64, TILE_H = 4;

struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap make_tap(int dst, float scale, int off, int in) {
  float src = __fmaf_rn(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  src = fminf(fmaxf(src - (float)off, 0.0f), (float)(in - 1));
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

// the geometry checks of both entry points: positive sizes, the crop inside the resized frame
static inline bool geometry_ok(int H, int W, int h1, int w1, int top, int left, int H0, int W0) {
  return H > 0 && W > 0 && h1 > 0 && w1 > 0 && H0 > 0 && W0 > 0 && top >= 0 && left >= 0 && (int64_t)top + H <= h1 &&
         (int64_t)left + W <= w1;
}

}  // namespace export_geom
