// Fused clip point cloud: the confident pixels of the exported depth maps, accumulated into a voxel hash table.
//
// vipe_cloud_fuse walks the native-size grid of depth_export.hip / depth_consistency.hip (same tiles, same taps, same
// blended disparity d), back-projects every pixel that takes part to the world and adds it to the voxel it falls in:
//
//   take    = x % stride == 0 and y % stride == 0 and (no conf or (conf & 15) >= min_agree) and d > 0
//   (u, v)  = (tx.i0 + tx.l1, ty.i0 + ty.l1)            the clamped source coordinate, as in depth_consistency.hip
//   ray     = cam::iproj<CAM>(I[view of r], u, v)
//   (R, t)  = to_rigid((rig[v]^-1 G[p])^-1)             camera -> world, built once per workgroup in LDS
//   Xw      = transform_ray<CAM>((R, t), ray, d) / d    three divisions; vipe_iproj's act(pose^-1, (ray, d)) / d
//   per axis: s = Xw * inv_voxel, i = floorf(s);  not (|i| < 2^20) (that includes every s that is not finite): the
//             point is counted out of range and dropped, before anything becomes an integer
//   key     = (ix + 2^20) | (iy + 2^20) << 21 | (iz + 2^20) << 42;   q = min(255, (int)((s - i) * 256.0f)) per axis
//   slot    = first slot from hash(key) on, linear and wrapping at cap, that holds the key or is empty (-1) and is
//             taken with one 64-bit atomicCAS; after PROBE_LIMIT (or cap) slots the point is counted as dropped.  A
//             thread never waits for another one: a lost CAS either shows the same key (use the slot) or another one
//             (next slot)
//   hash    = ((uint64)key * 0x9E3779B97F4A7C15 >> 32) & (cap - 1)
//   acc[slot] += {1, qx, qy, qz, r, g, b, 0} unless acc[slot].count reads >= 2^23 (then the point is counted as
//             saturated): the sums are 32-bit patterns read as unsigned, 255 * 2^24 < 2^32, and a count passes 2^23 by
//             no more than the points in flight (at most 2^19 resident threads)
//
// All accumulators are integers: the table's content (not which slot a key lives in) is independent of the order of the
// pixels, of the launches they come in, and of the run.
//
// Tile aggregation.  Neighbouring pixels mostly share voxels, and a scattered one-lane global atomic costs an order of
// magnitude more than an LDS one.  A workgroup therefore merges its 64 x 4 tile in an LDS hash of LDS_SLOTS entries
// (key + seven u32 sums, LDS atomics, at most LDS_PROBES probes), and thread t then sends entry t to the table with one
// insert and one set of global atomics.  A point that finds no LDS slot goes straight to the table.  With
// LDS_SLOTS = 0 the kernel is the direct form - every point straight to the table - which leaves the same table bit
// for bit; the library carries the aggregated one (DESIGN.md section 18 has both times; scratch/cloud_fuse_time.py
// builds the other from this file with -DVIPE_CLOUD_FUSE_LDS_SLOTS=0).
//
// vipe_cloud_extract: one thread per slot, kept slots claim their output position from a device counter (one atomic
// per wave).
#include "export_taps.cuh"
#include "term_geom.cuh"

#ifndef VIPE_CLOUD_FUSE_LDS_SLOTS
#define VIPE_CLOUD_FUSE_LDS_SLOTS 256
#endif

namespace {

using namespace export_geom;

constexpr int MAX_VIEWS = 8;
constexpr int LDS_SLOTS = VIPE_CLOUD_FUSE_LDS_SLOTS, LDS_PROBES = 8;
constexpr int PROBE_LIMIT = 128;
constexpr int AXIS_BIAS = 1 << 20;
constexpr unsigned SATURATED = 1u << 23;
constexpr long long EMPTY = -1;
static_assert(LDS_SLOTS == 0 || LDS_SLOTS == TILE_W * TILE_H, "thread t flushes LDS entry t");

using u64 = unsigned long long;

struct FuseArgs {
  const float *disp, *poses, *rig, *intr;  // [R,H,W], [R/V,7], [V,7], [V,idim]
  const int64_t* rows;                     // [N] or null
  const unsigned char* conf;               // [N,H0,W0] or null
  const void* rgb;                         // [N,H0,W0,3] or null
  long long* keys;                         // [cap]
  unsigned* acc;                           // [cap,8]
  u64* stats;                              // [4]
  int rgb_dtype, min_agree, stride, R, V, idim, H, W, H0, W0, top, left;
  unsigned cap_mask;
  int probe_limit;
  float scale_y, scale_x, inv_voxel;
};

enum { ST_INSERTED = 0, ST_FULL = 1, ST_RANGE = 2, ST_SATURATED = 3 };

__device__ __forceinline__ unsigned hash_start(long long key, unsigned mask) {
  return (unsigned)(((u64)key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

__device__ __forceinline__ unsigned colour_byte(const void* rgb, int dtype, int64_t i) {
  if (dtype == VIPE_U8) return ((const unsigned char*)rgb)[i];
  const float c = dtype == VIPE_F16 ? (float)((const half_t*)rgb)[i] : ((const float*)rgb)[i];
  return (unsigned)(int)(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f);  // a NaN clamps to 0
}

// n points with the sums v[1..6] into the table; counts what becomes of them in the workgroup's counters
__device__ __forceinline__ void table_add(const FuseArgs& a, long long key, const unsigned (&v)[7], unsigned* wg_stats) {
  unsigned slot = hash_start(key, a.cap_mask);
  bool found = false;
  for (int p = 0; p < a.probe_limit && !found; ++p) {
    long long k = __hip_atomic_load(a.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == EMPTY) {
      k = (long long)atomicCAS((u64*)(a.keys + slot), (u64)EMPTY, (u64)key);
      if (k == EMPTY) k = key;  // the slot is ours
    }
    found = k == key;
    if (!found) slot = (slot + 1) & a.cap_mask;
  }
  if (!found) {
    atomicAdd(wg_stats + ST_FULL, v[0]);
    return;
  }
  unsigned* row = a.acc + (size_t)slot * 8;
  if (__hip_atomic_load(row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= SATURATED) {
    atomicAdd(wg_stats + ST_SATURATED, v[0]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i)
    if (v[i]) atomicAdd(row + i, v[i]);
  atomicAdd(wg_stats + ST_INSERTED, v[0]);
}

template <int CAM>
__global__ __launch_bounds__(TILE_W* TILE_H) void cloud_fuse_kernel(FuseArgs a) {
  __shared__ Rigid Twc;
  __shared__ cam::Intr Ii;
  __shared__ unsigned wg_stats[4];
  __shared__ long long l_key[LDS_SLOTS > 0 ? LDS_SLOTS : 1];
  __shared__ unsigned l_sum[LDS_SLOTS > 0 ? LDS_SLOTS : 1][7];
  const int64_t n = blockIdx.z;
  const int64_t r = a.rows ? a.rows[n] : n;
  const bool row_ok = r >= 0 && r < a.R;  // workgroup-uniform
  if (!row_ok) return;
  if (threadIdx.x == 0) {
    using SE3f = lie::SE3<float>;
    const int p = (int)(r / a.V), v = (int)(r % a.V);
    Twc = to_rigid((SE3f(a.rig + 7 * v).inv() * SE3f(a.poses + 7 * p)).inv());
    Ii = cam::load<CAM>(a.intr + v * a.idim, a.idim - 4, 1.0f, a.H, a.W);
  }
  if (threadIdx.x < 4) wg_stats[threadIdx.x] = 0;
  if constexpr (LDS_SLOTS > 0) {
    l_key[threadIdx.x] = EMPTY;
#pragma unroll
    for (int i = 0; i < 7; ++i) l_sum[threadIdx.x][i] = 0;
  }
  __syncthreads();
  const int x = blockIdx.x * TILE_W + (threadIdx.x & (TILE_W - 1));
  const int y = blockIdx.y * TILE_H + (threadIdx.x / TILE_W);
  bool take = x < a.W0 && y < a.H0 && x % a.stride == 0 && y % a.stride == 0;
  const int64_t pix = take ? (n * a.H0 + y) * (int64_t)a.W0 + x : 0;
  if (take && a.conf) take = (int)(a.conf[pix] & 15) >= a.min_agree;
  float d = 0.0f;
  Tap ty, tx;
  if (take) {
    ty = make_tap(y, a.scale_y, a.top, a.H), tx = make_tap(x, a.scale_x, a.left, a.W);
    const float* m = a.disp + r * ((int64_t)a.H * a.W);
    const float* r0 = m + (int64_t)ty.i0 * a.W;
    const float* r1 = m + (int64_t)ty.i1 * a.W;
    d = blend(ty, tx, r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1]);
    take = d > 0.0f;  // false for a NaN
  }
  if (take) {
    const float u = (float)tx.i0 + tx.l1, v = (float)ty.i0 + ty.l1;  // exact: the clamped source coordinate
    float X0, Y0, Z0 = 1.0f, dX[1], dY[1], X[3];
    cam::iproj<CAM, 0>(Ii, u, v, X0, Y0, Z0, dX, dY);
    transform_ray<CAM>(Twc, X0, Y0, Z0, d, X[0], X[1], X[2]);
    long long key = 0;
    unsigned val[7] = {1, 0, 0, 0, 0, 0, 0};
    bool in_range = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float s = (X[i] / d) * a.inv_voxel;
      const float fi = floorf(s);
      in_range = in_range && fabsf(fi) < (float)AXIS_BIAS;  // false for anything that is not finite
      const float safe = in_range ? fi : 0.0f;
      key |= (long long)((int)safe + AXIS_BIAS) << (21 * i);
      val[1 + i] = (unsigned)min(255, (int)((in_range ? s - fi : 0.0f) * 256.0f));
    }
    if (!in_range) {
      atomicAdd(wg_stats + ST_RANGE, 1u);
    } else {
      if (a.rgb) {
#pragma unroll
        for (int i = 0; i < 3; ++i) val[4 + i] = colour_byte(a.rgb, a.rgb_dtype, pix * 3 + i);
      }
      bool merged = false;
      if constexpr (LDS_SLOTS > 0) {
        unsigned slot = hash_start(key, LDS_SLOTS - 1);
        for (int p = 0; p < LDS_PROBES && !merged; ++p) {
          long long k = __hip_atomic_load(l_key + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (k == EMPTY) {
            k = (long long)atomicCAS((u64*)(l_key + slot), (u64)EMPTY, (u64)key);
            if (k == EMPTY) k = key;
          }
          merged = k == key;
          if (!merged) slot = (slot + 1) & (LDS_SLOTS - 1);
        }
        if (merged) {
#pragma unroll
          for (int i = 0; i < 7; ++i)
            if (val[i]) atomicAdd(&l_sum[slot][i], val[i]);
        }
      }
      if (!merged) table_add(a, key, val, wg_stats);
    }
  }
  if constexpr (LDS_SLOTS > 0) {
    __syncthreads();
    const long long key = l_key[threadIdx.x];
    if (key != EMPTY) {
      unsigned val[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) val[i] = l_sum[threadIdx.x][i];
      table_add(a, key, val, wg_stats);
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && wg_stats[threadIdx.x]) atomicAdd(a.stats + threadIdx.x, (u64)wg_stats[threadIdx.x]);
}

struct ExtractArgs {
  const long long* keys;
  const unsigned* acc;
  float* xyz;
  unsigned char* rgb;
  int* count;
  long long* key;
  u64* num_out;
  int64_t cap, max_out;
  unsigned min_count;
  float voxel;
};

__global__ __launch_bounds__(256) void cloud_extract_kernel(ExtractArgs a) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  long long key = EMPTY;
  unsigned row[7] = {0, 0, 0, 0, 0, 0, 0};
  if (slot < a.cap) {
    key = a.keys[slot];
#pragma unroll
    for (int i = 0; i < 7; ++i) row[i] = a.acc[slot * 8 + i];
  }
  const bool keep = key != EMPTY && row[0] >= a.min_count;
  const u64 mask = __ballot(keep);
  if (mask == 0) return;  // wave-uniform
  const int lane = lane_id();
  const int first = __ffsll((long long)mask) - 1;
  u64 base = 0;
  if (lane == first) base = atomicAdd(a.num_out, (u64)__popcll(mask));
  base = __shfl(base, first, WAVE);
  const int64_t o = (int64_t)base + __popcll(mask & ((1ull << lane) - 1ull));
  if (!keep || o >= a.max_out) return;
  const double cnt = (double)row[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int idx = (int)((key >> (21 * i)) & 0x1fffff) - AXIS_BIAS;
    a.xyz[o * 3 + i] = (float)(((double)idx + ((double)row[1 + i] / cnt + 0.5) / 256.0) * (double)a.voxel);
  }
  if (a.rgb) {
#pragma unroll
    for (int i = 0; i < 3; ++i) a.rgb[o * 3 + i] = (unsigned char)(((u64)row[4 + i] + row[0] / 2) / row[0]);
  }
  a.count[o] = (int)row[0];
  a.key[o] = key;
}

inline bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

VIPE_EXPORT int vipe_cloud_fuse(const float* d_disp, const float* d_poses, const float* d_rig, const float* d_intrinsics,
                                int intr_dim, int camera, const int64_t* d_rows, const unsigned char* d_conf, int min_agree,
                                const void* d_rgb, int rgb_dtype, int stride, float inv_voxel, int64_t* d_keys, int* d_acc,
                                int64_t cap, int64_t* d_stats, int N, int R, int n_views, int H, int W, int h1, int w1,
                                int top, int left, int H0, int W0, void* stream) {
  VIPE_CHECK_ARG(N >= 0 && R >= 0);
  VIPE_CHECK_ARG(geometry_ok(H, W, h1, w1, top, left, H0, W0));
  VIPE_CHECK_ARG(n_views >= 1 && n_views <= MAX_VIEWS && R % n_views == 0);
  VIPE_CHECK_ARG(camera == VIPE_CAM_PINHOLE || camera == VIPE_CAM_MEI || camera == VIPE_CAM_PANORAMA);
  VIPE_CHECK_ARG(intr_dim == (camera == VIPE_CAM_MEI ? 5 : 4));
  if (camera == VIPE_CAM_PANORAMA) VIPE_CHECK_ARG(top == 0 && left == 0 && h1 == H && w1 == W);  // a crop breaks the sphere
  VIPE_CHECK_ARG(min_agree >= 0 && min_agree <= 8);
  VIPE_CHECK_ARG(stride >= 1 && stride <= 8);
  VIPE_CHECK_ARG(inv_voxel > 0.0f && inv_voxel <= 3.0e38f);  // positive and finite
  VIPE_CHECK_ARG(pow2(cap) && cap <= ((int64_t)1 << 30));
  VIPE_CHECK_ARG(!d_rgb || rgb_dtype == VIPE_F16 || rgb_dtype == VIPE_F32 || rgb_dtype == VIPE_U8);
  VIPE_CHECK_ARG(d_rows || N <= R);
  const int by = (H0 + TILE_H - 1) / TILE_H;
  VIPE_CHECK_ARG(by <= 65535 && N <= 65535);  // grid.y / grid.z: an error, not a silent truncation
  if (N == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_disp && d_poses && d_rig && d_intrinsics && d_keys && d_acc && d_stats);
  FuseArgs a;
  a.disp = d_disp; a.poses = d_poses; a.rig = d_rig; a.intr = d_intrinsics;
  a.rows = d_rows; a.conf = d_conf; a.rgb = d_rgb;
  a.keys = (long long*)d_keys; a.acc = (unsigned*)d_acc; a.stats = (u64*)d_stats;
  a.rgb_dtype = rgb_dtype; a.min_agree = min_agree; a.stride = stride;
  a.R = R; a.V = n_views; a.idim = intr_dim;
  a.H = H; a.W = W; a.H0 = H0; a.W0 = W0; a.top = top; a.left = left;
  a.cap_mask = (unsigned)(cap - 1);
  a.probe_limit = (int)(cap < PROBE_LIMIT ? cap : PROBE_LIMIT);
  a.scale_y = (float)h1 / (float)H0;
  a.scale_x = (float)w1 / (float)W0;
  a.inv_voxel = inv_voxel;
  const dim3 grid((W0 + TILE_W - 1) / TILE_W, by, N);
  hipStream_t s = as_stream(stream);
  if (camera == VIPE_CAM_PINHOLE) cloud_fuse_kernel<VIPE_CAM_PINHOLE><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  else if (camera == VIPE_CAM_MEI) cloud_fuse_kernel<VIPE_CAM_MEI><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  else cloud_fuse_kernel<VIPE_CAM_PANORAMA><<<grid, TILE_W * TILE_H, 0, s>>>(a);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_cloud_extract(const int64_t* d_keys, const int* d_acc, int64_t cap, float voxel, int min_count,
                                   float* d_xyz, unsigned char* d_rgb, int* d_count, int64_t* d_key, int64_t max_out,
                                   int64_t* d_num_out, void* stream) {
  VIPE_CHECK_ARG(pow2(cap) && cap <= ((int64_t)1 << 30));
  VIPE_CHECK_ARG(voxel > 0.0f && voxel <= 3.0e38f);
  VIPE_CHECK_ARG(min_count >= 1 && max_out >= 0);
  VIPE_CHECK_ARG(d_keys && d_acc && d_num_out);
  VIPE_CHECK_ARG(max_out == 0 || (d_xyz && d_count && d_key));  // d_rgb is optional: a cloud without colour
  ExtractArgs a;
  a.keys = (const long long*)d_keys; a.acc = (const unsigned*)d_acc;
  a.xyz = d_xyz; a.rgb = d_rgb; a.count = d_count; a.key = (long long*)d_key; a.num_out = (u64*)d_num_out;
  a.cap = cap; a.max_out = max_out; a.min_count = (unsigned)min_count; a.voxel = voxel;
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(d_num_out, 0, sizeof(int64_t), s) != hipSuccess) return vipe_launch_status();
  cloud_extract_kernel<<<(unsigned)((cap + 255) / 256), 256, 0, s>>>(a);
  return vipe_launch_status();
}
