// Geometry and addressing of VIPE_PYRAMID_BLOCKED (described in include/vipe_amd.h), written once for the kernel that
// stores it (corr_build.hip) and the kernel that reads it (corr_lookup.hip).
#pragma once
#include <stdint.h>

// The h x w grid padded to G groups of 64 source pixels, S strips of 32 target columns and R groups of 4 target rows
// (always even: whole level-1 tiles); nch = chunks of 4 x 32 targets, w2p / w3p = row pitches of the level-2 / 3 slabs.
struct BlockedDims {
  int G, S, R, nch, w2p, w3p;
  __host__ __device__ BlockedDims(int h, int w)
      : G((h * w + 63) / 64), S((w + 31) / 32), R(((h + 7) / 8) * 2), nch(S * R), w2p(8 * S), w3p((4 * S + 7) / 8 * 8) {}

  // source pixel p1 of `slot`, counted over the padded groups of all slots
  __host__ __device__ int64_t pixel(int64_t slot, int p1) const { return slot * (G * 64) + p1; }

  // Levels 0 / 1: offset in halves of the 16-byte piece (row y, columns 8 c .. 8 c + 7, level-l coordinates) of source pixel
  // p1 in `slot`: run ((x-strip) * (R >> l) + y / 4) of the pixel's group of 64, tile c % T, tile row y % 4 - the T = 4 >> l
  // tiles of a pixel's part of a run are contiguous, 4 pieces each
  __host__ __device__ int64_t piece01(int l, int64_t slot, int p1, int y, int c) const {
    const int T = 4 >> l, rgs = R >> l;
    const int64_t gp = pixel(slot, p1);  // group gp / 64, pixel gp % 64 of the group
    const int64_t run = (gp >> 6) * ((int64_t)rgs * S) + (c / T) * rgs + (y >> 2);
    return (run * 64 + (gp & 63)) * (T * 32) + (c % T) * 32 + (y & 3) * 8;
  }

  // Levels 2 / 3: one slab per source pixel of every group of 64: R >> (l - 2) rows of 8 S / round_up(4 S, 8) entries
  struct Slab { int64_t base; int rows, pitch; };  // base: offset in halves
  __host__ __device__ Slab slab23(int l, int64_t slot, int p1) const {
    const int rows = R >> (l - 2), pitch = l == 2 ? w2p : w3p;
    return {pixel(slot, p1) * ((int64_t)rows * pitch), rows, pitch};
  }
};
