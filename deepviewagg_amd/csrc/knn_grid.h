// The uniform hash grid of the exact neighbour searches (knn.hip, nearest_seen.hip): cell keys, the open-addressing cell
// table and the squared distance whose rounding the search contracts name.
#pragma once
#include "dva_common.h"

namespace dva {

constexpr int CELL_BITS = 21;
constexpr int64_t CELL_BIAS = 1 << 20;

__device__ __forceinline__ uint64_t cell_key(int64_t cx, int64_t cy, int64_t cz) {
  return ((uint64_t)(cx + CELL_BIAS) << (2 * CELL_BITS)) | ((uint64_t)(cy + CELL_BIAS) << CELL_BITS) |
         (uint64_t)(cz + CELL_BIAS);
}
__device__ __forceinline__ uint32_t hash64(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return (uint32_t)k;
}
__device__ __forceinline__ int cell_of(float p, float origin, float inv_cell) {
  return (int)floorf((p - origin) * inv_cell);
}

// first sorted position of the cell with key k, -1 when the cell is empty
__device__ __forceinline__ int cell_start(const uint64_t* __restrict__ tkeys, const int32_t* __restrict__ tvals,
                                          uint32_t mask, uint64_t k) {
  uint32_t h = hash64(k) & mask;
  for (;;) {
    const uint64_t t = tkeys[h];
    if (t == k) return tvals[h];
    if (t == ~0ULL) return -1;
    h = (h + 1) & mask;
  }
}

// d2 = ((dx*dx + dy*dy) + dz*dz) in fp32, every operation rounded on its own (the sources are built with
// -ffp-contract=off; the intrinsics hold it under any flag)
__device__ __forceinline__ float dist2_f32(float qx, float qy, float qz, float px, float py, float pz) {
  const float ex = __fsub_rn(qx, px), ey = __fsub_rn(qy, py), ez = __fsub_rn(qz, pz);
  return __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
}

}  // namespace dva
