// What the entries of the mapping operations (merge, select, pick, collate) share: the host checks of the arrays of a
// nested CSR point -> views -> atoms, and the two device helpers that keep a CSR range inside its array.  Every entry
// keeps its own ORDER of checks (which of DVA_ERR_INVALID and DVA_ERR_UNSUPPORTED wins is part of the C ABI).
#pragma once
#include <initializer_list>

#include "dva_common.h"

namespace dva {

constexpr int64_t I31_LIMIT = 0x7fffffffLL;      // the kernels index points, views and atoms with an int below this

// the pixels are int16 pairs; the other integer widths are a dtype the kernels do not take, anything else no dtype
static inline int pixel_bytes_code(int32_t pixel_bytes) {
  if (pixel_bytes == 2) return DVA_OK;
  return pixel_bytes == 1 || pixel_bytes == 4 || pixel_bytes == 8 ? DVA_ERR_UNSUPPORTED : DVA_ERR_INVALID;
}

// DVA_ERR_UNSUPPORTED if one of the sizes is 2^31 - 1 or more
static inline int fits_i31(std::initializer_list<int64_t> sizes) {
  for (const int64_t n : sizes)
    if (n >= I31_LIMIT) return DVA_ERR_UNSUPPORTED;
  return DVA_OK;
}

static inline bool any_negative(std::initializer_list<int64_t> sizes) {
  for (const int64_t n : sizes)
    if (n < 0) return true;
  return false;
}

// the arrays behind views and atoms: atom_ptr always has an entry, images / pixels may be null when empty, and the
// kernels read a pixel pair as one 32-bit word
static inline bool mapping_arrays_ok(const void* images, const void* atom_ptr, const void* pixels, int64_t n_views,
                                     int64_t n_atoms) {
  return atom_ptr && (n_views <= 0 || images) && (n_atoms <= 0 || pixels) && ((uintptr_t)pixels & 3) == 0;
}

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// the range [*a, *b) of group i of a CSR, inside [0, hi] whatever the pointers hold
__device__ __forceinline__ void csr_range(const int64_t* ptr, int64_t i, int64_t hi, int64_t* a, int64_t* b) {
  *a = clamp_i64(ptr[i], 0, hi);
  *b = clamp_i64(ptr[i + 1], *a, hi);
}

}  // namespace dva
