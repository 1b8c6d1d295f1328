// 16-byte and element accesses to VEC consecutive channels of one row, shared by the fused gather + pool kernels
// (gather_reduce.hip, interp_reduce.hip).
#pragma once
#include "dva_common.h"

namespace dva {

// VEC consecutive channels of one row <-> fp32.  VEC = 16 / sizeof(T): one 16-byte access (C % VEC == 0 and 16-byte
// aligned bases: the caller decides); VEC = 1: element accesses, any C and any base.
template <typename T, int VEC>
struct RowChunk {
  static __device__ __forceinline__ void ld(const T* p, float* f) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    if constexpr (sizeof(T) == 4) {
      f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y);
      f[2 % VEC] = __uint_as_float(r.z); f[3 % VEC] = __uint_as_float(r.w);
    } else {
      unpack_h8<T>(r, f);
    }
  }
  static __device__ __forceinline__ void st(T* p, const float* f) {
    if constexpr (sizeof(T) == 4)
      *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2 % VEC], f[3 % VEC]);
    else
      *reinterpret_cast<uint4*>(p) = pack_h8<T>(f);
  }
  // the uint16 arg offsets of the same channels
  static __device__ __forceinline__ void ld_arg(const uint16_t* p, uint32_t* k) {
    if constexpr (VEC == 4) {
      const uint2 a = *reinterpret_cast<const uint2*>(p);
      k[0] = a.x & 0xffffu; k[1] = a.x >> 16; k[2 % VEC] = a.y & 0xffffu; k[3 % VEC] = a.y >> 16;
    } else {
      const uint4 a = *reinterpret_cast<const uint4*>(p);
      const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        k[(2 * e) % VEC] = w[e] & 0xffffu;
        k[(2 * e + 1) % VEC] = w[e] >> 16;
      }
    }
  }
  static __device__ __forceinline__ void st_arg(uint16_t* p, const uint32_t* k) {
    if constexpr (VEC == 4)
      *reinterpret_cast<uint2*>(p) = make_uint2(k[0] | (k[1] << 16), k[2 % VEC] | (k[3 % VEC] << 16));
    else
      *reinterpret_cast<uint4*>(p) = make_uint4(k[0] | (k[1] << 16), k[2 % VEC] | (k[3 % VEC] << 16),
                                                k[4 % VEC] | (k[5 % VEC] << 16), k[6 % VEC] | (k[7 % VEC] << 16));
  }
};
template <typename T>
struct RowChunk<T, 1> {
  static __device__ __forceinline__ void ld(const T* p, float* f) { f[0] = Elt<T>::ld(p, 0); }
  static __device__ __forceinline__ void st(T* p, const float* f) { Elt<T>::st(p, 0, f[0]); }
  static __device__ __forceinline__ void ld_arg(const uint16_t* p, uint32_t* k) { k[0] = p[0]; }
  static __device__ __forceinline__ void st_arg(uint16_t* p, const uint32_t* k) { p[0] = (uint16_t)k[0]; }
};

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace dva
