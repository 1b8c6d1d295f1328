// What the fused gather + pool kernels (gather_reduce.hip: nearest gather, interp_reduce.hip: bilinear gather) share: 16-byte
// and element accesses to VEC consecutive channels of one row, the pooling step and its gradient term, the argument checks
// and the choice of a kernel instantiation from (dtype, wide) and reduce.  The two files differ where the gathers differ.
#pragma once
#include "dva_common.h"

namespace dva {

// VEC consecutive channels of one row <-> fp32.  VEC = 16 / sizeof(T): one 16-byte access (C % VEC == 0 and 16-byte
// aligned bases: the caller decides); VEC = 1: element accesses, any C and any base.
template <typename T, int VEC>
struct RowChunk {
  static __device__ __forceinline__ void ld(const T* p, float* f) {
    Chunk16<T>::unpack(*reinterpret_cast<const typename Chunk16<T>::raw*>(p), f);
  }
  static __device__ __forceinline__ void st(T* p, const float* f) {
    *reinterpret_cast<typename Chunk16<T>::raw*>(p) = Chunk16<T>::pack(f);
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

constexpr int64_t POOL_SIZE_MAX = 0x7fffffffLL;  // int32 row / tap plan, int32 segment of item

constexpr bool keeps_arg(int reduce) { return reduce == DVA_MAX || reduce == DVA_MIN; }

// lanes of a wavefront that own the chunks of one row: the power of two that covers them, at most 64 (wider rows are
// walked in column passes)
static inline int lanes_per_row(int chunks) {
  int lpr = 1;
  while (lpr < chunks && lpr < 64) lpr <<= 1;
  return lpr;
}

static inline int check_sizes(int64_t S, int64_t P, int64_t R, int C, int dtype, int reduce) {
  if (S < 0 || P < 0 || R < 0 || C < 0) return DVA_ERR_INVALID;
  if (!dtype_ok(dtype)) return DVA_ERR_INVALID;
  if (reduce < DVA_SUM || reduce > DVA_MIN) return DVA_ERR_INVALID;
  return DVA_OK;
}

// One item joins the pool of a channel, as dva_segment_csr_fwd has it: fp32 sum from 0 in item order (sum, mean), or the
// extremum with the offset of its item -- the first item on ties, a NaN wins only as the first item.
template <int REDUCE>
__device__ __forceinline__ void pool_step(float& acc, uint32_t& best, float f, bool first, uint32_t off) {
  if constexpr (REDUCE == DVA_MAX || REDUCE == DVA_MIN) {
    if (first || (REDUCE == DVA_MAX ? f > acc : f < acc)) {
      acc = f;
      best = off;
    }
  } else {
    acc = __fadd_rn(acc, f);
  }
}

// What an item of a segment of `count` items at offset koff hands on of the segment's gradient g, times the weight w of the
// tap it goes to (1 under a nearest gather): w g (sum), w (g / count) (mean, fp32 true division as segment_csr_bwd_kernel)
// or w g where the stored arg offset ak is the item's (max / min).
template <int REDUCE>
__device__ __forceinline__ float pool_term(float g, float w, float count, uint32_t ak, uint32_t koff) {
  if constexpr (REDUCE == DVA_SUM) return w * g;
  else if constexpr (REDUCE == DVA_MEAN) return w * (g / count);
  else return ak == koff ? w * g : 0.f;
}

// f(RowType<T, VEC>) for the run-time dtype (checked by check_sizes): 16-byte chunks when wide, elements otherwise
template <typename T_, int VEC_>
struct RowType {
  using T = T_;
  static constexpr int VEC = VEC_;
};
static inline int row_vec(int dtype) { return dtype == DVA_F32 ? 4 : 8; }
template <typename F>
static inline void with_row_type(int dtype, bool wide, F&& f) {
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::T;
    wide ? f(RowType<T, Chunk16<T>::N>{}) : f(RowType<T, 1>{});
  });
}

}  // namespace dva
