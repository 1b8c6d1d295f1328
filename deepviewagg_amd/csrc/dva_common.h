// Internal helpers shared by the gfx950 kernels of libdva_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/dva.h"

#define DVA_WAVE 64

#define DVA_CHECK_LAUNCH()                           \
  do {                                               \
    hipError_t e__ = hipGetLastError();              \
    if (e__ != hipSuccess) return DVA_ERR_LAUNCH;    \
  } while (0)

namespace dva {

typedef uint16_t bf16_t;  // raw bfloat16 bits

__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

// float -> bfloat16, round-to-nearest-even (same rounding as torch): gfx950 has the packed hardware
// conversion v_cvt_pk_bf16_f32 (one instruction per pair, NaN stays NaN).
typedef __bf16 dva_bf16x2 __attribute__((ext_vector_type(2)));
typedef float dva_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  const dva_f32x2 v = {lo, hi};
  const dva_bf16x2 b = __builtin_convertvector(v, dva_bf16x2);
  return __builtin_bit_cast(uint32_t, b);
}
__device__ __forceinline__ bf16_t f2bf(float f) { return (bf16_t)(pack_bf16x2(f, 0.f) & 0xffffu); }

// IEEE binary16 (DVA_F16, the storage type of torch.float16).  A type of its own, not a second uint16_t: the Elt<> /
// Pair16<> / dotv<> specialisations must tell it from bf16_t.  float -> fp16 rounds to nearest even (v_cvt_f16_f32,
// v_cvt_pk_f16_f32 in the default round mode; never v_cvt_pkrtz): overflow gives +-inf and NaN stays NaN, as in torch
// -- GradScaler's overflow check depends on both.
typedef _Float16 f16_t;
typedef _Float16 dva_f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi) {
  const dva_f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, dva_f16x2));
}

// Two 16-bit elements of one 32-bit word (element 0 in the low half) <-> fp32, per 2-byte storage type.
template <typename T>
struct Pair16;
template <>
struct Pair16<bf16_t> {
  static __device__ __forceinline__ float lo(uint32_t w) { return __uint_as_float(w << 16); }
  static __device__ __forceinline__ float hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
  static __device__ __forceinline__ uint32_t pack(float a, float b) { return pack_bf16x2(a, b); }
  static __device__ __forceinline__ uint16_t one(float a) { return f2bf(a); }
};
template <>
struct Pair16<f16_t> {
  static __device__ __forceinline__ float lo(uint32_t w) {
    return (float)__builtin_bit_cast(f16_t, (uint16_t)(w & 0xffffu));
  }
  static __device__ __forceinline__ float hi(uint32_t w) { return (float)__builtin_bit_cast(f16_t, (uint16_t)(w >> 16)); }
  static __device__ __forceinline__ uint32_t pack(float a, float b) { return pack_f16x2(a, b); }
  static __device__ __forceinline__ uint16_t one(float a) { return __builtin_bit_cast(uint16_t, (f16_t)a); }
};
// 8 elements of a 16-byte chunk <-> fp32
template <typename T>
__device__ __forceinline__ void unpack_h8(const uint4& r, float* f) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = Pair16<T>::lo(w[i]);
    f[2 * i + 1] = Pair16<T>::hi(w[i]);
  }
}
template <typename T>
__device__ __forceinline__ uint4 pack_h8(const float* f) {
  return make_uint4(Pair16<T>::pack(f[0], f[1]), Pair16<T>::pack(f[2], f[3]), Pair16<T>::pack(f[4], f[5]),
                    Pair16<T>::pack(f[6], f[7]));
}

// The 16 bytes of N consecutive elements of a row, as one load / store, <-> fp32
template <typename T>
struct Chunk16 {
  static constexpr int N = 8;
  typedef uint4 raw;
  static __device__ __forceinline__ void unpack(const raw& r, float* f) { unpack_h8<T>(r, f); }
  static __device__ __forceinline__ raw pack(const float* f) { return pack_h8<T>(f); }
};
template <>
struct Chunk16<float> {
  static constexpr int N = 4;
  typedef float4 raw;
  static __device__ __forceinline__ void unpack(const raw& r, float* f) { f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w; }
  static __device__ __forceinline__ raw pack(const float* f) { return make_float4(f[0], f[1], f[2], f[3]); }
};

template <typename T>
struct Elt;
template <>
struct Elt<float> {
  static __device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
  static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
};
template <>
struct Elt<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t* p, int64_t i) { return bf2f(p[i]); }
  static __device__ __forceinline__ void st(bf16_t* p, int64_t i, float v) { p[i] = f2bf(v); }
};
template <>
struct Elt<f16_t> {
  static __device__ __forceinline__ float ld(const f16_t* p, int64_t i) { return (float)p[i]; }
  static __device__ __forceinline__ void st(f16_t* p, int64_t i, float v) { p[i] = (f16_t)v; }
};

// expand_group_feat (pooling.py:737-755): the first (C mod G) groups own floor(C/G)+1 channels,
// the others floor(C/G).  Returns the group of channel c.
__host__ __device__ __forceinline__ int group_of_channel(int c, int C, int G) {
  if (G <= 1) return 0;
  if (G >= C) return c;
  const int base = C / G, rem = C % G;
  const int split = rem * (base + 1);
  return c < split ? c / (base + 1) : rem + (c - split) / base;
}
// first channel of group g
__host__ __device__ __forceinline__ int group_begin(int g, int C, int G) {
  if (g >= G) return C;
  if (G <= 1) return 0;
  if (G >= C) return g;
  const int base = C / G, rem = C % G;
  return g < rem ? g * (base + 1) : rem * (base + 1) + (g - rem) * base;
}

// 8-byte packed gather index of one atom: {int32 image, int16 x, int16 y}
struct __attribute__((aligned(8))) PackedIdx {
  int32_t img;
  int16_t x;
  int16_t y;
};

// torch.floor_divide on floats (c10::div_floor_floating): floor of the exact quotient a/b.  The pixel rounding of every
// kernel that maps a pixel onto a feature map (gather.hip, plan_split.hip).
__device__ __forceinline__ float floordiv_f32(float a, float b) {
  const float mod = fmodf(a, b);
  float div = __fdiv_rn(__fsub_rn(a, mod), b);
  if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) div = __fsub_rn(div, 1.f);
  if (div != 0.f) {
    float fl = floorf(div);
    if (__fsub_rn(div, fl) > 0.5f) fl = __fadd_rn(fl, 1.f);
    return fl;
  }
  return copysignf(0.f, __fdiv_rn(a, b));
}

static inline int blocks_for(int64_t n, int threads) { return (int)((n + threads - 1) / threads); }

// Launch grid of a grid-stride kernel: ceil(n / per_block) blocks, at most `cap`, at least 1.
static inline int capped_grid(int64_t n, int64_t per_block, int64_t cap) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

constexpr int64_t GRID_CAP = 256 * 32;  // 256 CUs x 32 blocks, grid-stride beyond

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline bool dtype_ok(int dtype) { return dtype == DVA_F32 || dtype == DVA_BF16 || dtype == DVA_F16; }

// f(DType<T>) for the run-time storage code; false, and f not called, for any other code.  with_f32_bf16 is for the
// entries that have no fp16 kernels: they answer DVA_F16 with DVA_ERR_UNSUPPORTED before they get here.
template <typename T_>
struct DType {
  using T = T_;
};
template <typename F>
static inline bool with_f32_bf16(int dtype, F&& f) {
  if (dtype == DVA_F32) f(DType<float>{});
  else if (dtype == DVA_BF16) f(DType<bf16_t>{});
  else return false;
  return true;
}
template <typename F>
static inline bool with_dtype(int dtype, F&& f) {
  if (dtype != DVA_F16) return with_f32_bf16(dtype, f);
  f(DType<f16_t>{});
  return true;
}

// f(std::integral_constant<int, REDUCE>) for the run-time reduce (DVA_SUM .. DVA_MIN, checked by the caller)
template <typename F>
static inline void with_reduce(int reduce, F&& f) {
  if (reduce == DVA_SUM) f(std::integral_constant<int, DVA_SUM>{});
  else if (reduce == DVA_MEAN) f(std::integral_constant<int, DVA_MEAN>{});
  else if (reduce == DVA_MAX) f(std::integral_constant<int, DVA_MAX>{});
  else f(std::integral_constant<int, DVA_MIN>{});
}

// Zero fill of `words` 32-bit words at a 4-byte-aligned address, as a kernel.  The entries that promise to be capturable
// in a HIP graph clear their accumulators with this and not with hipMemsetAsync.  Observed with ROCm 7.2.0 on gfx950,
// through two tests (tests/test_gpu_graph_replay.py: the Lovasz counters and gradient, the sparse convolution's weight
// gradient): with the memsets captured, the first replay was right and every later one left other bits than zeros in
// those buffers.  Why the runtime does that was not looked into; a kernel node was replayed correctly every time.
static __global__ __launch_bounds__(256) void zero_words_kernel(uint32_t* __restrict__ p, int64_t words) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) p[i] = 0u;
}

static inline void zero_words(void* p, int64_t words, hipStream_t s) {
  if (words <= 0) return;
  hipLaunchKernelGGL(zero_words_kernel, dim3(capped_grid(words, 256 * 4, 2048)), dim3(256), 0, s, (uint32_t*)p, words);
}

// `align` is a power of two: 256 for the regions of a workspace (16 inside the mapping merge's).
static inline size_t align_up(size_t bytes, size_t align = 256) { return (bytes + align - 1) & ~(align - 1); }

// Carves a caller-provided workspace into typed regions, each padded to `align` bytes.  A null base answers a size
// query: the same sequence of take() calls then only adds up used().  (Addresses are uintptr_t, so that is defined.)
class Carver {
 public:
  explicit Carver(void* base, size_t align = 256) : base_((uintptr_t)base), align_(align) {}
  template <typename T>
  T* take(size_t count) {
    T* p = (T*)(base_ + off_);
    off_ += align_up(count * sizeof(T), align_);
    return p;
  }
  size_t used() const { return off_; }

 private:
  uintptr_t base_;
  size_t off_ = 0, align_;
};

}  // namespace dva
