// Wavefront helpers, and the exclusive scan of n int32 counts in three kernels (block partial sums, a one-block
// spine, apply), shared by the mapping merge and the mapping selection.  S is the type of the sums: int where the total is known to stay below
// 2^31, int64_t where the caller checks the total afterwards.  out[0 .. n], out[n] = total; bsum holds
// scan_blocks(n) + 1 sums.  The kernels are static: every translation unit that includes this header has its own.
#pragma once
#include "dva_common.h"

namespace dva {

typedef unsigned long long u64;

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;

static inline int64_t scan_blocks(int64_t n) { return (n + SCAN_BLOCK - 1) / SCAN_BLOCK; }

// orders the LDS / global accesses of the lanes of ONE wavefront (the block-wide kernels use __syncthreads)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ u64 lanes_below(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, DVA_WAVE);
  return v;
}
__device__ __forceinline__ long long wave_incl_scan(long long v, int lane) {
#pragma unroll
  for (int o = 1; o < DVA_WAVE; o <<= 1) {
    const long long t = __shfl_up(v, o, DVA_WAVE);
    if (lane >= o) v += t;
  }
  return v;
}

template <typename S>
__device__ __forceinline__ S block_excl_scan(S v, S* total, S* wsum) {
  const int lane = threadIdx.x & (DVA_WAVE - 1), w = threadIdx.x / DVA_WAVE;
  const S incl = (S)wave_incl_scan((long long)v, lane);
  __syncthreads();      // wsum of the previous call has been read
  if (lane == DVA_WAVE - 1) wsum[w] = incl;
  __syncthreads();
  S before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < SCAN_THREADS / DVA_WAVE; ++k) {
    const S s = wsum[k];
    if (k < w) before += s;
    all += s;
  }
  *total = all;
  return before + incl - v;
}

template <typename S>
static __global__ __launch_bounds__(SCAN_THREADS) void scan_partial_kernel(const int* __restrict__ in, int64_t n,
                                                                            S* __restrict__ bsum) {
  __shared__ S wsum[SCAN_THREADS / DVA_WAVE];
  const int64_t i0 = blockIdx.x * (int64_t)SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
  S s = 0;
#pragma unroll
  for (int c = 0; c < SCAN_ITEMS; ++c)
    if (i0 + c < n) s += in[i0 + c];
  S total;
  block_excl_scan<S>(s, &total, wsum);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

template <typename S>
static __global__ __launch_bounds__(SCAN_THREADS) void scan_spine_kernel(S* __restrict__ bsum, int64_t nb) {
  __shared__ S wsum[SCAN_THREADS / DVA_WAVE];
  S carry = 0;
  for (int64_t c0 = 0; c0 < nb; c0 += SCAN_THREADS) {
    const int64_t i = c0 + threadIdx.x;
    const S v = i < nb ? bsum[i] : 0;
    S total;
    const S excl = block_excl_scan<S>(v, &total, wsum);
    if (i < nb) bsum[i] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}

template <typename S>
static __global__ __launch_bounds__(SCAN_THREADS) void scan_apply_kernel(const int* __restrict__ in, int64_t n,
                                                                          const S* __restrict__ bsum, int64_t nb,
                                                                          S* __restrict__ out) {
  __shared__ S wsum[SCAN_THREADS / DVA_WAVE];
  const int64_t i0 = blockIdx.x * (int64_t)SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
  S v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int c = 0; c < SCAN_ITEMS; ++c) {
    v[c] = i0 + c < n ? in[i0 + c] : 0;
    s += v[c];
  }
  S total;
  S run = bsum[blockIdx.x] + block_excl_scan<S>(s, &total, wsum);
#pragma unroll
  for (int c = 0; c < SCAN_ITEMS; ++c) {
    if (i0 + c < n) out[i0 + c] = run;
    run += v[c];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

// n >= 1
template <typename S>
static inline void launch_scan(const int* in, int64_t n, S* bsum, int64_t nb, S* out, hipStream_t s) {
  hipLaunchKernelGGL(scan_partial_kernel<S>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, in, n, bsum);
  hipLaunchKernelGGL(scan_spine_kernel<S>, dim3(1), dim3(SCAN_THREADS), 0, s, bsum, nb);
  hipLaunchKernelGGL(scan_apply_kernel<S>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, in, n, (const S*)bsum, nb,
                     out);
}

}  // namespace dva
