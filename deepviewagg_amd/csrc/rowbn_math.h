// Per-element arithmetic of the weighted row BatchNorm + LeakyReLU (formulas: header of rowbn.hip), one definition
// for the row-streaming kernels (rowbn.hip) and the fused E_mod row kernels (emod_rows.hip): both evaluate the same
// fp32 operations in the same order, so a value has the same bits whichever kernel produces it.  The library is
// built with -ffp-contract=off: a * b + c below is two roundings, not an fma.
#pragma once
#include "dva_common.h"

namespace dva {
namespace rowbn {

// a = normalised y
__device__ __forceinline__ float norm(float y, float mean, float invstd) { return (y - mean) * invstd; }
// z = pre-activation
__device__ __forceinline__ float affine(float a, float gamma, float beta) { return a * gamma + beta; }
__device__ __forceinline__ float act(float z, float slope) { return z > 0.f ? z : slope * z; }
__device__ __forceinline__ float dact(float z, float slope) { return z > 0.f ? 1.f : slope; }
// dy = gamma invstd (dz - w S1/n - w a S2/n),  w = views of the row
__device__ __forceinline__ float grad_y(float dz, float a, float w, float gamma, float invstd, float s1n, float s2n) {
  return gamma * invstd * (dz - w * s1n - w * a * s2n);
}

}  // namespace rowbn
}  // namespace dva
