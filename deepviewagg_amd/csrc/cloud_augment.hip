// The positional 3D augmentations of the per-sample transform chains on the device: RandomNoise, RandomRotate /
// Random3AxisRotation, RandomScaleAnisotropic, RandomSymmetry and Center (reference:
// core/data_transform/transforms.py:463-563, features.py:30-81; RandomRotate and Center are torch_geometric's) as an
// ordered list of at most DVA_CLOUD_MAX_STEPS steps over pos fp32 [n, 3] and, where a step asks for it, norm fp32
// [n, 3].  The random draws are made by the host; matrices and scales arrive by value.
//
// All arithmetic is fp32, every operation rounded on its own (contraction off), divisions and square roots correctly
// rounded.  Per point p (and its normal v), in list order:
//   NOISE    p_c = p_c + e_c                                          e = noise fp32 [n, 3]
//   LINEAR   q_i = ((p_0 M_i0 + p_1 M_i1) + p_2 M_i2), p = q          the same for v when with_norm is set
//   SCALE    p_c = p_c * s_c;  with_norm: v_c = v_c / s_c, l = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2),
//            v_c = v_c / max(l, 1e-12f)
//   FLIP     p_c = m_c - p_c on every flagged axis, m_c = the exact maximum of p_c over the points at this stage
//   CENTER   p_c = p_c - mu_c, mu_c = f32(S_c / n), S_c = the fp64 sum of the stage's fp32 values, divided in fp64
//
// Kernels.  cloud_reduce_kernel, one launch per FLIP / CENTER step in list order: it evaluates the steps in front of
// that step on every point (with the constants of the earlier reductions) and writes one row of partial column maxima
// or fp64 column sums per block.  Nobody adds the rows up in a launch of its own: the NEXT launch (the next reduction,
// or the apply kernel) combines them at the start of every block, in a fixed order (ca_combine: lane t takes rows t,
// t + 256, ..., then a shuffle tree and the four waves in order), so every block holds the same bits; block 0 also
// stores the row of `consts`, which all later launches read from memory.  cloud_apply_kernel evaluates the whole list
// and writes pos_out (norm_out).  No atomics at all; the grid of a reduction is a function of n alone, so the same call
// gives the same bytes.  A lane owns CA_PPT = 4 consecutive points: three 16-byte loads and stores per array (lane i
// at base + 48 i) when the arrays are 16-byte aligned, point by point otherwise and in the tail chunk.
// NaN coordinates are not supported (a maximum skips them).
#include "dva_common.h"

#pragma clang fp contract(off)

namespace dva {

constexpr int CA_TPB = 256;
constexpr int CA_PPT = 4;             // points per lane
constexpr int CA_PART_ROWS = 1024;    // blocks of a reduction launch, at most: rows of partials per reducing step

struct CaSteps {
  int n;                              // steps in the list
  int code[DVA_CLOUD_MAX_STEPS];
  int flag[DVA_CLOUD_MAX_STEPS];      // LINEAR / SCALE: with_norm; FLIP: bit c = axis c is flagged
  int slot[DVA_CLOUD_MAX_STEPS];      // FLIP / CENTER: its row of consts
  float p[DVA_CLOUD_MAX_STEPS][9];    // LINEAR: M row-major; SCALE: s
};

// the rows of partials of the reduction a launch follows, and what they are: the launch combines them into consts[slot]
struct CaPending {
  const double* part;                 // [rows, 3]; null: nothing is pending
  int rows;
  int slot;
  int is_max;                         // FLIP (column maxima) or CENTER (column sums)
  int mask;                           // FLIP: the flagged axes
};

__device__ __forceinline__ double ca_wave(double v, bool is_max) {
#pragma unroll
  for (int off = DVA_WAVE / 2; off > 0; off >>= 1) {
    const double o = __shfl_xor(v, off);
    v = is_max ? fmax(v, o) : v + o;
  }
  return v;
}

// The block's three column values, reduced in a fixed order; valid in thread 0.
__device__ __forceinline__ void ca_block(double* v, bool is_max, double (*sh)[3]) {
  const int lane = threadIdx.x & (DVA_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c] = ca_wave(v[c], is_max);
    if (lane == 0) sh[wave][c] = v[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double a = sh[0][c];
      for (int w = 1; w < CA_TPB / DVA_WAVE; ++w) a = is_max ? fmax(a, sh[w][c]) : a + sh[w][c];
      v[c] = a;
    }
  }
}

// consts[pend.slot] from the pending partials, the same bits in every block: fresh[0..2] (LDS), and block 0 stores it
__device__ __forceinline__ void ca_combine(const CaPending& pend, int64_t n, float* __restrict__ consts, float* fresh) {
  __shared__ double sh[CA_TPB / DVA_WAVE][3];
  if (!pend.part) return;
  const double id = pend.is_max ? -(double)__uint_as_float(0x7f800000u) : 0.0;
  double v[3] = {id, id, id};
  for (int r = threadIdx.x; r < pend.rows; r += CA_TPB) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double o = pend.part[(int64_t)r * 3 + c];
      v[c] = pend.is_max ? fmax(v[c], o) : v[c] + o;
    }
  }
  ca_block(v, pend.is_max, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float m;
      if (pend.is_max)
        m = ((pend.mask >> c) & 1) ? (float)v[c] : 0.f;      // a float held in a double: exact
      else
        m = (float)(v[c] / (double)n);
      fresh[c] = m;
      if (blockIdx.x == 0) consts[pend.slot * 3 + c] = m;
    }
  }
  __syncthreads();
}

// The steps [0, upto) on P points.  Row `fresh_slot` of the constants comes from `fresh`, earlier rows from `consts`.
template <int P, bool NORM>
__device__ __forceinline__ void ca_eval(const CaSteps& st, int upto, const float* __restrict__ consts, int fresh_slot,
                                        const float* fresh, const float (*e)[3], float (*p)[3], float (*v)[3]) {
  for (int k = 0; k < upto; ++k) {
    const int code = st.code[k];
    if (code == DVA_CLOUD_NOISE) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p[j][c] = p[j][c] + e[j][c];
      }
    } else if (code == DVA_CLOUD_LINEAR) {
      float M[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) M[i] = st.p[k][i];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float a = p[j][0], b = p[j][1], c = p[j][2];
#pragma unroll
        for (int i = 0; i < 3; ++i) p[j][i] = (a * M[3 * i] + b * M[3 * i + 1]) + c * M[3 * i + 2];
        if (NORM && st.flag[k]) {
          const float x = v[j][0], y = v[j][1], z = v[j][2];
#pragma unroll
          for (int i = 0; i < 3; ++i) v[j][i] = (x * M[3 * i] + y * M[3 * i + 1]) + z * M[3 * i + 2];
        }
      }
    } else if (code == DVA_CLOUD_SCALE) {
      const float s[3] = {st.p[k][0], st.p[k][1], st.p[k][2]};
#pragma unroll
      for (int j = 0; j < P; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p[j][c] = p[j][c] * s[c];
        if (NORM && st.flag[k]) {
#pragma unroll
          for (int c = 0; c < 3; ++c) v[j][c] = __fdiv_rn(v[j][c], s[c]);
          // sqrtf is the correctly rounded square root (__fsqrt_rn is the native approximation in this toolchain)
          const float l = sqrtf((v[j][0] * v[j][0] + v[j][1] * v[j][1]) + v[j][2] * v[j][2]);
          const float d = fmaxf(l, 1e-12f);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[j][c] = __fdiv_rn(v[j][c], d);
        }
      }
    } else {
      const int slot = st.slot[k];
      float m[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) m[c] = slot == fresh_slot ? fresh[c] : consts[slot * 3 + c];
      if (code == DVA_CLOUD_FLIP) {
        const int mask = st.flag[k];
#pragma unroll
        for (int j = 0; j < P; ++j) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if ((mask >> c) & 1) p[j][c] = m[c] - p[j][c];
        }
      } else {
#pragma unroll
        for (int j = 0; j < P; ++j) {
#pragma unroll
          for (int c = 0; c < 3; ++c) p[j][c] = p[j][c] - m[c];
        }
      }
    }
  }
}

// CA_PPT points from element 3 i0 of `a` (16-byte aligned there)
__device__ __forceinline__ void ca_load4(const float* __restrict__ a, int64_t i0, float (*r)[3]) {
  const float4* q = reinterpret_cast<const float4*>(a + 3 * i0);
  const float4 x = q[0], y = q[1], z = q[2];
  r[0][0] = x.x, r[0][1] = x.y, r[0][2] = x.z, r[1][0] = x.w;
  r[1][1] = y.x, r[1][2] = y.y, r[2][0] = y.z, r[2][1] = y.w;
  r[2][2] = z.x, r[3][0] = z.y, r[3][1] = z.z, r[3][2] = z.w;
}

__device__ __forceinline__ void ca_store4(float* __restrict__ a, int64_t i0, const float (*r)[3]) {
  float4* q = reinterpret_cast<float4*>(a + 3 * i0);
  q[0] = make_float4(r[0][0], r[0][1], r[0][2], r[1][0]);
  q[1] = make_float4(r[1][1], r[1][2], r[2][0], r[2][1]);
  q[2] = make_float4(r[2][2], r[3][0], r[3][1], r[3][2]);
}

__device__ __forceinline__ void ca_load1(const float* __restrict__ a, int64_t i, float (*r)[3]) {
  r[0][0] = a[3 * i], r[0][1] = a[3 * i + 1], r[0][2] = a[3 * i + 2];
}

// ---------------------------------------------------------------------------------------------------------------
// the reduction of step `at` (a FLIP or a CENTER): part[block] = the block's column maxima or fp64 column sums of the
// points after the steps [0, at).  grid-stride over chunks of CA_PPT points.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CA_TPB) void cloud_reduce_kernel(const float* __restrict__ pos,
                                                              const float* __restrict__ noise, int64_t n, CaSteps st,
                                                              int at, CaPending pend, float* __restrict__ consts,
                                                              double* __restrict__ part, int aligned) {
  __shared__ float fresh[3];
  __shared__ double sh[CA_TPB / DVA_WAVE][3];
  ca_combine(pend, n, consts, fresh);
  const int fresh_slot = pend.part ? pend.slot : -1;
  const bool is_max = st.code[at] == DVA_CLOUD_FLIP;
  const double id = is_max ? -(double)__uint_as_float(0x7f800000u) : 0.0;
  double acc[3] = {id, id, id};
  const int64_t chunks = (n + CA_PPT - 1) / CA_PPT;
  for (int64_t t = (int64_t)blockIdx.x * CA_TPB + threadIdx.x; t < chunks; t += (int64_t)gridDim.x * CA_TPB) {
    const int64_t i0 = t * CA_PPT;
    if (aligned && i0 + CA_PPT <= n) {
      float p[CA_PPT][3], e[CA_PPT][3];
      ca_load4(pos, i0, p);
      if (noise) ca_load4(noise, i0, e);
      ca_eval<CA_PPT, false>(st, at, consts, fresh_slot, fresh, e, p, nullptr);
#pragma unroll
      for (int j = 0; j < CA_PPT; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = is_max ? fmax(acc[c], (double)p[j][c]) : acc[c] + (double)p[j][c];
      }
    } else {
      const int64_t i1 = i0 + CA_PPT < n ? i0 + CA_PPT : n;
      for (int64_t i = i0; i < i1; ++i) {
        float p[1][3], e[1][3];
        ca_load1(pos, i, p);
        if (noise) ca_load1(noise, i, e);
        ca_eval<1, false>(st, at, consts, fresh_slot, fresh, e, p, nullptr);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = is_max ? fmax(acc[c], (double)p[0][c]) : acc[c] + (double)p[0][c];
      }
    }
  }
  ca_block(acc, is_max, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) part[(int64_t)blockIdx.x * 3 + c] = acc[c];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// apply: the whole list on every point; one lane per chunk of CA_PPT points
// ---------------------------------------------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(CA_TPB) void cloud_apply_kernel(const float* __restrict__ pos,
                                                             const float* __restrict__ norm,
                                                             const float* __restrict__ noise, int64_t n, CaSteps st,
                                                             CaPending pend, float* __restrict__ consts,
                                                             float* __restrict__ out, float* __restrict__ norm_out,
                                                             int aligned) {
  __shared__ float fresh[3];
  ca_combine(pend, n, consts, fresh);                       // before any exit: it holds barriers
  const int fresh_slot = pend.part ? pend.slot : -1;
  const int64_t i0 = ((int64_t)blockIdx.x * CA_TPB + threadIdx.x) * CA_PPT;
  if (i0 >= n) return;
  if (aligned && i0 + CA_PPT <= n) {
    float p[CA_PPT][3], e[CA_PPT][3], v[CA_PPT][3];
    ca_load4(pos, i0, p);
    if (noise) ca_load4(noise, i0, e);
    if (NORM) ca_load4(norm, i0, v);
    ca_eval<CA_PPT, NORM>(st, st.n, consts, fresh_slot, fresh, e, p, v);
    ca_store4(out, i0, p);
    if (NORM) ca_store4(norm_out, i0, v);
    return;
  }
  const int64_t i1 = i0 + CA_PPT < n ? i0 + CA_PPT : n;
  for (int64_t i = i0; i < i1; ++i) {
    float p[1][3], e[1][3], v[1][3];
    ca_load1(pos, i, p);
    if (noise) ca_load1(noise, i, e);
    if (NORM) ca_load1(norm, i, v);
    ca_eval<1, NORM>(st, st.n, consts, fresh_slot, fresh, e, p, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = p[0][c];
    if (NORM) {
#pragma unroll
      for (int c = 0; c < 3; ++c) norm_out[3 * i + c] = v[0][c];
    }
  }
}

static inline bool ca_reduces(int code) { return code == DVA_CLOUD_FLIP || code == DVA_CLOUD_CENTER; }

static inline int ca_part_rows(int64_t n) { return capped_grid((n + CA_PPT - 1) / CA_PPT, CA_TPB, CA_PART_ROWS); }

// 3 n floats are indexed with int64, but the Python side sizes its tensors, and every other pos kernel its grid, below 2^31
static inline bool ca_fits(int64_t n) { return n <= (0x7fffffffLL) / 3; }

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_cloud_augment_workspace_bytes(int64_t n, int32_t n_steps) {
  if (n < 0 || n_steps < 0 || n_steps > DVA_CLOUD_MAX_STEPS) return DVA_ERR_INVALID;
  if (!ca_fits(n)) return DVA_ERR_UNSUPPORTED;
  Carver ws(nullptr);
  for (int k = 0; k < n_steps; ++k) ws.take<double>((size_t)ca_part_rows(n) * 3);
  return (int64_t)ws.used();
}

int dva_cloud_augment_f32(const float* pos, const float* norm, const float* noise, int64_t n, const int32_t* codes,
                          const float* params, int32_t n_steps, float* out, float* norm_out, float* consts,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || n_steps < 0 || n_steps > DVA_CLOUD_MAX_STEPS) return DVA_ERR_INVALID;
  if (n_steps > 0 && (!codes || !params)) return DVA_ERR_INVALID;
  CaSteps st = {};
  st.n = n_steps;
  int n_reduce = 0;
  bool with_norm = false, with_noise = false;
  for (int k = 0; k < n_steps; ++k) {
    const float* p = params + (size_t)k * DVA_CLOUD_STEP_PARAMS;
    st.code[k] = codes[k];
    switch (codes[k]) {
      case DVA_CLOUD_NOISE:
        if (!noise) return DVA_ERR_INVALID;
        with_noise = true;
        break;
      case DVA_CLOUD_LINEAR:
      case DVA_CLOUD_SCALE:
        for (int i = 0; i < (codes[k] == DVA_CLOUD_LINEAR ? 9 : 3); ++i) st.p[k][i] = p[i];
        st.flag[k] = p[9] != 0.f;
        if (st.flag[k] && !norm) return DVA_ERR_INVALID;
        with_norm = with_norm || st.flag[k];
        break;
      case DVA_CLOUD_FLIP:
        st.flag[k] = (p[0] != 0.f ? 1 : 0) | (p[1] != 0.f ? 2 : 0) | (p[2] != 0.f ? 4 : 0);
        if (!st.flag[k]) return DVA_ERR_INVALID;             // a flip of no axis is no step
        st.slot[k] = n_reduce++;
        break;
      case DVA_CLOUD_CENTER:
        st.slot[k] = n_reduce++;
        break;
      default:
        return DVA_ERR_INVALID;
    }
  }
  if (!ca_fits(n)) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return DVA_OK;
  if (!pos || !out || (with_norm && !norm_out)) return DVA_ERR_INVALID;
  const int rows = ca_part_rows(n);
  Carver ws(workspace);
  double* parts[DVA_CLOUD_MAX_STEPS];
  for (int r = 0; r < n_reduce; ++r) parts[r] = ws.take<double>((size_t)rows * 3);
  if (n_reduce > 0) {
    if (!consts || !workspace || workspace_bytes < (int64_t)ws.used()) return DVA_ERR_INVALID;
    if (out == pos || (with_norm && norm_out == norm)) return DVA_ERR_INVALID;
  }
  if (!with_noise) noise = nullptr;
  const int aligned = ((uintptr_t)pos % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                      (!noise || ((uintptr_t)noise % 16) == 0) &&
                      (!with_norm || (((uintptr_t)norm % 16) == 0 && ((uintptr_t)norm_out % 16) == 0));
  hipStream_t s = (hipStream_t)stream;
  CaPending pend = {};
  for (int k = 0; k < n_steps; ++k) {
    if (!ca_reduces(st.code[k])) continue;
    double* part = parts[st.slot[k]];
    hipLaunchKernelGGL(cloud_reduce_kernel, dim3((unsigned)rows), dim3(CA_TPB), 0, s, pos, noise, n, st, k, pend, consts,
                       part, aligned);
    pend.part = part;
    pend.rows = rows;
    pend.slot = st.slot[k];
    pend.is_max = st.code[k] == DVA_CLOUD_FLIP;
    pend.mask = st.flag[k];
  }
  const dim3 grid((unsigned)blocks_for((n + CA_PPT - 1) / CA_PPT, CA_TPB));
  if (with_norm)
    hipLaunchKernelGGL((cloud_apply_kernel<true>), grid, dim3(CA_TPB), 0, s, pos, norm, noise, n, st, pend, consts, out,
                       norm_out, aligned);
  else
    hipLaunchKernelGGL((cloud_apply_kernel<false>), grid, dim3(CA_TPB), 0, s, pos, norm, noise, n, st, pend, consts,
                       out, norm_out, aligned);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
