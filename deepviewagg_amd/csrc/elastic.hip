// ElasticDistortion on the device (reference: core/data_transform/grid_transform.py:194-256, which runs six
// scipy.ndimage.convolve calls over a noise volume and a scipy RegularGridInterpolator over every point, on the host).
//
// One distortion level is
//   bounds    column min / max of pos (fp32 [N, 3]); the host derives the volume's shape and its three knot axes
//             from them with the reference's own numpy expressions;
//   smooth    two rounds of three 3-tap box passes along axes 0, 1, 2 of the noise volume fp32 [Dx, Dy, Dz, 3], zero
//             padded.  scipy.ndimage.convolve accumulates in double, taps in ascending order starting from 0.0, every
//             product (tap * w, w = (double)(1.0f / 3.0f)) and every sum rounded on its own, and stores the pass as
//             float32: so does elastic_smooth_kernel, pass by pass;
//   displace  per point and axis the cell i = the largest index with ax[i] <= x, clipped to [0, d - 2], the normalised
//             distance y = (x - ax[i]) / (ax[i + 1] - ax[i]), the eight corners in itertools.product order (axis 0
//             slowest, lower corner first) with weight ((1 - y0 | y0) * (1 - y1 | y1)) * (1 - y2 | y2), value +=
//             field[corner] * weight starting from 0.0, all in fp64; a point outside the axes gets 0;
//             out = fp32(fp64(pos) + value * magnitude).
// Every fp64 operation is spelled __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn (no fused multiply-add, the
// translation unit is compiled with contraction off, the division is correctly rounded), so the results are the
// reference's bit for bit.  No atomics: the same call gives the same bytes.
#include "dva_common.h"

#pragma clang fp contract(off)

namespace dva {

constexpr int EL_TPB = 256;
constexpr int EL_MINMAX_BLOCKS = 256;                 // partial rows of the bounds reduction
constexpr int EL_LDS_AXES = 4096;                     // knots (of the three axes together) staged in LDS: 32 KiB
constexpr int64_t EL_MAX_ELEMS = 0x7fffffffLL;        // elements of pos and of the volume

// ---------------------------------------------------------------------------------------------------------------
// bounds: out[0..2] = column minima, out[3..5] = column maxima.  min / max are exact and order-free.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void minmax_wave(float* lo, float* hi) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int off = DVA_WAVE / 2; off > 0; off >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], off));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], off));
    }
  }
}

// Reduces the block's values; thread 0 writes the row {lo[3], hi[3]}.
__device__ __forceinline__ void minmax_block_store(float* lo, float* hi, float* __restrict__ row) {
  __shared__ float sh[EL_TPB / DVA_WAVE][6];
  minmax_wave(lo, hi);
  const int lane = threadIdx.x & (DVA_WAVE - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sh[wave][c] = lo[c];
      sh[wave][3 + c] = hi[c];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float l = sh[0][c], h = sh[0][3 + c];
      for (int w = 1; w < EL_TPB / DVA_WAVE; ++w) {
        l = fminf(l, sh[w][c]);
        h = fmaxf(h, sh[w][3 + c]);
      }
      row[c] = l;
      row[3 + c] = h;
    }
  }
}

__global__ __launch_bounds__(EL_TPB) void minmax3_partial_kernel(const float* __restrict__ pos, int64_t n,
                                                                 float* __restrict__ part) {
  const float inf = __uint_as_float(0x7f800000u);
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  const int64_t stride = (int64_t)gridDim.x * EL_TPB;
  for (int64_t i = (int64_t)blockIdx.x * EL_TPB + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = pos[3 * i + c];
      lo[c] = fminf(lo[c], v);
      hi[c] = fmaxf(hi[c], v);
    }
  }
  minmax_block_store(lo, hi, part + (int64_t)blockIdx.x * 6);
}

__global__ __launch_bounds__(EL_TPB) void minmax3_final_kernel(const float* __restrict__ part, int rows,
                                                               float* __restrict__ out) {
  const float inf = __uint_as_float(0x7f800000u);
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (int r = threadIdx.x; r < rows; r += EL_TPB) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], part[r * 6 + c]);
      hi[c] = fmaxf(hi[c], part[r * 6 + 3 + c]);
    }
  }
  minmax_block_store(lo, hi, out);
}

// ---------------------------------------------------------------------------------------------------------------
// one 3-tap pass along one axis: `stride` elements between neighbours on that axis, `dim` entries on it
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EL_TPB) void elastic_smooth_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                int total, int stride, int dim) {
  const int i = blockIdx.x * EL_TPB + threadIdx.x;     // total < 2^31, and so is the rounded-up grid (checked)
  if (i >= total) return;
  const double w = (double)(1.0f / 3.0f);
  const int k = (i / stride) % dim;
  const double a = k > 0 ? (double)src[i - stride] : 0.0;
  const double b = (double)src[i];
  const double c = k + 1 < dim ? (double)src[i + stride] : 0.0;
  double acc = __dadd_rn(0.0, __dmul_rn(a, w));
  acc = __dadd_rn(acc, __dmul_rn(b, w));
  acc = __dadd_rn(acc, __dmul_rn(c, w));
  dst[i] = (float)acc;
}

// ---------------------------------------------------------------------------------------------------------------
// displacement
// ---------------------------------------------------------------------------------------------------------------
// The cell of x on one axis (d >= 2 ascending knots): i = the largest index with ax[i] <= x, clipped to [0, d - 2]
// (numpy.searchsorted(ax, x, side='right') - 1, clipped), from the estimate (x - ax[0]) / step corrected against the
// knots themselves; *y = (x - ax[i]) / (ax[i + 1] - ax[i]); returns false when x lies outside [ax[0], ax[d - 1]].
template <typename AX>
__device__ __forceinline__ bool elastic_cell(const AX ax, int d, double inv_step, double x, int* cell, double* y) {
  const double first = ax[0], last = ax[d - 1];
  double e = __dmul_rn(__dsub_rn(x, first), inv_step);
  e = fmin(fmax(e, 0.0), (double)(d - 2));             // a NaN estimate becomes 0; the cast below is defined
  int i = (int)e;
  while (i > 0 && ax[i] > x) --i;
  while (i < d - 2 && ax[i + 1] <= x) ++i;
  const double a = ax[i], b = ax[i + 1];
  *cell = i;
  *y = __ddiv_rn(__dsub_rn(x, a), __dsub_rn(b, a));
  return !(x < first) && !(x > last);
}

template <bool LDS>
__global__ __launch_bounds__(EL_TPB) void elastic_displace_kernel(const float* __restrict__ pos, int64_t n,
                                                                  const float* __restrict__ field,
                                                                  const double* __restrict__ axes, int dx, int dy,
                                                                  int dz, double magnitude, float* __restrict__ out) {
  extern __shared__ double sax[];
  const double* ax = axes;
  if (LDS) {
    for (int k = threadIdx.x; k < dx + dy + dz; k += EL_TPB) sax[k] = axes[k];
    __syncthreads();
    ax = sax;
  }
  const int64_t p = (int64_t)blockIdx.x * EL_TPB + threadIdx.x;
  if (p >= n) return;
  const double* ax0 = ax;
  const double* ax1 = ax + dx;
  const double* ax2 = ax + dx + dy;
  const float fx = pos[3 * p], fy = pos[3 * p + 1], fz = pos[3 * p + 2];
  const double x0 = (double)fx, x1 = (double)fy, x2 = (double)fz;
  int i0, i1, i2;
  double y0, y1, y2;
  // the estimate's scale only has to land near the cell: the knots decide
  const double s0 = (double)(dx - 1) / (ax0[dx - 1] - ax0[0]);
  const double s1 = (double)(dy - 1) / (ax1[dy - 1] - ax1[0]);
  const double s2 = (double)(dz - 1) / (ax2[dz - 1] - ax2[0]);
  bool inside = elastic_cell(ax0, dx, s0, x0, &i0, &y0);
  inside = elastic_cell(ax1, dy, s1, x1, &i1, &y1) && inside;
  inside = elastic_cell(ax2, dz, s2, x2, &i2, &y2) && inside;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (inside) {
    const double w0[2] = {__dsub_rn(1.0, y0), y0};
    const double w1[2] = {__dsub_rn(1.0, y1), y1};
    const double w2[2] = {__dsub_rn(1.0, y2), y2};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const double wt = __dmul_rn(__dmul_rn(w0[a], w1[b]), w2[c]);      // 1 * w0 is exact
          const float* f = field + 3 * (((int64_t)(i0 + a) * dy + (i1 + b)) * dz + (i2 + c));
          v0 = __dadd_rn(v0, __dmul_rn((double)f[0], wt));
          v1 = __dadd_rn(v1, __dmul_rn((double)f[1], wt));
          v2 = __dadd_rn(v2, __dmul_rn((double)f[2], wt));
        }
      }
    }
  }
  out[3 * p] = (float)__dadd_rn(x0, __dmul_rn(v0, magnitude));
  out[3 * p + 1] = (float)__dadd_rn(x1, __dmul_rn(v1, magnitude));
  out[3 * p + 2] = (float)__dadd_rn(x2, __dmul_rn(v2, magnitude));
}

// elements of a [dx, dy, dz, 3] volume, or a DVA_ERR_* code
static int64_t elastic_volume(int64_t dx, int64_t dy, int64_t dz) {
  if (dx < 1 || dy < 1 || dz < 1) return DVA_ERR_INVALID;
  if (dx > EL_MAX_ELEMS || dy > EL_MAX_ELEMS || dz > EL_MAX_ELEMS) return DVA_ERR_UNSUPPORTED;
  const int64_t xy = dx * dy;                           // < 2^62
  if (xy > EL_MAX_ELEMS || xy * dz > EL_MAX_ELEMS / 3) return DVA_ERR_UNSUPPORTED;
  return xy * dz * 3;
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_minmax3_workspace_bytes(void) { return (int64_t)align_up((size_t)EL_MINMAX_BLOCKS * 6 * sizeof(float)); }

int dva_minmax3_f32(const float* pos, int64_t n, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 1 || !pos || !out || !workspace) return DVA_ERR_INVALID;
  if (workspace_bytes < dva_minmax3_workspace_bytes()) return DVA_ERR_INVALID;
  if (n > EL_MAX_ELEMS / 3) return DVA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = (n + EL_TPB - 1) / EL_TPB;
  if (blocks > EL_MINMAX_BLOCKS) blocks = EL_MINMAX_BLOCKS;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(minmax3_partial_kernel, dim3((unsigned)blocks), dim3(EL_TPB), 0, s, pos, n, part);
  hipLaunchKernelGGL(minmax3_final_kernel, dim3(1), dim3(EL_TPB), 0, s, (const float*)part, (int)blocks, out);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int64_t dva_elastic_workspace_bytes(int64_t dx, int64_t dy, int64_t dz) {
  const int64_t total = elastic_volume(dx, dy, dz);
  if (total < 0) return total;
  return (int64_t)(2 * align_up((size_t)total * sizeof(float)));
}

int dva_elastic_smooth(const float* noise, int64_t dx, int64_t dy, int64_t dz, float* out, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  const int64_t total = elastic_volume(dx, dy, dz);
  if (total < 0) return (int)total;
  if (!noise || !out || !workspace) return DVA_ERR_INVALID;
  if (workspace_bytes < dva_elastic_workspace_bytes(dx, dy, dz)) return DVA_ERR_INVALID;
  if (total > EL_MAX_ELEMS - EL_TPB) return DVA_ERR_UNSUPPORTED;       // the rounded-up grid stays an int
  hipStream_t s = (hipStream_t)stream;
  float* buf[2] = {(float*)workspace, (float*)((char*)workspace + align_up((size_t)total * sizeof(float)))};
  const int stride[3] = {(int)(dy * dz * 3), (int)(dz * 3), 3};
  const int dim[3] = {(int)dx, (int)dy, (int)dz};
  const dim3 grid((unsigned)((total + EL_TPB - 1) / EL_TPB));
  const float* src = noise;
  for (int pass = 0; pass < 6; ++pass) {
    float* dst = pass == 5 ? out : buf[pass & 1];
    hipLaunchKernelGGL(elastic_smooth_kernel, grid, dim3(EL_TPB), 0, s, src, dst, (int)total, stride[pass % 3],
                       dim[pass % 3]);
    src = dst;
  }
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_elastic_displace(const float* pos, int64_t n, const float* field, const double* axes, int64_t dx, int64_t dy,
                         int64_t dz, double magnitude, float* out, void* stream) {
  if (n < 0) return DVA_ERR_INVALID;
  const int64_t total = elastic_volume(dx, dy, dz);
  if (total < 0) return (int)total;
  if (dx < 2 || dy < 2 || dz < 2) return DVA_ERR_INVALID;              // a cell needs two knots
  if (!field || !axes || (n > 0 && (!pos || !out))) return DVA_ERR_INVALID;
  if (n > EL_MAX_ELEMS / 3) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return DVA_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + EL_TPB - 1) / EL_TPB));
  const int64_t knots = dx + dy + dz;
  if (knots <= EL_LDS_AXES)
    hipLaunchKernelGGL(elastic_displace_kernel<true>, grid, dim3(EL_TPB), (size_t)knots * sizeof(double), s, pos, n,
                       field, axes, (int)dx, (int)dy, (int)dz, magnitude, out);
  else
    hipLaunchKernelGGL(elastic_displace_kernel<false>, grid, dim3(EL_TPB), 0, s, pos, n, field, axes, (int)dx, (int)dy,
                       (int)dz, magnitude, out);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
