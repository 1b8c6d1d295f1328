// The view-level loss of the image-only models (reference: models/segmentation/multimodal/no3d.py:145-154):
// nll_loss(log_softmax(last_view_x_mod), repeat_interleave(labels, views per point)) for views that are a gather of
// rows, x_view[v] = rows[row_idx[v]].  Every view of a row has the row's log-softmax, so loss and gradient are functions
// of the per-row label histogram cnt[r][c] = #{views v of row r whose point is labelled c}:
//
//   loss          = sum_r sum_c cnt[r][c] w_c (-logp_r[c]) / sum_r sum_c cnt[r][c] w_c
//   d loss / rows = (sum_c' cnt[r][c'] w_c') softmax_r[c] - cnt[r][c] w_c,   over the same denominator.
//
// The counts are integers (int32 atomics): exact, so two runs give the same bits.  The class weights enter in the
// dense passes, one thread per row (K <= 64); numerator and denominator are reduced in fp64 from per-block partials in
// a fixed order, as the point-level loss of segloss.hip.  No [V, K] and no [V] tensor exists anywhere.
#include "dva_common.h"

namespace dva {

constexpr int VL_THREADS = 256;
constexpr int VL_MAX_BLOCKS = 1024;      // per-block partials of the reduction
constexpr int VL_MAX_K = 64;

// sum of v over the block's 256 threads, in a fixed order; every thread gets the result.  red: LDS [256]
__device__ __forceinline__ double vl_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = VL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// row_idx null: the identity (a plain [V, K] tensor).  The owner of view v is the last point i with csr[i] <= v.
__global__ __launch_bounds__(VL_THREADS) void view_counts_kernel(const int32_t* __restrict__ row_idx, int64_t V,
                                                                  const int64_t* __restrict__ csr,
                                                                  const int64_t* __restrict__ labels, int64_t N,
                                                                  int64_t ignore, int64_t R, int K,
                                                                  int32_t* __restrict__ cnt) {
  for (int64_t v = blockIdx.x * (int64_t)VL_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * VL_THREADS) {
    int64_t lo = 0, hi = N + 1;                  // first index with csr[index] > v, in [0, N + 1]
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (csr[mid] <= v) lo = mid + 1; else hi = mid;
    }
    const int64_t owner = lo - 1;
    if (owner < 0 || owner >= N) continue;       // a view outside the pointers: owned by no point
    const int64_t lab = labels[owner];
    if (lab == ignore || lab < 0 || lab >= K) continue;
    const int64_t r = row_idx ? (int64_t)row_idx[v] : v;
    if (r < 0 || r >= R) continue;
    atomicAdd(&cnt[r * K + lab], 1);
  }
}

template <typename T>
__global__ __launch_bounds__(VL_THREADS) void view_nll_fwd_kernel(const T* __restrict__ rows,
                                                                   const int32_t* __restrict__ cnt,
                                                                   const float* __restrict__ weight, int64_t R, int K,
                                                                   double* __restrict__ partial) {
  __shared__ double red[VL_THREADS];
  double num = 0.0, den = 0.0;
  for (int64_t r = blockIdx.x * (int64_t)VL_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * VL_THREADS) {
    const int64_t base = r * K;
    int any = 0;
    for (int j = 0; j < K; ++j) any |= cnt[base + j];
    if (!any) continue;                           // a row that no counted view reads takes no part, whatever it holds
    float m = Elt<T>::ld(rows, base);
    for (int j = 1; j < K; ++j) m = fmaxf(m, Elt<T>::ld(rows, base + j));
    float s = 0.f;
    for (int j = 0; j < K; ++j) s += expf(Elt<T>::ld(rows, base + j) - m);
    const float ls = logf(s);
    for (int j = 0; j < K; ++j) {
      const int c = cnt[base + j];
      if (!c) continue;
      const float lp = (Elt<T>::ld(rows, base + j) - m) - ls;
      const double w = (double)c * (weight ? (double)weight[j] : 1.0);
      num += w * -(double)lp;
      den += w;
    }
  }
  const double bn = vl_block_sum(num, red);
  const double bd = vl_block_sum(den, red);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = bn;
    partial[2 * blockIdx.x + 1] = bd;
  }
}

__global__ __launch_bounds__(VL_THREADS) void view_nll_finish_kernel(const double* __restrict__ partial, int n_blocks,
                                                                      double* __restrict__ numden,
                                                                      float* __restrict__ loss) {
  __shared__ double red[VL_THREADS];
  double num = 0.0, den = 0.0;
  for (int b = threadIdx.x; b < n_blocks; b += VL_THREADS) {
    num += partial[2 * b];
    den += partial[2 * b + 1];
  }
  num = vl_block_sum(num, red);
  den = vl_block_sum(den, red);
  if (threadIdx.x == 0) {
    numden[0] = num;
    numden[1] = den;
    loss[0] = (float)(num / den);            // 0 / 0 = NaN when no view takes part, as torch
  }
}

template <typename T>
__global__ __launch_bounds__(VL_THREADS) void view_nll_bwd_kernel(const T* __restrict__ rows,
                                                                   const int32_t* __restrict__ cnt,
                                                                   const float* __restrict__ weight,
                                                                   const double* __restrict__ numden,
                                                                   const float* __restrict__ grad_loss, int64_t R,
                                                                   int K, T* __restrict__ grad_rows) {
  const double coef = (double)grad_loss[0] / numden[1];
  for (int64_t r = blockIdx.x * (int64_t)VL_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * VL_THREADS) {
    const int64_t base = r * K;
    double tot = 0.0;
    for (int j = 0; j < K; ++j) {
      const int c = cnt[base + j];
      if (c) tot += (double)c * (weight ? (double)weight[j] : 1.0);
    }
    if (tot == 0.0) {                             // no counted view (or only zero-weight classes): no gradient
      for (int j = 0; j < K; ++j) Elt<T>::st(grad_rows, base + j, 0.f);
      continue;
    }
    float m = Elt<T>::ld(rows, base);
    for (int j = 1; j < K; ++j) m = fmaxf(m, Elt<T>::ld(rows, base + j));
    float s = 0.f;
    for (int j = 0; j < K; ++j) s += expf(Elt<T>::ld(rows, base + j) - m);
    const float ls = logf(s);
    for (int j = 0; j < K; ++j) {
      const float lp = (Elt<T>::ld(rows, base + j) - m) - ls;
      const double cw = (double)cnt[base + j] * (weight ? (double)weight[j] : 1.0);
      Elt<T>::st(grad_rows, base + j, (float)(coef * (tot * (double)expf(lp) - cw)));
    }
  }
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_view_nll_workspace_bytes(void) { return (int64_t)align_up(VL_MAX_BLOCKS * 2 * sizeof(double)); }

int dva_view_nll_counts(const int32_t* row_idx, int64_t n_views, const int64_t* csr_idx, const int64_t* labels,
                        int64_t n_points, int64_t ignore_index, int64_t n_rows, int32_t K, int32_t* cnt,
                        void* stream) {
  if (n_views < 0 || n_points < 0 || n_rows < 0 || K < 1) return DVA_ERR_INVALID;
  if (K > VL_MAX_K || n_rows * (int64_t)K >= (1LL << 31) || n_views > 0x7fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n_rows == 0) return DVA_OK;
  if (!cnt || !csr_idx || (n_points > 0 && !labels)) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  zero_words(cnt, n_rows * K, s);
  if (n_views > 0 && n_points > 0)
    hipLaunchKernelGGL(view_counts_kernel, dim3(capped_grid(n_views, VL_THREADS, 8192)), dim3(VL_THREADS), 0, s, row_idx,
                       n_views, csr_idx, labels, n_points, ignore_index, n_rows, K, cnt);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_view_nll_fwd(const void* rows, int32_t dtype, const int32_t* cnt, const float* weight, int64_t n_rows,
                     int32_t K, float* loss, double* numden, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_rows < 0 || K < 1 || !dtype_ok(dtype)) return DVA_ERR_INVALID;
  if (K > VL_MAX_K || n_rows * (int64_t)K >= (1LL << 31)) return DVA_ERR_UNSUPPORTED;
  if (!loss || !numden || !workspace || (n_rows > 0 && (!rows || !cnt))) return DVA_ERR_INVALID;
  if (workspace_bytes < dva_view_nll_workspace_bytes()) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const int blocks = capped_grid(n_rows, VL_THREADS, VL_MAX_BLOCKS);
  const bool known = with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL(view_nll_fwd_kernel<T>, dim3(blocks), dim3(VL_THREADS), 0, s, (const T*)rows, cnt, weight, n_rows,
                       K, partial);
  });
  if (!known) return DVA_ERR_INVALID;
  hipLaunchKernelGGL(view_nll_finish_kernel, dim3(1), dim3(VL_THREADS), 0, s, partial, blocks, numden, loss);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_view_nll_bwd(const void* rows, int32_t dtype, const int32_t* cnt, const float* weight, const double* numden,
                     const float* grad_loss, int64_t n_rows, int32_t K, void* grad_rows, void* stream) {
  if (n_rows < 0 || K < 1 || !dtype_ok(dtype)) return DVA_ERR_INVALID;
  if (K > VL_MAX_K || n_rows * (int64_t)K >= (1LL << 31)) return DVA_ERR_UNSUPPORTED;
  if (n_rows == 0) return DVA_OK;
  if (!rows || !cnt || !numden || !grad_loss || !grad_rows) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = capped_grid(n_rows, VL_THREADS, 8192);
  const bool known = with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL(view_nll_bwd_kernel<T>, dim3(blocks), dim3(VL_THREADS), 0, s, (const T*)rows, cnt, weight, numden,
                       grad_loss, n_rows, K, (T*)grad_rows);
  });
  if (!known) return DVA_ERR_INVALID;
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
