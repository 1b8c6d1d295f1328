// The tail of the segmentation step for gfx950 (reference: models/segmentation/sparseconv3d.py:42-55 log_softmax +
// nll_loss + lovasz_softmax, metrics/lovasz_loss.py:155-202, metrics/segmentation_tracker.py:71-91 argmax + bincount).
//
//   log-softmax + weighted NLL   one thread per row (C <= 64); the loss is reduced in fp64 from per-block partials
//                                in a fixed order (no float atomics): two runs give the same bits.
//   confusion counts             one thread per row, per-block LDS histogram (int32), added to the int64 matrix with
//                                integer atomics.
//   Lovasz-softmax               one 64-bit key per (point, class) -- class | ~bits(err) | fg | sign -- one stable
//                                radix sort over the class and error bits, then a segmented pass per class whose
//                                Jaccard values come from INTEGER counts in fp64: J_k = 1 - (G - n_k) / (G + k - n_k).
//                                The increments J_k - J_{k-1} are the gradient.  Nothing is read back to the host:
//                                ignored points and unused classes sort into a sentinel segment at the end.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "dva_common.h"

namespace dva {

constexpr int SEG_THREADS = 256;
constexpr int SEG_MAX_BLOCKS = 1024;                      // per-block partials of the NLL reduction
constexpr int LOVASZ_ITEMS = DVA_LOVASZ_TILE / SEG_THREADS;
static_assert(LOVASZ_ITEMS * SEG_THREADS == DVA_LOVASZ_TILE, "tile = threads x items");
constexpr int SEG_MAX_C = 64;


// sum of v over the block's 256 threads, in a fixed order; every thread gets the result.  red: LDS [256]
template <typename V>
__device__ __forceinline__ V block_sum(V v, V* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = SEG_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// ---------------------------------------------------------------------------------------------------------------
// log-softmax + NLL
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void seg_nll_fwd_kernel(const T* __restrict__ logits,
                                                                   const int64_t* __restrict__ labels,
                                                                   const float* __restrict__ weight, int64_t ignore,
                                                                   int64_t P, int C, float* __restrict__ logp,
                                                                   double* __restrict__ partial) {
  __shared__ double red[SEG_THREADS];
  double num = 0.0, den = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)SEG_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * SEG_THREADS) {
    const int64_t base = i * C;
    float m = Elt<T>::ld(logits, base);
    for (int j = 1; j < C; ++j) m = fmaxf(m, Elt<T>::ld(logits, base + j));
    float s = 0.f;
    for (int j = 0; j < C; ++j) s += expf(Elt<T>::ld(logits, base + j) - m);
    const float ls = logf(s);
    const int64_t lab = labels[i];
    const bool counted = lab != ignore && lab >= 0 && lab < C;
    for (int j = 0; j < C; ++j) {
      const float lp = (Elt<T>::ld(logits, base + j) - m) - ls;
      logp[base + j] = lp;
      if (counted && j == (int)lab) {
        const double w = weight ? (double)weight[lab] : 1.0;
        num += w * -(double)lp;
        den += w;
      }
    }
  }
  const double bn = block_sum(num, red);
  const double bd = block_sum(den, red);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = bn;
    partial[2 * blockIdx.x + 1] = bd;
  }
}

__global__ __launch_bounds__(SEG_THREADS) void seg_nll_finish_kernel(const double* __restrict__ partial, int n_blocks,
                                                                      double* __restrict__ numden,
                                                                      float* __restrict__ loss) {
  __shared__ double red[SEG_THREADS];
  double num = 0.0, den = 0.0;
  for (int b = threadIdx.x; b < n_blocks; b += SEG_THREADS) {
    num += partial[2 * b];
    den += partial[2 * b + 1];
  }
  num = block_sum(num, red);
  den = block_sum(den, red);
  if (threadIdx.x == 0) {
    numden[0] = num;
    numden[1] = den;
    loss[0] = (float)(num / den);            // 0 / 0 = NaN when every label is ignored, as torch
  }
}

template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void seg_nll_bwd_kernel(const float* __restrict__ logp,
                                                                   const int64_t* __restrict__ labels,
                                                                   const float* __restrict__ weight,
                                                                   const double* __restrict__ numden,
                                                                   const float* __restrict__ grad_loss,
                                                                   const float* __restrict__ grad_logp, int64_t ignore,
                                                                   int64_t P, int C, T* __restrict__ grad_logits) {
  const double den = numden[1];
  const double up = grad_loss ? (double)grad_loss[0] : 0.0;
  for (int64_t i = blockIdx.x * (int64_t)SEG_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * SEG_THREADS) {
    const int64_t base = i * C;
    const int64_t lab = labels[i];
    const bool counted = grad_loss && lab != ignore && lab >= 0 && lab < C;
    float coef = 0.f;
    if (counted) coef = (float)(-((weight ? (double)weight[lab] : 1.0) / den) * up);
    float sum = coef;
    if (grad_logp)
      for (int j = 0; j < C; ++j) sum += grad_logp[base + j];
    for (int j = 0; j < C; ++j) {
      float g = grad_logp ? grad_logp[base + j] : 0.f;
      if (counted && j == (int)lab) g += coef;
      Elt<T>::st(grad_logits, base + j, g - expf(logp[base + j]) * sum);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// confusion counts
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void confusion_kernel(const T* __restrict__ outputs,
                                                                 const int64_t* __restrict__ labels, int64_t ignore,
                                                                 int64_t P, int C, long long* __restrict__ counts,
                                                                 long long* __restrict__ n_bad) {
  __shared__ int hist[SEG_MAX_C * SEG_MAX_C];
  __shared__ int bad;
  for (int k = threadIdx.x; k < C * C; k += SEG_THREADS) hist[k] = 0;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)SEG_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * SEG_THREADS) {
    const int64_t lab = labels[i];
    if (lab == ignore) continue;
    if (lab < 0 || lab >= C) {
      atomicAdd(&bad, 1);
      continue;
    }
    const int64_t base = i * C;
    float best = Elt<T>::ld(outputs, base);
    int arg = 0;
    for (int j = 1; j < C; ++j) {                       // np.argmax: the first maximum; a NaN is the maximum
      const float x = Elt<T>::ld(outputs, base + j);
      if (!(best != best) && (x > best || x != x)) {
        best = x;
        arg = j;
      }
    }
    atomicAdd(&hist[(int)lab * C + arg], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < C * C; k += SEG_THREADS)
    if (hist[k]) atomicAdd((unsigned long long*)&counts[k], (unsigned long long)hist[k]);
  if (threadIdx.x == 0 && bad) atomicAdd((unsigned long long*)n_bad, (unsigned long long)bad);
}

// ---------------------------------------------------------------------------------------------------------------
// Lovasz-softmax
// ---------------------------------------------------------------------------------------------------------------
// key = class << 35 | (0xFFFFFFFF - bits(err)) << 3 | fg << 2 | sign ; the sort reads bits [3, 35 + class bits) only
constexpr int LV_LOW_BITS = 3;
constexpr int LV_CLASS_SHIFT = 35;

static int lovasz_class_bits(int C) {
  int b = 1;
  while ((1 << b) <= C) ++b;     // classes 0 .. C (C = the sentinel)
  return b;
}

struct LovaszLayout {
  uint64_t *k0, *k1;
  uint32_t *v0, *v1, *cnt, *tile_cnt;
  double* tile_loss;
  char* temp;
  size_t temp_bytes, total;
  int64_t tiles;
};

// cnt: uint32 [C + 1] = foreground points per class, then the number of valid points
__global__ __launch_bounds__(SEG_THREADS) void lovasz_keys_kernel(const float* __restrict__ probas,
                                                                   const int64_t* __restrict__ labels, int64_t ignore,
                                                                   int use_ignore,
                                                                   const uint8_t* __restrict__ class_mask, int64_t P,
                                                                   int C, uint64_t* __restrict__ keys,
                                                                   uint32_t* __restrict__ vals,
                                                                   uint32_t* __restrict__ cnt) {
  __shared__ uint32_t hist[SEG_MAX_C + 1];
  if (threadIdx.x <= C) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t N = P * C;
  for (int64_t e = blockIdx.x * (int64_t)SEG_THREADS + threadIdx.x; e < N; e += (int64_t)gridDim.x * SEG_THREADS) {
    const int64_t i = e / C;
    const int c = (int)(e - i * C);
    const int64_t lab = labels[i];
    const bool valid = !(use_ignore && lab == ignore);
    const bool enabled = class_mask ? class_mask[c] != 0 : true;
    const bool is_fg = lab == c;
    const float fg = is_fg ? 1.f : 0.f;
    const float p = probas[e];
    const float err = fabsf(fg - p);
    const float d = p - fg;
    const uint32_t sgn = d > 0.f ? 1u : (d < 0.f ? 2u : 0u);
    const uint64_t cls = (valid && enabled) ? (uint64_t)c : (uint64_t)C;
    keys[e] = (cls << LV_CLASS_SHIFT) | ((uint64_t)(0xFFFFFFFFu - __float_as_uint(err)) << LV_LOW_BITS) |
              ((uint64_t)(is_fg ? 1u : 0u) << 2) | sgn;
    vals[e] = (uint32_t)e;
    if (valid) {
      if (is_fg) atomicAdd(&hist[c], 1u);
      if (c == 0) atomicAdd(&hist[C], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x <= C && hist[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], hist[threadIdx.x]);
}

struct LovaszClass {
  int used, rank, n_used;
  uint32_t G, V;
};

// Which classes take part, from the device-side counts: used = enabled and (present or not present_only);
// rank = enabled classes before c (their segments precede c's in the sorted array).
__device__ __forceinline__ LovaszClass lovasz_class(const uint32_t* cnt, const uint8_t* class_mask, int present_only,
                                                    int C, int c) {
  LovaszClass r;
  r.used = 0; r.rank = 0; r.n_used = 0;
  r.V = cnt[C];
  r.G = cnt[c];
  for (int j = 0; j < C; ++j) {
    const bool enabled = class_mask ? class_mask[j] != 0 : true;
    const bool used = enabled && r.V > 0 && (!present_only || cnt[j] > 0);
    if (enabled && j < c) ++r.rank;
    if (used) ++r.n_used;
    if (used && j == c) r.used = 1;
  }
  return r;
}

// foreground points per tile of every used class: tile_cnt[c * tiles + t]
__global__ __launch_bounds__(SEG_THREADS) void lovasz_count_kernel(const uint64_t* __restrict__ keys,
                                                                    const uint32_t* __restrict__ cnt,
                                                                    const uint8_t* __restrict__ class_mask,
                                                                    int present_only, int C, int64_t tiles,
                                                                    uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t red[SEG_THREADS];
  const int c = blockIdx.y;
  const int64_t t = blockIdx.x;
  const LovaszClass k = lovasz_class(cnt, class_mask, present_only, C, c);
  const int64_t first = t * DVA_LOVASZ_TILE;
  if (!k.used || first >= (int64_t)k.V) return;          // uniform over the block
  const int64_t start = (int64_t)k.rank * k.V;
  uint32_t n = 0;
#pragma unroll
  for (int r = 0; r < LOVASZ_ITEMS; ++r) {
    const int64_t pos = first + r * SEG_THREADS + threadIdx.x;
    if (pos < (int64_t)k.V) n += (uint32_t)((keys[start + pos] >> 2) & 1u);
  }
  n = block_sum(n, red);
  if (threadIdx.x == 0) tile_cnt[c * tiles + t] = n;
}

// tile_cnt[c * tiles + t] -> the number of foreground points in the tiles before t (exclusive prefix, in place): one
// block per class walks its live tiles in chunks of 256 with an LDS scan, so the carry costs O(tiles), not O(tiles^2)
__global__ __launch_bounds__(SEG_THREADS) void lovasz_prefix_kernel(const uint32_t* __restrict__ cnt,
                                                                     const uint8_t* __restrict__ class_mask,
                                                                     int present_only, int C, int64_t tiles,
                                                                     uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t scan[SEG_THREADS];
  const int c = blockIdx.x;
  const LovaszClass k = lovasz_class(cnt, class_mask, present_only, C, c);
  if (!k.used) return;                                    // uniform over the block
  const int64_t live = ((int64_t)k.V + DVA_LOVASZ_TILE - 1) / DVA_LOVASZ_TILE;     // <= tiles
  uint32_t carry = 0;
  for (int64_t base = 0; base < live; base += SEG_THREADS) {
    const int64_t t = base + threadIdx.x;
    const uint32_t v = t < live ? tile_cnt[c * tiles + t] : 0u;
    __syncthreads();                                      // the previous chunk's total has been read
    scan[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < SEG_THREADS; s <<= 1) {           // inclusive scan (Hillis-Steele)
      const uint32_t add = (int)threadIdx.x >= s ? scan[threadIdx.x - s] : 0u;
      __syncthreads();
      scan[threadIdx.x] += add;
      __syncthreads();
    }
    if (t < live) tile_cnt[c * tiles + t] = carry + scan[threadIdx.x] - v;
    carry += scan[SEG_THREADS - 1];
  }
}

__global__ __launch_bounds__(SEG_THREADS) void lovasz_scan_kernel(const uint64_t* __restrict__ keys,
                                                                   const uint32_t* __restrict__ vals,
                                                                   const uint32_t* __restrict__ cnt,
                                                                   const uint8_t* __restrict__ class_mask,
                                                                   int present_only, int C, int64_t tiles,
                                                                   const uint32_t* __restrict__ tile_cnt,
                                                                   double* __restrict__ tile_loss,
                                                                   float* __restrict__ grad) {
  __shared__ double redd[SEG_THREADS];
  __shared__ uint32_t wave_n[SEG_THREADS / DVA_WAVE];
  const int c = blockIdx.y;
  const int64_t t = blockIdx.x;
  const LovaszClass k = lovasz_class(cnt, class_mask, present_only, C, c);
  const int64_t first = t * DVA_LOVASZ_TILE;
  if (!k.used || first >= (int64_t)k.V) return;          // uniform over the block
  const int64_t start = (int64_t)k.rank * k.V;
  uint32_t carry = tile_cnt[c * tiles + t];               // foreground points in the tiles before this one
  const int lane = threadIdx.x & (DVA_WAVE - 1), wave = threadIdx.x / DVA_WAVE;
  const double G = (double)k.G, inv_used = 1.0 / (double)k.n_used;
  double loss = 0.0;
  for (int r = 0; r < LOVASZ_ITEMS; ++r) {
    const int64_t pos = first + r * SEG_THREADS + threadIdx.x;
    const bool live = pos < (int64_t)k.V;
    const uint64_t key = live ? keys[start + pos] : 0;
    const uint32_t fg = (uint32_t)((key >> 2) & 1u);
    const unsigned long long ballot = __ballot(fg != 0);
    const uint32_t incl = (uint32_t)__popcll(ballot & ((2ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEG_THREADS / DVA_WAVE; ++w) {
      if (w < wave) off += wave_n[w];
      total += wave_n[w];
    }
    if (live) {
      const double nk = (double)(carry + off + incl);       // foreground among the first kk
      const double kk = (double)(pos + 1);
      const double jk = 1.0 - (G - nk) / (G + kk - nk);
      const double n1 = nk - (double)fg, k1 = kk - 1.0;
      const double j1 = pos == 0 ? 0.0 : 1.0 - (G - n1) / (G + k1 - n1);
      const double g = jk - j1;
      const float err = __uint_as_float(0xFFFFFFFFu - (uint32_t)(key >> LV_LOW_BITS));
      loss += (double)err * g;
      const uint32_t sgn = (uint32_t)(key & 3u);
      const double sg = sgn == 1u ? 1.0 : (sgn == 2u ? -1.0 : 0.0);
      grad[vals[start + pos]] = (float)(sg * g * inv_used);
    }
    carry += total;
  }
  loss = block_sum(loss, redd);
  if (threadIdx.x == 0) tile_loss[c * tiles + t] = loss;
}

__global__ __launch_bounds__(SEG_THREADS) void lovasz_finish_kernel(const uint32_t* __restrict__ cnt,
                                                                     const uint8_t* __restrict__ class_mask,
                                                                     int present_only, int C, int64_t tiles,
                                                                     const double* __restrict__ tile_loss,
                                                                     float* __restrict__ loss) {
  __shared__ double red[SEG_THREADS];
  double total = 0.0;
  int n_used = 0;
  for (int c = 0; c < C; ++c) {                           // class after class, each summed in a fixed order
    const LovaszClass k = lovasz_class(cnt, class_mask, present_only, C, c);
    n_used = k.n_used;
    if (!k.used) continue;                                // uniform over the block
    const int64_t live = ((int64_t)k.V + DVA_LOVASZ_TILE - 1) / DVA_LOVASZ_TILE;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < live; t += SEG_THREADS) s += tile_loss[c * tiles + t];
    total += block_sum(s, red);
  }
  if (threadIdx.x == 0) loss[0] = n_used > 0 ? (float)(total / (double)n_used) : 0.f;
}

static hipError_t lovasz_sort(void* temp, size_t& tmp, rocprim::double_buffer<uint64_t>& k,
                              rocprim::double_buffer<uint32_t>& v, size_t n, int C, hipStream_t s) {
  return rocprim::radix_sort_pairs(temp, tmp, k, v, n, LV_LOW_BITS, LV_CLASS_SHIFT + lovasz_class_bits(C), s);
}

static int lovasz_layout(void* ws, int64_t P, int C, LovaszLayout* L) {
  const size_t N = (size_t)P * C;
  size_t tmp = 0;
  rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
  rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
  if (lovasz_sort(nullptr, tmp, k, v, N, C, (hipStream_t)0) != hipSuccess) return DVA_ERR_LAUNCH;
  L->tiles = (P + DVA_LOVASZ_TILE - 1) / DVA_LOVASZ_TILE;
  Carver c(ws);
  L->k0 = c.take<uint64_t>(N);
  L->k1 = c.take<uint64_t>(N);
  L->v0 = c.take<uint32_t>(N);
  L->v1 = c.take<uint32_t>(N);
  L->cnt = c.take<uint32_t>((size_t)(C + 1));
  L->tile_cnt = c.take<uint32_t>((size_t)C * L->tiles);
  L->tile_loss = c.take<double>((size_t)C * L->tiles);
  L->temp_bytes = tmp;
  L->temp = c.take<char>(tmp);
  L->total = c.used();
  return DVA_OK;
}

// 1 <= C <= 64 and P * C < 2^31
static int seg_shape(int64_t P, int32_t C) {
  if (P < 0 || C < 1) return DVA_ERR_INVALID;
  if (C > SEG_MAX_C) return DVA_ERR_UNSUPPORTED;
  if (P > 0x7fffffffLL / C) return DVA_ERR_UNSUPPORTED;
  if (P * C >= 0x80000000LL) return DVA_ERR_UNSUPPORTED;
  return DVA_OK;
}

}  // namespace dva

using namespace dva;

extern "C" {

int dva_lovasz_tile(void) { return DVA_LOVASZ_TILE; }

int64_t dva_seg_nll_workspace_bytes(void) { return (int64_t)SEG_MAX_BLOCKS * 2 * sizeof(double); }

int dva_seg_logsoftmax_nll_fwd(const void* logits, int32_t dtype, const int64_t* labels, const float* weight,
                               int64_t ignore_index, int64_t P, int32_t C, float* log_probs, float* loss,
                               double* numden, void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = seg_shape(P, C);
  if (rc) return rc;
  if (!dtype_ok(dtype)) return DVA_ERR_INVALID;
  if (!loss || !numden || !workspace || workspace_bytes < dva_seg_nll_workspace_bytes()) return DVA_ERR_INVALID;
  if (P > 0 && (!logits || !labels || !log_probs)) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const int grid = capped_grid(P, SEG_THREADS, SEG_MAX_BLOCKS);
  const bool known = with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL(seg_nll_fwd_kernel<T>, dim3(grid), dim3(SEG_THREADS), 0, s, (const T*)logits, labels, weight,
                       ignore_index, P, (int)C, log_probs, partial);
  });
  if (!known) return DVA_ERR_INVALID;
  hipLaunchKernelGGL(seg_nll_finish_kernel, dim3(1), dim3(SEG_THREADS), 0, s, partial, grid, numden, loss);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_seg_logsoftmax_nll_bwd(const float* log_probs, const int64_t* labels, const float* weight,
                               const double* numden, const float* grad_loss, const float* grad_log_probs,
                               int64_t ignore_index, int64_t P, int32_t C, void* grad_logits, int32_t dtype,
                               void* stream) {
  int rc = seg_shape(P, C);
  if (rc) return rc;
  if (!dtype_ok(dtype)) return DVA_ERR_INVALID;
  if (!numden) return DVA_ERR_INVALID;
  if (P == 0) return DVA_OK;
  if (!log_probs || !labels || !grad_logits) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int grid = capped_grid(P, SEG_THREADS, 1 << 16);
  const bool known = with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL(seg_nll_bwd_kernel<T>, dim3(grid), dim3(SEG_THREADS), 0, s, log_probs, labels, weight, numden,
                       grad_loss, grad_log_probs, ignore_index, P, (int)C, (T*)grad_logits);
  });
  if (!known) return DVA_ERR_INVALID;
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_confusion_counts(const void* outputs, int32_t dtype, const int64_t* labels, int64_t ignore_index, int64_t P,
                         int32_t C, int64_t* counts, int64_t* n_bad, void* stream) {
  int rc = seg_shape(P, C);
  if (rc) return rc;
  if (!dtype_ok(dtype)) return DVA_ERR_INVALID;
  if (!counts || !n_bad) return DVA_ERR_INVALID;
  if (P == 0) return DVA_OK;
  if (!outputs || !labels) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int grid = capped_grid(P, SEG_THREADS, 2048);
  const bool known = with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL(confusion_kernel<T>, dim3(grid), dim3(SEG_THREADS), 0, s, (const T*)outputs, labels, ignore_index,
                       P, (int)C, (long long*)counts, (long long*)n_bad);
  });
  if (!known) return DVA_ERR_INVALID;
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int64_t dva_lovasz_workspace_bytes(int64_t P, int32_t C) {
  int rc = seg_shape(P, C);
  if (rc) return rc;
  if (P == 0) return 256;
  LovaszLayout L;
  rc = lovasz_layout(nullptr, P, C, &L);
  if (rc) return rc;
  return (int64_t)L.total;
}

int dva_lovasz_softmax(const float* probas, const int64_t* labels, int64_t P, int32_t C, int64_t ignore_index,
                       int32_t use_ignore, const uint8_t* class_mask, int32_t present_only, float* loss, float* grad,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = seg_shape(P, C);
  if (rc) return rc;
  if (!loss) return DVA_ERR_INVALID;
  if (P > 0 && (!probas || !labels || !grad || !workspace)) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) {
    zero_words(loss, 1, s);
    DVA_CHECK_LAUNCH();
    return DVA_OK;
  }
  LovaszLayout L;
  rc = lovasz_layout(workspace, P, C, &L);
  if (rc) return rc;
  if ((int64_t)L.total > workspace_bytes) return DVA_ERR_INVALID;
  const int64_t N = P * C;
  rocprim::double_buffer<uint64_t> keys(L.k0, L.k1);
  rocprim::double_buffer<uint32_t> vals(L.v0, L.v1);
  zero_words(L.cnt, C + 1, s);          // kernels, not memset nodes: the entry is capturable (dva_common.h)
  zero_words(grad, N, s);
  hipLaunchKernelGGL(lovasz_keys_kernel, dim3(capped_grid(N, SEG_THREADS, 8192)), dim3(SEG_THREADS), 0, s, probas,
                     labels, ignore_index, (int)use_ignore, class_mask, P, (int)C, keys.current(), vals.current(),
                     L.cnt);
  size_t tmp = L.temp_bytes;
  if (lovasz_sort(L.temp, tmp, keys, vals, (size_t)N, C, s) != hipSuccess) return DVA_ERR_LAUNCH;
  const dim3 grid((unsigned)L.tiles, (unsigned)C);
  hipLaunchKernelGGL(lovasz_count_kernel, grid, dim3(SEG_THREADS), 0, s, keys.current(), L.cnt, class_mask,
                     (int)present_only, (int)C, L.tiles, L.tile_cnt);
  hipLaunchKernelGGL(lovasz_prefix_kernel, dim3((unsigned)C), dim3(SEG_THREADS), 0, s, L.cnt, class_mask,
                     (int)present_only, (int)C, L.tiles, L.tile_cnt);
  hipLaunchKernelGGL(lovasz_scan_kernel, grid, dim3(SEG_THREADS), 0, s, keys.current(), vals.current(), L.cnt,
                     class_mask, (int)present_only, (int)C, L.tiles, L.tile_cnt, L.tile_loss, grad);
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(SEG_THREADS), 0, s, L.cnt, class_mask, (int)present_only,
                     (int)C, L.tiles, L.tile_loss, loss);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
