// Voting on the raw cloud and K-NN interpolation of the votes for gfx950 (reference: metrics/s3dis_tracker.py:56-61,
// 94-118, metrics/segmentation_helpers.py SegmentationVoter, metrics/kitti360_tracker.py:144-152, 188-222;
// torch_geometric.nn.unpool.knn_interpolate).
//
//   vote accumulation   votes[ids] += outputs; counts[ids] += 1 where an id that occurs several times counts once: the
//                       LAST occurrence in ids.  Three passes, no float atomics: an integer atomicMax of the row
//                       position into one int32 slot per raw point picks the winner, the winning row alone adds its C
//                       values with plain loads and stores (lanes over (row, class): the outputs are read as one
//                       contiguous stream, a vote row as one contiguous segment), the last pass puts the touched slots
//                       back to -1.
//   K-NN interpolation  16 lanes per query (lane = class, class + 16, ...; 4 queries per wavefront): the k neighbour
//                       rows of x are gathered as contiguous segments, summed in rank order in fp32 with every
//                       operation rounded on its own, divided, and reduced to the first maximum across the 16 lanes
//                       with shuffles.  The confusion counts go through a per-block LDS histogram (int32) and integer
//                       atomics, as in segloss.hip.  Bandwidth-bound gathers: no MFMA.
#include "dva_common.h"

namespace dva {

constexpr int VOTE_THREADS = 256;
constexpr int VOTE_MAX_C = 64;
constexpr int VOTE_MAX_K = 128;
constexpr int VOTE_GROUP = 16;                            // lanes per query
constexpr int VOTE_ROWS = VOTE_THREADS / VOTE_GROUP;      // queries per block and step
constexpr int VOTE_PER_LANE = VOTE_MAX_C / VOTE_GROUP;    // classes per lane
static_assert(DVA_WAVE % VOTE_GROUP == 0, "a query's lanes stay inside one wavefront");

// ---------------------------------------------------------------------------------------------------------------
// vote accumulation
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VOTE_THREADS) void vote_claim_kernel(const int64_t* __restrict__ ids, int64_t P, int64_t N,
                                                                   int* __restrict__ slots,
                                                                   long long* __restrict__ n_bad) {
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int64_t p = blockIdx.x * (int64_t)VOTE_THREADS + threadIdx.x; p < P; p += (int64_t)gridDim.x * VOTE_THREADS) {
    const int64_t id = ids[p];
    if (id < 0 || id >= N)
      atomicAdd(&bad, 1);
    else
      atomicMax(&slots[id], (int)p);                      // the last occurrence wins
  }
  __syncthreads();
  if (threadIdx.x == 0 && bad) atomicAdd((unsigned long long*)n_bad, (unsigned long long)bad);
}

template <typename T>
__global__ __launch_bounds__(VOTE_THREADS) void vote_apply_kernel(const int64_t* __restrict__ ids,
                                                                   const T* __restrict__ outputs, int64_t P, int C,
                                                                   int64_t N, const int* __restrict__ slots,
                                                                   float* __restrict__ votes,
                                                                   int* __restrict__ counts) {
  const int64_t E = P * C;
  for (int64_t e = blockIdx.x * (int64_t)VOTE_THREADS + threadIdx.x; e < E; e += (int64_t)gridDim.x * VOTE_THREADS) {
    const int64_t p = e / C;
    const int c = (int)(e - p * C);
    const int64_t id = ids[p];
    if (id < 0 || id >= N) continue;
    if (slots[id] != (int)p) continue;                    // another row of this call holds the point
    const int64_t at = id * C + c;
    votes[at] = votes[at] + Elt<T>::ld(outputs, e);       // the one writer of this element in this call
    if (c == 0) counts[id] = counts[id] + 1;
  }
}

__global__ __launch_bounds__(VOTE_THREADS) void vote_release_kernel(const int64_t* __restrict__ ids, int64_t P,
                                                                     int64_t N, int* __restrict__ slots) {
  for (int64_t p = blockIdx.x * (int64_t)VOTE_THREADS + threadIdx.x; p < P; p += (int64_t)gridDim.x * VOTE_THREADS) {
    const int64_t id = ids[p];
    if (id >= 0 && id < N) slots[id] = -1;                // every writer of a slot stores the same value
  }
}

// ---------------------------------------------------------------------------------------------------------------
// K-NN interpolation
// ---------------------------------------------------------------------------------------------------------------
// is (a, ia) ahead of (b, ib) for numpy's argmax: a NaN is the maximum, equal values go to the lower index
__device__ __forceinline__ bool vote_ahead(float a, int ia, float b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}

__global__ __launch_bounds__(VOTE_THREADS) void knn_interpolate_kernel(
    const float* __restrict__ x, int64_t M, int C, const int* __restrict__ nbr, const float* __restrict__ d2, int64_t n,
    int k, const int* __restrict__ own, float* __restrict__ y, long long* __restrict__ pred,
    const int64_t* __restrict__ labels, int64_t ignore, long long* __restrict__ counts,
    long long* __restrict__ n_bad) {
  __shared__ int hist[VOTE_MAX_C * VOTE_MAX_C];
  __shared__ int bad;
  if (counts)
    for (int q = threadIdx.x; q < C * C; q += VOTE_THREADS) hist[q] = 0;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const int g = threadIdx.x / VOTE_GROUP, l = threadIdx.x % VOTE_GROUP;
  const float nan = __uint_as_float(0x7fc00000u);
  // the bound is uniform over the block: every lane reaches the shuffles
  for (int64_t i0 = blockIdx.x * (int64_t)VOTE_ROWS; i0 < n; i0 += (int64_t)gridDim.x * VOTE_ROWS) {
    const int64_t i = i0 + g;
    const bool live = i < n;
    bool ok = live;
    int64_t src = -1;                                     // the row of x this query keeps as it is
    if (live && own) {
      const int o = own[i];
      if (o >= 0) {
        if (o < M) src = o;
        else ok = false;
      }
    }
    float v[VOTE_PER_LANE];
#pragma unroll
    for (int q = 0; q < VOTE_PER_LANE; ++q) v[q] = 0.f;
    if (ok && src < 0) {
      float den = 0.f;
      for (int r = 0; r < k; ++r) {                       // rank order; the same for the 16 lanes of the query
        const int j = nbr[i * k + r];
        if (j < 0 || j >= M) {
          ok = false;
          break;
        }
        float d = d2[i * k + r];
        d = d < 1e-16f ? 1e-16f : d;                      // torch.clamp(min=1e-16): a NaN stays
        const float w = 1.0f / d;
        den = den + w;
#pragma unroll
        for (int q = 0; q < VOTE_PER_LANE; ++q) {
          const int c = l + q * VOTE_GROUP;
          if (c < C) v[q] = v[q] + x[(int64_t)j * C + c] * w;
        }
      }
#pragma unroll
      for (int q = 0; q < VOTE_PER_LANE; ++q) v[q] = v[q] / den;
    } else if (ok) {
#pragma unroll
      for (int q = 0; q < VOTE_PER_LANE; ++q) {
        const int c = l + q * VOTE_GROUP;
        if (c < C) v[q] = x[src * C + c];
      }
    }
    float best = -__builtin_inff();
    int arg = 1 << 30;                                    // a lane without a class loses to every class
#pragma unroll
    for (int q = 0; q < VOTE_PER_LANE; ++q) {
      const int c = l + q * VOTE_GROUP;
      if (c < C) {
        if (!ok) v[q] = nan;
        if (live && y) y[i * C + c] = v[q];
        if (vote_ahead(v[q], c, best, arg)) {
          best = v[q];
          arg = c;
        }
      }
    }
#pragma unroll
    for (int off = VOTE_GROUP / 2; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, VOTE_GROUP);
      const int oa = __shfl_xor(arg, off, VOTE_GROUP);
      if (vote_ahead(ob, oa, best, arg)) {
        best = ob;
        arg = oa;
      }
    }
    if (live && l == 0) {
      if (pred) pred[i] = ok ? (long long)arg : -1LL;
      if (!ok) {
        atomicAdd(&bad, 1);                               // a neighbour or an own row outside [0, M)
      } else if (counts) {
        const int64_t lab = labels[i];
        if (lab != ignore) {
          if (lab < 0 || lab >= C) atomicAdd(&bad, 1);
          else atomicAdd(&hist[(int)lab * C + arg], 1);
        }
      }
    }
  }
  __syncthreads();
  if (counts)
    for (int q = threadIdx.x; q < C * C; q += VOTE_THREADS)
      if (hist[q]) atomicAdd((unsigned long long*)&counts[q], (unsigned long long)hist[q]);
  if (threadIdx.x == 0 && bad && n_bad) atomicAdd((unsigned long long*)n_bad, (unsigned long long)bad);
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_vote_workspace_bytes(int64_t N) {
  if (N < 0) return DVA_ERR_INVALID;
  if (N > 0x7fffffffLL) return DVA_ERR_UNSUPPORTED;
  const int64_t bytes = (int64_t)align_up((size_t)N * 4);
  return bytes < 256 ? 256 : bytes;
}

int dva_vote_add(float* votes, int32_t* counts, int64_t N, int32_t C, const int64_t* ids, const void* outputs,
                 int32_t dtype, int64_t P, int32_t* slots, int64_t slots_bytes, int64_t* n_bad, void* stream) {
  if (N < 0 || P < 0 || C < 1) return DVA_ERR_INVALID;
  if (!dtype_ok(dtype)) return DVA_ERR_INVALID;
  if (C > VOTE_MAX_C || N > 0x7fffffffLL || P > 0x7fffffffLL) return DVA_ERR_UNSUPPORTED;   // a row position is int32
  if (!slots || !n_bad || slots_bytes < dva_vote_workspace_bytes(N)) return DVA_ERR_INVALID;
  if (N > 0 && (!votes || !counts)) return DVA_ERR_INVALID;
  if (P == 0) return DVA_OK;
  if (!ids || !outputs) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int rows_grid = capped_grid(P, VOTE_THREADS, 1 << 16);
  const int elts_grid = capped_grid(P * C, VOTE_THREADS, 1 << 16);
  hipLaunchKernelGGL(vote_claim_kernel, dim3(rows_grid), dim3(VOTE_THREADS), 0, s, ids, P, N, slots,
                     (long long*)n_bad);
  const bool known = with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL(vote_apply_kernel<T>, dim3(elts_grid), dim3(VOTE_THREADS), 0, s, ids, (const T*)outputs, P, (int)C,
                       N, slots, votes, counts);
  });
  if (!known) return DVA_ERR_INVALID;
  hipLaunchKernelGGL(vote_release_kernel, dim3(rows_grid), dim3(VOTE_THREADS), 0, s, ids, P, N, slots);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_knn_interpolate(const float* x, int64_t M, int32_t C, const int32_t* neighbors, const float* dist2, int64_t n,
                        int32_t k, const int32_t* own, float* y, int64_t* pred, const int64_t* labels,
                        int64_t ignore_index, int64_t* counts, int64_t* n_bad, void* stream) {
  if (M < 0 || n < 0 || C < 1 || k < 1) return DVA_ERR_INVALID;
  if (C > VOTE_MAX_C || k > VOTE_MAX_K) return DVA_ERR_UNSUPPORTED;
  if (M > 0x7fffffffLL || n > 0x7fffffffLL / k) return DVA_ERR_UNSUPPORTED;       // int32 neighbours; n k < 2^31
  if (!y && !pred && !counts) return DVA_ERR_INVALID;                            // nothing to write
  if (counts && !n_bad) return DVA_ERR_INVALID;
  if (n == 0) return DVA_OK;
  if ((int64_t)k > M) return DVA_ERR_INVALID;
  if (!x || !neighbors || !dist2) return DVA_ERR_INVALID;
  if (counts && !labels) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_interpolate_kernel, dim3(capped_grid(n, VOTE_ROWS, 2048)), dim3(VOTE_THREADS), 0, s, x, M,
                     (int)C, neighbors, dist2, n, (int)k, own, y, (long long*)pred, labels, ignore_index,
                     (long long*)counts, (long long*)n_bad);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
