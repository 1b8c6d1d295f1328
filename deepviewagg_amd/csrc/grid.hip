// Voxel-grid subsampling: the device side of GridSampling3D (reference:
// core/data_transform/grid_transform.py:24-191 over torch_cluster grid_cluster / torch_geometric voxel_grid +
// consecutive_cluster / torch_scatter scatter_add + scatter_mean, all on the CPU).
//
// Four steps, each a C-ABI entry (include/dva.h):
//   quantise  coords = rint(pos / size) in the dtype of pos (correctly rounded division, no reciprocal), int32 [n, 3],
//             plus the per-axis min / max (and of the batch column) and a flag word, reduced through per-block
//             partials into 9 int64 words: the caller reads them once to size the sort (the key's bit count).
//   cluster   mixed-radix key (batch, z, y, x) (x fastest: grid_cluster's key; batch slowest: voxel_grid's extra
//             column), stable rocPRIM radix sort of (key, point) over end_bit bits, run heads -> inclusive scan ->
//             voxel ids in ascending key order (consecutive_cluster's sorted unique), offsets [M + 1], cluster [n],
//             and the representative of every voxel: the member of largest rank (largest point index without ranks),
//             which is the winner of consecutive_cluster's CPU scatter_ (last write).
//   mean      rows permuted once into sorted order (one gather, coalesced writes), then one lane per (voxel, channel)
//             sums its contiguous segment sequentially in ascending point index, in the dtype of the rows, and divides
//             by the count in that dtype: torch_scatter's CPU scatter_mean, bit for bit.  No atomics, no split of a
//             chain (a split would change the fp32 sum), so a voxel of many points is one long chain; its loads are
//             issued 16 ahead of the adds.
//   majority  second radix sort of (voxel id, label - min) keys, run-length encode, and per voxel the run of largest
//             count, ties to the smallest label (one_hot + scatter_add + argmax of group_data).
// Per-voxel maxima (representative, majority) go through a wave-segmented max (ids are sorted, so a voxel occupies
// consecutive lanes) and one 64-bit atomicMax per voxel piece per wave: max is order independent, so the result is
// deterministic.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "dva_common.h"

namespace dva {

constexpr int GRID_TPB = 256;
constexpr int GRID_QBLOCKS = 1024;          // quantise partials: at most this many blocks
constexpr int GRID_STATS = 9;               // min x y z b, max x y z b, flags
constexpr int64_t GRID_MAX_N = 0x7fffffffLL; // point indices ride in 32 bits of the packed maxima
constexpr int GRID_UNROLL = 16;

// ---------------------------------------------------------------------------------------------------------------
// quantise
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gquot(float p, float s) { return p / s; }     // IEEE division (no fast-math)
__device__ __forceinline__ double gquot(double p, double s) { return p / s; }

template <typename T>
__global__ __launch_bounds__(GRID_TPB) void grid_quantize_kernel(const T* __restrict__ pos, int64_t n, T size,
                                                                 const int64_t* __restrict__ batch,
                                                                 int32_t* __restrict__ coords,
                                                                 int64_t* __restrict__ partials) {
  __shared__ int64_t sh[GRID_STATS][GRID_TPB];
  int64_t v[GRID_STATS];
  for (int d = 0; d < 4; ++d) {
    v[d] = INT64_MAX;
    v[4 + d] = INT64_MIN;
  }
  v[8] = 0;
  for (int64_t i = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GRID_TPB) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const T p = pos[3 * i + d];
      const T q = gquot(p, size);
      int32_t c = 0;
      if (!isfinite(p))
        v[8] |= 1;
      else if (!(fabs(q) < (T)16777216))   // 2^24: beyond it the reference's float grid arithmetic is inexact
        v[8] |= 2;
      else
        c = (int32_t)rint(q);              // half to even
      coords[3 * i + d] = c;
      v[d] = min(v[d], (int64_t)c);
      v[4 + d] = max(v[4 + d], (int64_t)c);
    }
    const int64_t b = batch ? batch[i] : 0;
    v[3] = min(v[3], b);
    v[7] = max(v[7], b);
  }
  for (int k = 0; k < GRID_STATS; ++k) sh[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = GRID_TPB / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = min(sh[k][threadIdx.x], sh[k][threadIdx.x + w]);
      for (int k = 4; k < 8; ++k) sh[k][threadIdx.x] = max(sh[k][threadIdx.x], sh[k][threadIdx.x + w]);
      sh[8][threadIdx.x] |= sh[8][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < GRID_STATS) partials[blockIdx.x * GRID_STATS + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void grid_stats_reduce_kernel(const int64_t* __restrict__ partials, int nb,
                                                               int64_t* __restrict__ stats) {
  const int k = threadIdx.x;
  if (k >= GRID_STATS) return;
  int64_t r = partials[k];
  for (int b = 1; b < nb; ++b) {
    const int64_t x = partials[b * GRID_STATS + k];
    r = k < 4 ? min(r, x) : (k < 8 ? max(r, x) : (r | x));
  }
  stats[k] = r;
}

// ---------------------------------------------------------------------------------------------------------------
// cluster
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRID_TPB) void grid_key_kernel(const int32_t* __restrict__ coords,
                                                            const int64_t* __restrict__ batch, int64_t n,
                                                            const int64_t* __restrict__ stats,
                                                            uint64_t* __restrict__ keys) {
  const int64_t lx = stats[0], ly = stats[1], lz = stats[2], lb = stats[3];
  const uint64_t ex = (uint64_t)(stats[4] - lx + 1), ey = (uint64_t)(stats[5] - ly + 1),
                 ez = (uint64_t)(stats[6] - lz + 1);
  for (int64_t i = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GRID_TPB) {
    const uint64_t b = (uint64_t)((batch ? batch[i] : 0) - lb);
    const uint64_t x = (uint64_t)(coords[3 * i] - lx), y = (uint64_t)(coords[3 * i + 1] - ly),
                   z = (uint64_t)(coords[3 * i + 2] - lz);
    keys[i] = ((b * ez + z) * ey + y) * ex + x;
  }
}

__global__ __launch_bounds__(GRID_TPB) void grid_head_kernel(const uint64_t* __restrict__ sorted, int64_t n,
                                                             int64_t* __restrict__ head) {
  for (int64_t i = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GRID_TPB)
    head[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

// Max of `val` over the lanes of the wave that share `seg` (seg non-decreasing along the lanes; inactive lanes carry
// a seg of their own), then one atomicMax per (segment, wave) from the segment's first lane in the wave.
__device__ __forceinline__ void seg_atomic_max(uint64_t* __restrict__ dst, int64_t seg, uint64_t val, bool active) {
  const int lane = threadIdx.x & (DVA_WAVE - 1);
#pragma unroll
  for (int off = 1; off < DVA_WAVE; off <<= 1) {
    const uint64_t ov = __shfl_down(val, off, DVA_WAVE);
    const int64_t os = __shfl_down(seg, off, DVA_WAVE);
    if (lane + off < DVA_WAVE && os == seg && ov > val) val = ov;
  }
  const int64_t ps = __shfl_up(seg, 1, DVA_WAVE);
  if (active && (lane == 0 || ps != seg)) atomicMax((unsigned long long*)&dst[seg], (unsigned long long)val);
}

// per sorted position i: voxel id, cluster of the point, offsets of run heads, representative candidates
__global__ __launch_bounds__(GRID_TPB) void grid_finish_kernel(const int64_t* __restrict__ vid1,
                                                               const int64_t* __restrict__ order,
                                                               const int64_t* __restrict__ rank, int64_t n,
                                                               int64_t* __restrict__ cluster,
                                                               int64_t* __restrict__ offsets,
                                                               int64_t* __restrict__ n_voxels,
                                                               uint64_t* __restrict__ best) {
  for (int64_t base = blockIdx.x * (int64_t)GRID_TPB; base < n; base += (int64_t)gridDim.x * GRID_TPB) {
    const int64_t i = base + threadIdx.x;
    const bool ok = i < n;
    int64_t v = -1 - (int64_t)threadIdx.x;   // inactive lanes: distinct segments
    uint64_t packed = 0;
    if (ok) {
      v = vid1[i] - 1;
      const int64_t p = order[i];
      cluster[p] = v;
      if (i == 0 || vid1[i - 1] != vid1[i]) offsets[v] = i;
      if (i == n - 1) {
        offsets[v + 1] = n;
        *n_voxels = v + 1;
      }
      const int64_t r = rank ? rank[p] : p;
      packed = ((uint64_t)r << 32) | (uint64_t)p;
    }
    seg_atomic_max(best, v, packed, ok);
  }
}

__global__ __launch_bounds__(GRID_TPB) void grid_rep_kernel(const uint64_t* __restrict__ best,
                                                            const int64_t* __restrict__ n_voxels,
                                                            const int32_t* __restrict__ coords, int64_t n,
                                                            int64_t* __restrict__ rep, int32_t* __restrict__ vcoords) {
  const int64_t m = *n_voxels;
  for (int64_t v = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; v < m && v < n; v += (int64_t)gridDim.x * GRID_TPB) {
    const int64_t p = (int64_t)(best[v] & 0xffffffffull);
    rep[v] = p;
    if (vcoords) {
      vcoords[3 * v] = coords[3 * p];
      vcoords[3 * v + 1] = coords[3 * p + 1];
      vcoords[3 * v + 2] = coords[3 * p + 2];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// segmented mean
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
struct MeanOp {   // floating: IEEE add, count in T as torch_scatter's sum of ones (fp32 saturates at 2^24)
  static __device__ __forceinline__ T add(T a, T b) { return a + b; }
  static __device__ __forceinline__ T div(T s, int64_t cnt) {
    if (sizeof(T) == 4 && cnt > (1 << 24)) cnt = 1 << 24;
    return s / (T)cnt;
  }
};
template <>
struct MeanOp<int32_t> {   // wrapping sum, quotient rounded toward zero
  static __device__ __forceinline__ int32_t add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
  static __device__ __forceinline__ int32_t div(int32_t s, int64_t cnt) { return (int32_t)((int64_t)s / cnt); }
};
template <>
struct MeanOp<int64_t> {
  static __device__ __forceinline__ int64_t add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
  static __device__ __forceinline__ int64_t div(int64_t s, int64_t cnt) { return s / cnt; }
};

template <typename T>
__global__ __launch_bounds__(GRID_TPB) void grid_permute_kernel(const T* __restrict__ src,
                                                                const int64_t* __restrict__ order, int64_t n, int C,
                                                                T* __restrict__ dst) {
  const int64_t total = n * (int64_t)C;
  for (int64_t e = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; e < total; e += (int64_t)gridDim.x * GRID_TPB) {
    const int64_t i = e / C;
    dst[e] = src[order[i] * C + (e - i * C)];
  }
}

template <typename T>
__global__ __launch_bounds__(GRID_TPB) void grid_mean_kernel(const T* __restrict__ sorted,
                                                             const int64_t* __restrict__ offsets, int64_t m, int C,
                                                             T* __restrict__ out) {
  const int64_t total = m * (int64_t)C;
  for (int64_t t = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; t < total; t += (int64_t)gridDim.x * GRID_TPB) {
    const int64_t v = t / C;
    const int c = (int)(t - v * C);
    const int64_t b = offsets[v], e = offsets[v + 1];
    const T* col = sorted + c;
    T acc = 0;
    int64_t j = b;
    for (; j + GRID_UNROLL <= e; j += GRID_UNROLL) {
      T x[GRID_UNROLL];
#pragma unroll
      for (int u = 0; u < GRID_UNROLL; ++u) x[u] = col[(j + u) * C];
#pragma unroll
      for (int u = 0; u < GRID_UNROLL; ++u) acc = MeanOp<T>::add(acc, x[u]);
    }
    for (; j < e; ++j) acc = MeanOp<T>::add(acc, col[j * C]);
    out[t] = MeanOp<T>::div(acc, e - b);
  }
}

template <typename T>
static int launch_mean(const void* src, int64_t n, int C, const int64_t* order, const int64_t* offsets, int64_t m,
                       void* out, void* ws, hipStream_t s) {
  hipLaunchKernelGGL(grid_permute_kernel<T>, dim3(capped_grid(n * (int64_t)C, GRID_TPB, 8192)), dim3(GRID_TPB), 0, s,
                     (const T*)src, order, n, C, (T*)ws);
  hipLaunchKernelGGL(grid_mean_kernel<T>, dim3(capped_grid(m * (int64_t)C, GRID_TPB, 8192)), dim3(GRID_TPB), 0, s,
                     (const T*)ws, offsets, m, C, (T*)out);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// majority label
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRID_TPB) void grid_label_key_kernel(const int64_t* __restrict__ labels,
                                                                  const int64_t* __restrict__ cluster, int64_t n,
                                                                  int64_t lmin, int64_t nl,
                                                                  uint64_t* __restrict__ keys) {
  for (int64_t i = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GRID_TPB)
    keys[i] = (uint64_t)cluster[i] * (uint64_t)nl + (uint64_t)(labels[i] - lmin);
}

// one run = one (voxel, label): pack (count, ~label) so that the max is the largest count, then the smallest label
__global__ __launch_bounds__(GRID_TPB) void grid_runs_kernel(const uint64_t* __restrict__ uniq,
                                                             const uint32_t* __restrict__ counts,
                                                             const uint32_t* __restrict__ n_runs, int64_t n,
                                                             int64_t nl, int64_t m, uint64_t* __restrict__ best) {
  const int64_t r_end = (int64_t)*n_runs;
  for (int64_t base = blockIdx.x * (int64_t)GRID_TPB; base < n; base += (int64_t)gridDim.x * GRID_TPB) {
    const int64_t r = base + threadIdx.x;
    bool ok = r < r_end;
    int64_t v = -1 - (int64_t)threadIdx.x;
    uint64_t packed = 0;
    if (ok) {
      const uint64_t k = uniq[r];
      const uint64_t q = k / (uint64_t)nl;
      ok = q < (uint64_t)m;             // a cluster id outside [0, n_voxels) writes nothing
      if (ok) {
        v = (int64_t)q;
        packed = ((uint64_t)counts[r] << 32) | (0xffffffffull - (k - q * (uint64_t)nl));
      }
    }
    seg_atomic_max(best, v, packed, ok);
  }
}

__global__ __launch_bounds__(GRID_TPB) void grid_majority_out_kernel(const uint64_t* __restrict__ best, int64_t m,
                                                                     int64_t lmin, int64_t* __restrict__ out) {
  for (int64_t v = blockIdx.x * (int64_t)GRID_TPB + threadIdx.x; v < m; v += (int64_t)gridDim.x * GRID_TPB)
    out[v] = lmin + (int64_t)(0xffffffffull - (best[v] & 0xffffffffull));
}

// ---------------------------------------------------------------------------------------------------------------
// workspace layouts
// ---------------------------------------------------------------------------------------------------------------
struct GridLayout {
  uint64_t *a, *b, *c;
  uint32_t* d;
  int64_t* runs;
  char* temp;
  size_t temp_bytes, total;
};

static int grid_layout(void* ws, int64_t n, GridLayout* L) {
  size_t sort_tmp = 0, keys_tmp = 0, scan_tmp = 0, rle_tmp = 0;
  uint64_t* k = nullptr;
  int64_t* v = nullptr;
  uint32_t* c = nullptr;
  rocprim::counting_iterator<int64_t> it(0);
  if (rocprim::radix_sort_pairs(nullptr, sort_tmp, k, k, it, v, (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
    return DVA_ERR_LAUNCH;
  if (rocprim::radix_sort_keys(nullptr, keys_tmp, k, k, (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
    return DVA_ERR_LAUNCH;
  if (rocprim::inclusive_scan(nullptr, scan_tmp, v, v, (size_t)n, rocprim::plus<int64_t>(), (hipStream_t)0) !=
      hipSuccess)
    return DVA_ERR_LAUNCH;
  if (rocprim::run_length_encode(nullptr, rle_tmp, k, (unsigned int)n, k, c, c, (hipStream_t)0) != hipSuccess)
    return DVA_ERR_LAUNCH;
  size_t t = sort_tmp;
  if (keys_tmp > t) t = keys_tmp;
  if (scan_tmp > t) t = scan_tmp;
  if (rle_tmp > t) t = rle_tmp;
  Carver w(ws);
  L->a = w.take<uint64_t>((size_t)n);                      // keys in / head flags / representative maxima / uniq
  L->b = w.take<uint64_t>((size_t)n);                      // sorted keys
  L->c = w.take<uint64_t>((size_t)n);                      // voxel ids (+1) / majority maxima
  L->d = w.take<uint32_t>((size_t)n);                      // run counts
  L->runs = w.take<int64_t>(GRID_QBLOCKS * GRID_STATS);    // run count / quantise partials
  L->temp_bytes = t;
  L->temp = w.take<char>(t);
  L->total = w.used();
  return DVA_OK;
}

static int grid_check(int64_t n, void* ws, int64_t wsb, GridLayout* L) {
  if (!ws) return DVA_ERR_INVALID;
  const int rc = grid_layout(ws, n, L);
  if (rc) return rc;
  return (int64_t)L->total > wsb ? DVA_ERR_INVALID : DVA_OK;
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_grid_workspace_bytes(int64_t n, int64_t row_bytes) {
  if (n < 0 || row_bytes < 0) return DVA_ERR_INVALID;
  if (n > GRID_MAX_N) return DVA_ERR_UNSUPPORTED;
  if (row_bytes > 0) return (int64_t)align_up((size_t)n * (size_t)row_bytes);
  if (n == 0) return 256;
  GridLayout L;
  const int rc = grid_layout(nullptr, n, &L);
  return rc ? rc : (int64_t)L.total;
}

int dva_grid_quantize(const void* pos, int32_t dtype, int64_t n, double size, const int64_t* batch, int32_t* coords,
                      int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n <= 0 || !pos || !coords || !stats || !workspace) return DVA_ERR_INVALID;
  if (!(size > 0.0) || (dtype != DVA_GRID_F32 && dtype != DVA_GRID_F64)) return DVA_ERR_INVALID;
  if (n > GRID_MAX_N) return DVA_ERR_UNSUPPORTED;
  GridLayout L;
  const int rc = grid_check(n, workspace, workspace_bytes, &L);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  int64_t* partials = L.runs;
  int nb = (int)((n + GRID_TPB - 1) / GRID_TPB);
  if (nb > GRID_QBLOCKS) nb = GRID_QBLOCKS;
  if (dtype == DVA_GRID_F32)
    hipLaunchKernelGGL(grid_quantize_kernel<float>, dim3(nb), dim3(GRID_TPB), 0, s, (const float*)pos, n,
                       (float)size, batch, coords, partials);
  else
    hipLaunchKernelGGL(grid_quantize_kernel<double>, dim3(nb), dim3(GRID_TPB), 0, s, (const double*)pos, n, size,
                       batch, coords, partials);
  hipLaunchKernelGGL(grid_stats_reduce_kernel, dim3(1), dim3(64), 0, s, partials, nb, stats);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_grid_cluster(const int32_t* coords, const int64_t* batch, const int64_t* rank, int64_t n,
                     const int64_t* stats, int32_t end_bit, int64_t* order, int64_t* cluster, int64_t* offsets,
                     int64_t* rep, int32_t* voxel_coords, int64_t* n_voxels, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  if (n <= 0 || !coords || !stats || !order || !cluster || !offsets || !rep || !n_voxels) return DVA_ERR_INVALID;
  if (end_bit < 1 || end_bit > 63) return DVA_ERR_INVALID;
  if (n > GRID_MAX_N) return DVA_ERR_UNSUPPORTED;
  GridLayout L;
  const int rc = grid_check(n, workspace, workspace_bytes, &L);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint64_t* keys = L.a;
  uint64_t* sorted = L.b;
  int64_t* vid1 = (int64_t*)L.c;
  const int g = capped_grid(n, GRID_TPB, 8192);
  hipLaunchKernelGGL(grid_key_kernel, dim3(g), dim3(GRID_TPB), 0, s, coords, batch, n, stats, keys);
  size_t tmp = L.temp_bytes;
  rocprim::counting_iterator<int64_t> iota(0);
  if (rocprim::radix_sort_pairs(L.temp, tmp, keys, sorted, iota, order, (size_t)n, 0, (unsigned)end_bit, s) !=
      hipSuccess)
    return DVA_ERR_LAUNCH;
  int64_t* head = (int64_t*)keys;   // the unsorted keys are consumed
  hipLaunchKernelGGL(grid_head_kernel, dim3(g), dim3(GRID_TPB), 0, s, sorted, n, head);
  tmp = L.temp_bytes;
  if (rocprim::inclusive_scan(L.temp, tmp, head, vid1, (size_t)n, rocprim::plus<int64_t>(), s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  uint64_t* best = keys;            // the head flags are consumed
  if (hipMemsetAsync(best, 0, (size_t)n * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(grid_finish_kernel, dim3(g), dim3(GRID_TPB), 0, s, vid1, order, rank, n, cluster, offsets,
                     n_voxels, best);
  hipLaunchKernelGGL(grid_rep_kernel, dim3(g), dim3(GRID_TPB), 0, s, best, n_voxels, coords, n, rep, voxel_coords);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_grid_mean(const void* src, int32_t dtype, int64_t n, int32_t C, const int64_t* order, const int64_t* offsets,
                  int64_t n_voxels, void* out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n <= 0 || C <= 0 || n_voxels <= 0 || n_voxels > n || !src || !order || !offsets || !out || !workspace)
    return DVA_ERR_INVALID;
  if (n > GRID_MAX_N) return DVA_ERR_UNSUPPORTED;
  size_t esz;
  switch (dtype) {
    case DVA_GRID_F32: case DVA_GRID_I32: esz = 4; break;
    case DVA_GRID_F64: case DVA_GRID_I64: esz = 8; break;
    default: return DVA_ERR_INVALID;
  }
  if ((int64_t)align_up((size_t)n * C * esz) > workspace_bytes) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case DVA_GRID_F32: return launch_mean<float>(src, n, C, order, offsets, n_voxels, out, workspace, s);
    case DVA_GRID_F64: return launch_mean<double>(src, n, C, order, offsets, n_voxels, out, workspace, s);
    case DVA_GRID_I32: return launch_mean<int32_t>(src, n, C, order, offsets, n_voxels, out, workspace, s);
    default: return launch_mean<int64_t>(src, n, C, order, offsets, n_voxels, out, workspace, s);
  }
}

int dva_grid_majority(const int64_t* labels, int64_t n, const int64_t* cluster, int64_t n_voxels, int64_t label_min,
                      int64_t n_labels, int32_t end_bit, int64_t* out, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  if (n <= 0 || n_voxels <= 0 || n_voxels > n || n_labels <= 0 || !labels || !cluster || !out) return DVA_ERR_INVALID;
  if (n_labels > 0xffffffffLL || end_bit < 1 || end_bit > 63) return DVA_ERR_INVALID;
  if (n > GRID_MAX_N) return DVA_ERR_UNSUPPORTED;
  GridLayout L;
  const int rc = grid_check(n, workspace, workspace_bytes, &L);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint64_t* keys = L.a;
  uint64_t* sorted = L.b;
  uint64_t* best = L.c;
  uint32_t* counts = L.d;
  uint32_t* n_runs = (uint32_t*)L.runs;
  const int g = capped_grid(n, GRID_TPB, 8192);
  hipLaunchKernelGGL(grid_label_key_kernel, dim3(g), dim3(GRID_TPB), 0, s, labels, cluster, n, label_min, n_labels,
                     keys);
  size_t tmp = L.temp_bytes;
  if (rocprim::radix_sort_keys(L.temp, tmp, keys, sorted, (size_t)n, 0, (unsigned)end_bit, s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  uint64_t* uniq = keys;            // the unsorted keys are consumed
  tmp = L.temp_bytes;
  if (rocprim::run_length_encode(L.temp, tmp, sorted, (unsigned int)n, uniq, counts, n_runs, s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  if (hipMemsetAsync(best, 0, (size_t)n_voxels * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(grid_runs_kernel, dim3(g), dim3(GRID_TPB), 0, s, uniq, counts, n_runs, n, n_labels, n_voxels,
                     best);
  hipLaunchKernelGGL(grid_majority_out_kernel, dim3(capped_grid(n_voxels, GRID_TPB, 8192)), dim3(GRID_TPB), 0, s, best,
                     n_voxels, label_min, out);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
