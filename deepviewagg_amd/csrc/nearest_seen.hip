// Nearest-seen fill: the eval-mode tail of the image-only models (reference:
// models/segmentation/multimodal/no3d.py:105-125, a KeOps LazyTensor argmin of the unseen points against the seen ones).
//
// One cloud, one mask.  Every point gets a 64-bit key: its grid cell (knn_grid.h) in the low 63 bits, the UNSEEN flag in
// bit 63.  One radix sort over all 64 bits then leaves the seen points first, in cell order, and the unseen points
// behind them, in cell order too: the cell table is built from the first part alone and the second part is the list
// of queries, walked by wavefronts whose lanes share a few cells.  Nothing is compacted and the number of seen points
// is never needed: a thread that finds a key without the flag has a seen point and is done.
//
// The search is the shell walk of knn.hip for one neighbour, with its bound (after shell R every unvisited point is
// farther than R * cell - slack) and its level scheme: a call walks at most max_shell shells and leaves the queries
// that are not provably final to a later call with a coarser cell; the `last` call walks every shell that the box
// holds, so it finishes every query for ANY cell.  The last call also writes src of the seen points, any_seen, and,
// when x is given, the rows filled[i] = x[src[i]] (copied as bits) -- in the same launch as the search.
#include <rocprim/device/device_radix_sort.hpp>

#include "dva_common.h"
#include "knn_grid.h"

namespace dva {

constexpr int NS_TPB = 64;
constexpr uint64_t NS_UNSEEN = 1ULL << 63;

// The cell the grid is built with: `cell`, but never so small that an axis would hold 2^19 cells or more.  The last
// call walks every shell the box holds, so its cell is at least 1/16 of the extent: however small the caller's cell, a
// query that the finer grids left open walks 18 shells at the most (through fuller cells).
__device__ __forceinline__ float ns_cell(const float* __restrict__ bbox, float cell, int last) {
  const float ext = fmaxf(fmaxf(bbox[3] - bbox[0], bbox[4] - bbox[1]), bbox[5] - bbox[2]);
  return fmaxf(fmaxf(cell, ext * (last ? 1.f / 16.f : 1.f / 524288.f)), 1e-12f);
}

__global__ __launch_bounds__(256) void ns_keys_kernel(const float* __restrict__ pos, const uint8_t* __restrict__ seen,
                                                       int64_t n, const float* __restrict__ bbox, float cell, int last,
                                                       uint64_t* __restrict__ keys, int32_t* __restrict__ ids) {
  const float inv_cell = 1.f / ns_cell(bbox, cell, last);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = cell_key(cell_of(pos[3 * i], bbox[0], inv_cell), cell_of(pos[3 * i + 1], bbox[1], inv_cell),
                                cell_of(pos[3 * i + 2], bbox[2], inv_cell)) & ~NS_UNSEEN;
    keys[i] = seen[i] ? k : (k | NS_UNSEEN);
    ids[i] = (int32_t)i;
  }
}

// sorted copy of the points (x, y, z, original index) + cell table of the seen part: key -> first sorted position
__global__ __launch_bounds__(256) void ns_cells_kernel(const float* __restrict__ pos,
                                                        const uint64_t* __restrict__ keys_sorted,
                                                        const int32_t* __restrict__ perm, int64_t n,
                                                        float4* __restrict__ pts, uint64_t* __restrict__ tkeys,
                                                        int32_t* __restrict__ tvals, uint32_t mask) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t o = perm[i];
    pts[i] = make_float4(pos[3 * (int64_t)o], pos[3 * (int64_t)o + 1], pos[3 * (int64_t)o + 2], __int_as_float(o));
    const uint64_t k = keys_sorted[i];
    if (!(k & NS_UNSEEN) && (i == 0 || keys_sorted[i - 1] != k)) {
      uint32_t h = hash64(k) & mask;
      for (;;) {
        const unsigned long long old = atomicCAS((unsigned long long*)&tkeys[h], ~0ULL, (unsigned long long)k);
        if (old == ~0ULL || old == k) {
          tvals[h] = (int32_t)i;
          break;
        }
        h = (h + 1) & mask;
      }
    }
  }
}

// One thread per sorted position.  E = the storage word of a row element (uint16_t / uint32_t): rows are copied as bits.
template <typename E>
__global__ __launch_bounds__(NS_TPB) void ns_query_kernel(
    const float4* __restrict__ pts, const uint64_t* __restrict__ keys_sorted, int64_t n,
    const float* __restrict__ bbox, float cell_arg, const uint64_t* __restrict__ tkeys,
    const int32_t* __restrict__ tvals, uint32_t mask, int max_shell, int last, uint8_t* __restrict__ done,
    int32_t* __restrict__ src, uint8_t* __restrict__ any_seen, const E* __restrict__ x, int K, E* __restrict__ filled) {
  __shared__ int32_t s_from[NS_TPB], s_to[NS_TPB];
  const int t = threadIdx.x;
  const float cell = ns_cell(bbox, cell_arg, last);
  const float inv_cell = 1.f / cell;
  const float ext = fmaxf(fmaxf(bbox[3] - bbox[0], bbox[4] - bbox[1]), bbox[5] - bbox[2]);
  const float slack = 1e-5f * (ext + cell);
  const int r_all = (int)(ext * inv_cell) + 2;          // shells that cover the whole cloud
  const int r_max = (last || max_shell > r_all) ? r_all : max_shell;
  const bool none_seen = (keys_sorted[0] & NS_UNSEEN) != 0;      // the seen points sort first
  if (last && blockIdx.x == 0 && t == 0) any_seen[0] = none_seen ? 0 : 1;
  for (int64_t base = blockIdx.x * (int64_t)NS_TPB; base < n; base += (int64_t)gridDim.x * NS_TPB) {
    const int64_t s0 = base + t;
    int o = -1, from = -1;
    if (s0 < n) {
      const float4 q = pts[s0];
      o = __float_as_int(q.w);
      if (!(keys_sorted[s0] & NS_UNSEEN)) {
        from = o;                                        // a seen point keeps its own row
        if (last) src[o] = o;
      } else if (done[o]) {
        from = src[o];                                   // finished on a finer grid
      } else if (none_seen) {
        from = o;                                        // nothing to search: the point keeps its own row
        src[o] = o;
        done[o] = 1;
      } else {
        const int cx = cell_of(q.x, bbox[0], inv_cell), cy = cell_of(q.y, bbox[1], inv_cell),
                  cz = cell_of(q.z, bbox[2], inv_cell);
        float bd = INFINITY;
        int bi = -1;
        bool finished = false;
        for (int R = 0; R <= r_max; ++R) {
          for (int dx = -R; dx <= R; ++dx)
            for (int dy = -R; dy <= R; ++dy) {
              const bool face = (dx == -R || dx == R || dy == -R || dy == R);
              const int step = face ? 1 : 2 * R;          // interior columns: only the two end caps
              for (int dz = -R; dz <= R; dz += (step > 0 ? step : 1)) {
                const uint64_t key = cell_key(cx + dx, cy + dy, cz + dz) & ~NS_UNSEEN;
                int s = cell_start(tkeys, tvals, mask, key);
                if (s < 0) continue;
                for (; s < n && keys_sorted[s] == key; ++s) {
                  const float4 p = pts[s];
                  const float d = dist2_f32(q.x, q.y, q.z, p.x, p.y, p.z);
                  const int j = __float_as_int(p.w);
                  if (d < bd || (d == bd && (bi < 0 || j < bi))) { bd = d; bi = j; }
                }
                if (R == 0) break;
              }
            }
          if (bi >= 0) {
            const float bound = (float)R * cell - slack;
            if (bound > 0.f && bd < bound * bound) { finished = true; break; }
          }
        }
        // not provably final within max_shell shells: left to a coarser grid, unless the shells covered the cloud
        if (finished || r_max >= r_all) {
          from = bi >= 0 ? bi : o;                       // no seen point at all: the point keeps its own row
          src[o] = from;
          done[o] = 1;
        }
      }
      if (from < 0 || from >= n) from = o;
    }
    if (x) {                                             // uniform over the block; only the last call passes rows
      __syncthreads();
      s_from[t] = from;
      s_to[t] = o;
      __syncthreads();
      const int64_t left = n - base;
      const int m = left < NS_TPB ? (int)left : NS_TPB;
      for (int e = t; e < m * K; e += NS_TPB) {
        const int p = e / K, c = e - p * K;
        filled[(int64_t)s_to[p] * K + c] = x[(int64_t)s_from[p] * K + c];
      }
    }
  }
}

struct NsLayout {
  uint64_t *keys, *keys_sorted, *tkeys;
  int32_t *ids, *perm, *tvals;
  float4* pts;
  char* temp;
  size_t temp_bytes, total;
  uint64_t cap;
};

static int ns_layout(void* ws, int64_t n, NsLayout* L) {
  size_t tmp = 0;
  uint64_t* nk = nullptr;
  int32_t* nv = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, tmp, nk, nk, nv, nv, (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
    return DVA_ERR_LAUNCH;
  uint64_t cap = 64;
  while (cap < 2 * (uint64_t)n) cap <<= 1;
  L->cap = cap;
  Carver c(ws);
  L->keys = c.take<uint64_t>((size_t)n);
  L->ids = c.take<int32_t>((size_t)n);
  L->keys_sorted = c.take<uint64_t>((size_t)n);
  L->perm = c.take<int32_t>((size_t)n);
  L->pts = c.take<float4>((size_t)n);
  L->tkeys = c.take<uint64_t>(cap);
  L->tvals = c.take<int32_t>(cap);
  L->temp_bytes = tmp;
  L->temp = c.take<char>(tmp);
  L->total = c.used();
  return DVA_OK;
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_nearest_seen_workspace_bytes(int64_t n) {
  if (n < 0) return DVA_ERR_INVALID;
  if (n > 0x3fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return 256;
  NsLayout L;
  int rc = ns_layout(nullptr, n, &L);
  if (rc) return rc;
  return (int64_t)L.total;
}

int dva_nearest_seen(const float* pos, const uint8_t* seen, int64_t n, const float* bbox, float cell,
                     int32_t max_shell, int32_t last, uint8_t* done, int32_t* src, uint8_t* any_seen, const void* x,
                     int32_t K, int32_t dtype, void* filled, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || !(cell > 0.f) || max_shell < 1) return DVA_ERR_INVALID;
  if ((x != nullptr) != (filled != nullptr)) return DVA_ERR_INVALID;
  if (x) {
    if (!last || K < 1 || x == filled) return DVA_ERR_INVALID;
    if (K > (1 << 20)) return DVA_ERR_UNSUPPORTED;
    if (!dtype_ok(dtype)) return DVA_ERR_INVALID;
  }
  if (n > 0x3fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return DVA_OK;
  if (!pos || !seen || !bbox || !done || !src || !workspace || (last && !any_seen)) return DVA_ERR_INVALID;
  NsLayout L;
  int rc = ns_layout(workspace, n, &L);
  if (rc) return rc;
  if ((int64_t)L.total > workspace_bytes) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ns_keys_kernel, dim3(capped_grid(n, 256, 8192)), dim3(256), 0, s, pos, seen, n, bbox, cell, last,
                     L.keys, L.ids);
  size_t tmp = L.temp_bytes;
  if (rocprim::radix_sort_pairs(L.temp, tmp, L.keys, L.keys_sorted, L.ids, L.perm, (size_t)n, 0, 64, s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  if (hipMemsetAsync(L.tkeys, 0xff, L.cap * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(ns_cells_kernel, dim3(capped_grid(n, 256, 8192)), dim3(256), 0, s, pos, L.keys_sorted, L.perm, n,
                     L.pts, L.tkeys, L.tvals, (uint32_t)(L.cap - 1));
  const dim3 grid(capped_grid(n, NS_TPB, GRID_CAP)), block(NS_TPB);
  const uint32_t mask = (uint32_t)(L.cap - 1);
  if (x && dtype == DVA_F32)
    hipLaunchKernelGGL(ns_query_kernel<uint32_t>, grid, block, 0, s, L.pts, L.keys_sorted, n, bbox, cell, L.tkeys,
                       L.tvals, mask, max_shell, last, done, src, any_seen, (const uint32_t*)x, K, (uint32_t*)filled);
  else
    hipLaunchKernelGGL(ns_query_kernel<uint16_t>, grid, block, 0, s, L.pts, L.keys_sorted, n, bbox, cell, L.tkeys,
                       L.tvals, mask, max_shell, last, done, src, any_seen, (const uint16_t*)x, K, (uint16_t*)filled);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
