// Exact k-nearest-neighbour search on a uniform hash grid + per-view occlusion counts: the device side of
// NeighborhoodBasedMappingFeatures (reference: core/data_transform/multimodal/image.py:431-612, which uses
// KeOps `argKmin` over all pairs, or FAISS).  Mapping features 7-8 of the `in_map: 8` configurations:
//   density   ~ (k+1) / (pi d_k^2) with d_k the distance to the k-th neighbour (the point itself included),
//   occlusion = (1 + #neighbours seen by the same image) / (k+1) for every (point, image) view.
//
// Contract (what `argKmin(k)` of the fp32 squared distances ((dx*dx + dy*dy) + dz*dz) returns when ties are
// broken by the lower index): neighbours sorted ascending by (d2, index); the query point itself is its own
// first neighbour.  Exactness: cells are visited in Chebyshev shells around the query's cell; after shell R
// every unvisited point is farther than R*cell - slack, so the search stops as soon as the current k-th
// distance is below that bound (slack absorbs the float rounding of the cell assignment).
// dva_knn_query (PCAComputePointwise, reference core/data_transform/features.py:360-485) runs the same search for
// the points of a separate query cloud, walked in the cell order of the search cloud's grid; the order is then
// (d2, search index) alone, with no self-first rule.  The argument holds for queries outside the search cloud's
// box as long as bbox covers both clouds.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "dva_common.h"
#include "knn_grid.h"

namespace dva {

constexpr int KNN_TPB = 64;      // one wavefront per block: the candidate lists live in LDS, [slot][thread]
constexpr int KNN_KMAX = 128;     // k <= 64: 32 KB of candidate lists per block; k <= 128 (BiasuttiVisibility, k = 75): 64 KB

// bbox = min xyz | max xyz (device memory, written by the caller's stream)
__global__ __launch_bounds__(256) void knn_keys_kernel(const float* __restrict__ xyz, int64_t n,
                                                        const float* __restrict__ bbox, float inv_cell,
                                                        uint64_t* __restrict__ keys, int32_t* __restrict__ ids) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    keys[i] = cell_key(cell_of(xyz[3 * i], bbox[0], inv_cell), cell_of(xyz[3 * i + 1], bbox[1], inv_cell),
                       cell_of(xyz[3 * i + 2], bbox[2], inv_cell));
    ids[i] = (int32_t)i;
  }
}

// sorted copy of the points (x, y, z, original index) + cell table: key -> first sorted position
__global__ __launch_bounds__(256) void knn_cells_kernel(const float* __restrict__ xyz,
                                                         const uint64_t* __restrict__ keys_sorted,
                                                         const int32_t* __restrict__ perm, int64_t n,
                                                         float4* __restrict__ pts, uint64_t* __restrict__ tkeys,
                                                         int32_t* __restrict__ tvals, uint32_t mask) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t o = perm[i];
    pts[i] = make_float4(xyz[3 * (int64_t)o], xyz[3 * (int64_t)o + 1], xyz[3 * (int64_t)o + 2], __int_as_float(o));
    const uint64_t k = keys_sorted[i];
    if (i == 0 || keys_sorted[i - 1] != k) {
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

// the query points of a separate query cloud, in the cell order of their keys: qpts[i] = (xyz, original index)
__global__ __launch_bounds__(256) void knn_query_points_kernel(const float* __restrict__ xyz,
                                                                const int32_t* __restrict__ perm, int64_t n,
                                                                float4* __restrict__ qpts) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t o = perm[i];
    qpts[i] = make_float4(xyz[3 * (int64_t)o], xyz[3 * (int64_t)o + 1], xyz[3 * (int64_t)o + 2], __int_as_float(o));
  }
}

// qpts [nq] = the queries (x, y, z, query index) in cell order; pts / keys_sorted [n] = the search cloud.  dva_knn
// passes its sorted cloud as both.
template <int KCAP>
__global__ __launch_bounds__(KNN_TPB) void knn_query_kernel(
    const float4* __restrict__ qpts, int64_t nq, const float4* __restrict__ pts,
    const uint64_t* __restrict__ keys_sorted, int64_t n, const float* __restrict__ bbox, float cell,
    const uint64_t* __restrict__ tkeys, const int32_t* __restrict__ tvals, uint32_t mask, int k, int max_shell,
    uint8_t* __restrict__ done, int32_t* __restrict__ nbr, float* __restrict__ d2_out) {
  __shared__ float s_d[KCAP][KNN_TPB];
  __shared__ int32_t s_i[KCAP][KNN_TPB];
  const int t = threadIdx.x;
  const float inv_cell = 1.f / cell;
  const float ext = fmaxf(fmaxf(bbox[3] - bbox[0], bbox[4] - bbox[1]), bbox[5] - bbox[2]);
  const float slack = 1e-5f * (ext + cell);
  const int r_all = (int)(ext * inv_cell) + 2;          // shells that cover the whole cloud
  const int r_max = max_shell < r_all ? max_shell : r_all;
  // queries in sorted (cell) order: the threads of a wavefront walk the same few cells
  for (int64_t qs = blockIdx.x * (int64_t)KNN_TPB + t; qs < nq; qs += (int64_t)gridDim.x * KNN_TPB) {
    const float4 q = qpts[qs];
    const int qi = __float_as_int(q.w);
    if (done && done[qi]) continue;      // finished on a finer grid
    const int cx = cell_of(q.x, bbox[0], inv_cell), cy = cell_of(q.y, bbox[1], inv_cell),
              cz = cell_of(q.z, bbox[2], inv_cell);
    int cnt = 0, wslot = 0;
    float wd = -1.f;
    int wi = -1;
    bool finished = false;
    for (int R = 0; R <= r_max; ++R) {
      for (int dx = -R; dx <= R; ++dx)
        for (int dy = -R; dy <= R; ++dy) {
          const bool face = (dx == -R || dx == R || dy == -R || dy == R);
          const int step = face ? 1 : 2 * R;          // interior columns: only the two end caps
          for (int dz = -R; dz <= R; dz += (step > 0 ? step : 1)) {
            const uint64_t key = cell_key(cx + dx, cy + dy, cz + dz);
            int s = cell_start(tkeys, tvals, mask, key);
            if (s < 0) continue;
            for (; s < n && keys_sorted[s] == key; ++s) {
              const float4 p = pts[s];
              const float d = dist2_f32(q.x, q.y, q.z, p.x, p.y, p.z);
              const int j = __float_as_int(p.w);
              if (cnt < k) {
                s_d[cnt][t] = d;
                s_i[cnt][t] = j;
                if (d > wd || (d == wd && j > wi)) { wd = d; wi = j; wslot = cnt; }
                ++cnt;
              } else if (d < wd || (d == wd && j < wi)) {
                s_d[wslot][t] = d;
                s_i[wslot][t] = j;
                wd = -1.f; wi = -1;
                for (int m = 0; m < k; ++m) {
                  const float dm = s_d[m][t];
                  const int im = s_i[m][t];
                  if (dm > wd || (dm == wd && im > wi)) { wd = dm; wi = im; wslot = m; }
                }
              }
            }
            if (R == 0) break;
          }
        }
      if (cnt == k) {
        const float bound = (float)R * cell - slack;
        if (bound > 0.f && wd < bound * bound) { finished = true; break; }
      }
    }
    // not provably complete within max_shell shells (sparse region): left to a coarser grid, unless these
    // shells already covered the whole cloud
    if (!finished && r_max < r_all) continue;
    if (done) done[qi] = 1;
    // ascending (d2, index): insertion sort of the thread's column
    for (int a = 1; a < cnt; ++a) {
      const float da = s_d[a][t];
      const int ia = s_i[a][t];
      int b = a - 1;
      while (b >= 0 && (s_d[b][t] > da || (s_d[b][t] == da && s_i[b][t] > ia))) {
        s_d[b + 1][t] = s_d[b][t];
        s_i[b + 1][t] = s_i[b][t];
        --b;
      }
      s_d[b + 1][t] = da;
      s_i[b + 1][t] = ia;
    }
    for (int m = 0; m < k; ++m) {
      nbr[(int64_t)qi * k + m] = m < cnt ? s_i[m][t] : -1;
      if (d2_out) d2_out[(int64_t)qi * k + m] = m < cnt ? s_d[m][t] : INFINITY;
    }
  }
}

// bit (image) of word (image / 64) of point p: the views of the mapping as bit sets
__global__ __launch_bounds__(256) void view_bits_kernel(const int32_t* __restrict__ view_point,
                                                         const int64_t* __restrict__ images, int64_t V,
                                                         int n_words, unsigned long long* __restrict__ bits) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t img = images[v];
    atomicOr(&bits[(int64_t)view_point[v] * n_words + (img >> 6)], 1ULL << (img & 63));
  }
}

// out[v][c] = (1 + #{i < k_list[c] : neighbour i of the view's point is seen by the view's image}) / (k_c + 1)
__global__ __launch_bounds__(256) void occlusion_kernel(const int32_t* __restrict__ view_point,
                                                         const int64_t* __restrict__ images, int64_t V,
                                                         const int32_t* __restrict__ nbr, int k,
                                                         const unsigned long long* __restrict__ bits, int n_words,
                                                         const int32_t* __restrict__ k_list, int n_k,
                                                         float* __restrict__ out) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = view_point[v], img = images[v];
    const int w = (int)(img >> 6);
    const unsigned long long bit = 1ULL << (img & 63);
    int seen = 0, c = 0;
    for (int i = 0; i < k && c < n_k; ++i) {
      const int32_t q = nbr[p * k + i];
      if (q >= 0 && (bits[(int64_t)q * n_words + w] & bit)) ++seen;
      while (c < n_k && i + 1 == k_list[c]) {
        out[v * n_k + c] = (float)(1 + seen) / (float)(k_list[c] + 1);
        ++c;
      }
    }
  }
}

struct KnnLayout {
  uint64_t *keys, *keys_sorted, *tkeys, *qkeys, *qkeys_sorted;
  int32_t *ids, *perm, *tvals, *qids, *qperm;
  float4 *pts, *qpts;
  char* temp;
  size_t temp_bytes, total;
  uint64_t cap;
};
// n search points; nq > 0: a separate query cloud (dva_knn_query) with its own sort; the two sorts share the
// temp storage
static int knn_layout(void* ws, int64_t n, KnnLayout* L, int64_t nq = 0) {
  size_t tmp = 0, qtmp = 0;
  uint64_t* nk = nullptr;
  int32_t* nv = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, tmp, nk, nk, nv, nv, (size_t)n, 0, 3 * CELL_BITS, (hipStream_t)0) !=
      hipSuccess)
    return DVA_ERR_LAUNCH;
  if (nq > 0 && rocprim::radix_sort_pairs(nullptr, qtmp, nk, nk, nv, nv, (size_t)nq, 0, 3 * CELL_BITS,
                                          (hipStream_t)0) != hipSuccess)
    return DVA_ERR_LAUNCH;
  if (qtmp > tmp) tmp = qtmp;
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
  L->qkeys = c.take<uint64_t>((size_t)nq);
  L->qids = c.take<int32_t>((size_t)nq);
  L->qkeys_sorted = c.take<uint64_t>((size_t)nq);
  L->qperm = c.take<int32_t>((size_t)nq);
  L->qpts = c.take<float4>((size_t)nq);
  L->temp_bytes = tmp;
  L->temp = c.take<char>(tmp);
  L->total = c.used();
  return DVA_OK;
}

static void launch_knn_query(const float4* qpts, int64_t nq, const float4* pts, const uint64_t* keys_sorted,
                             int64_t n, const float* bbox, float cell, const uint64_t* tkeys, const int32_t* tvals,
                             uint32_t mask, int k, int max_shell, uint8_t* done, int32_t* neighbors, float* dist2,
                             hipStream_t s) {
  int64_t qb = (nq + KNN_TPB - 1) / KNN_TPB;
  if (qb > 256 * 32) qb = 256 * 32;
  if (k <= 64)
    hipLaunchKernelGGL(knn_query_kernel<64>, dim3((int)qb), dim3(KNN_TPB), 0, s, qpts, nq, pts, keys_sorted, n, bbox,
                       cell, tkeys, tvals, mask, k, max_shell, done, neighbors, dist2);
  else
    hipLaunchKernelGGL(knn_query_kernel<128>, dim3((int)qb), dim3(KNN_TPB), 0, s, qpts, nq, pts, keys_sorted, n, bbox,
                       cell, tkeys, tvals, mask, k, max_shell, done, neighbors, dist2);
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_knn_workspace_bytes(int64_t n) {
  if (n < 0) return DVA_ERR_INVALID;
  if (n > 0x3fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return 256;
  KnnLayout L;
  int rc = knn_layout(nullptr, n, &L);
  if (rc) return rc;
  return (int64_t)L.total;
}

int dva_knn(const float* xyz, int64_t n, const float* bbox, float cell, int32_t k, int32_t max_shell,
            uint8_t* done, int32_t* neighbors, float* dist2, void* workspace, int64_t workspace_bytes,
            void* stream) {
  if (n < 0 || k <= 0 || k > KNN_KMAX || !(cell > 0.f) || max_shell < 1) return DVA_ERR_INVALID;
  if (n > 0x3fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return DVA_OK;
  if (!xyz || !bbox || !neighbors || !workspace) return DVA_ERR_INVALID;
  KnnLayout L;
  int rc = knn_layout(workspace, n, &L);
  if (rc) return rc;
  if ((int64_t)L.total > workspace_bytes) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_keys_kernel, dim3(capped_grid(n, 256, 8192)), dim3(256), 0, s, xyz, n, bbox, 1.f / cell,
                     L.keys, L.ids);
  size_t tmp = L.temp_bytes;
  if (rocprim::radix_sort_pairs(L.temp, tmp, L.keys, L.keys_sorted, L.ids, L.perm, (size_t)n, 0, 3 * CELL_BITS, s) !=
      hipSuccess)
    return DVA_ERR_LAUNCH;
  if (hipMemsetAsync(L.tkeys, 0xff, L.cap * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(knn_cells_kernel, dim3(capped_grid(n, 256, 8192)), dim3(256), 0, s, xyz, L.keys_sorted, L.perm, n,
                     L.pts, L.tkeys, L.tvals, (uint32_t)(L.cap - 1));
  launch_knn_query(L.pts, n, L.pts, L.keys_sorted, n, bbox, cell, L.tkeys, L.tvals, (uint32_t)(L.cap - 1), k, max_shell,
                   done, neighbors, dist2, s);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int64_t dva_knn_query_workspace_bytes(int64_t n_query, int64_t n_search) {
  if (n_query < 0 || n_search < 0) return DVA_ERR_INVALID;
  if (n_query > 0x7fffffffLL || n_search > 0x3fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n_query == 0 || n_search == 0) return 256;
  KnnLayout L;
  int rc = knn_layout(nullptr, n_search, &L, n_query);
  if (rc) return rc;
  return (int64_t)L.total;
}

int dva_knn_query(const float* query_xyz, int64_t n_query, const float* search_xyz, int64_t n_search,
                  const float* bbox, float cell, int32_t k, int32_t max_shell, uint8_t* done, int32_t* neighbors,
                  float* dist2, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_query < 0 || n_search < 0 || k <= 0 || k > KNN_KMAX || n_search < k || !(cell > 0.f) || max_shell < 1)
    return DVA_ERR_INVALID;
  if (n_query > 0x7fffffffLL || n_search > 0x3fffffffLL) return DVA_ERR_UNSUPPORTED;
  if (n_query == 0) return DVA_OK;
  if (!query_xyz || !search_xyz || !bbox || !neighbors || !workspace) return DVA_ERR_INVALID;
  KnnLayout L;
  int rc = knn_layout(workspace, n_search, &L, n_query);
  if (rc) return rc;
  if ((int64_t)L.total > workspace_bytes) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const float inv_cell = 1.f / cell;
  // the grid of the search cloud
  hipLaunchKernelGGL(knn_keys_kernel, dim3(capped_grid(n_search, 256, 8192)), dim3(256), 0, s, search_xyz, n_search,
                     bbox, inv_cell, L.keys, L.ids);
  size_t tmp = L.temp_bytes;
  if (rocprim::radix_sort_pairs(L.temp, tmp, L.keys, L.keys_sorted, L.ids, L.perm, (size_t)n_search, 0, 3 * CELL_BITS,
                                s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  if (hipMemsetAsync(L.tkeys, 0xff, L.cap * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(knn_cells_kernel, dim3(capped_grid(n_search, 256, 8192)), dim3(256), 0, s, search_xyz,
                     L.keys_sorted, L.perm, n_search, L.pts, L.tkeys, L.tvals, (uint32_t)(L.cap - 1));
  // the queries in the cell order of the same grid, so that the lanes of a wavefront walk the same cells
  hipLaunchKernelGGL(knn_keys_kernel, dim3(capped_grid(n_query, 256, 8192)), dim3(256), 0, s, query_xyz, n_query, bbox,
                     inv_cell, L.qkeys, L.qids);
  tmp = L.temp_bytes;
  if (rocprim::radix_sort_pairs(L.temp, tmp, L.qkeys, L.qkeys_sorted, L.qids, L.qperm, (size_t)n_query, 0,
                                3 * CELL_BITS, s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(knn_query_points_kernel, dim3(capped_grid(n_query, 256, 8192)), dim3(256), 0, s, query_xyz,
                     L.qperm, n_query, L.qpts);
  launch_knn_query(L.qpts, n_query, L.pts, L.keys_sorted, n_search, bbox, cell, L.tkeys, L.tvals, (uint32_t)(L.cap - 1),
                   k, max_shell, done, neighbors, dist2, s);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_view_occlusion(const int32_t* view_point, const int64_t* images, int64_t n_views, int64_t n_points,
                       int32_t n_images, const int32_t* neighbors, int32_t k, const int32_t* k_list,
                       int32_t n_k, uint64_t* bits, float* out, void* stream) {
  if (n_views < 0 || n_points < 0 || n_images <= 0 || k <= 0 || n_k <= 0) return DVA_ERR_INVALID;
  if (n_views == 0) return DVA_OK;
  if (!view_point || !images || !neighbors || !k_list || !bits || !out) return DVA_ERR_INVALID;
  const int n_words = (n_images + 63) / 64;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(bits, 0, (size_t)n_points * n_words * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(view_bits_kernel, dim3(capped_grid(n_views, 256, 8192)), dim3(256), 0, s, view_point, images,
                     n_views, n_words, (unsigned long long*)bits);
  hipLaunchKernelGGL(occlusion_kernel, dim3(capped_grid(n_views, 256, 8192)), dim3(256), 0, s, view_point, images,
                     n_views, neighbors, k, (const unsigned long long*)bits, n_words, k_list, n_k, out);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
