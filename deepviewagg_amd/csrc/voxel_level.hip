// One strided level of the voxel pyramid in one device op: the output coordinates of a strided sparse convolution,
// the parent of every input voxel and, for kernel_size = 2 / stride = 2 / dilation = 1, both kernel maps
// (modules/SparseConv3d/nn.py `Conv3d._build`, modules/multimodal/modules.py `forward_3d_block_down`; the torch
// composition `downsample_coords` + two `dva_voxel_kernel_map` + `dva_voxel_parent_index` finds the same relation
// three times through three hash tables).
//
// All four results are functions of one sort:
//   bounds   per-column min / max of a coordinate tensor through per-block partials (the caller reads them once per
//            pyramid and floors them on the host for every coarser level: floor is monotone, so the floored bounds of
//            the finest tensor are the exact bounds of the floored rows of every level).
//   level    key = mixed radix of (batch, z, y, x) over the QUOTIENTS floor(c / ratio) - floor(lo / ratio), x fastest
//            (the order of downsample_coords' packed key: dividing every digit by ratio keeps the order and saves
//            sort passes); stable rocPRIM radix sort of (key, row) over the bits of the key; run heads; exclusive scan
//            (scan.h: a run of equal keys may straddle any block boundary, the scan is global); then per sorted
//            position one store of parent[row] and, at a run head, one int4 store of the floored row.
//   map      for ratio = 2 * in_stride every input voxel has one parent and one offset: d = (c - floor_to(c, ratio)) /
//            in_stride in {0,1}^3, k = (d_x * 2 + d_y) * 2 + d_z (kernel_offsets' order for an even volume: z fastest);
//            nbr_t[k, i] = parent[i] and -1 on the other seven rows, one plain store per element;
//            nbr[k, parent[i]] = i by an unsigned atomicMin over a 0xff-filled buffer: the smallest row id wins
//            (dva_voxel_kernel_map's rule for duplicate rows) and -1 stays where nothing wrote.  No hash table.
// Integer work only; no float atomics.  floor is voxel.hip's floor_to (exact, negative coordinates included).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "scan.h"

namespace dva {

constexpr int VL_TPB = 256;
constexpr int VL_BOUND_BLOCKS = 512;           // bounds partials: at most this many blocks
constexpr int64_t VL_MAX_N = 0x3fffffffLL;     // as the other voxel entries: row ids and their sums stay in int32

// floor(a / s) for s > 0; floor_div(a, s) * s is voxel.hip's floor_to(a, s)
__host__ __device__ __forceinline__ int floor_div(int a, int s) {
  int q = a / s;
  if ((a % s != 0) && (a < 0)) --q;
  return q;
}
static inline int64_t floor_div64(int64_t a, int64_t s) {
  int64_t q = a / s;
  if ((a % s != 0) && (a < 0)) --q;
  return q;
}

struct LevelGrid {     // of the quotients floor(c / ratio) (batch: c itself)
  int32_t lo[4];
  uint32_t ext[4];     // hi - lo + 1
};

// ---------------------------------------------------------------------------------------------------------------
// bounds
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VL_TPB) void level_bounds_kernel(const int4* __restrict__ coords, int64_t n,
                                                              int32_t* __restrict__ partials) {
  __shared__ int32_t sh[VL_TPB / DVA_WAVE][8];
  int32_t v[8] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
  for (int64_t i = blockIdx.x * (int64_t)VL_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VL_TPB) {
    const int4 c = coords[i];
    v[0] = min(v[0], c.x); v[1] = min(v[1], c.y); v[2] = min(v[2], c.z); v[3] = min(v[3], c.w);
    v[4] = max(v[4], c.x); v[5] = max(v[5], c.y); v[6] = max(v[6], c.z); v[7] = max(v[7], c.w);
  }
#pragma unroll
  for (int o = DVA_WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = min(v[k], __shfl_xor(v[k], o, DVA_WAVE));
#pragma unroll
    for (int k = 4; k < 8; ++k) v[k] = max(v[k], __shfl_xor(v[k], o, DVA_WAVE));
  }
  const int lane = threadIdx.x & (DVA_WAVE - 1), w = threadIdx.x / DVA_WAVE;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    int32_t r = sh[0][k];
    for (int j = 1; j < VL_TPB / DVA_WAVE; ++j) r = k < 4 ? min(r, sh[j][k]) : max(r, sh[j][k]);
    partials[blockIdx.x * 8 + k] = r;
  }
}

// one block: 32 slices of the partials per value, then the slices
__global__ __launch_bounds__(VL_TPB) void level_bounds_reduce_kernel(const int32_t* __restrict__ partials, int nb,
                                                                     int64_t* __restrict__ bounds) {
  __shared__ int32_t sh[VL_TPB / 8][8];
  const int k = threadIdx.x & 7, slice = threadIdx.x >> 3;
  int32_t r = k < 4 ? INT32_MAX : INT32_MIN;
  for (int b = slice; b < nb; b += VL_TPB / 8) {
    const int32_t x = partials[b * 8 + k];
    r = k < 4 ? min(r, x) : max(r, x);
  }
  sh[slice][k] = r;
  __syncthreads();
  if (threadIdx.x < 8) {
    r = sh[0][k];
    for (int j = 1; j < VL_TPB / 8; ++j) r = k < 4 ? min(r, sh[j][k]) : max(r, sh[j][k]);
    bounds[k] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// level
// ---------------------------------------------------------------------------------------------------------------
// record[0] = n_out, record[1] = flags
__global__ __launch_bounds__(64) void level_record_kernel(u64* __restrict__ record, u64 n_out, u64 flags) {
  if (threadIdx.x == 0) {
    record[0] = n_out;
    record[1] = flags;
  }
}

__global__ __launch_bounds__(VL_TPB) void level_key_kernel(const int4* __restrict__ coords, int64_t n, int ratio,
                                                           int in_stride, LevelGrid g, uint64_t* __restrict__ keys,
                                                           u64* __restrict__ record) {
  unsigned flags = 0;
  for (int64_t i = blockIdx.x * (int64_t)VL_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VL_TPB) {
    const int4 c = coords[i];
    if ((c.x % in_stride) | (c.y % in_stride) | (c.z % in_stride)) flags |= DVA_VOXEL_LEVEL_FLAG_STRIDE;
    // differences of int32 values taken in 64 bits; a row outside the grid becomes a huge unsigned value
    const uint64_t x = (uint64_t)((int64_t)floor_div(c.x, ratio) - g.lo[0]);
    const uint64_t y = (uint64_t)((int64_t)floor_div(c.y, ratio) - g.lo[1]);
    const uint64_t z = (uint64_t)((int64_t)floor_div(c.z, ratio) - g.lo[2]);
    const uint64_t b = (uint64_t)((int64_t)c.w - g.lo[3]);
    uint64_t key = 0;
    if (x < g.ext[0] && y < g.ext[1] && z < g.ext[2] && b < g.ext[3])
      key = ((b * g.ext[2] + z) * g.ext[1] + y) * g.ext[0] + x;
    else
      flags |= DVA_VOXEL_LEVEL_FLAG_BOUNDS;
    keys[i] = key;
  }
#pragma unroll
  for (int o = DVA_WAVE / 2; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, DVA_WAVE);
  if ((threadIdx.x & (DVA_WAVE - 1)) == 0 && flags) atomicOr(&record[1], (u64)flags);
}

__global__ __launch_bounds__(VL_TPB) void level_head_kernel(const uint64_t* __restrict__ sorted, int64_t n,
                                                            int* __restrict__ head) {
  for (int64_t i = blockIdx.x * (int64_t)VL_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VL_TPB)
    head[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

// per sorted position i: the voxel of its run = (heads before i) + head[i] - 1, in [0, n) since head[0] = 1
__global__ __launch_bounds__(VL_TPB) void level_scatter_kernel(const int4* __restrict__ coords,
                                                               const int32_t* __restrict__ order,
                                                               const int* __restrict__ head,
                                                               const int* __restrict__ before, int64_t n, int ratio,
                                                               int4* __restrict__ out_coords,
                                                               int64_t* __restrict__ parent, u64* __restrict__ record) {
  for (int64_t i = blockIdx.x * (int64_t)VL_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VL_TPB) {
    const int h = head[i];
    const int v = before[i] + h - 1;
    const int32_t row = order[i];
    parent[row] = v;
    if (h) {
      int4 c = coords[row];
      c.x = floor_div(c.x, ratio) * ratio;
      c.y = floor_div(c.y, ratio) * ratio;
      c.z = floor_div(c.z, ratio) * ratio;
      out_coords[v] = c;
    }
    if (i == 0) record[0] = (u64)before[n];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the kernel_size = 2, stride = 2 maps
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VL_TPB) void level_map_kernel(const int4* __restrict__ coords,
                                                           const int64_t* __restrict__ parent, int64_t n,
                                                           int64_t n_out, int ratio, int in_stride,
                                                           int32_t* __restrict__ nbr, int32_t* __restrict__ nbr_t) {
  for (int64_t i = blockIdx.x * (int64_t)VL_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VL_TPB) {
    const int4 c = coords[i];
    const int64_t p = parent[i];
    // c - floor_to(c, ratio) lies in [0, ratio) = [0, 2 in_stride): every digit is 0 or 1
    const int dx = (c.x - floor_div(c.x, ratio) * ratio) / in_stride;
    const int dy = (c.y - floor_div(c.y, ratio) * ratio) / in_stride;
    const int dz = (c.z - floor_div(c.z, ratio) * ratio) / in_stride;
    const int k = (dx * 2 + dy) * 2 + dz;
    const bool ok = p >= 0 && p < n_out;      // parent comes from the caller: never index with it unchecked
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) nbr_t[(int64_t)kk * n + i] = (ok && kk == k) ? (int32_t)p : -1;
    if (ok) atomicMin((unsigned*)&nbr[(int64_t)k * n_out + p], (unsigned)i);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------------------------
struct LevelLayout {
  uint64_t *keys, *sorted;
  int32_t* order;
  int *head, *before, *bsum;
  int32_t* partials;
  char* temp;
  size_t temp_bytes, total;
};

static int level_layout(void* ws, int64_t n, LevelLayout* L) {
  size_t sort_tmp = 0;
  uint64_t* k = nullptr;
  int32_t* v = nullptr;
  rocprim::counting_iterator<int32_t> it(0);
  if (rocprim::radix_sort_pairs(nullptr, sort_tmp, k, k, it, v, (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
    return DVA_ERR_LAUNCH;
  Carver w(ws);
  L->keys = w.take<uint64_t>((size_t)n);
  L->sorted = w.take<uint64_t>((size_t)n);
  L->order = w.take<int32_t>((size_t)n);
  L->head = w.take<int>((size_t)n);
  L->before = w.take<int>((size_t)n + 1);
  L->bsum = w.take<int>((size_t)scan_blocks(n) + 1);
  L->partials = w.take<int32_t>(VL_BOUND_BLOCKS * 8);
  L->temp_bytes = sort_tmp;
  L->temp = w.take<char>(sort_tmp);
  L->total = w.used();
  return DVA_OK;
}

static int level_check(int64_t n, void* ws, int64_t wsb, LevelLayout* L) {
  const int rc = level_layout(ws, n, L);
  if (rc) return rc;
  return (int64_t)L->total > wsb ? DVA_ERR_INVALID : DVA_OK;
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_voxel_level_workspace_bytes(int64_t n) {
  if (n < 0) return DVA_ERR_INVALID;
  if (n > VL_MAX_N) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return 256;
  LevelLayout L;
  const int rc = level_layout(nullptr, n, &L);
  return rc ? rc : (int64_t)L.total;
}

int dva_voxel_bounds(const int32_t* coords, int64_t n, int64_t* bounds, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  if (n < 0) return DVA_ERR_INVALID;
  if (n > VL_MAX_N) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return DVA_OK;
  if (!coords || !bounds || !workspace) return DVA_ERR_INVALID;
  if (!aligned16(coords)) return DVA_ERR_INVALID;   // rows are read as int4
  LevelLayout L;
  const int rc = level_check(n, workspace, workspace_bytes, &L);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int nb = capped_grid(n, VL_TPB * 4, VL_BOUND_BLOCKS);
  hipLaunchKernelGGL(level_bounds_kernel, dim3(nb), dim3(VL_TPB), 0, s, (const int4*)coords, n, L.partials);
  hipLaunchKernelGGL(level_bounds_reduce_kernel, dim3(1), dim3(VL_TPB), 0, s, (const int32_t*)L.partials, nb, bounds);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_voxel_level(const int32_t* in_coords, int64_t n, int32_t ratio, int32_t in_stride, const int64_t* bounds,
                    int32_t* out_coords, int64_t* parent, int64_t* record, void* workspace, int64_t workspace_bytes,
                    void* stream) {
  if (n < 0 || ratio <= 0 || in_stride <= 0) return DVA_ERR_INVALID;
  if (n > VL_MAX_N) return DVA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (record) {
      hipLaunchKernelGGL(level_record_kernel, dim3(1), dim3(64), 0, s, (u64*)record, (u64)0, (u64)0);
      DVA_CHECK_LAUNCH();
    }
    return DVA_OK;
  }
  if (!in_coords || !bounds || !out_coords || !parent || !record || !workspace) return DVA_ERR_INVALID;
  if (!aligned16(in_coords) || !aligned16(out_coords)) return DVA_ERR_INVALID;   // rows are read and written as int4
  // bounds (host): lo x y z batch, hi x y z batch of the floored rows
  LevelGrid g;
  unsigned __int128 cells = 1, quot = 1;
  for (int d = 0; d < 4; ++d) {
    const int64_t lo = bounds[d], hi = bounds[4 + d];
    if (lo > hi || lo < INT32_MIN || hi > INT32_MAX) return DVA_ERR_INVALID;
    cells *= (unsigned __int128)(hi - lo + 1);          // four factors <= 2^32: no overflow of 128 bits
    const int64_t r = d < 3 ? ratio : 1;
    const int64_t qlo = floor_div64(lo, r), qhi = floor_div64(hi, r);
    g.lo[d] = (int32_t)qlo;
    g.ext[d] = (uint32_t)(qhi - qlo + 1);
    quot *= (unsigned __int128)g.ext[d];
  }
  if (cells >= ((unsigned __int128)1 << 62)) {          // downsample_coords' packing limit: the caller takes that route
    hipLaunchKernelGGL(level_record_kernel, dim3(1), dim3(64), 0, s, (u64*)record, (u64)0,
                       (u64)DVA_VOXEL_LEVEL_FLAG_KEY);
    DVA_CHECK_LAUNCH();
    return DVA_OK;
  }
  LevelLayout L;
  const int rc = level_check(n, workspace, workspace_bytes, &L);
  if (rc) return rc;
  unsigned end_bit = 1;
  while (end_bit < 62 && ((unsigned __int128)1 << end_bit) < quot) ++end_bit;    // keys < quot <= cells < 2^62
  const int grid = capped_grid(n, VL_TPB, GRID_CAP);
  hipLaunchKernelGGL(level_record_kernel, dim3(1), dim3(64), 0, s, (u64*)record, (u64)0, (u64)0);
  hipLaunchKernelGGL(level_key_kernel, dim3(grid), dim3(VL_TPB), 0, s, (const int4*)in_coords, n, (int)ratio,
                     (int)in_stride, g, L.keys, (u64*)record);
  size_t tmp = L.temp_bytes;
  rocprim::counting_iterator<int32_t> iota(0);
  if (rocprim::radix_sort_pairs(L.temp, tmp, L.keys, L.sorted, iota, L.order, (size_t)n, 0, end_bit, s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(level_head_kernel, dim3(grid), dim3(VL_TPB), 0, s, (const uint64_t*)L.sorted, n, L.head);
  launch_scan<int>(L.head, n, L.bsum, scan_blocks(n), L.before, s);
  hipLaunchKernelGGL(level_scatter_kernel, dim3(grid), dim3(VL_TPB), 0, s, (const int4*)in_coords,
                     (const int32_t*)L.order, (const int*)L.head, (const int*)L.before, n, (int)ratio,
                     (int4*)out_coords, parent, (u64*)record);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_voxel_level_maps(const int32_t* in_coords, const int64_t* parent, int64_t n, int64_t n_out, int32_t ratio,
                         int32_t in_stride, int32_t* nbr, int32_t* nbr_t, void* stream) {
  if (n < 0 || n_out < 0 || n_out > n || in_stride <= 0 || ratio <= 0) return DVA_ERR_INVALID;
  if ((int64_t)ratio != 2 * (int64_t)in_stride) return DVA_ERR_INVALID;   // kernel_size 2, stride 2 only
  if (n > VL_MAX_N) return DVA_ERR_UNSUPPORTED;
  if (n == 0) return DVA_OK;
  if (!in_coords || !parent || !nbr_t || (n_out > 0 && !nbr)) return DVA_ERR_INVALID;
  if (!aligned16(in_coords)) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (n_out > 0 && hipMemsetAsync(nbr, 0xff, (size_t)n_out * 8 * sizeof(int32_t), s) != hipSuccess)
    return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(level_map_kernel, dim3(capped_grid(n, VL_TPB, GRID_CAP)), dim3(VL_TPB), 0, s,
                     (const int4*)in_coords, parent, n, n_out, (int)ratio, (int)in_stride, nbr, nbr_t);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
