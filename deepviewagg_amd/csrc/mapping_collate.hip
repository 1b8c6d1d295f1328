// Mapping collation: B mappings (nested CSR point -> views -> atoms) stacked into one, the batch that
// CSRBatch.from_csr_list builds for ImageMappings (reference core/multimodal/csr.py:352-420), with the empty groups of
// insert_empty_groups (:197-229) written in the same pass.
//
// Item b has n_b points, v_b views and a_b atoms, all three array SHAPES known to the host, and a destination
// point_base_b (ascending, no overlap).  view_base_b and atom_base_b are the sums of v and a of the items before it.
//
//   out_pointers[0] = 0, out_pointers[point_base_b + i] = pointers_b[i] + view_base_b (1 <= i <= n_b); every entry no
//     item covers holds the views stacked so far (view_base of the next item, the total after the last);
//   out_images[view_base_b + j] = images_b[j] + off_b, off_b = sum over c < b of (max(images_c) + 1, 0 without views);
//   out_atom_ptr[0] = 0, out_atom_ptr[view_base_b + j] = atom_ptr_b[j] + atom_base_b (1 <= j <= v_b);
//   pixels and features are copied as bits.
//
// The only data-dependent quantity is off.  Three kinds of launches, no host read:
//   1. maxima: block (x, item) reduces a slice of the item's images to one partial maximum in the workspace (every
//      partial slot is written, INT64_MIN for an empty slice; no atomics, no initialisation pass);
//   2. scan: one block reduces the partials of every item to its step and scans the steps;
//   3. fill: block (x, item) grid-strides over the five output ranges the item owns.  Every output element has one
//      owner and is written once; ranges are bounded by the shapes alone, no value read from `pointers` or `atom_ptr`
//      is ever used as an address.
// Item descriptors travel by value as kernel arguments, COLLATE_GROUP items per launch (5 pointers + 8 int64 each,
// 3.3 KB): a larger batch takes more launches of 1 and 3, and the entry holds no host memory after it returns.
#include "mapping_args.h"
#include "scan.h"

namespace dva {

constexpr int COLLATE_GROUP = 32;        // items per launch
constexpr int COLLATE_THREADS = 256;
constexpr int COLLATE_PARTIALS = 128;    // partial maxima per item (blocks of the maxima launch along x)
constexpr int COLLATE_GRID = 1024;       // blocks per item of the fill (grid-stride above)
constexpr int COLLATE_MAX_F = 1 << 16;
constexpr int64_t COLLATE_NONE = -0x7fffffffffffffffLL - 1;

struct CollateItem {
  const int64_t* pointers;
  const int64_t* images;
  const int64_t* atom_ptr;
  const uint32_t* pixels;      // int16 (x, y) pairs
  const uint32_t* features;    // fp32 [v, F] as bits, or null
  int64_t n, v, a;
  int64_t point_base, view_base, atom_base;
  int64_t lead;                // the entries [0, lead) of out_pointers in front of the first item of the batch (else 0)
  int64_t gap;                 // the entries after the item's own that it fills: up to the next item or the end
};

struct CollateGroup {
  CollateItem item[COLLATE_GROUP];
};

struct CollateLayout {
  int64_t *partial, *step, *off;
  int64_t total;
};

static inline CollateLayout collate_layout(void* ws, int64_t n_items) {
  CollateLayout L;
  Carver c(ws, 16);
  L.partial = c.take<int64_t>(n_items * COLLATE_PARTIALS);
  L.step = c.take<int64_t>(n_items);
  L.off = c.take<int64_t>(n_items);
  L.total = (int64_t)c.used();
  return L;
}

// ---------------------------------------------------------------------------------------------------------------
// 1. partial maxima of the image ids
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(COLLATE_THREADS) void collate_max_kernel(CollateGroup g, int64_t first_item,
                                                                       int64_t* __restrict__ partial) {
  __shared__ long long wmax[COLLATE_THREADS / DVA_WAVE];
  const CollateItem& it = g.item[blockIdx.y];
  const int64_t* __restrict__ images = it.images;
  long long m = COLLATE_NONE;
  for (int64_t j = blockIdx.x * (int64_t)COLLATE_THREADS + threadIdx.x; j < it.v;
       j += (int64_t)gridDim.x * COLLATE_THREADS)
    m = max(m, (long long)images[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (long long)__shfl_xor(m, o, DVA_WAVE));
  if ((threadIdx.x & (DVA_WAVE - 1)) == 0) wmax[threadIdx.x / DVA_WAVE] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < COLLATE_THREADS / DVA_WAVE; ++k) m = max(m, wmax[k]);
    partial[(first_item + blockIdx.y) * COLLATE_PARTIALS + blockIdx.x] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// 2. steps and their exclusive scan: off[b] = sum over c < b of step[c]
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SCAN_THREADS) void collate_scan_kernel(const int64_t* __restrict__ partial,
                                                                     int n_partials, int64_t n_items,
                                                                     int64_t* __restrict__ step,
                                                                     int64_t* __restrict__ off,
                                                                     int64_t* __restrict__ out_offsets) {
  __shared__ int64_t wsum[SCAN_THREADS / DVA_WAVE];
  const int lane = threadIdx.x & (DVA_WAVE - 1), w = threadIdx.x / DVA_WAVE;
  // one wavefront per item: the maximum of its partials; an item without views has none
  for (int64_t b = w; b < n_items; b += SCAN_THREADS / DVA_WAVE) {
    long long m = COLLATE_NONE;
    for (int k = lane; k < n_partials; k += DVA_WAVE) m = max(m, (long long)partial[b * COLLATE_PARTIALS + k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (long long)__shfl_xor(m, o, DVA_WAVE));
    // max + 1 in int64 arithmetic (wrapping, as the int64 tensors add)
    if (lane == 0) step[b] = m == COLLATE_NONE ? 0 : (int64_t)((u64)m + 1ull);
  }
  __syncthreads();
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < n_items; c0 += SCAN_THREADS) {
    const int64_t i = c0 + threadIdx.x;
    const int64_t s = i < n_items ? step[i] : 0;
    int64_t total;
    const int64_t excl = block_excl_scan<int64_t>(s, &total, wsum);
    if (i < n_items) {
      off[i] = carry + excl;
      if (out_offsets) out_offsets[i] = carry + excl;
    }
    carry += total;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// 3. fill
// ---------------------------------------------------------------------------------------------------------------

// dst[i] = src[i] for n 32-bit words, both 4-byte aligned: 16-byte accesses over the part where dst is 16-byte aligned
// when src is aligned with it, single words before and after, and single words throughout when it is not.
__device__ __forceinline__ void copy_words(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int64_t n,
                                           int64_t tid, int64_t nthreads) {
  int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  if (((uintptr_t)(src + head) & 15u) != 0) {
    for (int64_t i = tid; i < n; i += nthreads) dst[i] = src[i];
    return;
  }
  const int64_t nvec = (n - head) >> 2;
  for (int64_t i = tid; i < head; i += nthreads) dst[i] = src[i];
  const uint4* __restrict__ s4 = (const uint4*)(src + head);
  uint4* __restrict__ d4 = (uint4*)(dst + head);
  for (int64_t i = tid; i < nvec; i += nthreads) d4[i] = s4[i];
  for (int64_t i = head + 4 * nvec + tid; i < n; i += nthreads) dst[i] = src[i];
}

__global__ __launch_bounds__(COLLATE_THREADS) void collate_fill_kernel(CollateGroup g, int64_t first_item,
                                                                        const int64_t* __restrict__ off, int F,
                                                                        int64_t* __restrict__ out_pointers,
                                                                        int64_t* __restrict__ out_images,
                                                                        int64_t* __restrict__ out_atom_ptr,
                                                                        uint32_t* __restrict__ out_pixels,
                                                                        uint32_t* __restrict__ out_features) {
  const CollateItem& it = g.item[blockIdx.y];
  const int64_t tid = blockIdx.x * (int64_t)COLLATE_THREADS + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * COLLATE_THREADS;
  const int64_t n = it.n, v = it.v, a = it.a, vb = it.view_base, ab = it.atom_base;

  // pointers: [0, lead) zeros, the item's n entries behind point_base, `gap` entries of the views stacked so far
  for (int64_t i = tid; i < it.lead; i += nthreads) out_pointers[i] = 0;
  {
    const int64_t* __restrict__ src = it.pointers + 1;
    int64_t* __restrict__ dst = out_pointers + it.point_base + 1;
    for (int64_t i = tid; i < n; i += nthreads) dst[i] = src[i] + vb;
    for (int64_t i = tid; i < it.gap; i += nthreads) dst[n + i] = vb + v;
  }
  // images
  {
    const int64_t o = off[first_item + blockIdx.y];
    const int64_t* __restrict__ src = it.images;
    int64_t* __restrict__ dst = out_images + vb;
    for (int64_t j = tid; j < v; j += nthreads) dst[j] = src[j] + o;
  }
  // atom pointers; entry 0 belongs to the first item of the batch
  {
    const int64_t* __restrict__ src = it.atom_ptr + 1;
    int64_t* __restrict__ dst = out_atom_ptr + vb + 1;
    for (int64_t j = tid; j < v; j += nthreads) dst[j] = src[j] + ab;
    if (it.lead > 0 && tid == 0) out_atom_ptr[0] = 0;
  }
  if (a > 0) copy_words(it.pixels, out_pixels + ab, a, tid, nthreads);
  if (F > 0 && v > 0) copy_words(it.features, out_features + vb * F, v * F, tid, nthreads);
}

}  // namespace dva

using namespace dva;

extern "C" {

int dva_mapping_collate_group_items(void) { return COLLATE_GROUP; }

int64_t dva_mapping_collate_workspace_bytes(int64_t n_items) {
  if (n_items < 1) return DVA_ERR_INVALID;
  if (n_items >= I31_LIMIT / COLLATE_PARTIALS) return DVA_ERR_UNSUPPORTED;
  return collate_layout(nullptr, n_items).total;
}

int dva_mapping_collate(const struct dva_collate_item* items, int64_t n_items, int32_t pixel_bytes, int32_t F,
                        int64_t n_points_out, int64_t n_views_out, int64_t n_atoms_out, int64_t* out_pointers,
                        int64_t* out_images, int64_t* out_atom_ptr, void* out_pixels, float* out_features,
                        int64_t* out_image_offsets, void* workspace, int64_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  if (!items || n_items < 1 || !out_pointers || !out_atom_ptr || !workspace) return DVA_ERR_INVALID;
  if (any_negative({n_points_out, n_views_out, n_atoms_out, F})) return DVA_ERR_INVALID;
  if ((n_views_out > 0 && !out_images) || (n_atoms_out > 0 && !out_pixels)) return DVA_ERR_INVALID;
  if ((F > 0 && n_views_out > 0 && !out_features) || (F == 0 && out_features)) return DVA_ERR_INVALID;
  if (((uintptr_t)out_pixels & 3) || ((uintptr_t)out_features & 3) || ((uintptr_t)workspace & 15))
    return DVA_ERR_INVALID;
  int64_t end = 0, views = 0, atoms = 0, v_max = 0, work = 0;
  for (int64_t b = 0; b < n_items; ++b) {
    const struct dva_collate_item& it = items[b];
    if (any_negative({it.n_points, it.n_views, it.n_atoms})) return DVA_ERR_INVALID;
    if (!it.pointers || !mapping_arrays_ok(it.images, it.atom_ptr, it.pixels, it.n_views, it.n_atoms))
      return DVA_ERR_INVALID;
    if ((F > 0 && it.n_views > 0 && !it.features) || (F == 0 && it.features)) return DVA_ERR_INVALID;
    if ((uintptr_t)it.features & 3) return DVA_ERR_INVALID;
    if (it.point_base < end) return DVA_ERR_INVALID;      // not ascending, or inside the item before
    if (it.n_points > n_points_out - it.point_base) return DVA_ERR_INVALID;
    end = it.point_base + it.n_points;
    if (it.n_views > n_views_out - views || it.n_atoms > n_atoms_out - atoms) return DVA_ERR_INVALID;
    views += it.n_views;
    atoms += it.n_atoms;
    v_max = it.n_views > v_max ? it.n_views : v_max;
  }
  if (views != n_views_out || atoms != n_atoms_out) return DVA_ERR_INVALID;
  if (pixel_bytes != 2 || F > COLLATE_MAX_F) return DVA_ERR_UNSUPPORTED;
  if (fits_i31({n_points_out, n_views_out, n_atoms_out}) != DVA_OK || n_items >= I31_LIMIT / COLLATE_PARTIALS)
    return DVA_ERR_UNSUPPORTED;
  const CollateLayout L = collate_layout(workspace, n_items);
  if (workspace_bytes < L.total) return DVA_ERR_INVALID;

  hipStream_t s = (hipStream_t)stream;
  const int n_partials = capped_grid(v_max, 4 * COLLATE_THREADS, COLLATE_PARTIALS);
  const int64_t n_groups = (n_items + COLLATE_GROUP - 1) / COLLATE_GROUP;
  for (int pass = 0; pass < 2; ++pass) {
    views = atoms = 0;
    for (int64_t gi = 0; gi < n_groups; ++gi) {
      const int64_t b0 = gi * COLLATE_GROUP;
      const int count = (int)(n_items - b0 < COLLATE_GROUP ? n_items - b0 : COLLATE_GROUP);
      CollateGroup g;
      work = 1;
      for (int k = 0; k < count; ++k) {
        const struct dva_collate_item& it = items[b0 + k];
        const int64_t next = b0 + k + 1 < n_items ? items[b0 + k + 1].point_base : n_points_out;
        CollateItem& c = g.item[k];
        c = CollateItem{it.pointers, it.images, it.atom_ptr, (const uint32_t*)it.pixels, (const uint32_t*)it.features,
                        it.n_points, it.n_views, it.n_atoms, it.point_base, views, atoms,
                        b0 + k == 0 ? it.point_base + 1 : 0, next - (it.point_base + it.n_points)};
        views += it.n_views;
        atoms += it.n_atoms;
        // 16 bytes per thread and step: 2 int64 or 4 words
        const int64_t w[4] = {(c.lead + c.n + c.gap) * 2, c.v * 2, c.a, c.v * F};
        for (int q = 0; q < 4; ++q) work = w[q] > work ? w[q] : work;
      }
      for (int k = count; k < COLLATE_GROUP; ++k) g.item[k] = CollateItem{};
      if (pass == 0)
        hipLaunchKernelGGL(collate_max_kernel, dim3(n_partials, count), dim3(COLLATE_THREADS), 0, s, g, b0, L.partial);
      else
        hipLaunchKernelGGL(collate_fill_kernel, dim3(capped_grid(work, 4 * 4 * COLLATE_THREADS, COLLATE_GRID), count),
                           dim3(COLLATE_THREADS), 0, s, g, b0, (const int64_t*)L.off, (int)F, out_pointers, out_images,
                           out_atom_ptr, (uint32_t*)out_pixels, (uint32_t*)out_features);
    }
    if (pass == 0)
      hipLaunchKernelGGL(collate_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, (const int64_t*)L.partial, n_partials,
                         n_items, L.step, L.off, out_image_offsets);
  }
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
