// The two image picks that walk the nested CSR point -> views -> atoms for small exact integer results.
//
// CenterRoll (reference core/data_transform/multimodal/image.py:999-1029).  Per image, C = the distinct 8-bit angular
// columns col8 = long(float(x) * 256 / W) of its atoms; for every candidate roll r in arange(0, 256, int(256 / res)),
// lo / hi = min / max of (c + r) mod 256 over C, cost = (hi - lo) + int(|(float(hi) + lo) / 2 - 128|); the first
// candidate of minimal cost wins and rolling = long(float(r) / 256 * W).  For 0 <= x < W <= 32767 the three float
// expressions are exact integer functions: col8 = (x * 256) / W, the centre term |hi + lo - 256| >> 1 and
// rolling = (r * W) >> 8 (tests/test_image_pick_host.py holds them to the torch expressions), so everything here is
// integer arithmetic, and C is a 256-bit occupancy bitmap per image: no sort, no [pixels, candidates] tensor.
//   1. bits: one thread per view ORs the bits of its atoms into the eight words of its image.  A view's atoms are a
//      splat of neighbouring columns, so a thread gathers the bits of one word in a register and touches memory when
//      the word changes; it first reads the word and skips the atomic when its bits are there already (the read may
//      be stale, which costs a redundant atomic and nothing else).  After the first few thousand views nearly every
//      bit of an image is set, and the B * 8 hot words see loads, not atomics.  Integer OR: order-free.
//   2. pick: one wavefront per image, the words in LDS, a lane per candidate: rotate the bitmap left by r, lowest and
//      highest set bit, cost; wave minimum of (cost << 8 | candidate index) = the first minimum.  An image without
//      atoms gets rolling 0 and adds 1 to info[0].
//   3. roll (dva_mapping_roll_pixels): x = (x + rollings[image]) mod W in place, one thread per view.
// info = {images without atoms, flags}: flag bit 0 a view whose image is outside [0, B), bit 1 an atom whose column
// is outside [0, W) -- the cases the integer restatement does not cover; the caller then takes the composition.
//
// Coverage counts of PickImagesFromMemoryCredit (:803-868).  The reference keeps unseen[i, p] = image i sees point p
// and no picked image sees p, sums its rows before every draw and clears the columns of the pick after it.  Here the
// state is covered uint8 [N], and one step is one launch over every setting (item): the thread that owns point p first
// sets covered[p] if a view of p belongs to `pick`, and for a point still uncovered adds 1 to the count of every image
// that sees it -- into an LDS histogram per workgroup up to COVER_HIST images in all, flushed with one global integer
// atomic per non-zero bin, and with global integer atomics above that.  Integer sums: order-free.  The same launch
// clears the row the NEXT step will count into, so a step is one launch and no host round trip.  A view is a distinct
// (point, image) pair in every mapping the library builds (from_dense unites repeated pairs); a repeated pair would
// count twice.  Item descriptors travel by value, COVER_GROUP per launch, the item of the pick with every launch.
#include "dva_common.h"
#include "mapping_args.h"
#include "scan.h"

namespace dva {

constexpr int CENTER_THREADS = 256;
constexpr int CENTER_GRID = 4096;
constexpr int COVER_GROUP = 32;       // items per launch
constexpr int COVER_THREADS = 256;
constexpr int COVER_GRID = 1024;
constexpr int COVER_HIST = 1024;      // images in all up to which a workgroup counts in LDS: 4 KiB

enum { CI_EMPTY = 0, CI_FLAGS = 1, CI_COUNT = 2 };

// ---------------------------------------------------------------------------------------------------------------
// CenterRoll
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void center_init_kernel(uint32_t* __restrict__ bitmap, int64_t words,
                                                          int* __restrict__ info) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t i = i0; i < words; i += (int64_t)gridDim.x * 256) bitmap[i] = 0u;
  if (i0 < CI_COUNT) info[i0] = 0;
}

__device__ __forceinline__ void center_flush(uint32_t* __restrict__ bitmap, int64_t word, uint32_t bits) {
  if (bits == 0u) return;
  if ((bitmap[word] & bits) != bits) atomicOr(&bitmap[word], bits);
}

__global__ __launch_bounds__(CENTER_THREADS) void center_bits_kernel(const int64_t* __restrict__ images,
                                                                     const int64_t* __restrict__ atom_ptr,
                                                                     const uint32_t* __restrict__ pixels, int64_t V,
                                                                     int64_t P, int64_t B, int W,
                                                                     uint32_t* __restrict__ bitmap,
                                                                     int* __restrict__ info) {
  for (int64_t v = blockIdx.x * (int64_t)CENTER_THREADS + threadIdx.x; v < V;
       v += (int64_t)gridDim.x * CENTER_THREADS) {
    const int64_t img = images[v];
    if (img < 0 || img >= B) {
      atomicOr(&info[CI_FLAGS], 1);
      continue;
    }
    int64_t a0, a1;
    csr_range(atom_ptr, v, P, &a0, &a1);
    int cur = -1;
    uint32_t bits = 0u;
    bool outside = false;
    for (int64_t a = a0; a < a1; ++a) {
      const int x = (int16_t)(pixels[a] & 0xffffu);
      if (x < 0 || x >= W) {
        outside = true;
        continue;
      }
      const int col = (x * 256) / W;      // < 256 for x < W
      const int w = col >> 5;
      if (w != cur) {
        if (cur >= 0) center_flush(bitmap, img * 8 + cur, bits);
        cur = w;
        bits = 0u;
      }
      bits |= 1u << (col & 31);
    }
    if (cur >= 0) center_flush(bitmap, img * 8 + cur, bits);
    if (outside) atomicOr(&info[CI_FLAGS], 2);
  }
}

__global__ __launch_bounds__(DVA_WAVE) void center_pick_kernel(const uint32_t* __restrict__ bitmap, int64_t B, int W,
                                                               int step, int n_cand, int64_t* __restrict__ rollings,
                                                               int* __restrict__ info) {
  __shared__ uint32_t words[8];
  const int lane = threadIdx.x;
  for (int64_t img = blockIdx.x; img < B; img += gridDim.x) {
    if (lane < 8) words[lane] = bitmap[img * 8 + lane];
    __syncthreads();
    uint32_t any = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) any |= words[i];
    int best = 0x7fffffff;
    if (any != 0u) {
      for (int k = lane; k < n_cand; k += DVA_WAVE) {
        const int r = k * step;
        const int q = r >> 5, s = r & 31;
        // bit c of the set moves to (c + r) mod 256: word i of the rotated set
        int lo = -1, hi = -1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const uint32_t a = words[(i - q) & 7], b = words[(i - q - 1) & 7];
          const uint32_t w = s ? ((a << s) | (b >> (32 - s))) : a;
          if (w != 0u) {
            if (lo < 0) lo = 32 * i + __builtin_ctz(w);
            hi = 32 * i + 31 - __builtin_clz(w);
          }
        }
        int centre = hi + lo - 256;
        centre = (centre < 0 ? -centre : centre) >> 1;
        const int key = (((hi - lo) + centre) << 8) | k;
        best = key < best ? key : best;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(best, o, DVA_WAVE);
      best = other < best ? other : best;
    }
    if (lane == 0) {
      if (any == 0u) {
        rollings[img] = 0;
        atomicAdd(&info[CI_EMPTY], 1);
      } else {
        const int64_t r = (int64_t)(best & 255) * step;
        rollings[img] = (r * W) >> 8;
      }
    }
    __syncthreads();      // the words are reused by the next image
  }
}

__global__ __launch_bounds__(CENTER_THREADS) void roll_pixels_kernel(const int64_t* __restrict__ images,
                                                                     const int64_t* __restrict__ atom_ptr,
                                                                     uint32_t* __restrict__ pixels, int64_t V,
                                                                     int64_t P, const int64_t* __restrict__ rollings,
                                                                     int64_t B, int64_t W) {
  for (int64_t v = blockIdx.x * (int64_t)CENTER_THREADS + threadIdx.x; v < V;
       v += (int64_t)gridDim.x * CENTER_THREADS) {
    const int64_t img = images[v];
    if (img < 0 || img >= B) continue;
    const int64_t roll = rollings[img];
    int64_t a0, a1;
    csr_range(atom_ptr, v, P, &a0, &a1);
    for (int64_t a = a0; a < a1; ++a) {
      const uint32_t px = pixels[a];
      // the remainder takes the sign of W > 0, as the int64 tensors compute it
      int64_t x = ((int64_t)(int16_t)(px & 0xffffu) + roll) % W;
      if (x < 0) x += W;
      pixels[a] = (px & 0xffff0000u) | (uint32_t)(uint16_t)(int16_t)x;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// coverage counts
// ---------------------------------------------------------------------------------------------------------------

struct CoverItem {
  const int64_t* pointers;
  const int64_t* images;
  int64_t n, v, b, base;      // points, views, images, global id of its image 0
};

struct CoverGroup {
  CoverItem item[COVER_GROUP];
};

template <bool HIST>
__global__ __launch_bounds__(COVER_THREADS) void coverage_step_kernel(CoverGroup g, int count, CoverItem picked,
                                                                       int64_t pick_local, int64_t n_points,
                                                                       int64_t n_images,
                                                                       uint8_t* __restrict__ covered,
                                                                       u64* __restrict__ counts,
                                                                       int64_t* __restrict__ clear) {
  __shared__ int hist[HIST ? COVER_HIST : 1];
  if (HIST) {
    for (int i = threadIdx.x; i < (int)n_images; i += COVER_THREADS) hist[i] = 0;
    __syncthreads();
  }
  if (clear && blockIdx.x == 0)
    for (int64_t i = threadIdx.x; i < n_images; i += COVER_THREADS) clear[i] = 0;
  for (int64_t p = blockIdx.x * (int64_t)COVER_THREADS + threadIdx.x; p < n_points;
       p += (int64_t)gridDim.x * COVER_THREADS) {
    bool c = covered[p] != 0;
    if (!c && pick_local >= 0 && p < picked.n) {
      int64_t v0, v1;
      csr_range(picked.pointers, p, picked.v, &v0, &v1);
      for (int64_t v = v0; v < v1 && !c; ++v) c = picked.images[v] == pick_local;
      if (c) covered[p] = 1;      // p has one owner
    }
    if (c) continue;
    for (int k = 0; k < count; ++k) {
      const CoverItem& it = g.item[k];
      if (p >= it.n) continue;
      int64_t v0, v1;
      csr_range(it.pointers, p, it.v, &v0, &v1);
      for (int64_t v = v0; v < v1; ++v) {
        const int64_t img = it.images[v];
        if (img < 0 || img >= it.b) continue;      // base + b <= n_images: checked by the entry
        if (HIST)
          atomicAdd(&hist[it.base + img], 1);
        else
          atomicAdd(&counts[it.base + img], (u64)1);
      }
    }
  }
  if (HIST) {
    __syncthreads();
    for (int i = threadIdx.x; i < (int)n_images; i += COVER_THREADS) {
      const int h = hist[i];
      if (h != 0) atomicAdd(&counts[i], (u64)h);
    }
  }
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_mapping_center_workspace_bytes(int64_t n_images) {
  if (n_images < 0) return DVA_ERR_INVALID;
  if (n_images >= I31_LIMIT / 8) return DVA_ERR_UNSUPPORTED;
  return (int64_t)align_up((size_t)(n_images > 0 ? n_images : 1) * 8 * sizeof(uint32_t), 16);
}

int dva_mapping_center_rollings(const int64_t* images, const int64_t* atom_ptr, const void* pixels, int32_t pixel_bytes,
                                int64_t n_views, int64_t n_atoms, int64_t n_images, int64_t width, int32_t angular_res,
                                int64_t* rollings, int32_t* info, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  if (any_negative({n_views, n_atoms, n_images}) || width < 1 || angular_res < 1 || angular_res > 256)
    return DVA_ERR_INVALID;
  const int rc = pixel_bytes_code(pixel_bytes);
  if (rc != DVA_OK) return rc;
  if (fits_i31({n_views, n_atoms}) != DVA_OK || n_images >= I31_LIMIT / 8 || width > 32767) return DVA_ERR_UNSUPPORTED;
  if (!info || !workspace || ((uintptr_t)workspace & 3) || (n_images > 0 && !rollings)) return DVA_ERR_INVALID;
  if (!mapping_arrays_ok(images, atom_ptr, pixels, n_views, n_atoms)) return DVA_ERR_INVALID;
  if (workspace_bytes < dva_mapping_center_workspace_bytes(n_images)) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* bitmap = (uint32_t*)workspace;
  const int step = 256 / angular_res;               // int(256 / angular_res) >= 1
  const int n_cand = (255 + step) / step;           // len(arange(0, 256, step))
  hipLaunchKernelGGL(center_init_kernel, dim3(capped_grid(n_images * 8, 256 * 4, 1024)), dim3(256), 0, s, bitmap,
                     n_images * 8, (int*)info);
  if (n_views > 0)
    hipLaunchKernelGGL(center_bits_kernel, dim3(capped_grid(n_views, CENTER_THREADS, CENTER_GRID)),
                       dim3(CENTER_THREADS), 0, s, images, atom_ptr, (const uint32_t*)pixels, n_views, n_atoms,
                       n_images, (int)width, bitmap, (int*)info);
  if (n_images > 0)
    hipLaunchKernelGGL(center_pick_kernel, dim3(capped_grid(n_images, 1, CENTER_GRID)), dim3(DVA_WAVE), 0, s,
                       (const uint32_t*)bitmap, n_images, (int)width, step, n_cand, rollings, (int*)info);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_mapping_roll_pixels(const int64_t* images, const int64_t* atom_ptr, void* pixels, int32_t pixel_bytes,
                            int64_t n_views, int64_t n_atoms, const int64_t* rollings, int64_t n_images,
                            int64_t width, void* stream) {
  if (any_negative({n_views, n_atoms, n_images}) || width < 1) return DVA_ERR_INVALID;
  const int rc = pixel_bytes_code(pixel_bytes);
  if (rc != DVA_OK) return rc;
  if (fits_i31({n_views, n_atoms, n_images}) != DVA_OK || width > 32767) return DVA_ERR_UNSUPPORTED;
  if ((n_images > 0 && !rollings) || !mapping_arrays_ok(images, atom_ptr, pixels, n_views, n_atoms))
    return DVA_ERR_INVALID;
  if (n_views == 0 || n_atoms == 0 || n_images == 0) return DVA_OK;
  hipLaunchKernelGGL(roll_pixels_kernel, dim3(capped_grid(n_views, CENTER_THREADS, CENTER_GRID)),
                     dim3(CENTER_THREADS), 0, (hipStream_t)stream, images, atom_ptr, (uint32_t*)pixels, n_views,
                     n_atoms, rollings, n_images, width);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_mapping_coverage_group_items(void) { return COVER_GROUP; }

int dva_mapping_coverage_hist_images(void) { return COVER_HIST; }

int dva_mapping_coverage_step(const struct dva_coverage_item* items, int64_t n_items, int64_t n_points,
                              int64_t n_images, int64_t pick, uint8_t* covered, int64_t* counts, int64_t* clear,
                              void* stream) {
  // every check comes before the first HIP call
  if (!items || n_items < 1 || n_points < 1 || n_images < 1 || !covered || !counts || counts == clear)
    return DVA_ERR_INVALID;
  if (pick < -1 || pick >= n_images) return DVA_ERR_INVALID;
  if (fits_i31({n_points, n_images}) != DVA_OK) return DVA_ERR_UNSUPPORTED;
  int64_t end = 0, pick_item = -1;
  for (int64_t b = 0; b < n_items; ++b) {
    const struct dva_coverage_item& it = items[b];
    if (any_negative({it.n_points, it.n_views, it.n_images}) || it.n_points > n_points) return DVA_ERR_INVALID;
    if (fits_i31({it.n_views}) != DVA_OK) return DVA_ERR_UNSUPPORTED;
    if ((it.n_points > 0 && !it.pointers) || (it.n_views > 0 && !it.images)) return DVA_ERR_INVALID;
    if (it.image_base < end || it.n_images > n_images - it.image_base) return DVA_ERR_INVALID;      // ascending, no overlap
    end = it.image_base + it.n_images;
    if (pick >= it.image_base && pick < end) pick_item = b;
  }
  CoverItem picked = CoverItem{};
  int64_t pick_local = -1;
  if (pick_item >= 0) {
    const struct dva_coverage_item& it = items[pick_item];
    picked = CoverItem{it.pointers, it.images, it.n_points, it.n_views, it.n_images, it.image_base};
    pick_local = pick - it.image_base;
  }
  hipStream_t s = (hipStream_t)stream;
  const bool hist = n_images <= COVER_HIST;
  const dim3 grid(capped_grid(n_points, COVER_THREADS, COVER_GRID));
  const int64_t n_groups = (n_items + COVER_GROUP - 1) / COVER_GROUP;
  for (int64_t gi = 0; gi < n_groups; ++gi) {
    const int64_t b0 = gi * COVER_GROUP;
    const int count = (int)(n_items - b0 < COVER_GROUP ? n_items - b0 : COVER_GROUP);
    CoverGroup g;
    for (int k = 0; k < count; ++k) {
      const struct dva_coverage_item& it = items[b0 + k];
      g.item[k] = CoverItem{it.pointers, it.images, it.n_points, it.n_views, it.n_images, it.image_base};
    }
    for (int k = count; k < COVER_GROUP; ++k) g.item[k] = CoverItem{};
    int64_t* clr = gi == 0 ? clear : nullptr;
    if (hist)
      hipLaunchKernelGGL(coverage_step_kernel<true>, grid, dim3(COVER_THREADS), 0, s, g, count, picked, pick_local,
                         n_points, n_images, covered, (u64*)counts, clr);
    else
      hipLaunchKernelGGL(coverage_step_kernel<false>, grid, dim3(COVER_THREADS), 0, s, g, count, picked, pick_local,
                         n_points, n_images, covered, (u64*)counts, clr);
  }
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
