// Mapping selection: the four ImageMapping methods that filter the nested CSR point -> views -> atoms, compact it and
// renumber its images (reference core/multimodal/image.py:2029-2093 select_images, :2095-2165 select_views,
// :2167-2210 select_points(mode='pick') = csr.py:235-294, :2279-2342 crop followed by from_dense :1728-1795).
//
// Output point m is source point point_idx[m] (any order, duplicates allowed; all points in order without it).  A
// source view survives if its mask is set and its image has a new id >= 0 -- looked up in a table image_map[n_map],
// or by binary search in the ascending image_keys[n_map] with image_map[k] the new id of key k, the form that needs
// no bound on the image ids -- and, with a crop, if at least one of its atoms is inside the box.  `compact` gives a
// surviving view the rank of its image among the distinct surviving images.
//
//   1. crop only: one thread per SOURCE view counts its atoms inside the box into vcnt[V] (0 for a masked view).
//   2. count pass, one wavefront per output point (points have 0 to a few hundred views, mostly fewer than 32: a
//      wavefront reads a point's views in one coalesced access and needs no LDS without a crop): surviving views and
//      atoms of the point, and the per-image `seen` flags, plain stores of the value 1.
//   3. two scans (int64 sums: picked duplicates can make the result larger than the source) give the first view and
//      the first atom of every output point; a one-block kernel ranks the seen images and writes the single readback
//      buffer {V', P', distinct images, flags, seen[...]}.
//   4. fill pass, same work mapping: every output element is written exactly once.  No float atomics; the features
//      are copied as bits, except under a crop.
// Under a crop the surviving views of a point are ordered by ascending image id, stably (from_dense's lexsort).  A
// view's place is the number of surviving views of its point with a smaller (image, source index), counted by its
// lane over the point's (image, count) pairs: staged in LDS for a point of up to SELECT_TILE views, read from the
// source arrays and the vcnt workspace above that.  Two surviving views of one point with the same image are what
// from_dense would unite: the count pass raises the `unsupported` flag and the caller takes the composition.
#include "dva_common.h"
#include "mapping_args.h"
#include "scan.h"

namespace dva {

constexpr int SELECT_TILE = 256;     // views of a point staged in LDS under a crop: 3 KiB
constexpr int SELECT_GRID = 32768;   // blocks of the per-point kernels (grid-stride above)
constexpr int SELECT_MAX_F = 1 << 16;

enum { SF_UNSUPPORTED = 0, SF_RANGE = 1, SF_COUNT = 8 };      // flag words at the start of the workspace

struct SelectLayout {
  int *flags, *seen, *rank, *nviews, *natoms, *vcnt;
  int64_t *view_base, *atom_base, *bsum;
  int64_t total, nb;
};

static inline SelectLayout select_layout(void* ws, int64_t M, int64_t V, int64_t B, bool crop) {
  SelectLayout L;
  L.nb = scan_blocks(M);
  Carver c(ws, 16);
  L.flags = c.take<int>(SF_COUNT);
  L.seen = c.take<int>(B);
  L.rank = c.take<int>(B);
  L.nviews = c.take<int>(M);
  L.natoms = c.take<int>(M);
  L.view_base = c.take<int64_t>(M + 1);
  L.atom_base = c.take<int64_t>(M + 1);
  L.bsum = c.take<int64_t>(L.nb + 1);
  L.vcnt = c.take<int>(crop ? V : 0);
  L.total = (int64_t)c.used();
  return L;
}

struct SelectIn {
  const int64_t* pointers;
  const int64_t* images;
  const int64_t* atom_ptr;
  const uint32_t* pixels;       // int16 (x, y) pairs, x in the low half
  const int64_t* point_idx;     // [M] or null
  const uint8_t* view_mask;     // [V] or null
  const int64_t* image_keys;    // ascending [n_map] or null
  const int64_t* image_map;     // [n_map] or null
  const int64_t* offsets;       // [B, 2] with a crop
  int64_t N, V, P, M, n_map, B, W, H;
  int compact, crop;
};

struct SelectOut {
  int64_t* pointers;
  int64_t* images;
  int64_t* atom_ptr;
  uint32_t* pixels;
  uint32_t* features;
};

// the views [v0, v1) of source point p, inside [0, V] whatever the pointers hold
__device__ __forceinline__ void point_views(const SelectIn& in, int64_t p, int64_t* v0, int64_t* v1) {
  csr_range(in.pointers, p, in.V, v0, v1);
}
__device__ __forceinline__ void view_atoms(const SelectIn& in, int64_t v, int64_t* a0, int64_t* a1) {
  csr_range(in.atom_ptr, v, in.P, a0, a1);
}

// Does view v survive the mask and the image selection?  *id = its new image id (its own image with compact, which
// the fill pass ranks).  An image outside [0, B) with compact is the caller's error: flagged, the view dropped.
__device__ __forceinline__ bool view_kept(const SelectIn& in, int64_t v, int64_t* id, int* flags) {
  if (in.view_mask && !in.view_mask[v]) return false;
  const int64_t img = in.images[v];
  *id = img;
  if (in.image_keys) {
    int64_t lo = 0, hi = in.n_map;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (in.image_keys[mid] < img) lo = mid + 1; else hi = mid;
    }
    if (lo >= in.n_map || in.image_keys[lo] != img) return false;
    *id = in.image_map[lo];
    return *id >= 0;
  }
  if (in.image_map) {
    if (img < 0 || img >= in.n_map) return false;
    *id = in.image_map[img];
    return *id >= 0;
  }
  if (in.compact && (img < 0 || img >= in.B)) {
    flags[SF_RANGE] = 1;
    return false;
  }
  return true;
}

// pixel - offset in int16, as the int16 tensors subtract (wrapping); inside [0, W) x [0, H)?
__device__ __forceinline__ bool crop_pixel(uint32_t px, int16_t ox, int16_t oy, int64_t W, int64_t H, uint32_t* out) {
  const int16_t x = (int16_t)((int)(int16_t)(px & 0xffffu) - (int)ox);
  const int16_t y = (int16_t)((int)(int16_t)(px >> 16) - (int)oy);
  *out = (uint32_t)(uint16_t)x | ((uint32_t)(uint16_t)y << 16);
  return x >= 0 && y >= 0 && (int64_t)x < W && (int64_t)y < H;
}

// ---------------------------------------------------------------------------------------------------------------
// crop: atoms of every source view inside the box
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void select_crop_count_kernel(SelectIn in, int* __restrict__ vcnt,
                                                                 int* __restrict__ seen, int* __restrict__ flags) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < in.V; v += (int64_t)gridDim.x * blockDim.x) {
    int c = 0;
    if (!in.view_mask || in.view_mask[v]) {
      const int64_t img = in.images[v];
      if (img < 0 || img >= in.B) {
        flags[SF_RANGE] = 1;      // an image without a crop offset
      } else {
        seen[img] = 1;
        const int16_t ox = (int16_t)in.offsets[2 * img], oy = (int16_t)in.offsets[2 * img + 1];
        int64_t a0, a1;
        view_atoms(in, v, &a0, &a1);
        for (int64_t a = a0; a < a1; ++a) {
          uint32_t moved;
          c += crop_pixel(in.pixels[a], ox, oy, in.W, in.H, &moved) ? 1 : 0;
        }
      }
    }
    vcnt[v] = c;
  }
}

// The (image, surviving atoms) pairs of the n views of a point from v0 on: the LDS tile for n <= SELECT_TILE, the
// source arrays above (generic pointers, so that one loop serves both).
struct PointViews {
  const long long* img;
  const int* cnt;
};

__device__ __forceinline__ PointViews stage_point(const SelectIn& in, const int* vcnt, int64_t v0, int64_t n,
                                                  long long* timg, int* tcnt, int lane) {
  PointViews pv;
  if (n <= SELECT_TILE) {
    for (int64_t i = lane; i < n; i += DVA_WAVE) {
      timg[i] = in.images[v0 + i];
      tcnt[i] = vcnt[v0 + i];
    }
    wave_sync();
    pv.img = timg;
    pv.cnt = tcnt;
  } else {
    pv.img = (const long long*)in.images + v0;
    pv.cnt = vcnt + v0;
  }
  return pv;
}

// Place of surviving view i among the surviving views of its point in (image, index) order, the atoms in front of
// it, and whether another surviving view has its image.
__device__ __forceinline__ void rank_view(const PointViews& pv, int64_t n, int64_t i, int64_t* pos, int64_t* aoff,
                                          bool* dup) {
  const long long mine = pv.img[i];
  int64_t r = 0, a = 0;
  bool d = false;
  for (int64_t j = 0; j < n; ++j) {
    const int c = pv.cnt[j];
    if (c <= 0 || j == i) continue;
    const long long other = pv.img[j];
    d |= other == mine;
    if (other < mine || (other == mine && j < i)) {
      ++r;
      a += c;
    }
  }
  *pos = r;
  *aoff = a;
  *dup = d;
}

// ---------------------------------------------------------------------------------------------------------------
// count pass
// ---------------------------------------------------------------------------------------------------------------

template <bool CROP>
__global__ __launch_bounds__(DVA_WAVE) void select_count_kernel(SelectIn in, const int* __restrict__ vcnt,
                                                                 int* __restrict__ nviews, int* __restrict__ natoms,
                                                                 int* __restrict__ seen, int* __restrict__ flags) {
  __shared__ long long timg[CROP ? SELECT_TILE : 1];
  __shared__ int tcnt[CROP ? SELECT_TILE : 1];
  const int lane = threadIdx.x;
  for (int64_t m = blockIdx.x; m < in.M; m += gridDim.x) {
    const int64_t p = in.point_idx ? in.point_idx[m] : m;
    long long nv = 0, na = 0;
    if (p < 0 || p >= in.N) {
      if (lane == 0) flags[SF_RANGE] = 1;
    } else {
      int64_t v0, v1;
      point_views(in, p, &v0, &v1);
      if (CROP) {
        const int64_t n = v1 - v0;
        const PointViews pv = stage_point(in, vcnt, v0, n, timg, tcnt, lane);
        for (int64_t i = lane; i < n; i += DVA_WAVE) {
          const int c = pv.cnt[i];
          if (c <= 0) continue;
          int64_t pos, aoff;
          bool dup;
          rank_view(pv, n, i, &pos, &aoff, &dup);
          if (dup) flags[SF_UNSUPPORTED] = 1;
          ++nv;
          na += c;
        }
        wave_sync();      // the tile is reused by the next point
      } else {
        for (int64_t v = v0 + lane; v < v1; v += DVA_WAVE) {
          int64_t id;
          if (!view_kept(in, v, &id, flags)) continue;
          if (in.compact) seen[id] = 1;
          int64_t a0, a1;
          view_atoms(in, v, &a0, &a1);
          ++nv;
          na += a1 - a0;
        }
      }
      nv = wave_sum(nv);
      na = wave_sum(na);
    }
    if (lane == 0) {
      nviews[m] = (int)nv;
      natoms[m] = (int)na;
    }
  }
}

// Ranks of the seen images, the seen list and the sizes: sizes = {V', P', distinct images, flags, seen[...]}.
// flags: bit 0 unsupported (images to unite, or 2^31 or more views or atoms), bit 1 an index out of range, bit 2 a
// repeated image key.
__global__ __launch_bounds__(SCAN_THREADS) void select_sizes_kernel(const int* __restrict__ seen, int64_t B,
                                                                     int* __restrict__ rank,
                                                                     const int64_t* __restrict__ image_keys,
                                                                     int64_t n_keys, const int* __restrict__ flags,
                                                                     const int64_t* __restrict__ view_base,
                                                                     const int64_t* __restrict__ atom_base, int64_t M,
                                                                     int64_t* __restrict__ sizes) {
  __shared__ int wsum[SCAN_THREADS / DVA_WAVE];
  __shared__ int repeated;
  if (threadIdx.x == 0) repeated = 0;
  __syncthreads();
  if (image_keys)
    for (int64_t k = threadIdx.x; k + 1 < n_keys; k += SCAN_THREADS)
      if (image_keys[k] == image_keys[k + 1]) repeated = 1;
  int carry = 0;
  for (int64_t c0 = 0; c0 < B; c0 += SCAN_THREADS) {
    const int64_t i = c0 + threadIdx.x;
    const int s = i < B && seen[i] != 0 ? 1 : 0;
    int total;
    const int excl = block_excl_scan<int>(s, &total, wsum);
    if (i < B) rank[i] = carry + excl;
    if (s) sizes[4 + carry + excl] = i;
    carry += total;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t Vp = view_base[M], Pp = atom_base[M];
    int64_t f = 0;
    if (flags[SF_UNSUPPORTED] || Vp >= I31_LIMIT || Pp >= I31_LIMIT) f |= 1;
    if (flags[SF_RANGE]) f |= 2;
    if (repeated) f |= 4;
    sizes[0] = Vp;
    sizes[1] = Pp;
    sizes[2] = carry;
    sizes[3] = f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// fill pass
// ---------------------------------------------------------------------------------------------------------------

template <bool CROP>
__global__ __launch_bounds__(DVA_WAVE) void select_fill_kernel(SelectIn in, const int* __restrict__ vcnt,
                                                                const int* __restrict__ rank,
                                                                const int64_t* __restrict__ view_base,
                                                                const int64_t* __restrict__ atom_base,
                                                                const uint32_t* __restrict__ feat, int F, SelectOut out,
                                                                int64_t Vp, int64_t Pp) {
  __shared__ long long timg[CROP ? SELECT_TILE : 1];
  __shared__ int tcnt[CROP ? SELECT_TILE : 1];
  __shared__ int unused_flags[SF_COUNT];      // view_kept flags what the count pass has flagged already
  const int lane = threadIdx.x;
  for (int64_t m = blockIdx.x; m < in.M; m += gridDim.x) {
    const int64_t vb = view_base[m], ab = atom_base[m];
    if (lane == 0) {
      out.pointers[m] = vb;
      if (m == in.M - 1) {
        out.pointers[in.M] = Vp;
        out.atom_ptr[Vp] = Pp;
      }
    }
    const int64_t p = in.point_idx ? in.point_idx[m] : m;
    if (p < 0 || p >= in.N) continue;
    int64_t v0, v1;
    point_views(in, p, &v0, &v1);
    if (CROP) {
      const int64_t n = v1 - v0;
      const PointViews pv = stage_point(in, vcnt, v0, n, timg, tcnt, lane);
      for (int64_t i = lane; i < n; i += DVA_WAVE) {
        const int c = pv.cnt[i];
        if (c <= 0) continue;
        int64_t pos, aoff;
        bool dup;
        rank_view(pv, n, i, &pos, &aoff, &dup);
        const int64_t o = vb + pos, v = v0 + i, img = pv.img[i];
        int64_t w = ab + aoff;
        if (o >= Vp || w + c > Pp) continue;      // the inputs changed between the passes: write nothing outside
        out.images[o] = img;
        out.atom_ptr[o] = w;
        if (feat) {
          // the mean of c copies of the value, added one after the other: what the per-view mean of the rows
          // expanded to atoms computes
          for (int f = 0; f < F; ++f) {
            const float x = __uint_as_float(feat[v * F + f]);
            float acc = 0.f;
            for (int t = 0; t < c; ++t) acc += x;
            acc /= (float)c;
            out.features[o * F + f] = __float_as_uint(acc);
          }
        }
        const int16_t ox = (int16_t)in.offsets[2 * img], oy = (int16_t)in.offsets[2 * img + 1];
        int64_t a0, a1;
        view_atoms(in, v, &a0, &a1);
        for (int64_t a = a0; a < a1; ++a) {
          uint32_t moved;
          if (crop_pixel(in.pixels[a], ox, oy, in.W, in.H, &moved) && w < Pp) out.pixels[w++] = moved;
        }
      }
      wave_sync();      // the tile is reused by the next point
    } else {
      int64_t nv = 0, abase = 0;
      const u64 below = lanes_below(lane);
      for (int64_t c0 = v0; c0 < v1; c0 += DVA_WAVE) {
        const int64_t v = c0 + lane;
        int64_t id = 0, a0 = 0, a1 = 0;
        bool keep = false;
        if (v < v1) keep = view_kept(in, v, &id, unused_flags);
        if (keep) view_atoms(in, v, &a0, &a1);
        const long long cnt = a1 - a0;
        const u64 mask = __ballot(keep);
        const long long incl = wave_incl_scan(cnt, lane);
        const int64_t o = vb + nv + __popcll(mask & below);
        const int64_t w = ab + abase + incl - cnt;
        if (keep && o < Vp && w + cnt <= Pp) {
          out.images[o] = in.compact ? (int64_t)rank[id] : id;
          out.atom_ptr[o] = w;
          if (feat)
            for (int f = 0; f < F; ++f) out.features[o * F + f] = feat[v * F + f];
          for (long long a = 0; a < cnt; ++a) out.pixels[w + a] = in.pixels[a0 + a];
        }
        nv += __popcll(mask);
        abase += __shfl(incl, DVA_WAVE - 1, DVA_WAVE);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// per-image statistics
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void image_stats_init_kernel(long long* __restrict__ stats, int64_t B) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 5 * B; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / B;
    stats[i] = row == 0 ? 0 : ((row == 1 || row == 3) ? 0x7fffffffffffffffLL : (-0x7fffffffffffffffLL - 1));
  }
}

__global__ __launch_bounds__(256) void image_stats_kernel(const int64_t* __restrict__ images,
                                                           const int64_t* __restrict__ atom_ptr,
                                                           const uint32_t* __restrict__ pixels, int64_t V, int64_t P,
                                                           int64_t B, long long* __restrict__ stats) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t img = images[v];
    if (img < 0 || img >= B) continue;
    int64_t a0, a1;
    csr_range(atom_ptr, v, P, &a0, &a1);
    if (a1 == a0) continue;
    long long x0 = 32767, x1 = -32768, y0 = 32767, y1 = -32768;
    for (int64_t a = a0; a < a1; ++a) {
      const uint32_t px = pixels[a];
      const long long x = (int16_t)(px & 0xffffu), y = (int16_t)(px >> 16);
      x0 = min(x0, x);
      x1 = max(x1, x);
      y0 = min(y0, y);
      y1 = max(y1, y);
    }
    // integer atomics: the result does not depend on their order
    atomicAdd((u64*)&stats[img], (u64)(a1 - a0));
    __hip_atomic_fetch_min(&stats[B + img], x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&stats[2 * B + img], x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(&stats[3 * B + img], y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&stats[4 * B + img], y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

static inline int select_check_sizes(int64_t N, int64_t V, int64_t P, int64_t M, int64_t B) {
  if (N < 1 || M < 1 || any_negative({V, P, B})) return DVA_ERR_INVALID;
  return fits_i31({N, V, P, M, B});
}

// the checks the two entries share; fills `in`
static int select_arguments(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                            const void* pixels, int32_t pixel_bytes, int64_t n_points, int64_t n_views,
                            int64_t n_atoms, const int64_t* point_idx, int64_t n_out, const uint8_t* view_mask,
                            const int64_t* image_keys, const int64_t* image_map, int64_t n_map, int32_t compact,
                            int64_t n_images, int64_t crop_w, int64_t crop_h, const int64_t* crop_offsets,
                            const void* workspace, SelectIn* in) {
  int rc = select_check_sizes(n_points, n_views, n_atoms, n_out, n_images);
  if (rc != DVA_OK) return rc;
  if ((rc = pixel_bytes_code(pixel_bytes)) != DVA_OK) return rc;
  if (!pointers || !workspace || ((uintptr_t)workspace & 15)) return DVA_ERR_INVALID;
  if (!mapping_arrays_ok(images, atom_ptr, pixels, n_views, n_atoms)) return DVA_ERR_INVALID;
  if (!point_idx && n_out != n_points) return DVA_ERR_INVALID;
  if (n_map < 0 || (image_keys && !image_map) || (image_map && compact) || (!image_map && n_map != 0))
    return DVA_ERR_INVALID;
  if (crop_offsets && (compact || image_map || crop_w < 1 || crop_h < 1)) return DVA_ERR_INVALID;
  if (!compact && !crop_offsets && n_images != 0) return DVA_ERR_INVALID;
  *in = SelectIn{pointers, images, atom_ptr, (const uint32_t*)pixels, point_idx, view_mask, image_keys, image_map,
                 crop_offsets, n_points, n_views, n_atoms, n_out, n_map, n_images, crop_w, crop_h, compact ? 1 : 0,
                 crop_offsets ? 1 : 0};
  return DVA_OK;
}

}  // namespace dva

using namespace dva;

extern "C" {

int dva_mapping_select_tile_views(void) { return SELECT_TILE; }

int64_t dva_mapping_select_workspace_bytes(int64_t n_out, int64_t n_views, int64_t n_images, int32_t crop) {
  const int rc = select_check_sizes(1, n_views, 0, n_out, n_images);
  if (rc != DVA_OK) return rc;
  return select_layout(nullptr, n_out, n_views, n_images, crop != 0).total;
}

int dva_mapping_select_count(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                             const void* pixels, int32_t pixel_bytes, int64_t n_points, int64_t n_views,
                             int64_t n_atoms, const int64_t* point_idx, int64_t n_out, const uint8_t* view_mask,
                             const int64_t* image_keys, const int64_t* image_map, int64_t n_map, int32_t compact,
                             int64_t n_images, int64_t crop_w, int64_t crop_h, const int64_t* crop_offsets,
                             int64_t* sizes, void* workspace, int64_t workspace_bytes, void* stream) {
  SelectIn in;
  const int rc = select_arguments(pointers, images, atom_ptr, pixels, pixel_bytes, n_points, n_views, n_atoms,
                                  point_idx, n_out, view_mask, image_keys, image_map, n_map, compact, n_images, crop_w,
                                  crop_h, crop_offsets, workspace, &in);
  if (rc != DVA_OK) return rc;
  if (!sizes) return DVA_ERR_INVALID;
  const SelectLayout L = select_layout(workspace, in.M, in.V, in.B, in.crop);
  if (workspace_bytes < L.total) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  // flags and seen are adjacent
  if (hipMemsetAsync(L.flags, 0, (size_t)((char*)L.rank - (char*)L.flags), s) != hipSuccess) return DVA_ERR_LAUNCH;
  const dim3 grid(capped_grid(in.M, 1, SELECT_GRID));
  if (in.crop) {
    hipLaunchKernelGGL(select_crop_count_kernel, dim3(capped_grid(in.V, 256, 4096)), dim3(256), 0, s, in, L.vcnt,
                       L.seen, L.flags);
    hipLaunchKernelGGL(select_count_kernel<true>, grid, dim3(DVA_WAVE), 0, s, in, (const int*)L.vcnt, L.nviews,
                       L.natoms, L.seen, L.flags);
  } else {
    hipLaunchKernelGGL(select_count_kernel<false>, grid, dim3(DVA_WAVE), 0, s, in, (const int*)nullptr, L.nviews,
                       L.natoms, L.seen, L.flags);
  }
  launch_scan<int64_t>(L.nviews, in.M, L.bsum, L.nb, L.view_base, s);
  launch_scan<int64_t>(L.natoms, in.M, L.bsum, L.nb, L.atom_base, s);
  hipLaunchKernelGGL(select_sizes_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)L.seen, in.B, L.rank,
                     image_keys, n_map, (const int*)L.flags, (const int64_t*)L.view_base,
                     (const int64_t*)L.atom_base, in.M, sizes);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_mapping_select_fill(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                            const void* pixels, int32_t pixel_bytes, const float* features, int32_t F,
                            int64_t n_points, int64_t n_views, int64_t n_atoms, const int64_t* point_idx,
                            int64_t n_out, const uint8_t* view_mask, const int64_t* image_keys,
                            const int64_t* image_map, int64_t n_map, int32_t compact, int64_t n_images, int64_t crop_w,
                            int64_t crop_h, const int64_t* crop_offsets, int64_t n_views_out, int64_t n_atoms_out,
                            int64_t* out_pointers, int64_t* out_images, int64_t* out_atom_ptr, void* out_pixels,
                            float* out_features, void* workspace, int64_t workspace_bytes, void* stream) {
  SelectIn in;
  const int rc = select_arguments(pointers, images, atom_ptr, pixels, pixel_bytes, n_points, n_views, n_atoms,
                                  point_idx, n_out, view_mask, image_keys, image_map, n_map, compact, n_images, crop_w,
                                  crop_h, crop_offsets, workspace, &in);
  if (rc != DVA_OK) return rc;
  if (any_negative({n_views_out, n_atoms_out, F})) return DVA_ERR_INVALID;
  if (fits_i31({n_views_out, n_atoms_out}) != DVA_OK || F > SELECT_MAX_F) return DVA_ERR_UNSUPPORTED;
  if (!out_pointers || !out_atom_ptr) return DVA_ERR_INVALID;
  if ((n_views_out > 0 && !out_images) || (n_atoms_out > 0 && !out_pixels)) return DVA_ERR_INVALID;
  if ((!features && out_features) || (features && (F < 1 || (n_views_out > 0 && !out_features)))) return DVA_ERR_INVALID;
  if ((uintptr_t)out_pixels & 3) return DVA_ERR_INVALID;
  const SelectLayout L = select_layout(workspace, in.M, in.V, in.B, in.crop);
  if (workspace_bytes < L.total) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const SelectOut out = {out_pointers, out_images, out_atom_ptr, (uint32_t*)out_pixels, (uint32_t*)out_features};
  const dim3 grid(capped_grid(in.M, 1, SELECT_GRID));
  if (in.crop)
    hipLaunchKernelGGL(select_fill_kernel<true>, grid, dim3(DVA_WAVE), 0, s, in, (const int*)L.vcnt,
                       (const int*)L.rank, (const int64_t*)L.view_base, (const int64_t*)L.atom_base,
                       (const uint32_t*)features, (int)F, out, n_views_out, n_atoms_out);
  else
    hipLaunchKernelGGL(select_fill_kernel<false>, grid, dim3(DVA_WAVE), 0, s, in, (const int*)nullptr,
                       (const int*)L.rank, (const int64_t*)L.view_base, (const int64_t*)L.atom_base,
                       (const uint32_t*)features, (int)F, out, n_views_out, n_atoms_out);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_mapping_image_stats(const int64_t* images, const int64_t* atom_ptr, const void* pixels, int32_t pixel_bytes,
                            int64_t n_views, int64_t n_atoms, int64_t n_images, int64_t* stats, void* stream) {
  if (any_negative({n_views, n_atoms, n_images})) return DVA_ERR_INVALID;
  int rc = fits_i31({n_views, n_atoms, n_images});
  if (rc == DVA_OK) rc = pixel_bytes_code(pixel_bytes);
  if (rc != DVA_OK) return rc;
  if (n_images == 0) return DVA_OK;
  if (!stats || !mapping_arrays_ok(images, atom_ptr, pixels, n_views, n_atoms)) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(image_stats_init_kernel, dim3(capped_grid(5 * n_images, 256, 4096)), dim3(256), 0, s,
                     (long long*)stats, n_images);
  if (n_views > 0)
    hipLaunchKernelGGL(image_stats_kernel, dim3(capped_grid(n_views, 256, 4096)), dim3(256), 0, s, images, atom_ptr,
                       (const uint32_t*)pixels, n_views, n_atoms, n_images, (long long*)stats);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
