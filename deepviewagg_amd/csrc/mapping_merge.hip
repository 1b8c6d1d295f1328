// Mapping merge after a strided 3D convolution (reference core/multimodal/image.py:2211-2273
// `select_points(mode='merge')` followed by `from_dense`, :1728-1795): point i becomes voxel idx[i]; the views of
// the points of a voxel are united per image, duplicate pixels of a merged view removed, the features of a merged
// view are the mean over its source views.
//
// The reference expands the mapping to atom rows and sorts all of them globally (lexargunique, then from_dense).
// Here a voxel is one unit of work:
//   1. histogram of the voxel ids (which is also the coverage check "every id in [0, M) has a point") + exclusive
//      scan + scatter: the members of every voxel.  The scatter is not stable and need not be: the atoms of a
//      voxel are a set, and the source views of a merged view are ordered by their own index below.
//   2. count pass, one wavefront per voxel: the atoms of the members are staged in LDS as 64-bit keys
//      image << 32 | x << 16 | y, sorted by a bitonic network, and the distinct keys / distinct images counted.
//   3. two scans give the first view and the first atom of every voxel; one kernel writes (M, V', P', ok) for the
//      single host readback that sizes the outputs.
//   4. fill pass: the same sort again, then every output element is written exactly once.  Features: the source
//      views are sorted by image << 32 | view index (ascending view index == ascending point index, the points
//      own contiguous view ranges), and one lane per (merged view, channel) adds them in that order in fp32 and
//      divides by their number -- no float atomics, the same bits on every call.
// A voxel with more than MERGE_TILE atoms takes the second route: its keys live in the workspace (a bump
// allocation of at most P atom keys and V view keys in total), a 1024-thread block sorts them there in the count
// pass and the fill pass reads the sorted keys back.
//
// Image ids are < 2^31 and pixels are non-negative int16 (the key packing); a view without atoms contributes
// nothing (the reference drops it when it expands to atom rows).
#include "dva_common.h"
#include "mapping_args.h"
#include "scan.h"

namespace dva {

constexpr int MERGE_TILE = 512;      // atoms of a voxel staged in LDS: 2 x 4 KiB of keys per wavefront
constexpr int MERGE_GRID = 32768;    // blocks of the per-voxel kernels (grid-stride above)
constexpr int BIG_THREADS = 1024;
constexpr int BIG_GRID = 256;
constexpr int MERGE_MAX_F = 1 << 16;

// counters at the start of the workspace
enum { C_BAD = 0, C_M = 1, C_NBIG = 2, C_AUSED = 3, C_VUSED = 4, C_COUNT = 8 };

struct MergeLayout {
  u64 *ctr, *scratch_a, *scratch_v;
  int *hist, *voxel_ptr, *members, *nviews, *natoms, *view_base, *atom_base, *bsum, *big_j, *big_na, *big_nv;
  int64_t *big_aoff, *big_voff;
  int64_t total, bigcap, nb;
};

static inline MergeLayout merge_layout(void* ws, int64_t N, int64_t V, int64_t P) {
  MergeLayout L;
  L.nb = (N + SCAN_BLOCK - 1) / SCAN_BLOCK;
  L.bigcap = P / (MERGE_TILE + 1) + 1;
  Carver c(ws, 16);
  L.ctr = c.take<u64>(C_COUNT);
  L.hist = c.take<int>(N);
  L.voxel_ptr = c.take<int>(N + 1);
  L.members = c.take<int>(N);
  L.nviews = c.take<int>(N);
  L.natoms = c.take<int>(N);
  L.view_base = c.take<int>(N + 1);
  L.atom_base = c.take<int>(N + 1);
  L.bsum = c.take<int>(L.nb + 1);
  L.big_j = c.take<int>(L.bigcap);
  L.big_na = c.take<int>(L.bigcap);
  L.big_nv = c.take<int>(L.bigcap);
  L.big_aoff = c.take<int64_t>(L.bigcap);
  L.big_voff = c.take<int64_t>(L.bigcap);
  L.scratch_a = c.take<u64>(P);
  L.scratch_v = c.take<u64>(V);
  L.total = (int64_t)c.used();
  return L;
}

// ---------------------------------------------------------------------------------------------------------------
// wavefront helpers
// ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, DVA_WAVE));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------
// members of every voxel
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void merge_hist_kernel(const int64_t* __restrict__ idx, int64_t N,
                                                          int* __restrict__ hist, u64* __restrict__ ctr) {
  int top = 0;
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = idx[i];
    if (id < 0 || id >= N) {
      bad = true;     // more voxels than points: some id below the maximum has no point
    } else {
      atomicAdd(&hist[id], 1);
      top = max(top, (int)id + 1);
    }
  }
  top = wave_max(top);
  const bool any_bad = __ballot(bad) != 0;
  if ((threadIdx.x & (DVA_WAVE - 1)) == 0) {
    if (top > 0) atomicMax(&ctr[C_M], (u64)top);
    if (any_bad) atomicMax(&ctr[C_BAD], 1ull);
  }
}

__global__ __launch_bounds__(256) void merge_scatter_kernel(const int64_t* __restrict__ idx, int64_t N,
                                                             int* __restrict__ hist,
                                                             const int* __restrict__ voxel_ptr,
                                                             int* __restrict__ members) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = idx[i];
    if (id < 0 || id >= N) continue;
    const int slot = atomicSub(&hist[id], 1) - 1;      // in [0, count of id)
    members[voxel_ptr[id] + slot] = (int)i;
  }
}

// the exclusive scans (n int32, totals < 2^31) are launch_scan<int> of scan.h

// ---------------------------------------------------------------------------------------------------------------
// per-voxel work.  The staging and the passes over the sorted keys are run by ONE wavefront (lane = 0 .. 63); the
// sort by `nt` threads.  I = int for the LDS tile, int64_t for keys in the workspace.
// ---------------------------------------------------------------------------------------------------------------

struct MergeIn {
  const int64_t* pointers;
  const int64_t* images;
  const int64_t* atom_ptr;
  const uint32_t* pixels;     // int16 (x, y) pairs
  const int* voxel_ptr;
  const int* members;
};

// View keys image << 32 | view of the views (with at least one atom) of the members of voxel j, the first `cap` of
// them written to vkey; *na = the atoms of all of them.  Returns their number.
template <typename I>
__device__ __forceinline__ I stage_views(const MergeIn& in, int64_t j, u64* vkey, I cap, int lane, long long* na) {
  const int m0 = in.voxel_ptr[j], m1 = in.voxel_ptr[j + 1];
  I nv = 0;
  long long atoms = 0;
  for (int m = m0; m < m1; ++m) {
    const int i = in.members[m];
    const int64_t v0 = in.pointers[i], v1 = in.pointers[i + 1];
    for (int64_t vb = v0; vb < v1; vb += DVA_WAVE) {
      const int64_t v = vb + lane;
      long long cnt = 0;
      if (v < v1) cnt = in.atom_ptr[v + 1] - in.atom_ptr[v];
      const bool keep = cnt > 0;
      const u64 mask = __ballot(keep);
      if (keep) {
        const I pos = nv + (I)__popcll(mask & lanes_below(lane));
        if (pos < cap) vkey[pos] = ((u64)in.images[v] << 32) | (u64)(uint32_t)v;
        atoms += cnt;
      }
      nv += (I)__popcll(mask);
    }
  }
  *na = wave_sum(atoms);
  return nv;
}

// Atom keys image << 32 | x << 16 | y of the staged views, at most `cap` of them written.
template <typename I>
__device__ __forceinline__ void stage_atoms(const MergeIn& in, const u64* vkey, I nv, u64* akey, I cap, int lane) {
  long long base = 0;
  for (I t0 = 0; t0 < nv; t0 += DVA_WAVE) {
    const I t = t0 + lane;
    u64 key = 0;
    int64_t a0 = 0;
    long long cnt = 0;
    if (t < nv) {
      key = vkey[t];
      const int64_t v = (int64_t)(uint32_t)key;
      a0 = in.atom_ptr[v];
      cnt = in.atom_ptr[v + 1] - a0;
    }
    const long long incl = wave_incl_scan(cnt, lane);
    const long long off = base + incl - cnt;
    const u64 hi = key & 0xffffffff00000000ull;
    for (long long c = 0; c < cnt; ++c) {
      if (off + c < (long long)cap) {
        const uint32_t px = in.pixels[a0 + c];      // x in the low half, y in the high half
        akey[off + c] = hi | ((u64)(px & 0xffffu) << 16) | (u64)(px >> 16);
      }
    }
    base += __shfl(incl, DVA_WAVE - 1, DVA_WAVE);
  }
}

__device__ __forceinline__ void compare_exchange(u64* a, int64_t i, int64_t l) {
  const u64 x = a[i], y = a[l];
  if (x > y) {
    a[i] = y;
    a[l] = x;
  }
}

// Ascending bitonic sort of a[0 .. n) for any n: the network in which every comparator puts the smaller key at the
// lower index (a flip stage, then half-cleaners), so that the keys an index >= n would hold act as +infinity and
// their comparators are no-ops that can be left out.
template <typename I, bool BLOCK>
__device__ __forceinline__ void bitonic_sort(u64* a, I n, int tid, int nt) {
  if (n < 2) return;
  int lg = 1;
  while (((int64_t)1 << lg) < (int64_t)n) ++lg;
  const I half = (I)((int64_t)1 << (lg - 1));
  for (int lk = 1; lk <= lg; ++lk) {
    {   // flip: i and its mirror within the block of 2^lk
      const int lh = lk - 1;
      for (I p = tid; p < half; p += nt) {
        const I b = p >> lh, t = p - (b << lh);
        const I i = (b << lk) + t, l = (b << lk) + (((I)1 << lk) - 1 - t);
        if (l < n) compare_exchange(a, i, l);
      }
      if (BLOCK) __syncthreads(); else wave_sync();
    }
    for (int lj = lk - 2; lj >= 0; --lj) {
      for (I p = tid; p < half; p += nt) {
        const I b = p >> lj, t = p - (b << lj);
        const I i = (b << (lj + 1)) + t, l = i + ((I)1 << lj);
        if (l < n) compare_exchange(a, i, l);
      }
      if (BLOCK) __syncthreads(); else wave_sync();
    }
  }
}

struct MergeOut {
  int64_t* pointers;
  int64_t* images;
  int64_t* atom_ptr;
  uint32_t* pixels;
  float* features;
};

// One pass over the sorted atom keys: counts the distinct keys (*natoms) and the distinct images (return value);
// FILL writes the pixels of the distinct keys from atom `ab` on, and the image and first atom of the merged views
// from view `vb` on.
template <typename I, bool FILL>
__device__ __forceinline__ I atoms_pass(const u64* akey, I na, int lane, I* natoms, const MergeOut& out, int64_t vb,
                                        int64_t ab) {
  I r = 0, q = 0;
  const u64 below = lanes_below(lane);
  for (I i0 = 0; i0 < na; i0 += DVA_WAVE) {
    const I i = i0 + lane;
    const bool ok = i < na;
    const u64 key = ok ? akey[i] : 0;
    const u64 prev = (ok && i > 0) ? akey[i - 1] : ~key;
    const bool head = ok && key != prev;
    const bool ihead = ok && (key >> 32) != (prev >> 32);
    const u64 hm = __ballot(head), im = __ballot(ihead);
    if (FILL) {
      const I rr = r + (I)__popcll(hm & below);
      if (head) out.pixels[ab + rr] = (uint32_t)((key >> 16) & 0xffffu) | ((uint32_t)(key & 0xffffu) << 16);
      if (ihead) {
        const I qq = q + (I)__popcll(im & below);
        out.images[vb + qq] = (int64_t)(key >> 32);
        out.atom_ptr[vb + qq] = ab + rr;
      }
    }
    r += (I)__popcll(hm);
    q += (I)__popcll(im);
  }
  *natoms = r;
  return q;
}

// Sorted view keys image << 32 | view  ->  (rank of the image among the voxel's images) << 32 | view.
template <typename I>
__device__ __forceinline__ void rank_views(u64* vkey, I nv, int lane) {
  I q = 0;
  uint32_t carry = 0;     // image of the last key of the previous chunk
  const u64 upto = lanes_below(lane) | (1ull << lane);
  for (I i0 = 0; i0 < nv; i0 += DVA_WAVE) {
    const I i = i0 + lane;
    const bool ok = i < nv;
    const u64 key = ok ? vkey[i] : 0;
    const uint32_t img = (uint32_t)(key >> 32);
    uint32_t prev = ok && lane > 0 ? (uint32_t)(vkey[i - 1] >> 32) : carry;
    const bool ihead = ok && (i == 0 || img != prev);
    const u64 im = __ballot(ihead);
    carry = (uint32_t)__shfl((int)img, DVA_WAVE - 1, DVA_WAVE);
    wave_sync();      // every lane has read its neighbour
    if (ok) vkey[i] = ((u64)(uint32_t)(q + (I)__popcll(im & upto) - 1) << 32) | (key & 0xffffffffull);
    q += (I)__popcll(im);
    wave_sync();
  }
}

// features of the merged views: item (first key of a rank, channel) adds the rows of the rank in key order
template <typename I>
__device__ __forceinline__ void mean_features(const u64* vkey, I nv, const float* __restrict__ feat, int F,
                                              float* __restrict__ out, int64_t vb, int tid, int nt) {
  const I items = nv * (I)F;
  for (I e = tid; e < items; e += nt) {
    const I i = e / (I)F;
    const int f = (int)(e - i * (I)F);
    const u64 key = vkey[i];
    const uint32_t q = (uint32_t)(key >> 32);
    if (i > 0 && (uint32_t)(vkey[i - 1] >> 32) == q) continue;
    float s = feat[(int64_t)(uint32_t)key * F + f];
    int c = 1;
    for (I t = i + 1; t < nv; ++t) {
      const u64 k2 = vkey[t];
      if ((uint32_t)(k2 >> 32) != q) break;
      s = s + feat[(int64_t)(uint32_t)k2 * F + f];
      ++c;
    }
    out[(vb + q) * F + f] = s / (float)c;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// count pass
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(DVA_WAVE) void merge_count_small_kernel(MergeIn in, int64_t N, u64* __restrict__ ctr,
                                                                      int* __restrict__ nviews,
                                                                      int* __restrict__ natoms,
                                                                      int* __restrict__ big_j,
                                                                      int* __restrict__ big_na,
                                                                      int* __restrict__ big_nv, int64_t bigcap) {
  __shared__ u64 vkey[MERGE_TILE];
  __shared__ u64 akey[MERGE_TILE];
  const int lane = threadIdx.x;
  const int64_t M = min((int64_t)ctr[C_M], N);
  const MergeOut none = {};
  for (int64_t j = blockIdx.x; j < N; j += gridDim.x) {
    int nv_out = 0, na_out = 0;
    if (j < M) {
      if (in.voxel_ptr[j + 1] == in.voxel_ptr[j]) {
        if (lane == 0) atomicMax(&ctr[C_BAD], 1ull);      // an id below the maximum without a point
      } else {
        long long na;
        const int nv = stage_views<int>(in, j, vkey, MERGE_TILE, lane, &na);
        if (na > MERGE_TILE) {
          if (lane == 0) {
            const u64 k = atomicAdd(&ctr[C_NBIG], 1ull);
            if ((int64_t)k < bigcap) {
              big_j[k] = (int)j;
              big_na[k] = (int)na;
              big_nv[k] = nv;
            }
          }
        } else {
          wave_sync();
          stage_atoms<int>(in, vkey, nv, akey, MERGE_TILE, lane);
          wave_sync();
          bitonic_sort<int, false>(akey, (int)na, lane, DVA_WAVE);
          nv_out = atoms_pass<int, false>(akey, (int)na, lane, &na_out, none, 0, 0);
          wave_sync();      // the tiles are reused by the next voxel
        }
      }
    }
    if (lane == 0) {
      nviews[j] = nv_out;
      natoms[j] = na_out;
    }
  }
}

__global__ __launch_bounds__(BIG_THREADS) void merge_count_big_kernel(MergeIn in, u64* __restrict__ ctr,
                                                                       int* __restrict__ nviews,
                                                                       int* __restrict__ natoms,
                                                                       const int* __restrict__ big_j,
                                                                       int* __restrict__ big_na,
                                                                       const int* __restrict__ big_nv,
                                                                       int64_t* __restrict__ big_aoff,
                                                                       int64_t* __restrict__ big_voff,
                                                                       int64_t bigcap, u64* __restrict__ scratch_a,
                                                                       u64* __restrict__ scratch_v, int64_t P,
                                                                       int64_t V) {
  __shared__ int64_t s_aoff, s_voff;
  const int64_t nbig = min((int64_t)ctr[C_NBIG], bigcap);
  const int tid = threadIdx.x;
  const MergeOut none = {};
  for (int64_t k = blockIdx.x; k < nbig; k += gridDim.x) {
    const int64_t j = big_j[k];
    const int64_t na = big_na[k], nv = big_nv[k];
    __syncthreads();      // s_aoff / s_voff of the previous entry have been read
    if (tid == 0) {
      int64_t aoff = (int64_t)atomicAdd(&ctr[C_AUSED], (u64)na);
      int64_t voff = (int64_t)atomicAdd(&ctr[C_VUSED], (u64)nv);
      if (aoff + na > P || voff + nv > V) {      // pointers that are no CSR: refuse the call, touch nothing
        atomicMax(&ctr[C_BAD], 1ull);
        aoff = voff = -1;
      }
      big_aoff[k] = aoff;
      big_voff[k] = voff;
      s_aoff = aoff;
      s_voff = voff;
    }
    __syncthreads();
    const int64_t aoff = s_aoff, voff = s_voff;
    if (aoff < 0) {
      if (tid == 0) big_na[k] = 0;
      continue;
    }
    u64* akey = scratch_a + aoff;
    u64* vkey = scratch_v + voff;
    if (tid < DVA_WAVE) {
      long long na2;
      stage_views<int64_t>(in, j, vkey, nv, tid, &na2);
      wave_sync();
      stage_atoms<int64_t>(in, vkey, nv, akey, na, tid);
    }
    __syncthreads();
    bitonic_sort<int64_t, true>(akey, na, tid, BIG_THREADS);
    if (tid < DVA_WAVE) {
      int64_t r;
      const int64_t q = atoms_pass<int64_t, false>(akey, na, tid, &r, none, 0, 0);
      if (tid == 0) {
        nviews[j] = (int)q;
        natoms[j] = (int)r;
      }
    }
  }
}

__global__ void merge_sizes_kernel(const u64* __restrict__ ctr, const int* __restrict__ view_base,
                                   const int* __restrict__ atom_base, int64_t N, int64_t* __restrict__ sizes) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sizes[0] = (int64_t)ctr[C_M];
    sizes[1] = view_base[N];
    sizes[2] = atom_base[N];
    sizes[3] = ctr[C_BAD] == 0 ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// fill pass
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(DVA_WAVE) void merge_fill_small_kernel(MergeIn in, const float* __restrict__ feat,
                                                                     int F, int64_t M,
                                                                     const int* __restrict__ view_base,
                                                                     const int* __restrict__ atom_base,
                                                                     MergeOut out, int64_t Vp, int64_t Pp) {
  __shared__ u64 vkey[MERGE_TILE];
  __shared__ u64 akey[MERGE_TILE];
  const int lane = threadIdx.x;
  for (int64_t j = blockIdx.x; j < M; j += gridDim.x) {
    const int64_t vb = view_base[j], ab = atom_base[j];
    if (lane == 0) {
      out.pointers[j] = vb;
      if (j == M - 1) {
        out.pointers[M] = Vp;
        out.atom_ptr[Vp] = Pp;
      }
    }
    long long na;
    const int nv = stage_views<int>(in, j, vkey, MERGE_TILE, lane, &na);
    if (na > MERGE_TILE || na == 0) continue;
    wave_sync();
    stage_atoms<int>(in, vkey, nv, akey, MERGE_TILE, lane);
    wave_sync();
    bitonic_sort<int, false>(akey, (int)na, lane, DVA_WAVE);
    int r;
    atoms_pass<int, true>(akey, (int)na, lane, &r, out, vb, ab);
    if (feat) {
      bitonic_sort<int, false>(vkey, nv, lane, DVA_WAVE);
      rank_views<int>(vkey, nv, lane);
      mean_features<int>(vkey, nv, feat, F, out.features, vb, lane, DVA_WAVE);
    }
    wave_sync();
  }
}

__global__ __launch_bounds__(BIG_THREADS) void merge_fill_big_kernel(const u64* __restrict__ ctr,
                                                                      const float* __restrict__ feat, int F,
                                                                      const int* __restrict__ view_base,
                                                                      const int* __restrict__ atom_base,
                                                                      const int* __restrict__ big_j,
                                                                      const int* __restrict__ big_na,
                                                                      const int* __restrict__ big_nv,
                                                                      const int64_t* __restrict__ big_aoff,
                                                                      const int64_t* __restrict__ big_voff,
                                                                      int64_t bigcap, u64* __restrict__ scratch_a,
                                                                      u64* __restrict__ scratch_v, MergeOut out) {
  const int64_t nbig = min((int64_t)ctr[C_NBIG], bigcap);
  const int tid = threadIdx.x;
  for (int64_t k = blockIdx.x; k < nbig; k += gridDim.x) {
    const int64_t j = big_j[k];
    const int64_t na = big_na[k], nv = big_nv[k];
    const int64_t aoff = big_aoff[k], voff = big_voff[k];
    if (aoff < 0 || na == 0) continue;
    const int64_t vb = view_base[j], ab = atom_base[j];
    u64* vkey = scratch_v + voff;
    if (tid < DVA_WAVE) {
      int64_t r;
      atoms_pass<int64_t, true>(scratch_a + aoff, na, tid, &r, out, vb, ab);      // sorted by the count pass
    }
    if (feat) {
      bitonic_sort<int64_t, true>(vkey, nv, tid, BIG_THREADS);
      if (tid < DVA_WAVE) rank_views<int64_t>(vkey, nv, tid);
      __syncthreads();
      mean_features<int64_t>(vkey, nv, feat, F, out.features, vb, tid, BIG_THREADS);
    }
  }
}

static inline int merge_check_sizes(int64_t N, int64_t V, int64_t P) {
  if (N < 1 || any_negative({V, P})) return DVA_ERR_INVALID;
  return fits_i31({N, V, P});
}

}  // namespace dva

using namespace dva;

extern "C" {

int dva_mapping_merge_tile_atoms(void) { return MERGE_TILE; }

int64_t dva_mapping_merge_workspace_bytes(int64_t n_points, int64_t n_views, int64_t n_atoms) {
  const int rc = merge_check_sizes(n_points, n_views, n_atoms);
  if (rc != DVA_OK) return rc;
  return merge_layout(nullptr, n_points, n_views, n_atoms).total;
}

int dva_mapping_merge_count(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                            const void* pixels, int32_t pixel_bytes, const int64_t* idx, int64_t n_points,
                            int64_t n_views, int64_t n_atoms, int64_t* sizes, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  int rc = merge_check_sizes(n_points, n_views, n_atoms);
  if (rc != DVA_OK) return rc;
  if ((rc = pixel_bytes_code(pixel_bytes)) != DVA_OK) return rc;
  if (!pointers || !idx || !sizes || !workspace || ((uintptr_t)workspace & 15)) return DVA_ERR_INVALID;
  if (!mapping_arrays_ok(images, atom_ptr, pixels, n_views, n_atoms)) return DVA_ERR_INVALID;
  const MergeLayout L = merge_layout(workspace, n_points, n_views, n_atoms);
  if (workspace_bytes < L.total) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = n_points;
  // ctr and hist are adjacent
  if (hipMemsetAsync(L.ctr, 0, (size_t)((char*)L.voxel_ptr - (char*)L.ctr), s) != hipSuccess) return DVA_ERR_LAUNCH;
  hipLaunchKernelGGL(merge_hist_kernel, dim3(capped_grid(N, 256, 4096)), dim3(256), 0, s, idx, N, L.hist, L.ctr);
  launch_scan(L.hist, N, L.bsum, L.nb, L.voxel_ptr, s);
  hipLaunchKernelGGL(merge_scatter_kernel, dim3(capped_grid(N, 256, 4096)), dim3(256), 0, s, idx, N, L.hist,
                     L.voxel_ptr, L.members);
  const MergeIn in = {pointers, images, atom_ptr, (const uint32_t*)pixels, L.voxel_ptr, L.members};
  hipLaunchKernelGGL(merge_count_small_kernel, dim3(capped_grid(N, 1, MERGE_GRID)), dim3(DVA_WAVE), 0, s, in, N, L.ctr,
                     L.nviews, L.natoms, L.big_j, L.big_na, L.big_nv, L.bigcap);
  hipLaunchKernelGGL(merge_count_big_kernel, dim3(capped_grid(L.bigcap, 1, BIG_GRID)), dim3(BIG_THREADS), 0, s, in,
                     L.ctr, L.nviews, L.natoms, L.big_j, L.big_na, L.big_nv, L.big_aoff, L.big_voff, L.bigcap,
                     L.scratch_a, L.scratch_v, n_atoms, n_views);
  launch_scan(L.nviews, N, L.bsum, L.nb, L.view_base, s);
  launch_scan(L.natoms, N, L.bsum, L.nb, L.atom_base, s);
  hipLaunchKernelGGL(merge_sizes_kernel, dim3(1), dim3(1), 0, s, L.ctr, L.view_base, L.atom_base, N, sizes);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_mapping_merge_fill(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                           const void* pixels, int32_t pixel_bytes, const float* features, int32_t F,
                           int64_t n_points, int64_t n_views, int64_t n_atoms, int64_t n_voxels,
                           int64_t n_views_out, int64_t n_atoms_out, int64_t* out_pointers, int64_t* out_images,
                           int64_t* out_atom_ptr, void* out_pixels, float* out_features, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  int rc = merge_check_sizes(n_points, n_views, n_atoms);
  if (rc != DVA_OK) return rc;
  if ((rc = pixel_bytes_code(pixel_bytes)) != DVA_OK) return rc;
  if (n_voxels < 1 || n_voxels > n_points || n_views_out < 0 || n_views_out > n_views || n_atoms_out < 0 ||
      n_atoms_out > n_atoms || F < 0)
    return DVA_ERR_INVALID;
  if (F > MERGE_MAX_F) return DVA_ERR_UNSUPPORTED;
  if (!pointers || !workspace || !out_pointers || !out_atom_ptr) return DVA_ERR_INVALID;
  if (!mapping_arrays_ok(images, atom_ptr, pixels, n_views, n_atoms)) return DVA_ERR_INVALID;
  if ((n_views_out > 0 && !out_images) || (n_atoms_out > 0 && !out_pixels)) return DVA_ERR_INVALID;
  if ((features != nullptr) != (out_features != nullptr) || (features && F < 1)) return DVA_ERR_INVALID;
  if (((uintptr_t)out_pixels & 3) || ((uintptr_t)workspace & 15)) return DVA_ERR_INVALID;
  const MergeLayout L = merge_layout(workspace, n_points, n_views, n_atoms);
  if (workspace_bytes < L.total) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const MergeIn in = {pointers, images, atom_ptr, (const uint32_t*)pixels, L.voxel_ptr, L.members};
  const MergeOut out = {out_pointers, out_images, out_atom_ptr, (uint32_t*)out_pixels, out_features};
  hipLaunchKernelGGL(merge_fill_small_kernel, dim3(capped_grid(n_voxels, 1, MERGE_GRID)), dim3(DVA_WAVE), 0, s, in,
                     features, (int)F, n_voxels, L.view_base, L.atom_base, out, n_views_out, n_atoms_out);
  hipLaunchKernelGGL(merge_fill_big_kernel, dim3(capped_grid(L.bigcap, 1, BIG_GRID)), dim3(BIG_THREADS), 0, s, L.ctr,
                     features, (int)F, L.view_base, L.atom_base, L.big_j, L.big_na, L.big_nv, L.big_aoff, L.big_voff,
                     L.bigcap, L.scratch_a, L.scratch_v, out);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
