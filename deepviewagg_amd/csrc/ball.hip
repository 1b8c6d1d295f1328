// Exact radius query: the device side of SphereSampling / CylinderSampling and their Grid* tilings (reference:
// core/data_transform/transforms.py:99-232, :301-405 over scikit-learn KDTree.query_radius, one centre at a time on
// the host).
//
// Predicate (scikit-learn's leaf test): point p is a member of centre c iff d <= r * r, with
//   d = ((dx * dx) + dy * dy) + dz * dz,   dx = (double)p.x - c.x,
// every product and every sum rounded on its own in fp64 (no fused multiply-add; the translation unit is compiled with
// contraction off and the operations are spelled __dmul_rn / __dadd_rn / __dsub_rn), r * r computed once, the
// boundary inclusive.  dims = 2 leaves the z term out (the cylinder).  A point with a non-finite coordinate is never
// a member: it is loaded as NaN, so that every comparison with it is false.
//
// Brute force over all (point, centre) pairs, two passes, no atomics, bitwise reproducible:
//   count  a TILE is the BALL_PPT x 64 consecutive points one wavefront holds in registers (point j of lane l is
//          tile base + 64 j + l) as doubles; the four wavefronts of a block share the centres, staged in LDS in chunks
//          of BALL_CHUNK {x, y, z, r^2}.  Per centre a wavefront sums the popcounts of its BALL_PPT ballots; lane k
//          keeps the count of centre k of a group of 64, and the group is written as one row segment of the count
//          table cnt[tile][centre] (centre fastest: one coalesced 256-byte store per tile and group).
//   scan   per centre over the tiles (in segments of BALL_SEG tiles: segment sums, exclusive scan of the segment sums
//          and, over the centres, of the totals -> ptr int64 [B + 1], then the tile offsets in place), so that
//          cnt[tile][centre] becomes the number of members of the centre in the tiles before this one.
//   fill   the predicate again; member (j, l) of tile t is written at ptr[c] + cnt[t][c] + (members of the wavefront's
//          earlier ballots) + (members in lower lanes of this ballot, v_mbcnt): ascending point index for free.
// Because a tile belongs to one wavefront, the rank needs no exchange between the wavefronts of a block.
// The count table bounds the centres of one call: the host wrapper (ops.radius_query) splits them to a budget.
#include "dva_common.h"

#pragma clang fp contract(off)

namespace dva {

constexpr int BALL_TPB = 256;
constexpr int BALL_WAVES = BALL_TPB / DVA_WAVE;
constexpr int BALL_PPT = 8;                          // points per lane
constexpr int BALL_TILE = BALL_PPT * DVA_WAVE;       // points per wavefront
constexpr int BALL_CHUNK = 256;                      // centres staged in LDS at a time (a multiple of 64)
constexpr int BALL_SEG = 128;                        // tiles per scan segment
constexpr int BALL_SCAN_TPB = 1024;
constexpr int64_t BALL_MAX_N = 0x7fffffffLL;

struct __attribute__((aligned(32))) BallCentre {
  double x, y, z, r2;
};

static inline int64_t ball_tiles(int64_t n) { return (n + BALL_TILE - 1) / BALL_TILE; }
static inline int64_t ball_segs(int64_t tiles) { return (tiles + BALL_SEG - 1) / BALL_SEG; }

template <int DIMS>
__device__ __forceinline__ bool ball_member(double px, double py, double pz, const BallCentre& c) {
  const double dx = __dsub_rn(px, c.x);
  const double dy = __dsub_rn(py, c.y);
  double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
  if (DIMS == 3) {
    const double dz = __dsub_rn(pz, c.z);
    d = __dadd_rn(d, __dmul_rn(dz, dz));
  }
  return d <= c.r2;
}

// The wavefront's tile, as doubles.  Lanes past the end of the cloud and non-finite points hold NaN.
__device__ __forceinline__ void ball_load_tile(const float* __restrict__ pos, int64_t n, int64_t tile, int lane,
                                               double* px, double* py, double* pz) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int j = 0; j < BALL_PPT; ++j) {
    const int64_t i = tile * BALL_TILE + j * DVA_WAVE + lane;
    px[j] = nan;
    py[j] = nan;
    pz[j] = nan;
    if (i < n) {
      const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
      if (isfinite(x) && isfinite(y) && isfinite(z)) {
        px[j] = (double)x;
        py[j] = (double)y;
        pz[j] = (double)z;
      }
    }
  }
}

// Centres c0 .. c0 + m of the chunk into LDS, r * r computed here, once per centre.  A negative or NaN radius gives
// an empty ball.
template <int DIMS>
__device__ __forceinline__ void ball_stage(const double* __restrict__ centres, double radius,
                                           const double* __restrict__ radii, int64_t c0, int m, BallCentre* sc) {
  for (int k = threadIdx.x; k < m; k += BALL_TPB) {
    const int64_t c = c0 + k;
    const double r = radii ? radii[c] : radius;
    BallCentre v;
    v.x = centres[c * DIMS];
    v.y = centres[c * DIMS + 1];
    v.z = DIMS == 3 ? centres[c * DIMS + 2] : 0.0;
    v.r2 = r >= 0.0 ? __dmul_rn(r, r) : -1.0;
    sc[k] = v;
  }
}

template <int DIMS>
__global__ __launch_bounds__(BALL_TPB) void ball_count_kernel(const float* __restrict__ pos, int64_t n,
                                                              const double* __restrict__ centres, int64_t B,
                                                              double radius, const double* __restrict__ radii,
                                                              int64_t tiles, uint32_t* __restrict__ cnt) {
  __shared__ BallCentre sc[BALL_CHUNK];
  const int lane = threadIdx.x & (DVA_WAVE - 1);
  const int64_t tile = blockIdx.x * (int64_t)BALL_WAVES + (threadIdx.x >> 6);
  double px[BALL_PPT], py[BALL_PPT], pz[BALL_PPT];
  ball_load_tile(pos, n, tile, lane, px, py, pz);
  for (int64_t c0 = 0; c0 < B; c0 += BALL_CHUNK) {
    const int m = (int)(B - c0 < BALL_CHUNK ? B - c0 : BALL_CHUNK);
    __syncthreads();                                   // the previous chunk is consumed
    ball_stage<DIMS>(centres, radius, radii, c0, m, sc);
    __syncthreads();
    for (int g = 0; g < m; g += DVA_WAVE) {
      const int ge = m - g < DVA_WAVE ? m - g : DVA_WAVE;
      uint32_t mine = 0;
      for (int k = 0; k < ge; ++k) {
        const BallCentre c = sc[g + k];
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < BALL_PPT; ++j)
          total += (uint32_t)__popcll(__ballot(ball_member<DIMS>(px[j], py[j], pz[j], c)));
        if (lane == k) mine = total;
      }
      if (tile < tiles && lane < ge) cnt[tile * B + c0 + g + lane] = mine;
    }
  }
}

template <int DIMS>
__global__ __launch_bounds__(BALL_TPB) void ball_fill_kernel(const float* __restrict__ pos, int64_t n,
                                                             const double* __restrict__ centres, int64_t B,
                                                             double radius, const double* __restrict__ radii,
                                                             int64_t tiles, const uint32_t* __restrict__ cnt,
                                                             const int64_t* __restrict__ ptr, int64_t* __restrict__ idx,
                                                             int64_t capacity) {
  __shared__ BallCentre sc[BALL_CHUNK];
  __shared__ int64_t sp[BALL_CHUNK];
  const int lane = threadIdx.x & (DVA_WAVE - 1);
  const int64_t tile = blockIdx.x * (int64_t)BALL_WAVES + (threadIdx.x >> 6);
  const bool live = tile < tiles;
  double px[BALL_PPT], py[BALL_PPT], pz[BALL_PPT];
  ball_load_tile(pos, n, tile, lane, px, py, pz);
  const int64_t first = tile * BALL_TILE + lane;
  for (int64_t c0 = 0; c0 < B; c0 += BALL_CHUNK) {
    const int m = (int)(B - c0 < BALL_CHUNK ? B - c0 : BALL_CHUNK);
    __syncthreads();
    ball_stage<DIMS>(centres, radius, radii, c0, m, sc);
    for (int k = threadIdx.x; k < m; k += BALL_TPB) sp[k] = ptr[c0 + k];
    __syncthreads();
    if (!live) continue;                               // wave-uniform; the barriers above are still reached
    for (int g = 0; g < m; g += DVA_WAVE) {
      const int ge = m - g < DVA_WAVE ? m - g : DVA_WAVE;
      const uint32_t off = lane < ge ? cnt[tile * B + c0 + g + lane] : 0u;
      for (int k = 0; k < ge; ++k) {
        const BallCentre c = sc[g + k];
        int64_t base = sp[g + k] + (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)off, k);
#pragma unroll
        for (int j = 0; j < BALL_PPT; ++j) {
          const bool in = ball_member<DIMS>(px[j], py[j], pz[j], c);
          const uint64_t mask = __ballot(in);
          const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
          const int64_t at = base + below;
          if (in && at < capacity) idx[at] = first + j * DVA_WAVE;
          base += __popcll(mask);
        }
      }
    }
  }
}

// seg[s][c] = members of centre c in the tiles of segment s
__global__ __launch_bounds__(BALL_TPB) void ball_seg_sum_kernel(const uint32_t* __restrict__ cnt, int64_t B,
                                                                int64_t tiles, uint32_t* __restrict__ seg) {
  const int64_t c = blockIdx.x * (int64_t)BALL_TPB + threadIdx.x;
  if (c >= B) return;
  const int64_t s = blockIdx.y;
  const int64_t t0 = s * BALL_SEG, t1 = t0 + BALL_SEG < tiles ? t0 + BALL_SEG : tiles;
  uint32_t sum = 0;
  for (int64_t t = t0; t < t1; ++t) sum += cnt[t * B + c];
  seg[s * B + c] = sum;
}

// One block: per centre the exclusive scan of its segment sums (in place) and its total; ptr = exclusive scan of the
// totals over the centres, ptr[B] = the number of members of all centres.
__global__ __launch_bounds__(BALL_SCAN_TPB) void ball_ptr_kernel(uint32_t* __restrict__ seg, int64_t B, int64_t segs,
                                                                 int64_t* __restrict__ ptr) {
  __shared__ int64_t sh[BALL_SCAN_TPB];
  __shared__ int64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < B; c0 += BALL_SCAN_TPB) {
    const int64_t c = c0 + threadIdx.x;
    int64_t total = 0;
    if (c < B) {
      for (int64_t s = 0; s < segs; ++s) {
        const uint32_t v = seg[s * B + c];
        seg[s * B + c] = (uint32_t)total;              // a centre has at most n < 2^31 members
        total += v;
      }
    }
    sh[threadIdx.x] = total;
    __syncthreads();
    for (int w = 1; w < BALL_SCAN_TPB; w <<= 1) {      // inclusive scan
      const int64_t add = threadIdx.x >= w ? sh[threadIdx.x - w] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    const int64_t before = carry;
    if (c < B) ptr[c] = before + sh[threadIdx.x] - total;
    __syncthreads();
    if (threadIdx.x == BALL_SCAN_TPB - 1) carry = before + sh[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) ptr[B] = carry;
}

// cnt[t][c] -> members of centre c in the tiles before t
__global__ __launch_bounds__(BALL_TPB) void ball_tile_offset_kernel(uint32_t* __restrict__ cnt, int64_t B,
                                                                    int64_t tiles, const uint32_t* __restrict__ seg) {
  const int64_t c = blockIdx.x * (int64_t)BALL_TPB + threadIdx.x;
  if (c >= B) return;
  const int64_t s = blockIdx.y;
  const int64_t t0 = s * BALL_SEG, t1 = t0 + BALL_SEG < tiles ? t0 + BALL_SEG : tiles;
  uint32_t run = seg[s * B + c];
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t v = cnt[t * B + c];
    cnt[t * B + c] = run;
    run += v;
  }
}

struct BallLayout {
  uint32_t *cnt, *seg;
  size_t total;
};

static void ball_layout(void* ws, int64_t n, int64_t B, BallLayout* L) {
  const int64_t tiles = ball_tiles(n);
  Carver c(ws);
  L->cnt = c.take<uint32_t>((size_t)tiles * (size_t)B);
  L->seg = c.take<uint32_t>((size_t)ball_segs(tiles) * (size_t)B);
  L->total = c.used() < 256 ? 256 : c.used();
}

static int ball_check(const float* pos, int64_t n, const double* centres, int64_t B, int32_t dims, double radius,
                      const double* radii, const void* ws) {
  if (n < 0 || B < 0 || (dims != 2 && dims != 3)) return DVA_ERR_INVALID;
  if ((n > 0 && !pos) || (B > 0 && !centres) || !ws) return DVA_ERR_INVALID;
  if (!radii && !(radius >= 0.0)) return DVA_ERR_INVALID;     // negative or NaN
  if (n > BALL_MAX_N) return DVA_ERR_UNSUPPORTED;
  return DVA_OK;
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_radius_query_workspace_bytes(int64_t n, int64_t n_centres) {
  if (n < 0 || n_centres < 0) return DVA_ERR_INVALID;
  if (n > BALL_MAX_N) return DVA_ERR_UNSUPPORTED;
  BallLayout L;
  ball_layout(nullptr, n, n_centres, &L);
  return (int64_t)L.total;
}

int dva_radius_count(const float* pos, int64_t n, const double* centres, int64_t n_centres, int32_t dims,
                     double radius, const double* radii, int64_t* ptr, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  const int rc = ball_check(pos, n, centres, n_centres, dims, radius, radii, workspace);
  if (rc) return rc;
  if (!ptr) return DVA_ERR_INVALID;
  BallLayout L;
  ball_layout(workspace, n, n_centres, &L);
  if ((int64_t)L.total > workspace_bytes) return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = n_centres, tiles = ball_tiles(n), segs = ball_segs(tiles);
  if (B == 0 || n == 0) {
    if (hipMemsetAsync(ptr, 0, (size_t)(B + 1) * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
    return DVA_OK;
  }
  const dim3 pgrid((unsigned)((tiles + BALL_WAVES - 1) / BALL_WAVES));
  if (dims == 3)
    hipLaunchKernelGGL(ball_count_kernel<3>, pgrid, dim3(BALL_TPB), 0, s, pos, n, centres, B, radius, radii, tiles,
                       L.cnt);
  else
    hipLaunchKernelGGL(ball_count_kernel<2>, pgrid, dim3(BALL_TPB), 0, s, pos, n, centres, B, radius, radii, tiles,
                       L.cnt);
  const dim3 sgrid((unsigned)((B + BALL_TPB - 1) / BALL_TPB), (unsigned)segs);
  hipLaunchKernelGGL(ball_seg_sum_kernel, sgrid, dim3(BALL_TPB), 0, s, L.cnt, B, tiles, L.seg);
  hipLaunchKernelGGL(ball_ptr_kernel, dim3(1), dim3(BALL_SCAN_TPB), 0, s, L.seg, B, segs, ptr);
  hipLaunchKernelGGL(ball_tile_offset_kernel, sgrid, dim3(BALL_TPB), 0, s, L.cnt, B, tiles, L.seg);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_radius_fill(const float* pos, int64_t n, const double* centres, int64_t n_centres, int32_t dims,
                    double radius, const double* radii, const int64_t* ptr, int64_t* idx, int64_t idx_capacity,
                    void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = ball_check(pos, n, centres, n_centres, dims, radius, radii, workspace);
  if (rc) return rc;
  if (!ptr || idx_capacity < 0 || (idx_capacity > 0 && !idx)) return DVA_ERR_INVALID;
  BallLayout L;
  ball_layout(workspace, n, n_centres, &L);
  if ((int64_t)L.total > workspace_bytes) return DVA_ERR_INVALID;
  const int64_t B = n_centres, tiles = ball_tiles(n);
  if (B == 0 || n == 0 || idx_capacity == 0) return DVA_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 pgrid((unsigned)((tiles + BALL_WAVES - 1) / BALL_WAVES));
  if (dims == 3)
    hipLaunchKernelGGL(ball_fill_kernel<3>, pgrid, dim3(BALL_TPB), 0, s, pos, n, centres, B, radius, radii, tiles,
                       L.cnt, ptr, idx, idx_capacity);
  else
    hipLaunchKernelGGL(ball_fill_kernel<2>, pgrid, dim3(BALL_TPB), 0, s, pos, n, centres, B, radius, radii, tiles,
                       L.cnt, ptr, idx, idx_capacity);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
