// Fused DeepSetFeat + E_score chain for gfx950: the per-view mapping-feature encoder of
// GroupBimodalCSRPool / QKVBimodalCSRPool (reference: modules/multimodal/pooling.py:604-673 DeepSetFeat
// with pool='max', fusion='concatenation'; :258,:282 E_score; MLP / FastBatchNorm1d of
// core/common_modules/base_modules.py:38-48,:131-156), forward AND backward, exact fp32.
//
// Why: the chain is six tiny Linear(<=64 -> 32) layers with train-mode BatchNorm between them over
// V = tens of millions of views.  Library GEMM + BN + activation kernels move ~4 KB/view and the
// skinny GEMMs run at <5 % of HBM speed; here every stage between two batch-statistics barriers is
// ONE pass that reads the previous pre-BN activation (128 B/view), applies BN + LeakyReLU on load,
// does the 32x32 product and writes the next pre-BN activation (128 B/view) while accumulating the
// next layer's statistics.
//
// This file holds the C entry points of the family (dva_deepset_*, dva_csr_expand: argument checks,
// then the launch) and the kernels that are not 32x32 layer passes:
//   dsf_segmax_kernel     max over the views of a point, with the arg row (both storage types)
//   dsf_bwd_first_kernel  weight gradient of the first layer (x_map [V,8] -> 32), used with fp32
//                         storage; with bf16 storage the layer pass before it folds this in
//   csr_expand_kernel     view -> point index from the CSR pointers
// The layer passes themselves (first, layer, score, their backward and the max-path join) are the
// fp32-MFMA kernels of deepset_mfma.hip, reached through the dsm_launch_* functions declared below.
#include "dva_common.h"

namespace dva {

constexpr int D = 32;       // nc_inner of the fused path
constexpr int TILE = 32;    // rows per wavefront tile
constexpr float SLOPE = 0.2f;

struct BNc {  // batch-norm constants of one channel
  float mean, invstd, gamma, beta;
};
// bn arrays are [4][D] = mean | invstd | gamma | beta
__device__ __forceinline__ BNc load_bn(const float* __restrict__ bn, int c) {
  BNc b;
  b.mean = bn[c]; b.invstd = bn[D + c]; b.gamma = bn[2 * D + c]; b.beta = bn[3 * D + c];
  return b;
}
__device__ __forceinline__ float bn_hat(float a, const BNc& b) { return (a - b.mean) * b.invstd; }
__device__ __forceinline__ float bn_z(float a, const BNc& b) { return bn_hat(a, b) * b.gamma + b.beta; }
__device__ __forceinline__ float leaky(float z) { return z > 0.f ? z : SLOPE * z; }

// Intra-wavefront LDS hand-off.  The DS instructions of one wavefront execute in program order, so
// a later ds_read sees an earlier ds_write of another lane of the same wavefront; only the compiler
// must be kept from reordering.  Deliberately NOT a memory fence: a release fence waits for
// vmcnt(0), i.e. for the tile's global STORES to be acknowledged before the next tile's loads can
// issue, which made the first version of these kernels latency-bound (17 us per tile per wave).
__device__ __forceinline__ void wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// sum_k row[k] * w[k], k ascending, row broadcast from LDS
template <int K>
__device__ __forceinline__ float dot_row(const float* __restrict__ row, const float (&w)[K]) {
  // two independent fma chains (even / odd float4 blocks) halve the dependent-latency exposure
  float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
  for (int k4 = 0; k4 < K / 4; k4 += 2) {
    const float4 x = *reinterpret_cast<const float4*>(row + 4 * k4);
    const float4 y = *reinterpret_cast<const float4*>(row + 4 * k4 + 4);
    acc0 = fmaf(x.x, w[4 * k4], acc0);
    acc1 = fmaf(y.x, w[4 * k4 + 4], acc1);
    acc0 = fmaf(x.y, w[4 * k4 + 1], acc0);
    acc1 = fmaf(y.y, w[4 * k4 + 5], acc1);
    acc0 = fmaf(x.z, w[4 * k4 + 2], acc0);
    acc1 = fmaf(y.z, w[4 * k4 + 6], acc1);
    acc0 = fmaf(x.w, w[4 * k4 + 3], acc0);
    acc1 = fmaf(y.w, w[4 * k4 + 7], acc1);
  }
  return acc0 + acc1;
}

// pooled[p, c] = max over the point's views of leaky(BN(a[v, c])) (first row on ties), arg = that row.
// One half-wave per point: every lane reads 16 bytes (VEC channels) of a row, 32/LPR rows are in flight
// per half-wave and four row loads per lane are issued before the first is used; the row slots are then
// merged with xor-shuffles (value, row) -- larger value wins, smaller row on ties.
// LPP lanes per point (32, 16 or 8; at least LPR): the host picks it from the average segment length so that
// short ragged segments (a handful of views per point) do not leave most row slots idle.
template <typename AT, int LPP>
__global__ __launch_bounds__(256) void dsf_segmax_kernel(const AT* __restrict__ a,
                                                          const float* __restrict__ bn,
                                                          const int64_t* __restrict__ ptr,
                                                          float* __restrict__ pooled,
                                                          int32_t* __restrict__ arg, int64_t N) {
  constexpr int VEC = Chunk16<AT>::N, LPR = D / VEC, SLOTS = LPP / LPR, U = 4, PPW = 64 / LPP;
  static_assert(LPP >= LPR && SLOTS >= 1, "a point needs at least one row of lanes");
  typedef typename Chunk16<AT>::raw raw_t;
  const int lane = threadIdx.x & 63, hl = lane & (LPP - 1), h = lane / LPP;
  const int cl = hl % LPR, slot = hl / LPR, c0 = cl * VEC;
  BNc b[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) b[k] = load_bn(bn, c0 + k);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t p2 = wave * PPW; p2 < N; p2 += n_waves * PPW) {
    const int64_t p = p2 + h;
    const bool valid = p < N;
    const int64_t beg = valid ? ptr[p] : 0;
    const int64_t end = valid ? ptr[p + 1] : 0;
    float m[VEC];
    int am[VEC];            // row offset inside the segment (32-bit: halves the shuffle / select work)
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      m[k] = -INFINITY;
      am[k] = -1;
    }
    // the points of a wavefront iterate together (shuffles below need every lane)
    const int n_seg = (int)(end - beg);
    int n_max = n_seg;
#pragma unroll
    for (int off = LPP; off < 64; off <<= 1) n_max = max(n_max, __shfl_xor(n_max, off));
    for (int i0 = 0; i0 < n_max; i0 += SLOTS * U) {
      raw_t raw[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * SLOTS + slot;
        ok[u] = i < n_seg;
        const int64_t r = n_seg > 0 ? beg + (ok[u] ? i : 0) : 0;   // clamped: loads are unconditional
        raw[u] = *reinterpret_cast<const raw_t*>(a + r * D + c0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float f[VEC];
        Chunk16<AT>::unpack(raw[u], f);
        const int i = i0 + u * SLOTS + slot;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float v = leaky(bn_z(f[k], b[k]));
          if (ok[u] && v > m[k]) {   // rows ascend within a lane: strict > keeps the first row on ties
            m[k] = v;
            am[k] = i;
          }
        }
      }
    }
    // merge the row slots: lanes hl, hl ^ off hold the same channels for different rows
#pragma unroll
    for (int off = LPR; off < LPP; off <<= 1) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float ov = __shfl_xor(m[k], off);
        const int oa = __shfl_xor(am[k], off);
        if (oa >= 0 && (am[k] < 0 || ov > m[k] || (ov == m[k] && oa < am[k]))) {
          m[k] = ov;
          am[k] = oa;
        }
      }
    }
    if (valid && slot == 0) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        pooled[p * D + c0 + k] = am[k] >= 0 ? m[k] : 0.f;
        arg[p * D + c0 + k] = am[k] >= 0 ? (int32_t)(beg + am[k]) : -1;
      }
    }
  }
}

// First layer: a1 = x.Wa^T recomputed, da1 = BN-backward(dz1), dWa[n][j] += da1[v][n] x[v][j]
template <typename AT>
__global__ __launch_bounds__(256) void dsf_bwd_first_kernel(
    const AT* __restrict__ dz1, const float* __restrict__ x_map, const float* __restrict__ Wa,
    const float* __restrict__ bn1, const float* __restrict__ sm1, float* __restrict__ dWa, int64_t V) {
  __shared__ __attribute__((aligned(16))) float s_x[4][TILE * 8];
  __shared__ float s_red[D * 8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
  const BNc b = load_bn(bn1, n);
  const float s1m = sm1[n], s2m = sm1[D + n], gsc = b.gamma * b.invstd;
  float wa[8], acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    wa[k] = Wa[n * 8 + k];
    acc[k] = 0.f;
  }
  const int64_t tiles = (V + TILE - 1) / TILE;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t t = wave; t < tiles; t += n_waves) {
    const int64_t row0 = t * TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = i * 64 + lane;
      const int64_t g = row0 * 8 + e;
      s_x[wv][e] = g < V * 8 ? x_map[g] : 0.f;
    }
    wave_sync();
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int row = 2 * i + h;
      const int64_t r = row0 + row;
      if (r < V) {
        const float a1 = dot_row<8>(&s_x[wv][row * 8], wa);
        const float da = gsc * (Elt<AT>::ld(dz1, r * D + n) - s1m - bn_hat(a1, b) * s2m);
        const float4 x0 = *reinterpret_cast<const float4*>(&s_x[wv][row * 8]);
        const float4 x1 = *reinterpret_cast<const float4*>(&s_x[wv][row * 8 + 4]);
        acc[0] = fmaf(da, x0.x, acc[0]); acc[1] = fmaf(da, x0.y, acc[1]);
        acc[2] = fmaf(da, x0.z, acc[2]); acc[3] = fmaf(da, x0.w, acc[3]);
        acc[4] = fmaf(da, x1.x, acc[4]); acc[5] = fmaf(da, x1.y, acc[5]);
        acc[6] = fmaf(da, x1.z, acc[6]); acc[7] = fmaf(da, x1.w, acc[7]);
      }
    }
    wave_sync();
  }
  for (int i = threadIdx.x; i < D * 8; i += blockDim.x) s_red[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = acc[k] + __shfl_xor(acc[k], 32);
    if (lane < 32) atomicAdd(&s_red[n * 8 + k], v);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < D * 8; i += blockDim.x) atomicAdd(&dWa[i], s_red[i]);
}

// the last lane whose `start` (nondecreasing over the wavefront, start of lane 0 <= o) is at most o: six steps in registers
__device__ __forceinline__ int last_start_at_most(int start, int o) {
  int pos = 0;
#pragma unroll
  for (int step = 32; step; step >>= 1) pos += __shfl(start, pos + step) <= o ? step : 0;
  return pos;
}

// view -> point index (dense expansion of the CSR pointers): a wavefront takes 64 points and reads their pointers
// coalesced.  Long segments: the wavefront sweeps the views of its points 256 at a time, every lane owns four
// consecutive views = one 16-byte store (vp_mis = the int32 index of vp modulo 4: the sweep starts on a 16-byte
// boundary) and finds their points by a search among the 64 loaded pointers.  (Writing the views of one point after the
// other with all lanes took 64 serial trips of half-empty dword stores on the 32-views-per-point scenes; one thread per
// point wrote 4-byte words 128 bytes apart.)
__global__ __launch_bounds__(256) void csr_expand_kernel(const int64_t* __restrict__ ptr, int64_t N,
                                                          int32_t* __restrict__ vp, int vp_mis) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t p0 = wave * 64; p0 < N; p0 += n_waves * 64) {
    const int64_t pl = p0 + lane < N ? p0 + lane : N - 1;
    const int64_t b = ptr[pl], e = ptr[pl + 1];
    const int n_here = (int)(N - p0 < 64 ? N - p0 : 64);
    const int64_t first = __shfl(b, 0), last = __shfl(e, n_here - 1);
    if (last - first <= 8 * n_here) {
      // short segments (ragged scenes): every lane writes the few views of its own point (2^20 points: 11.7 against
      // 12.6 us with the sweep below at min(32, 1 + Geom(0.2)) views per point, 3.6 against 7.3 us at one view each)
      if (lane < n_here)
        for (int64_t r = b; r < e; ++r) vp[r] = (int32_t)(p0 + lane);
    } else {
      for (int64_t r0 = first - ((first + vp_mis) & 3); r0 < last; r0 += 256) {
        // where the lane's point starts inside this window of 256 views, clamped to it (lanes without a point: behind it)
        const int64_t rb = b - r0;
        const int start = lane < n_here ? (int)(rb < 0 ? 0 : rb > 256 ? 256 : rb) : 256;
        const int o = lane * 4;
        int pt[4];
        pt[0] = last_start_at_most(start, o);
        pt[3] = last_start_at_most(start, o + 3);
        pt[1] = pt[2] = pt[0];
        if (__any(pt[0] != pt[3])) {              // (uniform) some lane's four views belong to more than one point
          pt[1] = last_start_at_most(start, o + 1);
          pt[2] = last_start_at_most(start, o + 2);
        }
        const int64_t r = r0 + o;
        const int32_t base = (int32_t)p0;
        if (r >= first && r + 4 <= last) {
          *reinterpret_cast<int4*>(vp + r) = make_int4(base + pt[0], base + pt[1], base + pt[2], base + pt[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (r + j >= first && r + j < last) vp[r + j] = base + pt[j];
        }
      }
    }
  }
}

static inline int grid_rows(int64_t V) {
  // one wavefront per 32-row tile, 4 wavefronts per block, capped at 8 blocks per CU
  return capped_grid((V + TILE - 1) / TILE, 4, 256 * 8);
}

// the fp32-MFMA layer kernels (deepset_mfma.hip); bf = bf16 activation storage
int dsm_launch_fwd_first(const float*, const float*, const float*, const float*, void*, double*, int64_t,
                         int, int, hipStream_t);
int dsm_launch_fwd_layer(const void*, const float*, const float*, const float*, const int32_t*, void*,
                         double*, int64_t, int, hipStream_t);
int dsm_launch_fwd_score(const void*, const float*, const float*, const float*, float*, int64_t, int, int,
                         hipStream_t);
int dsm_launch_bwd_layer(const void*, const void*, const float*, const float*, const float*, const void*,
                         const float*, const float*, void*, float*, double*, float*, const int32_t*, float*,
                         int64_t, int, int, int, hipStream_t);
int dsm_launch_bwd_max(const void*, const void*, const float*, const int32_t*, const float*, const int32_t*,
                       void*, double*, int64_t, int, hipStream_t);
int dsm_launch_bwd_score(const float*, const void*, const float*, const float*, void*, float*, float*,
                         double*, int64_t, int, int, hipStream_t);

// activation storage code of the C ABI -> 0 (fp32) / 1 (bf16) / -1 (invalid)
static inline int act_bf(int32_t act_dtype) {
  return act_dtype == DVA_F32 ? 0 : act_dtype == DVA_BF16 ? 1 : -1;
}

}  // namespace dva

using namespace dva;

extern "C" {

int dva_csr_expand(const int64_t* ptr, int64_t n_groups, int32_t* group_of_row, void* stream) {
  if (n_groups < 0 || !ptr) return DVA_ERR_INVALID;
  if (n_groups == 0) return DVA_OK;
  if (!group_of_row) return DVA_ERR_INVALID;
  int64_t b = (n_groups + 255) / 256;            // 4 wavefronts x 64 points per block
  if (b > 8192) b = 8192;
  hipLaunchKernelGGL(csr_expand_kernel, dim3((int)b), dim3(256), 0, (hipStream_t)stream, ptr, n_groups,
                     group_of_row, (int)(((uintptr_t)group_of_row >> 2) & 3));
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_fwd_first(const float* x_map, const float* Wa, const float* bn1, const float* Wb,
                          void* a2, double* stats, int64_t V, int32_t F, int32_t stats_only,
                          int32_t act_dtype, void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (V < 0 || !stats || bf < 0) return DVA_ERR_INVALID;
  if (F != 8) return DVA_ERR_UNSUPPORTED;
  if (V == 0) return DVA_OK;
  if (!x_map || !Wa) return DVA_ERR_INVALID;
  if (!stats_only && (!bn1 || !Wb || !a2)) return DVA_ERR_INVALID;
  dsm_launch_fwd_first(x_map, Wa, bn1, Wb, a2, stats, V, stats_only, bf, (hipStream_t)stream);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_segmax(const void* a, const float* bn, const int64_t* ptr, float* pooled,
                       int32_t* arg, int64_t N, int64_t n_views, int32_t act_dtype, void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (N < 0 || bf < 0) return DVA_ERR_INVALID;
  if (N == 0) return DVA_OK;
  if (!a || !bn || !ptr || !pooled || !arg) return DVA_ERR_INVALID;
  // lanes per point from the average segment: a batch covers 4 * (lanes / lanes-per-row) views
  const double avg = n_views > 0 ? (double)n_views / (double)N : 32.0;
  const int lpr = bf ? 4 : 8;
  int lpp = 32;
  while (lpp > lpr && lpp > 8 && 4.0 * (lpp / 2 / lpr) >= 3.0 * avg) lpp >>= 1;
  const int ppb = 4 * (64 / lpp);   // points per block
  int64_t b = (N + ppb - 1) / ppb;
  if (b > 256 * 8) b = 256 * 8;
  hipStream_t s = (hipStream_t)stream;
#define DVA_SM(T, L) \
  hipLaunchKernelGGL((dsf_segmax_kernel<T, L>), dim3((int)b), dim3(256), 0, s, (const T*)a, bn, ptr, pooled, arg, N)
  if (bf) {
    if (lpp == 32) DVA_SM(bf16_t, 32);
    else if (lpp == 16) DVA_SM(bf16_t, 16);
    else DVA_SM(bf16_t, 8);
  } else {
    if (lpp == 32) DVA_SM(float, 32);
    else if (lpp == 16) DVA_SM(float, 16);
    else DVA_SM(float, 8);
  }
#undef DVA_SM
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_fwd_layer(const void* a_in, const float* bn_in, const float* W, const float* addend,
                          const int32_t* group_of_row, void* a_out, double* stats, int64_t V,
                          int32_t act_dtype, void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (V < 0 || !stats || bf < 0) return DVA_ERR_INVALID;
  if (V == 0) return DVA_OK;
  if (!a_in || !W || !a_out) return DVA_ERR_INVALID;
  if (addend && !group_of_row) return DVA_ERR_INVALID;
  dsm_launch_fwd_layer(a_in, bn_in, W, addend, group_of_row, a_out, stats, V, bf, (hipStream_t)stream);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_fwd_score(const void* a, const float* bn, const float* Ws, const float* bs,
                          float* compat, int64_t V, int32_t G, int32_t act_dtype, void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (V < 0 || G <= 0 || G > 32 || bf < 0) return DVA_ERR_INVALID;
  if (V == 0) return DVA_OK;
  if (!a || !bn || !Ws || !bs || !compat) return DVA_ERR_INVALID;
  dsm_launch_fwd_score(a, bn, Ws, bs, compat, V, G, bf, (hipStream_t)stream);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_bwd_score(const float* dcompat, const void* a, const float* bn, const float* Ws,
                          void* dz, float* dWs, float* dbs, double* st, int64_t V, int32_t G,
                          int32_t act_dtype, void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (V < 0 || G <= 0 || bf < 0) return DVA_ERR_INVALID;
  if (G > 32) return DVA_ERR_UNSUPPORTED;
  if (V == 0) return DVA_OK;
  if (!dcompat || !a || !bn || !Ws || !dz || !dWs || !dbs || !st) return DVA_ERR_INVALID;
  dsm_launch_bwd_score(dcompat, a, bn, Ws, dz, dWs, dbs, st, V, G, bf, (hipStream_t)stream);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_bwd_layer(const void* dz_L, const void* a_L, const float* bn_L, const float* sm_L,
                          const float* W_L, const void* a_prev, const float* Wa, const float* bn_prev,
                          void* out, float* dW, double* st_prev, float* dt,
                          const int32_t* group_of_row, float* first_grad, int64_t V,
                          int32_t prev_is_xmap, int32_t raw_out, int32_t act_dtype, void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (V < 0 || bf < 0) return DVA_ERR_INVALID;
  // fused first-layer gradient: bf16 storage, x_map input, batch-norm output, no per-point sum
  if (first_grad && (!bf || !prev_is_xmap || raw_out || dt)) return DVA_ERR_UNSUPPORTED;
  if (V == 0) return DVA_OK;
  if (!dz_L || !a_L || !bn_L || !sm_L || !W_L || !a_prev || (!out && !first_grad) || !dW)
    return DVA_ERR_INVALID;
  if (!bn_prev && (!raw_out || prev_is_xmap)) return DVA_ERR_UNSUPPORTED;
  if (!raw_out && !st_prev) return DVA_ERR_INVALID;
  if (prev_is_xmap && !Wa) return DVA_ERR_INVALID;
  if (dt && !group_of_row) return DVA_ERR_INVALID;
  dsm_launch_bwd_layer(dz_L, a_L, bn_L, sm_L, W_L, a_prev, Wa, bn_prev, out, dW, st_prev, dt, group_of_row,
                       first_grad, V, prev_is_xmap, raw_out, bf, (hipStream_t)stream);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_bwd_max(const void* dcat, const void* a2, const float* bn2, const int32_t* arg,
                        const float* dpooled, const int32_t* group_of_row, void* dz2, double* st,
                        int64_t V, int32_t act_dtype, void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (V < 0 || bf < 0) return DVA_ERR_INVALID;
  if (V == 0) return DVA_OK;
  if (!dcat || !a2 || !bn2 || !arg || !dpooled || !group_of_row || !dz2 || !st) return DVA_ERR_INVALID;
  dsm_launch_bwd_max(dcat, a2, bn2, arg, dpooled, group_of_row, dz2, st, V, bf, (hipStream_t)stream);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_deepset_bwd_first(const void* dz1, const float* x_map, const float* Wa, const float* bn1,
                          const float* sm1, float* dWa, int64_t V, int32_t F, int32_t act_dtype,
                          void* stream) {
  const int bf = act_bf(act_dtype);
  if (act_dtype == DVA_F16) return DVA_ERR_UNSUPPORTED;      // fp32 / bf16 activations only
  if (V < 0 || bf < 0) return DVA_ERR_INVALID;
  if (F != 8) return DVA_ERR_UNSUPPORTED;
  if (V == 0) return DVA_OK;
  if (!dz1 || !x_map || !Wa || !bn1 || !sm1 || !dWa) return DVA_ERR_INVALID;
  if (bf)
    hipLaunchKernelGGL((dsf_bwd_first_kernel<bf16_t>), dim3(grid_rows(V)), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)dz1, x_map, Wa, bn1, sm1, dWa, V);
  else
    hipLaunchKernelGGL((dsf_bwd_first_kernel<float>), dim3(grid_rows(V)), dim3(256), 0,
                       (hipStream_t)stream, (const float*)dz1, x_map, Wa, bn1, sm1, dWa, V);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
