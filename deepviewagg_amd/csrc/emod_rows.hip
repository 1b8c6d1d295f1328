// E_mod on the R feature-map rows as fused row kernels: a two-block MLP [Linear -> count-weighted BatchNorm ->
// LeakyReLU] x 2 on [R, C] bf16 rows in train mode (the hoisting: header of rowbn.hip), widths 32 or 64.  The Linear
// of a block, the BatchNorm + activation of the block before it and the statistics of the BatchNorm after it are ONE
// pass over the rows; the matrix products run on v_mfma_f32_32x32x16_bf16.
//
//   forward   F1  y_a = bf16(x W_a^T),                     sums_a = sum w y_a | sum w y_a^2   (from the rounded y_a)
//             F2  a_a = bf16(leaky(BN_a(y_a))) in registers, y_b = bf16(a_a W_b^T), sums_b
//             F3  out = bf16(leaky(BN_b(y_b)))              = dva_rowbn_apply (no product: the row kernel is the pass)
//   backward  B1  S1 = sum dz_b, S2 = sum dz_b a_b          = dva_rowbn_bwd_stats (likewise)
//             B2  dy_b (formula of rowbn.hip, rounded to bf16), dW_b += dy_b^T a_a (a_a recomputed from y_a),
//                 g_a = bf16(dy_b W_b) stored, statistics of dz_a = g_a leaky'(z_a)
//             B3  dy_a, dW_a += dy_a^T x, g_x = bf16(dy_a W_a) stored
// dva_bn_finalize / dva_bn_bwd_consts run between the passes as they do between the rowbn passes.  Every rounding
// point is where the composition of library GEMMs and rowbn passes has it; the per-element BatchNorm arithmetic is
// rowbn_math.h's.
//
// Geometry (chain_common.h): a wavefront owns a tile of 32 rows, lane l = (j, h) = (l & 31, l >> 5) holds row j.  Of
// every block nb of 32 channels the lane holds the 16 consecutive channels 32 nb + 16 h + r, r < 16 -- 32 bytes of the
// row: two 16-byte loads, which ARE the B operands of the k-blocks 2 nb and 2 nb + 1.  Row i of a weight operand
// carries output channel 32 ob + 16 ((i >> 2) & 1) + (i & 3) + 4 (i >> 3), so that accumulator register r of lane
// (j, h) is channel 32 ob + 16 h + r again: a product's result packs into the operand of the next product, and into
// two 16-byte stores, without any data movement.  Weight operands are rounded from the fp32 parameters and staged in
// LDS once per block.  Weight gradients: natural tiles + transpose reads (tileN_put_packed / wgradN), per-wavefront
// accumulators, summed over the wavefronts of a block in a fixed order, one fp32 [C_out][C_in] partial per block in a
// workspace, added in a fixed order by dw_reduce_kernel: no float atomics.  Statistics: fp32 over the four rows of a lane
// quad and FLUSH_TILES tiles, fp32 over the eight quads of the tile at a flush (a fixed tree), fp64 from there on (per
// lane, per block in wavefront order, fp64 atomics per block as in rowbn.hip).
#include "chain_common.h"
#include "rowbn_math.h"

namespace dva {
namespace emod_rows {

using namespace chain;

constexpr int WAVES = 4;        // wavefronts per block
constexpr int FLUSH_TILES = 4;  // tiles a lane adds in fp32 before the sums go to fp64

// image column (16 h + r) held by row i of a weight operand: the inverse of chain::cperm
__host__ __device__ __forceinline__ int icol(int i) { return 16 * ((i >> 2) & 1) + (i & 3) + 4 * (i >> 3); }

__device__ __forceinline__ f32x16 zero16() {
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.f;
  return c;
}

// ---- weight operands ------------------------------------------------------------------------------------------------
// y = x W^T, W fp32 [CO][CI]: entry (ob * (CI / 16) + kb) * 64 + lane; k-block kb = 2 nb + t of lane half hh covers the
// input channels 32 nb + 16 hh + 8 t + s
template <int CI, int CO>
__device__ __forceinline__ void stage_w(uint4* s_w, const float* __restrict__ W) {
  constexpr int NKB = CI / 16, NOB = CO / 32;
  for (int e = threadIdx.x; e < NOB * NKB * 64; e += blockDim.x) {
    const int l = e & 63, kb = (e >> 6) % NKB, ob = (e >> 6) / NKB;
    const int row = 32 * ob + icol(l & 31);
    const int k0 = 32 * (kb >> 1) + 16 * (l >> 5) + 8 * (kb & 1);
    const float4 a = *reinterpret_cast<const float4*>(W + row * CI + k0);
    const float4 b = *reinterpret_cast<const float4*>(W + row * CI + k0 + 4);
    s_w[e] = make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
  }
}
// g = dy W: rows = input channels, k = output channels; entry (ib * (CO / 16) + kb) * 64 + lane
template <int CI, int CO>
__device__ __forceinline__ void stage_wt(uint4* s_w, const float* __restrict__ W) {
  constexpr int NKB = CO / 16, NIB = CI / 32;
  for (int e = threadIdx.x; e < NIB * NKB * 64; e += blockDim.x) {
    const int l = e & 63, kb = (e >> 6) % NKB, ib = (e >> 6) / NKB;
    const int col = 32 * ib + icol(l & 31);
    const int k0 = 32 * (kb >> 1) + 16 * (l >> 5) + 8 * (kb & 1);
    float v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) v[s] = W[(k0 + s) * CI + col];
    s_w[e] = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                        pack_bf16x2(v[6], v[7]));
  }
}

// ---- row fragments ----------------------------------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ void load_frag(__amdgpu_buffer_rsrc_t rs, uint32_t row, int h, bf16x8 (&f)[C / 16]) {
#pragma unroll
  for (int nb = 0; nb < C / 32; ++nb) {
    const uint32_t off = row * (uint32_t)(2 * C) + (uint32_t)(64 * nb + 32 * h);
    f[2 * nb] = __builtin_bit_cast(bf16x8, ld128(rs, off));
    f[2 * nb + 1] = __builtin_bit_cast(bf16x8, ld128(rs, off + 16));
  }
}
template <int C>
__device__ __forceinline__ void store_frag(__amdgpu_buffer_rsrc_t rs, uint32_t row, int h, const bf16x8 (&f)[C / 16]) {
#pragma unroll
  for (int nb = 0; nb < C / 32; ++nb) {
    const uint32_t off = row * (uint32_t)(2 * C) + (uint32_t)(64 * nb + 32 * h);
    st128(rs, off, __builtin_bit_cast(u32x4, f[2 * nb]));
    st128(rs, off + 16, __builtin_bit_cast(u32x4, f[2 * nb + 1]));
  }
}
// first channel of k-block kb in lane half h
__device__ __forceinline__ int frag_c0(int kb, int h) { return 32 * (kb >> 1) + 16 * h + 8 * (kb & 1); }

__device__ __forceinline__ void lds8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// acc[ob] = sum_kb W-operand(ob, kb) x a[kb]
template <int NKB, int NOB>
__device__ __forceinline__ void mm(const uint4* s_w, int lane, const bf16x8 (&a)[NKB], f32x16 (&acc)[NOB]) {
  asm volatile("" ::: "memory");      // keep the ds_read_b128 inside the tile loop
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) {
    f32x16 c = zero16();
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) c = CH_MFMA(lds_op(s_w, ob * NKB + kb, lane), a[kb], c);
    acc[ob] = c;
  }
}
// the accumulators rounded to bf16: the fragment that is stored, and the operand of the next product
template <int NOB>
__device__ __forceinline__ void pack_acc(const f32x16 (&acc)[NOB], bf16x8 (&p)[2 * NOB]) {
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) {
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = acc[ob][r];
    p[2 * ob] = pack8(&v[0]);
    p[2 * ob + 1] = pack8(&v[8]);
  }
}

// a = bf16(leaky(BN(y))) of a raw fragment; tab = LDS fp32 [4][C] = mean | invstd | gamma | beta
template <int C>
__device__ __forceinline__ void bn_act_frag(const bf16x8 (&raw)[C / 16], const float* tab, int h, float slope,
                                            uint32_t keep, bf16x8 (&out)[C / 16]) {
  asm volatile("" ::: "memory");      // the constants stay in LDS: 4 C registers otherwise
#pragma unroll
  for (int kb = 0; kb < C / 16; ++kb) {
    const int c0 = frag_c0(kb, h);
    float v[8], mu[8], is[8], ga[8], be[8], o[8];
    unpack8(raw[kb], v);
    lds8(tab + c0, mu);
    lds8(tab + C + c0, is);
    lds8(tab + 2 * C + c0, ga);
    lds8(tab + 3 * C + c0, be);
#pragma unroll
    for (int s = 0; s < 8; ++s) o[s] = rowbn::act(rowbn::affine(rowbn::norm(v[s], mu[s], is[s]), ga[s], be[s]), slope);
    out[kb] = mask8(pack8(o), keep);
  }
}

// ---- statistics -------------------------------------------------------------------------------------------------------
// A lane produces C values per row: value q = stat * (C / 2) + 16 nb + r is one of the two statistics of one of its
// C / 2 channels.  Holding C fp32 sums per lane costs the backward kernel an occupancy step, so a value is first added
// over the four lanes of its quad (two DPP operations) and kept by ONE of them: lane j keeps the values q with
// (q & 3) == (j & 3) in st4[q >> 2] -- C / 4 registers.  qm[k] = 1 for k == (j & 3), else 0.
template <int C>
__device__ __forceinline__ void quad_add(float v, int q, const float (&qm)[4], float (&st4)[C / 4]) {
  v += dpp_mov<0xB1>(v);      // quad_perm [1, 0, 3, 2]
  v += dpp_mov<0x4E>(v);      // quad_perm [2, 3, 0, 1]
  st4[q >> 2] = fmaf(v, qm[q & 3], st4[q >> 2]);
}
// the eight quads of the half-wave (lanes j ^ 4, j ^ 8, j ^ 16 keep the same values), then fp64: of the C / 4 sums
// every lane of a class (j & 3) now holds, lane j adds the C / 32 with index i / (C / 32) == (j >> 2) to its accd
template <int C>
__device__ __forceinline__ void flush_lane_sums(float (&st4)[C / 4], double (&accd)[C / 32], int j) {
  constexpr int ND = C / 32;
#pragma unroll
  for (int i = 0; i < C / 4; ++i) {
    float t = st4[i];
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 8);
    t += __shfl_xor(t, 16);
    if (i / ND == (j >> 2)) accd[i % ND] += (double)t;
    st4[i] = 0.f;
  }
}
// the wavefronts of the block in order (fp64), then one fp64 atomic per (block, value); s_red: WAVES * 2 C doubles
template <int C>
__device__ __forceinline__ void block_sums_out(const double (&accd)[C / 32], double* s_red, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < C / 32; ++d) {
    const int q = 4 * ((j >> 2) * (C / 32) + d) + (j & 3), stat = q / (C / 2), rem = q % (C / 2);
    s_red[wv * 2 * C + stat * C + 32 * (rem >> 4) + 16 * h + (rem & 15)] = accd[d];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
    double a = 0.0;
    for (int w = 0; w < WAVES; ++w) a += s_red[w * 2 * C + i];
    atomicAdd(&sums[i], a);
  }
}

// ---- tile loop ----------------------------------------------------------------------------------------------------------
// Tiles t0, t0 + stride, ... of a wavefront.  PREFETCH: the loads of the next tile are in flight while a tile is
// computed, two register sets in ping-pong (chain::run_tiles has the reason); load() of a tile beyond the last one
// reads no memory (its rows are clamped to R: zeros).
template <typename Pre, bool PREFETCH, typename LoadF, typename BodyF>
__device__ __forceinline__ void run_rows(int t0, int n_tiles, int stride, LoadF&& load, BodyF&& body) {
  if (t0 >= n_tiles) return;
  if (!PREFETCH) {
    for (int t = t0; t < n_tiles; t += stride) {
      const Pre a = load(t);
      body(a);
    }
    return;
  }
  Pre a = load(t0);
  int t = t0 + stride;
  Pre b = load(t);
  body(a);
  while (t < n_tiles) {
    a = load(t + stride);
    body(b);
    t += stride;
    if (t >= n_tiles) break;
    b = load(t + stride);
    body(a);
    t += stride;
  }
}
template <int NA, int NB, int NC>
struct RowsPre {      // the raw fragments of a tile's inputs, the views of the lane's row, the row
  bf16x8 a[NA], b[NB], c[NC];
  float w;
  uint32_t row;
};

// ---- forward: y = bf16(op(in) W^T), op = identity (F1) or bf16(leaky(BN_in(.))) (F2); statistics of y ------------------
template <int CI, int CO, bool ACT>
__global__ __launch_bounds__(64 * WAVES) void fwd_kernel(const bf16_t* __restrict__ in, const float* __restrict__ W,
                                                         const float* __restrict__ bn_in,
                                                         const int32_t* __restrict__ counts, bf16_t* __restrict__ y,
                                                         double* __restrict__ sums, int n_rows, int n_tiles,
                                                         float slope) {
  constexpr int NKB = CI / 16, NOB = CO / 32;
  __shared__ uint4 s_w[NOB * NKB * 64];
  __shared__ __attribute__((aligned(16))) float s_tab[ACT ? 4 * CI : 4];
  __shared__ double s_red[WAVES * 2 * CO];
  stage_w<CI, CO>(s_w, W);
  if (ACT)
    for (int i = threadIdx.x; i < 4 * CI; i += blockDim.x) s_tab[i] = bn_in[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int wave = rfl((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)), n_waves = (int)((gridDim.x * blockDim.x) >> 6);
  const __amdgpu_buffer_rsrc_t r_in = make_rsrc(in, (uint64_t)n_rows * (2 * CI));
  const __amdgpu_buffer_rsrc_t r_y = make_rsrc(y, (uint64_t)n_rows * (2 * CO));
  const __amdgpu_buffer_rsrc_t r_cnt = make_rsrc(counts, counts ? (uint64_t)n_rows * 4 : 0);
  float st[CO / 4], qm[4];
  double accd[CO / 32];
#pragma unroll
  for (int q = 0; q < CO / 4; ++q) st[q] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) qm[k] = (j & 3) == k ? 1.f : 0.f;
#pragma unroll
  for (int d = 0; d < CO / 32; ++d) accd[d] = 0.0;
  int pending = 0;
  typedef RowsPre<NKB, 1, 1> Pre;
  auto load = [&](int t) {
    Pre p;
    p.row = 32u * (uint32_t)t + (uint32_t)j;
    const uint32_t rc = p.row < (uint32_t)n_rows ? p.row : (uint32_t)n_rows;      // a row beyond R loads zeros: y = 0 there
    load_frag<CI>(r_in, rc, h, p.a);
    p.w = counts ? (float)(int)ld32(r_cnt, rc * 4u) : 1.f;
    return p;
  };
  auto body = [&](const Pre& in) {
    const uint32_t row = in.row;
    const uint32_t keep = row < (uint32_t)n_rows ? ~0u : 0u;
    const float w = in.w;
    bf16x8 a[NKB];
    if (ACT) {
      bn_act_frag<CI>(in.a, s_tab, h, slope, keep, a);
    } else {
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) a[kb] = in.a[kb];
    }
    f32x16 acc[NOB];
    mm<NKB, NOB>(s_w, lane, a, acc);
    bf16x8 p[2 * NOB];
    pack_acc<NOB>(acc, p);
    store_frag<CO>(r_y, row, h, p);      // rows beyond R: dropped by the range check
    // statistics of the ROUNDED y: w y and w y^2 are exact in fp32 (8-bit significands, w < 2^5)
#pragma unroll
    for (int kb = 0; kb < 2 * NOB; ++kb) {
      float v[8];
      unpack8(p[kb], v);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int q = 16 * (kb >> 1) + 8 * (kb & 1) + s;
        const float wv = w * v[s];
        quad_add<CO>(wv, q, qm, st);
        quad_add<CO>(wv * v[s], CO / 2 + q, qm, st);
      }
    }
    if (++pending == FLUSH_TILES) {
      flush_lane_sums<CO>(st, accd, j);
      pending = 0;
    }
  };
  run_rows<Pre, true>(wave, n_tiles, n_waves, load, body);
  flush_lane_sums<CO>(st, accd, j);
  block_sums_out<CO>(accd, s_red, sums);
}

// ---- backward of one block: dy = BatchNorm-backward(g leaky'(z)) [R, CO], dW += dy^T op(xin), gx = bf16(dy W) [R, CI];
// ACT (B2): op = bf16(leaky(BN_in(.))) and the statistics of gx leaky'(z_in) for the BatchNorm below --------------------
template <int CI, int CO, bool ACT>
__global__ __launch_bounds__(64 * WAVES, 2) void bwd_kernel(
    const bf16_t* __restrict__ gin, const bf16_t* __restrict__ y, const float* __restrict__ bn,
    const float* __restrict__ sm, const int32_t* __restrict__ counts, const bf16_t* __restrict__ xin,
    const float* __restrict__ bn_in, const float* __restrict__ W, bf16_t* __restrict__ gx, float* __restrict__ dw_ws,
    double* __restrict__ sums, int n_rows, int n_tiles, float slope, float slope_in) {
  constexpr int NKO = CO / 16, NKI = CI / 16, NBO = CO / 32, NBI = CI / 32;
  constexpr int TILE = 32 * TSB;                       // bf16 elements of one 32-row x 32-channel natural tile
  constexpr int WAVE_TILES = (NBO + NBI) * TILE;
  static_assert(WAVES * WAVE_TILES * 2 >= CO * CI * 4, "the block's dW sum reuses the tile memory");
  __shared__ uint4 s_wt[NBI * NKO * 64];
  __shared__ __attribute__((aligned(16))) float s_tab[6 * CO];      // mean | invstd | gamma | beta | S1/n | S2/n
  __shared__ __attribute__((aligned(16))) float s_tin[ACT ? 4 * CI : 4];
  __shared__ __attribute__((aligned(16))) bf16_t s_tiles[WAVES * WAVE_TILES];
  __shared__ double s_red[ACT ? WAVES * 2 * CI : 1];
  stage_wt<CI, CO>(s_wt, W);
  for (int i = threadIdx.x; i < 4 * CO; i += blockDim.x) s_tab[i] = bn[i];
  for (int i = threadIdx.x; i < 2 * CO; i += blockDim.x) s_tab[4 * CO + i] = sm[i];
  if (ACT)
    for (int i = threadIdx.x; i < 4 * CI; i += blockDim.x) s_tin[i] = bn_in[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
  const int wave = rfl((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)), n_waves = (int)((gridDim.x * blockDim.x) >> 6);
  const __amdgpu_buffer_rsrc_t r_g = make_rsrc(gin, (uint64_t)n_rows * (2 * CO));
  const __amdgpu_buffer_rsrc_t r_y = make_rsrc(y, (uint64_t)n_rows * (2 * CO));
  const __amdgpu_buffer_rsrc_t r_x = make_rsrc(xin, (uint64_t)n_rows * (2 * CI));
  const __amdgpu_buffer_rsrc_t r_gx = make_rsrc(gx, gx ? (uint64_t)n_rows * (2 * CI) : 0);
  const __amdgpu_buffer_rsrc_t r_cnt = make_rsrc(counts, counts ? (uint64_t)n_rows * 4 : 0);
  bf16_t* t_dy = s_tiles + wv * WAVE_TILES;
  bf16_t* t_x = t_dy + NBO * TILE;
  f32x16 dw[NBO][NBI];
#pragma unroll
  for (int ob = 0; ob < NBO; ++ob)
#pragma unroll
    for (int ib = 0; ib < NBI; ++ib) dw[ob][ib] = zero16();
  constexpr int NST = ACT ? CI : 32;
  float st[NST / 4], qm[4];
  double accd[NST / 32];
#pragma unroll
  for (int q = 0; q < NST / 4; ++q) st[q] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) qm[k] = (j & 3) == k ? 1.f : 0.f;
#pragma unroll
  for (int d = 0; d < NST / 32; ++d) accd[d] = 0.0;
  int pending = 0;
  // registers: the 64 x 64 pass with the statistics has no room for a second set of inputs at two wavefronts per SIMD
  constexpr bool PREFETCH = !(ACT && CI == 64 && CO == 64);
  typedef RowsPre<NKO, NKO, NKI> Pre;
  auto load = [&](int t) {
    Pre p;
    p.row = 32u * (uint32_t)t + (uint32_t)j;
    const uint32_t rc = p.row < (uint32_t)n_rows ? p.row : (uint32_t)n_rows;
    load_frag<CO>(r_g, rc, h, p.a);
    load_frag<CO>(r_y, rc, h, p.b);
    load_frag<CI>(r_x, rc, h, p.c);
    p.w = counts ? (float)(int)ld32(r_cnt, rc * 4u) : 1.f;
    return p;
  };
  auto body = [&](const Pre& in) {
    const uint32_t row = in.row;
    const uint32_t keep = row < (uint32_t)n_rows ? ~0u : 0u;
    const float w = in.w;
    const bf16x8 (&g)[NKO] = in.a;
    const bf16x8 (&yr)[NKO] = in.b;
    const bf16x8 (&xr)[NKI] = in.c;
    // dy, rounded to bf16; zero in the rows beyond R (w = 1 there when there are no counts)
    bf16x8 dyp[NKO];
    asm volatile("" ::: "memory");
#pragma unroll
    for (int kb = 0; kb < NKO; ++kb) {
      const int c0 = frag_c0(kb, h);
      float gv[8], v[8], mu[8], is[8], ga[8], be[8], s1[8], s2[8], o[8];
      unpack8(g[kb], gv);
      unpack8(yr[kb], v);
      lds8(s_tab + c0, mu);
      lds8(s_tab + CO + c0, is);
      lds8(s_tab + 2 * CO + c0, ga);
      lds8(s_tab + 3 * CO + c0, be);
      lds8(s_tab + 4 * CO + c0, s1);
      lds8(s_tab + 5 * CO + c0, s2);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float a = rowbn::norm(v[s], mu[s], is[s]);
        const float z = rowbn::affine(a, ga[s], be[s]);
        const float dz = gv[s] * rowbn::dact(z, slope);
        o[s] = rowbn::grad_y(dz, a, w, ga[s], is[s], s1[s], s2[s]);
      }
      dyp[kb] = mask8(pack8(o), keep);
    }
    // the other factor of the weight gradient (finite in the rows beyond R, where dy is zero)
    bf16x8 xp[NKI];
    if (ACT) {
      bn_act_frag<CI>(xr, s_tin, h, slope_in, ~0u, xp);
    } else {
#pragma unroll
      for (int kb = 0; kb < NKI; ++kb) xp[kb] = xr[kb];
    }
#pragma unroll
    for (int ob = 0; ob < NBO; ++ob) {
      const bf16x8 two[2] = {dyp[2 * ob], dyp[2 * ob + 1]};
      tileN_put_packed(t_dy + ob * TILE, j, h, two);
    }
#pragma unroll
    for (int ib = 0; ib < NBI; ++ib) {
      const bf16x8 two[2] = {xp[2 * ib], xp[2 * ib + 1]};
      tileN_put_packed(t_x + ib * TILE, j, h, two);
    }
    wave_sync();
#pragma unroll
    for (int ob = 0; ob < NBO; ++ob)
#pragma unroll
      for (int ib = 0; ib < NBI; ++ib) dw[ob][ib] = wgradN(t_dy + ob * TILE, t_x + ib * TILE, lane, dw[ob][ib]);
    wave_sync();      // the transpose reads are issued before the next tile's stores (DS operations of a wavefront run in order)
    if (gx) {
      f32x16 acc[NBI];
      mm<NKO, NBI>(s_wt, lane, dyp, acc);
      bf16x8 p[NKI];
      pack_acc<NBI>(acc, p);
      store_frag<CI>(r_gx, row, h, p);
      if (ACT) {
        // dz_in = gx (as stored) leaky'(z_in): S1 += dz_in, S2 += dz_in a_in -- the arithmetic of rowbn_bwd_stats
        asm volatile("" ::: "memory");
#pragma unroll
        for (int kb = 0; kb < NKI; ++kb) {
          const int c0 = frag_c0(kb, h);
          float gv[8], v[8], mu[8], is[8], ga[8], be[8];
          unpack8(p[kb], gv);
          unpack8(xr[kb], v);
          lds8(s_tin + c0, mu);
          lds8(s_tin + CI + c0, is);
          lds8(s_tin + 2 * CI + c0, ga);
          lds8(s_tin + 3 * CI + c0, be);
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const int q = 16 * (kb >> 1) + 8 * (kb & 1) + s;
            const float a = rowbn::norm(v[s], mu[s], is[s]);
            const float z = rowbn::affine(a, ga[s], be[s]);
            const float dz = gv[s] * rowbn::dact(z, slope_in);
            quad_add<NST>(dz, q, qm, st);
            quad_add<NST>(dz * a, CI / 2 + q, qm, st);
          }
        }
        if (++pending == FLUSH_TILES) {
          flush_lane_sums<NST>(st, accd, j);
          pending = 0;
        }
      }
    }
  };
  run_rows<Pre, PREFETCH>(wave, n_tiles, n_waves, load, body);
  if (ACT) {
    flush_lane_sums<NST>(st, accd, j);
    block_sums_out<NST>(accd, s_red, sums);
  }
  // the block's weight gradient: wavefront after wavefront into one fp32 [CO][CI] image (over the tile memory), then
  // this block's slice of the workspace
  float* s_dw = reinterpret_cast<float*>(s_tiles);
  for (int turn = 0; turn < WAVES; ++turn) {
    __syncthreads();
    if (wv == turn) {
#pragma unroll
      for (int ob = 0; ob < NBO; ++ob)
#pragma unroll
        for (int ib = 0; ib < NBI; ++ib)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float* p = s_dw + (32 * ob + chan(r, h)) * CI + 32 * ib + j;
            *p = turn == 0 ? dw[ob][ib][r] : *p + dw[ob][ib][r];
          }
    }
  }
  __syncthreads();
  float* out = dw_ws + (size_t)blockIdx.x * (CO * CI);
  for (int i = threadIdx.x; i < CO * CI; i += blockDim.x) out[i] = s_dw[i];
}

// out[i] = sum_p ws[p][i], p ascending inside each of 16 slices, the slices in order: 16 elements x 16 slices per block
__global__ __launch_bounds__(256) void dw_reduce_kernel(const float* __restrict__ ws_a, int n_a, int parts_a,
                                                        float* __restrict__ out_a, const float* __restrict__ ws_b,
                                                        int n_b, int parts_b, float* __restrict__ out_b) {
  __shared__ float s_part[16][17];
  const int e = threadIdx.x & 15, s = threadIdx.x >> 4;
  int i = blockIdx.x * 16 + e;
  const bool first = i < n_a;
  const float* ws = first ? ws_a : ws_b;
  float* out = first ? out_a : out_b;
  const int n = first ? n_a : n_b, parts = first ? parts_a : parts_b;
  if (!first) i -= n_a;
  float acc = 0.f;
  if (i < n)
    for (int p = s; p < parts; p += 16) acc += ws[(size_t)p * n + i];
  s_part[s][e] = acc;
  __syncthreads();
  if (s == 0 && i < n) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) a += s_part[q][e];
    out[i] = a;
  }
}

static inline int rows_grid(int64_t R, int backward, int max_blocks) {
  // two blocks per CU: four tiles per wavefront at the headline size (the fixed costs of a block -- staging the
  // operands, the fp64 atomics, the weight-gradient partial -- weigh less; the next tile's loads are in flight)
  (void)backward;
  int64_t b = chain_grid(2);
  const int64_t need = (R + 32 * WAVES - 1) / (32 * WAVES);
  if (b > need) b = need;
  if (max_blocks > 0 && b > max_blocks) b = max_blocks;
  return (int)(b < 1 ? 1 : b);
}
static inline bool width_ok(int c) { return c == 32 || c == 64; }
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// every byte offset of a tile's rows, the ones beyond R included, must stay below 2^32
static inline bool rows_ok(int64_t R) { return (R + 32) * 128 <= 0xfffffff0ll; }

}  // namespace emod_rows
}  // namespace dva

using namespace dva;
using namespace dva::emod_rows;

extern "C" {

int dva_emod_rows_grid(int64_t R, int32_t backward, int32_t max_blocks) {
  if (R < 0 || max_blocks < 0) return DVA_ERR_INVALID;
  return rows_grid(R, backward, max_blocks);
}

int dva_emod_rows_fwd(const void* in, const float* W, const float* bn_in, const int32_t* counts, void* y,
                      double* sums, int64_t R, int32_t C_in, int32_t C_out, float slope, int32_t max_blocks,
                      void* stream) {
  if (R < 0 || max_blocks < 0) return DVA_ERR_INVALID;
  if (!width_ok(C_in) || !width_ok(C_out)) return DVA_ERR_UNSUPPORTED;
  if (R == 0) return DVA_OK;
  if (!in || !W || !y || !sums || !al16(in) || !al16(W) || !al16(y) || ((uintptr_t)counts & 3)) return DVA_ERR_INVALID;
  if (!rows_ok(R)) return DVA_ERR_UNSUPPORTED;
  const dim3 grid(rows_grid(R, 0, max_blocks)), block(64 * WAVES);
  const int n_rows = (int)R, n_tiles = (int)((R + 31) / 32);
#define DVA_EMOD_FWD(CI_, CO_)                                                                                     \
  do {                                                                                                             \
    if (bn_in)                                                                                                     \
      hipLaunchKernelGGL((fwd_kernel<CI_, CO_, true>), grid, block, 0, (hipStream_t)stream, (const bf16_t*)in, W,  \
                         bn_in, counts, (bf16_t*)y, sums, n_rows, n_tiles, slope);                                 \
    else                                                                                                           \
      hipLaunchKernelGGL((fwd_kernel<CI_, CO_, false>), grid, block, 0, (hipStream_t)stream, (const bf16_t*)in, W, \
                         bn_in, counts, (bf16_t*)y, sums, n_rows, n_tiles, slope);                                 \
  } while (0)
  if (C_in == 32 && C_out == 32) DVA_EMOD_FWD(32, 32);
  else if (C_in == 32) DVA_EMOD_FWD(32, 64);
  else if (C_out == 32) DVA_EMOD_FWD(64, 32);
  else DVA_EMOD_FWD(64, 64);
#undef DVA_EMOD_FWD
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_emod_rows_bwd(const void* grad_in, const void* y, const float* bn, const float* sm, const int32_t* counts,
                      const void* x_in, const float* bn_in, const float* W, void* grad_x, float* dw_ws,
                      double* sums, int64_t R, int32_t C_in, int32_t C_out, float slope, float slope_in,
                      int32_t max_blocks, void* stream) {
  if (R < 0 || max_blocks < 0) return DVA_ERR_INVALID;
  if (!width_ok(C_in) || !width_ok(C_out)) return DVA_ERR_UNSUPPORTED;
  if (!dw_ws) return DVA_ERR_INVALID;
  if (R == 0) return DVA_OK;      // nothing is written: a caller with no rows has no partials to reduce
  if (!grad_in || !y || !bn || !sm || !x_in || !W || !al16(grad_in) || !al16(y) || !al16(x_in) || !al16(W) ||
      !al16(grad_x) || !al16(dw_ws) || ((uintptr_t)counts & 3))
    return DVA_ERR_INVALID;
  if (bn_in && (!sums || !grad_x)) return DVA_ERR_INVALID;
  if (!rows_ok(R)) return DVA_ERR_UNSUPPORTED;
  const dim3 grid(rows_grid(R, 1, max_blocks)), block(64 * WAVES);
  const int n_rows = (int)R, n_tiles = (int)((R + 31) / 32);
#define DVA_EMOD_BWD(CI_, CO_)                                                                                       \
  do {                                                                                                               \
    if (bn_in)                                                                                                       \
      hipLaunchKernelGGL((bwd_kernel<CI_, CO_, true>), grid, block, 0, (hipStream_t)stream, (const bf16_t*)grad_in,  \
                         (const bf16_t*)y, bn, sm, counts, (const bf16_t*)x_in, bn_in, W, (bf16_t*)grad_x, dw_ws,    \
                         sums, n_rows, n_tiles, slope, slope_in);                                                    \
    else                                                                                                             \
      hipLaunchKernelGGL((bwd_kernel<CI_, CO_, false>), grid, block, 0, (hipStream_t)stream, (const bf16_t*)grad_in, \
                         (const bf16_t*)y, bn, sm, counts, (const bf16_t*)x_in, bn_in, W, (bf16_t*)grad_x, dw_ws,    \
                         sums, n_rows, n_tiles, slope, slope_in);                                                    \
  } while (0)
  if (C_in == 32 && C_out == 32) DVA_EMOD_BWD(32, 32);
  else if (C_in == 32) DVA_EMOD_BWD(32, 64);
  else if (C_out == 32) DVA_EMOD_BWD(64, 32);
  else DVA_EMOD_BWD(64, 64);
#undef DVA_EMOD_BWD
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_emod_rows_dw_reduce(const float* ws_a, int32_t n_a, int32_t parts_a, float* out_a, const float* ws_b,
                            int32_t n_b, int32_t parts_b, float* out_b, void* stream) {
  if (n_a < 0 || n_b < 0 || parts_a < 0 || parts_b < 0) return DVA_ERR_INVALID;
  if ((n_a > 0 && (!ws_a || !out_a)) || (n_b > 0 && (!ws_b || !out_b))) return DVA_ERR_INVALID;
  if (n_a + n_b == 0) return DVA_OK;
  // n_a a multiple of 16 keeps the two matrices in separate blocks' elements (C_out C_in always is)
  if (n_a % 16) return DVA_ERR_INVALID;
  hipLaunchKernelGGL(dw_reduce_kernel, dim3((n_a + n_b + 15) / 16), dim3(256), 0, (hipStream_t)stream, ws_a, (int)n_a,
                     (int)parts_a, out_a, ws_b, (int)n_b, (int)parts_b, out_b);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
