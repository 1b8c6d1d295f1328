// Lazy bilinear gather fused with the max / mean / sum / min pool behind it, for gfx950 (reference: x_mod =
// sparse_interpolation(x, coords, batch), core/multimodal/image.py:105-170, followed by BimodalCSRPool(mode) =
// torch_scatter.segment_csr over the items of each segment, modules/multimodal/pooling.py:14-71).
//
// forward   out[s][c] = reduce over the items p in [seg_ptr[s], seg_ptr[s + 1]) of v(p, c),
//           v(p, c) = ((w0 x0 + w1 x1) + w2 x2) + w3 x3, x_k = rows[tap_rows[p][k]][c], rounded to the storage type
// backward  grad_rows[r][c] = sum over the taps (p, k) with tap_rows[p][k] == r of tap_weights[p][k] g(p, c)
//
// No [P, C] tensor in either direction.  The forward evaluates every item as gather_bilinear_fwd_kernel does (products
// and sums rounded one by one, then one rounding to the storage type, which is what the [P, C] tensor would have held) and
// reduces the items as dva_segment_csr_fwd does (fp32 accumulation from 0 in item order, one division for the mean, one
// rounding; max / min: first item on ties, a NaN wins only as the first item), so it equals the materialised composition
// bit for bit.  One wavefront owns a segment: its 64 / lpr slots interpolate that many items at once (the loads, which are
// what takes the time, overlap), then the slots' values are folded into the accumulator one after the other IN ITEM ORDER
// through wave shuffles -- the order of the additions is that of the one-lane loop, the latency is not.
// The backward is a segmented reduction over the row plan of the 4 P taps (perm = taps sorted by map row, row_ptr): one
// wavefront per map row, fp32 accumulators, every element of grad_rows written once in the rows' storage type -- no float
// atomics, so two runs agree bit for bit.  Where C / VEC is a power of two <= 64 (fp32, bf16) the caller takes the anchor
// plan instead (interp_anchor_sum_kernel below + dva_anchor_combine + interp_anchor_fixup_kernel): P keys, every gradient
// row read once per item.
//
// Bytes: forward P (32 + 4 C s) [taps; four map rows per item, out of the cache hierarchy] + S (8 + C s) (+ 2 S C: the arg
//        offsets of max / min);
//        backward 4 P (12 + C s) [plan entry, weight, segment of the item; gradient rows of the segments, cached]
//        (+ 32 P: mean / max / min read seg_ptr, + 8 P C: max / min read the arg rows) + R (4 + C s);
//        on the anchor plan P (24 + C s) (+ 16 P, + 2 P C) + A (4 + 32 C) [per-anchor sums written and read] + 4 R C.
#include "dva_common.h"
#include "row_chunk.h"

namespace dva {

// The value the [P, C] tensor of storage type T would have held.
template <typename T>
__device__ __forceinline__ float stored_value(float v);
template <>
__device__ __forceinline__ float stored_value<float>(float v) { return v; }
template <>
__device__ __forceinline__ float stored_value<bf16_t>(float v) { return bf2f(f2bf(v)); }
template <>
__device__ __forceinline__ float stored_value<f16_t>(float v) { return (float)(f16_t)v; }

// One wavefront per segment s.  lpr lanes (a power of two) own the VEC-channel chunks of a row, the 64 / lpr slots take
// consecutive items; rows wider than lpr chunks are walked in column passes of lpr chunks.
template <typename T, int VEC, int REDUCE>
__global__ __launch_bounds__(256) void interp_segment_reduce_fwd_kernel(
    const T* __restrict__ rows, const int4* __restrict__ tap_rows, const float4* __restrict__ tap_weights,
    const int64_t* __restrict__ seg_ptr, T* __restrict__ out, uint16_t* __restrict__ arg, int64_t S, int C, int lpr) {
  const int chunks = C / VEC;
  const int lane = threadIdx.x & 63;
  const int lane_r = lane & (lpr - 1), slot = lane / lpr, slots = 64 / lpr;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = wave; s < S; s += n_waves) {
    const int64_t beg = seg_ptr[s], end = seg_ptr[s + 1];
    for (int ch0 = 0; ch0 < chunks; ch0 += lpr) {
      const bool live = ch0 + lane_r < chunks;                 // lanes behind the last chunk of the row idle along
      const int64_t col = (int64_t)(live ? ch0 + lane_r : 0) * VEC;
      float acc[VEC];
      uint32_t best[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        acc[k] = 0.f;
        best[k] = 0xffffu;
      }
      for (int64_t i0 = beg; i0 < end; i0 += slots) {
        const int64_t p = i0 + slot < end ? i0 + slot : beg;   // slots behind the segment's end repeat an item, unused
        const int4 tr = tap_rows[p];
        const float4 tw = tap_weights[p];
        float x0[VEC], x1[VEC], x2[VEC], x3[VEC], v[VEC];
        RowChunk<T, VEC>::ld(rows + (int64_t)tr.x * C + col, x0);
        RowChunk<T, VEC>::ld(rows + (int64_t)tr.y * C + col, x1);
        RowChunk<T, VEC>::ld(rows + (int64_t)tr.z * C + col, x2);
        RowChunk<T, VEC>::ld(rows + (int64_t)tr.w * C + col, x3);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          float a = __fmul_rn(tw.x, x0[k]);
          a = __fadd_rn(a, __fmul_rn(tw.y, x1[k]));
          a = __fadd_rn(a, __fmul_rn(tw.z, x2[k]));
          v[k] = stored_value<T>(__fadd_rn(a, __fmul_rn(tw.w, x3[k])));
        }
        const int n = end - i0 < slots ? (int)(end - i0) : slots;      // wave-uniform
        for (int j = 0; j < n; ++j) {
          const int src = j * lpr + lane_r;
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            pool_step<REDUCE>(acc[k], best[k], __shfl(v[k], src), i0 + j == beg, (uint32_t)(i0 + j - beg));
        }
      }
      if (REDUCE == DVA_MEAN && end > beg) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] /= (float)(end - beg);
      }
      if (slot == 0 && live) {
        RowChunk<T, VEC>::st(out + s * C + col, acc);
        if (keeps_arg(REDUCE)) RowChunk<T, VEC>::st_arg(arg + s * C + col, best);
      }
    }
  }
}

// One wavefront per map row r: its taps perm[row_ptr[r] .. row_ptr[r + 1]) are spread over 64 / lpr slots, lpr lanes own the
// VEC-channel chunks of a row, wider rows are walked in column passes.  Tap t = 4 p + k of item p of segment s =
// seg_of_item[p] contributes tap_weights[t] times grad_out[s][c] (sum), grad_out[s][c] / count_s (mean, fp32 true division as
// segment_csr_bwd_kernel) or grad_out[s][c] where arg[s][c] == p - seg_ptr[s] (max / min).  The slots are summed with
// wave64 xor shuffles in a fixed order.
template <typename T, int VEC, int REDUCE>
__global__ __launch_bounds__(256) void interp_segment_reduce_bwd_kernel(
    const T* __restrict__ gout, const uint16_t* __restrict__ arg, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ row_ptr, const float* __restrict__ tap_weights,
    const int32_t* __restrict__ seg_of_item, T* __restrict__ grows, int64_t R, int C, int lpr) {
  constexpr int U = 2;
  const int chunks = C / VEC;
  const int lane = threadIdx.x & 63;
  const int lane_r = lane & (lpr - 1), slot = lane / lpr, slots = 64 / lpr;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < R; r += n_waves) {
    const int beg = row_ptr[r], end = row_ptr[r + 1];
    for (int ch0 = 0; ch0 < chunks; ch0 += lpr) {
      const bool live = ch0 + lane_r < chunks;
      const int64_t col = (int64_t)(live ? ch0 + lane_r : 0) * VEC;
      float acc[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      for (int i0 = beg; i0 < end; i0 += slots * U) {
        int64_t s[U];
        uint32_t koff[U];
        float w[U], count[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * slots + slot;
          ok[u] = i < end && live;
          const int t = perm[i < end ? i : beg];
          const int p = t >> 2;
          w[u] = tap_weights[t];
          s[u] = seg_of_item[p];
          koff[u] = 0xfffeu;                                   // 0xfffe never is a stored offset
          count[u] = 1.f;
          if (REDUCE != DVA_SUM) {
            const int64_t sb = seg_ptr[s[u]];
            if (REDUCE == DVA_MEAN) count[u] = (float)(seg_ptr[s[u] + 1] - sb);
            if (keeps_arg(REDUCE)) koff[u] = (uint32_t)((int64_t)p - sb);
          }
        }
        float g[U][VEC];
        uint32_t ak[U][VEC] = {};
#pragma unroll
        for (int u = 0; u < U; ++u) {
          RowChunk<T, VEC>::ld(gout + s[u] * C + col, g[u]);
          if (keeps_arg(REDUCE)) RowChunk<T, VEC>::ld_arg(arg + s[u] * C + col, ak[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const float term = pool_term<REDUCE>(g[u][k], w[u], count[u], ak[u][k], koff[u]);
            acc[k] += ok[u] ? term : 0.f;
          }
        }
      }
      for (int off = lpr; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += __shfl_xor(acc[k], off);
      }
      if (slot == 0 && live) RowChunk<T, VEC>::st(grows + r * C + col, acc);
    }
  }
}

// The backward over the ANCHOR plan (views grouped by the padded cell of their top-left tap, as dva_anchor_rows_sum has it
// for the materialised gradient): one wavefront per anchor a, S[a][k][:] = sum over the items p of anchor a of
// tap_weights[p][k] g(p, :) for the four taps k, g evaluated on the fly as above.  P keys to sort instead of 4 P, and the
// gradient row of an item's segment is read once instead of four times; the map gradient follows from S by
// dva_anchor_combine.  C / VEC lanes (a power of two <= 64) cover a row.
template <typename T, int VEC, int REDUCE>
__global__ __launch_bounds__(256) void interp_anchor_sum_kernel(
    const T* __restrict__ gout, const uint16_t* __restrict__ arg, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ row_ptr, const float4* __restrict__ tap_weights,
    const int32_t* __restrict__ seg_of_item, float* __restrict__ S, int64_t A, int C, int lpr) {
  constexpr int U = 2;
  const int lane = threadIdx.x & 63;
  const int lane_r = lane & (lpr - 1), slot = lane / lpr, slots = 64 / lpr;
  const int64_t col = (int64_t)lane_r * VEC;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t a = wave; a < A; a += n_waves) {
    const int beg = row_ptr[a], end = row_ptr[a + 1];
    float acc[4][VEC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[k][e] = 0.f;
    }
    for (int i0 = beg; i0 < end; i0 += slots * U) {
      int64_t s[U];
      uint32_t koff[U];
      float count[U];
      float4 w[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * slots + slot;
        ok[u] = i < end;
        const int p = perm[ok[u] ? i : beg];
        w[u] = tap_weights[p];
        s[u] = seg_of_item[p];
        koff[u] = 0xfffeu;
        count[u] = 1.f;
        if (REDUCE != DVA_SUM) {
          const int64_t sb = seg_ptr[s[u]];
          if (REDUCE == DVA_MEAN) count[u] = (float)(seg_ptr[s[u] + 1] - sb);
          if (keeps_arg(REDUCE)) koff[u] = (uint32_t)((int64_t)p - sb);
        }
      }
      float g[U][VEC];
      uint32_t ak[U][VEC] = {};
#pragma unroll
      for (int u = 0; u < U; ++u) {
        RowChunk<T, VEC>::ld(gout + s[u] * C + col, g[u]);
        if (keeps_arg(REDUCE)) RowChunk<T, VEC>::ld_arg(arg + s[u] * C + col, ak[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float ww[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float term = pool_term<REDUCE>(g[u][e], 1.f, count[u], ak[u][e], koff[u]);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k][e] += ok[u] ? ww[k] * term : 0.f;
        }
      }
    }
    for (int off = lpr; off < 64; off <<= 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[k][e] += __shfl_xor(acc[k][e], off);
      }
    }
    if (slot == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float* dst = S + (a * 4 + k) * C + col;
#pragma unroll
        for (int e = 0; e < VEC; e += 4)
          *reinterpret_cast<float4*>(dst + e) = make_float4(acc[k][e], acc[k][e + 1], acc[k][e + 2], acc[k][e + 3]);
      }
    }
  }
}

// The items of the dummy anchor (no 2 x 2 tap block: dva_anchor_combine cannot place them), tap by tap into the fp32 map
// gradient that dva_anchor_combine wrote.  One block; thread c owns channel c and walks the items in plan order, so no two
// threads touch an element and the order of the additions is fixed (real data holds no such item, a test a handful).
template <typename T, int REDUCE>
__global__ __launch_bounds__(256) void interp_anchor_fixup_kernel(
    const T* __restrict__ gout, const uint16_t* __restrict__ arg, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ tap_rows,
    const float* __restrict__ tap_weights, const int32_t* __restrict__ seg_of_item, float* __restrict__ dY, int64_t dummy,
    int C) {
  const int beg = row_ptr[dummy], end = row_ptr[dummy + 1];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    for (int i = beg; i < end; ++i) {
      const int64_t p = perm[i];
      const int64_t s = seg_of_item[p];
      const float count = REDUCE == DVA_MEAN ? (float)(seg_ptr[s + 1] - seg_ptr[s]) : 1.f;
      const uint32_t ak = keeps_arg(REDUCE) ? arg[s * C + c] : 0u, koff = (uint16_t)(p - seg_ptr[s]);
      const float g = pool_term<REDUCE>(Elt<T>::ld(gout, s * C + c), 1.f, count, ak, koff);
      for (int k = 0; k < 4; ++k) dY[(int64_t)tap_rows[4 * p + k] * C + c] += tap_weights[4 * p + k] * g;
    }
  }
}

}  // namespace dva

using namespace dva;

extern "C" {

int dva_interp_segment_reduce_fwd(const void* rows, const int32_t* tap_rows, const float* tap_weights,
                                  const int64_t* seg_ptr, void* out, void* arg, int64_t S, int64_t P, int64_t R, int32_t C,
                                  int32_t dtype, int32_t reduce, void* stream) {
  int rc = check_sizes(S, P, R, C, dtype, reduce);
  if (rc) return rc;
  if (S > 0 && C > 0 &&
      (!seg_ptr || !out || (keeps_arg(reduce) && !arg) || (P > 0 && (!rows || !tap_rows || !tap_weights))))
    return DVA_ERR_INVALID;
  if (S > POOL_SIZE_MAX || P > POOL_SIZE_MAX / 4 || R > POOL_SIZE_MAX) return DVA_ERR_UNSUPPORTED;
  if (S == 0 || C == 0) return DVA_OK;
  hipStream_t s = (hipStream_t)stream;
  // the taps are read as 16-byte records on both paths: [P, 4] tensors of 4-byte elements
  if (P > 0 && (!aligned16(tap_rows) || !aligned16(tap_weights))) return DVA_ERR_UNSUPPORTED;
  const bool wide = C % row_vec(dtype) == 0 && aligned16(rows) && aligned16(out) && aligned16(arg);
  const dim3 grid(capped_grid(S, 4, GRID_CAP));      // four wavefronts, four segments per block
  with_row_type(dtype, wide, [&](auto row) {
    using T = typename decltype(row)::T;
    constexpr int VEC = decltype(row)::VEC;
    with_reduce(reduce, [&](auto rd) {
      hipLaunchKernelGGL((interp_segment_reduce_fwd_kernel<T, VEC, decltype(rd)::value>), grid, dim3(256), 0, s,
                         (const T*)rows, (const int4*)tap_rows, (const float4*)tap_weights, seg_ptr, (T*)out,
                         (uint16_t*)arg, S, (int)C, lanes_per_row(C / VEC));
    });
  });
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_interp_segment_reduce_bwd(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                                  const int32_t* row_ptr, const float* tap_weights, const int32_t* seg_of_item,
                                  void* grad_rows, int64_t S, int64_t P, int64_t R, int32_t C, int32_t dtype,
                                  int32_t reduce, void* stream) {
  int rc = check_sizes(S, P, R, C, dtype, reduce);
  if (rc) return rc;
  if (S > 0 && C > 0 && R > 0 &&
      (!grad_rows || !row_ptr ||
       (P > 0 && (!grad_out || !seg_ptr || !perm || !tap_weights || !seg_of_item || (keeps_arg(reduce) && !arg)))))
    return DVA_ERR_INVALID;
  if (S > POOL_SIZE_MAX || P > POOL_SIZE_MAX / 4 || R > POOL_SIZE_MAX) return DVA_ERR_UNSUPPORTED;
  if (R == 0 || C == 0) return DVA_OK;
  if (!grad_rows || !row_ptr) return DVA_ERR_INVALID;     // S == 0: every row still gets its zeros
  hipStream_t s = (hipStream_t)stream;
  const bool wide = C % row_vec(dtype) == 0 && aligned16(grad_out) && aligned16(grad_rows) && aligned16(arg);
  const dim3 grid(capped_grid(R, 4, GRID_CAP));      // four wavefronts, four map rows per block
  with_row_type(dtype, wide, [&](auto row) {
    using T = typename decltype(row)::T;
    constexpr int VEC = decltype(row)::VEC;
    with_reduce(reduce, [&](auto rd) {
      hipLaunchKernelGGL((interp_segment_reduce_bwd_kernel<T, VEC, decltype(rd)::value>), grid, dim3(256), 0, s,
                         (const T*)grad_out, (const uint16_t*)arg, seg_ptr, perm, row_ptr, tap_weights, seg_of_item,
                         (T*)grad_rows, R, (int)C, lanes_per_row(C / VEC));
    });
  });
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_interp_anchor_rows_sum(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                               const int32_t* row_ptr, const float* tap_weights, const int32_t* seg_of_item, float* S,
                               int64_t n_anchors, int64_t P, int32_t C, int32_t dtype, int32_t reduce, void* stream) {
  int rc = check_sizes(n_anchors, P, 0, C, dtype, reduce);
  if (rc) return rc;
  if (n_anchors > 0 && C > 0 &&
      (!row_ptr || !S ||
       (P > 0 && (!grad_out || !seg_ptr || !perm || !tap_weights || !seg_of_item || (keeps_arg(reduce) && !arg)))))
    return DVA_ERR_INVALID;
  if (dtype == DVA_F16 || n_anchors > POOL_SIZE_MAX || P > POOL_SIZE_MAX) return DVA_ERR_UNSUPPORTED;
  if (n_anchors == 0 || C == 0) return DVA_OK;
  const int vec = row_vec(dtype), lpr = C / vec;
  if (C % vec || (lpr & (lpr - 1)) || lpr > 64 || !aligned16(grad_out) || !aligned16(S) || !aligned16(arg) ||
      !aligned16(tap_weights))
    return DVA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(capped_grid(n_anchors, 4, GRID_CAP));
  auto launch = [&](auto row) {
    using T = typename decltype(row)::T;
    constexpr int VEC = decltype(row)::VEC;
    with_reduce(reduce, [&](auto rd) {
      hipLaunchKernelGGL((interp_anchor_sum_kernel<T, VEC, decltype(rd)::value>), grid, dim3(256), 0, s,
                         (const T*)grad_out, (const uint16_t*)arg, seg_ptr, perm, row_ptr, (const float4*)tap_weights,
                         seg_of_item, S, n_anchors, (int)C, lpr);
    });
  };
  if (dtype == DVA_F32) launch(RowType<float, 4>{});
  else launch(RowType<bf16_t, 8>{});
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_interp_anchor_fixup(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                            const int32_t* row_ptr, const int32_t* tap_rows, const float* tap_weights,
                            const int32_t* seg_of_item, float* grad_rows, int64_t dummy, int64_t P, int32_t C,
                            int32_t dtype, int32_t reduce, void* stream) {
  int rc = check_sizes(dummy, P, 0, C, dtype, reduce);
  if (rc) return rc;
  if (dtype == DVA_F16 || dummy >= POOL_SIZE_MAX || P > POOL_SIZE_MAX) return DVA_ERR_UNSUPPORTED;
  if (P == 0 || C == 0) return DVA_OK;
  if (!grad_out || !seg_ptr || !perm || !row_ptr || !tap_rows || !tap_weights || !seg_of_item || !grad_rows ||
      (keeps_arg(reduce) && !arg))
    return DVA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&](auto row) {
    using T = typename decltype(row)::T;
    with_reduce(reduce, [&](auto rd) {
      hipLaunchKernelGGL((interp_anchor_fixup_kernel<T, decltype(rd)::value>), dim3(1), dim3(256), 0, s,
                         (const T*)grad_out, (const uint16_t*)arg, seg_ptr, perm, row_ptr, tap_rows, tap_weights,
                         seg_of_item, grad_rows, dummy, (int)C);
    });
  };
  if (dtype == DVA_F32) launch(RowType<float, 1>{});
  else launch(RowType<bf16_t, 1>{});
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
