// Lazy nearest gather fused with the max / mean / sum / min pool behind it, for gfx950 (reference: x_mod = features[idx],
// core/multimodal/image.py:1262-1287, followed by BimodalCSRPool(mode) = torch_scatter.segment_csr over the items of each
// segment, modules/multimodal/pooling.py:14-71).
//
// forward   out[s][c] = reduce over the items a in [seg_ptr[s], seg_ptr[s + 1]) of rows[row_idx[a]][c]
// backward  grad_rows[r][c] = sum over the items a with row_idx[a] == r of g(a, c)
//
// No [P, C] tensor in either direction.  The forward is dva_segment_csr_fwd's arithmetic on the rows it would have been
// handed (fp32 accumulation from 0 in item order, one division for the mean, one rounding; max / min: first item on ties,
// a NaN wins only as the first item), so it equals the materialised composition bit for bit.  The backward is a segmented
// reduction over the row plan of the items (perm = items sorted by map row, row_ptr): one wavefront per map row, fp32
// accumulators, every element of grad_rows written once in the rows' storage type -- no float atomics, so two runs agree
// bit for bit, and one rounding per map row where the materialised route rounds per item and again per row.
//
// Bytes: forward P (4 + C s) [map rows, out of the cache hierarchy] + S (8 + C s) (+ 2 S C: the arg offsets of max / min);
//        backward P (8 + C s) [gradient rows of the segments, cached] (+ 8 P: mean / max / min read seg_ptr, + 2 P C: the
//        arg rows of max / min) + R (4 + C s).
#include "dva_common.h"
#include "row_chunk.h"

namespace dva {

// One thread per (segment, VEC-channel chunk) walks the segment's items in order: the loop of segment_csr_fwd_kernel /
// _vec_kernel (segment.hip) with the row index in between.
template <typename T, int VEC, int REDUCE>
__global__ __launch_bounds__(256) void gather_segment_reduce_fwd_kernel(const T* __restrict__ rows,
                                                                         const int32_t* __restrict__ row_idx,
                                                                         const int64_t* __restrict__ seg_ptr,
                                                                         T* __restrict__ out, uint16_t* __restrict__ arg,
                                                                         int64_t S, int C) {
  const int cpr = C / VEC;
  const int64_t total = S * (int64_t)cpr;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = t / cpr;
    const int c0 = (int)(t - s * cpr) * VEC;
    const int64_t beg = seg_ptr[s], end = seg_ptr[s + 1];
    float acc[VEC];
    uint32_t best[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      acc[k] = 0.f;
      best[k] = 0xffffu;
    }
    for (int64_t a = beg; a < end; ++a) {
      float f[VEC];
      RowChunk<T, VEC>::ld(rows + (int64_t)row_idx[a] * C + c0, f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) pool_step<REDUCE>(acc[k], best[k], f[k], a == beg, (uint32_t)(a - beg));
    }
    if (REDUCE == DVA_MEAN && end > beg) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] /= (float)(end - beg);
    }
    RowChunk<T, VEC>::st(out + s * C + c0, acc);
    if (keeps_arg(REDUCE)) RowChunk<T, VEC>::st_arg(arg + s * C + c0, best);
  }
}

// One wavefront per map row r: its items perm[row_ptr[r] .. row_ptr[r + 1]) are spread over 64 / lpr slots, lpr lanes (a
// power of two) own the VEC-channel chunks of a row; rows wider than lpr chunks are walked in column passes of lpr chunks.
// Item a of segment s = seg_of_item[a] contributes pool_term of grad_out[s][c].  The slots are summed with wave64 xor
// shuffles in a fixed order.
template <typename T, int VEC, int REDUCE>
__global__ __launch_bounds__(256) void gather_segment_reduce_bwd_kernel(
    const T* __restrict__ gout, const uint16_t* __restrict__ arg, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ seg_of_item,
    T* __restrict__ grows, int64_t R, int C, int lpr) {
  constexpr int U = 2;
  const int chunks = C / VEC;
  const int lane = threadIdx.x & 63;
  const int lane_r = lane & (lpr - 1), slot = lane / lpr, slots = 64 / lpr;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < R; r += n_waves) {
    const int beg = row_ptr[r], end = row_ptr[r + 1];
    for (int ch0 = 0; ch0 < chunks; ch0 += lpr) {
      const bool live = ch0 + lane_r < chunks;                 // lanes behind the last chunk of the row carry zeros
      const int64_t col = (int64_t)(live ? ch0 + lane_r : 0) * VEC;
      float acc[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      for (int i0 = beg; i0 < end; i0 += slots * U) {
        int64_t s[U];
        uint32_t koff[U];
        float count[U];                                        // items of the segment; 0: no item in this slot
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * slots + slot;
          const bool ok = i < end && live;
          const int a = perm[i < end ? i : beg];
          s[u] = seg_of_item[a];
          koff[u] = 0xfffeu;                                   // 0xfffe never is a stored offset
          count[u] = ok ? 1.f : 0.f;
          if (REDUCE != DVA_SUM) {
            const int64_t sb = seg_ptr[s[u]];
            if (REDUCE == DVA_MEAN) count[u] = ok ? (float)(seg_ptr[s[u] + 1] - sb) : 0.f;
            if (keeps_arg(REDUCE) && ok) koff[u] = (uint32_t)((int64_t)a - sb);
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
            const float term = pool_term<REDUCE>(g[u][k], 1.f, count[u], ak[u][k], koff[u]);
            acc[k] += count[u] != 0.f ? term : 0.f;
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

}  // namespace dva

using namespace dva;

extern "C" {

int dva_gather_segment_reduce_fwd(const void* rows, const int32_t* row_idx, const int64_t* seg_ptr, void* out, void* arg,
                                  int64_t S, int64_t P, int64_t R, int32_t C, int32_t dtype, int32_t reduce,
                                  void* stream) {
  int rc = check_sizes(S, P, R, C, dtype, reduce);
  if (rc) return rc;
  if (S > 0 && C > 0 && (!seg_ptr || !out || (keeps_arg(reduce) && !arg) || (P > 0 && (!rows || !row_idx))))
    return DVA_ERR_INVALID;
  if (S > POOL_SIZE_MAX || P > POOL_SIZE_MAX || R > POOL_SIZE_MAX) return DVA_ERR_UNSUPPORTED;
  if (S == 0 || C == 0) return DVA_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool wide = C % row_vec(dtype) == 0 && aligned16(rows) && aligned16(out) && aligned16(arg);
  with_row_type(dtype, wide, [&](auto row) {
    using T = typename decltype(row)::T;
    constexpr int VEC = decltype(row)::VEC;
    const dim3 grid(capped_grid(S * (int64_t)(C / VEC), 256, GRID_CAP));
    with_reduce(reduce, [&](auto rd) {
      hipLaunchKernelGGL((gather_segment_reduce_fwd_kernel<T, VEC, decltype(rd)::value>), grid, dim3(256), 0, s,
                         (const T*)rows, row_idx, seg_ptr, (T*)out, (uint16_t*)arg, S, (int)C);
    });
  });
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_gather_segment_reduce_bwd(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                                  const int32_t* row_ptr, const int32_t* seg_of_item, void* grad_rows, int64_t S,
                                  int64_t P, int64_t R, int32_t C, int32_t dtype, int32_t reduce, void* stream) {
  int rc = check_sizes(S, P, R, C, dtype, reduce);
  if (rc) return rc;
  if (S > 0 && C > 0 && R > 0 &&
      (!grad_rows || !row_ptr ||
       (P > 0 && (!grad_out || !seg_ptr || !perm || !seg_of_item || (keeps_arg(reduce) && !arg)))))
    return DVA_ERR_INVALID;
  if (S > POOL_SIZE_MAX || P > POOL_SIZE_MAX || R > POOL_SIZE_MAX) return DVA_ERR_UNSUPPORTED;
  if (R == 0 || C == 0) return DVA_OK;
  if (!grad_rows || !row_ptr) return DVA_ERR_INVALID;     // S == 0: every row still gets its zeros
  hipStream_t s = (hipStream_t)stream;
  const bool wide = C % row_vec(dtype) == 0 && aligned16(grad_out) && aligned16(grad_rows) && aligned16(arg);
  const dim3 grid(capped_grid(R, 4, GRID_CAP));      // four wavefronts, four map rows per block
  with_row_type(dtype, wide, [&](auto row) {
    using T = typename decltype(row)::T;
    constexpr int VEC = decltype(row)::VEC;
    with_reduce(reduce, [&](auto rd) {
      hipLaunchKernelGGL((gather_segment_reduce_bwd_kernel<T, VEC, decltype(rd)::value>), grid, dim3(256), 0, s,
                         (const T*)grad_out, (const uint16_t*)arg, seg_ptr, perm, row_ptr, seg_of_item, (T*)grad_rows, R,
                         (int)C, lanes_per_row(C / VEC));
    });
  });
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
