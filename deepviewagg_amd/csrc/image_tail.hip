// The image tail of the multimodal transform chains on the device: ColorJitter -> RandomHorizontalFlip -> ToFloatImage ->
// Normalize (reference: core/data_transform/multimodal/image.py:1195-1282, which hands ColorJitter and Normalize to
// torchvision.transforms 0.8.2).  torchvision is no dependency of this project and no fixture of it exists, so parity
// with it is UNPINNED: the arithmetic below, restated from torchvision 0.8.2's ColorJitter.forward and
// functional_tensor (_blend, rgb_to_grayscale, adjust_brightness / _contrast / _saturation), is the contract.
//
// All arithmetic is fp32, every operation rounded on its own (contraction off), divisions correctly rounded;
// u8(v) = truncation toward zero.  Per pixel (r, g, b) of a uint8 image [B, 3, H, W]:
//   gray            u8((f32(0.2989) r + f32(0.587) g) + f32(0.114) b)
//   blend(p, q, f)  u8(clamp(f32(f) p + f32(1.0 - f) q, 0, 255)), 1.0 - f taken in double by the host
//   brightness      blend(p, 0, f)             per channel
//   saturation      blend(p, gray(pixel), f)   per channel
//   contrast        blend(p, m_i, f), m_i = f32(S_i) / f32(H W), S_i = the exact integer sum of gray over image i in
//                   its state at that point of the op list (after the ops that precede contrast)
// then ToFloatImage f32(p) / f32(255), Normalize (v - mean[c]) / std[c], and under flip output column w takes source
// column W - 1 - w.
//
// Two kernels.  image_gray_sums_kernel (launched only with contrast in the list) accumulates S_i: integer partial sums,
// one wave reduction, one 64-bit integer atomic add per block -- order-free, so the same call gives the same bytes; the
// accumulators are cleared on the stream by every call.  image_tail_u8_kernel reads the three uint8 planes once and
// writes uint8 (jitter / flip alone) or fp32 (either tail step).  A lane owns VEC consecutive pixels of one row in each
// plane (VEC = 16 for uint8 output, 4 for fp32 output: 16-byte stores, lane i at base + 16 i); a chunk that is not full
// (row tail) or whose address is not a multiple of its vector width (rows of a width that is no multiple of VEC) takes
// the scalar path.  image_normalize_f32_kernel is the float32-input mode: Normalize alone, any channel count up to
// DVA_IMAGE_MAX_CHANNELS.  No float atomics, no LDS beyond the block reduction of the sums.
//
// The windowed tail (dva_image_window_u8) runs the same two passes over a window of a source image that is never
// materialised: image index[b] of src [N, 3, H, W], rolled along W by rolls[b], cropped to Wc x Hc at offsets[b].  Its
// kernels image_window_gray_sums_kernel / image_window_u8_kernel share every device function above with the plain
// tail; the contrast mean is taken over the window alone.  The destination chunk of a lane is aligned as before, its
// source address is arbitrary (offsets[b, 0] - rolls[b] per image), so a full chunk inside a row loads through
// it_load_any (the aligned vector load, or the covering aligned dwords shifted into place) and a chunk across the wrap
// column W goes byte by byte; image_window_u8_kernel's comment lists the cases.
#include "dva_common.h"

#pragma clang fp contract(off)

namespace dva {

constexpr int IT_TPB = 256;
constexpr int IT_SUM_VEC = 16;                        // pixels per lane and iteration of the sums kernel
constexpr int IT_SUM_BLOCKS = 512;                    // blocks per image of the sums kernel, at most
constexpr int64_t IT_MAX_THREADS = 0x7fffffffLL - IT_TPB;

enum { IT_BRIGHTNESS = DVA_JITTER_BRIGHTNESS, IT_CONTRAST = DVA_JITTER_CONTRAST, IT_SATURATION = DVA_JITTER_SATURATION };

struct ItOps {
  int n;              // ops to apply, in order
  int code[3];
  float f[3];         // f32(factor)
  float g[3];         // f32(1.0 - factor), the subtraction in double
};

struct ItNorm {
  int on;
  float mean[DVA_IMAGE_MAX_CHANNELS];
  float std[DVA_IMAGE_MAX_CHANNELS];
};

__device__ __forceinline__ float it_gray(float r, float g, float b) {
  return truncf((0.2989f * r + 0.587f * g) + 0.114f * b);
}

__device__ __forceinline__ float it_blend(float p, float q, float f, float g) {
  return truncf(fminf(fmaxf(f * p + g * q, 0.f), 255.f));
}

// the first `n` ops of the list on one pixel; m = the gray mean of the pixel's image (read by contrast only)
__device__ __forceinline__ void it_jitter(const ItOps& ops, int n, float m, float& r, float& g, float& b) {
  for (int k = 0; k < n; ++k) {
    const float f = ops.f[k], c = ops.g[k];
    if (ops.code[k] == IT_BRIGHTNESS) {
      r = it_blend(r, 0.f, f, c);
      g = it_blend(g, 0.f, f, c);
      b = it_blend(b, 0.f, f, c);
    } else if (ops.code[k] == IT_SATURATION) {
      const float q = it_gray(r, g, b);
      r = it_blend(r, q, f, c);
      g = it_blend(g, q, f, c);
      b = it_blend(b, q, f, c);
    } else {
      r = it_blend(r, m, f, c);
      g = it_blend(g, m, f, c);
      b = it_blend(b, m, f, c);
    }
  }
}

// ToFloatImage, then Normalize when it is on
__device__ __forceinline__ float it_tail(float p, const ItNorm& nrm, int c) {
  p = __fdiv_rn(p, 255.f);
  if (nrm.on) p = __fdiv_rn(p - nrm.mean[c], nrm.std[c]);
  return p;
}

// VEC bytes held in VEC / 4 words (byte k of the chunk = bits 8 (k mod 4) of word k / 4) as floats; `rev`: in reverse
// order (the mirrored source chunk of a flipped row)
template <int VEC>
__device__ __forceinline__ void it_unpack(uint32_t* w, bool rev, float* v) {
  if (rev) {
#pragma unroll
    for (int j = 0; j < VEC / 8; ++j) {
      const uint32_t a = __builtin_bswap32(w[VEC / 4 - 1 - j]);
      w[VEC / 4 - 1 - j] = __builtin_bswap32(w[j]);
      w[j] = a;
    }
    if (VEC == 4) w[0] = __builtin_bswap32(w[0]);
  }
#pragma unroll
  for (int j = 0; j < VEC / 4; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[4 * j + k] = (float)((w[j] >> (8 * k)) & 0xffu);
  }
}

// VEC consecutive uint8 at an address that is a multiple of VEC, as floats
template <int VEC>
__device__ __forceinline__ void it_load(const uint8_t* p, bool rev, float* v);
template <>
__device__ __forceinline__ void it_load<4>(const uint8_t* p, bool rev, float* v) {
  uint32_t w[1] = {*reinterpret_cast<const uint32_t*>(p)};
  it_unpack<4>(w, rev, v);
}
template <>
__device__ __forceinline__ void it_load<16>(const uint8_t* p, bool rev, float* v) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  uint32_t w[4] = {q.x, q.y, q.z, q.w};
  it_unpack<16>(w, rev, v);
}

// VEC consecutive uint8 at ANY address, as VEC / 4 words: the aligned load where the address allows it, otherwise the
// aligned words that cover the chunk (VEC / 4, one more when the address is no multiple of 4), shifted into place.
// Every word read holds at least one byte of the chunk, so no read leaves the pages of the chunk.
template <int VEC>
__device__ __forceinline__ void it_words_any(const uint8_t* p, uint32_t* w) {
  const uintptr_t a = (uintptr_t)p;
  if (VEC == 16 && (a % 16) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    return;
  }
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const int sh = (int)(a & 3) * 8;
  uint32_t lo = q[0];
#pragma unroll
  for (int j = 0; j < VEC / 4; ++j) {
    const uint32_t hi = (j + 1 < VEC / 4 || sh) ? q[j + 1] : 0u;
    w[j] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    lo = hi;
  }
}

template <int VEC>
__device__ __forceinline__ void it_load_any(const uint8_t* p, bool rev, float* v) {
  uint32_t w[VEC / 4];
  it_words_any<VEC>(p, w);
  it_unpack<VEC>(w, rev, v);
}

__device__ __forceinline__ uint32_t it_pack4(const float* v) {
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

__device__ __forceinline__ float it_mean(const int64_t* __restrict__ sums, int64_t b, int64_t hw) {
  return sums ? __fdiv_rn((float)sums[b], (float)hw) : 0.f;
}

// the finished chunk of VEC pixels (three planes, `hw` elements apart) at element dst0 of `out`, 16-byte stores: fp32
// after ToFloatImage / Normalize (FOUT) or uint8
template <int VEC, bool FOUT>
__device__ __forceinline__ void it_store_chunk(void* __restrict__ out, int64_t dst0, int64_t hw, const float* r,
                                               const float* g, const float* bl, const ItNorm& nrm) {
  if (FOUT) {
    float* o = static_cast<float*>(out) + dst0;
#pragma unroll
    for (int k0 = 0; k0 < VEC; k0 += 4) {
      *reinterpret_cast<float4*>(o + k0) =
          make_float4(it_tail(r[k0], nrm, 0), it_tail(r[k0 + 1], nrm, 0),
                      it_tail(r[k0 + 2], nrm, 0), it_tail(r[k0 + 3], nrm, 0));
      *reinterpret_cast<float4*>(o + hw + k0) =
          make_float4(it_tail(g[k0], nrm, 1), it_tail(g[k0 + 1], nrm, 1),
                      it_tail(g[k0 + 2], nrm, 1), it_tail(g[k0 + 3], nrm, 1));
      *reinterpret_cast<float4*>(o + 2 * hw + k0) =
          make_float4(it_tail(bl[k0], nrm, 2), it_tail(bl[k0 + 1], nrm, 2),
                      it_tail(bl[k0 + 2], nrm, 2), it_tail(bl[k0 + 3], nrm, 2));
    }
  } else {
    uint8_t* o = static_cast<uint8_t*>(out) + dst0;
    if (VEC == 16) {
      *reinterpret_cast<uint4*>(o) = make_uint4(it_pack4(r), it_pack4(r + 4), it_pack4(r + 8), it_pack4(r + 12));
      *reinterpret_cast<uint4*>(o + hw) = make_uint4(it_pack4(g), it_pack4(g + 4), it_pack4(g + 8), it_pack4(g + 12));
      *reinterpret_cast<uint4*>(o + 2 * hw) =
          make_uint4(it_pack4(bl), it_pack4(bl + 4), it_pack4(bl + 8), it_pack4(bl + 12));
    } else {
      *reinterpret_cast<uint32_t*>(o) = it_pack4(r);
      *reinterpret_cast<uint32_t*>(o + hw) = it_pack4(g);
      *reinterpret_cast<uint32_t*>(o + 2 * hw) = it_pack4(bl);
    }
  }
}

// one finished pixel at element d of `out`
template <bool FOUT>
__device__ __forceinline__ void it_store_pixel(void* __restrict__ out, int64_t d, int64_t hw, float r, float g, float bl,
                                               const ItNorm& nrm) {
  if (FOUT) {
    float* o = static_cast<float*>(out);
    o[d] = it_tail(r, nrm, 0);
    o[d + hw] = it_tail(g, nrm, 1);
    o[d + 2 * hw] = it_tail(bl, nrm, 2);
  } else {
    uint8_t* o = static_cast<uint8_t*>(out);
    o[d] = (uint8_t)r;
    o[d + hw] = (uint8_t)g;
    o[d + 2 * hw] = (uint8_t)bl;
  }
}

// sums[slot] += the block's total of `acc`: one wave reduction, one 64-bit integer atomic add per block
__device__ __forceinline__ void it_block_add(unsigned long long acc, int64_t* __restrict__ sums, int64_t slot) {
  __shared__ unsigned long long sh[IT_TPB / DVA_WAVE];
#pragma unroll
  for (int off = DVA_WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  const int lane = threadIdx.x & (DVA_WAVE - 1), wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = sh[0];
    for (int w = 1; w < IT_TPB / DVA_WAVE; ++w) s += sh[w];
    if (s) atomicAdd(reinterpret_cast<unsigned long long*>(sums) + slot, s);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// gray sums: sums[b] += sum over the pixels of image b of gray(after the first ops.n ops).  grid (blocks, B).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IT_TPB) void image_gray_sums_kernel(const uint8_t* __restrict__ x, int64_t hw, ItOps ops,
                                                                 int64_t* __restrict__ sums) {
  const uint8_t* r0 = x + (int64_t)blockIdx.y * 3 * hw;
  const uint8_t* g0 = r0 + hw;
  const uint8_t* b0 = g0 + hw;
  // the planes of an image are contiguous, so the chunks run over the whole plane, rows ignored; all three planes
  // share the alignment of a chunk when hw is a multiple of the vector width
  const bool vec_ok = (hw % IT_SUM_VEC) == 0 && ((uintptr_t)r0 % IT_SUM_VEC) == 0;
  const int64_t chunks = (hw + IT_SUM_VEC - 1) / IT_SUM_VEC;
  unsigned long long acc = 0;
  for (int64_t j = (int64_t)blockIdx.x * IT_TPB + threadIdx.x; j < chunks; j += (int64_t)gridDim.x * IT_TPB) {
    const int64_t i0 = j * IT_SUM_VEC;
    uint32_t part = 0;
    if (vec_ok) {
      const uint4 qr = *reinterpret_cast<const uint4*>(r0 + i0);
      const uint4 qg = *reinterpret_cast<const uint4*>(g0 + i0);
      const uint4 qb = *reinterpret_cast<const uint4*>(b0 + i0);
      const uint32_t wr[4] = {qr.x, qr.y, qr.z, qr.w}, wg[4] = {qg.x, qg.y, qg.z, qg.w}, wb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float r = (float)((wr[j] >> (8 * k)) & 0xffu), g = (float)((wg[j] >> (8 * k)) & 0xffu),
                b = (float)((wb[j] >> (8 * k)) & 0xffu);
          it_jitter(ops, ops.n, 0.f, r, g, b);
          part += (uint32_t)it_gray(r, g, b);
        }
      }
    } else {
      const int64_t i1 = i0 + IT_SUM_VEC < hw ? i0 + IT_SUM_VEC : hw;
      for (int64_t i = i0; i < i1; ++i) {
        float r = (float)r0[i], g = (float)g0[i], b = (float)b0[i];
        it_jitter(ops, ops.n, 0.f, r, g, b);
        part += (uint32_t)it_gray(r, g, b);
      }
    }
    acc += part;
  }
  it_block_add(acc, sums, blockIdx.y);
}

// ---------------------------------------------------------------------------------------------------------------
// apply, uint8 in: one thread per chunk of VEC consecutive pixels of one row, all three planes
// ---------------------------------------------------------------------------------------------------------------
template <int VEC, bool FOUT>
__global__ __launch_bounds__(IT_TPB) void image_tail_u8_kernel(const uint8_t* __restrict__ x, int64_t rows, int H, int W,
                                                               int chunks_per_row, ItOps ops,
                                                               const int64_t* __restrict__ sums, int flip,
                                                               ItNorm nrm, void* __restrict__ out, int aligned) {
  const int64_t t = (int64_t)blockIdx.x * IT_TPB + threadIdx.x;
  if (t >= rows * chunks_per_row) return;
  const int64_t row = t / chunks_per_row;               // b * H + h
  const int c0 = (int)(t - row * chunks_per_row) * VEC;  // first output column of the chunk
  const int64_t b = row / H;
  const int64_t h = row - b * H;
  const int64_t hw = (int64_t)H * W;
  const float m = it_mean(sums, b, hw);
  const int64_t dst0 = (b * 3 * H + h) * W + c0;         // plane 0; plane c adds c * hw
  const int s0 = flip ? W - c0 - VEC : c0;               // first source column of a full chunk
  const int64_t src0 = (b * 3 * H + h) * W + s0;
  // plane c lies c * hw further on: with hw a multiple of VEC the three planes share the chunk's alignment
  const bool vec = aligned && c0 + VEC <= W && (dst0 % VEC) == 0 && (src0 % VEC) == 0 && (hw % VEC) == 0;
  if (vec) {
    float r[VEC], g[VEC], bl[VEC];
    it_load<VEC>(x + src0, flip, r);
    it_load<VEC>(x + src0 + hw, flip, g);
    it_load<VEC>(x + src0 + 2 * hw, flip, bl);
#pragma unroll
    for (int k = 0; k < VEC; ++k) it_jitter(ops, ops.n, m, r[k], g[k], bl[k]);
    it_store_chunk<VEC, FOUT>(out, dst0, hw, r, g, bl, nrm);
    return;
  }
  const int c1 = c0 + VEC < W ? c0 + VEC : W;
  const int64_t line = (b * 3 * H + h) * W;
  for (int c = c0; c < c1; ++c) {
    const int64_t s = line + (flip ? W - 1 - c : c), d = line + c;
    float r = (float)x[s], g = (float)x[s + hw], bl = (float)x[s + 2 * hw];
    it_jitter(ops, ops.n, m, r, g, bl);
    it_store_pixel<FOUT>(out, d, hw, r, g, bl, nrm);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// apply, float32 in: out = (x - mean[c]) / std[c]; one thread per chunk of 4 consecutive elements of one plane
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IT_TPB) void image_normalize_f32_kernel(const float* __restrict__ x, int64_t planes, int C,
                                                                     int64_t hw, int64_t chunks_per_plane, ItNorm nrm,
                                                                     float* __restrict__ out, int aligned) {
  const int64_t t = (int64_t)blockIdx.x * IT_TPB + threadIdx.x;
  if (t >= planes * chunks_per_plane) return;
  const int64_t plane = t / chunks_per_plane;
  const int64_t i0 = (t - plane * chunks_per_plane) * 4;
  const int c = (int)(plane % C);
  const float mu = nrm.mean[c], sd = nrm.std[c];
  const int64_t e0 = plane * hw + i0;
  if (aligned && i0 + 4 <= hw && (e0 % 4) == 0) {
    const float4 v = *reinterpret_cast<const float4*>(x + e0);
    *reinterpret_cast<float4*>(out + e0) = make_float4(__fdiv_rn(v.x - mu, sd), __fdiv_rn(v.y - mu, sd),
                                                       __fdiv_rn(v.z - mu, sd), __fdiv_rn(v.w - mu, sd));
    return;
  }
  const int64_t i1 = i0 + 4 < hw ? i0 + 4 : hw;
  for (int64_t i = i0; i < i1; ++i) out[plane * hw + i] = __fdiv_rn(x[plane * hw + i] - mu, sd);
}

// ---------------------------------------------------------------------------------------------------------------
// the windowed tail: the same passes over a window of a source image that is never materialised
//   win[b, c, y, x] = src[index[b], c, offsets[b, 1] + y, (offsets[b, 0] + x - rolls[b]) mod W]
// ---------------------------------------------------------------------------------------------------------------
// output image b in its source: plane 0 of the source image, the first source row of the window and the source column
// of window column 0.  index / offsets / rolls are device data nobody has validated: the image is clamped to [0, N - 1]
// and the rows to [0, H - 1] (iw_row), the column is in [0, W) by the mod.
struct IwImage {
  const uint8_t* plane0;
  int64_t y0;
  int64_t x0;
};

__device__ __forceinline__ IwImage iw_image(const uint8_t* __restrict__ src, int64_t N, int64_t hw, int64_t H, int64_t W,
                                            const int64_t* __restrict__ index, const int64_t* __restrict__ rolls,
                                            const int64_t* __restrict__ offsets, int64_t b) {
  int64_t i = index[b];
  i = i < 0 ? 0 : (i >= N ? N - 1 : i);
  // the difference in unsigned arithmetic: absurd values wrap (their result is unspecified) instead of overflowing
  int64_t x0 = (int64_t)((uint64_t)offsets[2 * b] - (uint64_t)rolls[b]) % W;
  if (x0 < 0) x0 += W;
  int64_t y0 = offsets[2 * b + 1];
  y0 = y0 < 0 ? 0 : (y0 >= H ? H - 1 : y0);
  return {src + i * 3 * hw, y0, x0};
}

__device__ __forceinline__ int64_t iw_row(const IwImage& im, int64_t y, int64_t H) {
  return im.y0 + y < H ? im.y0 + y : H - 1;
}

// source column of window column w (w < Wc <= W, so one subtraction wraps)
__device__ __forceinline__ int64_t iw_col(const IwImage& im, int64_t w, int64_t W) {
  const int64_t s = im.x0 + w;
  return s >= W ? s - W : s;
}

// gray sums over the window: sums[b] += sum over the Hc x Wc window pixels of gray(after the first ops.n ops).
// grid (blocks, B); a lane takes chunks of IT_SUM_VEC pixels of one window row, loaded as in the apply kernel.
__global__ __launch_bounds__(IT_TPB) void image_window_gray_sums_kernel(
    const uint8_t* __restrict__ src, int64_t N, int H, int W, const int64_t* __restrict__ index,
    const int64_t* __restrict__ rolls, const int64_t* __restrict__ offsets, int Hc, int Wc, ItOps ops,
    int64_t* __restrict__ sums) {
  const int64_t hw = (int64_t)H * W;
  const IwImage im = iw_image(src, N, hw, H, W, index, rolls, offsets, blockIdx.y);
  const int chunks_per_row = (Wc + IT_SUM_VEC - 1) / IT_SUM_VEC;
  const int64_t chunks = (int64_t)Hc * chunks_per_row;
  unsigned long long acc = 0;
  for (int64_t j = (int64_t)blockIdx.x * IT_TPB + threadIdx.x; j < chunks; j += (int64_t)gridDim.x * IT_TPB) {
    const int64_t y = j / chunks_per_row;
    const int c0 = (int)(j - y * chunks_per_row) * IT_SUM_VEC;
    const int n = Wc - c0 < IT_SUM_VEC ? Wc - c0 : IT_SUM_VEC;
    const uint8_t* line = im.plane0 + iw_row(im, y, H) * W;
    const int64_t s = iw_col(im, c0, W);
    uint32_t part = 0;
    if (n == IT_SUM_VEC && s + IT_SUM_VEC <= W) {
      uint32_t wr[IT_SUM_VEC / 4], wg[IT_SUM_VEC / 4], wb[IT_SUM_VEC / 4];
      it_words_any<IT_SUM_VEC>(line + s, wr);
      it_words_any<IT_SUM_VEC>(line + s + hw, wg);
      it_words_any<IT_SUM_VEC>(line + s + 2 * hw, wb);
#pragma unroll
      for (int i = 0; i < IT_SUM_VEC / 4; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float r = (float)((wr[i] >> (8 * k)) & 0xffu), g = (float)((wg[i] >> (8 * k)) & 0xffu),
                bl = (float)((wb[i] >> (8 * k)) & 0xffu);
          it_jitter(ops, ops.n, 0.f, r, g, bl);
          part += (uint32_t)it_gray(r, g, bl);
        }
      }
    } else {
      for (int k = 0; k < n; ++k) {
        const int64_t col = iw_col(im, c0 + k, W);
        float r = (float)line[col], g = (float)line[col + hw], bl = (float)line[col + 2 * hw];
        it_jitter(ops, ops.n, 0.f, r, g, bl);
        part += (uint32_t)it_gray(r, g, bl);
      }
    }
    acc += part;
  }
  it_block_add(acc, sums, blockIdx.y);
}

// apply over the window: one thread per chunk of VEC consecutive output pixels of one window row, all three planes.
// Which load a chunk takes (all give the same bytes):
//   full chunk, its source columns do not pass the wrap column W, 16-byte aligned destination
//     source address a multiple of VEC (16 for uint8 output, 4 for fp32 output)   one aligned vector load per plane
//     any other source address (odd, or a multiple of 4 but not of 16)            the aligned dwords that cover the
//                                                                                 chunk, shifted into place
//   a chunk that is not full (row tail of a width that is no multiple of VEC), that straddles the wrap column, or
//   whose destination is not 16-byte aligned (Hc Wc no multiple of VEC)           byte by byte, the column wrapped
template <int VEC, bool FOUT>
__global__ __launch_bounds__(IT_TPB) void image_window_u8_kernel(
    const uint8_t* __restrict__ src, int64_t N, int H, int W, const int64_t* __restrict__ index,
    const int64_t* __restrict__ rolls, const int64_t* __restrict__ offsets, int64_t rows, int Hc, int Wc,
    int chunks_per_row, ItOps ops, const int64_t* __restrict__ sums, int flip, ItNorm nrm, void* __restrict__ out,
    int aligned) {
  const int64_t t = (int64_t)blockIdx.x * IT_TPB + threadIdx.x;
  if (t >= rows * chunks_per_row) return;
  const int64_t row = t / chunks_per_row;               // b * Hc + y
  const int c0 = (int)(t - row * chunks_per_row) * VEC;  // first output column of the chunk
  const int64_t b = row / Hc;
  const int64_t y = row - b * Hc;
  const int64_t hw = (int64_t)H * W, hwc = (int64_t)Hc * Wc;
  const float m = it_mean(sums, b, hwc);
  const IwImage im = iw_image(src, N, hw, H, W, index, rolls, offsets, b);
  const uint8_t* line = im.plane0 + iw_row(im, y, H) * W;
  const int64_t dst_line = (b * 3 * Hc + y) * Wc;        // plane 0; plane c adds c * hwc
  const int n = Wc - c0 < VEC ? Wc - c0 : VEC;
  // a flipped chunk reads the mirrored window columns Wc - c0 - n .. Wc - 1 - c0 in reverse
  const int64_t s = iw_col(im, flip ? Wc - c0 - n : c0, W);
  if (aligned && n == VEC && s + VEC <= W && ((dst_line + c0) % VEC) == 0 && (hwc % VEC) == 0) {
    float r[VEC], g[VEC], bl[VEC];
    it_load_any<VEC>(line + s, flip, r);
    it_load_any<VEC>(line + s + hw, flip, g);
    it_load_any<VEC>(line + s + 2 * hw, flip, bl);
#pragma unroll
    for (int k = 0; k < VEC; ++k) it_jitter(ops, ops.n, m, r[k], g[k], bl[k]);
    it_store_chunk<VEC, FOUT>(out, dst_line + c0, hwc, r, g, bl, nrm);
    return;
  }
  for (int c = c0; c < c0 + n; ++c) {
    const int64_t col = iw_col(im, flip ? Wc - 1 - c : c, W);
    float r = (float)line[col], g = (float)line[col + hw], bl = (float)line[col + 2 * hw];
    it_jitter(ops, ops.n, m, r, g, bl);
    it_store_pixel<FOUT>(out, dst_line + c, hwc, r, g, bl, nrm);
  }
}

static inline int64_t it_sums_bytes(int64_t B) { return (int64_t)align_up((size_t)(B > 0 ? B : 1) * 8); }

// mean / std (host, C floats each, both or neither) into the kernel argument
static int it_norm(const float* mean, const float* std, int64_t C, ItNorm* nrm) {
  nrm->on = 0;
  if (!mean && !std) return DVA_OK;
  if (!mean || !std) return DVA_ERR_INVALID;
  if (C > DVA_IMAGE_MAX_CHANNELS) return DVA_ERR_UNSUPPORTED;
  for (int64_t c = 0; c < C; ++c) {
    if (std[c] == 0.f) return DVA_ERR_INVALID;
    nrm->mean[c] = mean[c];
    nrm->std[c] = std[c];
  }
  nrm->on = 1;
  return DVA_OK;
}

// the op list (host arrays) into the kernel argument; *contrast_at = the position of contrast in it, or -1
static int it_ops(const int32_t* op_codes, const double* factors, int32_t n_ops, ItOps* ops, int* contrast_at) {
  if (n_ops < 0 || n_ops > 3) return DVA_ERR_INVALID;
  if (n_ops > 0 && (!op_codes || !factors)) return DVA_ERR_INVALID;
  *contrast_at = -1;
  for (int k = 0; k < n_ops; ++k) {
    const int code = op_codes[k];
    if (code != IT_BRIGHTNESS && code != IT_CONTRAST && code != IT_SATURATION) return DVA_ERR_INVALID;
    for (int j = 0; j < k; ++j)
      if (ops->code[j] == code) return DVA_ERR_INVALID;
    if (!(factors[k] >= 0.0)) return DVA_ERR_INVALID;      // negative or NaN
    ops->code[k] = code;
    ops->f[k] = (float)factors[k];
    ops->g[k] = (float)(1.0 - factors[k]);
    if (code == IT_CONTRAST) *contrast_at = k;
  }
  ops->n = n_ops;
  return DVA_OK;
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_image_tail_workspace_bytes(int64_t B) {
  if (B < 0) return DVA_ERR_INVALID;
  return it_sums_bytes(B);
}

int dva_image_tail_u8(const uint8_t* x, int64_t B, int64_t H, int64_t W, const int32_t* op_codes,
                      const double* factors, int32_t n_ops, int32_t flip, int32_t to_float, const float* mean,
                      const float* std, void* out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (B < 0 || H < 0 || W < 0) return DVA_ERR_INVALID;
  ItOps ops = {};
  int contrast_at = -1;
  if (it_ops(op_codes, factors, n_ops, &ops, &contrast_at) != DVA_OK) return DVA_ERR_INVALID;
  ItNorm nrm = {};
  const int rc = it_norm(mean, std, 3, &nrm);
  if (rc != DVA_OK) return rc;
  if (nrm.on && !to_float) return DVA_ERR_INVALID;          // Normalize takes the [0, 1] floats of ToFloatImage
  if (B == 0 || H == 0 || W == 0) return DVA_OK;
  if (!x || !out) return DVA_ERR_INVALID;
  if (contrast_at >= 0 && (!workspace || workspace_bytes < it_sums_bytes(B))) return DVA_ERR_INVALID;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL - 16 || B > 65535) return DVA_ERR_UNSUPPORTED;
  const bool fout = to_float != 0;
  const int vec = fout ? 4 : 16;
  const int64_t chunks_per_row = (W + vec - 1) / vec;
  if (B * H > IT_MAX_THREADS / chunks_per_row) return DVA_ERR_UNSUPPORTED;
  const int64_t threads = B * H * chunks_per_row;
  const int64_t hw = H * W;                                  // < 2^31 * 16
  hipStream_t s = (hipStream_t)stream;
  int64_t* sums = nullptr;
  if (contrast_at >= 0) {
    sums = (int64_t*)workspace;
    if (hipMemsetAsync(sums, 0, (size_t)B * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
    ItOps pre = ops;
    pre.n = contrast_at;
    int64_t blocks = ((hw + IT_SUM_VEC - 1) / IT_SUM_VEC + IT_TPB - 1) / IT_TPB;
    if (blocks > IT_SUM_BLOCKS) blocks = IT_SUM_BLOCKS;
    hipLaunchKernelGGL(image_gray_sums_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(IT_TPB), 0, s, x, hw, pre,
                       sums);
  }
  const int aligned = ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0;
  const dim3 grid((unsigned)((threads + IT_TPB - 1) / IT_TPB));
  if (fout)
    hipLaunchKernelGGL((image_tail_u8_kernel<4, true>), grid, dim3(IT_TPB), 0, s, x, B * H, (int)H, (int)W,
                       (int)chunks_per_row, ops, (const int64_t*)sums, (int)(flip != 0), nrm, out, aligned);
  else
    hipLaunchKernelGGL((image_tail_u8_kernel<16, false>), grid, dim3(IT_TPB), 0, s, x, B * H, (int)H, (int)W,
                       (int)chunks_per_row, ops, (const int64_t*)sums, (int)(flip != 0), nrm, out, aligned);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int64_t dva_image_window_workspace_bytes(int64_t B) {
  if (B < 0) return DVA_ERR_INVALID;
  return it_sums_bytes(B);
}

int dva_image_window_u8(const uint8_t* src, int64_t N, int64_t H, int64_t W, const int64_t* index,
                        const int64_t* rolls, const int64_t* offsets, int64_t B, int64_t Wc, int64_t Hc,
                        const int32_t* op_codes, const double* factors, int32_t n_ops, int32_t flip, int32_t to_float,
                        const float* mean, const float* std, void* out, void* workspace, int64_t workspace_bytes,
                        void* stream) {
  if (N < 0 || H < 0 || W < 0 || B < 0 || Wc < 0 || Hc < 0 || Wc > W || Hc > H) return DVA_ERR_INVALID;
  ItOps ops = {};
  int contrast_at = -1;
  if (it_ops(op_codes, factors, n_ops, &ops, &contrast_at) != DVA_OK) return DVA_ERR_INVALID;
  ItNorm nrm = {};
  const int rc = it_norm(mean, std, 3, &nrm);
  if (rc != DVA_OK) return rc;
  if (nrm.on && !to_float) return DVA_ERR_INVALID;          // Normalize takes the [0, 1] floats of ToFloatImage
  if (B == 0) return DVA_OK;
  if (N < 1 || Wc < 1 || Hc < 1) return DVA_ERR_INVALID;    // nothing to index, or no window
  if (!src || !index || !rolls || !offsets || !out) return DVA_ERR_INVALID;
  if (contrast_at >= 0 && (!workspace || workspace_bytes < it_sums_bytes(B))) return DVA_ERR_INVALID;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL - 16 || B > 65535) return DVA_ERR_UNSUPPORTED;
  const bool fout = to_float != 0;
  const int vec = fout ? 4 : 16;
  const int64_t chunks_per_row = (Wc + vec - 1) / vec;
  if (B * Hc > IT_MAX_THREADS / chunks_per_row) return DVA_ERR_UNSUPPORTED;
  const int64_t threads = B * Hc * chunks_per_row;
  hipStream_t s = (hipStream_t)stream;
  int64_t* sums = nullptr;
  if (contrast_at >= 0) {
    sums = (int64_t*)workspace;
    if (hipMemsetAsync(sums, 0, (size_t)B * 8, s) != hipSuccess) return DVA_ERR_LAUNCH;
    ItOps pre = ops;
    pre.n = contrast_at;
    const int64_t sum_chunks = Hc * ((Wc + IT_SUM_VEC - 1) / IT_SUM_VEC);
    const dim3 sgrid((unsigned)capped_grid(sum_chunks, IT_TPB, IT_SUM_BLOCKS), (unsigned)B);
    hipLaunchKernelGGL(image_window_gray_sums_kernel, sgrid, dim3(IT_TPB), 0, s, src, N, (int)H, (int)W, index, rolls,
                       offsets, (int)Hc, (int)Wc, pre, sums);
  }
  const int aligned = ((uintptr_t)out % 16) == 0;
  const dim3 grid((unsigned)blocks_for(threads, IT_TPB));
  if (fout)
    hipLaunchKernelGGL((image_window_u8_kernel<4, true>), grid, dim3(IT_TPB), 0, s, src, N, (int)H, (int)W, index,
                       rolls, offsets, B * Hc, (int)Hc, (int)Wc, (int)chunks_per_row, ops, (const int64_t*)sums,
                       (int)(flip != 0), nrm, out, aligned);
  else
    hipLaunchKernelGGL((image_window_u8_kernel<16, false>), grid, dim3(IT_TPB), 0, s, src, N, (int)H, (int)W, index,
                       rolls, offsets, B * Hc, (int)Hc, (int)Wc, (int)chunks_per_row, ops, (const int64_t*)sums,
                       (int)(flip != 0), nrm, out, aligned);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_image_normalize_f32(const float* x, int64_t B, int64_t C, int64_t HW, const float* mean, const float* std,
                            float* out, void* stream) {
  if (B < 0 || C < 1 || HW < 0 || !mean || !std) return DVA_ERR_INVALID;
  ItNorm nrm = {};
  const int rc = it_norm(mean, std, C, &nrm);
  if (rc != DVA_OK) return rc;
  if (B == 0 || HW == 0) return DVA_OK;
  if (!x || !out) return DVA_ERR_INVALID;
  const int64_t chunks_per_plane = (HW + 3) / 4;
  if (B > IT_MAX_THREADS / C || B * C > IT_MAX_THREADS / chunks_per_plane) return DVA_ERR_UNSUPPORTED;
  const int64_t threads = B * C * chunks_per_plane;
  const int aligned = ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0;
  hipLaunchKernelGGL(image_normalize_f32_kernel, dim3((unsigned)((threads + IT_TPB - 1) / IT_TPB)), dim3(IT_TPB), 0,
                     (hipStream_t)stream, x, B * C, (int)C, HW, chunks_per_plane, nrm, out, aligned);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
