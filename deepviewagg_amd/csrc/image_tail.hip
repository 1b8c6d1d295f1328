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

// VEC consecutive uint8 as floats; `rev`: in reverse order (the mirrored source chunk of a flipped row)
template <int VEC>
__device__ __forceinline__ void it_load(const uint8_t* p, bool rev, float* v);
template <>
__device__ __forceinline__ void it_load<4>(const uint8_t* p, bool rev, float* v) {
  uint32_t w = *reinterpret_cast<const uint32_t*>(p);
  if (rev) w = __builtin_bswap32(w);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (float)((w >> (8 * k)) & 0xffu);
}
template <>
__device__ __forceinline__ void it_load<16>(const uint8_t* p, bool rev, float* v) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  uint32_t w[4] = {q.x, q.y, q.z, q.w};
  if (rev) {
    const uint32_t a = __builtin_bswap32(w[3]), b = __builtin_bswap32(w[2]);
    w[3] = __builtin_bswap32(w[0]);
    w[2] = __builtin_bswap32(w[1]);
    w[0] = a;
    w[1] = b;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[4 * j + k] = (float)((w[j] >> (8 * k)) & 0xffu);
  }
}

__device__ __forceinline__ uint32_t it_pack4(const float* v) {
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

__device__ __forceinline__ float it_mean(const int64_t* __restrict__ sums, int64_t b, int64_t hw) {
  return sums ? __fdiv_rn((float)sums[b], (float)hw) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// gray sums: sums[b] += sum over the pixels of image b of gray(after the first ops.n ops).  grid (blocks, B).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IT_TPB) void image_gray_sums_kernel(const uint8_t* __restrict__ x, int64_t hw, ItOps ops,
                                                                 int64_t* __restrict__ sums) {
  __shared__ unsigned long long sh[IT_TPB / DVA_WAVE];
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
#pragma unroll
  for (int off = DVA_WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  const int lane = threadIdx.x & (DVA_WAVE - 1), wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = sh[0];
    for (int w = 1; w < IT_TPB / DVA_WAVE; ++w) s += sh[w];
    if (s) atomicAdd(reinterpret_cast<unsigned long long*>(sums) + blockIdx.y, s);
  }
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
    return;
  }
  const int c1 = c0 + VEC < W ? c0 + VEC : W;
  const int64_t line = (b * 3 * H + h) * W;
  for (int c = c0; c < c1; ++c) {
    const int64_t s = line + (flip ? W - 1 - c : c), d = line + c;
    float r = (float)x[s], g = (float)x[s + hw], bl = (float)x[s + 2 * hw];
    it_jitter(ops, ops.n, m, r, g, bl);
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
  if (B < 0 || H < 0 || W < 0 || n_ops < 0 || n_ops > 3) return DVA_ERR_INVALID;
  if (n_ops > 0 && (!op_codes || !factors)) return DVA_ERR_INVALID;
  ItOps ops = {};
  int contrast_at = -1;
  for (int k = 0; k < n_ops; ++k) {
    const int code = op_codes[k];
    if (code != IT_BRIGHTNESS && code != IT_CONTRAST && code != IT_SATURATION) return DVA_ERR_INVALID;
    for (int j = 0; j < k; ++j)
      if (ops.code[j] == code) return DVA_ERR_INVALID;
    if (!(factors[k] >= 0.0)) return DVA_ERR_INVALID;      // negative or NaN
    ops.code[k] = code;
    ops.f[k] = (float)factors[k];
    ops.g[k] = (float)(1.0 - factors[k]);
    if (code == IT_CONTRAST) contrast_at = k;
  }
  ops.n = n_ops;
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
