// Loading images on the device: the pixel arithmetic of SameSettingImageData.read_images (reference:
// core/multimodal/image.py:1059-1099) and of NonStaticMask (core/data_transform/multimodal/image.py:130-154) after the
// files are decoded.  The reference resizes with PIL.Image.resize, which for an RGB image is Pillow's 8-bit BICUBIC
// resample; that arithmetic, restated in include/dva.h at dva_image_resample_u8, is the contract, bit for bit.
//
// image_resample_u8_kernel<AXIS> is ONE pass of that resample along x (AXIS 0) or y (AXIS 1) over a batch.  The host
// computes the fixed-point coefficient tables in double (ops.image_resample_tables) and uploads them; the kernel does
// the integer part: int32 s = 2^21 + sum_k pixel * coefficient, out = clamp(s >> 22, 0, 255).  Source and destination
// are described by byte strides, so the same kernel reads the decoder's HWC bytes, the HWC intermediate between two
// passes or a planar batch, and writes the HWC intermediate or the planar [B, 3, H, W] result.  Three per-image shifts
// fold the roll and the crop of read_images into a pass, so that no rolled or cropped image is ever written:
//   shifts[b, 0]  on the pass's OUTPUT index along its axis: output i is row (i + shift) of the coefficient table
//                 (a crop along the axis; with out_period the roll of the pass's result)
//   shifts[b, 1]  on the SOURCE index along the axis: tap k of a row reads source (xmin + k + shift) (with src_period
//                 the roll of the pass's source)
//   shifts[b, 2]  on the index along the OTHER axis: output j reads source (j + shift) (a crop, or with other_period a
//                 roll, across the pass)
// A period of 0 makes the shift a plain offset; otherwise the sum is taken modulo the period (non-negative).
//
// A lane owns IL_VEC = 4 adjacent output pixels of one row, all three channels (x is the fastest spatial dimension of
// both layouts).  Horizontal pass: four table rows per lane, every tap one packed 3-byte pixel read through the aligned
// dwords that cover it.  Vertical pass: one table row per lane (wave-uniform but for the row ends), every tap the 12
// packed bytes of the four pixels through the 3 or 4 aligned dwords that cover them.  Stores are dwords where the
// address allows: three for 4 HWC pixels, one per plane for 4 planar pixels; the row tail, a row that starts at an
// address that is no multiple of 4 (widths that are no multiple of 4), a chunk across the wrap column and any other
// stride pattern go byte by byte.  The tap loop is a loop over the row's own xmax <= ksize taps: any ksize is served,
// nothing is staged in LDS (neighbouring lanes share most of their taps, which the vector cache serves).
//
// Tables, table index and shifts are device data that nobody has validated: the kernel clamps the table, the table row,
// the tap range and every source index into range, so no access leaves the arrays whatever they hold.
//
// image_nonstatic_mask_kernel: mask[x, y] = OR_{i >= 1} AND_c (img[0, c, y, x] != img[i, c, y, x]) for uint8
// [n, 3, H, W], written TRANSPOSED as [W, H] (the reference's proj_size orientation) through a 64 x 64 LDS tile, so
// that the reads run along x and the writes along y.  One launch.
#include "dva_common.h"

namespace dva {

constexpr int IL_TPB = 256;
constexpr int IL_VEC = 4;                 // adjacent output pixels of a lane
constexpr int64_t IL_MAX_BLOCKS = 1 << 20;
constexpr int IL_BITS = 22;               // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int NM_TILE = 64;

struct IlPass {
  const uint8_t* src;
  uint8_t* dst;
  int64_t B;
  int64_t sb, sy, sx, sc;                 // byte strides of the source: image, row, column, channel
  int64_t db, dy, dx, dc;                 // and of the destination
  int src_h, src_w, dst_h, dst_w;
  const int32_t* coeffs;                  // [n_tables, table_rows, ksize]
  const int32_t* bounds;                  // [n_tables, table_rows, 2] = (xmin, xmax)
  const int32_t* table_index;             // [B] or null (table 0)
  const int32_t* shifts;                  // [B, 3] or null (zeros)
  int n_tables, table_rows, ksize;
  int out_period, src_period, other_period;
};

__device__ __forceinline__ int il_clampi(int64_t v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// the first index of a shifted run: (v mod period) with a period, v itself without
__device__ __forceinline__ int64_t il_start(int64_t v, int period) {
  if (period > 0) {
    v %= period;
    if (v < 0) v += period;
  }
  return v;
}

// index `start + k` of a run (0 <= k < size): wrapped once with a period (start < period == size), then clamped into
// the axis whatever the arguments were
__device__ __forceinline__ int il_at(int64_t start, int k, int period, int size) {
  int64_t v = start + k;
  if (period > 0 && v >= period) v -= period;
  return il_clampi(v, 0, size - 1);
}

// 3 packed bytes at ANY address in bits 0..23, through the aligned dwords that hold them
__device__ __forceinline__ uint32_t il_load3(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const int sh = (int)(a & 3) * 8;
  uint32_t v = q[0] >> sh;
  if (sh > 8) v |= q[1] << (32 - sh);     // the pixel runs into the next dword
  return v & 0xffffffu;
}

// 12 packed bytes at ANY address as 3 words, through the 3 (aligned address) or 4 aligned dwords that hold them
__device__ __forceinline__ void il_load12(const uint8_t* p, uint32_t* w) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const int sh = (int)(a & 3) * 8;
  uint32_t lo = q[0];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint32_t hi = (j < 2 || sh) ? q[j + 1] : 0u;
    w[j] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    lo = hi;
  }
}

__device__ __forceinline__ uint32_t il_clip8(int s) {
  s >>= IL_BITS;                           // arithmetic shift
  return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

struct IlRow {
  const int32_t* k;
  int xmin, xmax;
};

// row `r` of a table over a source axis of `size` pixels, the tap range clamped into the axis and into ksize
__device__ __forceinline__ IlRow il_row(const IlPass& P, const int32_t* coeffs, const int32_t* bounds, int64_t r,
                                        int size) {
  const int row = il_clampi(il_start(r, P.out_period), 0, P.table_rows - 1);
  IlRow o;
  o.k = coeffs + (int64_t)row * P.ksize;
  o.xmin = il_clampi(bounds[2 * row], 0, size - 1);
  const int room = size - o.xmin < P.ksize ? size - o.xmin : P.ksize;
  o.xmax = il_clampi(bounds[2 * row + 1], 0, room);
  return o;
}

template <int AXIS>
__global__ __launch_bounds__(IL_TPB) void image_resample_u8_kernel(IlPass P) {
  const int chunks = (P.dst_w + IL_VEC - 1) / IL_VEC;
  const int64_t total = P.B * P.dst_h * chunks;
  const bool src_packed = P.sc == 1 && P.sx == 3;
  for (int64_t t = (int64_t)blockIdx.x * IL_TPB + threadIdx.x; t < total; t += (int64_t)gridDim.x * IL_TPB) {
    const int64_t line = t / chunks;                          // b * dst_h + y
    const int x0 = (int)(t - line * chunks) * IL_VEC;
    const int64_t b = line / P.dst_h;
    const int y = (int)(line - b * P.dst_h);
    const int n = P.dst_w - x0 < IL_VEC ? P.dst_w - x0 : IL_VEC;
    const int table = P.table_index ? il_clampi(P.table_index[b], 0, P.n_tables - 1) : 0;
    const int64_t sh_out = P.shifts ? P.shifts[3 * b] : 0, sh_src = P.shifts ? P.shifts[3 * b + 1] : 0,
                  sh_oth = P.shifts ? P.shifts[3 * b + 2] : 0;
    const int32_t* coeffs = P.coeffs + (int64_t)table * P.table_rows * P.ksize;
    const int32_t* bounds = P.bounds + (int64_t)table * P.table_rows * 2;
    const uint8_t* simg = P.src + b * P.sb;
    int acc[IL_VEC][3];
#pragma unroll
    for (int p = 0; p < IL_VEC; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 1 << (IL_BITS - 1);

    if (AXIS == 0) {
      // along x: the other axis is y; every output pixel has its own table row
      const int sy = il_at(il_start(y + sh_oth, P.other_period), 0, P.other_period, P.src_h);
      const uint8_t* srow = simg + sy * P.sy;
      for (int p = 0; p < n; ++p) {
        const IlRow r = il_row(P, coeffs, bounds, x0 + p + sh_out, P.src_w);
        const int64_t start = il_start(r.xmin + sh_src, P.src_period);
        for (int k = 0; k < r.xmax; ++k) {
          const uint8_t* px = srow + il_at(start, k, P.src_period, P.src_w) * P.sx;
          const int c = r.k[k];
          if (src_packed) {
            const uint32_t v = il_load3(px);
            acc[p][0] += (int)(v & 0xffu) * c;
            acc[p][1] += (int)((v >> 8) & 0xffu) * c;
            acc[p][2] += (int)(v >> 16) * c;
          } else {
            acc[p][0] += (int)px[0] * c;
            acc[p][1] += (int)px[P.sc] * c;
            acc[p][2] += (int)px[2 * P.sc] * c;
          }
        }
      }
    } else {
      // along y: the other axis is x; the four pixels share one table row
      const IlRow r = il_row(P, coeffs, bounds, y + sh_out, P.src_h);
      const int64_t start = il_start(r.xmin + sh_src, P.src_period);
      const int64_t ostart = il_start(x0 + sh_oth, P.other_period);
      const int ox0 = il_at(ostart, 0, P.other_period, P.src_w);
      // the four source columns are adjacent when the chunk neither wraps nor meets the clamp
      const bool run = src_packed && n == IL_VEC && ostart >= 0 && ostart + IL_VEC <= P.src_w;
      int ox[IL_VEC];
#pragma unroll
      for (int p = 0; p < IL_VEC; ++p) ox[p] = il_at(ostart, p, P.other_period, P.src_w);
      for (int k = 0; k < r.xmax; ++k) {
        const uint8_t* srow = simg + il_at(start, k, P.src_period, P.src_h) * P.sy;
        const int c = r.k[k];
        if (run) {
          uint32_t w[3];
          il_load12(srow + (int64_t)ox0 * 3, w);
#pragma unroll
          for (int j = 0; j < 12; ++j) acc[j / 3][j % 3] += (int)((w[j / 4] >> (8 * (j % 4))) & 0xffu) * c;
        } else {
          for (int p = 0; p < n; ++p) {
            const uint8_t* px = srow + ox[p] * P.sx;
            acc[p][0] += (int)px[0] * c;
            acc[p][1] += (int)px[P.sc] * c;
            acc[p][2] += (int)px[2 * P.sc] * c;
          }
        }
      }
    }

    uint8_t* d = P.dst + b * P.db + y * P.dy + x0 * P.dx;
    uint32_t v[IL_VEC][3];
#pragma unroll
    for (int p = 0; p < IL_VEC; ++p) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[p][c] = il_clip8(acc[p][c]);
    }
    if (n == IL_VEC && P.dc == 1 && P.dx == 3 && ((uintptr_t)d & 3) == 0) {
      // four HWC pixels: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      uint32_t* o = reinterpret_cast<uint32_t*>(d);
      o[0] = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[1][0] << 24);
      o[1] = v[1][1] | (v[1][2] << 8) | (v[2][0] << 16) | (v[2][1] << 24);
      o[2] = v[2][2] | (v[3][0] << 8) | (v[3][1] << 16) | (v[3][2] << 24);
    } else if (n == IL_VEC && P.dx == 1 && ((uintptr_t)d & 3) == 0 && (P.dc & 3) == 0) {
      // four pixels of each plane
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<uint32_t*>(d + c * P.dc) = v[0][c] | (v[1][c] << 8) | (v[2][c] << 16) | (v[3][c] << 24);
    } else {
      for (int p = 0; p < n; ++p) {
        d[p * P.dx] = (uint8_t)v[p][0];
        d[p * P.dx + P.dc] = (uint8_t)v[p][1];
        d[p * P.dx + 2 * P.dc] = (uint8_t)v[p][2];
      }
    }
  }
}

// grid (ceil(W / 64), ceil(H / 64)), 256 lanes = 64 columns x 4 rows of the tile at a time
__global__ __launch_bounds__(IL_TPB) void image_nonstatic_mask_kernel(const uint8_t* __restrict__ img, int n, int H, int W,
                                                                      uint8_t* __restrict__ out) {
  __shared__ uint8_t tile[NM_TILE][NM_TILE + 4];
  const int x0 = blockIdx.x * NM_TILE, y0 = blockIdx.y * NM_TILE;
  const int lx = threadIdx.x & (NM_TILE - 1), ly = threadIdx.x / NM_TILE;
  const int64_t hw = (int64_t)H * W;
#pragma unroll 1
  for (int yy = ly; yy < NM_TILE; yy += IL_TPB / NM_TILE) {
    const int x = x0 + lx, y = y0 + yy;
    uint8_t m = 0;
    if (x < W && y < H) {
      const int64_t e = (int64_t)y * W + x;
      const uint8_t r = img[e], g = img[e + hw], bl = img[e + 2 * hw];
#pragma unroll 1
      for (int i = 1; i < n; ++i) {
        const uint8_t* q = img + (int64_t)i * 3 * hw + e;
        m |= (uint8_t)((q[0] != r) & (q[hw] != g) & (q[2 * hw] != bl));
      }
    }
    tile[yy][lx] = m;
  }
  __syncthreads();
  for (int xx = ly; xx < NM_TILE; xx += IL_TPB / NM_TILE) {
    const int x = x0 + xx, y = y0 + lx;
    if (x < W && y < H) out[(int64_t)x * H + y] = tile[lx][xx];
  }
}

// the last byte a strided [B, h, w, 3] array touches, or -1 when that does not fit int64 comfortably
static int64_t il_extent(int64_t B, int64_t h, int64_t w, int64_t sb, int64_t sy, int64_t sx, int64_t sc) {
  const int64_t lim = (int64_t)1 << 60;
  const int64_t n[4] = {B - 1, h - 1, w - 1, 2}, s[4] = {sb, sy, sx, sc};
  int64_t e = 0;
  for (int i = 0; i < 4; ++i) {
    if (n[i] > 0 && s[i] > lim / n[i]) return -1;
    e += n[i] * s[i];
    if (e > lim) return -1;
  }
  return e;
}

}  // namespace dva

using namespace dva;

extern "C" {

int64_t dva_image_resample_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  if (B < 0 || H < 0 || W < 0) return DVA_ERR_INVALID;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL || B > 0x7fffffffLL) return DVA_ERR_UNSUPPORTED;
  const int64_t lim = (int64_t)1 << 40;
  if (H * W > lim / 3 || (B > 0 && H * W * 3 > lim / B)) return DVA_ERR_UNSUPPORTED;
  return (int64_t)align_up((size_t)(B * H * W * 3 > 0 ? B * H * W * 3 : 1));
}

int dva_image_resample_u8(const uint8_t* src, int64_t B, int64_t src_h, int64_t src_w, int64_t src_stride_b,
                          int64_t src_stride_y, int64_t src_stride_x, int64_t src_stride_c, uint8_t* dst, int64_t dst_h,
                          int64_t dst_w, int64_t dst_stride_b, int64_t dst_stride_y, int64_t dst_stride_x,
                          int64_t dst_stride_c, int32_t axis, const int32_t* coeffs, const int32_t* bounds,
                          int64_t n_tables, int64_t table_rows, int32_t ksize, const int32_t* table_index,
                          const int32_t* shifts, int32_t out_period, int32_t src_period, int32_t other_period,
                          void* stream) {
  if (B < 0 || src_h < 0 || src_w < 0 || dst_h < 0 || dst_w < 0) return DVA_ERR_INVALID;
  if (axis != 0 && axis != 1) return DVA_ERR_INVALID;
  if (n_tables < 1 || table_rows < 1 || ksize < 1) return DVA_ERR_INVALID;
  if (out_period < 0 || src_period < 0 || other_period < 0) return DVA_ERR_INVALID;
  if (src_stride_b < 0 || src_stride_y < 1 || src_stride_x < 1 || src_stride_c < 1) return DVA_ERR_INVALID;
  if (dst_stride_b < 1 || dst_stride_y < 1 || dst_stride_x < 1 || dst_stride_c < 1) return DVA_ERR_INVALID;
  // a period is the length of the axis it wraps
  const int64_t axis_size = axis == 0 ? src_w : src_h, other_size = axis == 0 ? src_h : src_w;
  if ((src_period && src_period != axis_size) || (other_period && other_period != other_size)) return DVA_ERR_INVALID;
  if (out_period > table_rows) return DVA_ERR_INVALID;
  if (B == 0 || dst_h == 0 || dst_w == 0) return DVA_OK;
  if (src_h < 1 || src_w < 1) return DVA_ERR_INVALID;         // something to write and nothing to read
  if (!src || !dst || !coeffs || !bounds) return DVA_ERR_INVALID;
  if (src_h > 0x7fffffffLL || src_w > 0x7fffffffLL || dst_h > 0x7fffffffLL || dst_w > 0x7fffffffLL - IL_VEC ||
      n_tables > 0x7fffffffLL || table_rows > 0x7fffffffLL || B > 0x7fffffffLL)
    return DVA_ERR_UNSUPPORTED;
  if (il_extent(B, src_h, src_w, src_stride_b, src_stride_y, src_stride_x, src_stride_c) < 0 ||
      il_extent(B, dst_h, dst_w, dst_stride_b, dst_stride_y, dst_stride_x, dst_stride_c) < 0)
    return DVA_ERR_UNSUPPORTED;
  const int64_t chunks = (dst_w + IL_VEC - 1) / IL_VEC;
  if (B * dst_h > ((int64_t)1 << 60) / chunks) return DVA_ERR_UNSUPPORTED;
  IlPass P;
  P.src = src, P.dst = dst, P.B = B;
  P.sb = src_stride_b, P.sy = src_stride_y, P.sx = src_stride_x, P.sc = src_stride_c;
  P.db = dst_stride_b, P.dy = dst_stride_y, P.dx = dst_stride_x, P.dc = dst_stride_c;
  P.src_h = (int)src_h, P.src_w = (int)src_w, P.dst_h = (int)dst_h, P.dst_w = (int)dst_w;
  P.coeffs = coeffs, P.bounds = bounds, P.table_index = table_index, P.shifts = shifts;
  P.n_tables = (int)n_tables, P.table_rows = (int)table_rows, P.ksize = ksize;
  P.out_period = out_period, P.src_period = src_period, P.other_period = other_period;
  const dim3 grid((unsigned)capped_grid(B * dst_h * chunks, IL_TPB, IL_MAX_BLOCKS));
  if (axis == 0)
    hipLaunchKernelGGL(image_resample_u8_kernel<0>, grid, dim3(IL_TPB), 0, (hipStream_t)stream, P);
  else
    hipLaunchKernelGGL(image_resample_u8_kernel<1>, grid, dim3(IL_TPB), 0, (hipStream_t)stream, P);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

int dva_image_nonstatic_mask(const uint8_t* images, int64_t n, int64_t H, int64_t W, uint8_t* mask, void* stream) {
  if (n < 1 || H < 0 || W < 0) return DVA_ERR_INVALID;
  if (H == 0 || W == 0) return DVA_OK;
  if (!images || !mask) return DVA_ERR_INVALID;
  if (n > 0x7fffffffLL || W > 0x7fffffffLL - NM_TILE || H > (int64_t)65535 * NM_TILE) return DVA_ERR_UNSUPPORTED;
  if (H * W > ((int64_t)1 << 40) / (3 * n)) return DVA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks_for(W, NM_TILE), (unsigned)blocks_for(H, NM_TILE));
  hipLaunchKernelGGL(image_nonstatic_mask_kernel, grid, dim3(IL_TPB), 0, (hipStream_t)stream, images, (int)n, (int)H,
                     (int)W, mask);
  DVA_CHECK_LAUNCH();
  return DVA_OK;
}

}  // extern "C"
