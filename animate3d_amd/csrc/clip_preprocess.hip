// CLIP image pre-processing of rendered frames (host side and contract: animate3d_amd/clip.py, preprocess_frames).
//
// Replaces the device -> host -> PIL -> CLIPImageProcessor -> device round trip of the reference's guidance step
// (custom/threestudio-animate3d/guidance/animatemv_guidance.py:546-555, animatediff/utils/util.py:268-287) by one launch that is bit-equal
// to it: Pillow's 8-bit resampler is integer arithmetic on fixed-point coefficients (22 precision bits), which the host computes exactly
// as Pillow does, and the /255 + mean/std normalisation of a byte is a 256-entry table per channel.
//
// One workgroup makes one tile of one selected frame: `tile_rows` output rows (one row of patches) x crop columns x 3 channels.
//   pass 1 (horizontal): for exactly the input rows r0 .. r1 the tile's vertical pass reads, every output column of every channel:
//           byte = clip8((1 << 21) + sum_k q(rgb[row, first + k, c]) * coef_x[col, k]), with q(v) = (uint8)(v * 255.0f); kept in LDS as
//           [row][channel][column] bytes.  This intermediate is why the tile is not the whole frame: 224 x 3 bytes per input row.
//   pass 2 (vertical): the same arithmetic down the LDS rows, then the look-up and the stores.
// A pass whose table has ksize 0 is skipped as Pillow skips it (equal sizes): it copies at the crop offset.
// No atomics, no dependence on launch geometry: every output element is written once by one thread from integers.
#include "f32_common.h"

namespace {

constexpr int CLIP_PRECISION_BITS = 22;               // Pillow: 32 - 8 - 2
constexpr int CLIP_THREADS = 1024;
constexpr int64_t CLIP_LDS_LIMIT = 64 * 1024;         // dynamic LDS one workgroup may ask for without an attribute change

struct ClipPreArgs {
  const float* rgb;
  int64_t s_img, s_y, s_x, s_c;                        // element strides of rgb
  const int* image_index;                              // [n_img] or NULL (frame n)
  const int *coef_x, *bounds_x, *coef_y, *bounds_y;    // [crop, ksize] and [crop, 2] = (first, count); NULL when ksize is 0
  const float* table;                                  // [3, 256]
  void *pixel_values, *patch_rows;
  uint8_t* u8;
  int n_src, in_h, in_w, crop, ksize_x, ksize_y, off_x, off_y, tile_rows, n_tiles, max_rows, dtype, patch, kp;
};

// (uint8)(v * 255.0f): one float32 multiply, rounded to nearest, then truncation.  NaN and negatives give 0, values above 255 give 255.
A3D_DEV int quantise(float v) {
  float s = __fmul_rn(v, 255.0f);
  s = s >= 0.f ? s : 0.f;
  s = s <= 255.f ? s : 255.f;
  return (int)s;
}

A3D_DEV int clip8(int acc) {
  const int v = acc >> CLIP_PRECISION_BITS;           // arithmetic shift, as Pillow's
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

A3D_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

A3D_DEV void store_as(void* base, int64_t i, float f, int dtype) {
  if (dtype == A3D_F32) reinterpret_cast<float*>(base)[i] = f;
  else if (dtype == A3D_BF16) reinterpret_cast<uint16_t*>(base)[i] = f2bfbits(f);
  else reinterpret_cast<_Float16*>(base)[i] = (_Float16)f;      // round-to-nearest-even
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_preprocess_kernel(const ClipPreArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t inter[];     // [rows][3][crop]
  const int tile = blockIdx.x % a.n_tiles, n = blockIdx.x / a.n_tiles;
  const int src = a.image_index ? a.image_index[n] : n;
  const bool have = src >= 0 && src < a.n_src;                        // an index outside the batch reads nothing: a frame of zero bytes
  const float* img = a.rgb + (have ? (int64_t)src * a.s_img : 0);
  const int crop = a.crop, w3 = 3 * crop;
  const int oy0 = tile * a.tile_rows, oy1 = min(crop, oy0 + a.tile_rows);

  // the input rows this tile's vertical pass reads; clamped to the frame and to the rows the launch reserved LDS for
  int r0, r1;
  if (a.ksize_y == 0) {
    r0 = a.off_y + oy0; r1 = a.off_y + oy1;
  } else {
    r0 = a.bounds_y[2 * oy0];
    r1 = a.bounds_y[2 * (oy1 - 1)] + a.bounds_y[2 * (oy1 - 1) + 1];
  }
  r0 = clampi(r0, 0, a.in_h);
  r1 = min(clampi(r1, r0, a.in_h), r0 + a.max_rows);
  const int rows = r1 - r0;

  for (int e = threadIdx.x; e < rows * w3; e += CLIP_THREADS) {
    const int row = e / w3, rem = e - row * w3, c = rem / crop, ox = rem - c * crop;
    const float* p = img + (int64_t)(r0 + row) * a.s_y + (int64_t)c * a.s_c;
    int v = 0;
    if (have) {
      if (a.ksize_x == 0) {
        v = quantise(p[(int64_t)(a.off_x + ox) * a.s_x]);
      } else {
        const int first = clampi(a.bounds_x[2 * ox], 0, a.in_w);
        const int count = clampi(a.bounds_x[2 * ox + 1], 0, min(a.ksize_x, a.in_w - first));
        const int* k = a.coef_x + (int64_t)ox * a.ksize_x;
        int acc = 1 << (CLIP_PRECISION_BITS - 1);
        for (int i = 0; i < count; ++i) acc += quantise(p[(int64_t)(first + i) * a.s_x]) * k[i];
        v = clip8(acc);
      }
    }
    inter[e] = (uint8_t)v;
  }
  __syncthreads();

  const int out_rows = oy1 - oy0;
  const int g = a.patch > 0 ? crop / a.patch : 0;                     // patches per side
  for (int e = threadIdx.x; e < out_rows * w3; e += CLIP_THREADS) {
    const int oyl = e / w3, rem = e - oyl * w3, c = rem / crop, ox = rem - c * crop;
    const int oy = oy0 + oyl, col = c * crop + ox;
    int b;
    if (a.ksize_y == 0) {
      const int row = a.off_y + oy - r0;
      b = row < rows ? inter[row * w3 + col] : 0;
    } else {
      const int first = clampi(a.bounds_y[2 * oy] - r0, 0, rows);
      const int count = clampi(a.bounds_y[2 * oy + 1], 0, min(a.ksize_y, rows - first));
      const int* k = a.coef_y + (int64_t)oy * a.ksize_y;
      int acc = 1 << (CLIP_PRECISION_BITS - 1);
      for (int i = 0; i < count; ++i) acc += (int)inter[(first + i) * w3 + col] * k[i];
      b = clip8(acc);
    }
    if (a.u8) a.u8[((int64_t)(n * crop + oy) * crop + ox) * 3 + c] = (uint8_t)b;
    const float f = a.table[c * 256 + b];
    if (a.pixel_values) store_as(a.pixel_values, ((int64_t)(n * 3 + c) * crop + oy) * crop + ox, f, a.dtype);
    if (a.patch_rows) {                                               // tile_rows == patch: this tile is patch row `tile`; (c, ky, kx) order
      const int px = ox / a.patch, kx = ox - px * a.patch, ky = oy - tile * a.patch;
      const int64_t r = ((int64_t)n * g + tile) * g + px;
      store_as(a.patch_rows, r * a.kp + (c * a.patch + ky) * a.patch + kx, f, a.dtype);
    }
  }
  if (a.patch_rows) {                                                 // the GEMM contracts in steps of 64: columns k .. kp are zeros
    const int k = 3 * a.patch * a.patch, padc = a.kp - k;
    for (int e = threadIdx.x; e < g * padc; e += CLIP_THREADS) {
      const int px = e / padc, j = e - px * padc;
      store_as(a.patch_rows, (((int64_t)n * g + tile) * g + px) * a.kp + k + j, 0.f, a.dtype);
    }
  }
}

}  // namespace

extern "C" int64_t a3d_clip_preprocess_lds_limit(void) { return CLIP_LDS_LIMIT; }

extern "C" int a3d_clip_preprocess(a3d_stream_t stream, const float* rgb, int n_src, int in_h, int in_w, int64_t s_img, int64_t s_y,
                                   int64_t s_x, int64_t s_c, const int* image_index, int n_img, int crop, const int* coef_x,
                                   const int* bounds_x, int ksize_x, int off_x, const int* coef_y, const int* bounds_y, int ksize_y,
                                   int off_y, int tile_rows, int max_rows, const float* table, int dtype, void* pixel_values,
                                   void* patch_rows, int patch, int kp, uint8_t* u8) {
  if (!rgb || !table || n_src <= 0 || n_img <= 0 || in_h <= 0 || in_w <= 0 || crop <= 0 || tile_rows <= 0 || max_rows <= 0) return A3D_EINVAL;
  if (!pixel_values && !patch_rows && !u8) return A3D_EINVAL;
  if (dtype != A3D_F32 && dtype != A3D_BF16 && dtype != A3D_F16) return A3D_EINVAL;
  if (ksize_x < 0 || ksize_y < 0 || (ksize_x > 0 && (!coef_x || !bounds_x)) || (ksize_y > 0 && (!coef_y || !bounds_y))) return A3D_EINVAL;
  if (ksize_x == 0 && (off_x < 0 || off_x + crop > in_w)) return A3D_EINVAL;        // a skipped pass copies at the crop offset
  if (ksize_y == 0 && (off_y < 0 || off_y + crop > in_h)) return A3D_EINVAL;
  if (!a3d_aligned(4, rgb, table) || !a3d_aligned(4, image_index, coef_x, bounds_x, coef_y, bounds_y)) return A3D_EINVAL;
  if (reinterpret_cast<uintptr_t>(pixel_values) % (dtype == A3D_F32 ? 4 : 2) || reinterpret_cast<uintptr_t>(patch_rows) % (dtype == A3D_F32 ? 4 : 2))
    return A3D_EINVAL;
  if (patch_rows && (patch <= 0 || crop % patch != 0 || tile_rows != patch || kp < 3 * patch * patch)) return A3D_EINVAL;
  const int64_t n_tiles = (crop + tile_rows - 1) / tile_rows;
  if ((int64_t)n_img * 3 * crop * crop > 0x7fffffffLL || n_img * n_tiles > 0x7fffffffLL) return A3D_EINVAL;
  const int64_t lds = (int64_t)max_rows * 3 * crop;                                 // the tile's horizontal-pass intermediate, bytes
  if (lds > CLIP_LDS_LIMIT) return A3D_EUNSUPPORTED;                                // never a smaller intermediate than the passes need
  ClipPreArgs a;
  a.rgb = rgb; a.s_img = s_img; a.s_y = s_y; a.s_x = s_x; a.s_c = s_c;
  a.image_index = image_index;
  a.coef_x = coef_x; a.bounds_x = bounds_x; a.coef_y = coef_y; a.bounds_y = bounds_y;
  a.table = table; a.pixel_values = pixel_values; a.patch_rows = patch_rows; a.u8 = u8;
  a.n_src = n_src; a.in_h = in_h; a.in_w = in_w; a.crop = crop; a.ksize_x = ksize_x; a.ksize_y = ksize_y; a.off_x = off_x; a.off_y = off_y;
  a.tile_rows = tile_rows; a.n_tiles = (int)n_tiles; a.max_rows = max_rows; a.dtype = dtype; a.patch = patch_rows ? patch : 0; a.kp = kp;
  clip_preprocess_kernel<<<(unsigned)(n_img * n_tiles), CLIP_THREADS, (size_t)((lds + 15) / 16 * 16), (hipStream_t)stream>>>(a);
  return a3d_launch_status();
}
