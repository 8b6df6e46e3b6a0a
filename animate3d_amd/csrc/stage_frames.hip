// Frames of the 4-D stage on gfx950: 8-bit RGBA ground truth in, 8-bit RGBA test renders out; contract in animate3d_amd/frames.py.
// Replaces the per-image CPU arithmetic of custom/threestudio-animate3d/data/simple_multi_image.py:205-215 (astype(float32) / 255.0,
// alpha > 0.5) and of systems/animate3d.py:441-445 (torch.cat, (rgba_img * 255).astype(np.uint8)).
//
//   frames_unpack_kernel   one thread per output pixel of [S, H, W]: the k x k source pixels of rgba8 [S, k H, k W, 4] are read as one 4-byte
//                          word each and summed per channel in integers; q = (2 sum + k^2) / (2 k^2), the exact mean rounded half up
//                          (k = 1: q is the byte).  Written, each where asked for: the four q as one word, rgb = (float)q / 255.0f by IEEE
//                          division (a multiply by a reciprocal differs for 126 of the 256 bytes), mask = q_alpha >= 128 (q / 255.0f > 0.5f)
//   frames_pack_kernel     one thread per pixel of image [B, 3, P] planar and alpha [B, P]: the word of (uint8)(clamp01(v) * 255.0f),
//                          truncating, for r, g, b and alpha; a NaN gives 0
// No atomics, no workspace, no host synchronisation, one launch each; a result depends on its own inputs only.
#include "common.h"

namespace {

constexpr int SF_BLOCK = 256;
constexpr int SF_MAX_K = 16;                       // sums stay below 2^17

__global__ __launch_bounds__(SF_BLOCK) void frames_unpack_kernel(int64_t n, int H, int W, int k, const uint32_t* __restrict__ src,
                                                                 uint32_t* __restrict__ out8, float* __restrict__ rgb,
                                                                 uint8_t* __restrict__ mask) {
  const int64_t o = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;          // (s H + y) W + x
  if (o >= n) return;
  const int x = (int)(o % W);
  const int64_t row = o / W;                                                // s H + y: source rows k row .. k row + k - 1
  const uint32_t* p = src + (row * k * W + x) * k;                          // source row length k W
  uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int dy = 0; dy < k; ++dy, p += (int64_t)k * W)
    for (int dx = 0; dx < k; ++dx) {
      const uint32_t w = p[dx];
      s0 += w & 0xffu, s1 += (w >> 8) & 0xffu, s2 += (w >> 16) & 0xffu, s3 += w >> 24;
    }
  const uint32_t kk = (uint32_t)(k * k), den = 2u * kk;
  const uint32_t q0 = (2u * s0 + kk) / den, q1 = (2u * s1 + kk) / den, q2 = (2u * s2 + kk) / den, q3 = (2u * s3 + kk) / den;
  if (out8) out8[o] = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
  if (rgb) {
    rgb[3 * o] = (float)q0 / 255.0f;
    rgb[3 * o + 1] = (float)q1 / 255.0f;
    rgb[3 * o + 2] = (float)q2 / 255.0f;
  }
  if (mask) mask[o] = q3 >= 128u ? 1 : 0;
}

A3D_DEV uint32_t sf_byte(float v) { return (uint32_t)(uint8_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

__global__ __launch_bounds__(SF_BLOCK) void frames_pack_kernel(int64_t n, int64_t P, const float* __restrict__ image,
                                                               const float* __restrict__ alpha, uint32_t* __restrict__ out) {
  const int64_t o = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;          // b P + p
  if (o >= n) return;
  const int64_t b = o / P, p = o - b * P;
  const float* img = image + b * 3 * P + p;
  out[o] = sf_byte(img[0]) | (sf_byte(img[P]) << 8) | (sf_byte(img[2 * P]) << 16) | (sf_byte(alpha[o]) << 24);
}

// pixels of a launch: 0 for a refusal (an extent that is not positive, 2^39 pixels or more: one thread each, 2^31 - 1 blocks at most)
int64_t sf_pixels(int64_t a, int64_t b, int64_t c) {
  if (a <= 0 || b <= 0 || c <= 0) return 0;
  const int64_t limit = ((int64_t)1 << 39) - 1;
  if (b > limit / a || c > limit / (a * b)) return 0;
  return a * b * c;
}

unsigned sf_blocks(int64_t n) { return (unsigned)((n + SF_BLOCK - 1) / SF_BLOCK); }

}  // namespace

extern "C" int a3d_frames_unpack_u8(a3d_stream_t stream, int S, int h, int w, int k, const uint8_t* rgba8, uint8_t* out8, float* rgb,
                                    uint8_t* mask) {
  if (k < 1 || k > SF_MAX_K || h <= 0 || w <= 0 || h % k != 0 || w % k != 0) return A3D_EINVAL;
  if (sf_pixels(S, h, w) == 0) return A3D_EINVAL;                          // the source's extent bounds every index
  if (!rgba8 || (!out8 && !rgb && !mask) || !a3d_aligned(4, rgba8, out8) || !a3d_aligned(4, rgb)) return A3D_EINVAL;
  const int H = h / k, W = w / k;
  const int64_t n = (int64_t)S * H * W;
  frames_unpack_kernel<<<sf_blocks(n), SF_BLOCK, 0, (hipStream_t)stream>>>(n, H, W, k, reinterpret_cast<const uint32_t*>(rgba8),
                                                                           reinterpret_cast<uint32_t*>(out8), rgb, mask);
  return a3d_launch_status();
}

extern "C" int a3d_frames_pack_u8(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, uint8_t* rgba8) {
  const int64_t n = sf_pixels(B, H, W);
  if (n == 0 || !image || !alpha || !rgba8 || !a3d_aligned(4, image, alpha) || !a3d_aligned(4, rgba8)) return A3D_EINVAL;
  frames_pack_kernel<<<sf_blocks(n), SF_BLOCK, 0, (hipStream_t)stream>>>(n, (int64_t)H * W, image, alpha,
                                                                         reinterpret_cast<uint32_t*>(rgba8));
  return a3d_launch_status();
}
