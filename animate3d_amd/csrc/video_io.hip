// The two byte ends of MV-VDM generation on gfx950 (host side and contract: animate3d_amd/video.py, animate3d_amd/pipeline.py).
//
//   a3d_images_in_u8   the front of the reference's encode_latents (animatediff/pipelines/pipeline.py:548-554): condition images as bytes
//                      [n, H, W, Cin] (Cin 3 or 4, a fourth channel is ignored) -> fp32 planar [n, 3, H, W] = (b / 255.0f - 0.5f) / 0.5f, the
//                      bits of torch's uint8 / 255 followed by Normalize(0.5, 0.5) on the CPU: IEEE division and subtraction as written, no
//                      reciprocal multiply, nothing contracted.  Where asked for also unit [n, H, W, 3] = b / 255.0f, the float image
//                      clip.preprocess_frames reads: its (uint8)(v * 255.0f) returns b for every one of the 256 bytes.
//   a3d_video_to_u8    the tail decode_latents -> tensor2vid -> VaeImageProcessor.postprocess -> numpy_to_pil (:566-577, :237-255): the
//                      decoder's conv_out rows [(n F) H W, 4] in bf16 / fp16, or an fp32 planar video [n, 3, F, H, W], -> bytes at
//                      dst + v s_view + f s_frame + y s_row + x pixel.  Per value: widen to fp32, clamp(x / 2 + 0.5, 0, 1) * 255.0f rounded to
//                      fp32, then round half to even (numpy's round).  A NaN gives 0: the reference's astype(uint8) of a NaN is not defined.
//                      pixel 4: the fourth byte is 255.
//
// Memory-bound elementwise work: a thread owns four neighbouring pixels of one row (two 16-byte loads of 16-bit rows, one per channel plane of
// fp32; 16-byte stores of the planes, one 12- or 16-byte store of the bytes) in a grid-stride loop.  Shapes that do not allow that (a pixel
// count per image or a width that is no multiple of 4, a destination that is not 4-byte aligned on the planar path) run one pixel per thread
// with scalar accesses.  No LDS, no atomics, no workspace, no host synchronisation, one launch each; every output byte is written once.
#include "common.h"

namespace {

constexpr int VIO_BLOCK = 256;
constexpr int64_t VIO_MAX_PIXELS = 0x7fffffffLL;          // pixels of one launch: every quad and pixel index fits 31 bits

typedef uint32_t u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// (b / 255.0f - 0.5f) / 0.5f and b / 255.0f: each operation rounded once
A3D_DEV float vio_unit(uint32_t b) { return __fdiv_rn((float)b, 255.0f); }
A3D_DEV float vio_norm(float unit) { return __fdiv_rn(__fsub_rn(unit, 0.5f), 0.5f); }

// round_half_even(clamp(x / 2 + 0.5, 0, 1) * 255.0f); the comparisons are written so that a NaN takes the first branch
A3D_DEV uint32_t vio_byte(float x) {
  float t = __fadd_rn(__fdiv_rn(x, 2.0f), 0.5f);
  t = t >= 0.f ? t : 0.f;
  t = t <= 1.f ? t : 1.f;
  return (uint32_t)(int)rintf(__fmul_rn(t, 255.0f));
}

A3D_DEV float vio_widen(uint32_t bits16, int dtype) {
  return dtype == A3D_BF16 ? __uint_as_float(bits16 << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}

// ---- a3d_images_in_u8
// quads: a thread reads the 4 cin bytes of pixels 4 q .. 4 q + 3 (P % 4 == 0: all of one image) as words
__global__ __launch_bounds__(VIO_BLOCK) void images_in_quad_kernel(int64_t quads, int64_t P, int cin, const uint32_t* __restrict__ src,
                                                                   float* __restrict__ planar, float* __restrict__ unit) {
  for (int64_t q = (int64_t)blockIdx.x * VIO_BLOCK + threadIdx.x; q < quads; q += (int64_t)gridDim.x * VIO_BLOCK) {
    uint32_t b[4][3];
    if (cin == 4) {
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(src + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j][0] = w[j] & 0xffu, b[j][1] = (w[j] >> 8) & 0xffu, b[j][2] = (w[j] >> 16) & 0xffu;
    } else {
      const u32x3_a4 w = *reinterpret_cast<const u32x3_a4*>(src + 3 * q);
#pragma unroll
      for (int k = 0; k < 12; ++k) b[k / 3][k % 3] = (w[k / 4] >> (8 * (k % 4))) & 0xffu;
    }
    float u[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) u[j][c] = vio_unit(b[j][c]);
    const int64_t p0 = 4 * q, img = p0 / P, p = p0 - img * P;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4_t v = {vio_norm(u[0][c]), vio_norm(u[1][c]), vio_norm(u[2][c]), vio_norm(u[3][c])};
      *reinterpret_cast<f32x4_t*>(planar + (img * 3 + c) * P + p) = v;
    }
    if (unit) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const f32x4_t v = {u[(4 * k) / 3][(4 * k) % 3], u[(4 * k + 1) / 3][(4 * k + 1) % 3], u[(4 * k + 2) / 3][(4 * k + 2) % 3],
                             u[(4 * k + 3) / 3][(4 * k + 3) % 3]};
        *reinterpret_cast<f32x4_t*>(unit + 12 * q + 4 * k) = v;
      }
    }
  }
}

__global__ __launch_bounds__(VIO_BLOCK) void images_in_pixel_kernel(int64_t pixels, int64_t P, int cin, const uint8_t* __restrict__ src,
                                                                    float* __restrict__ planar, float* __restrict__ unit) {
  for (int64_t o = (int64_t)blockIdx.x * VIO_BLOCK + threadIdx.x; o < pixels; o += (int64_t)gridDim.x * VIO_BLOCK) {
    const int64_t img = o / P, p = o - img * P;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = vio_unit(src[o * cin + c]);
      planar[(img * 3 + c) * P + p] = vio_norm(u);
      if (unit) unit[3 * o + c] = u;
    }
  }
}

// ---- a3d_video_to_u8
struct VideoOutArgs {
  const void* src;
  uint8_t* dst;
  int64_t s_view, s_frame, s_row;
  int dtype, F, H, W, pixel;
};

// the bytes of four neighbouring pixels, b[j][c], at `at` (4-byte aligned): 12 bytes r g b r g b ... or four words r | g << 8 | b << 16 | 255 << 24
A3D_DEV void vio_store_quad(uint8_t* at, int pixel, const uint32_t (&b)[4][3]) {
  if (pixel == 4) {
    u32x4_a4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = b[j][0] | (b[j][1] << 8) | (b[j][2] << 16) | 0xff000000u;
    *reinterpret_cast<u32x4_a4*>(at) = w;
  } else {
    u32x3_a4 w = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k / 4] |= b[k / 3][k % 3] << (8 * (k % 4));
    *reinterpret_cast<u32x3_a4*>(at) = w;
  }
}

// quad q = ((v F + f) H + y) (W / 4) + xq
A3D_DEV uint8_t* vio_quad_dst(const VideoOutArgs& a, int64_t q, int64_t& vf, int& y, int& xq) {
  const int wq = a.W / 4;
  xq = (int)(q % wq);
  const int64_t row = q / wq;
  y = (int)(row % a.H);
  vf = row / a.H;
  const int64_t v = vf / a.F, f = vf - v * a.F;
  return a.dst + v * a.s_view + f * a.s_frame + (int64_t)y * a.s_row + (int64_t)xq * 4 * a.pixel;
}

// 16-bit rows [(n F) H W, 4]: quad q is 32 contiguous bytes, pixel j its words 2 j (channels 0 | 1) and 2 j + 1 (channel 2 | padding)
__global__ __launch_bounds__(VIO_BLOCK) void video_rows_quad_kernel(int64_t quads, const VideoOutArgs a) {
  const u32x4_t* src = reinterpret_cast<const u32x4_t*>(a.src);
  for (int64_t q = (int64_t)blockIdx.x * VIO_BLOCK + threadIdx.x; q < quads; q += (int64_t)gridDim.x * VIO_BLOCK) {
    const u32x4_t lo = src[2 * q], hi = src[2 * q + 1];
    const uint32_t w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    uint32_t b[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[j][0] = vio_byte(vio_widen(w[2 * j] & 0xffffu, a.dtype));
      b[j][1] = vio_byte(vio_widen(w[2 * j] >> 16, a.dtype));
      b[j][2] = vio_byte(vio_widen(w[2 * j + 1] & 0xffffu, a.dtype));
    }
    int64_t vf;
    int y, xq;
    uint8_t* at = vio_quad_dst(a, q, vf, y, xq);
    vio_store_quad(at, a.pixel, b);
  }
}

// fp32 planar [n, 3, F, H, W], W % 4 == 0: one 16-byte load per channel plane
__global__ __launch_bounds__(VIO_BLOCK) void video_planar_quad_kernel(int64_t quads, const VideoOutArgs a) {
  const float* src = reinterpret_cast<const float*>(a.src);
  const int64_t P = (int64_t)a.H * a.W, FP = a.F * P;
  for (int64_t q = (int64_t)blockIdx.x * VIO_BLOCK + threadIdx.x; q < quads; q += (int64_t)gridDim.x * VIO_BLOCK) {
    int64_t vf;
    int y, xq;
    uint8_t* at = vio_quad_dst(a, q, vf, y, xq);
    const int64_t v = vf / a.F, f = vf - v * a.F;
    const float* p = src + v * 3 * FP + f * P + (int64_t)y * a.W + 4 * xq;
    uint32_t b[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4_t x = *reinterpret_cast<const f32x4_t*>(p + c * FP);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j][c] = vio_byte(x[j]);
    }
    vio_store_quad(at, a.pixel, b);
  }
}

// fp32 planar, any W, any destination alignment: one pixel per thread, byte stores
__global__ __launch_bounds__(VIO_BLOCK) void video_planar_pixel_kernel(int64_t pixels, const VideoOutArgs a) {
  const float* src = reinterpret_cast<const float*>(a.src);
  const int64_t P = (int64_t)a.H * a.W, FP = a.F * P;
  for (int64_t o = (int64_t)blockIdx.x * VIO_BLOCK + threadIdx.x; o < pixels; o += (int64_t)gridDim.x * VIO_BLOCK) {
    const int x = (int)(o % a.W);
    const int64_t row = o / a.W;
    const int y = (int)(row % a.H);
    const int64_t vf = row / a.H, v = vf / a.F, f = vf - v * a.F;
    const float* p = src + v * 3 * FP + f * P + (int64_t)y * a.W + x;
    uint8_t* at = a.dst + v * a.s_view + f * a.s_frame + (int64_t)y * a.s_row + (int64_t)x * a.pixel;
#pragma unroll
    for (int c = 0; c < 3; ++c) at[c] = (uint8_t)vio_byte(p[c * FP]);
    if (a.pixel == 4) at[3] = 255;
  }
}

// pixels of a launch: 0 for a refusal (an extent that is not positive, more than VIO_MAX_PIXELS pixels)
int64_t vio_pixels(int64_t a, int64_t b, int64_t c, int64_t d) {
  if (a <= 0 || b <= 0 || c <= 0 || d <= 0) return 0;
  if (b > VIO_MAX_PIXELS / a || c > VIO_MAX_PIXELS / (a * b) || d > VIO_MAX_PIXELS / (a * b * c)) return 0;
  return a * b * c * d;
}

}  // namespace

extern "C" int a3d_images_in_u8(a3d_stream_t stream, const uint8_t* images, int n, int H, int W, int cin, float* planar, float* unit) {
  const int64_t pixels = vio_pixels(n, H, W, 1);
  if (pixels == 0 || !images || !planar || (cin != 3 && cin != 4)) return A3D_EINVAL;
  if (!a3d_aligned(4, images) || !a3d_aligned(16, planar, unit)) return A3D_EINVAL;
  const int64_t P = (int64_t)H * W;
  if (P % 4 == 0 && (cin == 3 || a3d_aligned(16, images))) {
    const int64_t quads = pixels / 4;
    images_in_quad_kernel<<<grid_for(quads, VIO_BLOCK), VIO_BLOCK, 0, (hipStream_t)stream>>>(quads, P, cin, reinterpret_cast<const uint32_t*>(images),
                                                                                            planar, unit);
  } else {
    images_in_pixel_kernel<<<grid_for(pixels, VIO_BLOCK), VIO_BLOCK, 0, (hipStream_t)stream>>>(pixels, P, cin, images, planar, unit);
  }
  return a3d_launch_status();
}

extern "C" int a3d_video_to_u8(a3d_stream_t stream, const void* video, int dtype, int n, int F, int H, int W, uint8_t* dst, int64_t s_view,
                               int64_t s_frame, int64_t s_row, int pixel) {
  const int64_t pixels = vio_pixels(n, F, H, W);
  if (pixels == 0 || !video || !dst || (pixel != 3 && pixel != 4)) return A3D_EINVAL;
  if (dtype != A3D_F32 && dtype != A3D_BF16 && dtype != A3D_F16) return A3D_EINVAL;
  if (s_view < 0 || s_frame < 0 || s_row < (int64_t)W * pixel) return A3D_EINVAL;
  const bool dst4 = a3d_aligned(4, dst) && ((s_view | s_frame | s_row) & 3) == 0;
  VideoOutArgs a;
  a.src = video; a.dst = dst; a.s_view = s_view; a.s_frame = s_frame; a.s_row = s_row;
  a.dtype = dtype; a.F = F; a.H = H; a.W = W; a.pixel = pixel;
  hipStream_t st = (hipStream_t)stream;
  if (dtype != A3D_F32) {                                  // the decoder's rows: quads only
    if (W % 4 != 0 || !dst4 || !a3d_aligned(16, video)) return A3D_EINVAL;
    video_rows_quad_kernel<<<grid_for(pixels / 4, VIO_BLOCK), VIO_BLOCK, 0, st>>>(pixels / 4, a);
  } else {
    if (!a3d_aligned(4, video)) return A3D_EINVAL;
    if (W % 4 == 0 && dst4 && a3d_aligned(16, video))
      video_planar_quad_kernel<<<grid_for(pixels / 4, VIO_BLOCK), VIO_BLOCK, 0, st>>>(pixels / 4, a);
    else
      video_planar_pixel_kernel<<<grid_for(pixels, VIO_BLOCK), VIO_BLOCK, 0, st>>>(pixels, a);
  }
  return a3d_launch_status();
}
