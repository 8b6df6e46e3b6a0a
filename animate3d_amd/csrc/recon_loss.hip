// Reconstruction loss of the 4-D stage on gfx950: the masked RGB / mask MSE of a batch of renders against the tracked frames; contract in
// animate3d_amd/stage4d.py (masked_recon_loss).  Replaces the torch chain of custom/threestudio-animate3d/systems/animate3d.py:160-184 (the
// val[sampled_idx] copies of the ground truth, the compositing with the mask, two F.mse_loss) and the clamp / permute in front of it
// (diff_gaussian_rasterizer_advanced_4d.py:180, gaussian_batch_renderer_4d.py:73).
//
//   recon_fwd_kernel<GT, VEC>  block j of image b covers pixels [j RL_PIXELS, (j + 1) RL_PIXELS) of that image; a thread accumulates RL_RUN
//                           pixels in fp32 (VEC: as RL_RUN / 4 groups of four neighbours, read 16 bytes at a time from the three colour
//                           planes, the alpha plane and the interleaved ground truth, four mask bytes at once), then the block writes
//                           one (rgb, mask) partial.  VEC needs H W % 4 == 0 and 16-byte bases: then every group starts on 16 bytes in
//                           every operand.
//   recon_final_kernel      one block adds the partials; the order of both steps is loss_reduce.h's (no atomics, two calls are bitwise
//                           equal).  out = {lambda_rgb mean_rgb + lambda_mask mean_mask, mean_rgb, mean_mask}
//   recon_bwd_kernel<GT, VEC>  recomputes from the four inputs in the same geometry and writes d_image / d_alpha in the planar layout
//                           a3d_gs_render_bwd_f32 reads; the upstream gradient is read through a device pointer
// GT is where the ground truth comes from, and nothing else of a kernel depends on it: GtF32 reads gt_rgb [S, P, 3] fp32 and gt_mask [S, P]
// bytes (a3d_recon_loss_f32), GtRgba8 reads gt_rgba8 [S, P, 4] bytes, 4 a pixel, 16 for four (a3d_recon_loss_rgba8_f32): colour
// (float)byte / 255.0f by IEEE division and inside = alpha byte >= 128, the bits the fp32 tensors of data/simple_multi_image.py:205-215 hold.
#include "loss_reduce.h"

namespace {

constexpr int RL_RUN = 8;                          // pixels per thread
constexpr int RL_PIXELS = LR_BLOCK * RL_RUN;       // pixels per block: a3d_recon_loss_f32's partials are B * ceil(H W / RL_PIXELS) pairs
static_assert(RL_RUN % 4 == 0 && RL_RUN <= 64, "a thread's run is a bounded number of 4-pixel groups");

// The two sources of the ground truth.  frame(s, P): the source moved to frame s.  inside / colours: pixel p's flag and (r, g, b);
// inside4 / colours4: those of pixels p .. p + 3 (p % 4 == 0) in 16-byte loads.  ok / wide (host): what the scalar / the 16-byte path needs.
#define RL_MEMBER __device__ __forceinline__          // A3D_DEV is static: not for a member
struct GtF32 {
  const float* rgb;     // [S, P, 3]
  const uint8_t* mask;  // [S, P], non-zero: inside
  RL_MEMBER GtF32 frame(int64_t s, int64_t P) const { return GtF32{rgb + s * P * 3, mask + s * P}; }
  RL_MEMBER bool inside(int64_t p) const { return mask[p] != 0; }
  RL_MEMBER void colours(int64_t p, float (&t)[3]) const { t[0] = rgb[3 * p], t[1] = rgb[3 * p + 1], t[2] = rgb[3 * p + 2]; }
  RL_MEMBER void inside4(int64_t p, bool (&m)[4]) const {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(mask + p);
    m[0] = (w & 0xffu) != 0, m[1] = (w & 0xff00u) != 0, m[2] = (w & 0xff0000u) != 0, m[3] = (w & 0xff000000u) != 0;
  }
  RL_MEMBER void colours4(int64_t p, float (&t)[4][3]) const {
    const float4* tp = reinterpret_cast<const float4*>(rgb + 3 * p);
    const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
    t[0][0] = t0.x, t[0][1] = t0.y, t[0][2] = t0.z, t[1][0] = t0.w, t[1][1] = t1.x, t[1][2] = t1.y;
    t[2][0] = t1.z, t[2][1] = t1.w, t[2][2] = t2.x, t[3][0] = t2.y, t[3][1] = t2.z, t[3][2] = t2.w;
  }
  bool ok() const { return rgb && mask && a3d_aligned(4, rgb); }
  bool wide() const { return a3d_aligned(16, rgb) && a3d_aligned(4, mask); }
};

struct GtRgba8 {
  const uint8_t* rgba;  // [S, P, 4]: r, g, b, a
  RL_MEMBER GtRgba8 frame(int64_t s, int64_t P) const { return GtRgba8{rgba + s * P * 4}; }
  static RL_MEMBER void unpack(uint32_t w, float (&t)[3]) {
    t[0] = (float)(w & 0xffu) / 255.0f, t[1] = (float)((w >> 8) & 0xffu) / 255.0f, t[2] = (float)((w >> 16) & 0xffu) / 255.0f;
  }
  RL_MEMBER bool inside(int64_t p) const { return (*reinterpret_cast<const uint32_t*>(rgba + 4 * p) >> 24) >= 128u; }
  RL_MEMBER void colours(int64_t p, float (&t)[3]) const { unpack(*reinterpret_cast<const uint32_t*>(rgba + 4 * p), t); }
  RL_MEMBER void inside4(int64_t p, bool (&m)[4]) const {
    const uint4 w = *reinterpret_cast<const uint4*>(rgba + 4 * p);
    m[0] = (w.x >> 24) >= 128u, m[1] = (w.y >> 24) >= 128u, m[2] = (w.z >> 24) >= 128u, m[3] = (w.w >> 24) >= 128u;
  }
  RL_MEMBER void colours4(int64_t p, float (&t)[4][3]) const {
    const uint4 w = *reinterpret_cast<const uint4*>(rgba + 4 * p);
    unpack(w.x, t[0]), unpack(w.y, t[1]), unpack(w.z, t[2]), unpack(w.w, t[3]);
  }
  bool ok() const { return rgba && a3d_aligned(4, rgba); }
  bool wide() const { return a3d_aligned(16, rgba); }
};

template <typename GT>
struct ReconArgs {
  int64_t P;            // H W
  int64_t chunks;       // blocks per image
  const float* image;   // [B, 3, P]
  const float* alpha;   // [B, P]
  GT gt;                // S frames of P pixels
  const int* index;     // [B] or NULL
  float bg;
};

A3D_DEV float rl_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// acc + d d.  Whether the product is fused into the sum is written down here and not left to the compiler's contraction, which differs
// from one instantiation of a kernel to the next: the two readers of the ground truth are held to equal bits, and so is a3d_recon_loss_f32
// from one build to the next.  rl_add_sq: one fma.  rl_add_sq_rounded: the product rounded to fp32, then the sum.
A3D_DEV float rl_add_sq(float acc, float d) { return __builtin_fmaf(d, d, acc); }
A3D_DEV float rl_add_sq_rounded(float acc, float d) {
#pragma clang fp contract(off)
  const float sq = d * d;
  return acc + sq;
}

// squared errors of one pixel: colours r, g, b and alpha a against ground truth t (composited over bg where the mask is off).  rounded01:
// the first two colour terms go through rl_add_sq_rounded (see RL_ROUNDED_GROUP)
A3D_DEV void rl_pixel(float r, float g, float b, float a, float t0, float t1, float t2, bool m, float bg, float& acc_rgb, float& acc_mask,
                      bool rounded01 = false) {
  const float d0 = rl_clamp01(r) - (m ? t0 : bg), d1 = rl_clamp01(g) - (m ? t1 : bg), d2 = rl_clamp01(b) - (m ? t2 : bg);
  const float dm = a - (m ? 1.f : 0.f);
  acc_rgb = rounded01 ? rl_add_sq_rounded(acc_rgb, d0) : rl_add_sq(acc_rgb, d0);
  acc_rgb = rounded01 ? rl_add_sq_rounded(acc_rgb, d1) : rl_add_sq(acc_rgb, d1);
  acc_rgb = rl_add_sq(acc_rgb, d2);
  acc_mask = rl_add_sq(acc_mask, dm);
}

// Every term of both kernels is one fma, with one exception that is history: before the arithmetic was written down, the compiler fused
// all of the 16-byte path's terms but the first two colour terms of the third pixel of a thread's second group (it squared them as a
// packed pair).  That choice is kept, so that a3d_recon_loss_f32 returns the bits it returned before; the 4-byte path was all fma.
constexpr int RL_ROUNDED_GROUP = 1;

// d_image of one value: torch's clamp rule (bounds inclusive), exactly 0 outside
A3D_DEV float rl_dimage(float v, float t, float coef) { return (v >= 0.f && v <= 1.f) ? coef * (v - t) : 0.f; }

struct ReconBlock {
  int64_t b, p0, s;     // image, first pixel of the block, ground-truth frame
};

template <typename GT>
A3D_DEV ReconBlock rl_block(const ReconArgs<GT>& a) {
  ReconBlock k;
  k.b = (int64_t)blockIdx.x / a.chunks;
  k.p0 = ((int64_t)blockIdx.x % a.chunks) * RL_PIXELS;
  k.s = a.index ? (int64_t)a.index[k.b] : k.b;
  return k;
}

template <typename GT, bool VEC>
__global__ __launch_bounds__(LR_BLOCK) void recon_fwd_kernel(ReconArgs<GT> a, float* __restrict__ partials, int64_t n_partials) {
  __shared__ float red[2][LR_BLOCK];
  const ReconBlock k = rl_block(a);
  const float* img = a.image + k.b * 3 * a.P;
  const float* alp = a.alpha + k.b * a.P;
  const GT gt = a.gt.frame(k.s, a.P);
  float acc_rgb = 0.f, acc_mask = 0.f;
  if (VEC) {
#pragma unroll
    for (int i = 0; i < RL_RUN / 4; ++i) {
      const int64_t p = k.p0 + 4 * ((int64_t)i * LR_BLOCK + threadIdx.x);
      if (p < a.P) {                                 // P % 4 == 0: the whole group is inside
        const float4 r = *reinterpret_cast<const float4*>(img + p), g = *reinterpret_cast<const float4*>(img + a.P + p),
                     bl = *reinterpret_cast<const float4*>(img + 2 * a.P + p), al = *reinterpret_cast<const float4*>(alp + p);
        float t[4][3];
        bool m[4];
        gt.colours4(p, t);
        gt.inside4(p, m);
        rl_pixel(r.x, g.x, bl.x, al.x, t[0][0], t[0][1], t[0][2], m[0], a.bg, acc_rgb, acc_mask);
        rl_pixel(r.y, g.y, bl.y, al.y, t[1][0], t[1][1], t[1][2], m[1], a.bg, acc_rgb, acc_mask);
        rl_pixel(r.z, g.z, bl.z, al.z, t[2][0], t[2][1], t[2][2], m[2], a.bg, acc_rgb, acc_mask, i == RL_ROUNDED_GROUP);
        rl_pixel(r.w, g.w, bl.w, al.w, t[3][0], t[3][1], t[3][2], m[3], a.bg, acc_rgb, acc_mask);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < RL_RUN; ++i) {
      const int64_t p = k.p0 + (int64_t)i * LR_BLOCK + threadIdx.x;
      if (p < a.P) {
        float t[3];
        gt.colours(p, t);
        rl_pixel(img[p], img[a.P + p], img[2 * a.P + p], alp[p], t[0], t[1], t[2], gt.inside(p), a.bg, acc_rgb, acc_mask);
      }
    }
  }
  lr_block_partials<2>({acc_rgb, acc_mask}, red, partials, n_partials);
}

__global__ __launch_bounds__(LR_BLOCK) void recon_final_kernel(const float* __restrict__ partials, int64_t n_partials, double n_rgb, double n_mask,
                                                               double lambda_rgb, double lambda_mask, float* __restrict__ out) {
  __shared__ double red[2][LR_BLOCK];
  lr_final_sums<2>(partials, n_partials, red);
  if (threadIdx.x == 0) {
    const double m_rgb = red[0][0] / n_rgb, m_mask = red[1][0] / n_mask;
    out[0] = (float)(lambda_rgb * m_rgb + lambda_mask * m_mask);
    out[1] = (float)m_rgb;
    out[2] = (float)m_mask;
  }
}

template <typename GT, bool VEC>
__global__ __launch_bounds__(LR_BLOCK) void recon_bwd_kernel(ReconArgs<GT> a, float coef_rgb, float coef_mask, const float* __restrict__ grad_out,
                                                             float* __restrict__ d_image, float* __restrict__ d_alpha) {
  const ReconBlock k = rl_block(a);
  const float g = grad_out[0];
  const float cr = g * coef_rgb, cm = g * coef_mask;
  const float* img = a.image + k.b * 3 * a.P;
  const float* alp = a.alpha + k.b * a.P;
  const GT gt = a.gt.frame(k.s, a.P);
  float* di = d_image ? d_image + k.b * 3 * a.P : nullptr;
  float* da = d_alpha ? d_alpha + k.b * a.P : nullptr;
  if (VEC) {
#pragma unroll
    for (int i = 0; i < RL_RUN / 4; ++i) {
      const int64_t p = k.p0 + 4 * ((int64_t)i * LR_BLOCK + threadIdx.x);
      if (p < a.P) {
        bool m[4];
        gt.inside4(p, m);
        const bool m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
        if (di) {
          const float4 r = *reinterpret_cast<const float4*>(img + p), gr = *reinterpret_cast<const float4*>(img + a.P + p),
                       bl = *reinterpret_cast<const float4*>(img + 2 * a.P + p);
          float t[4][3];
          gt.colours4(p, t);
          const float bg = a.bg;
          *reinterpret_cast<float4*>(di + p) = make_float4(rl_dimage(r.x, m0 ? t[0][0] : bg, cr), rl_dimage(r.y, m1 ? t[1][0] : bg, cr),
                                                           rl_dimage(r.z, m2 ? t[2][0] : bg, cr), rl_dimage(r.w, m3 ? t[3][0] : bg, cr));
          *reinterpret_cast<float4*>(di + a.P + p) = make_float4(rl_dimage(gr.x, m0 ? t[0][1] : bg, cr), rl_dimage(gr.y, m1 ? t[1][1] : bg, cr),
                                                                 rl_dimage(gr.z, m2 ? t[2][1] : bg, cr), rl_dimage(gr.w, m3 ? t[3][1] : bg, cr));
          *reinterpret_cast<float4*>(di + 2 * a.P + p) = make_float4(rl_dimage(bl.x, m0 ? t[0][2] : bg, cr), rl_dimage(bl.y, m1 ? t[1][2] : bg, cr),
                                                                     rl_dimage(bl.z, m2 ? t[2][2] : bg, cr), rl_dimage(bl.w, m3 ? t[3][2] : bg, cr));
        }
        if (da) {
          const float4 al = *reinterpret_cast<const float4*>(alp + p);
          *reinterpret_cast<float4*>(da + p) = make_float4(cm * (al.x - (m0 ? 1.f : 0.f)), cm * (al.y - (m1 ? 1.f : 0.f)),
                                                           cm * (al.z - (m2 ? 1.f : 0.f)), cm * (al.w - (m3 ? 1.f : 0.f)));
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < RL_RUN; ++i) {
      const int64_t p = k.p0 + (int64_t)i * LR_BLOCK + threadIdx.x;
      if (p < a.P) {
        const bool m = gt.inside(p);
        if (di) {
          float t[3];
          gt.colours(p, t);
          di[p] = rl_dimage(img[p], m ? t[0] : a.bg, cr);
          di[a.P + p] = rl_dimage(img[a.P + p], m ? t[1] : a.bg, cr);
          di[2 * a.P + p] = rl_dimage(img[2 * a.P + p], m ? t[2] : a.bg, cr);
        }
        if (da) da[p] = cm * (alp[p] - (m ? 1.f : 0.f));
      }
    }
  }
}

// the shared argument check: everything a launch depends on, before the first HIP call.  Returns the number of blocks, 0 for a refusal
template <typename GT>
int64_t recon_args(ReconArgs<GT>& a, int B, int H, int W, const float* image, const float* alpha, GT gt, const int* index, float bg) {
  if (B <= 0 || H <= 0 || W <= 0 || !image || !alpha || !gt.ok()) return 0;
  if (!a3d_aligned(4, image, alpha) || !a3d_aligned(4, index)) return 0;
  const int64_t P = (int64_t)H * W;
  if (P > (((int64_t)1 << 40) - 1) / B) return 0;                                           // B H W >= 2^40
  const int64_t chunks = (P + RL_PIXELS - 1) / RL_PIXELS;
  if (chunks > (int64_t)0x7fffffff / B) return 0;                                           // the grid's x extent
  a = ReconArgs<GT>{P, chunks, image, alpha, gt, index, bg};
  return chunks * B;
}

template <typename GT>
bool recon_vec(const ReconArgs<GT>& a, const float* d_image, const float* d_alpha) {
  return a.P % 4 == 0 && a3d_aligned(16, a.image, a.alpha, d_image, d_alpha) && a.gt.wide();
}

template <typename GT>
int recon_forward(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, GT gt, const int* index, float bg,
                  double lambda_rgb, double lambda_mask, float* partials, int64_t n_partials, float* out) {
  ReconArgs<GT> a;
  const int64_t blocks = recon_args(a, B, H, W, image, alpha, gt, index, bg);
  if (blocks == 0 || !partials || !out || !a3d_aligned(4, partials, out) || n_partials != blocks) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (recon_vec(a, nullptr, nullptr)) recon_fwd_kernel<GT, true><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, partials, n_partials);
  else recon_fwd_kernel<GT, false><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, partials, n_partials);
  recon_final_kernel<<<1, LR_BLOCK, 0, st>>>(partials, n_partials, 3.0 * (double)B * (double)a.P, (double)B * (double)a.P, lambda_rgb,
                                             lambda_mask, out);
  return a3d_launch_status();
}

template <typename GT>
int recon_backward(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, GT gt, const int* index, float bg,
                   float coef_rgb, float coef_mask, const float* grad_out, float* d_image, float* d_alpha) {
  ReconArgs<GT> a;
  const int64_t blocks = recon_args(a, B, H, W, image, alpha, gt, index, bg);
  if (blocks == 0 || !grad_out || (!d_image && !d_alpha) || !a3d_aligned(4, grad_out, d_image, d_alpha)) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (recon_vec(a, d_image, d_alpha))
    recon_bwd_kernel<GT, true><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, coef_rgb, coef_mask, grad_out, d_image, d_alpha);
  else recon_bwd_kernel<GT, false><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, coef_rgb, coef_mask, grad_out, d_image, d_alpha);
  return a3d_launch_status();
}

}  // namespace

extern "C" int a3d_recon_loss_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const float* gt_rgb,
                                  const uint8_t* gt_mask, const int* index, float bg, double lambda_rgb, double lambda_mask,
                                  float* partials, int64_t n_partials, float* out) {
  return recon_forward(stream, B, H, W, image, alpha, GtF32{gt_rgb, gt_mask}, index, bg, lambda_rgb, lambda_mask, partials, n_partials, out);
}

extern "C" int a3d_recon_loss_bwd_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const float* gt_rgb,
                                      const uint8_t* gt_mask, const int* index, float bg, float coef_rgb, float coef_mask,
                                      const float* grad_out, float* d_image, float* d_alpha) {
  return recon_backward(stream, B, H, W, image, alpha, GtF32{gt_rgb, gt_mask}, index, bg, coef_rgb, coef_mask, grad_out, d_image, d_alpha);
}

extern "C" int a3d_recon_loss_rgba8_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha,
                                        const uint8_t* gt_rgba8, const int* index, float bg, double lambda_rgb, double lambda_mask,
                                        float* partials, int64_t n_partials, float* out) {
  return recon_forward(stream, B, H, W, image, alpha, GtRgba8{gt_rgba8}, index, bg, lambda_rgb, lambda_mask, partials, n_partials, out);
}

extern "C" int a3d_recon_loss_rgba8_bwd_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha,
                                            const uint8_t* gt_rgba8, const int* index, float bg, float coef_rgb, float coef_mask,
                                            const float* grad_out, float* d_image, float* d_alpha) {
  return recon_backward(stream, B, H, W, image, alpha, GtRgba8{gt_rgba8}, index, bg, coef_rgb, coef_mask, grad_out, d_image, d_alpha);
}
