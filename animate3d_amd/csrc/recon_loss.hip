// Reconstruction loss of the 4-D stage on gfx950: the masked RGB / mask MSE of a batch of renders against the tracked frames; contract in
// animate3d_amd/stage4d.py (masked_recon_loss).  Replaces the torch chain of custom/threestudio-animate3d/systems/animate3d.py:160-184 (the
// val[sampled_idx] copies of the ground truth, the compositing with the mask, two F.mse_loss) and the clamp / permute in front of it
// (diff_gaussian_rasterizer_advanced_4d.py:180, gaussian_batch_renderer_4d.py:73).
//
//   recon_fwd_kernel<VEC>   block j of image b covers pixels [j RL_PIXELS, (j + 1) RL_PIXELS) of that image; a thread accumulates RL_RUN
//                           pixels in fp32 (VEC: as RL_RUN / 4 groups of four neighbours, read 16 bytes at a time from the three colour
//                           planes, the alpha plane and the interleaved ground truth, four mask bytes at once), then the block writes
//                           one (rgb, mask) partial.  VEC needs H W % 4 == 0 and 16-byte bases: then every group starts on 16 bytes in
//                           every operand.
//   recon_final_kernel      one block adds the partials; the order of both steps is loss_reduce.h's (no atomics, two calls are bitwise
//                           equal).  out = {lambda_rgb mean_rgb + lambda_mask mean_mask, mean_rgb, mean_mask}
//   recon_bwd_kernel<VEC>   recomputes from the four inputs in the same geometry and writes d_image / d_alpha in the planar layout
//                           a3d_gs_render_bwd_f32 reads; the upstream gradient is read through a device pointer
#include "loss_reduce.h"

#ifndef A3D_STORAGE_F16

namespace {

constexpr int RL_RUN = 8;                          // pixels per thread
constexpr int RL_PIXELS = LR_BLOCK * RL_RUN;       // pixels per block: a3d_recon_loss_f32's partials are B * ceil(H W / RL_PIXELS) pairs
static_assert(RL_RUN % 4 == 0 && RL_RUN <= 64, "a thread's run is a bounded number of 4-pixel groups");

struct ReconArgs {
  int64_t P;            // H W
  int64_t chunks;       // blocks per image
  const float* image;   // [B, 3, P]
  const float* alpha;   // [B, P]
  const float* gt;      // [S, P, 3]
  const uint8_t* mask;  // [S, P]
  const int* index;     // [B] or NULL
  float bg;
};

A3D_DEV float rl_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// squared errors of one pixel: colours r, g, b and alpha a against ground truth t (composited over bg where the mask is off)
A3D_DEV void rl_pixel(float r, float g, float b, float a, float t0, float t1, float t2, bool m, float bg, float& acc_rgb, float& acc_mask) {
  const float d0 = rl_clamp01(r) - (m ? t0 : bg), d1 = rl_clamp01(g) - (m ? t1 : bg), d2 = rl_clamp01(b) - (m ? t2 : bg);
  const float dm = a - (m ? 1.f : 0.f);
  acc_rgb += d0 * d0;
  acc_rgb += d1 * d1;
  acc_rgb += d2 * d2;
  acc_mask += dm * dm;
}

// d_image of one value: torch's clamp rule (bounds inclusive), exactly 0 outside
A3D_DEV float rl_dimage(float v, float t, float coef) { return (v >= 0.f && v <= 1.f) ? coef * (v - t) : 0.f; }

struct ReconBlock {
  int64_t b, p0, s;     // image, first pixel of the block, ground-truth frame
};

A3D_DEV ReconBlock rl_block(const ReconArgs& a) {
  ReconBlock k;
  k.b = (int64_t)blockIdx.x / a.chunks;
  k.p0 = ((int64_t)blockIdx.x % a.chunks) * RL_PIXELS;
  k.s = a.index ? (int64_t)a.index[k.b] : k.b;
  return k;
}

template <bool VEC>
__global__ __launch_bounds__(LR_BLOCK) void recon_fwd_kernel(ReconArgs a, float* __restrict__ partials, int64_t n_partials) {
  __shared__ float red[2][LR_BLOCK];
  const ReconBlock k = rl_block(a);
  const float* img = a.image + k.b * 3 * a.P;
  const float* alp = a.alpha + k.b * a.P;
  const float* gt = a.gt + k.s * a.P * 3;
  const uint8_t* msk = a.mask + k.s * a.P;
  float acc_rgb = 0.f, acc_mask = 0.f;
  if (VEC) {
#pragma unroll
    for (int i = 0; i < RL_RUN / 4; ++i) {
      const int64_t p = k.p0 + 4 * ((int64_t)i * LR_BLOCK + threadIdx.x);
      if (p < a.P) {                                 // P % 4 == 0: the whole group is inside
        const float4 r = *reinterpret_cast<const float4*>(img + p), g = *reinterpret_cast<const float4*>(img + a.P + p),
                     bl = *reinterpret_cast<const float4*>(img + 2 * a.P + p), al = *reinterpret_cast<const float4*>(alp + p);
        const float4* tp = reinterpret_cast<const float4*>(gt + 3 * p);
        const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
        const uint32_t m = *reinterpret_cast<const uint32_t*>(msk + p);
        rl_pixel(r.x, g.x, bl.x, al.x, t0.x, t0.y, t0.z, (m & 0xffu) != 0, a.bg, acc_rgb, acc_mask);
        rl_pixel(r.y, g.y, bl.y, al.y, t0.w, t1.x, t1.y, (m & 0xff00u) != 0, a.bg, acc_rgb, acc_mask);
        rl_pixel(r.z, g.z, bl.z, al.z, t1.z, t1.w, t2.x, (m & 0xff0000u) != 0, a.bg, acc_rgb, acc_mask);
        rl_pixel(r.w, g.w, bl.w, al.w, t2.y, t2.z, t2.w, (m & 0xff000000u) != 0, a.bg, acc_rgb, acc_mask);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < RL_RUN; ++i) {
      const int64_t p = k.p0 + (int64_t)i * LR_BLOCK + threadIdx.x;
      if (p < a.P)
        rl_pixel(img[p], img[a.P + p], img[2 * a.P + p], alp[p], gt[3 * p], gt[3 * p + 1], gt[3 * p + 2], msk[p] != 0, a.bg, acc_rgb, acc_mask);
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

template <bool VEC>
__global__ __launch_bounds__(LR_BLOCK) void recon_bwd_kernel(ReconArgs a, float coef_rgb, float coef_mask, const float* __restrict__ grad_out,
                                                             float* __restrict__ d_image, float* __restrict__ d_alpha) {
  const ReconBlock k = rl_block(a);
  const float g = grad_out[0];
  const float cr = g * coef_rgb, cm = g * coef_mask;
  const float* img = a.image + k.b * 3 * a.P;
  const float* alp = a.alpha + k.b * a.P;
  const float* gt = a.gt + k.s * a.P * 3;
  const uint8_t* msk = a.mask + k.s * a.P;
  float* di = d_image ? d_image + k.b * 3 * a.P : nullptr;
  float* da = d_alpha ? d_alpha + k.b * a.P : nullptr;
  if (VEC) {
#pragma unroll
    for (int i = 0; i < RL_RUN / 4; ++i) {
      const int64_t p = k.p0 + 4 * ((int64_t)i * LR_BLOCK + threadIdx.x);
      if (p < a.P) {
        const uint32_t m = *reinterpret_cast<const uint32_t*>(msk + p);
        const bool m0 = (m & 0xffu) != 0, m1 = (m & 0xff00u) != 0, m2 = (m & 0xff0000u) != 0, m3 = (m & 0xff000000u) != 0;
        if (di) {
          const float4 r = *reinterpret_cast<const float4*>(img + p), gr = *reinterpret_cast<const float4*>(img + a.P + p),
                       bl = *reinterpret_cast<const float4*>(img + 2 * a.P + p);
          const float4* tp = reinterpret_cast<const float4*>(gt + 3 * p);
          const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
          const float bg = a.bg;
          *reinterpret_cast<float4*>(di + p) = make_float4(rl_dimage(r.x, m0 ? t0.x : bg, cr), rl_dimage(r.y, m1 ? t0.w : bg, cr),
                                                           rl_dimage(r.z, m2 ? t1.z : bg, cr), rl_dimage(r.w, m3 ? t2.y : bg, cr));
          *reinterpret_cast<float4*>(di + a.P + p) = make_float4(rl_dimage(gr.x, m0 ? t0.y : bg, cr), rl_dimage(gr.y, m1 ? t1.x : bg, cr),
                                                                 rl_dimage(gr.z, m2 ? t1.w : bg, cr), rl_dimage(gr.w, m3 ? t2.z : bg, cr));
          *reinterpret_cast<float4*>(di + 2 * a.P + p) = make_float4(rl_dimage(bl.x, m0 ? t0.z : bg, cr), rl_dimage(bl.y, m1 ? t1.y : bg, cr),
                                                                     rl_dimage(bl.z, m2 ? t2.x : bg, cr), rl_dimage(bl.w, m3 ? t2.w : bg, cr));
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
        const bool m = msk[p] != 0;
        if (di) {
          di[p] = rl_dimage(img[p], m ? gt[3 * p] : a.bg, cr);
          di[a.P + p] = rl_dimage(img[a.P + p], m ? gt[3 * p + 1] : a.bg, cr);
          di[2 * a.P + p] = rl_dimage(img[2 * a.P + p], m ? gt[3 * p + 2] : a.bg, cr);
        }
        if (da) da[p] = cm * (alp[p] - (m ? 1.f : 0.f));
      }
    }
  }
}

// the shared argument check: everything a launch depends on, before the first HIP call.  Returns the number of blocks, 0 for a refusal
int64_t recon_args(ReconArgs& a, int B, int H, int W, const float* image, const float* alpha, const float* gt_rgb, const uint8_t* gt_mask,
                   const int* index, float bg) {
  if (B <= 0 || H <= 0 || W <= 0 || !image || !alpha || !gt_rgb || !gt_mask) return 0;
  if (!a3d_aligned(4, image, alpha, gt_rgb) || !a3d_aligned(4, index)) return 0;
  const int64_t P = (int64_t)H * W;
  if (P > (((int64_t)1 << 40) - 1) / B) return 0;                                           // B H W >= 2^40
  const int64_t chunks = (P + RL_PIXELS - 1) / RL_PIXELS;
  if (chunks > (int64_t)0x7fffffff / B) return 0;                                           // the grid's x extent
  a = ReconArgs{P, chunks, image, alpha, gt_rgb, gt_mask, index, bg};
  return chunks * B;
}

bool recon_vec(const ReconArgs& a, const float* d_image, const float* d_alpha) {
  return a.P % 4 == 0 && a3d_aligned(16, a.image, a.alpha, a.gt, d_image, d_alpha) && a3d_aligned(4, a.mask);
}

}  // namespace

extern "C" int a3d_recon_loss_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const float* gt_rgb,
                                  const uint8_t* gt_mask, const int* index, float bg, double lambda_rgb, double lambda_mask,
                                  float* partials, int64_t n_partials, float* out) {
  ReconArgs a;
  const int64_t blocks = recon_args(a, B, H, W, image, alpha, gt_rgb, gt_mask, index, bg);
  if (blocks == 0 || !partials || !out || !a3d_aligned(4, partials, out) || n_partials != blocks) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (recon_vec(a, nullptr, nullptr)) recon_fwd_kernel<true><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, partials, n_partials);
  else recon_fwd_kernel<false><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, partials, n_partials);
  recon_final_kernel<<<1, LR_BLOCK, 0, st>>>(partials, n_partials, 3.0 * (double)B * (double)a.P, (double)B * (double)a.P, lambda_rgb,
                                             lambda_mask, out);
  return a3d_launch_status();
}

extern "C" int a3d_recon_loss_bwd_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const float* gt_rgb,
                                      const uint8_t* gt_mask, const int* index, float bg, float coef_rgb, float coef_mask,
                                      const float* grad_out, float* d_image, float* d_alpha) {
  ReconArgs a;
  const int64_t blocks = recon_args(a, B, H, W, image, alpha, gt_rgb, gt_mask, index, bg);
  if (blocks == 0 || !grad_out || (!d_image && !d_alpha) || !a3d_aligned(4, grad_out, d_image, d_alpha)) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (recon_vec(a, d_image, d_alpha)) recon_bwd_kernel<true><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, coef_rgb, coef_mask, grad_out, d_image, d_alpha);
  else recon_bwd_kernel<false><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, coef_rgb, coef_mask, grad_out, d_image, d_alpha);
  return a3d_launch_status();
}

#endif  // A3D_STORAGE_F16
