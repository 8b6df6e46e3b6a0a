// The SDS-side glue of the 4D-SDS step on gfx950: everything of the guidance's reconstruction loss but the UNet call;
// contract in animate3d_amd/sds.py (sds_recon_loss_fused).  Replaces the torch chain of
// custom/threestudio-animate3d/guidance/animatemv_guidance.py:415-503 (add_noise, the CFG-doubled "(b n) c f h w" batch, the CFG combine,
// both x0 reconstructions, the std rescale, the pinned first frame, the loss) and its autograd backward.  The tensors are fp32 arithmetic, the statistics and the scalar fp64; the UNet boundary is
// this build's 16-bit storage type, or fp32 for a UNet that runs in fp32.
//
// Sizes: b videos-of-views, n views, f frames, c channels, P = h w.  latents / latents_noisy / latents_recon / noise_pred / grad are
// [(b n f), c, P] fp32; noise [b, n, f - 1, c, P] fp32; sample and eps [2 b n, c, f, P] at the boundary ((text, uncond) halves).  Per b:
// a = table[t[b]] (t clamped into the table), sa = sqrt(a), s1 = sqrt(1 - a), in fp32 as torch computes them.
//
//   sds_pack_kernel      one thread per latent: noisy = frame 0 ? x : sa x + s1 noise; written to latents_noisy and to both halves of
//                        sample; the first b n threads also write timestep [2 b n] = t[b]
//   sds_stats_kernel     (recon_std_rescale != 0)  block j of b covers SG_ITEMS of b's n (f - 1) c P diffused elements; the thread keeps
//                        x0_text and x0_cfg of its SG_RUN elements in registers, formed in fp64 from latents, noise and eps.  Two passes
//                        inside the block, fp64 accumulators through loss_reduce.h's tree: the block's means, then the squared
//                        deviations from them.  stats [b, chunks, 4] fp64 = (mean_text, M2_text, mean_cfg, M2_cfg); a block's count
//                        follows from the geometry
//   sds_recon_kernel     block j of b covers SG_ITEMS of b's n f c P elements.  Thread 0 first merges b's stats in chunk order (Chan's
//                        pairwise update in fp64: nothing is ever a difference of two large sums), std = sqrt(M2 / (count - 1)),
//                        factor = (std_text + 1e-8) / (std_cfg + 1e-8).  Then per element, in fp32 with the factor rounded once: eps_cfg,
//                        x0, the blend r (x0 factor) + (1 - r) x0, frame 0 pinned to the latents' bits: the tensors, bit for bit what
//                        the torch ops give.  The loss does not inherit their rounding: its difference latents - recon is formed a
//                        second time in fp64 from latents, noise and eps, squared and added in fp64; the block's sum goes through the
//                        fixed tree in fp64 and is stored as an fp32 pair (hi, lo): partials [2, blocks]
//   sds_final_kernel     one block adds the partials in fp64 (loss_reduce.h): out[0] = 0.5 (hi + lo) / (b n f) * f / (f - 1), rounded
//                        once.  An fp32 scalar cannot be nearer to the float64 value of the formulas
//   sds_bwd_kernel       grad = frame 0 ? 0 : (latents - recon) (coef g), g = grad_out[0] read on the device
// No atomics; the chunking is per b, so b's rows do not depend on the other videos of the batch, and two calls are bitwise equal.
// Products and sums of the element-wise chain are not contracted: they round where torch's separate ops round.
#include "loss_reduce.h"

namespace {

constexpr int SG_RUN = 8;                          // elements per thread
constexpr int SG_ITEMS = LR_BLOCK * SG_RUN;        // elements per block of the stats and recon kernels

struct SdsDims {
  int64_t n, f, c, P;
  int64_t rest;          // n (f - 1) c P: the diffused elements of one b
  int64_t all;           // n f c P
  int64_t chunks_rest, chunks_all;
  int64_t half;          // b n c f P: one CFG half of sample / eps
};

template <bool F32>
A3D_DEV float sg_load(const void* ptr, int64_t i) {
  if constexpr (F32) return static_cast<const float*>(ptr)[i];
  else return h2f(static_cast<const uint16_t*>(ptr)[i]);
}
template <bool F32>
A3D_DEV void sg_store(void* ptr, int64_t i, float v) {
  if constexpr (F32) static_cast<float*>(ptr)[i] = v;
  else static_cast<uint16_t*>(ptr)[i] = f2h(v);
}

// alphas_cumprod[t[b]] -> (sqrt(a), sqrt(1 - a)); t is clamped: a timestep outside the table reads its nearest end, never past it
A3D_DEV void sg_alpha(const int64_t* t, const float* table, int table_len, int64_t b, float& sa, float& s1) {
  int64_t ti = t[b];
  ti = ti < 0 ? 0 : (ti >= table_len ? table_len - 1 : ti);
  const float a = table[ti];
  sa = sqrtf(a);
  s1 = sqrtf(1.f - a);
}

A3D_DEV float sg_noisy(float x, float noise, float sa, float s1) {
#pragma clang fp contract(off)
  const float p0 = sa * x, p1 = s1 * noise;
  return p0 + p1;
}
A3D_DEV float sg_cfg(float et, float eu, float scale) {
#pragma clang fp contract(off)
  const float d = et - eu;
  const float sd = scale * d;
  return et + sd;
}
A3D_DEV float sg_x0(float noisy, float e, float sa, float s1) {
#pragma clang fp contract(off)
  const float se = s1 * e;
  return (noisy - se) / sa;
}
A3D_DEV float sg_blend(float x0, float factor, float r, float one_minus_r) {
#pragma clang fp contract(off)
  const float adj = x0 * factor;
  const float p0 = r * adj, p1 = one_minus_r * x0;
  return p0 + p1;
}

// element e of b's n f c P latents, latents order ((view, frame), c, p) -> its place in one CFG half of the "(b n) c f P" boundary tensor
A3D_DEV int64_t sg_boundary_index(const SdsDims& d, int64_t b, int64_t e, int64_t& frame) {
  const int64_t p = e % d.P, r = e / d.P;
  const int64_t ch = r % d.c, vf = r / d.c;
  frame = vf % d.f;
  const int64_t view = vf / d.f;
  return (((b * d.n + view) * d.c + ch) * d.f + frame) * d.P + p;
}

template <bool F32>
__global__ __launch_bounds__(LR_BLOCK) void sds_pack_kernel(SdsDims d, int64_t b_count, const float* __restrict__ latents,
                                                            const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                            const float* __restrict__ table, int table_len, float* __restrict__ latents_noisy,
                                                            void* __restrict__ sample, void* __restrict__ timestep) {
  const int64_t i = (int64_t)blockIdx.x * LR_BLOCK + threadIdx.x;
  if (i < b_count * d.n) {
    int64_t ti = t[i / d.n];
    ti = ti < 0 ? 0 : (ti >= table_len ? table_len - 1 : ti);
    sg_store<F32>(timestep, i, (float)ti);
    sg_store<F32>(timestep, b_count * d.n + i, (float)ti);
  }
  if (i >= b_count * d.all) return;
  const int64_t b = i / d.all, e = i % d.all;
  int64_t frame;
  const int64_t o = sg_boundary_index(d, b, e, frame);
  float y = latents[i];
  if (frame != 0) {
    float sa, s1;
    sg_alpha(t, table, table_len, b, sa, s1);
    const int64_t p = e % d.P, r = e / d.P, ch = r % d.c, view = r / d.c / d.f;
    y = sg_noisy(y, noise[(((b * d.n + view) * (d.f - 1) + frame - 1) * d.c + ch) * d.P + p], sa, s1);
  }
  latents_noisy[i] = y;
  sg_store<F32>(sample, o, y);
  sg_store<F32>(sample, d.half + o, y);
}

// The fp64 twin of the chain, from the same inputs (a = (double)table[t[b]]): what the statistics and the loss are formed from, so that
// the factor and the scalar carry the rounding of their own result and nothing of the fp32 tensors'
struct SdsAlpha64 {
  double sa, s1;
};
A3D_DEV SdsAlpha64 sg_alpha64(const int64_t* t, const float* table, int table_len, int64_t b) {
  int64_t ti = t[b];
  ti = ti < 0 ? 0 : (ti >= table_len ? table_len - 1 : ti);
  const double a = (double)table[ti];
  return SdsAlpha64{sqrt(a), sqrt(1.0 - a)};
}
A3D_DEV double sg_x0_64(double x, double noise, double e, const SdsAlpha64& al) { return ((al.sa * x + al.s1 * noise) - al.s1 * e) / al.sa; }

// element q of b's n (f - 1) c P diffused elements, in the boundary's order ((view, c), frame - 1, p): eps is read in runs of (f - 1) P
template <bool F32>
__global__ __launch_bounds__(LR_BLOCK) void sds_stats_kernel(SdsDims d, const void* __restrict__ eps, const float* __restrict__ latents,
                                                             const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                             const float* __restrict__ table, int table_len, double scale,
                                                             double* __restrict__ stats) {
  __shared__ double red[2][LR_BLOCK];
  const int64_t b = (int64_t)blockIdx.x / d.chunks_rest, j = (int64_t)blockIdx.x % d.chunks_rest;
  const int64_t q0 = j * SG_ITEMS;
  const int64_t count = (d.rest - q0 < SG_ITEMS) ? d.rest - q0 : SG_ITEMS;
  const SdsAlpha64 al = sg_alpha64(t, table, table_len, b);
  double xt[SG_RUN], xc[SG_RUN];
  double sum_t = 0.0, sum_c = 0.0;
#pragma unroll
  for (int k = 0; k < SG_RUN; ++k) {
    const int64_t q = q0 + (int64_t)k * LR_BLOCK + threadIdx.x;
    xt[k] = xc[k] = 0.0;
    if (q < d.rest) {
      const int64_t p = q % d.P, r = q / d.P;
      const int64_t frame = 1 + r % (d.f - 1), vc = r / (d.f - 1);
      const int64_t ch = vc % d.c, view = vc / d.c;
      const int64_t o = (((b * d.n + view) * d.c + ch) * d.f + frame) * d.P + p;
      const double et = (double)sg_load<F32>(eps, o), eu = (double)sg_load<F32>(eps, d.half + o);
      const double x = (double)latents[(((b * d.n + view) * d.f + frame) * d.c + ch) * d.P + p];
      const double nz = (double)noise[(((b * d.n + view) * (d.f - 1) + frame - 1) * d.c + ch) * d.P + p];
      xt[k] = sg_x0_64(x, nz, et, al);
      xc[k] = sg_x0_64(x, nz, et + scale * (et - eu), al);
      sum_t += xt[k];
      sum_c += xc[k];
    }
  }
  red[0][threadIdx.x] = sum_t;
  red[1][threadIdx.x] = sum_c;
  lr_tree(red);
  const double mean_t = red[0][0] / (double)count, mean_c = red[1][0] / (double)count;
  __syncthreads();                                   // every thread has read the sums before the columns are written again
  double m2_t = 0.0, m2_c = 0.0;
#pragma unroll
  for (int k = 0; k < SG_RUN; ++k) {
    if (q0 + (int64_t)k * LR_BLOCK + threadIdx.x < d.rest) {
      const double dt = xt[k] - mean_t, dc = xc[k] - mean_c;
      m2_t += dt * dt;
      m2_c += dc * dc;
    }
  }
  red[0][threadIdx.x] = m2_t;
  red[1][threadIdx.x] = m2_c;
  lr_tree(red);
  if (threadIdx.x == 0) {
    double* out = stats + (int64_t)blockIdx.x * 4;
    out[0] = mean_t, out[1] = red[0][0], out[2] = mean_c, out[3] = red[1][0];
  }
}

// (count, mean, M2) of b's diffused elements from its chunks, in chunk order: Chan, Golub and LeVeque's update of two groups
A3D_DEV double sg_merged_std(const double* __restrict__ stats, const SdsDims& d, int which) {
  double count = 0.0, mean = 0.0, m2 = 0.0;
  for (int64_t j = 0; j < d.chunks_rest; ++j) {
    const int64_t left = d.rest - j * SG_ITEMS;
    const double cj = (double)(left < SG_ITEMS ? left : SG_ITEMS), mj = stats[j * 4 + 2 * which], m2j = stats[j * 4 + 2 * which + 1];
    const double total = count + cj, delta = mj - mean;
    mean += delta * (cj / total);
    m2 += m2j + delta * delta * (count * cj / total);
    count = total;
  }
  return sqrt(m2 / (count - 1.0));                   // unbiased, as torch.std; one element: NaN, as torch's
}

template <bool F32>
__global__ __launch_bounds__(LR_BLOCK) void sds_recon_kernel(SdsDims d, const void* __restrict__ eps, const float* __restrict__ latents_noisy,
                                                             const float* __restrict__ latents, const float* __restrict__ noise,
                                                             const int64_t* __restrict__ t, const float* __restrict__ table, int table_len,
                                                             double scale, double rescale, const double* __restrict__ stats,
                                                             float* __restrict__ latents_recon, float* __restrict__ noise_pred,
                                                             float* __restrict__ partials, int64_t n_partials) {
  __shared__ double red[1][LR_BLOCK];
  __shared__ double factor_s;
  const int64_t b = (int64_t)blockIdx.x / d.chunks_all, j = (int64_t)blockIdx.x % d.chunks_all;
  const bool rescaled = rescale != 0.0;
  if (rescaled) {
    if (threadIdx.x == 0) {
      const double* sb = stats + b * d.chunks_rest * 4;
      factor_s = (sg_merged_std(sb, d, 0) + 1e-8) / (sg_merged_std(sb, d, 1) + 1e-8);
    }
    __syncthreads();
  }
  const double factor64 = rescaled ? factor_s : 1.0;
  const float factor = (float)factor64, scale32 = (float)scale, r32 = (float)rescale, omr32 = (float)(1.0 - rescale);
  float sa, s1;
  sg_alpha(t, table, table_len, b, sa, s1);
  const SdsAlpha64 al = sg_alpha64(t, table, table_len, b);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < SG_RUN; ++k) {
    const int64_t e = j * SG_ITEMS + (int64_t)k * LR_BLOCK + threadIdx.x;
    if (e < d.all) {
      const int64_t i = b * d.all + e;
      int64_t frame;
      const int64_t o = sg_boundary_index(d, b, e, frame);
      const float et = sg_load<F32>(eps, o), eu = sg_load<F32>(eps, d.half + o);
      const float ec = sg_cfg(et, eu, scale32);
      if (noise_pred) noise_pred[i] = ec;
      const float x = latents[i];
      float target = x;                              // frame 0: the input's own frame, bit for bit
      if (frame != 0) {
        target = sg_x0(latents_noisy[i], ec, sa, s1);
        if (rescaled) target = sg_blend(target, factor, r32, omr32);
        // the loss's own difference, in fp64 from the inputs
        const int64_t p = e % d.P, r = e / d.P, ch = r % d.c, view = r / d.c / d.f;
        const double nz = (double)noise[(((b * d.n + view) * (d.f - 1) + frame - 1) * d.c + ch) * d.P + p];
        double x0 = sg_x0_64((double)x, nz, (double)et + scale * ((double)et - (double)eu), al);
        if (rescaled) x0 = rescale * (x0 * factor64) + (1.0 - rescale) * x0;
        const double diff = (double)x - x0;
        acc += diff * diff;
      }
      latents_recon[i] = target;
    }
  }
  // the block's sum through the fixed tree in fp64, stored as an fp32 pair (hi, lo): partials [2, n_partials]
  red[0][threadIdx.x] = acc;
  lr_tree(red);
  if (threadIdx.x == 0) {
    const float hi = (float)red[0][0];
    partials[blockIdx.x] = hi;
    partials[n_partials + blockIdx.x] = (float)(red[0][0] - (double)hi);
  }
}

__global__ __launch_bounds__(LR_BLOCK) void sds_final_kernel(const float* __restrict__ partials, int64_t n_partials, double images, double f,
                                                             float* __restrict__ out) {
  __shared__ double red[2][LR_BLOCK];
  lr_final_sums<2>(partials, n_partials, red);
  if (threadIdx.x == 0) out[0] = (float)(0.5 * (red[0][0] + red[1][0]) / images * f / (f - 1.0));
}

__global__ __launch_bounds__(LR_BLOCK) void sds_bwd_kernel(int64_t total, int64_t f, int64_t cP, const float* __restrict__ latents,
                                                           const float* __restrict__ latents_recon, float coef,
                                                           const float* __restrict__ grad_out, float* __restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * LR_BLOCK + threadIdx.x;
  if (i >= total) return;
  const float g = coef * grad_out[0];
  grad[i] = ((i / cP) % f == 0) ? 0.f : (latents[i] - latents_recon[i]) * g;
}

// the shared argument check: sizes, before the first HIP call.  false: a refusal
bool sds_dims(SdsDims& d, int64_t& total, int b, int n, int f, int c, int P) {
  if (b <= 0 || n <= 0 || f < 2 || c <= 0 || P <= 0) return false;
  const int64_t limit = (int64_t)1 << 40;
  int64_t all = n;
  for (int64_t m : {(int64_t)f, (int64_t)c, (int64_t)P}) {
    if (all > limit / m) return false;
    all *= m;
  }
  if (all > limit / b) return false;
  d.n = n, d.f = f, d.c = c, d.P = P;
  d.all = all;
  d.rest = all / f * (f - 1);
  d.chunks_all = (d.all + SG_ITEMS - 1) / SG_ITEMS;
  d.chunks_rest = (d.rest + SG_ITEMS - 1) / SG_ITEMS;
  d.half = all * b;
  total = all * b;
  return (total + LR_BLOCK - 1) / LR_BLOCK <= (int64_t)0x7fffffff;
}

#ifdef A3D_STORAGE_F16
constexpr int SG_STORAGE = A3D_F16;
#else
constexpr int SG_STORAGE = A3D_BF16;
#endif

}  // namespace

extern "C" int A3D_FN(a3d_sds_pack)(a3d_stream_t stream, int b, int n, int f, int c, int P, const float* latents, const float* noise,
                                    const int64_t* t, const float* table, int table_len, int dtype, float* latents_noisy, void* sample,
                                    void* timestep) {
  SdsDims d;
  int64_t total;
  if (!sds_dims(d, total, b, n, f, c, P) || !latents || !noise || !t || !table || table_len < 1 || !latents_noisy || !sample || !timestep)
    return A3D_EINVAL;
  if (dtype != A3D_F32 && dtype != SG_STORAGE) return A3D_EINVAL;
  if (!a3d_aligned(4, latents, noise, table, latents_noisy) || !a3d_aligned(8, t) || !a3d_aligned(dtype == A3D_F32 ? 4 : 2, sample, timestep))
    return A3D_EINVAL;
  const unsigned blocks = (unsigned)((total + LR_BLOCK - 1) / LR_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == A3D_F32)
    sds_pack_kernel<true><<<blocks, LR_BLOCK, 0, st>>>(d, b, latents, noise, t, table, table_len, latents_noisy, sample, timestep);
  else sds_pack_kernel<false><<<blocks, LR_BLOCK, 0, st>>>(d, b, latents, noise, t, table, table_len, latents_noisy, sample, timestep);
  return a3d_launch_status();
}

extern "C" int A3D_FN(a3d_sds_epilogue)(a3d_stream_t stream, int b, int n, int f, int c, int P, const void* eps, int dtype,
                                        const float* latents_noisy, const float* latents, const float* noise, const int64_t* t,
                                        const float* table, int table_len, double guidance_scale, double recon_std_rescale, double* stats,
                                        int64_t n_stats, float* latents_recon, float* noise_pred, float* partials, int64_t n_partials,
                                        float* out) {
  SdsDims d;
  int64_t total;
  if (!sds_dims(d, total, b, n, f, c, P) || !eps || !latents_noisy || !latents || !noise || !t || !table || table_len < 1 ||
      !latents_recon || !partials || !out)
    return A3D_EINVAL;
  if (dtype != A3D_F32 && dtype != SG_STORAGE) return A3D_EINVAL;
  const bool rescaled = recon_std_rescale != 0.0;
  if (n_partials != d.chunks_all * b || (rescaled && (!stats || n_stats != d.chunks_rest * b * 4))) return A3D_EINVAL;
  if (!a3d_aligned(4, latents_noisy, latents, noise, table, latents_recon, noise_pred, partials, out) || !a3d_aligned(8, t) ||
      !a3d_aligned(8, stats) || !a3d_aligned(dtype == A3D_F32 ? 4 : 2, eps))
    return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g_stats = (unsigned)(d.chunks_rest * b), g_all = (unsigned)(d.chunks_all * b);
  if (dtype == A3D_F32) {
    if (rescaled) sds_stats_kernel<true><<<g_stats, LR_BLOCK, 0, st>>>(d, eps, latents, noise, t, table, table_len, guidance_scale, stats);
    sds_recon_kernel<true><<<g_all, LR_BLOCK, 0, st>>>(d, eps, latents_noisy, latents, noise, t, table, table_len, guidance_scale,
                                                       recon_std_rescale, stats, latents_recon, noise_pred, partials, n_partials);
  } else {
    if (rescaled) sds_stats_kernel<false><<<g_stats, LR_BLOCK, 0, st>>>(d, eps, latents, noise, t, table, table_len, guidance_scale, stats);
    sds_recon_kernel<false><<<g_all, LR_BLOCK, 0, st>>>(d, eps, latents_noisy, latents, noise, t, table, table_len, guidance_scale,
                                                        recon_std_rescale, stats, latents_recon, noise_pred, partials, n_partials);
  }
  sds_final_kernel<<<1, LR_BLOCK, 0, st>>>(partials, n_partials, (double)b * n * f, (double)f, out);
  return a3d_launch_status();
}

#ifndef A3D_STORAGE_F16   // fp32 on both sides: one copy, in the bf16 build of this source
extern "C" int a3d_sds_epilogue_bwd_f32(a3d_stream_t stream, int b, int n, int f, int c, int P, const float* latents,
                                        const float* latents_recon, float coef, const float* grad_out, float* grad) {
  SdsDims d;
  int64_t total;
  if (!sds_dims(d, total, b, n, f, c, P) || !latents || !latents_recon || !grad_out || !grad ||
      !a3d_aligned(4, latents, latents_recon, grad_out, grad))
    return A3D_EINVAL;
  sds_bwd_kernel<<<(unsigned)((total + LR_BLOCK - 1) / LR_BLOCK), LR_BLOCK, 0, (hipStream_t)stream>>>(total, f, (int64_t)c * P, latents,
                                                                                                     latents_recon, coef, grad_out, grad);
  return a3d_launch_status();
}
#endif
