// Regularisers of the 4-D stage's training step on gfx950: the total variation of the clamped render and of the depth, the sparsity of
// alpha, and the three per-Gaussian terms (position, scale sum, opacity); contract in animate3d_amd/stage4d.py (image_regularizers,
// gaussian_regularizers).  Replaces the torch chains of custom/threestudio-animate3d/systems/animate3d.py:256-296 over
// threestudio/utils/loss.py:8-16: the clamped and permuted copy of the image, four shifted slices, their differences and squares, and the
// same again in the backward.
//
//   image_reg_fwd_kernel<G>   block j of image b covers pixels [j IR_PIXELS, (j + 1) IR_PIXELS) of that image in every plane that has a
//                             non-zero weight (three colour planes, depth, alpha): a run of whole rows at the stage's widths, so of the
//                             below-neighbours only the last row's, W of IR_PIXELS, lie in another block's run.  A thread accumulates
//                             IR_RUN pixels in fp32 as groups of G neighbours (G = 4: 16-byte reads; needs W % 4 == 0, so that a group
//                             lies in one row and its below-neighbours start on 16 bytes too, and 16-byte bases), then the block writes
//                             the five partials (tv down / right, depth-tv down / right, sparsity)
//   gauss_reg_fwd_kernel      the same over (image, Gaussian) pairs: GR_RUN pairs per thread, three partials
//   sr_final_kernel<K>        one block adds the K rows of partials; the order of both steps is loss_reduce.h's (no atomics, two calls
//                             are bitwise equal).  out = {sum of lambda * term, term 0, term 1, term 2}
//   image_reg_bwd_kernel<G>   gather form in the same geometry: the thread of pixel (y, x) recomputes its up to four differences from
//                             the inputs and writes d_image / d_depth / d_alpha in the planar layout a3d_gs_render_bwd_f32 reads
//   gauss_reg_bwd_kernel      d_means = c m / |m| (0 at |m| = 0, as torch.norm's backward), a constant d_scales, d_opacity = c |exp(s)|
// The upstream gradient is read through a device pointer; nothing but the inputs is needed.
#include "loss_reduce.h"

namespace {

constexpr int IR_RUN = 32;                         // pixels per thread
constexpr int IR_PIXELS = LR_BLOCK * IR_RUN;       // pixels per block: a3d_image_reg_f32's partials are B * ceil(H W / IR_PIXELS) fives
constexpr int GR_RUN = 4;                          // (image, Gaussian) pairs per thread
constexpr int GR_ITEMS = LR_BLOCK * GR_RUN;        // pairs per block: a3d_gaussian_reg_f32's partials are ceil(B N / GR_ITEMS) threes
static_assert(IR_RUN % 4 == 0, "a thread's run is a whole number of 4-pixel groups");

template <int G>
A3D_DEV void sr_load(const float* p, float (&v)[G]) {
  if constexpr (G == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int G>
A3D_DEV void sr_store(float* p, const float (&v)[G]) {
  if constexpr (G == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// the value the differences see: the render clamped as diff_gaussian_rasterizer_advanced_4d.py:180 does, the depth as it is
template <bool CLAMP>
A3D_DEV float sr_val(float v) { return CLAMP ? fminf(fmaxf(v, 0.f), 1.f) : v; }

// how the K sums become the three terms: sum k is scaled by scale[k] and added to term[k]; out[0] = sum of lambda[t] * term t
template <int K>
struct SrFinal {
  int term[K];
  double scale[K];
  double lambda[3];
};

template <int K>
__global__ __launch_bounds__(LR_BLOCK) void sr_final_kernel(const float* __restrict__ partials, int64_t n_partials, SrFinal<K> f,
                                                            float* __restrict__ out) {
  __shared__ double red[K][LR_BLOCK];
  lr_final_sums<K>(partials, n_partials, red);
  if (threadIdx.x == 0) {
    double t[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k) t[f.term[k]] += f.scale[k] * red[k][0];
    out[0] = (float)(f.lambda[0] * t[0] + f.lambda[1] * t[1] + f.lambda[2] * t[2]);
    out[1] = (float)t[0];
    out[2] = (float)t[1];
    out[3] = (float)t[2];
  }
}

// ---- the image terms

struct ImageRegArgs {
  int H, W, P;          // P = H W <= 2^30
  int64_t chunks;       // blocks per image
  const float* image;   // [B, 3, P] or NULL (lambda_tv = 0)
  const float* depth;   // [B, P] or NULL (lambda_depth_tv = 0)
  const float* alpha;   // [B, P] or NULL (lambda_sparsity = 0)
};

// squared differences of the G pixels at p (column x of their row) of plane pl to their below- and right-neighbours
template <int G, bool CLAMP>
A3D_DEV void ir_tv_fwd(const float* __restrict__ pl, int p, int x, bool below, int W, float& acc_h, float& acc_w) {
  float c[G];
  sr_load<G>(pl + p, c);
#pragma unroll
  for (int i = 0; i < G; ++i) c[i] = sr_val<CLAMP>(c[i]);
  if (below) {
    float d[G];
    sr_load<G>(pl + p + W, d);
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const float t = sr_val<CLAMP>(d[i]) - c[i];
      acc_h += t * t;
    }
  }
#pragma unroll
  for (int i = 0; i + 1 < G; ++i) {
    const float t = c[i + 1] - c[i];
    acc_w += t * t;
  }
  if (x + G < W) {
    const float t = sr_val<CLAMP>(pl[p + G]) - c[G - 1];
    acc_w += t * t;
  }
}

template <int G>
__global__ __launch_bounds__(LR_BLOCK) void image_reg_fwd_kernel(ImageRegArgs a, float* __restrict__ partials, int64_t n_partials) {
  __shared__ float red[5][LR_BLOCK];
  const int64_t b = (int64_t)blockIdx.x / a.chunks;
  const int p0 = (int)((int64_t)blockIdx.x % a.chunks) * IR_PIXELS;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < IR_RUN / G; ++i) {
    const int p = p0 + G * (i * LR_BLOCK + (int)threadIdx.x);
    if (p < a.P) {                                     // G = 4: P % 4 == 0, the whole group is inside and in one row
      const int y = p / a.W, x = p - y * a.W;
      const bool below = y + 1 < a.H;
      if (a.image) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ir_tv_fwd<G, true>(a.image + (b * 3 + c) * a.P, p, x, below, a.W, acc[0], acc[1]);
      }
      if (a.depth) ir_tv_fwd<G, false>(a.depth + b * a.P, p, x, below, a.W, acc[2], acc[3]);
      if (a.alpha) {
        float v[G];
        sr_load<G>(a.alpha + b * a.P + p, v);
#pragma unroll
        for (int j = 0; j < G; ++j) acc[4] += sqrtf(v[j] * v[j] + 0.01f);
      }
    }
  }
  lr_block_partials<5>(acc, red, partials, n_partials);
}

// d tv / d pl of the G pixels at p: ch (into - out of, vertically) + cw (the same horizontally), through the clamp rule for the render
template <int G, bool CLAMP>
A3D_DEV void ir_tv_bwd(const float* __restrict__ pl, float* __restrict__ dpl, int p, int y, int x, int H, int W, float ch, float cw) {
  float raw[G], c[G], gh[G], o[G];
  sr_load<G>(pl + p, raw);
#pragma unroll
  for (int i = 0; i < G; ++i) c[i] = sr_val<CLAMP>(raw[i]), gh[i] = 0.f;
  if (y > 0) {
    float u[G];
    sr_load<G>(pl + p - W, u);
#pragma unroll
    for (int i = 0; i < G; ++i) gh[i] += c[i] - sr_val<CLAMP>(u[i]);
  }
  if (y + 1 < H) {
    float d[G];
    sr_load<G>(pl + p + W, d);
#pragma unroll
    for (int i = 0; i < G; ++i) gh[i] -= sr_val<CLAMP>(d[i]) - c[i];
  }
  const bool has_left = x > 0, has_right = x + G < W;
  const float left = has_left ? sr_val<CLAMP>(pl[p - 1]) : 0.f, right = has_right ? sr_val<CLAMP>(pl[p + G]) : 0.f;
#pragma unroll
  for (int i = 0; i < G; ++i) {
    float gw = 0.f;
    if (i > 0 || has_left) gw += c[i] - (i > 0 ? c[i - 1] : left);
    if (i + 1 < G || has_right) gw -= (i + 1 < G ? c[i + 1] : right) - c[i];
    const float g = ch * gh[i] + cw * gw;
    o[i] = (!CLAMP || (raw[i] >= 0.f && raw[i] <= 1.f)) ? g : 0.f;     // torch's clamp rule: bounds inclusive, exactly 0 outside
  }
  sr_store<G>(dpl + p, o);
}

struct ImageRegCoefs {
  float tv_h, tv_w, dtv_h, dtv_w, sparsity;
};

template <int G>
__global__ __launch_bounds__(LR_BLOCK) void image_reg_bwd_kernel(ImageRegArgs a, ImageRegCoefs k, const float* __restrict__ grad_out,
                                                                 float* __restrict__ d_image, float* __restrict__ d_depth,
                                                                 float* __restrict__ d_alpha) {
  const int64_t b = (int64_t)blockIdx.x / a.chunks;
  const int p0 = (int)((int64_t)blockIdx.x % a.chunks) * IR_PIXELS;
  const float g = grad_out[0];
#pragma unroll
  for (int i = 0; i < IR_RUN / G; ++i) {
    const int p = p0 + G * (i * LR_BLOCK + (int)threadIdx.x);
    if (p < a.P) {
      const int y = p / a.W, x = p - y * a.W;
      if (d_image) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          ir_tv_bwd<G, true>(a.image + (b * 3 + c) * a.P, d_image + (b * 3 + c) * a.P, p, y, x, a.H, a.W, g * k.tv_h, g * k.tv_w);
      }
      if (d_depth) ir_tv_bwd<G, false>(a.depth + b * a.P, d_depth + b * a.P, p, y, x, a.H, a.W, g * k.dtv_h, g * k.dtv_w);
      if (d_alpha) {
        float v[G], o[G];
        sr_load<G>(a.alpha + b * a.P + p, v);
#pragma unroll
        for (int j = 0; j < G; ++j) o[j] = g * k.sparsity * v[j] / sqrtf(v[j] * v[j] + 0.01f);
        sr_store<G>(d_alpha + b * a.P + p, o);
      }
    }
  }
}

// the shared argument check: everything a launch depends on, before the first HIP call.  Returns the number of blocks, 0 for a refusal
int64_t image_reg_args(ImageRegArgs& a, int B, int H, int W, const float* image, const float* depth, const float* alpha) {
  if (B <= 0 || H <= 0 || W <= 0 || (!image && !depth && !alpha)) return 0;
  if ((image || depth) && (H < 2 || W < 2)) return 0;                                       // the reference divides by zero
  if (!a3d_aligned(4, image, depth, alpha)) return 0;
  const int64_t P = (int64_t)H * W;
  if (P > ((int64_t)1 << 30)) return 0;                                                     // pixel numbers within an image are ints
  const int64_t chunks = (P + IR_PIXELS - 1) / IR_PIXELS;
  if (chunks > (int64_t)0x7fffffff / B) return 0;                                           // the grid's x extent
  a = ImageRegArgs{H, W, (int)P, chunks, image, depth, alpha};
  return chunks * B;
}

bool image_reg_vec(const ImageRegArgs& a, const float* d_image, const float* d_depth, const float* d_alpha) {
  return a.W % 4 == 0 && a3d_aligned(16, a.image, a.depth, a.alpha, d_image, d_depth, d_alpha);
}

// ---- the per-Gaussian terms

struct GaussRegArgs {
  int BN, N;             // B N <= 2^30
  const float* means;    // [B, N, 3] or NULL (lambda_position = 0)
  const float* scales;   // image b at scales + b scales_bs, [N, 3]; or NULL (lambda_scales = 0)
  int64_t scales_bs;     // 3 N, or 0 for one [N, 3] shared by every image
  const float* scaling;  // [N, 3] log-scales, and
  const float* opacity;  // [N]; or both NULL (lambda_opacity = 0)
};

A3D_DEV float gr_norm3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

A3D_DEV float gr_scale_norm(const float* __restrict__ s) { return gr_norm3(expf(s[0]), expf(s[1]), expf(s[2])); }

__global__ __launch_bounds__(LR_BLOCK) void gauss_reg_fwd_kernel(GaussRegArgs a, float* __restrict__ partials, int64_t n_partials) {
  __shared__ float red[3][LR_BLOCK];
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < GR_RUN; ++r) {
    const int i = (int)blockIdx.x * GR_ITEMS + r * LR_BLOCK + (int)threadIdx.x;
    if (i < a.BN) {
      if (a.means) {
        const float* m = a.means + (int64_t)i * 3;
        acc[0] += gr_norm3(m[0], m[1], m[2]);
      }
      if (a.scales) {
        const int b = i / a.N, n = i - b * a.N;
        const float* s = a.scales + b * a.scales_bs + (int64_t)n * 3;
        acc[1] += s[0];
        acc[1] += s[1];
        acc[1] += s[2];
      }
      if (a.scaling && i < a.N) acc[2] += gr_scale_norm(a.scaling + (int64_t)i * 3) * a.opacity[i];
    }
  }
  lr_block_partials<3>(acc, red, partials, n_partials);
}

__global__ __launch_bounds__(LR_BLOCK) void gauss_reg_bwd_kernel(GaussRegArgs a, float coef_position, float coef_scales, float coef_opacity,
                                                                 const float* __restrict__ grad_out, float* __restrict__ d_means,
                                                                 float* __restrict__ d_scales, float* __restrict__ d_opacity) {
  const float g = grad_out[0];
#pragma unroll
  for (int r = 0; r < GR_RUN; ++r) {
    const int i = (int)blockIdx.x * GR_ITEMS + r * LR_BLOCK + (int)threadIdx.x;
    if (i < a.BN) {
      if (d_means) {
        const float* m = a.means + (int64_t)i * 3;
        const float x = m[0], y = m[1], z = m[2], len = gr_norm3(x, y, z);
        const float c = len > 0.f ? g * coef_position / len : 0.f;                          // torch.norm's backward: 0 at |m| = 0
        float* d = d_means + (int64_t)i * 3;
        d[0] = c * x, d[1] = c * y, d[2] = c * z;
      }
      if (d_scales) {
        float* d = d_scales + (int64_t)i * 3;
        d[0] = d[1] = d[2] = g * coef_scales;
      }
      if (d_opacity && i < a.N) d_opacity[i] = g * coef_opacity * gr_scale_norm(a.scaling + (int64_t)i * 3);
    }
  }
}

// Returns the number of blocks, 0 for a refusal
int64_t gauss_reg_args(GaussRegArgs& a, int B, int N, const float* means, const float* scales, int64_t scales_bs, const float* scaling,
                       const float* opacity) {
  if (B <= 0 || N <= 0 || (scales && scales_bs != 0 && scales_bs != (int64_t)3 * N)) return 0;
  if (!a3d_aligned(4, means, scales, scaling, opacity)) return 0;
  const int64_t BN = (int64_t)B * N;
  if (BN > ((int64_t)1 << 30)) return 0;                                                    // pair numbers are ints
  a = GaussRegArgs{(int)BN, N, means, scales, scales_bs, scaling, opacity};
  return (BN + GR_ITEMS - 1) / GR_ITEMS;
}

}  // namespace

extern "C" int a3d_image_reg_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* depth, const float* alpha,
                                 double lambda_tv, double lambda_depth_tv, double lambda_sparsity, float* partials, int64_t n_partials,
                                 float* out) {
  if ((lambda_tv != 0.0 && !image) || (lambda_depth_tv != 0.0 && !depth) || (lambda_sparsity != 0.0 && !alpha)) return A3D_EINVAL;
  ImageRegArgs a;
  const int64_t blocks = image_reg_args(a, B, H, W, lambda_tv != 0.0 ? image : nullptr, lambda_depth_tv != 0.0 ? depth : nullptr,
                                        lambda_sparsity != 0.0 ? alpha : nullptr);
  if (blocks == 0 || !partials || !out || !a3d_aligned(4, partials, out) || n_partials != blocks) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (image_reg_vec(a, nullptr, nullptr, nullptr)) image_reg_fwd_kernel<4><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, partials, n_partials);
  else image_reg_fwd_kernel<1><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, partials, n_partials);
  // tv(x) = 2 (sum_down / (C (H - 1) W) + sum_right / (C H (W - 1))) / B (threestudio/utils/loss.py:8-16); sparsity: a mean over B H W
  const double h = H, w = W, tv = 2.0 / (double)B;
  const double down = (h - 1.0) * w, right = h * (w - 1.0);                                 // 0 only where no TV term is on
  SrFinal<5> f{{0, 0, 1, 1, 2}, {a.image ? tv / (3.0 * down) : 0.0, a.image ? tv / (3.0 * right) : 0.0, a.depth ? tv / down : 0.0,
                                a.depth ? tv / right : 0.0, 1.0 / ((double)B * h * w)},
               {lambda_tv, lambda_depth_tv, lambda_sparsity}};
  sr_final_kernel<5><<<1, LR_BLOCK, 0, st>>>(partials, n_partials, f, out);
  return a3d_launch_status();
}

extern "C" int a3d_image_reg_bwd_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* depth, const float* alpha,
                                     float coef_tv_h, float coef_tv_w, float coef_depth_tv_h, float coef_depth_tv_w, float coef_sparsity,
                                     const float* grad_out, float* d_image, float* d_depth, float* d_alpha) {
  if ((d_image && !image) || (d_depth && !depth) || (d_alpha && !alpha) || (!d_image && !d_depth && !d_alpha)) return A3D_EINVAL;
  ImageRegArgs a;
  const int64_t blocks = image_reg_args(a, B, H, W, d_image ? image : nullptr, d_depth ? depth : nullptr, d_alpha ? alpha : nullptr);
  if (blocks == 0 || !grad_out || !a3d_aligned(4, grad_out, d_image, d_depth, d_alpha)) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const ImageRegCoefs k{coef_tv_h, coef_tv_w, coef_depth_tv_h, coef_depth_tv_w, coef_sparsity};
  if (image_reg_vec(a, d_image, d_depth, d_alpha))
    image_reg_bwd_kernel<4><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, k, grad_out, d_image, d_depth, d_alpha);
  else
    image_reg_bwd_kernel<1><<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, k, grad_out, d_image, d_depth, d_alpha);
  return a3d_launch_status();
}

extern "C" int a3d_gaussian_reg_f32(a3d_stream_t stream, int B, int N, const float* means, const float* scales, int64_t scales_bs,
                                    const float* scaling, const float* opacity, double lambda_position, double lambda_scales,
                                    double lambda_opacity, float* partials, int64_t n_partials, float* out) {
  if ((lambda_position != 0.0 && !means) || (lambda_scales != 0.0 && !scales) || (lambda_opacity != 0.0 && (!scaling || !opacity)))
    return A3D_EINVAL;
  GaussRegArgs a;
  const bool op = lambda_opacity != 0.0;
  const int64_t blocks = gauss_reg_args(a, B, N, lambda_position != 0.0 ? means : nullptr, lambda_scales != 0.0 ? scales : nullptr, scales_bs,
                                        op ? scaling : nullptr, op ? opacity : nullptr);
  if (blocks == 0 || (!a.means && !a.scales && !a.scaling) || !partials || !out || !a3d_aligned(4, partials, out) || n_partials != blocks)
    return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  gauss_reg_fwd_kernel<<<(unsigned)blocks, LR_BLOCK, 0, st>>>(a, partials, n_partials);
  // position: a mean over (B, N); the scale sum and the opacity term are sums
  SrFinal<3> f{{0, 1, 2}, {1.0 / ((double)B * (double)N), 1.0, 1.0}, {lambda_position, lambda_scales, lambda_opacity}};
  sr_final_kernel<3><<<1, LR_BLOCK, 0, st>>>(partials, n_partials, f, out);
  return a3d_launch_status();
}

extern "C" int a3d_gaussian_reg_bwd_f32(a3d_stream_t stream, int B, int N, const float* means, const float* scaling, float coef_position,
                                        float coef_scales, float coef_opacity, const float* grad_out, float* d_means, float* d_scales,
                                        float* d_opacity) {
  if ((d_means && !means) || (d_opacity && !scaling) || (!d_means && !d_scales && !d_opacity)) return A3D_EINVAL;
  GaussRegArgs a;
  // the backward reads no scales and no opacity: d_scales is a constant, d_opacity needs the log-scales only
  const int64_t blocks = gauss_reg_args(a, B, N, d_means ? means : nullptr, nullptr, 0, d_opacity ? scaling : nullptr, nullptr);
  if (blocks == 0 || !grad_out || !a3d_aligned(4, grad_out, d_means, d_scales, d_opacity)) return A3D_EINVAL;
  gauss_reg_bwd_kernel<<<(unsigned)blocks, LR_BLOCK, 0, (hipStream_t)stream>>>(a, coef_position, coef_scales, coef_opacity, grad_out, d_means,
                                                                              d_scales, d_opacity);
  return a3d_launch_status();
}
