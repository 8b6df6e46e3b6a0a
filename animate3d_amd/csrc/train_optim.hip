// Optimiser kernels of the training path (reference train.py:576-601: GradScaler, clip_grad_norm_, torch.optim.AdamW) on the fp32 master
// parameters, gradients and moments.  No 16-bit storage is touched, so there is one copy in the library (build.py SINGLE_STORAGE).
#include "common.h"

namespace {

// fp32 master parameters in one flat buffer
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { const float v = g[i]; s = fmaf(v, v, s); }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}
// ctrl[0] = factor applied to every gradient (1 / loss_scale, times the clip coefficient), ctrl[1] = 1 when the step must be skipped
// (non-finite gradients: GradScaler semantics of train.py:583-590), ctrl[2] = gradient norm after unscaling
__global__ void clip_ctrl_kernel(const float* __restrict__ sq, float max_norm, float inv_loss_scale, float* __restrict__ ctrl) {
  const float norm = sqrtf(sq[0]) * inv_loss_scale;
  const bool finite = isfinite(norm);
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(1.f, max_norm / (norm + 1e-6f));        // torch.nn.utils.clip_grad_norm_
  ctrl[0] = finite ? inv_loss_scale * coef : 0.f;
  ctrl[1] = finite ? 0.f : 1.f;
  ctrl[2] = norm;
}
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                     int64_t n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2,
                                                     const float* __restrict__ ctrl) {
  const float gs = ctrl ? ctrl[0] : 1.f;
  if (ctrl && ctrl[1] != 0.f) return;                                       // skipped step: parameters and moments untouched
  const float step = lr / bc1, rs = rsqrtf(bc2);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float gi = g[i] * gs;
    float pi = p[i] * (1.f - lr * wd);                                      // decoupled weight decay (torch.optim.AdamW)
    const float mi = fmaf(b1, m[i], (1.f - b1) * gi);
    const float vi = fmaf(b2, v[i], (1.f - b2) * gi * gi);
    pi -= step * mi / (sqrtf(vi) * rs + eps);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

}  // namespace

extern "C" int a3d_sqnorm_f32(a3d_stream_t stream, const float* g, int64_t n, float* out, int accumulate) {
  if (!g || !out || n <= 0) return A3D_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) { if (hipError_t e = hipMemsetAsync(out, 0, sizeof(float), s); e != hipSuccess) return (int)e; }
  int64_t blocks = (n + 2047) / 2048; if (blocks > 2048) blocks = 2048;
  sqnorm_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(g, n, out);
  return a3d_launch_status();
}

extern "C" int a3d_clip_ctrl_f32(a3d_stream_t stream, const float* sqnorm, float max_norm, float inv_loss_scale, float* ctrl) {
  if (!sqnorm || !ctrl) return A3D_EINVAL;
  clip_ctrl_kernel<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(sqnorm, max_norm, inv_loss_scale, ctrl);
  return a3d_launch_status();
}

extern "C" int a3d_adamw_f32(a3d_stream_t stream, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, float bias_corr1, float bias_corr2, const float* ctrl) {
  if (!p || !g || !m || !v || n <= 0 || bias_corr1 <= 0.f || bias_corr2 <= 0.f) return A3D_EINVAL;
  int64_t blocks = (n + 1023) / 1024; if (blocks > 4096) blocks = 4096;
  adamw_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, ctrl);
  return a3d_launch_status();
}
