// fp32 pieces of the denoise pipeline (gfx950): the VAE's few-channel 1x1 convolution, the CFG + DDIM epilogue of a step, and the
// library's version string.  No 16-bit storage is read or written here, so there is one copy of each in the library (build.py SINGLE_STORAGE).
#include "common.h"

namespace {

__global__ void cfg_ddim_kernel(const float* eps_pair, const float* x, const float* first, float* x_prev,
                                int64_t n, int C, int F, int64_t HW, float guidance, float sa_t, float s1a_t,
                                float sa_p, float s1a_p) {
  const int64_t per = (int64_t)C * F * HW, total = n * per;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t hw = i % HW;
    const int f = (int)((i / HW) % F);
    const int64_t vc = i / (HW * F);     // v*C + c
    if (f == 0) { x_prev[i] = first[vc * HW + hw]; continue; }
    const float eu = eps_pair[i], et = eps_pair[total + i];
    const float e = eu + guidance * (et - eu);
    const float x0 = (x[i] - s1a_t * e) / sa_t;
    x_prev[i] = sa_p * x0 + s1a_p * e;
  }
}

// y[b, o, p] = scale * (sum_c w[o, c] x[b, c, p]) + bias[o] on planar fp32 images with a handful of channels (VAE post_quant_conv)
__global__ void channel_mix_kernel(const float* X, const float* Wm, const float* bias, float* Y, int B, int Cin, int Cout, int64_t HW, float scale) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, px = i % HW;
    float xin[8];
    for (int c = 0; c < Cin; ++c) xin[c] = X[(b * Cin + c) * HW + px];
    for (int o = 0; o < Cout; ++o) {
      float acc = 0.f;
      for (int c = 0; c < Cin; ++c) acc = fmaf(Wm[o * Cin + c], xin[c], acc);
      Y[(b * Cout + o) * HW + px] = fmaf(scale, acc, bias ? bias[o] : 0.f);
    }
  }
}

}  // namespace

extern "C" const char* a3d_version(void) { return "animate3d_hip gfx950 r6 (bf16 + fp16 storage)"; }

extern "C" int a3d_channel_mix_f32(a3d_stream_t stream, const float* X, const float* W, const float* bias, float* Y,
                                   int B, int Cin, int Cout, int64_t HW, float scale) {
  if (!X || !W || !Y || B <= 0 || Cin <= 0 || Cin > 8 || Cout <= 0 || Cout > 8 || HW <= 0) return A3D_EINVAL;
  channel_mix_kernel<<<dim3(grid_for((int64_t)B * HW)), dim3(256), 0, (hipStream_t)stream>>>(X, W, bias, Y, B, Cin, Cout, HW, scale);
  return a3d_launch_status();
}

extern "C" int a3d_cfg_ddim_step_f32(a3d_stream_t stream, const float* eps_pair, const float* x, const float* first_frame,
                                     float* x_prev, int64_t n, int C, int F, int64_t HW, float guidance,
                                     float alpha_t, float alpha_prev) {
  if (!eps_pair || !x || !first_frame || !x_prev || n <= 0 || C <= 0 || F <= 0 || HW <= 0) return A3D_EINVAL;
  if (alpha_t <= 0.f || alpha_t > 1.f || alpha_prev <= 0.f || alpha_prev > 1.f) return A3D_EINVAL;
  cfg_ddim_kernel<<<grid_for(n * C * F * HW), 256, 0, (hipStream_t)stream>>>(
      eps_pair, x, first_frame, x_prev, n, C, F, HW, guidance, sqrtf(alpha_t), sqrtf(1.f - alpha_t), sqrtf(alpha_prev),
      sqrtf(1.f - alpha_prev));
  return a3d_launch_status();
}
