// Backward kernels of the VAE encoder's input gradient (4D-SDS: the loss reaches the rendered pixels only through
// AutoencoderKL.encode, animatemv_guidance.py:365-373): the adjoint of a3d_im2col_in (conv_in on the fp32 image) and the
// row-softmax backward of the single-head 512-wide mid-block attention.  Everything else of the encoder backward reuses the
// training-path kernels (conv dgrad, GroupNorm backward, transposes, GEMMs).
#include "common.h"

namespace {

// dX[v, c, f, y, x] = scale * sum_{ky, kx} dCol[pixel (v, f, y - ky + 1, x - kx + 1)][(ky*3 + kx)*C + c] over the taps whose output pixel
// exists: the gather form of the col2im scatter (no atomics, fixed summation order).  One thread per output element, x fastest, so
// neighbouring lanes read neighbouring dCol rows; the 9 taps of a row are shared by 9 neighbours through the L2.
__global__ __launch_bounds__(256) void im2col_in_bwd_kernel(const uint16_t* dcol, float* dx, int V, int C, int F, int H, int W, float scale) {
  const int64_t total = (int64_t)V * C * F * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int f = (int)((i / ((int64_t)W * H)) % F);
    const int c = (int)((i / ((int64_t)W * H * F)) % C);
    const int v = (int)(i / ((int64_t)W * H * F * C));
    const int64_t frame = ((int64_t)v * F + f) * H;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = y - ky + 1;
      if (yy < 0 || yy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = x - kx + 1;
        if (xx < 0 || xx >= W) continue;
        acc += h2f(dcol[((frame + yy) * W + xx) * 64 + (ky * 3 + kx) * C + c]);
      }
    }
    dx[i] = scale * acc;
  }
}

// dS = alpha * P o (dP - rowsum(P o dP)): one wave per row, 4 columns per lane (16-byte fp32 loads of dP, 8-byte loads of P / stores of dS),
// the fp32 row sum reduced across the wave, then a second pass over the L2-resident row
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const uint16_t* P, int64_t ldp, const float* dP, int64_t lddp, uint16_t* dS,
                                                               int64_t ldds, int64_t M, int N, float alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const uint16_t* p = P + m * ldp;
  const float* d = dP + m * lddp;
  float s = 0.f;
  for (int c = lane * 4; c < N; c += 256) {
    const u32x2_t pv = *reinterpret_cast<const u32x2_t*>(p + c);
    const float4 dv = *reinterpret_cast<const float4*>(d + c);
    s = fmaf(lo16(pv[0]), dv.x, s);
    s = fmaf(hi16(pv[0]), dv.y, s);
    s = fmaf(lo16(pv[1]), dv.z, s);
    s = fmaf(hi16(pv[1]), dv.w, s);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  uint16_t* out = dS + m * ldds;
  for (int c = lane * 4; c < N; c += 256) {
    const u32x2_t pv = *reinterpret_cast<const u32x2_t*>(p + c);
    const float4 dv = *reinterpret_cast<const float4*>(d + c);
    u32x2_t o;
    o[0] = pack16(alpha * lo16(pv[0]) * (dv.x - s), alpha * hi16(pv[0]) * (dv.y - s));
    o[1] = pack16(alpha * lo16(pv[1]) * (dv.z - s), alpha * hi16(pv[1]) * (dv.w - s));
    *reinterpret_cast<u32x2_t*>(out + c) = o;
  }
}

}  // namespace

extern "C" int A3D_FN_BARE(a3d_im2col_in_bwd)(a3d_stream_t stream, const void* dCol, float* dX, int V, int C, int F, int H, int W, float scale) {
  if (!dCol || !dX || V <= 0 || C <= 0 || F <= 0 || H <= 0 || W <= 0 || 9 * C > 64) return A3D_EINVAL;
  if (!a3d_aligned(2, dCol) || !a3d_aligned(4, dX)) return A3D_EINVAL;
  im2col_in_bwd_kernel<<<grid_for((int64_t)V * C * F * H * W), 256, 0, (hipStream_t)stream>>>((const uint16_t*)dCol, dX, V, C, F, H, W, scale);
  return a3d_launch_status();
}

extern "C" int A3D_FN(a3d_softmax_rows_bwd)(a3d_stream_t stream, const void* P, int64_t ldp, const float* dP, int64_t lddp, void* dS, int64_t ldds,
                                           int64_t M, int64_t N, float alpha) {
  if (!P || !dP || !dS || M <= 0 || N <= 0 || N % 4 != 0 || N > 0x7fffffffLL || ldp < N || lddp < N || ldds < N) return A3D_EINVAL;
  if (ldp % 4 != 0 || lddp % 4 != 0 || ldds % 4 != 0) return A3D_EINVAL;
  if (!a3d_aligned(8, P, dS) || !a3d_aligned(16, dP)) return A3D_EINVAL;
  const int64_t nblk = (M + 3) / 4;
  if (nblk > 0x7fffffffLL) return A3D_EINVAL;
  softmax_rows_bwd_kernel<<<dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream>>>((const uint16_t*)P, ldp, dP, lddp, (uint16_t*)dS, ldds, M,
                                                                                      (int)N, alpha);
  return a3d_launch_status();
}
