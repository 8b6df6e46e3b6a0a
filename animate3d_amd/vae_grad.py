"""Input gradient of the VAE encoder: the 4D-SDS loss reaches the rendered pixels only through it.

The reference's guidance step (custom/threestudio-animate3d/guidance/animatemv_guidance.py:365-373, called at :536-543) encodes the
renderer's ``comp_rgb`` with autograd on: ``vae.encode(imgs * 2 - 1).latent_dist.sample() * scaling_factor``.  The UNet runs under
``no_grad`` and the VAE is frozen (:300-301), so what the step needs from the encoder is its vector-Jacobian product with respect to
the image — no weight gradients.  ``VaeGradOps`` is the op set ``AutoencoderKLEncoder.encode_images`` runs on when that gradient is
wanted: ``AutogradOps`` (conv dgrad incl. stride 2 through ``a3d_zero_insert2x``, GroupNorm(+SiLU) backward, GEMM input gradients,
``unpack_out``) plus the pieces only the encoder has:

    im2col_images       conv_in's operand from the [0, 1] image: (imgs * 2 - 1) -> a3d_im2col_in;  backward a3d_im2col_in_bwd
    channel_mix         quant_conv (fp32 1x1);  backward a3d_channel_mix_f32 with W^T
    vae_mid_attention   the single-head 512-wide mid-block attention (_VaeMidAttention: GEMMs, a3d_softmax_rows_bwd, GroupNorm backward)

The encoder's ``conv_out`` (512 -> 8 channels) takes the zero-padded dgrad route of ``autograd_ops._Conv3x3``.

Gradient scale.  The cotangent entering the encoder is small: (latents - recon) / 64 * f / (f - 1), times ``scaling_factor`` (0.18215)
for the posterior mean.  With fp16 storage (the reference runs this VAE in fp16) the input gradients of the early, large feature maps
would sink into fp16's subnormal range.  ``GRAD_SCALE`` = 2^10 multiplies the cotangent where it enters the encoder backward (the
quant_conv backward) and ``a3d_im2col_in_bwd`` removes it in fp32 — a power of two, so both steps are exact.  2^10 leaves a factor of
about 1500 to fp16's largest value for a scaled cotangent of 40 (an unscaled |d latents| of 0.04).  bf16 has fp32's range: the
scale changes nothing there and is applied all the same (one code path).
"""
from __future__ import annotations

import torch

from .autograd_ops import AutogradOps, _c
from .vae import mid_attention

GRAD_SCALE = 2.0 ** 10


class _ImagesIm2col(torch.autograd.Function):
    """imgs [B, C, H, W] in [0, 1] -> im2col rows [B H W, 64] of the fp32 image ``imgs * 2 - 1`` (computed in ``imgs.dtype`` as the
    caller's expression is, then widened: the same operand ``encode(imgs * 2 - 1)`` gets)."""

    @staticmethod
    def forward(ctx, gops, imgs, device):
        B, C, H, W = imgs.shape
        ctx.gops, ctx.geom, ctx.src = gops, (B, C, H, W), (imgs.device, imgs.dtype)
        img = (imgs * 2 - 1).to(device=device, dtype=torch.float32).contiguous()
        return gops.base.im2col_in(img.reshape(B, C, 1, H, W))

    @staticmethod
    def backward(ctx, dcol):
        B, C, H, W = ctx.geom
        # the 2 of imgs * 2 - 1 and the removal of the gradient scale, in fp32 (both powers of two: exact)
        dx = ctx.gops.base.im2col_in_bwd(_c(dcol), B, C, 1, H, W, 2.0 / ctx.gops.grad_scale)
        return None, dx.reshape(B, C, H, W).to(device=ctx.src[0], dtype=ctx.src[1]), None


class _ChannelMix(torch.autograd.Function):
    """y = scale * (W x) + bias per pixel (fp32, <= 8 channels); backward dX = scale * grad_scale * (W^T dY): the gradient scale enters here."""

    @staticmethod
    def forward(ctx, gops, x, w, bias, scale):
        ctx.gops, ctx.scale = gops, scale
        ctx.save_for_backward(w)
        return gops.base.channel_mix(x, w, bias, scale)

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        dx = ctx.gops.base.channel_mix(_c(dy.float()), w.t(), None, ctx.scale * ctx.gops.grad_scale)
        return None, dx, None, None, None


class _VaeMidAttention(torch.autograd.Function):
    """out = x + Attn(GroupNorm(x)) of the mid block (vae.mid_attention, the same kernels as the inference forward).  Saves t = GroupNorm(x),
    Q and K; the probabilities P are recomputed per image in the backward (the same two deterministic kernels: the P the forward multiplied by V).
    Per image, with S = alpha Q K^T, alpha = C^-0.5:

        dA = dOut Wo            dP = dA V0^T (fp32; V0 = t Wv^T without bias: the bias adds a row constant to dP that the softmax backward cancels)
        dS = alpha P o (dP - rowsum(P o dP))      (a3d_softmax_rows_bwd)
        dQ = dS K      dK = dS^T Q      dV0 = P^T dA          dt = [dQ | dK | dV0] [Wq; Wk; Wv]      dx = dOut + GroupNorm^T(dt)"""

    @staticmethod
    def forward(ctx, gops, x, B, L, pk, groups):
        out, t, q, k = mid_attention(gops.base, x, B, L, pk, groups, keep=True)
        ctx.gops, ctx.geom, ctx.pk = gops, (B, L, groups), pk
        ctx.save_for_backward(x, t, q, k)
        return out

    @staticmethod
    def backward(ctx, dout):
        base = ctx.gops.base
        x, t, q, k = ctx.saved_tensors
        B, L, groups = ctx.geom
        pk = ctx.pk
        C = x.shape[1]
        alpha = C ** -0.5
        dout = _c(dout)
        dA = base.gemm(dout, base.transpose(pk.o[0], pad=1))                 # dOut Wo  [B L, C]
        dqkv = base.empty(B * L, 3 * C)                                     # [dQ | dK | dV0]
        Lp = -(-L // 64) * 64                       # contractions over L: zero-padded to the GEMM's multiple of 64, as in the forward
        p_pad = ds_pad = None
        if Lp != L:
            p_pad, ds_pad = base.empty(L, Lp).zero_(), base.empty(L, Lp).zero_()
        for b in range(B):
            rows = slice(b * L, (b + 1) * L)
            s = base.gemm_f32out(q[rows], k[rows], alpha=alpha)
            p = base.softmax_rows(s) if p_pad is None else base.softmax_rows(s, out=p_pad[:, :L])
            v0 = base.gemm(t[rows], pk.v[0])                                # t Wv^T  [L, C]
            dp = base.gemm_f32out(dA[rows], v0)                             # dA V0^T  [L, L] fp32
            ds = base.softmax_rows_bwd(p, dp, alpha) if ds_pad is None else base.softmax_rows_bwd(p, dp, alpha, out=ds_pad[:, :L])
            base.gemm(ds if ds_pad is None else ds_pad, base.transpose(k[rows]), out=dqkv[rows, :C])              # dS K
            base.gemm(base.transpose(ds), base.transpose(q[rows]), out=dqkv[rows, C:2 * C])                      # dS^T Q
            base.gemm(base.transpose(p), base.transpose(dA[rows]), out=dqkv[rows, 2 * C:])                       # P^T dA
            del s, dp
        w_qkv_t = base.transpose(torch.cat([pk.q[0], pk.k[0], pk.v[0]]), pad=1)                                 # [Wq; Wk; Wv]^T  [C, 3C]
        dt = base.gemm(dqkv, w_qkv_t)
        stats = base.group_norm_stats(x, B, L, groups, 1e-6)
        dx, _, _ = base.group_norm_bwd(x, dt, B, L, pk.gn[0], pk.gn[1], groups, stats, False)
        base.axpby_(dout, dx)                                               # + the residual path
        return None, dx, None, None, None, None


class VaeGradOps(AutogradOps):
    """``AutogradOps`` over ``base`` plus the encoder-only differentiable ops (module docstring).  An op whose input needs no gradient runs
    the plain kernel."""

    def __init__(self, base, grad_scale: float = GRAD_SCALE):
        super().__init__(base)
        self.grad_scale = float(grad_scale)

    @staticmethod
    def _wants_grad(x) -> bool:
        return torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad

    def im2col_images(self, imgs, device):
        if self._wants_grad(imgs):
            return _ImagesIm2col.apply(self, imgs, device)
        B, C, H, W = imgs.shape
        return self.base.im2col_in((imgs * 2 - 1).to(device=device, dtype=torch.float32).contiguous().reshape(B, C, 1, H, W))

    def channel_mix(self, x, w, bias, scale: float = 1.0):
        if self._wants_grad(x):
            return _ChannelMix.apply(self, x, w, bias, scale)
        return self.base.channel_mix(x, w, bias, scale)

    def vae_mid_attention(self, x, B: int, L: int, pk, groups: int):
        if self._wants_grad(x):
            return _VaeMidAttention.apply(self, x, B, L, pk, groups)
        return mid_attention(self.base, x, B, L, pk, groups)
