"""One optimisation step of the 4-D stage: the reconstruction branch on the gfx950 kernel of csrc/recon_loss.hip, the image and Gaussian
regularisers on those of csrc/stage_reg.hip, the renderer's policy and the step around them.

The reference's step is ``Animate3DSystem.training_step`` (custom/threestudio-animate3d/systems/animate3d.py:120-370) over
``Gaussian4DBatchRenderer.batch_forward`` (renderer/gaussian_batch_renderer_4d.py) and ``DiffGaussian4D.forward``
(renderer/diff_gaussian_rasterizer_advanced_4d.py:60-193).  Stage 1 (``motion_recon_frame_16.yaml``: ``load_guidance: false``) makes no
UNet call: its step is exactly the fp32 kernels of ``deform4d``, ``splat``, ``arap`` and this module.  fp32 only; CPU tensors raise, there
is no torch fallback.

``masked_recon_loss(image, alpha, gt_rgb, gt_mask, index=None, *, bg, lambda_rgb, lambda_mask) -> (loss, loss_rgb, loss_mask)``

* ``image [B, 3, H, W]``: the rasterizer's unclamped output; ``alpha [B, 1, H, W]`` or ``[B, H, W]``; ``gt_rgb [S, H, W, 3]``, the data
  module's tensor, read in place; ``gt_mask [S, H, W, 1]`` or ``[S, H, W]``, ``bool`` or ``uint8`` (a float mask raises ``TypeError``: the
  reference's mask is ``bool``, data/simple_multi_image.py:215, and with a two-valued mask the compositing is an exact select).
* ``index [B]``: image b is compared with frame ``index[b]`` (repeats are legal); it replaces ``batch[key] = val[sampled_idx]``
  (animate3d.py:160-165).  ``None`` is the identity and needs ``S == B``.  A list or CPU tensor is range-checked here; **a device tensor is
  not, and the kernels clamp nothing: the caller owns its range**.
* ``loss_rgb = mean((clamp(image, 0, 1) - (m ? gt : bg))^2)`` over ``B H W 3`` (``F.mse_loss(gt_rgb, pred_rgb)`` of animate3d.py:175-179
  with the clamp of advanced_4d.py:180; ``bg`` is one scalar because the reference uses ``back_ground_color[0]``);
  ``loss_mask = mean((alpha - m)^2)`` over ``B H W``, alpha unclamped (:183); ``loss = lambda_rgb loss_rgb + lambda_mask loss_mask``.
  All three are 0-d fp32; ``loss_rgb`` and ``loss_mask`` are detached (for logging): the gradient flows through ``loss`` only.
* Summation has no atomics and one fixed order (csrc/loss_reduce.h): two calls are bitwise equal.  The backward recomputes from the
  four inputs (no gradient buffer is kept: at 60 x 1024^2 it would be 1 GB): ``d_image = g (2 lambda_rgb / n_rgb)(c - y)`` where
  ``0 <= image <= 1`` and exactly 0 elsewhere (torch's clamp rule), ``d_alpha = g (2 lambda_mask / n_mask)(alpha - m)``, in the planar
  layout the rasterizer's backward reads.  The upstream gradient is read on the device: neither direction synchronises with the host.
  Without a gradient to compute nothing is saved.

``masked_recon_loss_rgba8(image, alpha, gt_rgba8, index=None, *, bg, lambda_rgb, lambda_mask)``: the same loss on the same two kernels,
reading ``gt_rgba8 [S, H, W, 4]`` uint8 (``frames.FrameSet``) as ``byte / 255.0f`` and ``alpha byte >= 128``: bit-equal results, 4 bytes of
ground truth a pixel where ``gt_rgb`` + ``gt_mask`` are 13.

``image_regularizers(image, depth, alpha, *, lambda_tv, lambda_depth_tv, lambda_sparsity) -> (loss, tv, depth_tv, sparsity)`` and
``gaussian_regularizers(means, scales, scaling, opacity, *, lambda_position, lambda_scales, lambda_opacity) -> (loss, position, scale_sum,
opacity_term)``: the six terms of animate3d.py:256-296, one forward and one backward kernel per call.

* ``tv(x) = 2 (sum (x[y+1] - x[y])^2 / (C (H-1) W) + sum (x[x+1] - x[x])^2 / (C H (W-1))) / B`` (threestudio/utils/loss.py:8-16) of
  ``x = clamp(image, 0, 1)`` (``C = 3``: the ``comp_rgb`` of the reference, never materialised) and, as ``depth_tv``, of the unnormalised
  ``depth [B, 1, H, W]`` (``C = 1``, no clamp); ``sparsity = mean(sqrt(alpha^2 + 0.01))`` over ``B H W``.  ``H < 2`` or ``W < 2`` with a
  TV weight raises ``ValueError`` before any launch (the reference divides by zero).  The gradient reaches the raw ``image`` through
  torch's clamp rule (it passes where ``0 <= image <= 1``, exactly 0 elsewhere; the differences use the clamped neighbours); the backward
  is gather form, recomputed from the inputs, in the planar layout the rasterizer's backward reads.
* ``position = mean over (B, N) of |means|`` (the renderer's *unmasked* means; the gradient at a zero-length mean is 0, as
  ``torch.norm``'s), ``scale_sum = sum(scales)`` (the activated ``[B, N, 3]`` the rasterizer receives; an ``[N, 3]`` expanded over the
  images is read in place and counted B times), ``opacity_term = sum_N |exp(scaling)| opacity`` with the static Gaussians' log-``scaling``
  detached: the gradient goes to ``opacity [N, 1]`` / ``[N]`` only.
* ``loss`` is the weighted sum and the only differentiable output; the named terms are detached and unweighted.  A term whose weight is 0
  is neither read nor computed (its operand may be ``None``, its named term is 0, its gradient ``None``).  Same rules as the
  reconstruction loss: fp32 CUDA tensors of exactly these shapes, no atomics (two calls are bitwise equal), the upstream gradient read
  on the device, nothing but the inputs saved, and nothing at all without a gradient to compute.

``sampled_frames`` / ``sampled_image_index`` restate the progressive frame schedule (animate3d.py:134-157); ``render_batch`` is the
renderer for a whole batch with the policy of advanced_4d.py:130-162; ``training_step`` is the step, with either ARAP branch (the k-NN
graph or the mesh's connectivity); ``vertex_trajectory`` the deformed means of every frame (``save_gaussian_trajectory``);
``field_param_groups`` the optimiser groups of geometry/gaussian_4d.py:344-391; ``fit`` the loop around the step, for any optimiser
(``stage_optim.StageAdam`` is the stage's own).
"""
from __future__ import annotations

import random
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Union

import torch

from .arap import ArapGraph, MeshGraph, arap_energy
from .cameras import CameraBatch
from .deform4d import HexPlaneDeformation
from .f32_stage import launch, launch_reduced, require_f32_cuda, require_index_cuda, require_shape
from .hip_ops import _p
from .splat import get_cam_info_gaussian, rasterize_gaussians

PIXELS_PER_BLOCK = 2048          # RL_PIXELS of csrc/recon_loss.hip: one (rgb, mask) partial per block
REG_PIXELS_PER_BLOCK = 8192      # IR_PIXELS of csrc/stage_reg.hip: five partials per block
REG_PAIRS_PER_BLOCK = 1024       # GR_ITEMS of csrc/stage_reg.hip: three partials per block
UNSUPPORTED_LAMBDAS = ("lambda_normal_tv",)   # the reference's renderer never produces comp_normal, and its own step fails at :354
IMAGE_REG_LAMBDAS = ("lambda_tv_loss", "lambda_depth_tv_loss", "lambda_sparsity")
GAUSSIAN_REG_LAMBDAS = ("lambda_position", "lambda_scales", "lambda_opacity")
REG_ORDER = (("lambda_position", "loss_position"), ("lambda_opacity", "loss_opacity"), ("lambda_sparsity", "loss_sparsity"),
             ("lambda_scales", "loss_scales"), ("lambda_tv_loss", "loss_tv"), ("lambda_depth_tv_loss", "loss_depth_tv"))   # animate3d.py:256-296


# ---- the loss kernels: a forward ends in csrc/loss_reduce.h's reduction (launch_reduced), a backward writes only the gradients asked for

def _upstream(d_out):                                            # g[0]: the gradient of `loss`, which the kernel reads on the device
    return d_out.detach().float().contiguous()


def _empty_grads(need, shapes, device):                          # a gradient for the kernel to fill where needed, else None (NULL)
    return [torch.empty(shape, dtype=torch.float32, device=device) if n else None for n, shape in zip(need, shapes)]


class _MaskedReconLoss(torch.autograd.Function):
    """``gt``: ``(gt_rgb, gt_mask)`` for the fp32 entry points, ``(gt_rgba8,)`` for the 8-bit ones; everything else is one code."""

    @staticmethod
    def forward(ctx, image, alpha, index, bg, lambda_rgb, lambda_mask, *gt):
        B, _, H, W = image.shape
        img, alp = image.detach().contiguous(), alpha.detach().contiguous()
        ctx.entry = "a3d_recon_loss" + ("_rgba8" if len(gt) == 1 else "")
        out = launch_reduced(ctx.entry + "_f32", image.device, (B, H, W), (_p(img), _p(alp), *(_p(t) for t in gt), _p(index), bg,
                             lambda_rgb, lambda_mask), 2, (B, H * W, PIXELS_PER_BLOCK), 3)
        ctx.need = tuple(ctx.needs_input_grad[:2])
        if any(ctx.need):
            ctx.save_for_backward(img, alp, index, *gt)
            ctx.consts = (bg, 2.0 * lambda_rgb / (3.0 * B * H * W), 2.0 * lambda_mask / (1.0 * B * H * W), alpha.shape)
        return out

    @staticmethod
    def backward(ctx, d_out):
        img, alp, index, *gt = ctx.saved_tensors
        bg, coef_rgb, coef_mask, alpha_shape = ctx.consts
        B, _, H, W = img.shape
        g = _upstream(d_out)
        d_image, d_alpha = _empty_grads(ctx.need, (img.shape, alpha_shape), img.device)
        launch(ctx.entry + "_bwd_f32", img.device, B, H, W, _p(img), _p(alp), *(_p(t) for t in gt), _p(index), bg, coef_rgb, coef_mask,
               _p(g), _p(d_image), _p(d_alpha))
        return (d_image, d_alpha, None, None, None, None, *(None for _ in gt))


def _recon_index(index, S: int, B: int, dev):
    """``index`` as the kernels take it: int32 ``[B]`` on ``dev``, or ``None``.  A list or CPU tensor is range-checked, a device tensor is not."""
    if index is None:
        return None
    if not (isinstance(index, torch.Tensor) and index.is_cuda):
        index = torch.as_tensor(index)
        if index.dtype not in (torch.int32, torch.int64) or index.dim() != 1:
            raise ValueError("index: a 1-D int32 / int64 tensor or a list of ints")
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= S):
            raise IndexError(f"index: values must lie in [0, {S}), got [{int(index.min())}, {int(index.max())}]")
        index = index.to(dev)
    require_index_cuda("index", index)
    if tuple(index.shape) != (B,):
        raise ValueError(f"index: expected [{B}], got {tuple(index.shape)}")
    return index.to(torch.int32).contiguous()


def masked_recon_loss(image: torch.Tensor, alpha: torch.Tensor, gt_rgb: torch.Tensor, gt_mask: torch.Tensor, index=None, *, bg: float,
                      lambda_rgb: float, lambda_mask: float):
    """(loss, loss_rgb, loss_mask) of the renders ``image`` / ``alpha`` against frames ``index`` of ``gt_rgb`` / ``gt_mask``; see the module
    docstring.  A device ``index`` is not range-checked: the caller owns its range."""
    if not isinstance(gt_mask, torch.Tensor) or gt_mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"gt_mask: expected a bool or uint8 tensor, got {getattr(gt_mask, 'dtype', type(gt_mask))} (the tracked masks are "
                        "two-valued; threshold a soft mask first)")
    for name, t in (("image", image), ("alpha", alpha), ("gt_rgb", gt_rgb)):
        require_shape(name, t)                                   # tensors all three, before any shape is judged
    require_shape("image", image, ("B", 3, "H", "W"), non_empty=True)
    B, _, H, W = image.shape
    require_shape("alpha", alpha, (B, 1, H, W), (B, H, W))
    require_shape("gt_rgb", gt_rgb, ("S", H, W, 3))
    S = gt_rgb.shape[0]
    require_shape("gt_mask", gt_mask, (S, H, W, 1), (S, H, W))
    if index is None and S != B:
        raise ValueError(f"index=None compares image b with frame b: needs S == B, got S = {S}, B = {B}")
    require_f32_cuda("image", image)
    require_f32_cuda("alpha", alpha)
    require_f32_cuda("gt_rgb", gt_rgb)
    if not gt_mask.is_cuda:
        raise RuntimeError("gt_mask: expected a CUDA tensor (no CPU fallback)")
    if gt_rgb.requires_grad:
        raise NotImplementedError("gt_rgb.requires_grad: the ground truth is data")
    index = _recon_index(index, S, B, image.device)
    gt = gt_rgb.detach().contiguous()                            # the data module's tensors are contiguous: no copy
    mask = gt_mask.contiguous()
    mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    out = _MaskedReconLoss.apply(image, alpha, index, float(bg), float(lambda_rgb), float(lambda_mask), gt, mask)
    return out[0], out[1].detach(), out[2].detach()


def masked_recon_loss_rgba8(image: torch.Tensor, alpha: torch.Tensor, gt_rgba8: torch.Tensor, index=None, *, bg: float, lambda_rgb: float,
                            lambda_mask: float):
    """``masked_recon_loss`` against 8-bit ground truth: ``gt_rgba8 [S, H, W, 4]`` uint8 (``frames.FrameSet.rgba8``) in place of ``gt_rgb`` and
    ``gt_mask``, 4 bytes a pixel where those are 13.  The kernels are the same two with another reader of the ground truth: colour
    ``byte / 255.0f`` by IEEE division and inside ``alpha byte >= 128``, so the three losses and both gradients are bit-equal to
    ``masked_recon_loss`` on ``gt_rgba8[..., :3].float() / 255`` and ``gt_rgba8[..., 3:] >= 128`` (the reference's tensors,
    data/simple_multi_image.py:205-215).  Everything else is that function's contract: ``index``, the reduction, a backward that recomputes
    from the inputs and saves nothing else."""
    for name, t in (("image", image), ("alpha", alpha), ("gt_rgba8", gt_rgba8)):
        require_shape(name, t)
    if gt_rgba8.dtype != torch.uint8:
        raise TypeError(f"gt_rgba8: expected a uint8 tensor, got {gt_rgba8.dtype}")
    require_shape("image", image, ("B", 3, "H", "W"), non_empty=True)
    B, _, H, W = image.shape
    require_shape("alpha", alpha, (B, 1, H, W), (B, H, W))
    require_shape("gt_rgba8", gt_rgba8, ("S", H, W, 4))
    S = gt_rgba8.shape[0]
    if index is None and S != B:
        raise ValueError(f"index=None compares image b with frame b: needs S == B, got S = {S}, B = {B}")
    require_f32_cuda("image", image)
    require_f32_cuda("alpha", alpha)
    if not gt_rgba8.is_cuda:
        raise RuntimeError("gt_rgba8: expected a CUDA tensor (no CPU fallback)")
    index = _recon_index(index, S, B, image.device)
    out = _MaskedReconLoss.apply(image, alpha, index, float(bg), float(lambda_rgb), float(lambda_mask), gt_rgba8.contiguous())
    return out[0], out[1].detach(), out[2].detach()


# ---- the regularisers (animate3d.py:256-296, threestudio/utils/loss.py:8-16; csrc/stage_reg.hip)

class _ImageReg(torch.autograd.Function):
    """out [4] = (loss, tv, depth_tv, sparsity); an operand whose lambda is 0 is handed to the kernel as NULL."""

    @staticmethod
    def forward(ctx, image, depth, alpha, shape, lambdas):
        B, H, W = shape
        ops = [t.detach().contiguous() if lam != 0.0 else None for t, lam in zip((image, depth, alpha), lambdas)]
        dev = next(t for t in ops if t is not None).device
        out = launch_reduced("a3d_image_reg_f32", dev, (B, H, W), (*(_p(t) for t in ops), *lambdas), 5, (B, H * W, REG_PIXELS_PER_BLOCK), 4)
        ctx.need = tuple(t is not None and need for t, need in zip(ops, ctx.needs_input_grad[:3]))
        if any(ctx.need):
            ctx.save_for_backward(*(t if need else None for t, need in zip(ops, ctx.need)))
            l_tv, l_dtv, l_sp = lambdas
            down, right, n = (H - 1.0) * W * B, H * (W - 1.0) * B, 1.0 * B * H * W
            ctx.consts = (shape, (4.0 * l_tv / (3.0 * down) if l_tv else 0.0, 4.0 * l_tv / (3.0 * right) if l_tv else 0.0,
                                  4.0 * l_dtv / down if l_dtv else 0.0, 4.0 * l_dtv / right if l_dtv else 0.0, l_sp / n))
        return out

    @staticmethod
    def backward(ctx, d_out):
        ops = ctx.saved_tensors
        (B, H, W), coefs = ctx.consts
        g = _upstream(d_out)
        grads = _empty_grads(ctx.need, (need and t.shape for t, need in zip(ops, ctx.need)), g.device)
        launch("a3d_image_reg_bwd_f32", g.device, B, H, W, *(_p(t) for t in ops), *coefs, _p(g), *(_p(t) for t in grads))
        return (*grads, None, None)


def image_regularizers(image: torch.Tensor, depth: Optional[torch.Tensor], alpha: Optional[torch.Tensor], *, lambda_tv: float,
                       lambda_depth_tv: float, lambda_sparsity: float):
    """(loss, tv, depth_tv, sparsity) of the raw render ``image [B, 3, H, W]``, ``depth [B, 1, H, W]`` and ``alpha [B, 1, H, W]`` /
    ``[B, H, W]``; see the module docstring.  ``depth`` / ``alpha`` may be ``None`` where their weight is 0."""
    lambdas = (float(lambda_tv), float(lambda_depth_tv), float(lambda_sparsity))
    if not any(lambdas):
        raise ValueError("image_regularizers: every weight is 0, there is nothing to compute")
    require_shape("image", image, ("B", 3, "H", "W"), non_empty=True)
    B, _, H, W = image.shape
    require_shape("depth", depth, (B, 1, H, W), optional=lambdas[1] == 0.0)
    require_shape("alpha", alpha, (B, 1, H, W), (B, H, W), optional=lambdas[2] == 0.0)
    if (lambdas[0] or lambdas[1]) and (H < 2 or W < 2):
        raise ValueError(f"a total-variation term needs H >= 2 and W >= 2, got {H} x {W} (the reference divides by zero)")
    for name, t in (("image", image), ("depth", depth), ("alpha", alpha)):
        if t is not None:
            require_f32_cuda(name, t)
    out = _ImageReg.apply(image, depth, alpha, (B, H, W), lambdas)
    return out[0], out[1].detach(), out[2].detach(), out[3].detach()


class _GaussianReg(torch.autograd.Function):
    """out [4] = (loss, position, scale_sum, opacity_term); an operand whose lambda is 0 is handed to the kernel as NULL."""

    @staticmethod
    def forward(ctx, means, scales, scaling, opacity, shape, lambdas):
        B, N = shape
        l_pos, l_sc, l_op = lambdas
        m = means.detach().contiguous() if l_pos else None
        sc, scales_bs = None, 0
        if l_sc:                                                 # one [N, 3] expanded over the images is read in place, B times
            shared = scales.stride(0) == 0 and scales[0].is_contiguous()
            sc, scales_bs = (scales[0].detach(), 0) if shared else (scales.detach().contiguous(), 3 * N)
        sg, op = (scaling.detach().contiguous(), opacity.detach().contiguous()) if l_op else (None, None)
        dev = next(t for t in (m, sc, sg) if t is not None).device
        out = launch_reduced("a3d_gaussian_reg_f32", dev, (B, N), (_p(m), _p(sc), scales_bs, _p(sg), _p(op), *lambdas), 3,
                             (1, B * N, REG_PAIRS_PER_BLOCK), 4)
        need = ctx.needs_input_grad
        ctx.need = (bool(l_pos) and need[0], bool(l_sc) and need[1], bool(l_op) and need[3])
        if any(ctx.need):
            ctx.save_for_backward(m if ctx.need[0] else None, sg if ctx.need[2] else None)
            ctx.consts = (shape, (l_pos / (1.0 * B * N), l_sc, l_op), opacity.shape if l_op else None, dev)
        return out

    @staticmethod
    def backward(ctx, d_out):
        m, sg = ctx.saved_tensors
        (B, N), coefs, opacity_shape, dev = ctx.consts
        g = _upstream(d_out)
        d_means, d_scales, d_opacity = _empty_grads(ctx.need, ((B, N, 3), (B, N, 3), opacity_shape), dev)
        launch("a3d_gaussian_reg_bwd_f32", dev, B, N, _p(m), _p(sg), *coefs, _p(g), _p(d_means), _p(d_scales), _p(d_opacity))
        return d_means, d_scales, None, d_opacity, None, None


def gaussian_regularizers(means: Optional[torch.Tensor], scales: Optional[torch.Tensor], scaling: Optional[torch.Tensor],
                          opacity: Optional[torch.Tensor], *, lambda_position: float, lambda_scales: float, lambda_opacity: float):
    """(loss, position, scale_sum, opacity_term) of the renderer's unmasked ``means [B, N, 3]`` and activated ``scales [B, N, 3]`` (an
    expanded ``[N, 3]`` is read in place) and the static Gaussians' log-``scaling [N, 3]`` and ``opacity [N, 1]`` / ``[N]``; see the module
    docstring.  An operand whose weight is 0 may be ``None``."""
    lambdas = (float(lambda_position), float(lambda_scales), float(lambda_opacity))
    if not any(lambdas):
        raise ValueError("gaussian_regularizers: every weight is 0, there is nothing to compute")
    given = [("means", means, lambdas[0]), ("scales", scales, lambdas[1]), ("scaling", scaling, lambdas[2]), ("opacity", opacity, lambdas[2])]
    for name, t, lam in given:
        require_shape(name, t, optional=lam == 0.0)              # tensors (or None at weight 0) all four, before any shape is judged
    require_shape("means", means, ("B", "N", 3), non_empty=True, optional=True)
    require_shape("scales", scales, ("B", "N", 3) if means is None else tuple(means.shape), non_empty=True, optional=True)
    per_image = [t for t in (means, scales) if t is not None]
    B, N = per_image[0].shape[:2] if per_image else (1, scaling.shape[0] if scaling.dim() else 0)
    require_shape("scaling", scaling, (N, 3), non_empty=True, optional=True)
    require_shape("opacity", opacity, (N, 1), (N,), optional=True)
    for name, t, _ in given:
        if t is not None:
            require_f32_cuda(name, t)
    out = _GaussianReg.apply(means, scales, scaling, opacity, (B, N), lambdas)
    return out[0], out[1].detach(), out[2].detach(), out[3].detach()


class _TotalInOrder(torch.autograd.Function):
    """``total + terms[0] + terms[1] + ...`` added one at a time in fp32, the reference's ``loss += ...``; the gradient goes to ``total``
    and, unchanged, to the ``carriers``: the differentiable weighted sums of the two regulariser calls, whose terms these are."""

    @staticmethod
    def forward(ctx, total, n_carriers, *rest):
        ctx.counts = (n_carriers, len(rest) - n_carriers)
        value = total.detach()
        for term in rest[n_carriers:]:
            value = value + term
        return value

    @staticmethod
    def backward(ctx, grad):
        return (grad, None, *([grad] * ctx.counts[0]), *([None] * ctx.counts[1]))


# ---- the frame schedule (animate3d.py:134-157)

def sampled_frames(global_step: int, n_frame: int, progressive_iter_per_frame: int, *, do_guidance: bool, strategy: str = "normal",
                   rng=random) -> List[int]:
    """The frames a step reconstructs: 1 .. start_index + 1, where ``start_index`` grows by one every ``progressive_iter_per_frame`` steps
    (all frames at once in a guidance step).  ``"light"`` takes one earlier frame drawn with ``rng.randint(1, start_index)`` plus the
    newest, and every frame once the schedule has reached the last one."""
    start_index = n_frame - 2 if do_guidance else min(global_step // progressive_iter_per_frame, n_frame - 2)
    if strategy == "normal":
        return list(range(1, start_index + 2))
    if strategy == "light":
        if start_index == 0:
            return [1]
        if global_step >= progressive_iter_per_frame * (n_frame - 1):
            return list(range(1, n_frame))
        return [rng.randint(1, start_index), start_index + 1]
    raise NotImplementedError(f"sample_strategy {strategy} not supported")


def sampled_image_index(frames: Sequence[int], n_view: int, n_frame: int, device=None) -> torch.Tensor:
    """int32 ``[n_view * len(frames)]``: ``view * n_frame + frame``, view-major: the ``index`` of ``masked_recon_loss`` and the gather of
    ``c2w``, ``fovy`` and ``timestamps``."""
    return torch.tensor([v * n_frame + f for v in range(n_view) for f in frames], dtype=torch.int32, device=device)


# ---- the renderer (gaussian_batch_renderer_4d.py:11-111, diff_gaussian_rasterizer_advanced_4d.py:60-193)

class Gaussians(NamedTuple):
    """The static Gaussians of the stage: ``xyz [N, 3]`` (a buffer: no gradient), ``scaling [N, 3]`` (log-scale) and ``rotation [N, 4]`` as
    stored, ``opacity [N, 1]`` and ``shs [N, M, 3]`` already activated as ``pc.get_opacity`` / ``pc.get_features`` are, ``sh_degree``."""
    xyz: torch.Tensor
    scaling: torch.Tensor
    rotation: torch.Tensor
    opacity: torch.Tensor
    shs: torch.Tensor
    sh_degree: int


class _KeepMask(torch.autograd.Function):
    """The renderer's random gradient mask (advanced_4d.py:147-154) without its blend.  ``t * keep + t.detach() * (1 - keep)`` with a 0/1
    ``keep`` is ``t`` exactly in the forward (``t * 1 + t * 0`` and ``t * 0 + t * 1``) and passes ``grad * keep`` in the backward: the forward
    returns the three tensors as they are, the backward multiplies the three incoming gradients in place."""

    @staticmethod
    def forward(ctx, keep, *tensors):
        ctx.save_for_backward(keep)
        return tensors

    @staticmethod
    def backward(ctx, *grads):
        (keep,) = ctx.saved_tensors
        return (None, *(None if g is None else g.mul_(keep) for g in grads))


class RenderOutput(dict):
    """``render_batch``'s result.  ``comp_rgb`` (the clamped, permuted ``[B, H, W, 3]`` image) is built on first access: a reconstruction
    step reads ``image`` and never pays for it."""

    def __missing__(self, key):
        if key != "comp_rgb":
            raise KeyError(key)
        self[key] = self["image"].clamp(0, 1).permute(0, 2, 3, 1)
        return self[key]

    def __contains__(self, key):
        return key == "comp_rgb" or super().__contains__(key)


def frames_of_images(timestamps: torch.Tensor):
    """Per-image ``timestamps [B]`` or ``[B, 1]`` -> (the distinct timestamps ``[T]`` ascending, ``image_to_time [B]`` int64): what
    ``deform_gaussians`` takes.  The number of distinct frames depends on the data: this synchronises with the host."""
    ts = timestamps.reshape(-1) if timestamps.dim() == 2 and timestamps.shape[1] == 1 else timestamps
    if ts.dim() != 1:
        raise ValueError(f"timestamps: expected [B] or [B, 1], got {tuple(timestamps.shape)}")
    frames, image_to_time = torch.unique(ts.detach(), sorted=True, return_inverse=True)
    return frames.contiguous(), image_to_time


def render_batch(field: HexPlaneDeformation, gaussians: Gaussians, c2w: Optional[torch.Tensor], fovy: Optional[torch.Tensor],
                 timestamps: Optional[torch.Tensor], height: Optional[int], width: Optional[int], bg, *, do_guidance: bool,
                 first_frame_trainable: bool = False, keep_prob: float = 0.1, generator: Optional[torch.Generator] = None,
                 cameras: Optional[CameraBatch] = None) -> RenderOutput:
    """``Gaussian4DBatchRenderer.batch_forward`` + ``DiffGaussian4D.forward`` for B images in one deformation call and one rasterizer call.

    ``c2w [B, 4, 4]``, ``fovy [B]`` and ``timestamps [B]`` / ``[B, 1]`` are per image, as the data module hands them over; ``bg [3]``.
    The policy (advanced_4d.py:130-162): the scales are deformed only in a guidance step (``deform_scales = do_guidance``); only outside
    one, the gradient reaches the field through a random ``keep_prob`` of the (image, Gaussian) pairs, drawn once per call as
    ``torch.rand(B, N, 1, generator=generator) < keep_prob`` on the device (a guidance step draws nothing); the rasterizer runs outside
    autocast.  Returns ``image [B, 3, H, W]`` (raw), ``comp_rgb [B, H, W, 3]`` (clamped; built on access), ``comp_mask`` / ``comp_depth
    [B, H, W, 1]``, ``radii [B, N]``, ``visibility_filter``, ``means3D`` / ``scales`` / ``rotations [B, N, .]``, the *unmasked* tensors
    (advanced_4d.py:186-188), and ``opacities``.

    ``cameras``: a ``cameras.CameraBatch`` in place of ``c2w`` / ``fovy`` / ``timestamps``, which must then be ``None`` (``ValueError``);
    ``height`` / ``width`` may be ``None`` and must not contradict the batch's.  Its ``w2c``, ``full_proj``, ``campos``, ``tanfov``,
    ``frames`` and ``image_to_time`` go to the field and the rasterizer as they are: no solver call, no ``torch.unique``, and no
    synchronisation with the host before the rasterizer's own."""
    g = gaussians
    if cameras is not None:
        if c2w is not None or fovy is not None or timestamps is not None:
            raise ValueError("cameras= replaces c2w, fovy and timestamps: pass None for all three")
        if (height is not None and int(height) != cameras.height) or (width is not None and int(width) != cameras.width):
            raise ValueError(f"height x width = {height} x {width}, but the cameras were made for {cameras.height} x {cameras.width}")
        frames, image_to_time = cameras.frames, cameras.image_to_time
    else:
        frames, image_to_time = frames_of_images(timestamps)
    plan = {} if cameras is None else dict(image_plan=cameras.image_plan)
    means, scales, rots = field(g.xyz, g.scaling, g.rotation, frames.float(), image_to_time, deform_scales=bool(do_guidance),
                                first_frame_trainable=first_frame_trainable, **plan)
    m_in, s_in, r_in = means, scales, rots
    if not do_guidance:
        keep = (torch.rand(*means.shape[:2], 1, generator=generator, device=means.device) < keep_prob).float()
        m_in, s_in, r_in = _KeepMask.apply(keep, means, scales, rots)
    with torch.autocast("cuda", enabled=False):
        if cameras is not None:
            w2c, proj, cam_p, tan, height, width = cameras.w2c, cameras.full_proj, cameras.campos, cameras.tanfov, cameras.height, cameras.width
        else:
            w2c, proj, cam_p = get_cam_info_gaussian(c2w, fovy, fovy, znear=0.1, zfar=100)
            tan = torch.tan(fovy.float().reshape(-1) / 2)
        image, radii, depth, alpha = rasterize_gaussians(m_in, s_in, r_in, g.opacity, shs=g.shs, viewmatrix=w2c, projmatrix=proj, campos=cam_p,
                                                         tanfovx=tan, tanfovy=tan, image_height=int(height), image_width=int(width), bg=bg,
                                                         sh_degree=g.sh_degree)
    return RenderOutput(image=image, alpha=alpha, comp_mask=alpha.permute(0, 2, 3, 1), comp_depth=depth.permute(0, 2, 3, 1), radii=radii,
                        visibility_filter=radii > 0, means3D=means, scales=scales, rotations=rots, opacities=g.opacity)


# ---- the step (animate3d.py:120-370)

def training_step(field: HexPlaneDeformation, gaussians: Gaussians, batch: Dict, *, loss: Dict[str, float], global_step: int, n_view: int,
                  n_frame: int, progressive_iter_per_frame: int, bg, graph: Optional[Union[ArapGraph, MeshGraph]] = None,
                  guidance: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, sample_strategy: str = "normal",
                  first_frame_trainable: bool = False, keep_prob: float = 0.1, generator: Optional[torch.Generator] = None, rng=random,
                  render: Callable[..., Dict] = render_batch) -> Dict[str, torch.Tensor]:
    """``Animate3DSystem.training_step``: the losses of one step; the caller runs ``out["loss"].backward()`` and the optimiser.

    ``batch``: the data module's resident tensors for all ``n_view * n_frame`` images, view-major (``rgb [., H, W, 3]``, ``mask
    [., H, W, 1]`` bool, or in their place ``rgba8 [., H, W, 4]`` uint8 / a ``frames.FrameSet``, read by ``masked_recon_loss_rgba8``: the
    same bits from 4 bytes a pixel; both or neither is a ``ValueError`` before anything is launched; ``c2w``, ``fovy``, ``timestamps``) and, for a guidance step, ``random_camera`` (``c2w``, ``fovy``, ``timestamps``,
    ``height``, ``width``).  Either may be a ``cameras.CameraBatch`` instead: ``batch["cameras"]`` (``data_view_cameras``) replaces ``c2w`` /
    ``fovy`` / ``timestamps`` of the images, ``batch["random_camera"]`` may be one (``RandomCameraSampler.sample``); ``render`` then gets
    ``cameras=`` and ``None`` for the three tensors, and only then.
    ``guidance``: a ``guidance.AnimateMVGuidance``, or any object with ``takes_batch = True``, is called as the reference calls
    ``self.guidance`` (animate3d.py:196): ``guidance(comp_rgb, batch.get("prompt_utils"), **batch["random_camera"], rgb_as_latents=False,
    generator=generator)["loss_sds"]``, with this step's cameras, a dict or a ``CameraBatch``.  A plain callable is ``comp_rgb [B, H, W, 3]
    -> loss_sds`` (how ``sds.sds_guidance_loss`` is bound) and sees nothing else.  A step with a guidance is the reference's
    ``load_guidance: true``.``loss``: the lambdas under the reference's names (``lambda_rgb``,
    ``lambda_mask``, ``lambda_sds``, ``lambda_arap``, ``arap_sample_num``, for the mesh branch ``arap_K``, and the six regulariser weights
    ``lambda_tv_loss``, ``lambda_depth_tv_loss``, ``lambda_sparsity``, ``lambda_position``, ``lambda_opacity``, ``lambda_scales``); a
    non-zero ``lambda_normal_tv`` raises ``NotImplementedError`` (the reference's renderer never produces ``comp_normal``), a negative
    regulariser weight ``ValueError`` (the reference tests ``> 0.0`` and would drop it silently).  ``bg``: the three background values.  ``render`` is ``render_batch``'s
    stand-in for tests.

    ``graph`` chooses the branch of animate3d.py:222-239.  An ``ArapGraph`` is the k-NN graph of ``xyz``, fixed for the stage.  A
    ``MeshGraph`` is the mesh's connectivity (``connected_vertices_info_path``): every step draws ``arap_K`` of each vertex's neighbours
    with ``graph.sample`` (``graph.Nv`` must be the number of Gaussians and ``loss["arap_K"]`` must be there: ``ValueError``, raised
    before anything touches a device).  Draws from ``generator`` within a step, in the reference's order (:224, then :241): the
    renders' keep-masks, then with a ``MeshGraph`` the sampler's seed (one int64), then ``arap_energy``'s ``sample_idx``.  With an
    ``ArapGraph`` the step draws exactly what it drew before the mesh branch existed.

    In the reference's order: the schedule and the ``(view, frame)`` index; one render of the gathered cameras and the masked RGB / mask
    MSE against ``rgb`` / ``mask`` read through the index; with guidance a render of the random cameras and ``lambda_sds * guidance(comp_rgb)``
    (both renders see the same ``do_guidance``, animate3d.py:131, 188); with ``lambda_arap > 0`` the ARAP energy of the *last* render's
    first ``len(sampled_frames)`` unmasked means (:218); then the regularisers with a non-zero weight, all on the *last* render
    (:256-296): ``gaussian_regularizers`` and ``image_regularizers`` are each called only when one of their weights is non-zero (a step
    with all six at 0 launches, draws and returns exactly what it did without them), and their terms are added to the total one by one
    in the reference's order (position, opacity, sparsity, scales, tv, depth_tv: the fp32 total depends on it).  Returns ``loss`` and,
    detached and times their lambdas, ``loss_rgb``, ``loss_mask``, ``loss_sds``, ``loss_arap``, ``loss_position``, ``loss_opacity``,
    ``loss_sparsity``, ``loss_scales``, ``loss_tv``, ``loss_depth_tv`` (all but the first two only when they are part of the step)."""
    for name in UNSUPPORTED_LAMBDAS:
        if float(loss.get(name, 0.0)) != 0.0:
            raise NotImplementedError(f"{name} = {loss[name]}: zero in every released config, not built")
    reg = {name: float(loss.get(name, 0.0)) for name in IMAGE_REG_LAMBDAS + GAUSSIAN_REG_LAMBDAS}
    for name, value in reg.items():
        if value < 0.0:
            raise ValueError(f"{name} = {value}: the reference tests `> 0.0` and would drop a negative weight without a word")
    do_guidance = guidance is not None
    lambda_arap = float(loss.get("lambda_arap", 0.0))
    if lambda_arap > 0.0 and graph is None:
        raise ValueError("lambda_arap > 0 needs graph=ArapGraph(xyz, K=arap_K, radius=arap_radius) or a MeshGraph")
    if lambda_arap > 0.0 and isinstance(graph, MeshGraph):
        if graph.Nv != gaussians.xyz.shape[0]:
            raise ValueError(f"graph: a mesh of {graph.Nv} vertices for {gaussians.xyz.shape[0]} Gaussians")
        if "arap_K" not in loss:
            raise ValueError("a MeshGraph needs loss['arap_K']: the number of neighbours drawn per vertex and step")
    rgba8 = batch.get("rgba8")
    rgba8 = getattr(rgba8, "rgba8", rgba8)                       # a frames.FrameSet stands for its tensor
    if (rgba8 is not None) == ("rgb" in batch or "mask" in batch):
        raise ValueError("batch: the ground truth is either 'rgba8' (uint8 [., H, W, 4], or a frames.FrameSet) or 'rgb' and 'mask', got "
                         + ("both" if rgba8 is not None else "neither"))
    rgb, mask = (rgba8, None) if rgba8 is not None else (batch["rgb"], batch["mask"])      # rgb: whichever holds the images' shape
    if rgb.shape[0] != n_view * n_frame:
        raise ValueError(f"batch['{'rgb' if rgba8 is None else 'rgba8'}']: expected {n_view * n_frame} images (n_view * n_frame), got {rgb.shape[0]}")
    if reg["lambda_tv_loss"] or reg["lambda_depth_tv_loss"]:      # the last render's size, before anything is rendered
        h, w = (batch["random_camera"]["height"], batch["random_camera"]["width"]) if do_guidance else rgb.shape[1:3]   # dict or CameraBatch
        if h < 2 or w < 2:
            raise ValueError(f"a total-variation term needs H >= 2 and W >= 2, got {h} x {w} (the reference divides by zero)")
    frames = sampled_frames(global_step, n_frame, progressive_iter_per_frame, do_guidance=do_guidance, strategy=sample_strategy, rng=rng)
    index = sampled_image_index(frames, n_view, n_frame, rgb.device)
    gather = index.long()
    common = dict(do_guidance=do_guidance, first_frame_trainable=first_frame_trainable, keep_prob=keep_prob, generator=generator)
    bg0 = float(bg[0])
    if isinstance(batch.get("cameras"), CameraBatch):             # the data views as a CameraBatch: gathered on the host
        taken = batch["cameras"].take([v * n_frame + f for v in range(n_view) for f in frames])
        out = render(field, gaussians, None, None, None, rgb.shape[1], rgb.shape[2], bg, cameras=taken, **common)
    else:
        out = render(field, gaussians, batch["c2w"][gather], batch["fovy"][gather], batch["timestamps"][gather], rgb.shape[1], rgb.shape[2], bg,
                     **common)
    if rgba8 is not None:
        total, loss_rgb, loss_mask = masked_recon_loss_rgba8(out["image"], out["alpha"], rgba8, index, bg=bg0, lambda_rgb=loss["lambda_rgb"],
                                                             lambda_mask=loss["lambda_mask"])
    else:
        total, loss_rgb, loss_mask = masked_recon_loss(out["image"], out["alpha"], rgb, mask, index, bg=bg0, lambda_rgb=loss["lambda_rgb"],
                                                       lambda_mask=loss["lambda_mask"])
    terms = {"loss_rgb": loss_rgb * float(loss["lambda_rgb"]), "loss_mask": loss_mask * float(loss["lambda_mask"])}
    if do_guidance:
        cam = batch["random_camera"]
        if isinstance(cam, CameraBatch):
            out = render(field, gaussians, None, None, None, cam.height, cam.width, bg, cameras=cam, **common)
        else:
            out = render(field, gaussians, cam["c2w"], cam["fovy"], cam["timestamps"], cam["height"], cam["width"], bg, **common)
        if getattr(guidance, "takes_batch", False):               # the guidance object: this step's cameras reach the UNet (animate3d.py:196)
            loss_sds = guidance(out["comp_rgb"], batch.get("prompt_utils"), **cam, rgb_as_latents=False, generator=generator)["loss_sds"]
        else:
            loss_sds = guidance(out["comp_rgb"])
        loss_sds = float(loss["lambda_sds"]) * loss_sds
        total = total + loss_sds
        terms["loss_sds"] = loss_sds.detach()
    if lambda_arap > 0.0:
        if isinstance(graph, MeshGraph):
            nn_idx = graph.sample(int(loss["arap_K"]), generator=generator)
        else:
            nn_idx = graph.refresh(gaussians.xyz).nn_idx
        loss_arap = lambda_arap * arap_energy(gaussians.xyz, out["means3D"][:len(frames)], nn_idx,
                                              sample_num=int(loss.get("arap_sample_num", 512)), generator=generator)
        total = total + loss_arap
        terms["loss_arap"] = loss_arap.detach()
    if any(reg.values()):                                        # animate3d.py:256-296, all on the last render
        carriers, unweighted = [], {}
        if any(reg[name] for name in GAUSSIAN_REG_LAMBDAS):
            carrier, *named = gaussian_regularizers(out["means3D"] if reg["lambda_position"] else None,
                                                    out["scales"] if reg["lambda_scales"] else None,
                                                    gaussians.scaling if reg["lambda_opacity"] else None,
                                                    gaussians.opacity if reg["lambda_opacity"] else None, lambda_position=reg["lambda_position"],
                                                    lambda_scales=reg["lambda_scales"], lambda_opacity=reg["lambda_opacity"])
            carriers.append(carrier)
            unweighted.update(zip(GAUSSIAN_REG_LAMBDAS, named))
        if any(reg[name] for name in IMAGE_REG_LAMBDAS):
            carrier, *named = image_regularizers(out["image"], out["comp_depth"].permute(0, 3, 1, 2) if reg["lambda_depth_tv_loss"] else None,
                                                 out["alpha"] if reg["lambda_sparsity"] else None, lambda_tv=reg["lambda_tv_loss"],
                                                 lambda_depth_tv=reg["lambda_depth_tv_loss"], lambda_sparsity=reg["lambda_sparsity"])
            carriers.append(carrier)
            unweighted.update(zip(IMAGE_REG_LAMBDAS, named))
        for name, key in REG_ORDER:                              # the reference's order: the fp32 total depends on it
            if reg[name]:
                terms[key] = unweighted[name] * reg[name]
        total = _TotalInOrder.apply(total, len(carriers), *carriers, *(terms[key] for name, key in REG_ORDER if reg[name]))
    return {"loss": total, **terms}


def vertex_trajectory(field: HexPlaneDeformation, gaussians: Gaussians, timestamps: torch.Tensor) -> torch.Tensor:
    """The deformed means of every frame, ``[T, N, 3]`` for ``timestamps [T]`` (frame t at ``timestamps[t]``, in the order given), in one
    deformation call without a graph for autograd.  The reference's ``save_gaussian_trajectory`` writes ``mesh_trajectory/{i}.npy`` from
    ``out["means3D"][0]`` of one render per frame (animate3d.py:465-471); row i of this is that array.  The scales are not deformed: the
    means do not depend on them.  No file is written here."""
    require_f32_cuda("timestamps", timestamps)
    if timestamps.dim() != 1:
        raise ValueError(f"timestamps: expected [T], got {tuple(timestamps.shape)}")
    g = gaussians
    with torch.no_grad():
        means, _, _ = field(g.xyz, g.scaling, g.rotation, timestamps.float().contiguous(), None, deform_scales=False)
    return means


def field_param_groups(field: HexPlaneDeformation, *, delta_xyz_network_lr: float, delta_rot_network_lr: float,
                       delta_scaling_network_lr: float, grid_lr: float, global_trans_lr: float = 0.0) -> List[Dict]:
    """The named parameter groups of ``Gaussian4DModel.training_setup`` (gaussian_4d.py:344-391) for
    ``torch.optim.Adam(groups, lr=0.0, eps=1e-15)``: ``delta_xyz_network``, ``delta_rot_network``, ``delta_scaling_network``, ``grid`` and,
    for a field with ``use_global_trans``, ``global_trans`` (both ``global_*`` networks, as the reference's name match takes them).  Every
    released config gives scalar rates; a list-valued one (a schedule) raises ``NotImplementedError``."""
    rates = dict(delta_xyz_network=delta_xyz_network_lr, delta_rot_network=delta_rot_network_lr,
                 delta_scaling_network=delta_scaling_network_lr, grid=grid_lr, global_trans=global_trans_lr)
    for name, lr in rates.items():
        if not isinstance(lr, (int, float)):
            raise NotImplementedError(f"{name}_lr = {lr!r}: only scalar rates are supported (no schedule is built)")
    named = list(field.named_parameters())
    match = dict(delta_xyz_network="delta_xyz", delta_rot_network="delta_rot", delta_scaling_network="delta_scaling", grid="grids.",
                 global_trans="global")
    groups = []
    for name, key in match.items():
        params = [p for n, p in named if (n.startswith(key) if name == "grid" else key in n)]
        if name == "global_trans" and not field.use_global_trans:
            continue
        groups.append({"params": params, "lr": float(rates[name]), "name": name})
    return groups


def fit(field: HexPlaneDeformation, gaussians: Gaussians, batch: Dict, optimizer, *, steps: int, start_step: int = 0, sampler=None,
        generator: Optional[torch.Generator] = None, rng=random, **step_kwargs) -> Dict[str, torch.Tensor]:
    """``steps`` optimisation steps ``s = start_step, start_step + 1, ...`` of ``training_step(field, gaussians, batch, **step_kwargs)``, in
    the reference's order (``forward`` sets the rates before it renders, animate3d.py:116; Lightning steps afterwards).  Each step, on a
    shallow copy of ``batch``:

    1. ``guidance.update_step(0, s)`` where the guidance has that method (``guidance.AnimateMVGuidance``: its timestep range; where
       threestudio updates its ``Updateable`` modules); with a ``sampler`` (``cameras.RandomCameraSampler``): ``sampler.update_step(s)`` and, when ``step_kwargs`` holds a ``guidance``,
       ``batch["random_camera"] = sampler.sample(generator, rng=rng)``;
    2. ``optimizer.update_learning_rate(s)`` where the optimiser has that method (``stage_optim.StageAdam``; any torch optimiser works
       without it);
    3. ``optimizer.zero_grad(set_to_none=True)``;
    4. ``out = training_step(..., global_step=s, generator=generator, rng=rng)``;
    5. ``out["loss"].backward()``;
    6. ``optimizer.step()``.

    Returns one ``[steps]`` fp32 device tensor per term ``training_step`` returned; a term that a step did not return is NaN there.  With
    an optimiser that has a ``skipped`` flag (``StageAdam``) the result also holds ``"skipped"``: 1 where the step was dropped for a
    non-finite gradient.  Logging is device-to-device copies: the loop adds no synchronisation with the host.  Training in segments
    (validate, checkpoint, continue) is another call with the next ``start_step``; there are no callbacks."""
    steps, start_step = int(steps), int(start_step)
    if steps < 1 or start_step < 0:
        raise ValueError(f"fit: steps = {steps}, start_step = {start_step}: expected steps >= 1 and start_step >= 0")
    for name in ("global_step", "generator", "rng"):
        if name in step_kwargs:
            raise TypeError(f"fit: {name} is the loop's to pass")
    update_rates = getattr(optimizer, "update_learning_rate", None)
    skipped = getattr(optimizer, "skipped", None)
    update_guidance = getattr(step_kwargs.get("guidance"), "update_step", None)
    logs: Dict[str, torch.Tensor] = {}

    def log(key, i, value):
        if key not in logs:
            logs[key] = torch.full((steps,), float("nan"), dtype=torch.float32, device=value.device)
        logs[key][i].copy_(value.detach().reshape(()))

    for i in range(steps):
        s = start_step + i
        step_batch = dict(batch)
        if update_guidance is not None:
            update_guidance(0, s)
        if sampler is not None:
            sampler.update_step(s)
            if step_kwargs.get("guidance") is not None:
                step_batch["random_camera"] = sampler.sample(generator, rng=rng)
        if update_rates is not None:
            update_rates(s)
        optimizer.zero_grad(set_to_none=True)
        out = training_step(field, gaussians, step_batch, global_step=s, generator=generator, rng=rng, **step_kwargs)
        out["loss"].backward()
        optimizer.step()
        for key, value in out.items():
            log(key, i, value)
        if skipped is not None:
            log("skipped", i, skipped)
    return logs
