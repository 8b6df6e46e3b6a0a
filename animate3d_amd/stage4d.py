"""One optimisation step of the 4-D stage: the reconstruction branch on the gfx950 kernel of csrc/recon_loss.hip, the renderer's policy and
the step around them.

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
* Summation has no atomics: two calls are bitwise equal.  The backward recomputes from the four inputs (no gradient buffer is kept: at
  60 x 1024^2 it would be 1 GB): ``d_image = g (2 lambda_rgb / n_rgb)(c - y)`` where ``0 <= image <= 1`` and exactly 0 elsewhere (torch's
  clamp rule), ``d_alpha = g (2 lambda_mask / n_mask)(alpha - m)``, in the planar layout the rasterizer's backward reads.  The upstream
  gradient is read on the device: neither direction synchronises with the host.  Without a gradient to compute nothing is saved.

``sampled_frames`` / ``sampled_image_index`` restate the progressive frame schedule (animate3d.py:134-157); ``render_batch`` is the
renderer for a whole batch with the policy of advanced_4d.py:130-162; ``training_step`` is the step, with either ARAP branch (the k-NN
graph or the mesh's connectivity); ``vertex_trajectory`` the deformed means of every frame (``save_gaussian_trajectory``);
``field_param_groups`` the optimiser groups of geometry/gaussian_4d.py:344-391.
"""
from __future__ import annotations

import random
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Union

import torch

from .arap import ArapGraph, MeshGraph, arap_energy
from .deform4d import HexPlaneDeformation
from .f32_stage import launch, require_f32_cuda, require_index_cuda
from .hip_ops import _p
from .splat import get_cam_info_gaussian, rasterize_gaussians

PIXELS_PER_BLOCK = 2048          # RL_PIXELS of csrc/recon_loss.hip: one (rgb, mask) partial per block
UNSUPPORTED_LAMBDAS = ("lambda_tv_loss", "lambda_depth_tv_loss", "lambda_normal_tv", "lambda_position", "lambda_opacity", "lambda_sparsity",
                       "lambda_scales")       # zero in every released config: not built


# ---- the loss kernel

class _MaskedReconLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, alpha, gt_rgb, gt_mask, index, bg, lambda_rgb, lambda_mask):
        B, _, H, W = image.shape
        dev = image.device
        img, alp = image.detach().contiguous(), alpha.detach().contiguous()
        n_partials = B * ((H * W + PIXELS_PER_BLOCK - 1) // PIXELS_PER_BLOCK)
        partials = torch.empty(2, n_partials, dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        launch("a3d_recon_loss_f32", dev, B, H, W, _p(img), _p(alp), _p(gt_rgb), _p(gt_mask), _p(index), bg, lambda_rgb, lambda_mask,
               _p(partials), n_partials, _p(out))
        ctx.need = tuple(ctx.needs_input_grad[:2])
        if any(ctx.need):
            ctx.save_for_backward(img, alp, gt_rgb, gt_mask, index)
            ctx.consts = (bg, 2.0 * lambda_rgb / (3.0 * B * H * W), 2.0 * lambda_mask / (1.0 * B * H * W), alpha.shape)
        return out

    @staticmethod
    def backward(ctx, d_out):
        img, alp, gt_rgb, gt_mask, index = ctx.saved_tensors
        bg, coef_rgb, coef_mask, alpha_shape = ctx.consts
        B, _, H, W = img.shape
        g = d_out.detach().float().contiguous()                  # g[0]: the gradient of `loss`; read on the device
        d_image = torch.empty_like(img) if ctx.need[0] else None
        d_alpha = torch.empty(alpha_shape, dtype=torch.float32, device=img.device) if ctx.need[1] else None
        launch("a3d_recon_loss_bwd_f32", img.device, B, H, W, _p(img), _p(alp), _p(gt_rgb), _p(gt_mask), _p(index), bg, coef_rgb, coef_mask,
               _p(g), _p(d_image), _p(d_alpha))
        return d_image, d_alpha, None, None, None, None, None, None


def masked_recon_loss(image: torch.Tensor, alpha: torch.Tensor, gt_rgb: torch.Tensor, gt_mask: torch.Tensor, index=None, *, bg: float,
                      lambda_rgb: float, lambda_mask: float):
    """(loss, loss_rgb, loss_mask) of the renders ``image`` / ``alpha`` against frames ``index`` of ``gt_rgb`` / ``gt_mask``; see the module
    docstring.  A device ``index`` is not range-checked: the caller owns its range."""
    if not isinstance(gt_mask, torch.Tensor) or gt_mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"gt_mask: expected a bool or uint8 tensor, got {getattr(gt_mask, 'dtype', type(gt_mask))} (the tracked masks are "
                        "two-valued; threshold a soft mask first)")
    for name, t in (("image", image), ("alpha", alpha), ("gt_rgb", gt_rgb)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if image.dim() != 4 or image.shape[1] != 3 or 0 in image.shape:
        raise ValueError(f"image: expected a non-empty [B, 3, H, W], got {tuple(image.shape)}")
    B, _, H, W = image.shape
    if tuple(alpha.shape) not in ((B, 1, H, W), (B, H, W)):
        raise ValueError(f"alpha: expected {(B, 1, H, W)} or {(B, H, W)}, got {tuple(alpha.shape)}")
    if gt_rgb.dim() != 4 or tuple(gt_rgb.shape[1:]) != (H, W, 3):
        raise ValueError(f"gt_rgb: expected [S, {H}, {W}, 3], got {tuple(gt_rgb.shape)}")
    S = gt_rgb.shape[0]
    if tuple(gt_mask.shape) not in ((S, H, W, 1), (S, H, W)):
        raise ValueError(f"gt_mask: expected {(S, H, W, 1)} or {(S, H, W)}, got {tuple(gt_mask.shape)}")
    if index is None and S != B:
        raise ValueError(f"index=None compares image b with frame b: needs S == B, got S = {S}, B = {B}")
    require_f32_cuda("image", image)
    require_f32_cuda("alpha", alpha)
    require_f32_cuda("gt_rgb", gt_rgb)
    if not gt_mask.is_cuda:
        raise RuntimeError("gt_mask: expected a CUDA tensor (no CPU fallback)")
    if gt_rgb.requires_grad:
        raise NotImplementedError("gt_rgb.requires_grad: the ground truth is data")
    dev = image.device
    if index is not None:
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
        index = index.to(torch.int32).contiguous()
    gt = gt_rgb.detach().contiguous()                            # the data module's tensors are contiguous: no copy
    mask = gt_mask.contiguous()
    mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    out = _MaskedReconLoss.apply(image, alpha, gt, mask, index, float(bg), float(lambda_rgb), float(lambda_mask))
    return out[0], out[1].detach(), out[2].detach()


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


def render_batch(field: HexPlaneDeformation, gaussians: Gaussians, c2w: torch.Tensor, fovy: torch.Tensor, timestamps: torch.Tensor,
                 height: int, width: int, bg, *, do_guidance: bool, first_frame_trainable: bool = False, keep_prob: float = 0.1,
                 generator: Optional[torch.Generator] = None) -> RenderOutput:
    """``Gaussian4DBatchRenderer.batch_forward`` + ``DiffGaussian4D.forward`` for B images in one deformation call and one rasterizer call.

    ``c2w [B, 4, 4]``, ``fovy [B]`` and ``timestamps [B]`` / ``[B, 1]`` are per image, as the data module hands them over; ``bg [3]``.
    The policy (advanced_4d.py:130-162): the scales are deformed only in a guidance step (``deform_scales = do_guidance``); only outside
    one, the gradient reaches the field through a random ``keep_prob`` of the (image, Gaussian) pairs, drawn once per call as
    ``torch.rand(B, N, 1, generator=generator) < keep_prob`` on the device (a guidance step draws nothing); the rasterizer runs outside
    autocast.  Returns ``image [B, 3, H, W]`` (raw), ``comp_rgb [B, H, W, 3]`` (clamped; built on access), ``comp_mask`` / ``comp_depth
    [B, H, W, 1]``, ``radii [B, N]``, ``visibility_filter``, ``means3D`` / ``scales`` / ``rotations [B, N, .]``, the *unmasked* tensors
    (advanced_4d.py:186-188), and ``opacities``."""
    g = gaussians
    frames, image_to_time = frames_of_images(timestamps)
    means, scales, rots = field(g.xyz, g.scaling, g.rotation, frames.float(), image_to_time, deform_scales=bool(do_guidance),
                                first_frame_trainable=first_frame_trainable)
    m_in, s_in, r_in = means, scales, rots
    if not do_guidance:
        keep = (torch.rand(*means.shape[:2], 1, generator=generator, device=means.device) < keep_prob).float()
        m_in, s_in, r_in = _KeepMask.apply(keep, means, scales, rots)
    with torch.autocast("cuda", enabled=False):
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
    [., H, W, 1]`` bool, ``c2w``, ``fovy``, ``timestamps``) and, for a guidance step, ``random_camera`` (``c2w``, ``fovy``, ``timestamps``,
    ``height``, ``width``).  ``guidance``: ``comp_rgb [B, H, W, 3] -> loss_sds`` (how ``sds.sds_guidance_loss`` is bound); a step with a
    guidance callable is the reference's ``load_guidance: true``.  ``loss``: the lambdas under the reference's names (``lambda_rgb``,
    ``lambda_mask``, ``lambda_sds``, ``lambda_arap``, ``arap_sample_num`` and, for the mesh branch, ``arap_K``); a non-zero value for one
    this module does not build raises ``NotImplementedError``.  ``bg``: the three background values.  ``render`` is ``render_batch``'s
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
    first ``len(sampled_frames)`` unmasked means (:218).  Returns ``loss`` and, detached and times their lambdas as the reference logs
    them, ``loss_rgb``, ``loss_mask``, ``loss_sds``, ``loss_arap`` (the last two only when they are part of the step)."""
    for name in UNSUPPORTED_LAMBDAS:
        if float(loss.get(name, 0.0)) != 0.0:
            raise NotImplementedError(f"{name} = {loss[name]}: zero in every released config, not built")
    do_guidance = guidance is not None
    lambda_arap = float(loss.get("lambda_arap", 0.0))
    if lambda_arap > 0.0 and graph is None:
        raise ValueError("lambda_arap > 0 needs graph=ArapGraph(xyz, K=arap_K, radius=arap_radius) or a MeshGraph")
    if lambda_arap > 0.0 and isinstance(graph, MeshGraph):
        if graph.Nv != gaussians.xyz.shape[0]:
            raise ValueError(f"graph: a mesh of {graph.Nv} vertices for {gaussians.xyz.shape[0]} Gaussians")
        if "arap_K" not in loss:
            raise ValueError("a MeshGraph needs loss['arap_K']: the number of neighbours drawn per vertex and step")
    rgb, mask = batch["rgb"], batch["mask"]
    if rgb.shape[0] != n_view * n_frame:
        raise ValueError(f"batch['rgb']: expected {n_view * n_frame} images (n_view * n_frame), got {rgb.shape[0]}")
    frames = sampled_frames(global_step, n_frame, progressive_iter_per_frame, do_guidance=do_guidance, strategy=sample_strategy, rng=rng)
    index = sampled_image_index(frames, n_view, n_frame, rgb.device)
    gather = index.long()
    common = dict(do_guidance=do_guidance, first_frame_trainable=first_frame_trainable, keep_prob=keep_prob, generator=generator)
    bg0 = float(bg[0])
    out = render(field, gaussians, batch["c2w"][gather], batch["fovy"][gather], batch["timestamps"][gather], rgb.shape[1], rgb.shape[2], bg,
                 **common)
    total, loss_rgb, loss_mask = masked_recon_loss(out["image"], out["alpha"], rgb, mask, index, bg=bg0, lambda_rgb=loss["lambda_rgb"],
                                                   lambda_mask=loss["lambda_mask"])
    terms = {"loss_rgb": loss_rgb * float(loss["lambda_rgb"]), "loss_mask": loss_mask * float(loss["lambda_mask"])}
    if do_guidance:
        cam = batch["random_camera"]
        out = render(field, gaussians, cam["c2w"], cam["fovy"], cam["timestamps"], cam["height"], cam["width"], bg, **common)
        loss_sds = float(loss["lambda_sds"]) * guidance(out["comp_rgb"])
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
