"""The 4D-SDS step around the UNet — SURVEY.md §8(c) "Python caller rows" / §8(f) item 3 (SDS-side glue).

Host-side mirror of ``AnimateMVDiffusionGuidance.compute_mvdream_recon_loss``
(custom/threestudio-animate3d/guidance/animatemv_guidance.py:391-507) for one optimisation step of the 4-D representation:

    latents [(b n f), 4, h, w]  (rendered + VAE-encoded, requires grad)
      -> keep frame 0 clean, diffuse frames 1.. to t                                   :415-430
      -> ONE UNet forward on the CFG-doubled batch in (text, uncond) order              :433-448   (pipeline uses (uncond, text))
      -> eps = eps_text + s * (eps_text - eps_uncond)                                   :451-459   (NOT uncond + s * (...))
      -> x0 reconstruction, optional std rescale against the un-guided reconstruction   :465-488
      -> frame 0 of the target := the input's frame 0; loss = 0.5 * SSE / N * f/(f-1)    :491-503

Everything outside the UNet call is element-wise work on a [(b n f), 4, 32, 32] tensor: torch ops, differentiable w.r.t.
``latents`` exactly where the reference's are (the target is detached).  The scheduler methods the reference calls
(diffusers ``DDIMScheduler.add_noise`` / ``.step(...).pred_original_sample``, third-party) reduce to the two closed forms
below with ``alphas_cumprod`` from ``denoise.ddim_schedule``.  For b > 1 the reference indexes ``alphas_cumprod[t]`` with t of
shape [b] and broadcasts it against ``(b n f) c h w`` (only well-formed for b = 1, its default); here alpha is applied per b.

``sds_recon_loss`` is that chain in torch ops.  ``sds_recon_loss_fused`` is the same step with the chain in the kernels of csrc/sds_glue.hip,
one ``torch.autograd.Function`` around the UNet call (CUDA tensors only, no torch fallback).  The quantities, with ``a = alphas_cumprod[t[b]]``
in fp32, ``sa = sqrt(a)``, ``s1 = sqrt(1 - a)``, ``s`` the guidance scale and ``r = recon_std_rescale``:

    noisy      = frame 0 ? latents : sa latents + s1 noise                      (latents_noisy; the UNet's sample, "(b n) c f h w", twice)
    eps_cfg    = eps_text + s (eps_text - eps_uncond)                            (noise_pred)
    x0(e)      = (noisy - s1 e) / sa
    factor[b]  = (std x0(eps_text) + 1e-8) / (std x0(eps_cfg) + 1e-8)            (unbiased std over frames 1.. of b: n (f - 1) c h w values)
    recon      = frame 0 ? latents : (r != 0 ? r x0(eps_cfg) factor + (1 - r) x0(eps_cfg) : x0(eps_cfg))        (latents_recon)
    loss       = 0.5 sum (latents - recon)^2 / (b n f) * f / (f - 1)
    d latents  = frame 0 ? 0 : (latents - recon) f / ((f - 1) b n f) * upstream

Launches: pack (1), epilogue (statistics, reconstruction + loss partials, final sum: 3, or 2 with r = 0), backward (1).  The tensors
are fp32 arithmetic that rounds where the torch ops round (bit for bit what ``sds_recon_loss`` returns, up to the factor's last bit).  The
statistics and the loss are formed in fp64 from ``latents``, ``noise`` and ``eps``: the statistics in two passes per block, merged
pairwise, never as a difference of sums; the loss's block sums through the fixed tree of csrc/loss_reduce.h in fp64, kept as fp32
(hi, lo) pairs and added by one block in fp64, so the scalar carries one rounding.  No atomics, two calls are bitwise equal, row b does
not depend on the rest of the batch, nothing synchronises with the host.  The UNet boundary (sample, timestep, eps) is
``weights_dtype``: float16, bfloat16, or float32 for a UNet run in fp32.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from .denoise import ddim_schedule, randn_like_reference
from .f32_stage import launch, launch_reduced, require_f32_cuda, require_index_cuda
from .hip_ops import _DTYPE_CODE, _p

GLUE_ITEMS_PER_BLOCK = 2048      # SG_ITEMS of csrc/sds_glue.hip: one loss partial, and one set of statistics, per block


def normalize_camera(c2w: torch.Tensor) -> torch.Tensor:
    """[B, 4, 4] camera-to-world -> [B, 16] with the translation on the unit sphere (pipeline.py:176-190, called by
    ``get_camera_cond``, animatemv_guidance.py:345-358, ``camera_condition_type == "rotation"``)."""
    m = c2w.reshape(-1, 4, 4).clone()
    tr = m[:, :3, 3]
    m[:, :3, 3] = tr / (torch.norm(tr, dim=1, keepdim=True) + 1e-8)
    return m.reshape(-1, 16)


def sds_recon_loss(unet, latents: torch.Tensor, t: torch.Tensor, text_embeddings: torch.Tensor, image_embeds: torch.Tensor,
                   c2w: Optional[torch.Tensor] = None, *, n_view: int = 4, n_frame: int = 8, guidance_scale: float = 100.0,
                   recon_std_rescale: float = 0.5, i2v_cond_time_zero: bool = False, alphas_cumprod: Optional[torch.Tensor] = None,
                   noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                   weights_dtype: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """One SDS reconstruction step.  ``latents`` [(b n f), 4, h, w]; ``t`` [b] long; ``text_embeddings`` [2 b n, L, D] in
    (text, uncond) order; ``image_embeds`` [b n, E] (the unconditional half is zeros, :439); ``c2w`` [(b n f), 4, 4] or None.
    Returns (loss, {"latents_noisy", "noise_pred", "latents_recon"}) like the reference's ``guidance_eval_utils``."""
    n, f = n_view, n_frame
    if latents.shape[0] % (n * f) != 0:
        raise ValueError(f"latents batch {latents.shape[0]} is not a multiple of n_view * n_frame = {n * f}")
    if f < 2:
        raise ValueError("n_frame must be >= 2 (frame 0 is the clean conditioning frame)")
    b = latents.shape[0] // (n * f)
    c, h, w = latents.shape[1:]
    if t.shape != (b,):
        raise ValueError(f"t must have shape [{b}]")
    if text_embeddings.shape[0] != 2 * b * n or image_embeds.shape[0] != b * n:
        raise ValueError("text_embeddings needs 2*b*n rows ((text, uncond) order), image_embeds b*n rows")
    if alphas_cumprod is None:
        alphas_cumprod = ddim_schedule(1)[1].float()
    acp = alphas_cumprod.to(device=latents.device, dtype=latents.dtype)[t.to(latents.device)]        # [b]
    wd = weights_dtype or latents.dtype

    videos = latents.reshape(b, n, f, c, h, w)
    with torch.no_grad():
        rest = videos[:, :, 1:]
        if noise is None:
            noise = randn_like_reference(rest.shape, generator, latents.device, latents.dtype)
        else:                                               # the reference draws it in "b n c f h w" order; accept that layout too
            noise = noise.to(latents)
            if noise.shape == (b, n, c, f - 1, h, w):
                noise = noise.permute(0, 1, 3, 2, 4, 5)
        a6 = acp.reshape(b, 1, 1, 1, 1, 1)
        noisy = torch.cat([videos[:, :, :1], a6.sqrt() * rest + (1 - a6).sqrt() * noise], dim=2)        # b n f c h w
        sample = noisy.permute(0, 1, 3, 2, 4, 5).reshape(b * n, c, f, h, w)                              # (b n) c f h w
        ts = t.reshape(b, 1).expand(b, n).reshape(-1)
        camera = None
        if c2w is not None:
            cam = normalize_camera(c2w.reshape(b, n, f, 4, 4)[:, :, 0].reshape(b * n, 4, 4)).to(latents.dtype)
            camera = torch.cat([cam, cam]).to(wd)
        embeds = torch.cat([image_embeds, torch.zeros_like(image_embeds)]).to(wd)
        eps = unet(torch.cat([sample, sample]).to(wd), torch.cat([ts, ts]).to(wd), encoder_hidden_states=text_embeddings.to(wd),
                   camera=camera, added_cond_kwargs={"image_embeds": embeds}, i2v_cond_time_zero=i2v_cond_time_zero).sample.to(latents.dtype)
        frames = lambda e: e.permute(0, 2, 1, 3, 4).reshape(b * n * f, c, h, w)                          # (b n) c f h w -> (b n f) c h w
        eps_text, eps_uncond = eps.chunk(2)
        eps_text, eps_uncond = frames(eps_text), frames(eps_uncond)
        eps_cfg = eps_text + guidance_scale * (eps_text - eps_uncond)
        noisy_flat = noisy.reshape(b * n * f, c, h, w)
        a4 = acp.repeat_interleave(n * f).reshape(-1, 1, 1, 1)
        x0 = lambda e: (noisy_flat - (1 - a4).sqrt() * e) / a4.sqrt()
        recon = x0(eps_cfg)
        if recon_std_rescale > 0:
            rest_std = lambda z: z.reshape(b, n, f, c, h, w)[:, :, 1:].std(dim=[1, 2, 3, 4, 5], keepdim=True)   # frames 1.., per b
            factor = (rest_std(x0(eps_text)) + 1e-8) / (rest_std(recon) + 1e-8)
            adjusted = recon * factor.reshape(b).repeat_interleave(n * f).reshape(-1, 1, 1, 1)
            recon = recon_std_rescale * adjusted + (1 - recon_std_rescale) * recon
        recon = recon.reshape(b * n, f, c, h, w)
        recon = torch.cat([videos.detach().reshape(b * n, f, c, h, w)[:, :1], recon[:, 1:]], dim=1).reshape(b * n * f, c, h, w)
    loss = 0.5 * ((latents - recon) ** 2).sum() / latents.shape[0] * f / (f - 1)
    return loss, {"latents_noisy": noisy_flat, "noise_pred": eps_cfg, "latents_recon": recon}


class _SdsReconFused(torch.autograd.Function):
    """(loss, latents_noisy, noise_pred or None, latents_recon) = the step around ``call_unet(sample, timestep) -> eps``; see the module
    docstring.  ``dims = (b, n, f, c, h, w)``; ``t`` int64 ``[b]`` and ``table`` fp32 on the device."""

    @staticmethod
    def forward(ctx, latents, call_unet, t, table, noise, dims, guidance_scale, recon_std_rescale, wd, want_noise_pred):
        b, n, f, c, h, w = dims
        dev, sizes = latents.device, (b, n, f, c, h * w)
        suffix, code = ("_f16" if wd == torch.float16 else "_bf16"), _DTYPE_CODE[wd]
        lat = latents.detach().contiguous()
        noisy = torch.empty_like(lat)
        sample = torch.empty(2 * b * n, c, f, h, w, dtype=wd, device=dev)
        timestep = torch.empty(2 * b * n, dtype=wd, device=dev)
        launch("a3d_sds_pack" + suffix, dev, *sizes, _p(lat), _p(noise), _p(t), _p(table), table.numel(), code, _p(noisy), _p(sample),
               _p(timestep))
        eps = call_unet(sample, timestep)
        if tuple(eps.shape) != tuple(sample.shape):
            raise ValueError(f"the UNet returned {tuple(eps.shape)} for a sample of {tuple(sample.shape)}")
        eps = eps.detach().to(wd).contiguous()
        recon = torch.empty_like(lat)
        noise_pred = torch.empty_like(lat) if want_noise_pred else None
        stats = None
        if recon_std_rescale != 0.0:
            rest = n * (f - 1) * c * h * w
            stats = torch.empty(b, (rest + GLUE_ITEMS_PER_BLOCK - 1) // GLUE_ITEMS_PER_BLOCK, 4, dtype=torch.float64, device=dev)
        out = launch_reduced("a3d_sds_epilogue" + suffix, dev, sizes,
                             (_p(eps), code, _p(noisy), _p(lat), _p(noise), _p(t), _p(table), table.numel(), guidance_scale, recon_std_rescale,
                              _p(stats), 0 if stats is None else stats.numel(), _p(recon), _p(noise_pred)), 2,
                             (b, n * f * c * h * w, GLUE_ITEMS_PER_BLOCK), 1)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(lat, recon)
            ctx.sizes, ctx.shape = sizes, latents.shape
        aux = [x for x in (noisy, noise_pred, recon) if x is not None]
        ctx.mark_non_differentiable(*aux)
        return out.reshape(()), noisy, noise_pred, recon

    @staticmethod
    def backward(ctx, d_loss, *_):
        lat, recon = ctx.saved_tensors
        b, n, f = ctx.sizes[:3]
        g = d_loss.detach().float().contiguous()             # read on the device, as stage4d._upstream
        grad = torch.empty_like(lat)
        launch("a3d_sds_epilogue_bwd_f32", lat.device, *ctx.sizes, _p(lat), _p(recon), f / ((f - 1.0) * b * n * f), _p(g), _p(grad))
        return (grad.reshape(ctx.shape), *([None] * 9))


def _table_on(alphas_cumprod: Optional[torch.Tensor], device) -> torch.Tensor:
    if alphas_cumprod is None:
        alphas_cumprod = ddim_schedule(1)[1]
    return alphas_cumprod.to(device=device, dtype=torch.float32).contiguous()


def _fused_step(unet, latents, t, text_embeddings, image_embeds, c2w, *, n_view, n_frame, guidance_scale, recon_std_rescale,
                i2v_cond_time_zero, table, noise, generator, weights_dtype, want_noise_pred):
    """``sds_recon_loss_fused`` behind its argument handling; ``table``: alphas_cumprod, fp32 on the latents' device."""
    n, f = n_view, n_frame
    require_f32_cuda("latents", latents)
    if latents.dim() != 4:
        raise ValueError(f"latents: expected [(b n f), c, h, w], got {tuple(latents.shape)}")
    if latents.shape[0] % (n * f) != 0:
        raise ValueError(f"latents batch {latents.shape[0]} is not a multiple of n_view * n_frame = {n * f}")
    if f < 2:
        raise ValueError("n_frame must be >= 2 (frame 0 is the clean conditioning frame)")
    b = latents.shape[0] // (n * f)
    c, h, w = latents.shape[1:]
    require_index_cuda("t", t)
    if t.shape != (b,):
        raise ValueError(f"t must have shape [{b}]")
    if text_embeddings.shape[0] != 2 * b * n or image_embeds.shape[0] != b * n:
        raise ValueError("text_embeddings needs 2*b*n rows ((text, uncond) order), image_embeds b*n rows")
    wd = weights_dtype or latents.dtype
    if wd not in _DTYPE_CODE:
        raise ValueError(f"weights_dtype {wd}: the UNet boundary is float16, bfloat16 or float32")
    dev = latents.device
    if noise is None:
        noise = randn_like_reference((b, n, f - 1, c, h, w), generator, dev, torch.float32)
    else:
        require_f32_cuda("noise", noise)
        if noise.shape == (b, n, c, f - 1, h, w):                          # the reference's "b n c f h w" order, as sds_recon_loss takes it
            noise = noise.permute(0, 1, 3, 2, 4, 5)
        if noise.shape != (b, n, f - 1, c, h, w):
            raise ValueError(f"noise: expected {[b, n, f - 1, c, h, w]}, got {list(noise.shape)}")
    noise = noise.detach().contiguous()
    camera = None
    if c2w is not None:
        cam = normalize_camera(c2w.reshape(b, n, f, 4, 4)[:, :, 0].reshape(b * n, 4, 4)).to(latents.dtype)
        camera = torch.cat([cam, cam]).to(wd)
    embeds = torch.cat([image_embeds, torch.zeros_like(image_embeds)]).to(wd)
    text = text_embeddings.to(wd)

    def call_unet(sample, timestep):
        return unet(sample, timestep, encoder_hidden_states=text, camera=camera, added_cond_kwargs={"image_embeds": embeds},
                    i2v_cond_time_zero=i2v_cond_time_zero).sample

    return _SdsReconFused.apply(latents, call_unet, t.to(torch.int64).contiguous(), table, noise, (b, n, f, c, h, w), float(guidance_scale),
                                float(recon_std_rescale), wd, want_noise_pred)


def sds_recon_loss_fused(unet, latents: torch.Tensor, t: torch.Tensor, text_embeddings: torch.Tensor, image_embeds: torch.Tensor,
                         c2w: Optional[torch.Tensor] = None, *, n_view: int = 4, n_frame: int = 8, guidance_scale: float = 100.0,
                         recon_std_rescale: float = 0.5, i2v_cond_time_zero: bool = False, alphas_cumprod: Optional[torch.Tensor] = None,
                         noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                         weights_dtype: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``sds_recon_loss`` with the chain around the UNet call in the kernels of csrc/sds_glue.hip: the same arguments, the same
    ``(loss, {"latents_noisy", "noise_pred", "latents_recon"})``; see the module docstring.  ``latents`` fp32 and ``t`` on a CUDA device
    (a CPU tensor raises: there is no torch fallback); ``noise``, where given, as well.  An ``alphas_cumprod`` that is not an fp32 tensor
    on that device already is copied there (the one copy a caller can hoist; ``AnimateMVGuidance`` does).  ``t`` is not range-checked on
    the host: the kernels clamp it into the table.  With ``recon_std_rescale`` of 0 the statistics are skipped."""
    loss, noisy, noise_pred, recon = _fused_step(
        unet, latents, t, text_embeddings, image_embeds, c2w, n_view=n_view, n_frame=n_frame, guidance_scale=guidance_scale,
        recon_std_rescale=recon_std_rescale, i2v_cond_time_zero=i2v_cond_time_zero, table=_table_on(alphas_cumprod, latents.device),
        noise=noise, generator=generator, weights_dtype=weights_dtype, want_noise_pred=True)
    return loss, {"latents_noisy": noisy, "noise_pred": noise_pred, "latents_recon": recon}


def first_frame_index(b: int, n_view: int, n_frame: int, device) -> torch.Tensor:
    """The positions of frame 0 of every (b, view) video in a ``(b n f)`` batch: ``arange(b * n_view) * n_frame``, int32 on ``device``
    (``rearrange(x, "(b f) c h w -> b f c h w", f=n_frame)[:, 0]``, animatemv_guidance.py:547)."""
    return torch.arange(b * n_view, device=device, dtype=torch.int32) * n_frame


def sds_guidance_loss(vae, unet, rgb: torch.Tensor, t: torch.Tensor, text_embeddings: torch.Tensor, image_embeds: Optional[torch.Tensor],
                      c2w: Optional[torch.Tensor], *, rgb_as_latents: bool = False, vae_generator: Optional[torch.Generator] = None,
                      vae_noise: Optional[torch.Tensor] = None, image_encoder=None, **sds_kw) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``AnimateMVDiffusionGuidance.__call__`` (animatemv_guidance.py:509-560) from the rendered frames to the loss.  ``rgb`` [(b n f), H, W, 3]
    in [0, 1] -> bilinear resize to 256^2 (align_corners=False, :532-535) -> ``vae.encode_images`` (an ``AutoencoderKLEncoder``, :536-543) ->
    ``sds_recon_loss``.  With ``rgb_as_latents`` (``rgb`` then has the 4 latent channels) the resize goes to 32^2 and the result is taken as
    the latents (:537-540).  ``vae_generator`` / ``vae_noise``: the posterior sample's noise.

    The CLIP image condition (:546-555): pass ``image_embeds`` [b n, E], or pass None and ``image_encoder`` (a
    ``clip.CLIPVisionEncoderWithProjection``): the embeddings then come from frame 0 of every video of ``rgb.detach()``, at the rendered
    size, through ``clip.encode_image_from_frames`` (the reference's host copy, PIL and ``CLIPImageProcessor``, on the GPU and bit-equal).
    Passing neither raises.

    Returns (loss, aux) as ``sds_recon_loss`` does, with aux["latents"] the encoded latents; ``loss.backward()`` fills ``rgb.grad`` through
    the encoder's input gradient."""
    if image_embeds is None:
        if image_encoder is None:
            raise ValueError("sds_guidance_loss needs image_embeds or image_encoder")
        from .clip import encode_image_from_frames
        n, f = sds_kw.get("n_view", 4), sds_kw.get("n_frame", 8)
        if rgb.shape[0] % (n * f) != 0:
            raise ValueError(f"rgb batch {rgb.shape[0]} is not a multiple of n_view * n_frame = {n * f}")
        first = first_frame_index(rgb.shape[0] // (n * f), n, f, rgb.device)
        image_embeds = encode_image_from_frames(image_encoder, rgb.detach(), first)[0]
    x = rgb.permute(0, 3, 1, 2)
    if rgb_as_latents:
        latents = F.interpolate(x, (32, 32), mode="bilinear", align_corners=False)
    else:
        latents = vae.encode_images(F.interpolate(x, (256, 256), mode="bilinear", align_corners=False), generator=vae_generator, noise=vae_noise)
    loss, aux = sds_recon_loss(unet, latents, t.to(latents.device), text_embeddings, image_embeds, c2w, **sds_kw)
    aux["latents"] = latents
    return loss, aux
