"""The 4D-SDS guidance object of the refine stage: what stands where ``self.guidance`` stands in ``Animate3DSystem.training_step``.

``AnimateMVGuidance`` has the call surface of the reference's ``AnimateMVDiffusionGuidance``
(custom/threestudio-animate3d/guidance/animatemv_guidance.py) over the package's own models: an ``AutoencoderKLEncoder``, the drop-in UNet
(or any callable with its signature) and a ``clip.CLIPVisionEncoderWithProjection``.  A call is ``__call__`` + ``compute_mvdream_recon_loss``
(:391-560):

    rgb [(b n f), H, W, 3] in [0, 1] -> bilinear 256^2 -> vae.encode_images (posterior sample)        :532-543
      -> CLIP image embeddings of frame 0 of every (b, view), from rgb.detach()                       :546-555
      -> t ~ randint(min_step, max_step + 1), one per b                                               :558-565
      -> text embeddings for the frame-0 (elevation, azimuth, camera_distances) per (b, view)          :411-413
      -> the camera condition normalize_camera(c2w of frame 0) per (b, view), "rotation" only          :436-438, 345-358
      -> the reconstruction loss around one UNet call (sds.py)                                        :415-503
      -> {"loss_sds", "min_step", "max_step"}                                                         :588-593

Random draws come from ``generator`` in the reference's order: the VAE posterior noise, then ``t``, then the diffusion noise.  ``t`` is
drawn on the device from the host-side integer bounds and ``alphas_cumprod[t]`` is gathered there by the kernels (``fused=True``) or by
an index (``fused=False``): a call adds no synchronisation with the host.  A CPU generator draws on the CPU and copies, as diffusers'
``randn_tensor`` does; pass a device generator to draw in place.

The timestep range is the object's: ``set_min_max_steps`` is :323-325 (``int(num_train_timesteps * percent)``: it truncates, which shows on the
interpolated values of a list schedule), ``update_step`` :767-793 with ``stage_optim.scheduled`` for threestudio's ``C`` (``min_step_percent`` / ``max_step_percent`` a
number or a list, ``sqrt_anneal`` with ``trainer_max_steps``).  ``stage4d.fit`` calls ``update_step(0, s)`` at the start of step ``s``.

``fused=True`` (the default) runs the glue on the kernels of csrc/sds_glue.hip (``sds.sds_recon_loss_fused``), ``fused=False`` on the torch
chain (``sds.sds_recon_loss``); both give the same quantities.  ``stage4d.training_step`` recognises the object by ``takes_batch`` and
hands it ``prompt_utils`` and this step's ``batch["random_camera"]``.

No tokenizer or prompt processor is built: ``prompt_utils`` is any object with the reference's
``get_text_embeddings(elevation, azimuth, camera_distances, view_dependent_prompting) -> [2 b n, L, D]`` in (text, uncond) order
(threestudio's ``PromptProcessorOutput``), or ``None`` with a ``(text, uncond)`` pair of ``[L, D]`` / ``[1, L, D]`` embeddings given at
construction.  ``grad_clip``, ``token_merging``, ``guidance_eval=True`` and ``recon_loss=False`` raise ``NotImplementedError``: no released
config uses them.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from . import sds
from .denoise import ddim_schedule
from .stage_optim import scheduled

Percent = Union[int, float, Sequence]


class AnimateMVGuidance:
    takes_batch = True           # stage4d.training_step: call with prompt_utils and **batch["random_camera"]

    def __init__(self, vae, unet, image_encoder=None, *, text_embeddings: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                 n_view: int = 4, n_frame: int = 8, guidance_scale: float = 100.0, recon_std_rescale: float = 0.5,
                 min_step_percent: Percent = 0.02, max_step_percent: Percent = 0.98, sqrt_anneal: bool = False,
                 trainer_max_steps: int = 25000, i2v_cond_time_zero: bool = False, half_precision_weights: bool = True,
                 weights_dtype: Optional[torch.dtype] = None, num_train_timesteps: int = 1000, beta_start: float = 0.00085,
                 beta_end: float = 0.012, camera_condition_type: str = "rotation", view_dependent_prompting: bool = False,
                 image_size: int = 256, grad_clip=None, token_merging: bool = False, guidance_eval: bool = False, recon_loss: bool = True,
                 fused: bool = True):
        if camera_condition_type != "rotation":
            raise NotImplementedError(f"Unknown camera_condition_type={camera_condition_type}")
        for name, value, off in (("grad_clip", grad_clip, None), ("token_merging", token_merging, False),
                                 ("guidance_eval", guidance_eval, False), ("recon_loss", recon_loss, True)):
            if value is not off and value != off:
                raise NotImplementedError(f"{name} = {value!r}: no released config uses it, not built")
        if n_frame < 2:
            raise ValueError("n_frame must be >= 2 (frame 0 is the clean conditioning frame)")
        self.vae, self.unet, self.image_encoder = vae, unet, image_encoder
        self.n_view, self.n_frame = int(n_view), int(n_frame)
        self.guidance_scale, self.recon_std_rescale = float(guidance_scale), float(recon_std_rescale)
        self.min_step_percent, self.max_step_percent = min_step_percent, max_step_percent
        self.sqrt_anneal, self.trainer_max_steps = bool(sqrt_anneal), trainer_max_steps
        self.i2v_cond_time_zero = bool(i2v_cond_time_zero)
        self.weights_dtype = weights_dtype or (torch.float16 if half_precision_weights else torch.float32)
        self.view_dependent_prompting = bool(view_dependent_prompting)
        self.image_size = int(image_size)
        self.num_train_timesteps = int(num_train_timesteps)
        self.alphas_cumprod = ddim_schedule(1, self.num_train_timesteps, beta_start, beta_end)[1].float()
        self._table: Dict[torch.device, torch.Tensor] = {}       # alphas_cumprod per device, copied once
        self.text_embeddings = text_embeddings
        self.fused = bool(fused)
        self.set_min_max_steps()                                 # the reference's defaults until the first update_step (:316)

    # ---- the timestep range (:323-325, :767-793)

    def set_min_max_steps(self, min_step_percent: float = 0.02, max_step_percent: float = 0.98) -> None:
        self.min_step = int(self.num_train_timesteps * min_step_percent)
        self.max_step = int(self.num_train_timesteps * max_step_percent)

    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False) -> None:
        low = scheduled(self.min_step_percent, global_step, epoch=epoch)
        if self.sqrt_anneal:
            percentage = (float(global_step) / self.trainer_max_steps) ** 0.5
            top = self.max_step_percent if type(self.max_step_percent) in (float, int) else self.max_step_percent[1]
            curr = (top - low) * (1 - percentage) + low
            self.set_min_max_steps(min_step_percent=curr, max_step_percent=curr)
        else:
            self.set_min_max_steps(min_step_percent=low, max_step_percent=scheduled(self.max_step_percent, global_step, epoch=epoch))

    # ---- the conditions

    def _alphas_on(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device not in self._table:
            self._table[device] = self.alphas_cumprod.to(device).contiguous()
        return self._table[device]

    def _frame0(self, x: torch.Tensor, b: int) -> torch.Tensor:
        return x.reshape(b, self.n_view, self.n_frame)[..., 0].reshape(-1)

    def get_text_embeddings(self, prompt_utils, elevation, azimuth, camera_distances, b: int) -> torch.Tensor:
        """``[2 b n, L, D]`` in (text for every (b, view), then uncond) order: from ``prompt_utils`` with the frame-0 values (:411-413), or
        the pair given at construction, expanded."""
        if prompt_utils is not None:
            return prompt_utils.get_text_embeddings(self._frame0(elevation, b), self._frame0(azimuth, b), self._frame0(camera_distances, b),
                                                    self.view_dependent_prompting)
        if self.text_embeddings is None:
            raise ValueError("AnimateMVGuidance needs prompt_utils or text_embeddings=(text, uncond) at construction")
        text, uncond = (e.reshape(1, *e.shape[-2:]) for e in self.text_embeddings)
        rows = b * self.n_view
        return torch.cat([text.expand(rows, -1, -1), uncond.expand(rows, -1, -1)])

    # ---- the call (:509-593)

    def __call__(self, rgb: torch.Tensor, prompt_utils=None, *, elevation: Optional[torch.Tensor] = None,
                 azimuth: Optional[torch.Tensor] = None, camera_distances: Optional[torch.Tensor] = None, c2w: torch.Tensor,
                 rgb_as_latents: bool = False, guidance_eval: bool = False, generator: Optional[torch.Generator] = None,
                 image_embeds: Optional[torch.Tensor] = None, **ignored) -> Dict:
        if guidance_eval:
            raise NotImplementedError("guidance_eval: the debug videos are not built")
        if self.min_step > self.max_step:
            raise ValueError(f"min_step = {self.min_step} > max_step = {self.max_step}: nothing to draw a timestep from")
        n, f = self.n_view, self.n_frame
        if rgb.dim() != 4 or rgb.shape[0] % (n * f) != 0:
            raise ValueError(f"rgb: expected [(b n f), H, W, C] with n f = {n * f}, got {tuple(rgb.shape)}")
        b = rgb.shape[0] // (n * f)
        if prompt_utils is not None and (elevation is None or azimuth is None or camera_distances is None):
            raise ValueError("prompt_utils needs elevation, azimuth and camera_distances")
        if image_embeds is None and self.image_encoder is None:
            raise ValueError("AnimateMVGuidance needs image_embeds or an image_encoder")
        dev = rgb.device
        x = rgb.permute(0, 3, 1, 2)
        if rgb_as_latents:
            latents = F.interpolate(x, (self.image_size // 8, self.image_size // 8), mode="bilinear", align_corners=False)
        else:
            latents = self.vae.encode_images(F.interpolate(x, (self.image_size, self.image_size), mode="bilinear", align_corners=False),
                                             generator=generator)                                        # draw 1: the posterior noise
        if image_embeds is None:
            from .clip import encode_image_from_frames
            image_embeds = encode_image_from_frames(self.image_encoder, rgb.detach(), sds.first_frame_index(b, n, f, dev))[0]
        gdev = generator.device if generator is not None else dev
        t = torch.randint(self.min_step, self.max_step + 1, [b], dtype=torch.long, generator=generator, device=gdev)     # draw 2
        t = t.to(dev, non_blocking=True)
        text = self.get_text_embeddings(prompt_utils, elevation, azimuth, camera_distances, b).to(dev)
        kw = dict(n_view=n, n_frame=f, guidance_scale=self.guidance_scale, recon_std_rescale=self.recon_std_rescale,
                  i2v_cond_time_zero=self.i2v_cond_time_zero, generator=generator, weights_dtype=self.weights_dtype)    # draw 3: the noise
        table = self._alphas_on(dev)
        if self.fused:
            loss = sds._fused_step(self.unet, latents, t, text, image_embeds, c2w, table=table, noise=None, want_noise_pred=False, **kw)[0]
        else:
            loss = sds.sds_recon_loss(self.unet, latents, t, text, image_embeds, c2w, alphas_cumprod=table, **kw)[0]
        return {"loss_sds": loss, "min_step": self.min_step, "max_step": self.max_step}
