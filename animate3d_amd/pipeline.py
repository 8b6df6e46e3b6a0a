"""MV-VDM generation as one object: four condition images and a prompt in, frames out.

``MVVideoPipeline`` has the call surface of the reference's ``AnimateDiffMVI2VPipeline`` (animatediff/pipelines/pipeline.py:880-1061, step 3 of
the reference's README: ``inference.py``) and composes this package's own modules in that order:

1. ``clip.encode_prompt``: prompt embeddings, (uncond, text), repeated per view                      pipeline.py:913-932
2. ``clip.encode_image_from_frames``: image embeddings, zeros as the unconditional half              :934-937
3. ``AutoencoderKLEncoder.encode_latents`` of the condition images                                   :951-953
4. ``denoise.prepare_latents`` for frames 1..                                                        :955-973
5. ``embeddings.get_camera(n)``                                                                      :984
6. ``denoise.denoise_free_init`` / ``denoise_loop``: the FreeInit passes around the loop             :987-1047
7. ``AutoencoderKLDecoder.decode_frames_u8`` / ``decode_latents``                                    :1049-1054
8. post-processing (``video.VideoFrames``)

``generator`` is consumed in this order, which is part of the contract: the posterior sample of the n condition images (3), the noise of
frames 1.. (4), FreeInit's fresh noise for each iteration after the first (6).

The condition images enter as bytes and stay bytes until a kernel reads them: ``video.images_in_u8`` makes the VAE's normalised planar
input (bit-equal to the reference's host arithmetic) and, in the same launch, the float image ``clip.preprocess_frames`` re-quantises to
exactly those bytes for the CLIP tower.  The frames leave as bytes: ``output_type="u8"`` / ``"pil"`` never make the fp32 video.

**Resizing.**  The reference resizes the condition images with torchvision's ``transforms.Resize``, which is not available to run or to compare
with: the images must already be ``height x width``, anything else raises ``ValueError`` (the policy of ``frames.load_frames`` for
``cv2.INTER_AREA``).  **Refused** with ``NotImplementedError`` naming the argument: ``guidance_scale <= 1`` (the fused step kernel takes the CFG
pair), a non-null ``i2v_similarity_init`` (null in configs/inference/inference.yaml; with FreeInit the reference itself reads an undefined
``strength`` at pipeline.py:997), ``eta != 0``, callbacks, ``clip_skip``, a ``cross_attention_kwargs`` other than ``{"scale": s}`` (there are
no LoRA layers for ``s`` to scale: it has no effect), ``ip_adapter_image_embeds``, FreeInit's ``use_fast_sampling``.  No vocabulary ships with
the package: ``tokenizer`` is any callable with the Hugging Face tokenizer interface, and ``prompt_ids`` / ``negative_prompt_ids`` [1, 77]
bypass it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import clip, denoise, embeddings
from .video import VideoFrames, images_in_u8

OUTPUT_TYPES = ("latent", "u8", "pil", "np", "pt")
_REFUSED_WHEN_SET = ("callback", "callback_steps", "callback_on_step_end", "callback_on_step_end_tensor_inputs", "clip_skip",
                     "ip_adapter_image_embeds")
_EXTRA = _REFUSED_WHEN_SET + ("eta", "cross_attention_kwargs")


@dataclass
class MVVideoPipelineOutput:
    """``frames``: what ``output_type`` names (``MVVideoPipeline.__call__``)."""
    frames: Any


def _not_built(name: str, value):
    raise NotImplementedError(f"{name} = {value!r}: no released config uses it, not built")


def check_output_type(output_type: str):
    if output_type not in OUTPUT_TYPES:
        raise ValueError(f"{output_type} does not exist. Please choose one of {list(OUTPUT_TYPES)}")


def condition_images(ip_adapter_image, height: Optional[int] = None, width: Optional[int] = None):
    """The accepted forms of ``ip_adapter_image`` as one uint8 ``[n, H, W, 3|4]`` array or tensor, checked on the host: a list of PIL images
    (converted to RGB as diffusers' ``load_image`` does), a numpy uint8 array, or a torch uint8 tensor on the host or the device.  All n
    images have one size, and that size is ``height x width`` where those are given: ``ValueError`` otherwise (module docstring)."""
    img = ip_adapter_image
    if isinstance(img, (list, tuple)):
        if not img:
            raise ValueError("ip_adapter_image: an empty list")
        if any(isinstance(i, (np.ndarray, torch.Tensor)) or not hasattr(i, "convert") for i in img):
            raise TypeError("ip_adapter_image: a list holds PIL images; pass arrays as one uint8 [n, H, W, 3|4]")
        sizes = {i.size for i in img}
        if len(sizes) != 1:
            raise ValueError(f"ip_adapter_image: the images have different sizes {sorted(sizes)} (width, height); all n views need one size")
        img = np.stack([np.asarray(i.convert("RGB")) for i in img])
    if not isinstance(img, (np.ndarray, torch.Tensor)):
        raise TypeError(f"ip_adapter_image: a list of PIL images, a numpy array or a tensor, got {type(ip_adapter_image)}")
    if img.dtype not in (np.uint8, torch.uint8) or img.ndim != 4 or img.shape[3] not in (3, 4) or 0 in img.shape:
        raise ValueError(f"ip_adapter_image: expected uint8 [n, H, W, 3|4], got {img.dtype} {list(img.shape)}")
    H, W = int(img.shape[1]), int(img.shape[2])
    if (height is not None and int(height) != H) or (width is not None and int(width) != W):
        raise ValueError(f"ip_adapter_image is {H} x {W}, the call asks for {height} x {width}: resize the images first. The reference resizes "
                         "with torchvision's transforms.Resize, which is not available to run or to compare with")
    return img


def float_frames(video: torch.Tensor, output_type: str):
    """``tensor2vid(video, processor, "np" | "pt")`` for the fp32 video ``[n, 3, F, H, W]``: ``(x / 2 + 0.5).clamp(0, 1)`` as ``"pt"``
    ``[n, F, 3, H, W]`` on the video's device, or as ``"np"`` float32 ``[n, F, H, W, 3]`` on the host."""
    unit = (video.float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 1, 3, 4)
    if output_type == "pt":
        return unit.contiguous()
    if output_type == "np":
        return unit.cpu().permute(0, 1, 3, 4, 2).float().numpy()
    raise ValueError(f"float_frames makes 'np' and 'pt', not {output_type!r}")


class MVVideoPipeline:
    """``MVVideoPipeline(unet, vae_encoder, vae_decoder, text_encoder, image_encoder, tokenizer=None, scheduler_kwargs=None)``: this package's
    ``MVUNetMotionModel``, ``AutoencoderKLEncoder`` / ``Decoder``, ``CLIPTextEncoder`` and ``CLIPVisionEncoderWithProjection`` on one device.
    ``scheduler_kwargs``: ``denoise.ddim_schedule``'s (the released DDIM configuration by default).  See the module docstring."""

    def __init__(self, unet, vae_encoder, vae_decoder, text_encoder, image_encoder, tokenizer=None, scheduler_kwargs: Optional[Dict] = None):
        self.unet, self.vae_encoder, self.vae_decoder = unet, vae_encoder, vae_decoder
        self.text_encoder, self.image_encoder, self.tokenizer = text_encoder, image_encoder, tokenizer
        self.scheduler_kwargs = dict(scheduler_kwargs) if scheduler_kwargs else None
        self._free_init = None

    # ---- FreeInit (diffusers' FreeInitMixin, parameter names as there)
    def enable_free_init(self, method: str = "butterworth", num_iters: int = 3, use_fast_sampling: bool = False, order: int = 4,
                         spatial_stop_frequency: float = 0.25, temporal_stop_frequency: float = 0.25):
        if use_fast_sampling:
            _not_built("use_fast_sampling", use_fast_sampling)
        if method not in ("butterworth", "gaussian", "ideal"):
            raise NotImplementedError(f"FreeInit filter method {method!r} (butterworth, gaussian, ideal)")
        if int(num_iters) < 1:
            raise ValueError("num_iters must be >= 1")
        self._free_init = dict(method=method, num_iters=int(num_iters), order=int(order), spatial_stop_frequency=float(spatial_stop_frequency),
                               temporal_stop_frequency=float(temporal_stop_frequency))

    def disable_free_init(self):
        self._free_init = None

    @property
    def free_init_enabled(self) -> bool:
        return self._free_init is not None

    @property
    def device(self) -> torch.device:
        return self.unet.device

    # ---- host-side checks: everything here runs before any device work
    def _check(self, prompt, negative_prompt, prompt_ids, negative_prompt_ids, num_frames, num_videos_per_prompt, guidance_scale,
               latents, i2v_similarity_init, output_type, extra: Dict):
        for name in extra:
            if name not in _EXTRA:
                raise TypeError(f"__call__() got an unexpected keyword argument {name!r}")
        if guidance_scale <= 1:
            _not_built("guidance_scale", guidance_scale)
        if i2v_similarity_init is not None:
            _not_built("i2v_similarity_init", i2v_similarity_init)
        if extra.get("eta", 0.0) != 0:
            _not_built("eta", extra["eta"])
        for name in _REFUSED_WHEN_SET:
            if extra.get(name) is not None:
                _not_built(name, extra[name])
        cak = extra.get("cross_attention_kwargs")
        if cak is not None and not (isinstance(cak, dict) and set(cak) == {"scale"}):
            _not_built("cross_attention_kwargs", cak)
        check_output_type(output_type)
        if (prompt is None) == (prompt_ids is None):
            raise ValueError("pass one of `prompt` and `prompt_ids`")
        if prompt is not None and not isinstance(prompt, str):
            raise ValueError(f"`prompt` is one string per call (the n views share it), got {type(prompt)}")
        if not isinstance(negative_prompt, str):
            raise ValueError(f"`negative_prompt` is one string, got {type(negative_prompt)}")
        if self.tokenizer is None:
            if prompt is not None:
                raise ValueError("`prompt` needs a tokenizer and the pipeline has none (no vocabulary ships with the package): construct it with "
                                 "tokenizer=..., or pass prompt_ids and negative_prompt_ids [1, 77]")
            if negative_prompt_ids is None:
                raise ValueError("without a tokenizer `negative_prompt_ids` [1, 77] (the ids of the negative prompt, \"\" as released) must be passed")
        for name, ids in (("prompt_ids", prompt_ids), ("negative_prompt_ids", negative_prompt_ids)):
            if ids is not None and not (isinstance(ids, torch.Tensor) and ids.dim() == 2 and ids.shape[0] == 1
                                        and ids.dtype in (torch.int32, torch.int64)):
                raise ValueError(f"{name}: expected an integer tensor [1, tokens], got {getattr(ids, 'dtype', type(ids))} "
                                 f"{list(getattr(ids, 'shape', []))}")
        if int(num_frames) < 2:
            raise ValueError("num_frames must be >= 2 (frame 0 is the conditioning frame)")
        if int(num_videos_per_prompt) < 1:
            raise ValueError("num_videos_per_prompt must be >= 1")
        if latents is not None and not (isinstance(latents, torch.Tensor) and latents.dim() == 5):
            raise ValueError("latents: the noise of frames 1.., [n, 4, num_frames - 1, height / 8, width / 8]")

    def _tokenize(self, text: str) -> torch.Tensor:
        tok = self.tokenizer
        return tok(text, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids

    @torch.no_grad()
    def __call__(self, prompt: Optional[str] = None, *, negative_prompt: str = "", prompt_ids: Optional[torch.Tensor] = None,
                 negative_prompt_ids: Optional[torch.Tensor] = None, ip_adapter_image, num_frames: int = 16, height: Optional[int] = None,
                 width: Optional[int] = None, num_videos_per_prompt: int = 4, num_inference_steps: int = 25, guidance_scale: float = 7.5,
                 generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None, i2v_cond_time_zero: bool = False,
                 i2v_similarity_init=None, output_type: str = "pil", return_dict: bool = True, **extra):
        """One generation.  ``ip_adapter_image``: the n = ``num_videos_per_prompt`` condition images (``condition_images``).  ``output_type``:
        ``"latent"`` fp32 ``[n, 4, F, h, w]``; ``"u8"`` a ``video.VideoFrames``; ``"pil"`` n lists of F PIL images, made from those bytes;
        ``"np"`` float32 ``[n, F, H, W, 3]`` in [0, 1]; ``"pt"`` float32 ``[n, F, 3, H, W]`` in [0, 1] on the device.  Returns an object with
        ``.frames``, or with ``return_dict=False`` a 1-tuple.  ``latents``: the noise of frames 1.. instead of a draw from ``generator``.
        ``extra`` takes the reference's remaining keywords so that they can be refused by name (module docstring)."""
        self._check(prompt, negative_prompt, prompt_ids, negative_prompt_ids, num_frames, num_videos_per_prompt, guidance_scale, latents,
                    i2v_similarity_init, output_type, extra)
        images = condition_images(ip_adapter_image, height, width)
        n, num_frames = int(num_videos_per_prompt), int(num_frames)
        if images.shape[0] != n:
            raise ValueError(f"ip_adapter_image holds {images.shape[0]} images, num_videos_per_prompt = {n}: one condition image per view")
        ids = prompt_ids if prompt_ids is not None else self._tokenize(prompt)
        neg_ids = negative_prompt_ids if negative_prompt_ids is not None else self._tokenize(negative_prompt)
        device = self.device

        # 1. prompt embeddings: (uncond, text), each repeated per view
        pe, ne = clip.encode_prompt(self.text_encoder, ids.to(device), neg_ids.to(device))
        prompt_embeds = torch.cat([ne.repeat(n, 1, 1), pe.repeat(n, 1, 1)])

        # 2. / 3. the condition images: bytes -> (VAE input, CLIP input) in one launch
        u8 = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        planar, unit = images_in_u8(u8.to(device), unit=True)
        image_embeds, negative_image_embeds = clip.encode_image_from_frames(self.image_encoder, unit)
        image_embeds = torch.cat([negative_image_embeds, image_embeds])
        first_frame_latents = self.vae_encoder.encode_latents(planar, generator).float()

        # 4. frames 1..
        if latents is None:
            latents, first = denoise.prepare_latents(first_frame_latents, num_frames, generator, device, torch.float32)
        else:
            first = first_frame_latents.unsqueeze(2)
            want = (n, first.shape[1], num_frames - 1) + tuple(first.shape[3:])
            if tuple(latents.shape) != want:
                raise ValueError(f"latents: expected the noise of frames 1.. {list(want)}, got {list(latents.shape)}")
            latents = torch.cat([first, latents.to(device=device, dtype=torch.float32)], dim=2)

        # 5. / 6.
        camera = embeddings.get_camera(n).to(device=device, dtype=prompt_embeds.dtype)
        loop = dict(num_inference_steps=int(num_inference_steps), guidance_scale=float(guidance_scale), i2v_cond_time_zero=bool(i2v_cond_time_zero),
                    scheduler_kwargs=self.scheduler_kwargs)
        if self._free_init is not None:
            latents = denoise.denoise_free_init(self.unet, latents, first, prompt_embeds, image_embeds, camera, generator=generator,
                                                **self._free_init, **loop)
        else:
            latents = denoise.denoise_loop(self.unet, latents, first, prompt_embeds, image_embeds, camera, **loop)

        # 7. / 8.
        if output_type == "latent":
            frames = latents
        elif output_type in ("u8", "pil"):
            frames = VideoFrames(self.vae_decoder.decode_frames_u8(latents))
            if output_type == "pil":
                frames = frames.pil()
        else:
            frames = float_frames(self.vae_decoder.decode_latents(latents), output_type)
        return MVVideoPipelineOutput(frames=frames) if return_dict else (frames,)
