"""float32 CPU restatements of the arithmetic of csrc/video_io.hip, with torch and numpy exactly as the reference chains them (a helper,
not a test; imports nothing of the package).

In: ``AnimateDiffMVI2VPipeline.encode_latents`` (animatediff/pipelines/pipeline.py:548-554): ``torch.from_numpy(np.array(image))``, ``/ 255``,
``permute``, torchvision's ``Normalize(0.5, 0.5)`` = ``tensor.sub_(mean).div_(std)`` with ``mean`` / ``std`` as ``[3, 1, 1]`` tensors.

Out: ``tensor2vid`` (:237-255) -> diffusers' ``VaeImageProcessor.postprocess`` (third-party, restated from 0.28.0: ``denormalize`` =
``(images / 2 + 0.5).clamp(0, 1)``, ``pt_to_numpy`` = ``.cpu().permute(0, 2, 3, 1).float().numpy()``, ``numpy_to_pil`` =
``(images * 255).round().astype("uint8")``)."""
from types import SimpleNamespace

import numpy as np
import torch


def unit_ref(images_u8: np.ndarray) -> torch.Tensor:
    """uint8 [n, H, W, 3|4] -> float32 [n, H, W, 3] = ``image_tensor / 255`` of the RGB channels (what ``np.array`` of an RGB image holds)."""
    image_tensor = torch.from_numpy(np.ascontiguousarray(images_u8[..., :3]))
    return image_tensor / 255


def images_in_ref(images_u8: np.ndarray) -> torch.Tensor:
    """uint8 [n, H, W, 3|4] -> float32 [n, 3, H, W]: the tensor ``encode_latents`` hands the VAE (``Resize`` at the images' own size is the
    identity)."""
    image_tensor = unit_ref(images_u8).permute(0, 3, 1, 2).contiguous()
    mean = torch.as_tensor([0.5, 0.5, 0.5], dtype=image_tensor.dtype)
    std = torch.as_tensor([0.5, 0.5, 0.5], dtype=image_tensor.dtype)
    return image_tensor.sub_(mean[:, None, None]).div_(std[:, None, None])


def denormalize_ref(images: torch.Tensor) -> torch.Tensor:
    return (images / 2 + 0.5).clamp(0, 1)


def numpy_to_u8_ref(images: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):                    # a NaN: numpy's cast is not defined, the kernel's byte is 0 (asserted apart)
        return (images * 255).round().astype("uint8")


def values_to_u8_ref(x: torch.Tensor) -> np.ndarray:
    """The chain on loose float32 values of any shape: uint8 of that shape."""
    assert x.dtype == torch.float32 and x.device.type == "cpu"
    return numpy_to_u8_ref(denormalize_ref(x).float().numpy())


def video_to_u8_ref(video: torch.Tensor) -> np.ndarray:
    """float32 [n, 3, F, H, W] (``decode_latents``) -> uint8 [n, F, H, W, 3]: the bytes of ``tensor2vid(video, processor, "pil")``'s images."""
    assert video.dtype == torch.float32 and video.device.type == "cpu" and video.dim() == 5 and video.shape[1] == 3
    outputs = []
    for batch_idx in range(video.shape[0]):
        batch_vid = video[batch_idx].permute(1, 0, 2, 3)
        images = denormalize_ref(batch_vid).cpu().permute(0, 2, 3, 1).float().numpy()
        outputs.append(numpy_to_u8_ref(images))
    return np.ascontiguousarray(np.stack(outputs))


def video_to_np_ref(video: torch.Tensor) -> np.ndarray:
    """``tensor2vid(video, processor, "np")``: float32 [n, F, H, W, 3] in [0, 1]."""
    return np.stack([denormalize_ref(v.permute(1, 0, 2, 3)).cpu().permute(0, 2, 3, 1).float().numpy() for v in video])


def strip_ref(frames_u8: np.ndarray) -> np.ndarray:
    """uint8 [n, F, H, W, 3] -> [F, H, n W, 3]: ``export_to_gif_mv`` pastes view i of frame f at x offset i W (animatediff/utils/util.py:190-220)."""
    n, F, H, W, C = frames_u8.shape
    return np.ascontiguousarray(frames_u8.transpose(1, 2, 0, 3, 4)).reshape(F, H, n * W, C)


# ---- deterministic stand-ins shared by tests/golden/make_pipeline_call_goldens.py (which runs the REFERENCE's statements with them) and
# tests/test_pipeline_golden.py (which runs MVVideoPipeline with them); the UNet stand-in is tests/sds_stub.py's
class StubVAE:
    """A cheap ``AutoencoderKL``: ``encode(x).latent_dist.sample()`` and ``decode(z).sample``, 8x down and up.  The posterior sample draws
    from ``generator``: the reference calls ``sample()`` without one (the global stream); handing the stand-in the call's generator is what
    makes the order of the draws visible in the vectors."""
    scale_factor = 8

    def __init__(self, generator=None, scaling_factor: float = 0.18215):
        self.config = SimpleNamespace(scaling_factor=scaling_factor)
        self.device, self.dtype, self.generator = torch.device("cpu"), torch.float32, generator

    def encode(self, x):
        pooled = torch.nn.functional.avg_pool2d(x.float(), self.scale_factor)
        mix = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, -0.25, 0.75]])
        mean = torch.einsum("oc,bchw->bohw", mix, pooled)
        std = 0.1 + 0.05 * pooled.mean(dim=1, keepdim=True).abs()
        gen = self.generator
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda: mean + std * torch.randn(mean.shape, generator=gen)))

    def decode(self, z):
        up = torch.nn.functional.interpolate(z.float(), scale_factor=self.scale_factor, mode="nearest")
        mix = torch.tensor([[0.9, 0.1, -0.2, 0.3], [-0.1, 0.8, 0.2, -0.3], [0.2, -0.2, 0.7, 0.4]])
        H, W = up.shape[-2:]
        ramp = torch.linspace(-0.4, 0.4, H)[:, None] + torch.linspace(-0.3, 0.3, W)[None, :]
        return SimpleNamespace(sample=0.04 * torch.einsum("oc,bchw->bohw", mix, up) + ramp)       # leaves [-1, 1] in places: both clamps


class StubEncoderHalf:
    """``AutoencoderKLEncoder.encode_latents(images, generator)`` over ``StubVAE`` (pipeline.py:556-560)."""

    def encode_latents(self, images, generator=None):
        vae = StubVAE(generator)
        return vae.encode(images).latent_dist.sample() * vae.config.scaling_factor


class StubDecoderHalf:
    """``AutoencoderKLDecoder.decode_latents`` / ``decode_frames_u8`` over ``StubVAE`` (pipeline.py:566-577 and the chain above)."""

    def decode_latents(self, latents):
        vae = StubVAE()
        b, c, f, h, w = latents.shape
        z = (1 / vae.config.scaling_factor * latents).permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
        image = vae.decode(z).sample
        return image[None, :].reshape((b, f, -1) + image.shape[2:]).permute(0, 2, 1, 3, 4).float()

    def decode_frames_u8(self, latents, out=None, strip=False):
        return torch.from_numpy(video_to_u8_ref(self.decode_latents(latents)))


def stub_text_encoder(input_ids):
    """ids [B, T] -> ([B, T, 16],): every token leaves a trace."""
    return (torch.sin(input_ids[..., None].float() * torch.arange(1, 17).float() * 0.37),)


def stub_image_embeds(unit_rgb):
    """float [n, H, W, 3] in [0, 1] -> [n, 12]."""
    m = unit_rgb.float().mean(dim=(1, 2))
    return 0.05 * torch.cat([m, m * m, torch.sin(3 * m), m.roll(1, dims=1) - 0.5], dim=1)


def split_gif_name(view: int, frame: int, frame_count: int) -> str:
    """The file tools/split_gif.py writes for square ``view`` of GIF frame ``frame``: ``f"{i * frame_count + frame_num}.png"``."""
    return f"{view * frame_count + frame}.png"
