"""The byte ends of MV-VDM generation: condition images in as bytes, generated frames out as bytes, on the gfx950 kernels of csrc/video_io.hip.

In.  The reference's ``encode_latents`` (animatediff/pipelines/pipeline.py:548-554) stacks the PIL images as uint8, divides by 255, permutes and
normalises on the host.  ``images_in_u8(images [n, H, W, 3|4] uint8)`` is that in one launch: ``planar [n, 3, H, W]`` fp32, bit for bit what
torch gives on the CPU, and with ``unit=True`` also ``[n, H, W, 3]`` fp32 = ``b / 255.0f`` for ``clip.preprocess_frames``, which re-quantises a
float image by truncation: ``(uint8)((b / 255.0f) * 255.0f)`` is ``b`` for all 256 bytes (tests/test_video_io_gpu.py), so the CLIP resampler
sees the input bytes.

Out.  The reference walks ``decode_latents``' fp32 ``[n, 3, F, H, W]`` video through ``tensor2vid`` -> ``VaeImageProcessor.postprocess``
(``(x / 2 + 0.5).clamp(0, 1)``, host copy, numpy) -> ``numpy_to_pil`` (``(images * 255).round().astype("uint8")``).  ``video_to_u8`` is that
arithmetic in one launch, from the fp32 video or straight from the VAE decoder's 16-bit ``conv_out`` rows (``AutoencoderKLDecoder.decode_frames_u8``:
the fp32 video is then never made), into per-view frames ``[n, F, H, W, 3]`` or the side-by-side strip ``[F, H, n W, 3]`` that
``export_to_gif_mv`` (animatediff/utils/util.py:190-220) pastes together.  A NaN gives byte 0; numpy's cast of a NaN is not defined.

``VideoFrames`` holds the bytes and writes the files: the GIF of the strip, and the ``{view * F + frame}.png`` files that the reference gets by
cutting that GIF up again (tools/split_gif.py) and that the 4-D stage starts from (``frames.load_frames``): here they are lossless and have not
been through a 256-colour palette.  ``with_alpha`` hands them to the 4-D stage without touching a file.

uint8 / fp32 / 16-bit CUDA tensors only for the kernels: CPU tensors raise, there is no torch fallback.  Files are written with PIL on the host."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from .f32_stage import launch, require_shape
from .frames import FrameSet, _require_u8_cuda
from .hip_ops import _DTYPE_CODE, _p


def images_in_u8(images: torch.Tensor, *, unit: bool = False):
    """``images [n, H, W, 3|4]`` uint8 CUDA (a fourth channel is ignored) -> ``planar [n, 3, H, W]`` fp32 = ``(b / 255 - 0.5) / 0.5``; with
    ``unit`` the pair ``(planar, unit [n, H, W, 3] fp32 = b / 255)``.  See the module docstring."""
    require_shape("images", images, ("n", "H", "W", 3), ("n", "H", "W", 4), non_empty=True)
    _require_u8_cuda("images", images)
    src = images.contiguous()
    n, H, W, cin = src.shape
    planar = torch.empty(n, 3, H, W, dtype=torch.float32, device=src.device)
    rgb = torch.empty(n, H, W, 3, dtype=torch.float32, device=src.device) if unit else None
    launch("a3d_images_in_u8", src.device, _p(src), n, H, W, cin, _p(planar), _p(rgb))
    return (planar, rgb) if unit else planar


def strip_as_views(strip: torch.Tensor, n: int) -> torch.Tensor:
    """The view ``[n, F, H, W, pixel]`` of a strip ``[F, H, n W, pixel]``: pixel (v, f, y, x) of the video is strip pixel (f, y, v W + x)."""
    F, H, nW, pixel = strip.shape
    if nW % n:
        raise ValueError(f"strip: width {nW} is not {n} views side by side")
    return strip.view(F, H, n, nW // n, pixel).permute(2, 0, 1, 3, 4)


def video_to_u8(video: torch.Tensor, shape: Optional[Tuple[int, int, int, int]] = None, *, out: Optional[torch.Tensor] = None,
                strip: bool = False, pixel: int = 3) -> torch.Tensor:
    """The reference's post-processing of a decoded video, to bytes (module docstring).

    ``video``: fp32 CUDA ``[n, 3, F, H, W]`` (what ``decode_latents`` returns), or the VAE decoder's ``conv_out`` rows ``[(n F) H W, 4]`` in
    bfloat16 / float16 with ``shape = (n, F, H, W)``, ``W % 4 == 0``.  ``out``: a uint8 CUDA tensor ``[n, F, H, W, pixel]`` to write into,
    any view whose pixels are contiguous (strides ``(.., .., .., pixel, 1)``): a slice of a larger buffer, or ``strip_as_views`` of a strip;
    bytes outside the addressed pixels are left alone.  Without ``out`` a fresh contiguous ``[n, F, H, W, pixel]`` is written, or with
    ``strip`` the strip ``[F, H, n W, pixel]``; that tensor is returned.  ``pixel`` 4: alpha = 255."""
    if not isinstance(video, torch.Tensor) or not video.is_cuda or video.dtype not in _DTYPE_CODE:
        raise RuntimeError(f"video: expected a float32 / bfloat16 / float16 CUDA tensor, got {getattr(video, 'dtype', type(video))} on "
                           f"{getattr(video, 'device', '?')} (no CPU fallback)")
    if video.dtype == torch.float32:
        require_shape("video", video, ("n", 3, "F", "H", "W"), non_empty=True)
        n, _, F, H, W = video.shape
        if shape is not None and tuple(shape) != (n, F, H, W):
            raise ValueError(f"shape {tuple(shape)} does not describe a video of {(n, F, H, W)}")
    else:
        if shape is None:
            raise ValueError("video: 16-bit rows need shape = (n, F, H, W)")
        n, F, H, W = (int(s) for s in shape)
        require_shape("video", video, (n * F * H * W, 4), non_empty=True)
        if W % 4:
            raise ValueError(f"video: the rows path needs W % 4 == 0, got W = {W}")
    if pixel not in (3, 4):
        raise ValueError(f"pixel = {pixel}: 3 (RGB) or 4 (RGBA, alpha 255)")
    src = video.detach().contiguous()
    result = out
    if out is None:
        result = torch.empty((F, H, n * W, pixel) if strip else (n, F, H, W, pixel), dtype=torch.uint8, device=src.device)
        out = strip_as_views(result, n) if strip else result
    else:
        _require_u8_cuda("out", out)
        require_shape("out", out, (n, F, H, W, pixel))
        if out.device != src.device or out.stride(4) != 1 or out.stride(3) != pixel or min(out.stride()[:3]) < 0:
            raise ValueError(f"out: expected a view on {src.device} whose pixels are contiguous, got strides {out.stride()}")
    launch("a3d_video_to_u8", src.device, _p(src), _DTYPE_CODE[src.dtype], n, F, H, W, _p(out), out.stride(0), out.stride(1), out.stride(2), pixel)
    return result


@dataclass(frozen=True, eq=False)
class VideoFrames:
    """The frames of one generation: ``u8 [n_view, F, H, W, 3]`` uint8, contiguous, on the device the pipeline ran on."""
    u8: torch.Tensor

    def __post_init__(self):
        require_shape("u8", self.u8, ("n_view", "F", "H", "W", 3), non_empty=True)
        if self.u8.dtype != torch.uint8 or not self.u8.is_contiguous():
            raise ValueError(f"u8: expected a contiguous uint8 tensor, got {self.u8.dtype} with strides {self.u8.stride()}")

    @property
    def n_view(self) -> int:
        return self.u8.shape[0]

    @property
    def n_frame(self) -> int:
        return self.u8.shape[1]

    @property
    def height(self) -> int:
        return self.u8.shape[2]

    @property
    def width(self) -> int:
        return self.u8.shape[3]

    def strip(self) -> torch.Tensor:
        """``[F, H, n W, 3]``: frame by frame the views side by side, ``export_to_gif_mv``'s layout."""
        n, F, H, W, _ = self.u8.shape
        return self.u8.permute(1, 2, 0, 3, 4).reshape(F, H, n * W, 3)

    def numpy(self) -> np.ndarray:
        """uint8 ``[n_view, F, H, W, 3]`` on the host."""
        return self.u8.cpu().numpy()

    def pil(self) -> List[list]:
        """n_view lists of F PIL images: the reference's ``output_type="pil"`` frames."""
        from PIL import Image
        return [[Image.fromarray(frame) for frame in view] for view in self.numpy()]

    def write_gif(self, path: str, fps: int = 10) -> str:
        """The strip as an animated GIF through PIL, as diffusers' ``export_to_gif`` writes the list ``export_to_gif_mv`` pastes together
        (``save_all``, ``append_images``, ``duration = 1000 / fps``, ``loop = 0``).  A GIF frame has 256 colours: PIL quantises each one.
        diffusers is not available to compare with, so agreement with its palette choice is not pinned and not claimed; the bytes themselves
        are in ``write_view_frames``' PNGs."""
        from PIL import Image
        images = [Image.fromarray(frame) for frame in self.strip().cpu().numpy()]
        folder = os.path.dirname(path)
        if folder:
            os.makedirs(folder, exist_ok=True)
        images[0].save(path, save_all=True, append_images=images[1:], duration=1000 / fps, loop=0)
        return path

    def write_view_frames(self, folder: str) -> List[str]:
        """``{view * F + frame}.png`` under ``folder`` as lossless RGB PNGs: the numbering the reference's tools/split_gif.py gives the pieces
        of the strip GIF (``i * frame_count + frame_num``), the folder the 4-D stage's data module reads.  Returns the paths in that order."""
        from PIL import Image
        os.makedirs(folder, exist_ok=True)
        paths = []
        host = self.numpy()
        F = self.n_frame
        for view in range(self.n_view):
            for frame in range(F):
                paths.append(os.path.join(folder, f"{view * F + frame}.png"))
                Image.fromarray(host[view, frame]).save(paths[-1])
        return paths

    def with_alpha(self, mask_u8: torch.Tensor):
        """A ``frames.FrameSet`` of these frames with ``mask_u8 [n_view, F, H, W]`` uint8 (a segmentation's foreground mask, 255 inside) as
        the alpha channel: the 4-D stage's ground truth without a file in between.  CUDA tensors, as ``FrameSet`` demands."""
        n, F, H, W, _ = self.u8.shape
        require_shape("mask_u8", mask_u8, (n, F, H, W))
        _require_u8_cuda("u8", self.u8)
        _require_u8_cuda("mask_u8", mask_u8)
        rgba = torch.cat([self.u8, mask_u8.to(self.u8.device).unsqueeze(-1)], dim=-1)
        return FrameSet(rgba.reshape(n * F, H, W, 4).contiguous(), n, F)
