"""The frames of the 4-D stage, where it touches the file system: 8-bit RGBA ground truth in, test renders out, on the gfx950 kernels of
csrc/stage_frames.hip.

In.  The reference's data module makes ``rgbs`` / ``masks`` in ``SimpleMultiImageDataBase.load_images`` (custom/threestudio-animate3d/
data/simple_multi_image.py:192-222): every ``<int>.png`` of ``image_root`` in numeric order, RGBA, resized with ``cv2.INTER_AREA``,
``astype(float32) / 255.0``, mask ``alpha > 0.5``; resident as fp32 + bool, 13 bytes a pixel.  The files hold bytes, so here the bytes
stay: a ``FrameSet`` keeps ``rgba8 [S, H, W, 4]`` uint8 on the device, 4 bytes a pixel, and ``stage4d.masked_recon_loss_rgba8`` reads it in the
loss kernel as ``byte / 255.0f`` and ``alpha byte >= 128``: the bits the reference's tensors hold.

Out.  ``Animate3DSystem.test_step`` (systems/animate3d.py:427-471) writes one RGBA PNG per test camera, ``(rgba_img * 255).astype(np.uint8)``
of ``cat([comp_rgb, comp_mask])``, and ``mesh_trajectory/{i}.npy``.  ``test_renders`` / ``write_test_renders`` / ``write_trajectory`` do that.
The refine stage's ``image_root`` is the reconstruction stage's ``four_view`` test output (``configs/refine_frame_16.yaml``), so
``load_frames`` on what ``write_test_renders`` wrote gives back the rendered bytes.

``FrameSet(rgba8, n_view, n_frame)``: ``rgba8 [n_view * n_frame, H, W, 4]`` uint8 on the device, view-major.  ``.rgb()`` ``[S, H, W, 3]`` fp32
and ``.mask()`` ``[S, H, W, 1]`` bool are the reference's tensors, made by the unpack kernel on each call, for a caller that wants them;
``.batch()`` is ``{"rgba8": rgba8}`` for ``stage4d.training_step`` (add the cameras).

``unpack_rgba8(rgba8, k=1, *, out8, rgb, mask)``: the unpack kernel.  ``k``: an integer reduction factor, every ``k x k`` block of source pixels
becomes one pixel; per channel, alpha included, ``q = (2 sum + k^2) // (2 k^2)``: the exact mean of the bytes, rounded half up
(``k = 2``: ``(a + b + c + d + 2) >> 2``; ``k = 1``: a copy).  ``rgb = q / 255.0f`` by IEEE division, ``mask = q_alpha >= 128``, which is
``q / 255.0f > 0.5f``.  Returns the tensors asked for in a dict.

``load_frames(image_root, height, width, *, n_view, n_frame, device)``: decodes with PIL, uploads the bytes once, one unpack call.
**Resizing.**  The reference resizes the 8-bit image with OpenCV's ``INTER_AREA``.  Built here: the files' own size (the refine chain), and
exact integer reduction factors up to 16 with the rule above.  For an integer factor ``INTER_AREA`` is a box mean as well, but its rounding
of the mean has not been compared with anything recorded: agreement with OpenCV for ``k >= 2`` is not claimed.  Any other ratio, different
factors in the two directions, and enlarging raise ``NotImplementedError``.  ``requires_depth`` is not built.

``pack_rgba8(image, alpha, out=None)``: ``render_batch``'s planar ``image [B, 3, H, W]`` and ``alpha [B, 1, H, W]`` / ``[B, H, W]`` -> ``[B, H, W, 4]``
uint8, ``(uint8)(clamp(v, 0, 1) * 255.0f)`` truncating.  The alpha is clamped as well: the reference does not clamp ``comp_mask``, and for a
rasterizer alpha, which lies in [0, 1], nothing changes; an alpha above 1 gives 255 here where numpy's cast would wrap.  A NaN gives 0.

fp32 and uint8 CUDA tensors only; CPU tensors raise, there is no torch fallback for the kernels.  Files are read and written with PIL and
numpy on the host."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .f32_stage import launch, require_f32_cuda, require_shape
from .hip_ops import _p

MAX_FACTOR = 16                  # SF_MAX_K of csrc/stage_frames.hip
_NAME = re.compile(r"^(\d+)\.[A-Za-z0-9]+$")


def _require_u8_cuda(name: str, t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise RuntimeError(f"{name}: expected a uint8 CUDA tensor, got {getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')} "
                           "(no CPU fallback)")


def unpack_rgba8(rgba8: torch.Tensor, k: int = 1, *, out8: bool = False, rgb: bool = False, mask: bool = False) -> Dict[str, torch.Tensor]:
    """``rgba8 [S, h, w, 4]`` uint8 reduced by the integer factor ``k``: of ``out8 [S, H, W, 4]`` uint8, ``rgb [S, H, W, 3]`` fp32 and ``mask
    [S, H, W, 1]`` bool those asked for, from one launch; see the module docstring."""
    require_shape("rgba8", rgba8, ("S", "h", "w", 4), non_empty=True)
    _require_u8_cuda("rgba8", rgba8)
    k = int(k)
    S, h, w, _ = rgba8.shape
    if not 1 <= k <= MAX_FACTOR or h % k or w % k:
        raise ValueError(f"k = {k}: an integer factor in 1 .. {MAX_FACTOR} that divides {h} x {w}")
    if not (out8 or rgb or mask):
        raise ValueError("unpack_rgba8: nothing asked for")
    H, W, dev = h // k, w // k, rgba8.device
    src = rgba8.contiguous()
    o8 = torch.empty(S, H, W, 4, dtype=torch.uint8, device=dev) if out8 else None
    o_rgb = torch.empty(S, H, W, 3, dtype=torch.float32, device=dev) if rgb else None
    o_mask = torch.empty(S, H, W, 1, dtype=torch.uint8, device=dev) if mask else None
    launch("a3d_frames_unpack_u8", dev, S, h, w, k, _p(src), _p(o8), _p(o_rgb), _p(o_mask))
    found = dict(out8=o8, rgb=o_rgb, mask=None if o_mask is None else o_mask.view(torch.bool))
    return {name: t for name, t in found.items() if t is not None}


def pack_rgba8(image: torch.Tensor, alpha: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``image [B, 3, H, W]`` and ``alpha [B, 1, H, W]`` / ``[B, H, W]`` fp32 -> ``[B, H, W, 4]`` uint8 (into ``out``, where given: a contiguous
    uint8 CUDA tensor of that shape); see the module docstring."""
    require_shape("image", image, ("B", 3, "H", "W"), non_empty=True)
    B, _, H, W = image.shape
    require_shape("alpha", alpha, (B, 1, H, W), (B, H, W))
    require_f32_cuda("image", image)
    require_f32_cuda("alpha", alpha)
    if out is None:
        out = torch.empty(B, H, W, 4, dtype=torch.uint8, device=image.device)
    else:
        require_shape("out", out, (B, H, W, 4))
        _require_u8_cuda("out", out)
        if not out.is_contiguous() or out.device != image.device:
            raise ValueError("out: expected a contiguous tensor on the image's device")
    launch("a3d_frames_pack_u8", image.device, B, H, W, _p(image.detach().contiguous()), _p(alpha.detach().contiguous()), _p(out))
    return out


@dataclass(frozen=True, eq=False)
class FrameSet:
    """The resident ground truth of the stage: ``rgba8 [n_view * n_frame, H, W, 4]`` uint8 on the device, view-major."""
    rgba8: torch.Tensor
    n_view: int
    n_frame: int

    def __post_init__(self):
        require_shape("rgba8", self.rgba8, ("S", "H", "W", 4), non_empty=True)
        _require_u8_cuda("rgba8", self.rgba8)
        if self.rgba8.shape[0] != self.n_view * self.n_frame:
            raise ValueError(f"rgba8: {self.rgba8.shape[0]} images for n_view * n_frame = {self.n_view} * {self.n_frame}")
        if not self.rgba8.is_contiguous():
            raise ValueError("rgba8: expected a contiguous tensor")

    @property
    def height(self) -> int:
        return self.rgba8.shape[1]

    @property
    def width(self) -> int:
        return self.rgba8.shape[2]

    def rgb(self) -> torch.Tensor:
        """``[S, H, W, 3]`` fp32: the reference's ``rgbs``, ``byte / 255.0f``."""
        return unpack_rgba8(self.rgba8, rgb=True)["rgb"]

    def mask(self) -> torch.Tensor:
        """``[S, H, W, 1]`` bool: the reference's ``masks``, ``alpha / 255.0f > 0.5f``."""
        return unpack_rgba8(self.rgba8, mask=True)["mask"]

    def batch(self) -> Dict[str, torch.Tensor]:
        """``{"rgba8": rgba8}``: the ground truth of ``stage4d.training_step``'s batch."""
        return {"rgba8": self.rgba8}


def frame_files(image_root: str) -> List[str]:
    """The file names of ``image_root`` in the reference's order, ``sorted(os.listdir(root), key=lambda x: int(x[:-4]))``: by the integer, so
    ``10.png`` comes after ``9.png``.  A name that is not ``<int>.<ext>`` raises ``ValueError`` (the reference's ``int()`` does too)."""
    names = os.listdir(image_root)
    for name in names:
        if not _NAME.match(name):
            raise ValueError(f"{os.path.join(image_root, name)}: the frames are named <int>.<ext>, sorted by the integer")
    return sorted(names, key=lambda name: int(name.split(".")[0]))


def reduction_factor(src_h: int, src_w: int, height: int, width: int) -> int:
    """The integer ``k`` with ``src = k * (height, width)``; ``NotImplementedError`` for every resize that is not one (module docstring)."""
    if (src_h, src_w) == (height, width):
        return 1
    k = src_h // height if height > 0 else 0
    if k < 2 or k > MAX_FACTOR or src_h != k * height or src_w != k * width:
        raise NotImplementedError(f"resize {src_h} x {src_w} -> {height} x {width}: only the files' own size and exact integer reduction factors "
                                  f"up to {MAX_FACTOR} (the same in both directions) are built. The reference resizes with OpenCV's INTER_AREA, "
                                  "which is not available to compare any other ratio, or enlarging, against")
    return k


def decode_frames(image_root: str, *, count: Optional[int] = None) -> np.ndarray:
    """``uint8 [S, h, w, 4]`` on the host: the frames of ``image_root`` in ``frame_files``' order, decoded with PIL.  ``ValueError`` for a file
    that is not 8-bit RGBA (the reference's ``COLOR_BGRA2RGBA`` fails on it), sizes that differ between files, and a count other than
    ``count``."""
    from PIL import Image
    names = frame_files(image_root)
    if count is not None and len(names) != count:
        raise ValueError(f"{image_root}: {len(names)} frames, expected n_view * n_frame = {count}")
    if not names:
        raise ValueError(f"{image_root}: no frames")
    out = None
    for i, name in enumerate(names):
        path = os.path.join(image_root, name)
        with Image.open(path) as im:
            if im.mode != "RGBA":
                raise ValueError(f"{path}: mode {im.mode}, expected 8-bit RGBA")
            arr = np.asarray(im)
        if out is None:
            out = np.empty((len(names), *arr.shape), np.uint8)
        elif arr.shape != out.shape[1:]:
            raise ValueError(f"{path}: {arr.shape[0]} x {arr.shape[1]}, the frames before it are {out.shape[1]} x {out.shape[2]}")
        out[i] = arr
    return out


def load_frames(image_root: str, height: int, width: int, *, n_view: int, n_frame: int, device=None) -> FrameSet:
    """``load_images`` (simple_multi_image.py:192-222) into a ``FrameSet`` at ``height x width``; see the module docstring for the refusals and
    for what is claimed of the resize."""
    n_view, n_frame, height, width = int(n_view), int(n_frame), int(height), int(width)
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"load_frames: device {device}: the frames are unpacked on the GPU (no CPU fallback)")
    host = decode_frames(image_root, count=n_view * n_frame)
    k = reduction_factor(host.shape[1], host.shape[2], height, width)
    src = torch.from_numpy(host).to(device)
    return FrameSet(src if k == 1 else unpack_rgba8(src, k, out8=True)["out8"], n_view, n_frame)


def test_renders(field, gaussians, cameras, bg, *, do_guidance: bool, chunk: int = 16) -> torch.Tensor:
    """``uint8 [B, H, W, 4]``: every camera of ``cameras`` (a ``cameras.CameraBatch``: ``testset_cameras``, ``orbit_cameras``,
    ``data_view_cameras``) rendered as ``test_step`` renders it (no gradient, ``do_guidance`` as the stage's ``load_guidance``) and packed as it
    quantises it.  ``chunk`` images go through one ``render_batch`` call and are packed into the result at once: no fp32 image of the whole
    set exists."""
    from .stage4d import render_batch
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk}: expected >= 1")
    B = cameras.c2w.shape[0]
    out = torch.empty(B, cameras.height, cameras.width, 4, dtype=torch.uint8, device=cameras.c2w.device)
    with torch.no_grad():
        for start in range(0, B, chunk):
            stop = min(start + chunk, B)
            r = render_batch(field, gaussians, None, None, None, None, None, bg, do_guidance=bool(do_guidance),
                             cameras=cameras.take(range(start, stop)))
            pack_rgba8(r["image"], r["alpha"], out=out[start:stop])
    return out


test_renders.__test__ = False      # a public name of the reference's vocabulary, not a test for pytest to collect


def render_paths(count: int, *, n_frame: int, test_option: str) -> List[str]:
    """The path of test image i under the save directory, for i in ``range(count)`` (animate3d.py:448-462)."""
    n_frame = int(n_frame)
    if test_option == "testset":
        return [os.path.join("images", f"elv_{i // (n_frame * 4)}_azi_{(i // n_frame) % 4}", f"{i % n_frame}.png") for i in range(count)]
    if test_option == "four_view":
        return [os.path.join("images", f"{i}.png") for i in range(count)]
    raise ValueError(f"test_option {test_option} not supported")


def write_test_renders(save_dir: str, rgba8, *, n_frame: int, test_option: str) -> List[str]:
    """One RGBA PNG per image of ``rgba8 [B, H, W, 4]`` uint8 (a tensor, as ``test_renders`` returns it, or an array) in the reference's layout:
    ``"testset"``: ``images/elv_{i // (4 n_frame)}_azi_{(i // n_frame) % 4}/{i % n_frame}.png``; ``"four_view"``: ``images/{i}.png``, the folder
    the refine stage reads as its ``image_root``.  Returns the paths written, relative to ``save_dir``."""
    from PIL import Image
    host = rgba8.detach().cpu().numpy() if isinstance(rgba8, torch.Tensor) else np.asarray(rgba8)
    if host.dtype != np.uint8 or host.ndim != 4 or host.shape[3] != 4:
        raise ValueError(f"rgba8: expected uint8 [B, H, W, 4], got {host.dtype} {list(host.shape)}")
    paths = render_paths(host.shape[0], n_frame=n_frame, test_option=test_option)
    for img, rel in zip(host, paths):
        path = os.path.join(save_dir, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(img).save(path)
    return paths


def write_trajectory(save_dir: str, trajectory) -> List[str]:
    """``mesh_trajectory/{t}.npy`` for every frame of ``stage4d.vertex_trajectory``'s ``[T, N, 3]`` (animate3d.py:465-471).  Returns the paths
    written, relative to ``save_dir``."""
    host = trajectory.detach().cpu().numpy() if isinstance(trajectory, torch.Tensor) else np.asarray(trajectory)
    if host.ndim != 3 or host.shape[2] != 3:
        raise ValueError(f"trajectory: expected [T, N, 3], got {list(host.shape)}")
    folder = os.path.join(save_dir, "mesh_trajectory")
    os.makedirs(folder, exist_ok=True)
    paths = [os.path.join("mesh_trajectory", f"{t}.npy") for t in range(host.shape[0])]
    for frame, rel in zip(host, paths):
        np.save(os.path.join(save_dir, rel), frame)
    return paths
