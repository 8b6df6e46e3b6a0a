"""The cameras of the 4-D stage: the guidance sampler, the data views and the evaluation sets, on the gfx950 kernels of
csrc/camera_batch.hip.

The reference makes ``batch["random_camera"]`` with ``HybridRandomCameraIterableDataset.collate`` (custom/threestudio-animate3d/data/
uncond_hybrid.py:188-423), the cameras of the reconstruction images with ``SimpleMultiImageDataBase.setup`` (data/simple_multi_image.py:
91-131, 167) and the validation / test cameras with ``HybridRandomCameraDataset`` / ``HybridRandomCameraTestDataset`` (uncond_hybrid.py:
426-558, 560-700), all on the CPU, with ``rays_o`` / ``rays_d [B, H, W, 3]`` that the Gaussian renderer never reads.  This module makes
the same cameras on the device, one launch per batch, together with the rasterizer's inputs, which ``stage4d.render_batch`` otherwise
recovers from ``c2w`` with two solver calls and a ``torch.unique``.  fp32 at the interface; the kernels compute in fp64 and round once.
CPU tensors raise, there is no torch fallback.

``CameraBatch``: ``c2w [B, 4, 4]``, ``fovy [B]`` (radians), ``w2c`` / ``full_proj [B, 4, 4]``, ``campos [B, 3]``, ``tanfov [B]`` (what
``rasterize_gaussians`` takes as ``viewmatrix``, ``projmatrix``, ``campos``, ``tanfovx`` = ``tanfovy``; znear 0.1, zfar 100), ``elevation``
/ ``azimuth`` (degrees) / ``camera_distances [B]`` where the cameras were made from them, and on the host ``height``, ``width``,
``frame_ids`` (the frame of every image) and ``frame_times`` (the timestamp of every frame id).  ``frames [T]`` (the distinct timestamps,
ascending), ``image_to_time [B]`` and ``timestamps [B, 1]`` are built from the host tuples without reading the device; they hold what
``stage4d.frames_of_images`` finds in ``timestamps``.  ``take(index)`` is the sub-batch of a host list of images.  Dict-style access gives
the reference batch's ``c2w``, ``fovy``, ``timestamps``, ``elevation``, ``azimuth``, ``camera_distances``, ``camera_positions``, ``height``,
``width``, so a ``CameraBatch`` stands where the reference's batch dict stands (``guidance(rgb, prompt_utils, **cameras)``); ``rays_o``,
``rays_d``, ``light_positions``, ``proj_mtx`` and ``mvp_mtx`` raise ``KeyError``: nothing in this package reads them.

``RandomCameraSampler(**cfg)`` takes ``HybridRandomCameraDataModuleConfig``'s names and defaults.  ``update_step(global_step)`` is
uncond_hybrid.py:161-186 (note that, as there, step 0 of a config with ``progressive_until: 0`` draws every camera at
``eval_elevation_deg`` and azimuth 0).  ``sample(generator, rng)`` draws the coin of :198 as ``rng.random() < 0.5`` on the host and then,
on the device and from ``generator``, in this order: ``torch.rand(R, 5)`` (per object: elevation, azimuth, fovy, distance, zoom),
``torch.rand(B, 3)`` (position perturbation), ``torch.randn(B, 6)`` (centre, up perturbation); ``R = batch_size // (n_view * total_frame)``.
The reference's light draws are not taken.  ``from_draws`` is the deterministic half.  ``timestamps`` has one row per image; the
reference's has ``n_view * total_frame`` rows whatever the batch size (:400-404), the same thing for the one object per step of every
released config.

``data_view_cameras``, ``orbit_cameras`` and ``testset_cameras`` are the three fixed sets; ``CameraBatch.from_c2w`` takes cameras that come
from elsewhere.  Out of scope: rays, lights, the GL ``proj_mtx`` / ``mvp_mtx``, image loading."""
from __future__ import annotations

import bisect
import ctypes
import math
import random
from dataclasses import dataclass, replace
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from .f32_stage import launch, require_f32_cuda, require_shape
from .hip_ops import _p

ZNEAR, ZFAR = 0.1, 100.0         # render_batch's planes (stage4d.py)
DEG = math.pi / 180.0
BATCH_KEYS = ("c2w", "fovy", "timestamps", "elevation", "azimuth", "camera_distances", "camera_positions", "height", "width")
NOT_BUILT = ("rays_o", "rays_d", "light_positions", "proj_mtx", "mvp_mtx")
# HybridRandomCameraDataModuleConfig's fields that only rays, lights and the evaluation sets read: accepted, so that a released config
# can be passed whole, and not used by the sampler
UNUSED_CFG = ("eval_height", "eval_width", "eval_batch_size", "n_val_views", "n_test_views", "light_position_perturb", "light_distance_range",
              "eval_camera_distance", "eval_fovy_deg", "light_sample_strategy", "batch_uniform_azimuth", "rays_d_normalize")


def _to_device(values, dtype, device) -> torch.Tensor:
    """A small host list as a device tensor, through pinned memory: the copy does not wait for the device."""
    host = torch.tensor(values, dtype=dtype)
    device = torch.device(device)
    if device.type != "cuda":
        return host
    return host.pin_memory().to(device, non_blocking=True)


def frame_times(total_frame: int) -> Tuple[float, ...]:
    """``torch.linspace(-1, 1, total_frame)`` in fp32 on the host, as the reference's data modules compute it."""
    return tuple(torch.linspace(-1, 1, steps=int(total_frame)).tolist())


def frame_structure(frame_ids: Sequence[int]) -> Tuple[List[int], List[int]]:
    """(the distinct frame ids ascending, for every image the position of its frame among them)."""
    distinct = sorted(set(frame_ids))
    rank = {f: i for i, f in enumerate(distinct)}
    return distinct, [rank[f] for f in frame_ids]


@dataclass(frozen=True, eq=False)
class CameraBatch(Mapping):
    c2w: torch.Tensor
    fovy: torch.Tensor
    w2c: torch.Tensor
    full_proj: torch.Tensor
    campos: torch.Tensor
    tanfov: torch.Tensor
    height: int
    width: int
    frame_ids: Tuple[int, ...]
    frame_times: Tuple[float, ...]
    elevation: Optional[torch.Tensor] = None
    azimuth: Optional[torch.Tensor] = None
    camera_distances: Optional[torch.Tensor] = None

    def __post_init__(self):
        if len(self.frame_ids) != self.c2w.shape[0]:
            raise ValueError(f"frame_ids: {len(self.frame_ids)} entries for {self.c2w.shape[0]} cameras")
        if self.frame_ids and not 0 <= min(self.frame_ids) <= max(self.frame_ids) < len(self.frame_times):
            raise ValueError(f"frame_ids: values must lie in [0, {len(self.frame_times)})")
        object.__setattr__(self, "_cache", {})

    # ---- the frame structure, from the host tuples

    def _cached(self, name, make):
        if name not in self._cache:
            self._cache[name] = make()
        return self._cache[name]

    @property
    def frames(self) -> torch.Tensor:
        """``[T]`` fp32: the distinct timestamps, ascending (``deform_gaussians``' ``timestamps``)."""
        return self._cached("frames", lambda: _to_device([self.frame_times[f] for f in frame_structure(self.frame_ids)[0]], torch.float32,
                                                         self.c2w.device))

    @property
    def image_to_time(self) -> torch.Tensor:
        """``[B]`` int64: the row of ``frames`` every image holds."""
        return self._cached("image_to_time", lambda: _to_device(frame_structure(self.frame_ids)[1], torch.int64, self.c2w.device))

    @property
    def image_plan(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(img_list [B], img_start [T + 1])`` int32: the images stable-sorted by frame and the first sorted position of every frame,
        ``deform_gaussians``' ``image_plan``, counted here on the host."""
        def make():
            distinct, i2t = frame_structure(self.frame_ids)
            order = sorted(range(len(i2t)), key=i2t.__getitem__)
            starts = [sum(1 for t in i2t if t < k) for k in range(len(distinct) + 1)]
            packed = _to_device(order + starts, torch.int32, self.c2w.device)
            return packed[:len(order)], packed[len(order):]
        return self._cached("image_plan", make)

    @property
    def timestamps(self) -> torch.Tensor:
        """``[B, 1]`` fp32, as the reference's batch carries them."""
        return self._cached("timestamps", lambda: _to_device([[self.frame_times[f]] for f in self.frame_ids], torch.float32, self.c2w.device))

    @property
    def camera_positions(self) -> torch.Tensor:
        return self.campos

    def __len__(self):                                  # Mapping: the number of keys; the number of cameras is c2w.shape[0]
        return sum(1 for _ in self)

    def __iter__(self):
        return (key for key in BATCH_KEYS if getattr(self, key) is not None)

    def __eq__(self, other):                            # a batch is its tensors: identity, not Mapping's item-wise comparison
        return self is other

    __hash__ = object.__hash__

    def __getitem__(self, key):
        if key in NOT_BUILT:
            raise KeyError(f"{key}: not built. The Gaussian renderer reads c2w and fovy only; rays, lights and the GL projection matrices "
                           "of the reference's batch are never read in this package")
        if key not in BATCH_KEYS:
            raise KeyError(key)
        value = getattr(self, key)
        if value is None:
            raise KeyError(f"{key}: this batch was made from c2w matrices, which carry no {key}")
        return value

    def take(self, index: Sequence[int]) -> "CameraBatch":
        """The images ``index`` (a host list of ints, repeats allowed, in that order) as a batch with its own frame structure."""
        index = [int(i) for i in index]
        B = self.c2w.shape[0]
        if any(not 0 <= i < B for i in index):
            raise IndexError(f"take: indices must lie in [0, {B})")
        idx = _to_device(index, torch.int64, self.c2w.device)
        pick = lambda t: None if t is None else t.index_select(0, idx)        # noqa: E731
        return replace(self, c2w=pick(self.c2w), fovy=pick(self.fovy), w2c=pick(self.w2c), full_proj=pick(self.full_proj),
                       campos=pick(self.campos), tanfov=pick(self.tanfov), elevation=pick(self.elevation), azimuth=pick(self.azimuth),
                       camera_distances=pick(self.camera_distances), frame_ids=tuple(self.frame_ids[i] for i in index))

    @classmethod
    def from_c2w(cls, c2w: torch.Tensor, fovy: torch.Tensor, timestamps: Sequence[float], height: int, width: int) -> "CameraBatch":
        """Cameras that come from elsewhere: ``c2w [B, 4, 4]``, ``fovy [B]`` in radians, the per-image ``timestamps`` given on the host.
        What ``get_cam_info_gaussian`` computes with a solver, by the adjugate in fp64."""
        require_shape("c2w", c2w, ("B", 4, 4), non_empty=True)
        B = c2w.shape[0]
        require_shape("fovy", fovy, (B,))
        require_f32_cuda("c2w", c2w)
        require_f32_cuda("fovy", fovy)
        times = [float(torch.tensor(float(t), dtype=torch.float32)) for t in timestamps]
        if len(times) != B:
            raise ValueError(f"timestamps: {len(times)} values for {B} cameras")
        distinct = sorted(set(times))
        c2w, fovy = c2w.detach().contiguous(), fovy.detach().contiguous()
        out = _outputs(B, c2w.device, with_c2w=False)
        launch("a3d_cameras_from_c2w_f32", c2w.device, B, _p(c2w), _p(fovy), ZNEAR, ZFAR, *(_p(t) for t in out))
        return cls(c2w, fovy, *out, int(height), int(width), tuple(distinct.index(t) for t in times), tuple(distinct))


def _outputs(B: int, device, with_c2w: bool = True):
    shapes = ([(B, 4, 4)] if with_c2w else []) + [(B, 4, 4), (B, 4, 4), (B, 3), (B,)]
    return [torch.empty(s, dtype=torch.float32, device=device) for s in shapes]


def _cuda(device) -> torch.device:
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"cameras are made on a CUDA device, got {device} (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _spherical(elevation_deg: Sequence[float], azimuth_deg: Sequence[float], distance: Sequence[float], fovy_deg: Sequence[float],
               frame_ids: Sequence[int], total_frame: int, height: int, width: int, device) -> CameraBatch:
    """The look-at cameras on the sphere with centre 0 and up +z, from host lists in degrees (converted in the kernel, in fp64)."""
    device = _cuda(device)
    B = len(elevation_deg)
    if not (len(azimuth_deg) == len(distance) == len(fovy_deg) == len(frame_ids) == B) or B == 0:
        raise ValueError(f"{B} elevations, {len(azimuth_deg)} azimuths, {len(distance)} distances, {len(fovy_deg)} fovs, "
                         f"{len(frame_ids)} frames: expected one non-empty length")
    host = torch.tensor([list(elevation_deg), list(azimuth_deg), list(distance), list(fovy_deg)], dtype=torch.float32)
    radians = (host[3].double() * DEG).float()                    # of the fp32 degrees the kernel reads, rounded once
    packed = _to_device(torch.cat([host, radians[None]]).tolist(), torch.float32, device)
    elev, azim, dist, fdeg, fovy = packed.unbind(0)
    out = _outputs(B, device)
    launch("a3d_cameras_spherical_f32", device, B, _p(elev), _p(azim), _p(dist), _p(fdeg), None, DEG, ZNEAR, ZFAR, *(_p(t) for t in out))
    return CameraBatch(out[0], fovy, *out[1:], int(height), int(width), tuple(int(f) for f in frame_ids), frame_times(total_frame),
                       elevation=elev, azimuth=azim, camera_distances=dist)


# ---- the guidance sampler (uncond_hybrid.py:114-423)

def _as_list(value) -> List[int]:
    return [int(value)] if isinstance(value, int) else [int(v) for v in value]


class RandomCameraSampler:
    """``HybridRandomCameraIterableDataset`` without rays and lights; see the module docstring."""

    def __init__(self, height=64, width=64, batch_size=1, resolution_milestones: Sequence[int] = (), elevation_range=(-10, 90),
                 azimuth_range=(-180, 180), camera_distance_range=(1, 1.5), fovy_range=(40, 70), camera_perturb: float = 0.1,
                 center_perturb: float = 0.2, up_perturb: float = 0.02, eval_elevation_deg: float = 15.0, progressive_until: int = 0,
                 relative_radius: bool = True, n_view: int = 4, zoom_range=(1.0, 1.0), total_frame: int = 8, device=None, **unused):
        unknown = sorted(set(unused) - set(UNUSED_CFG))
        if unknown:
            raise TypeError(f"RandomCameraSampler: unknown config names {unknown}")
        self.heights, self.widths, self.batch_sizes = _as_list(height), _as_list(width), _as_list(batch_size)
        if not len(self.heights) == len(self.widths) == len(self.batch_sizes):
            raise ValueError("height, width and batch_size: ints, or lists of one length")
        if len(self.heights) == 1:                                # the reference ignores the milestones then, with a warning
            self.resolution_milestones = [-1]
        else:
            if len(self.heights) != len(resolution_milestones) + 1:
                raise ValueError(f"{len(self.heights)} sizes need {len(self.heights) - 1} resolution_milestones, got {len(resolution_milestones)}")
            self.resolution_milestones = [-1] + [int(m) for m in resolution_milestones]
        self.n_view, self.total_frame = int(n_view), int(total_frame)
        if self.n_view < 1 or self.total_frame < 1:
            raise ValueError(f"n_view = {n_view}, total_frame = {total_frame}: expected positive ints")
        for size in self.batch_sizes:
            if size <= 0 or size % (self.n_view * self.total_frame) != 0:
                raise ValueError(f"batch_size ({size}) must be a positive multiple of n_view * total_frame ({self.n_view * self.total_frame})")
        pair = lambda r: (float(r[0]), float(r[1]))               # noqa: E731
        self.cfg_elevation_range, self.cfg_azimuth_range = pair(elevation_range), pair(azimuth_range)
        self.camera_distance_range, self.fovy_range, self.zoom_range = pair(camera_distance_range), pair(fovy_range), pair(zoom_range)
        self.camera_perturb, self.center_perturb, self.up_perturb = float(camera_perturb), float(center_perturb), float(up_perturb)
        self.eval_elevation_deg, self.progressive_until = float(eval_elevation_deg), int(progressive_until)
        self.relative_radius = bool(relative_radius)
        self.device = device
        self.height, self.width, self.batch_size = self.heights[0], self.widths[0], self.batch_sizes[0]
        self.elevation_range, self.azimuth_range = list(self.cfg_elevation_range), list(self.cfg_azimuth_range)
        self._frame_times = frame_times(self.total_frame)

    def update_step(self, global_step: int):
        """uncond_hybrid.py:161-186: the size of the schedule's current stage and the progressive elevation / azimuth ranges."""
        size_ind = bisect.bisect_right(self.resolution_milestones, global_step) - 1
        self.height, self.width, self.batch_size = self.heights[size_ind], self.widths[size_ind], self.batch_sizes[size_ind]
        r = min(1.0, global_step / (self.progressive_until + 1))
        ev, er, ar = self.eval_elevation_deg, self.cfg_elevation_range, self.cfg_azimuth_range
        self.elevation_range = [(1 - r) * ev + r * er[0], (1 - r) * ev + r * er[1]]
        self.azimuth_range = [(1 - r) * 0.0 + r * ar[0], (1 - r) * 0.0 + r * ar[1]]

    def sample(self, generator: Optional[torch.Generator] = None, rng=random) -> CameraBatch:
        device = _cuda(self.device)
        elev_mode = 0 if rng.random() < 0.5 else 1
        B = self.batch_size
        R = B // (self.n_view * self.total_frame)
        obj = torch.rand(R, 5, generator=generator, device=device)
        pert_u = torch.rand(B, 3, generator=generator, device=device)
        pert_n = torch.randn(B, 6, generator=generator, device=device)
        return self.from_draws(obj, pert_u, pert_n, elev_mode)

    def from_draws(self, obj: torch.Tensor, pert_u: torch.Tensor, pert_n: torch.Tensor, elev_mode: int) -> CameraBatch:
        """``collate`` on explicit draws: ``obj [R, 5]`` and ``pert_u [B, 3]`` uniform, ``pert_n [B, 6]`` normal, ``elev_mode`` 0 (uniform
        in degrees: the coin fell below 0.5) or 1 (uniform on the sphere); ``B = R * n_view * total_frame``, at the current size."""
        require_shape("obj", obj, ("R", 5), non_empty=True)
        R = obj.shape[0]
        B = R * self.n_view * self.total_frame
        require_shape("pert_u", pert_u, (B, 3))
        require_shape("pert_n", pert_n, (B, 6))
        for name, t in (("obj", obj), ("pert_u", pert_u), ("pert_n", pert_n)):
            require_f32_cuda(name, t)
        if elev_mode not in (0, 1):
            raise ValueError(f"elev_mode = {elev_mode}: 0 (uniform in degrees) or 1 (uniform on the sphere)")
        device = obj.device
        obj, pert_u, pert_n = obj.detach().contiguous(), pert_u.detach().contiguous(), pert_n.detach().contiguous()
        ranges = (ctypes.c_double * 10)(*self.elevation_range, *self.azimuth_range, *self.fovy_range, *self.camera_distance_range,
                                        *self.zoom_range)
        out = _outputs(B, device)
        elev, azim, fovy, dist = (torch.empty(B, dtype=torch.float32, device=device) for _ in range(4))
        launch("a3d_cameras_random_f32", device, R, self.n_view, self.total_frame, _p(obj), _p(pert_u), _p(pert_n), ranges, int(elev_mode),
               int(self.relative_radius), self.camera_perturb, self.center_perturb, self.up_perturb, ZNEAR, ZFAR, *(_p(t) for t in out),
               _p(elev), _p(azim), _p(fovy), _p(dist))
        frame_ids = tuple(b % self.total_frame for b in range(B))          # object-major, then view, then frame (:399-404)
        return CameraBatch(out[0], fovy, *out[1:], self.height, self.width, frame_ids, self._frame_times, elevation=elev, azimuth=azim,
                           camera_distances=dist)


# ---- the fixed sets

def _per_image(name: str, value, B: int) -> List[float]:
    """The reference's scalar-or-list handling (simple_multi_image.py:91-97): a number is repeated over the images, a list is per image."""
    if isinstance(value, (int, float)):
        return [float(value)] * B
    values = [float(v) for v in value]
    if len(values) != B:
        raise ValueError(f"{name}: a number, or a list of n_view * total_frame = {B} values, got {len(values)}")
    return values


def data_view_cameras(default_elevation_deg=0.0, default_azimuth_deg: Sequence[float] = (), default_camera_distance=1.2, default_fovy_deg=60.0,
                      n_view: int = 4, total_frame: int = 8, height: int = 96, width: int = 96, device=None) -> CameraBatch:
    """The cameras of the ``n_view * total_frame`` reconstruction images, view-major, with ``timestamps = linspace(-1, 1, total_frame)`` per
    view (simple_multi_image.py:91-131, 167).  ``default_azimuth_deg``: one value per view (repeated over its frames, :94-95) or one per
    image.  Where the reference's list branches cannot run (an int ``default_fovy_deg`` becomes an uninitialised tensor, a list distance
    reads a config name that does not exist) a number is a number and a list is per image.  An elevation of +-90 degrees makes the
    look-at singular (``lookat`` parallel to ``up``): ``ValueError``."""
    n_view, F = int(n_view), int(total_frame)
    B = n_view * F
    azimuth = [float(a) for a in default_azimuth_deg]
    if len(azimuth) // n_view < F:
        if len(azimuth) != n_view:
            raise ValueError(f"default_azimuth_deg: one value per view ({n_view}) or per image ({B}), got {len(azimuth)}")
        azimuth = [a for a in azimuth for _ in range(F)]
    elif len(azimuth) != B:
        raise ValueError(f"default_azimuth_deg: one value per view ({n_view}) or per image ({B}), got {len(azimuth)}")
    elevation = _per_image("default_elevation_deg", default_elevation_deg, B)
    if any(abs(abs(e) - 90.0) < 1e-6 for e in elevation):
        raise ValueError("default_elevation_deg = +-90: the look-at with up = +z is singular there")
    return _spherical(elevation, azimuth, _per_image("default_camera_distance", default_camera_distance, B),
                      _per_image("default_fovy_deg", default_fovy_deg, B), [f for _ in range(n_view) for f in range(F)], F, height, width, device)


def orbit_cameras(cfg: Dict, split: str, device=None) -> CameraBatch:
    """``HybridRandomCameraDataset(cfg, split)``, every item: ``n_val_views`` (``"val"``) or ``n_test_views`` cameras on the circle at
    ``eval_elevation_deg``; item i holds camera ``(i // total_frame) * total_frame`` at frame ``i % total_frame`` (:533-535).  ``cfg``: the
    reference's names, ``HybridRandomCameraDataModuleConfig``'s defaults."""
    n = int(cfg.get("n_val_views", 1) if split == "val" else cfg.get("n_test_views", 120))
    F = int(cfg.get("total_frame", 8))
    azimuth = (torch.linspace(0, 360.0, n + 1)[:n] if split == "val" else torch.linspace(0, 360.0, n)).tolist()
    held = [(i // F) * F for i in range(n)]
    return _spherical([float(cfg.get("eval_elevation_deg", 15.0))] * n, [azimuth[c] for c in held], [float(cfg.get("eval_camera_distance", 1.5))] * n,
                      [float(cfg.get("eval_fovy_deg", 70.0))] * n, [i % F for i in range(n)], F, cfg.get("eval_height", 512),
                      cfg.get("eval_width", 512), device)


def testset_cameras(cfg: Dict, split: str = "test", device=None) -> CameraBatch:
    """``HybridRandomCameraTestDataset(cfg, "test")``, every item: ``len(eval_elevation_deg) * len(eval_azimuth_deg[0]) * total_frame`` of
    them, item i holding camera ``i // total_frame`` (elevation-major) at frame ``i % total_frame``: ``test_step``'s ``elv_index`` /
    ``azi_index`` / ``frame_index`` (systems/animate3d.py:448-451).  The reference builds this set for ``"test"`` only."""
    if split != "test":
        raise ValueError(f"split = {split!r}: the reference builds the test set's cameras for 'test' only (validation uses orbit_cameras)")
    elevations = [float(e) for e in cfg.get("eval_elevation_deg", (15.0, 0.0, 30.0))]
    azimuths = [[float(a) for a in row] for row in cfg.get("eval_azimuth_deg", ((0.0, 90.0, 180.0, 270.0), (30.0, 120.0, 210.0, 300.0),
                                                                                  (-45.0, 45.0, 135.0, 225.0)))]
    if len(azimuths) != len(elevations) or any(len(row) != len(azimuths[0]) for row in azimuths):
        raise ValueError("eval_azimuth_deg: one row of equal length per entry of eval_elevation_deg")
    F = int(cfg.get("total_frame", 32))
    cams = [(e, a) for e, row in zip(elevations, azimuths) for a in row]
    n = len(cams) * F
    return _spherical([cams[i // F][0] for i in range(n)], [cams[i // F][1] for i in range(n)], [float(cfg.get("eval_camera_distance", 1.5))] * n,
                      [float(cfg.get("eval_fovy_deg", 70.0))] * n, [i % F for i in range(n)], F, cfg.get("eval_height", 512),
                      cfg.get("eval_width", 512), device)
