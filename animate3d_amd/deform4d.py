"""Differentiable 4-D Gaussian deformation field on the gfx950 kernels of csrc/deform4d.hip: every frame of a step in one call.

The reference optimises, in its 4-D stage, a two-scale K-Planes / HexPlane grid plus five small MLPs (``Gaussian4DModel``,
custom/threestudio-animate3d/geometry/gaussian_4d.py) and evaluates them once per image inside the Python loop of
gaussian_batch_renderer_4d.py:27-60.  ``deform_gaussians`` / ``HexPlaneDeformation`` are that field; their outputs feed
``splat.rasterize_gaussians`` directly.

Contract (all arithmetic fp32)

Inputs: ``xyz [N, 3]``, ``scaling [N, 3]`` (log-scale), ``rotation [N, 4]`` (r, x, y, z, un-normalised), ``timestamps [T]`` in [-1, 1],
optional ``image_to_time [B]`` (int64 or int32 index into ``timestamps``; default identity, B = T).  Any view is accepted: what is not
contiguous, or (``rotation``, the ``rotations`` cotangent) does not start on the 16 bytes the kernels read at a time, is copied first.
Parameters: ``grids[s][p]`` of shape ``[1, C, reso[b], reso[a]]`` for the plane over coordinates ``(a, b)`` in
``itertools.combinations(range(4), 2)`` order (the axis order is reversed, gaussian_4d.py:162-167); ``delta_xyz_network``,
``delta_rot_network``, ``delta_scaling_network`` and, with ``use_global_trans``, ``global_rot_network``, ``global_trans_network``: each
``layers.0.weight [32, 32]``, ReLU, ``layers.2.weight [k, 32]``, no bias (threestudio/models/networks.py:214-251).

Per frame f and Gaussian n (gaussian_4d.py:450-548, diff_gaussian_rasterizer_advanced_4d.py:77-135):

1. ``pts = (x, y, z, t_f)``.  Per scale s the feature is the product over the six planes of the bilinear sample at ``pts[(a, b)]``
   (``align_corners=True``, ``padding_mode="border"``; gaussian_4d.py:39-64); ``hidden`` = concatenation over the scales (32 values).
2. With ``use_global_trans``: ``g`` = mean over n of ``hidden``; ``angles = sigmoid(global_rot_network(g)) * 2 pi - pi``,
   ``R = Rz Ry Rx`` (geometry/utils.py:135-169); ``trans = sigmoid(global_trans_network(g)) * 2 - 1``; ``xyz' = R xyz + trans``;
   ``rot' = extract_rotation_torch(R @ build_rotation(rotation))`` (utils.py:33-60, 73-132, with its four-way branch, which fixes the sign
   of the quaternion, and its normalisation).
3. ``means = xyz' + delta_xyz_network(hidden)``; ``rotations = normalize(rot' + delta_rot_network(hidden))``;
   ``scales = exp(scaling + delta_scaling_network(hidden))``, or ``exp(scaling)`` with ``deform_scales=False`` (the reference's
   ``do_guidance=False`` path).
4. A frame whose timestamp is exactly -1 is the first frame: unless ``first_frame_trainable`` it bypasses 1-3 (``means = xyz``,
   ``scales = exp(scaling)``, ``rotations = normalize(rotation)``).

``scaling_activation`` / ``rotation_activation`` live in the threestudio-3dgs plugin, which the reference tree does not contain; they are
taken to be the standard 3DGS ``torch.exp`` and ``F.normalize``.

Outputs ``means [B, N, 3]``, ``scales [B, N, 3]``, ``rotations [B, N, 4]``; image b holds frame ``image_to_time[b]``, in the ``(b n f)`` image
order ``rasterize_gaussians`` and ``sds.sds_guidance_loss`` expect.

Gradients: every grid plane, every MLP weight, ``scaling``, ``rotation``: the exact derivative of the forward above (ReLU and the border
clamp have zero gradient where inactive; each ``extract_rotation_torch`` branch is differentiated as written).  ``xyz.requires_grad``
raises ``NotImplementedError`` (the reference keeps ``_xyz`` as a buffer in this stage, gaussian_4d.py:262-265); ``timestamps`` gets none.
The gradient of a frame shown in several images is the sum over those images in ascending image order.  No atomics: two backward passes
are bit-identical and parameter gradients do not depend on how images map to frames.  The plane gradients are computed in gather form
over a plan (per plane, the Gaussians stable-sorted by cell) that depends on ``xyz`` only: ``HexPlaneDeformation`` caches it, keyed on
``xyz``'s identity (a weak reference), storage and version.

Kernel support: 2 scales x 16 channels (32 hidden features), 32 neurons, one hidden layer, any plane resolutions >= 2; everything else
raises ``NotImplementedError``.  CPU tensors raise: there is no torch fallback.
"""
from __future__ import annotations

import ctypes
import itertools
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from .f32_stage import TensorKeyed, gather_plan, launch, require_f32_cuda
from .hip_ops import _p, load_library

PAIRS = tuple(itertools.combinations(range(4), 2))          # (x,y) (x,z) (x,t) (y,z) (y,t) (z,t)
CHANNELS, SCALES, NEURONS, NET_FLOATS = 16, 2, 32, 1152
LOCAL_NETS = ("delta_xyz_network", "delta_rot_network", "delta_scaling_network")
GLOBAL_NETS = ("global_rot_network", "global_trans_network")
NET_OUT = {"delta_xyz_network": 3, "delta_rot_network": 4, "delta_scaling_network": 3, "global_rot_network": 3, "global_trans_network": 3}


def plane_dims(grid_size: Sequence[Sequence[int]]):
    """Per plane k = 6 s + p: (W, H) = (reso[a], reso[b]) of pair (a, b)."""
    return [(int(reso[a]), int(reso[b])) for reso in grid_size for a, b in PAIRS]


def plane_cells(grid_size: Sequence[Sequence[int]]):
    """Cells per plane of the binning plan: (W - 1)(H - 1) for a spatial plane, W - 1 (the spatial axis) for a time plane."""
    return [(W - 1) if b == 3 else (W - 1) * (H - 1) for (W, H), (a, b) in zip(plane_dims(grid_size), PAIRS * len(grid_size))]


def _check_config(grid_size, n_grid_dims, n_neurons=NEURONS, n_hidden_layers=1):
    if len(grid_size) != SCALES:
        raise NotImplementedError(f"grid_size: {len(grid_size)} scales; the kernels support exactly {SCALES}")
    if any(len(r) != 4 for r in grid_size):
        raise NotImplementedError("grid_size: every scale needs four resolutions (x, y, z, t)")
    if any(int(v) < 2 for r in grid_size for v in r):
        raise NotImplementedError("grid_size: every resolution must be at least 2")
    if n_grid_dims != CHANNELS:
        raise NotImplementedError(f"n_grid_dims: {n_grid_dims}; the kernels support {CHANNELS} channels per scale")
    if n_neurons != NEURONS:
        raise NotImplementedError(f"n_neurons: {n_neurons}; the kernels support {NEURONS}")
    if n_hidden_layers != 1:
        raise NotImplementedError(f"n_hidden_layers: {n_hidden_layers}; the kernels support 1")


def _plane_desc(grid_size):
    dims = plane_dims(grid_size)
    offs, o = [], 0
    for W, H in dims:
        offs.append(o)
        o += W * H * CHANNELS
    desc = (ctypes.c_int64 * 36)(*offs, *[d[0] for d in dims], *[d[1] for d in dims])
    return desc, offs, o


def build_plan(cells: torch.Tensor, n_cells: Sequence[int]):
    """cells [12, N] -> (order [12, N] int32: Gaussians stable-sorted by cell; starts: per plane cells + 1 first positions, back to back)."""
    orders, starts = zip(*(gather_plan(cells[k], nc) for k, nc in enumerate(n_cells)))
    return torch.stack(orders).contiguous(), torch.cat(starts).contiguous()


def _grid_key(grid_size):
    return tuple(tuple(int(v) for v in r) for r in grid_size)


class BinningPlan(TensorKeyed):
    """The gather plan of the plane gradients for one ``xyz``; ``matches`` tells whether it still describes a tensor."""

    def __init__(self, xyz: torch.Tensor, grid_size):
        desc, _, _ = _plane_desc(grid_size)
        N = xyz.shape[0]
        x = xyz.detach().contiguous()
        cells = torch.empty(12, N, dtype=torch.int32, device=xyz.device)
        launch("a3d_dg_cells_f32", xyz.device, N, _p(x), desc, _p(cells))
        self.cells = cells                                       # [12, N] as a3d_dg_cells_f32 assigned them
        self.order, self.starts = build_plan(cells, plane_cells(grid_size))
        self.bind(xyz, _grid_key(grid_size))

    def matches(self, xyz, grid_size) -> bool:
        return super().matches(xyz, _grid_key(grid_size))


def _pack_weights(nets: Dict[str, Sequence[torch.Tensor]], device) -> torch.Tensor:
    w = torch.zeros(5, NET_FLOATS, dtype=torch.float32, device=device)
    for i, name in enumerate(LOCAL_NETS + GLOBAL_NETS):
        if name in nets:
            w0, w2 = nets[name]
            w[i, :1024] = w0.detach().reshape(-1)
            w[i, 1024:1024 + w2.numel()] = w2.detach().reshape(-1)
    return w


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """``t`` (contiguous) where the kernels may read it 16 bytes at a time: itself, or a copy when it is a view that starts elsewhere (a
    parameter inside a flat buffer, behind a number of floats that is no multiple of four)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _DeformGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, rotation, xyz, timestamps, image_to_time, image_plan, grid_size, flags, plan, net_names, *params):
        ctx.set_materialize_grads(False)                         # an output outside the loss arrives in backward as None, not as zeros
        lib, dev = load_library(), xyz.device
        N, T = xyz.shape[0], timestamps.shape[0]
        grids, weights = params[:12], params[12:]
        desc, offs, total = _plane_desc(grid_size)
        packed = torch.cat([g.detach()[0].permute(1, 2, 0).reshape(-1) for g in grids]).contiguous()        # texel-major [H][W][16] per plane
        nets = {name: (weights[2 * i], weights[2 * i + 1]) for i, name in enumerate(net_names)}
        w = _pack_weights(nets, dev)
        i2t = torch.arange(T, device=dev) if image_to_time is None else image_to_time.to(dev).long()
        B = i2t.shape[0]
        if image_plan is not None:                               # counted on the host by the caller: nothing is read back here
            img_list, img_start = image_plan
        else:
            img_list = torch.argsort(i2t, stable=True).to(torch.int32)
            img_start = torch.zeros(T + 1, dtype=torch.int32, device=dev)
            img_start[1:] = torch.cumsum(torch.bincount(i2t, minlength=T), 0)
        x, sc, ts = xyz.detach().contiguous(), scaling.detach().contiguous(), timestamps.detach().contiguous()
        ro = _aligned16(rotation.detach().contiguous())
        f32 = dict(dtype=torch.float32, device=dev)
        sp = torch.empty(N, 32, **f32)
        gmean = glob = mpart = None
        if flags & 1:
            mpart = torch.empty(T, int(lib.a3d_dg_mean_partials(N)), 32, **f32)
            gmean, glob = torch.zeros(T, 32, **f32), torch.zeros(T, 12, **f32)
        means, scales, rots = torch.empty(B, N, 3, **f32), torch.empty(B, N, 3, **f32), torch.empty(B, N, 4, **f32)
        launch("a3d_dg_forward_f32", dev, T, N, B, _p(x), _p(sc), _p(ro), _p(ts), _p(packed), desc, _p(w), flags, _p(img_start), _p(img_list),
               _p(sp), _p(mpart), _p(gmean), _p(glob), _p(means), _p(scales), _p(rots))
        ctx.save_for_backward(x, sc, ro, ts, packed, w, img_start, img_list, sp, gmean, glob, plan.order, plan.starts)
        ctx.meta = (T, N, B, flags, grid_size, offs, total, net_names, [g.shape for g in grids], [p.shape for p in weights])
        return means, scales, rots

    @staticmethod
    def backward(ctx, d_means, d_scales, d_rots):
        x, sc, ro, ts, packed, w, img_start, img_list, sp, gmean, glob, order, starts = ctx.saved_tensors
        T, N, B, flags, grid_size, offs, total, net_names, grid_shapes, weight_shapes = ctx.meta
        lib, dev = load_library(), x.device
        f32 = dict(dtype=torch.float32, device=dev)
        desc, _, _ = _plane_desc(grid_size)
        cot = [torch.zeros(B, N, k, **f32) if g is None else g.float().contiguous() for g, k in ((d_means, 3), (d_scales, 3), (d_rots, 4))]
        cot[2] = _aligned16(cot[2])
        ws = torch.empty(int(lib.a3d_dg_backward_ws_floats(T, N, desc)), **f32)
        d_grid, d_w = torch.empty(total, **f32), torch.empty(5, NET_FLOATS, **f32)
        d_scaling, d_rotation = torch.empty(N, 3, **f32), torch.empty(N, 4, **f32)
        launch("a3d_dg_backward_f32", dev, T, N, B, _p(x), _p(sc), _p(ro), _p(ts), _p(packed), desc, _p(w), flags, _p(img_start), _p(img_list),
               _p(sp), _p(gmean), _p(glob), _p(order), _p(starts), _p(cot[0]), _p(cot[1]), _p(cot[2]), _p(ws), _p(d_grid), _p(d_w),
               _p(d_scaling), _p(d_rotation))
        grads = []
        for off, shp in zip(offs, grid_shapes):
            _, C, H, W = shp
            grads.append(d_grid[off:off + H * W * C].view(H, W, C).permute(2, 0, 1).unsqueeze(0).contiguous())
        slot = {name: i for i, name in enumerate(LOCAL_NETS + GLOBAL_NETS)}
        for i, name in enumerate(net_names):
            k = NET_OUT[name]
            if name == "delta_scaling_network" and not flags & 2:
                grads += [torch.zeros(32, 32, **f32), torch.zeros(k, 32, **f32)]
                continue
            grads.append(d_w[slot[name], :1024].view(32, 32).clone())
            grads.append(d_w[slot[name], 1024:1024 + k * 32].view(k, 32).clone())
        return (d_scaling, d_rotation, None, None, None, None, None, None, None, None, *grads)


def deform_gaussians(xyz: torch.Tensor, scaling: torch.Tensor, rotation: torch.Tensor, timestamps: torch.Tensor, grids, networks, *,
                     image_to_time: Optional[torch.Tensor] = None, use_global_trans: bool = False, deform_scales: bool = True,
                     first_frame_trainable: bool = False, plan: Optional[BinningPlan] = None,
                     image_plan: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """``grids``: two sequences of six planes; ``networks``: {name: (layers.0.weight, layers.2.weight)} with the three ``delta_*`` networks
    and, for ``use_global_trans``, the two ``global_*`` ones.  Returns (means [B, N, 3], scales [B, N, 3], rotations [B, N, 4]).

    ``image_plan``: ``(img_list [B] int32, img_start [T + 1] int32)``, the images stable-sorted by frame and the first sorted position of
    every frame, for a caller that knows ``image_to_time`` on the host (``cameras.CameraBatch.image_plan``) and vouches for it.  Without
    it the two are counted from ``image_to_time`` on the device, which range-checks it and synchronises with the host."""
    for name, t in (("xyz", xyz), ("scaling", scaling), ("rotation", rotation), ("timestamps", timestamps)):
        require_f32_cuda(name, t)
    if xyz.requires_grad:
        raise NotImplementedError("xyz.requires_grad: the 4-D stage keeps the positions fixed; no gradient reaches the sampling coordinates")
    N = xyz.shape[0]
    if xyz.shape != (N, 3) or scaling.shape != (N, 3) or rotation.shape != (N, 4) or timestamps.dim() != 1:
        raise ValueError("expected xyz [N, 3], scaling [N, 3], rotation [N, 4], timestamps [T]")
    if len(grids) != SCALES or any(len(g) != 6 for g in grids):
        raise NotImplementedError(f"grids: the kernels support {SCALES} scales of six planes")
    flat = [p for g in grids for p in g]
    if any(p.shape[1] != CHANNELS for p in flat):
        raise NotImplementedError(f"n_grid_dims: the kernels support {CHANNELS} channels per scale")
    grid_size = []
    for g in grids:                          # plane (x,y) is [1, C, ry, rx], (z,t) is [1, C, rt, rz]
        grid_size.append((g[0].shape[3], g[0].shape[2], g[5].shape[3], g[5].shape[2]))
    grid_size = tuple(grid_size)
    _check_config(grid_size, CHANNELS)
    for (W, H), p in zip(plane_dims(grid_size), flat):
        if tuple(p.shape) != (1, CHANNELS, H, W):
            raise ValueError(f"plane of shape {tuple(p.shape)}: expected {(1, CHANNELS, H, W)}")
    names = LOCAL_NETS + (GLOBAL_NETS if use_global_trans else ())
    weights = []
    for name in names:
        if name not in networks:
            raise ValueError(f"networks: {name} is missing")
        w0, w2 = networks[name]
        if tuple(w0.shape) != (NEURONS, 32) or tuple(w2.shape) != (NET_OUT[name], NEURONS):
            raise NotImplementedError(f"{name}: the kernels support 32 -> {NEURONS} -> {NET_OUT[name]} with one hidden layer")
        weights += [w0, w2]
    if image_to_time is not None:
        if image_to_time.dim() != 1 or image_to_time.dtype not in (torch.int64, torch.int32):
            raise ValueError("image_to_time: a 1-D integer tensor of indices into timestamps")
    if image_plan is not None:
        B = timestamps.shape[0] if image_to_time is None else image_to_time.shape[0]
        img_list, img_start = image_plan
        for name, t, n in (("img_list", img_list, B), ("img_start", img_start, timestamps.shape[0] + 1)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (n,) and t.is_contiguous()):
                raise ValueError(f"image_plan: {name} must be a contiguous int32 CUDA tensor of shape [{n}]")
    if plan is None or not plan.matches(xyz, grid_size):
        plan = BinningPlan(xyz, grid_size)
    flags = (1 if use_global_trans else 0) | (2 if deform_scales else 0) | (4 if first_frame_trainable else 0)
    return _DeformGaussians.apply(scaling, rotation, xyz, timestamps, image_to_time, image_plan, grid_size, flags, plan, names, *flat, *weights)


class _MLP(nn.Module):
    """VanillaMLP with one hidden layer, ReLU, no bias (threestudio/models/networks.py:214-251): same parameter names."""

    def __init__(self, dim_in: int, dim_out: int, n_neurons: int):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(dim_in, n_neurons, bias=False), nn.ReLU(inplace=True), nn.Linear(n_neurons, dim_out, bias=False))
        nn.init.zeros_(self.layers[2].weight)                  # gaussian_4d.py:140-147

    def weights(self):
        return self.layers[0].weight, self.layers[2].weight


class HexPlaneDeformation(nn.Module):
    """The trainable parameters of ``Gaussian4DModel``'s deformation field with the reference's initialisation (gaussian_4d.py:101-174:
    time planes ones, the others U(0.1, 0.5), every ``layers.2.weight`` zero) and state-dict keys (``grids.{s}.{p}``,
    ``delta_xyz_network.layers.0.weight``, ...): ``load_state_dict(geometry.state_dict(), strict=False)`` binds a trained model."""

    def __init__(self, grid_size=((50, 50, 50, 8), (100, 100, 100, 16)), n_grid_dims: int = 16, use_global_trans: bool = False,
                 n_neurons: int = 32, n_hidden_layers: int = 1):
        super().__init__()
        grid_size = _grid_key(grid_size)
        _check_config(grid_size, n_grid_dims, n_neurons, n_hidden_layers)
        self.grid_size, self.use_global_trans = grid_size, bool(use_global_trans)
        self.grids = nn.ModuleList()
        for reso in grid_size:
            planes = nn.ParameterList()
            for a, b in PAIRS:
                p = nn.Parameter(torch.empty(1, n_grid_dims, reso[b], reso[a]))
                if b == 3:
                    nn.init.ones_(p)
                else:
                    nn.init.uniform_(p, a=0.1, b=0.5)
                planes.append(p)
            self.grids.append(planes)
        feat = n_grid_dims * len(grid_size)
        for name in LOCAL_NETS + (GLOBAL_NETS if use_global_trans else ()):
            setattr(self, name, _MLP(feat, NET_OUT[name], n_neurons))
        self._plan: Optional[BinningPlan] = None

    def plan_for(self, xyz: torch.Tensor) -> BinningPlan:
        if self._plan is None or not self._plan.matches(xyz, self.grid_size):
            self._plan = BinningPlan(xyz, self.grid_size)
        return self._plan

    def forward(self, xyz, scaling, rotation, timestamps, image_to_time=None, deform_scales: bool = True, first_frame_trainable: bool = False,
                image_plan=None):
        require_f32_cuda("xyz", xyz)
        if xyz.requires_grad:
            raise NotImplementedError("xyz.requires_grad: the 4-D stage keeps the positions fixed")
        names = LOCAL_NETS + (GLOBAL_NETS if self.use_global_trans else ())
        nets = {name: getattr(self, name).weights() for name in names}
        return deform_gaussians(xyz, scaling, rotation, timestamps, [list(g) for g in self.grids], nets, image_to_time=image_to_time,
                                use_global_trans=self.use_global_trans, deform_scales=deform_scales,
                                first_frame_trainable=first_frame_trainable, plan=self.plan_for(xyz), image_plan=image_plan)
