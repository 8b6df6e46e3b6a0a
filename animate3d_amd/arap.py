"""ARAP (as-rigid-as-possible) rigidity loss on the Gaussian trajectories and its exact k-NN graph, on the gfx950 kernels of csrc/arap.hip.

The reference adds ``lambda_arap * cal_arap_error(stack([_xyz] + means3D), ...)`` to the 4D-SDS loss (custom/threestudio-animate3d/
systems/animate3d.py:215-244, systems/util.py:38-215; every released config: ``lambda_arap: 12.``, ``arap_K: 3``, ``arap_radius: 0.01``,
``arap_sample_num: 512``).  It searches the K + 1 nearest neighbours of every Gaussian with ``pytorch3d.ops.knn_points`` on every step,
although ``_xyz`` is fixed in this stage, and then loops over the frames in Python.  Here the graph is searched once (``ArapGraph``) and
the loss of all frames is one call on the ``[B, N, 3]`` means of ``deform4d.deform_gaussians``.

Contract (fp32 at the interface; CPU tensors raise: there is no torch fallback)

``knn_graph(points [Nv, 3], K, radius=None, least_edge_num=3) -> (nn_idx [Nv, K] int32, nn_dist [Nv, K] fp32)``: for each point the K
nearest *other* points by ``dx*dx + dy*dy + dz*dz`` (fp32), ascending by (distance, index): exact, a point is never its own neighbour,
duplicated points are each other's neighbours at distance 0.  With ``radius``, columns ``>= least_edge_num`` whose distance is not below
``radius ** 2`` become index -1 and distance +inf (util.py:100-101).  1 <= K <= 16 (``NotImplementedError`` otherwise), Nv > K
(``ValueError``).

``arap_energy(source [Nv, 3], targets [F, Nv, 3], nn_idx [Nv, K], *, weight, sample_idx, sample_num, generator, return_rotations)``
is ``cal_arap_error(cat([source[None], targets]), ...)`` with ``estimate_rotation`` as written:

* edge ``e[v, k] = p[v] - p[nn_idx[v, k]]``, zero where ``nn_idx`` is -1; ``weight [Nv, K]`` defaults to 1 on edges, 0 elsewhere (what
  animate3d.py:241 uses: it passes none);
* ``sample_idx [S]`` (repeats allowed) defaults to every vertex if ``Nv <= sample_num`` and else to ``sample_num`` draws with replacement
  from ``generator`` on the device (the reference draws with ``np.random.choice`` on the host);
* per frame f and sample s: ``S = sum_k w_k src_k^T tgt_k``; ``R = W U^T`` of ``S = U Sigma W^T``, with the column of U of the smallest
  singular value flipped where ``det <= 0``; ``S`` is zeroed first, hence ``R = I``, when for some coordinate axis all K source and target
  edge components are equal as fp32 numbers (util.py:156-157; the first frame's means equal ``xyz`` exactly, so this is live);
  ``energy += sum_k w_k |tgt_k - R src_k|^2``;
* the loss is the plain sum over f, s, k, accumulated in a fixed order; returned as a 0-d fp32 tensor, with ``return_rotations`` also
  ``R [F, S, 3, 3]``.

Inside the kernels the edges, ``S``, the decomposition (a one-sided Jacobi SVD), ``R`` and the sums are fp64: there are only F x S problems,
and near-rigid motion makes ``tgt - R src`` a small difference of large terms.

Gradients: ``R`` is a constant (``torch.no_grad()`` in the reference).  ``d tgt_i += 2 w (tgt_e - R src_e)`` with the negative on the
neighbour; ``d src_i -= 2 w R^T (tgt_e - R src_e)`` with the negative on the neighbour, produced only when ``source.requires_grad``.  The
backward is in gather form over an inverse list built from ``sample_idx`` and ``nn_idx`` (stable sort, fixed shapes): no floating-point
atomics, two backward passes are bit-identical, the result does not depend on launch geometry, and rows no sample touches are exactly
zero.  ``targets`` may be a batch-strided view of the means (``means[:F]``, ``means[::2]``); each frame must be dense (``ValueError``
otherwise: nothing is copied silently).

Host synchronisation: nothing in ``arap_energy``'s forward or backward synchronises with the host.  There is no ``.item()``, no
``nonzero``, no data-dependent shape: out-of-range indices are handled in the kernels (such an edge is absent, such a sample contributes
nothing).  The step stays capturable.  (The drop-in ``cal_connectivity_from_points`` returns the reference's masked edge list, whose
length depends on the data: it synchronises, once per graph.)

The mesh branch (animate3d.py:222-234, ``connected_vertices_info_path``; ``configs/mesh_animation_frame_16.yaml``)

``MeshGraph`` holds a mesh's fixed, directed vertex adjacency in CSR form on the device (``row_start [Nv + 1]``, ``col [E]``, int32) and
``MeshGraph.sample(K)`` draws every step's ``nn_idx [Nv, K]`` from it in one launch of ``a3d_mesh_sample_neighbours``, where the
reference's ``sample_matrix_vectorized`` (util.py:320-344) makes a ``rand(Nv, Dmax)``, a masked add, a full sort along ``Dmax`` and an
advanced-index gather.  The sampling contract: for vertex v of degree d the row holds ``min(K, d)`` distinct positions of its adjacency
row, a uniformly random subset, in ascending row position, then -1; a row with ``d <= K`` holds all its neighbours, one with ``d = 0`` is
all -1.  The draw is a pure function of ``(seed, v)`` and the graph (selection sampling on Philox4x32-10; specified to the bit in
include/animate3d_hip.h), so it does not depend on the launch geometry and a host restatement is bit-exact.

Subset against tuple.  The reference's row is the first P columns of a random permutation of the d neighbours: a uniformly random
*ordered* P-tuple without repetition, followed by -1 where ``d < P`` (its -1 column index picks the padded last column; defined for
``P <= Dmax``).  Ours is the same tuple's *set*, listed in row order.  The set of a uniform ordered tuple is a uniform subset, and the
only consumer, ``cal_arap_error`` as ``training_step`` calls it (animate3d.py:241: no ``weight``), sums unit-weight terms over k, both in
the covariance ``S`` and in the energy: the column order changes nothing but the order of an fp64 summation.  Sampling is per vertex, not
per ``sample_idx`` entry: duplicated entries of ``sample_idx`` see the same row, as in the reference.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .f32_stage import TensorKeyed, gather_plan, launch, require_f32_cuda, require_index_cuda
from .hip_ops import _p

K_MAX = 16


def _check_k(K: int, Nv: int):
    if not 1 <= int(K) <= K_MAX:
        raise NotImplementedError(f"K = {K}: the k-NN kernel supports 1 <= K <= {K_MAX}")
    if Nv <= K:
        raise ValueError(f"Nv = {Nv} points cannot have K = {K} other neighbours each")


def knn_graph(points: torch.Tensor, K: int, radius: Optional[float] = None, least_edge_num: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact K nearest other points of each point: (nn_idx [Nv, K] int32, nn_dist [Nv, K] fp32 squared distances); see the module docstring."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected [Nv, 3], got {tuple(points.shape)}")
    Nv, K = points.shape[0], int(K)
    _check_k(K, Nv)
    require_f32_cuda("points", points)
    if least_edge_num < 0:
        raise ValueError("least_edge_num must not be negative")
    x = points.detach().contiguous()
    nn_idx = torch.empty(Nv, K, dtype=torch.int32, device=points.device)
    nn_dist = torch.empty(Nv, K, dtype=torch.float32, device=points.device)
    least, r2 = (K, float("inf")) if radius is None else (int(least_edge_num), float(radius) ** 2)
    launch("a3d_knn_f32", points.device, Nv, _p(x), K, least, r2, _p(nn_idx), _p(nn_dist))
    return nn_idx, nn_dist


class ArapGraph(TensorKeyed):
    """The k-NN graph of one ``xyz``: ``nn_idx`` / ``nn_dist`` of ``knn_graph``.  It is a ``f32_stage.TensorKeyed``, as ``deform4d.BinningPlan``
    is, with K, radius and ``least_edge_num`` in the key; an in-place change of ``xyz`` therefore invalidates it.  ``refresh(xyz)`` searches
    again only then, so the search runs once per stage, not once per step."""

    def __init__(self, xyz: torch.Tensor, K: int = 3, radius: Optional[float] = None, least_edge_num: int = 3, *, neighbours=None):
        self.K, self.radius, self.least_edge_num = int(K), None if radius is None else float(radius), int(least_edge_num)
        self.builds = 0
        self._bind(xyz, neighbours)

    def _bind(self, xyz, neighbours=None):
        if neighbours is None:
            neighbours = knn_graph(xyz, self.K, self.radius, self.least_edge_num)
        self.nn_idx, self.nn_dist = neighbours
        self.bind(xyz, self.K, self.radius, self.least_edge_num)
        self.builds += 1

    @classmethod
    def from_neighbours(cls, xyz: torch.Tensor, nn_idx: torch.Tensor, nn_dist: Optional[torch.Tensor] = None, radius: Optional[float] = None,
                        least_edge_num: int = 3) -> "ArapGraph":
        """A graph that was found elsewhere (a fixed dense ``nn_idx`` with -1 entries), under the same key.  A mesh's connectivity, whose
        neighbours are drawn again every step, is a ``MeshGraph``."""
        return cls(xyz, nn_idx.shape[1], radius, least_edge_num, neighbours=(nn_idx, nn_dist))

    def matches(self, xyz: torch.Tensor) -> bool:
        return super().matches(xyz, self.K, self.radius, self.least_edge_num)

    def refresh(self, xyz: torch.Tensor) -> "ArapGraph":
        if not self.matches(xyz):
            self._bind(xyz)
        return self


def _check_sample_k(K: int):
    if not 1 <= int(K) <= K_MAX:
        raise NotImplementedError(f"K = {K}: the sampling kernel supports 1 <= K <= {K_MAX}")


class MeshGraph:
    """A mesh's fixed, directed vertex adjacency in CSR form: ``row_start [Nv + 1]`` and ``col [E]`` int32 on one device; row v is
    ``col[row_start[v]:row_start[v + 1]]`` in the order it was given.  ``Nv``, ``max_degree`` and ``degrees [Nv]`` describe it.  The
    constructors run once per stage and may synchronise with the host; ``sample`` runs every step and does not.  See the module
    docstring for the sampling contract."""

    def __init__(self, row_start: torch.Tensor, col: torch.Tensor, max_degree: Optional[int] = None):
        if row_start.dim() != 1 or row_start.shape[0] < 2 or col.dim() != 1 or row_start.device != col.device:
            raise ValueError("expected row_start [Nv + 1] and col [E] on one device")
        self.row_start, self.col = row_start.to(torch.int32).contiguous(), col.to(torch.int32).contiguous()
        self.Nv = self.row_start.shape[0] - 1
        self.degrees = self.row_start[1:] - self.row_start[:-1]
        self.max_degree = int(self.degrees.max()) if max_degree is None else int(max_degree)

    @property
    def device(self) -> torch.device:
        return self.row_start.device

    @classmethod
    def _from_degrees(cls, degrees: torch.Tensor, col: torch.Tensor) -> "MeshGraph":
        Nv = degrees.shape[0]
        if Nv < 1:
            raise ValueError("a mesh graph needs at least one vertex")
        if col.numel() >= 2 ** 31:
            raise ValueError(f"{col.numel()} edges: the adjacency is indexed in 32 bits")
        if col.numel() and (int(col.min()) < 0 or int(col.max()) >= Nv):
            raise IndexError(f"neighbour indices must lie in [0, {Nv}), got [{int(col.min())}, {int(col.max())}]")
        row_start = torch.zeros(Nv + 1, dtype=torch.int64, device=degrees.device)
        row_start[1:] = torch.cumsum(degrees.long(), 0)
        return cls(row_start, col)

    @classmethod
    def from_connected_vertices(cls, info, device="cuda") -> "MeshGraph":
        """From the parsed JSON of ``connected_vertices_info_path``: ``{str(v): {str(u): anything, ...}, ...}`` with every vertex
        ``0 .. Nv - 1`` a key (``ValueError`` otherwise).  The neighbours of v are ``info[str(v)].keys()`` in dict order, as
        util.py:313-315 reads them; one outside ``[0, Nv)`` raises ``IndexError``."""
        Nv = len(info)
        rows = []
        for v in range(Nv):
            if str(v) not in info:
                raise ValueError(f"connected vertices: vertex {v} of {Nv} is not a key")
            rows.append([int(u) for u in info[str(v)].keys()])
        degrees = torch.tensor([len(r) for r in rows], dtype=torch.int64)
        col = torch.tensor([u for r in rows for u in r], dtype=torch.int64)
        return cls._from_degrees(degrees.to(device), col.to(device))

    @classmethod
    def from_padded(cls, nn_idx: torch.Tensor, mask: Optional[torch.Tensor] = None) -> "MeshGraph":
        """From a dense ``nn_idx [Nv, D]`` with -1 padding, the reference's in-memory form (``mask``: its ``max_idx``, by default
        ``nn_idx != -1``).  The -1 entries may sit anywhere in a row; the others keep their order.  Duplicates in a row are kept: they
        are drawn as the distinct positions they are, so a duplicated neighbour can appear twice in a sampled row, with twice the
        weight in the energy.  The caller owns them."""
        if nn_idx.dim() != 2 or nn_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"nn_idx: expected an int32 / int64 [Nv, D], got {nn_idx.dtype} {tuple(nn_idx.shape)}")
        mask = nn_idx != -1 if mask is None else mask.to(nn_idx.device).bool()
        if mask.shape != nn_idx.shape:
            raise ValueError(f"mask: expected {tuple(nn_idx.shape)}, got {tuple(mask.shape)}")
        return cls._from_degrees(mask.sum(1), nn_idx[mask].long())            # boolean indexing is row-major: each row keeps its order

    @classmethod
    def from_faces(cls, faces: torch.Tensor, Nv: int) -> "MeshGraph":
        """The undirected vertex adjacency of the triangles ``faces [F, 3]``: both directions of every edge, once each however many faces
        (or repeated faces) share it, every row ascending.  A degenerate face's repeated corner contributes no self-edge.  Torch ops on
        the device ``faces`` is on; an index outside ``[0, Nv)`` raises ``IndexError``."""
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"faces: expected an int32 / int64 [F, 3], got {faces.dtype} {tuple(faces.shape)}")
        Nv = int(Nv)
        f = faces.long()
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= Nv):
            raise IndexError(f"faces: vertex indices must lie in [0, {Nv}), got [{int(f.min())}, {int(f.max())}]")
        a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
        b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
        a, b = torch.cat([a, b]), torch.cat([b, a])
        keys = torch.unique((a * Nv + b)[a != b])                             # sorted: by vertex, then by neighbour
        src = torch.div(keys, Nv, rounding_mode="floor")
        return cls._from_degrees(torch.bincount(src, minlength=Nv), keys - src * Nv)

    def padded(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(nn_idx [Nv, max_degree] int64 with -1 padding, max_idx bool): what ``prepare_arap_from_mesh_vertices`` returns."""
        slot = torch.arange(self.max_degree, device=self.device)[None]
        max_idx = slot < self.degrees[:, None]
        nn_idx = torch.full((self.Nv, self.max_degree), -1, dtype=torch.int64, device=self.device)
        nn_idx[max_idx] = self.col.long()
        return nn_idx, max_idx

    def sample(self, K: int, *, generator: Optional[torch.Generator] = None, seed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step's neighbours: ``nn_idx [Nv, K]`` int32 under the module docstring's contract.  ``seed`` is a ``[1]`` int64 CUDA tensor,
        read on the device; by default ``torch.randint(0, 2**62, (1,), dtype=int64, generator=generator, device=dev)``: one draw from the
        generator, no ``.item()``.  One kernel launch, no host synchronisation, no ``Nv x max_degree`` temporary."""
        _check_sample_k(K)
        require_index_cuda("row_start", self.row_start)
        dev = self.device
        if seed is None:
            seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=generator, device=dev)
        elif not (isinstance(seed, torch.Tensor) and seed.is_cuda and seed.dtype == torch.int64 and tuple(seed.shape) == (1,)):
            raise ValueError("seed: a [1] int64 CUDA tensor (it is read on the device)")
        elif seed.device != dev:
            raise ValueError(f"seed is on {seed.device}, the graph on {dev}")
        nn_idx = torch.empty(self.Nv, int(K), dtype=torch.int32, device=dev)
        launch("a3d_mesh_sample_neighbours", dev, self.Nv, self.col.shape[0], _p(self.row_start), _p(self.col), int(K), _p(seed), _p(nn_idx))
        return nn_idx


def inverse_list(sample_idx: torch.Tensor, nn_idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The backward's gather plan: (order [S (K + 1)] int32, starts [Nv + 1] int32).  Pair ``s (K + 1) + c`` is sample s's own vertex
    (c = 0) or its neighbour c - 1; the pairs are stable-sorted by vertex, pairs without a vertex last; ``starts[v]`` is vertex v's first
    position.  Fixed shapes, no host synchronisation."""
    Nv = nn_idx.shape[0]
    v = sample_idx.long()
    ok = (v >= 0) & (v < Nv)
    nbr = nn_idx.long()[v.clamp(0, Nv - 1)]
    ids = torch.cat([v[:, None], nbr], dim=1)
    ids = torch.where(ok[:, None] & (ids >= 0) & (ids < Nv), ids, torch.full_like(ids, Nv)).reshape(-1)
    return gather_plan(ids, Nv)


class _ArapEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, source, targets, nn_idx, weight, sample_idx, want_rot):
        dev = source.device
        F, Nv, K, S = targets.shape[0], source.shape[0], nn_idx.shape[1], sample_idx.shape[0]
        src, tgt = source.detach(), targets.detach()
        rot = torch.empty(F, S, 9, dtype=torch.float64, device=dev)
        rot32 = torch.empty(F, S, 3, 3, dtype=torch.float32, device=dev) if want_rot else None
        energy = torch.empty(F * S, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        launch("a3d_arap_energy_f32", dev, F, Nv, K, S, _p(src), _p(tgt), tgt.stride(0), _p(nn_idx), _p(weight), _p(sample_idx), _p(rot),
               _p(rot32), _p(energy), _p(loss))
        ctx.save_for_backward(src, tgt, nn_idx, weight, sample_idx, rot)
        ctx.need_src = ctx.needs_input_grad[0]
        if want_rot:
            ctx.mark_non_differentiable(rot32)
            return loss, rot32
        return loss, None

    @staticmethod
    def backward(ctx, d_loss, _d_rot):
        src, tgt, nn_idx, weight, sample_idx, rot = ctx.saved_tensors
        dev = src.device
        F, Nv, K, S = tgt.shape[0], src.shape[0], nn_idx.shape[1], sample_idx.shape[0]
        g = None if d_loss is None else d_loss.detach().float().reshape(1).contiguous()
        order, starts = inverse_list(sample_idx, nn_idx)
        d_tgt = torch.empty(F, Nv, 3, dtype=torch.float32, device=dev)
        d_src = torch.empty(Nv, 3, dtype=torch.float32, device=dev) if ctx.need_src else None
        launch("a3d_arap_backward_f32", dev, F, Nv, K, S, _p(src), _p(tgt), tgt.stride(0), _p(nn_idx), _p(weight), _p(sample_idx), _p(rot),
               _p(order), _p(starts), _p(g), _p(d_tgt), _p(d_src))
        return d_src, d_tgt, None, None, None, None


def arap_energy(source: torch.Tensor, targets: torch.Tensor, nn_idx: torch.Tensor, *, weight: Optional[torch.Tensor] = None,
                sample_idx: Optional[torch.Tensor] = None, sample_num: int = 512, generator: Optional[torch.Generator] = None,
                return_rotations: bool = False):
    """The ARAP loss of ``targets [F, Nv, 3]`` against ``source [Nv, 3]`` over the graph ``nn_idx [Nv, K]`` (-1: no edge): a 0-d fp32 tensor,
    with ``return_rotations`` also ``R [F, S, 3, 3]``.  Semantics, gradients and guarantees: the module docstring.  Neither the forward nor
    the backward synchronises with the host."""
    require_f32_cuda("source", source)
    require_f32_cuda("targets", targets)
    require_index_cuda("nn_idx", nn_idx)
    Nv = source.shape[0]
    if source.dim() != 2 or source.shape[1] != 3 or targets.dim() != 3 or tuple(targets.shape[1:]) != (Nv, 3):
        raise ValueError(f"expected source [Nv, 3] and targets [F, Nv, 3], got {tuple(source.shape)} and {tuple(targets.shape)}")
    if nn_idx.dim() != 2 or nn_idx.shape[0] != Nv or nn_idx.shape[1] < 1:
        raise ValueError(f"nn_idx: expected [Nv, K], got {tuple(nn_idx.shape)}")
    F, K = targets.shape[0], nn_idx.shape[1]
    if F > 1 and (targets.stride(0) < 0 or 0 < targets.stride(0) < Nv * 3) or (F > 0 and Nv > 1 and tuple(targets.stride()[1:]) != (3, 1)):
        raise ValueError(f"targets: every frame must be dense ([Nv, 3] with strides (3, 1)) and the batch stride non-negative; got strides "
                         f"{tuple(targets.stride())}.  Call .contiguous() if a copy is what you want")
    if not source.is_contiguous():
        raise ValueError("source: expected a contiguous [Nv, 3] tensor")
    dev = source.device
    nn32 = nn_idx.detach().to(torch.int32).contiguous()
    if weight is not None:
        require_f32_cuda("weight", weight)
        if tuple(weight.shape) != (Nv, K):
            raise ValueError(f"weight: expected {(Nv, K)}, got {tuple(weight.shape)}")
        weight = weight.detach().contiguous()
    if sample_idx is None:
        if Nv <= sample_num:
            sample_idx = torch.arange(Nv, device=dev, dtype=torch.int32)
        else:
            sample_idx = torch.randint(Nv, (int(sample_num),), generator=generator, device=dev).to(torch.int32)
    else:
        if sample_idx.dim() != 1 or sample_idx.dtype not in (torch.int32, torch.int64) or not sample_idx.is_cuda:
            raise ValueError("sample_idx: a 1-D int32 / int64 CUDA tensor of vertex indices")
        sample_idx = sample_idx.detach().to(torch.int32).contiguous()
    S = sample_idx.shape[0]
    if F == 0 or S == 0:                                        # a sequence of the source alone: the reference's loop does not run
        loss = (source.sum() + targets.sum()) * 0.0
        return (loss, torch.empty(F, S, 3, 3, dtype=torch.float32, device=dev)) if return_rotations else loss
    loss, rot = _ArapEnergy.apply(source, targets, nn32, weight, sample_idx, bool(return_rotations))
    return (loss, rot) if return_rotations else loss


# ---- drop-ins with the reference's signatures (systems/util.py:58-117, 185-215)

def edges_to_dense(ii: torch.Tensor, jj: torch.Tensor, nn: torch.Tensor, Nv: int, K: int) -> torch.Tensor:
    """The reference's edge list (ii: vertex, jj: its neighbour, nn: the neighbour's column) as a dense ``nn_idx [Nv, K]`` int32, -1 where
    there is no edge.  No host synchronisation."""
    dense = torch.full((Nv, K), -1, dtype=torch.int32, device=jj.device)
    dense[ii.long(), nn.long()] = jj.to(torch.int32)
    return dense


def dense_to_edges(nn_idx: torch.Tensor):
    """``nn_idx [Nv, K]`` -> (ii, jj, nn) int64 with the -1 entries dropped, in row-major order (util.py:111-115).  The length depends on
    the data: this synchronises with the host."""
    Nv, K = nn_idx.shape
    dev = nn_idx.device
    ii = torch.arange(Nv, device=dev)[:, None].long().expand(Nv, K).reshape([-1])
    jj = nn_idx.long().reshape([-1])
    nn = torch.arange(K, device=dev)[None].long().expand(Nv, K).reshape([-1])
    mask = jj != -1
    return ii[mask], jj[mask], nn[mask]


def cal_connectivity_from_points(points=None, radius=0.1, K=10, trajectory=None, least_edge_num=3, node_radius=None, mode="nn", GraphK=4,
                                 adaptive_weighting=True):
    """Drop-in for util.py:58-117 with ``mode='nn'`` and ``trajectory=None``: ``points [T, Nv, 3]`` -> (ii, jj, nn, weight [Nv, K]).  The search
    is ``knn_graph`` on the first frame; the multi-frame radius test (util.py:80-84), the radius cut and ``weight`` are torch, exactly as
    written, quirks included: with ``adaptive_weighting`` a cut edge makes ``nn_dist.mean()`` infinite, so such a row's weights are NaN."""
    if trajectory is not None:
        raise NotImplementedError("trajectory=: only the graph of the points themselves is supported")
    if mode != "nn":
        raise NotImplementedError(f"mode={mode!r}: only 'nn' is supported")
    require_f32_cuda("points", points)
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError(f"points: expected [T, Nv, 3], got {tuple(points.shape)}")
    nn_idx, nn_dist = knn_graph(points[0], K)
    nn_idx = nn_idx.long()
    if points.shape[0] > 1:
        rest_knn_pts = points[1:][:, nn_idx]                                             # knn_gather: [T - 1, Nv, K, 3]
        rest_nn_dist = ((rest_knn_pts - points[0:1][:, :, None]) ** 2).sum(-1)
        nn_dist = torch.where((rest_nn_dist < radius ** 2).all(0), nn_dist, torch.ones_like(nn_dist) * torch.inf)
    nn_idx[:, least_edge_num:] = torch.where(nn_dist[:, least_edge_num:] < radius ** 2, nn_idx[:, least_edge_num:],
                                             - torch.ones_like(nn_idx[:, least_edge_num:]))
    nn_dist[:, least_edge_num:] = torch.where(nn_dist[:, least_edge_num:] < radius ** 2, nn_dist[:, least_edge_num:],
                                              torch.ones_like(nn_dist[:, least_edge_num:]) * torch.inf)
    if adaptive_weighting:
        weight = torch.exp(-nn_dist / nn_dist.mean())
    elif node_radius is None:
        weight = torch.exp(-nn_dist)
    else:
        nn_radius = node_radius[nn_idx]
        weight = torch.exp(-nn_dist / (2 * nn_radius ** 2))
    weight = weight / weight.sum(dim=-1, keepdim=True)
    ii, jj, nn = dense_to_edges(nn_idx)
    return ii, jj, nn, weight


def cal_arap_error(nodes_sequence, ii, jj, nn, K=10, weight=None, sample_num=512, *, sample_idx=None, generator=None,
                   return_rotations=False):
    """Drop-in for util.py:185-215: ``nodes_sequence [Nt, Nv, 3]``, frame 0 the source.  The keyword-only arguments are additions
    (the reference draws its sample on the host inside the function)."""
    require_f32_cuda("nodes_sequence", nodes_sequence)
    Nv = nodes_sequence.shape[1]
    nn_idx = edges_to_dense(ii, jj, nn, Nv, K)
    return arap_energy(nodes_sequence[0], nodes_sequence[1:], nn_idx, weight=weight, sample_idx=sample_idx, sample_num=sample_num,
                       generator=generator, return_rotations=return_rotations)


def prepare_arap_from_mesh_vertices(connected_vertices_info, device="cpu"):
    """Drop-in for util.py:300-318: (nn_idx [Nv, Dmax] int64 with -1 padding, max_idx bool), on the CPU as the reference returns them
    (``device`` is an addition).  ``training_step`` wants the ``MeshGraph`` itself: ``MeshGraph.from_connected_vertices(info)``."""
    return MeshGraph.from_connected_vertices(connected_vertices_info, device).padded()


def sample_matrix_vectorized(input_matrix, P, max_index, *, generator=None, seed=None):
    """Drop-in for util.py:320-344: ``input_matrix [N, Dmax]`` and its mask ``max_index`` -> int64 ``[N, P]`` under ``MeshGraph.sample``'s
    contract (a random subset in row order where the reference gives a random tuple; the module docstring says why that is
    equivalent).  The keyword-only arguments are additions.  This builds a ``MeshGraph.from_padded`` on every call, which synchronises
    with the host: a caller in a loop should hold the ``MeshGraph`` and call ``sample``."""
    require_index_cuda("input_matrix", input_matrix)
    return MeshGraph.from_padded(input_matrix, max_index).sample(P, generator=generator, seed=seed).long()
