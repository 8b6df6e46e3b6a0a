"""Mesh ingest: the 4-D stage's ``Gaussians`` and ``MeshGraph`` from a triangle mesh in one call, on the gfx950 kernels of
csrc/mesh_ingest.hip.

The reference starts its mesh-animation branch from two files that ``tools/mesh_animation/mesh2gaussian.py`` writes: a Gaussian PLY
(``geometry_convert_from``) and a JSON of every vertex's neighbours (``connected_vertices_info_path``).  The script needs pytorch3d,
which has no ROCm build, walks faces and vertices in Python with an ``.item()`` per edge, and ``Gaussian4DModel.load_ply`` and
``prepare_arap_from_mesh_vertices`` then parse its files again.  ``gaussians_from_mesh`` computes the same quantities from the adjacency
``MeshGraph.from_faces`` builds, in one launch, and hands over what ``stage4d.training_step`` takes.

Contract (fp32 at the interface; CPU tensors raise: there is no torch fallback)

``gaussians_from_mesh(verts [Nv, 3], faces [F, 3] int32 / int64, *, <one colour source>, rot_x_degree, rot_z_degree, scale_factor, shrink,
opacity) -> MeshGaussians(gaussians, graph, colors [Nv, 3], mean_edge [Nv, 3], edge_length [E])``

* ``graph`` is ``MeshGraph.from_faces(faces, Nv)``.  Its rows equal the reference's ``connected_vertices`` as sets; the reference keeps
  insertion order and ours ascends.  The step's sampler draws subsets of a row, so the order decides only which subset a seed yields.
* ``edge_length[e] = |x_v - x_col[e]|`` for e in v's row: the value the JSON stores (mesh2gaussian.py:77).
* ``mean_edge[v]``: the mean over v's row of ``|x_u - x_v|`` per axis (:36-63), summed in row order.
* ``colors[v]``: the mean over the face corners at v of the corner's colour (:15-33), summed in ascending corner order; the corner list
  is ``f32_stage.gather_plan(faces.reshape(-1), Nv)``.  The colour source is exactly one of ``vertex_colors [Nv, 3]`` (passed through
  unchanged), ``corner_colors [F, 3, 3]`` and ``texture [Ht, Wt, 3]`` with ``uvs [Nt, 2]`` and ``faces_uvs [F, 3]``; anything else
  raises ``ValueError``.  Textured corners are sampled in the kernel, bilinearly, under the convention pytorch3d documents for
  ``TexturesUV.faces_verts_textures_packed``: v axis flipped, ``align_corners=True``, border padding, i.e.
  ``F.grid_sample(flip(texture, rows), uv * 2 - 1, mode="bilinear", padding_mode="border", align_corners=True)``.  pytorch3d has
  no ROCm build and its source is not part of the reference: the convention is pinned to that torch call, not to pytorch3d itself.
* The Gaussians are ``convert_point_cloud_to_gaussian`` (:114-139) followed by ``load_ply``'s transform (gaussian_4d.py:177-260) with
  ``R = Rz Rx``: ``xyz = scale_factor (R x)``; ``scaling = log(mean_edge / shrink * scale_factor)``; ``rotation``: the unit quaternion
  (w, x, y, z) of R with ``w >= 0``, computed on the host in float64 and broadcast; ``opacity [Nv, 1]`` is ``opacity`` itself, already
  activated; ``shs [Nv, 1, 3] = (colors - 0.5) / C0``, ``sh_degree = 0``.  An axis on which all of a vertex's neighbours coincide with it
  has a zero mean edge and hence a ``-inf`` log-scale, as in the reference (``np.log(0)``): it is kept, the caller owns such a mesh.
* A vertex that is in no face raises ``ValueError`` naming how many there are: the reference's JSON would have no key for it, and the
  stage would index wrongly.  This check, the index-range checks and ``MeshGraph``'s constructor synchronise with the host; the call
  runs once per asset.

``to_mesh_frame`` is the inverse transform ``export_animated_mesh.py:97-99`` applies to ``stage4d.vertex_trajectory``'s rows;
``read_gaussian_ply`` is ``load_ply`` plus ``get_opacity`` / ``get_features`` for any 3DGS PLY (parsed with numpy, transformed on the
device, ``plyfile`` not needed); ``write_gaussian_ply`` and ``write_connected_vertices`` write the two files of ``mesh2gaussian.py`` for
the reference's own loaders; ``load_obj`` reads a Wavefront OBJ into the arguments of ``gaussians_from_mesh``."""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from .arap import MeshGraph
from .f32_stage import gather_plan, launch, require_f32_cuda, require_index_cuda, require_shape
from .hip_ops import _p
from .stage4d import Gaussians

C0 = 0.28209479177387814


class MeshGaussians(NamedTuple):
    gaussians: Gaussians
    graph: MeshGraph
    colors: torch.Tensor
    mean_edge: torch.Tensor
    edge_length: torch.Tensor


class ObjMesh(NamedTuple):
    """``load_obj``'s result: ``gaussians_from_mesh(m.verts, m.faces, **m.colors)``."""
    verts: torch.Tensor
    faces: torch.Tensor
    colors: Dict[str, torch.Tensor]


def frame_rotation(rot_x_degree: float = 0.0, rot_z_degree: float = 0.0) -> np.ndarray:
    """``R = Rz Rx`` in float64, as gaussian_4d.py:181-196 builds it."""
    tx, tz = np.deg2rad(float(rot_x_degree)), np.deg2rad(float(rot_z_degree))
    rx = np.array([[1, 0, 0], [0, np.cos(tx), -np.sin(tx)], [0, np.sin(tx), np.cos(tx)]], dtype=np.float64)
    rz = np.array([[np.cos(tz), -np.sin(tz), 0], [np.sin(tz), np.cos(tz), 0], [0, 0, 1]], dtype=np.float64)
    return rz @ rx


def quaternion_of(R: np.ndarray) -> np.ndarray:
    """The unit quaternion (w, x, y, z) of a rotation matrix with ``w >= 0``, in float64 (the largest component is found first)."""
    m = np.asarray(R, dtype=np.float64)
    t = np.array([m[0, 0] + m[1, 1] + m[2, 2], m[0, 0] - m[1, 1] - m[2, 2], m[1, 1] - m[0, 0] - m[2, 2], m[2, 2] - m[0, 0] - m[1, 1]])
    i = int(np.argmax(t))
    s = 2.0 * np.sqrt(1.0 + t[i])
    if i == 0:
        q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    elif i == 1:
        q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
    elif i == 2:
        q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
    else:
        q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
    q = np.array(q, dtype=np.float64)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _host_doubles(values):
    flat = np.asarray(values, dtype=np.float64).reshape(-1)
    return (ctypes.c_double * flat.size)(*flat.tolist())


def _positive(name: str, value) -> float:
    value = float(value)
    if not (value > 0.0 and np.isfinite(value)):
        raise ValueError(f"{name} = {value}: expected a positive finite number")
    return value


def _same_device(dev, **tensors):
    for name, t in tensors.items():
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, verts on {dev}")


def gaussians_from_mesh(verts: torch.Tensor, faces: torch.Tensor, *, vertex_colors: Optional[torch.Tensor] = None,
                        corner_colors: Optional[torch.Tensor] = None, texture: Optional[torch.Tensor] = None,
                        uvs: Optional[torch.Tensor] = None, faces_uvs: Optional[torch.Tensor] = None, rot_x_degree: float = 0.0,
                        rot_z_degree: float = 0.0, scale_factor: float = 1.0, shrink: float = 1.1,
                        opacity: float = 1 - 1e-5) -> MeshGaussians:
    """A triangle mesh -> the stage's ``Gaussians`` (one per vertex) and ``MeshGraph``; see the module docstring."""
    require_shape("verts", verts, ("Nv", 3), non_empty=True)
    require_shape("faces", faces, ("F", 3), non_empty=True)
    Nv, F = verts.shape[0], faces.shape[0]
    textured = [t is not None for t in (texture, uvs, faces_uvs)]
    sources = (vertex_colors is not None) + (corner_colors is not None) + any(textured)
    if sources != 1:
        raise ValueError(f"{sources} colour sources: give exactly one of vertex_colors, corner_colors and (texture, uvs, faces_uvs)")
    if any(textured) and not all(textured):
        raise ValueError("a textured mesh needs texture, uvs and faces_uvs together")
    require_shape("vertex_colors", vertex_colors, (Nv, 3), optional=True)
    require_shape("corner_colors", corner_colors, (F, 3, 3), optional=True)
    require_shape("texture", texture, ("Ht", "Wt", 3), non_empty=True, optional=True)
    require_shape("uvs", uvs, ("Nt", 2), non_empty=True, optional=True)
    require_shape("faces_uvs", faces_uvs, (F, 3), optional=True)
    scale_factor, shrink, opacity = _positive("scale_factor", scale_factor), _positive("shrink", shrink), float(opacity)
    if not 0.0 < opacity <= 1.0:
        raise ValueError(f"opacity = {opacity}: an activated opacity lies in (0, 1]")
    if Nv >= 2 ** 31 // 3 or F >= 2 ** 31 // 9:
        raise ValueError(f"{Nv} vertices, {F} faces: the mesh is indexed in 32 bits")
    if faces_uvs is not None and faces_uvs.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces_uvs: expected an int32 / int64 tensor, got {faces_uvs.dtype}")
    graph = MeshGraph.from_faces(faces, Nv)                         # checks the dtype and the range of faces
    if faces_uvs is not None:
        lo, hi = torch.stack([faces_uvs.min(), faces_uvs.max()]).tolist()
        if lo < 0 or hi >= uvs.shape[0]:
            raise IndexError(f"faces_uvs: uv indices must lie in [0, {uvs.shape[0]}), got [{lo}, {hi}]")
    unreferenced = int((torch.bincount(faces.reshape(-1).long(), minlength=Nv) == 0).sum())
    if unreferenced:
        raise ValueError(f"{unreferenced} of {Nv} vertices are in no face: they would have no neighbours, no colour and no row in the "
                         "connectivity; remove them from the mesh first")
    dev = verts.device
    require_f32_cuda("verts", verts)
    require_index_cuda("faces", faces)
    given = {k: t for k, t in dict(vertex_colors=vertex_colors, corner_colors=corner_colors, texture=texture, uvs=uvs).items() if t is not None}
    for name, t in given.items():
        require_f32_cuda(name, t)
    if faces_uvs is not None:
        require_index_cuda("faces_uvs", faces_uvs)
        given["faces_uvs"] = faces_uvs
    _same_device(dev, faces=faces, **given)

    x = verts.detach().contiguous()
    E = graph.col.shape[0]
    flat = {k: t.detach().contiguous() for k, t in given.items()}
    order = starts = corner_uv = None
    if vertex_colors is None:
        order, starts = gather_plan(faces.reshape(-1), Nv)
    if faces_uvs is not None:
        corner_uv = faces_uvs.reshape(-1).to(torch.int32).contiguous()
    Ht, Wt = (texture.shape[0], texture.shape[1]) if texture is not None else (0, 0)
    R = frame_rotation(rot_x_degree, rot_z_degree)
    out = {k: torch.empty(Nv, 3, dtype=torch.float32, device=dev) for k in ("xyz", "scaling", "shs", "colors", "mean_edge")}
    edge_length = torch.empty(E, dtype=torch.float32, device=dev)
    launch("a3d_mesh_vertex_gaussians_f32", dev, Nv, E, 3 * F, _p(x), _p(graph.row_start), _p(graph.col), _p(order), _p(starts),
           _p(flat.get("vertex_colors")), _p(flat.get("corner_colors")), _p(flat.get("texture")), Ht, Wt, _p(flat.get("uvs")),
           0 if uvs is None else uvs.shape[0], _p(corner_uv), _host_doubles(R), scale_factor, shrink, _p(out["xyz"]), _p(out["scaling"]),
           _p(out["shs"]), _p(out["colors"]), _p(out["mean_edge"]), _p(edge_length))
    rotation = torch.tensor(quaternion_of(R), dtype=torch.float32).to(dev).expand(Nv, 4).contiguous()
    gaussians = Gaussians(xyz=out["xyz"], scaling=out["scaling"], rotation=rotation,
                          opacity=torch.full((Nv, 1), opacity, dtype=torch.float32, device=dev), shs=out["shs"].reshape(Nv, 1, 3), sh_degree=0)
    return MeshGaussians(gaussians, graph, out["colors"], out["mean_edge"], edge_length)


def to_mesh_frame(trajectory: torch.Tensor, *, rot_x_degree: float = 0.0, rot_z_degree: float = 0.0, scale_factor: float = 1.0) -> torch.Tensor:
    """``(trajectory / scale_factor) R`` for ``trajectory [T, N, 3]``: the stage's positions back in the mesh's own frame, the inverse
    export_animated_mesh.py:97-99 applies to every ``mesh_trajectory/{i}.npy`` (``R^T p`` per point).  Plain torch: one matmul."""
    require_shape("trajectory", trajectory, ("T", "N", 3))
    scale_factor = _positive("scale_factor", scale_factor)
    R = torch.tensor(frame_rotation(rot_x_degree, rot_z_degree), dtype=trajectory.dtype, device=trajectory.device)
    return (trajectory / scale_factor) @ R


# ---- files: 3DGS PLY, the connectivity JSON, Wavefront OBJ

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def parse_ply_vertices(path) -> Dict[str, np.ndarray]:
    """{property name: [N] array} of a PLY's ``vertex`` element, which must come first (binary little-endian or ascii, scalar properties)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.find(b"\n", end) + 1
    fmt, n, props, elements = None, None, [], 0
    for line in data[:end].decode("ascii").splitlines():
        tok = line.split()
        if not tok or tok[0] in ("ply", "comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements += 1
            if elements == 1:
                if tok[1] != "vertex":
                    raise ValueError(f"{path}: the first element is {tok[1]!r}, expected 'vertex'")
                n = int(tok[2])
        elif tok[0] == "property" and elements == 1:
            if tok[1] == "list" or tok[1] not in _PLY_TYPES:
                raise ValueError(f"{path}: vertex property {' '.join(tok[1:])!r} is not a scalar of a known type")
            props.append((tok[2], _PLY_TYPES[tok[1]]))
    if n is None or not props:
        raise ValueError(f"{path}: no vertex element")
    if fmt == "binary_little_endian":
        dtype = np.dtype([(name, "<" + t) for name, t in props])
        if len(data) - body < n * dtype.itemsize:
            raise ValueError(f"{path}: {n} vertices of {dtype.itemsize} bytes do not fit in the file")
        rec = np.frombuffer(data, dtype=dtype, count=n, offset=body)
        return {name: np.ascontiguousarray(rec[name]) for name, _ in props}
    if fmt == "ascii":
        table = np.array(data[body:].split()[:n * len(props)], dtype=np.float64)
        if table.size != n * len(props):
            raise ValueError(f"{path}: {n} vertices of {len(props)} values do not fit in the file")
        table = table.reshape(n, len(props))
        return {name: table[:, i].astype(t) for i, (name, t) in enumerate(props)}
    raise NotImplementedError(f"{path}: PLY format {fmt!r} (binary_little_endian and ascii are read)")


def _numbered(fields: Dict[str, np.ndarray], prefix: str):
    names = sorted((k for k in fields if k.startswith(prefix)), key=lambda k: int(k.split("_")[-1]))
    return np.stack([fields[k].astype(np.float32) for k in names], 1) if names else np.zeros((len(next(iter(fields.values()))), 0), np.float32)


def parse_gaussian_ply(path) -> Dict[str, np.ndarray]:
    """The fields ``load_ply`` reads, as float32 arrays in the file's own frame: ``xyz [N, 3]``, ``f_dc [N, 3]``, ``f_rest [N, R]`` (in
    ``f_rest_i`` order), ``opacity [N, 1]`` (the logit), ``scale [N, 3]`` (log), ``rot [N, 4]`` (w first)."""
    fields = parse_ply_vertices(path)
    missing = [k for k in ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity") if k not in fields]
    if missing:
        raise ValueError(f"{path}: no vertex property {missing}: not a 3DGS PLY")
    out = {"xyz": np.stack([fields[k].astype(np.float32) for k in "xyz"], 1), "f_dc": _numbered(fields, "f_dc_"),
           "f_rest": _numbered(fields, "f_rest_"), "opacity": fields["opacity"].astype(np.float32)[:, None],
           "scale": _numbered(fields, "scale_"), "rot": _numbered(fields, "rot_")}
    if out["scale"].shape[1] != 3 or out["rot"].shape[1] != 4:
        raise ValueError(f"{path}: expected scale_0..2 and rot_0..3, got {out['scale'].shape[1]} and {out['rot'].shape[1]} properties")
    return out


def read_gaussian_ply(path, *, rot_x_degree: float = 0.0, rot_z_degree: float = 0.0, scale_factor: float = 1.0, max_sh_degree: int = 0,
                      device="cuda") -> Gaussians:
    """``Gaussian4DModel.load_ply`` (gaussian_4d.py:177-306) followed by ``get_opacity`` / ``get_features``: the stage's ``Gaussians`` from a
    3DGS PLY.  ``xyz = scale_factor (R x)``, ``scaling = scale + log(scale_factor)``, ``rotation = q_R (x) rot / |rot|`` (the reference goes
    through matrices and scipy, whose quaternion sign is not canonical: equal as rotations), on the device in one launch of
    a3d_gaussians_rigid_f32; ``opacity = sigmoid(opacity)``; ``shs [N, (max_sh_degree + 1)^2, 3]`` from ``f_dc`` and, for
    ``max_sh_degree > 0``, the ``3 (max_sh_degree + 1)^2 - 3`` ``f_rest`` properties (``ValueError`` for another number)."""
    scale_factor, M = _positive("scale_factor", scale_factor), (int(max_sh_degree) + 1) ** 2
    if not 0 <= int(max_sh_degree) <= 3:
        raise ValueError(f"max_sh_degree = {max_sh_degree}: expected 0 .. 3")
    rec = parse_gaussian_ply(path)
    N = rec["xyz"].shape[0]
    if N < 1:
        raise ValueError(f"{path}: no Gaussians")
    if M > 1 and rec["f_rest"].shape[1] != 3 * M - 3:
        raise ValueError(f"{path}: {rec['f_rest'].shape[1]} f_rest properties, max_sh_degree = {max_sh_degree} needs {3 * M - 3}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device {dev}: the transform runs on the GPU (no CPU fallback)")
    xyz_in, scale_in, rot_in = (torch.from_numpy(rec[k]).to(dev).contiguous() for k in ("xyz", "scale", "rot"))
    xyz, scaling, rotation = torch.empty_like(xyz_in), torch.empty_like(scale_in), torch.empty_like(rot_in)
    R = frame_rotation(rot_x_degree, rot_z_degree)
    launch("a3d_gaussians_rigid_f32", dev, N, _p(xyz_in), _p(scale_in), _p(rot_in), _host_doubles(R), _host_doubles(quaternion_of(R)),
           scale_factor, _p(xyz), _p(scaling), _p(rotation))
    shs = torch.from_numpy(rec["f_dc"])[:, None, :]
    if M > 1:                                                       # (N, 3 * (M - 1)) -> (N, 3, M - 1) -> (N, M - 1, 3), gaussian_4d.py:232-283
        shs = torch.cat([shs, torch.from_numpy(rec["f_rest"]).reshape(N, 3, M - 1).transpose(1, 2)], dim=1)
    return Gaussians(xyz=xyz, scaling=scaling, rotation=rotation, opacity=torch.sigmoid(torch.from_numpy(rec["opacity"]).to(dev)),
                     shs=shs.contiguous().to(dev), sh_degree=int(max_sh_degree))


def write_gaussian_ply(path, verts, colors, mean_edge, *, shrink: float = 1.1, opacity: float = 1 - 1e-5):
    """The PLY ``mesh2gaussian.py`` writes (:93-139), binary little-endian float32, in the mesh's own frame: ``x y z``, zero normals,
    ``f_dc = (colors - 0.5) / C0``, ``opacity`` as its logit, ``scale = log(mean_edge / shrink)``, ``rot = (1, 0, 0, 0)``.  ``verts``,
    ``colors`` and ``mean_edge`` are ``[Nv, 3]`` tensors or arrays (``MeshGaussians.colors`` / ``.mean_edge`` with the mesh's vertices);
    ``Gaussian4DModel.load_ply`` and ``read_gaussian_ply`` apply the frame transform when they read it."""
    shrink = _positive("shrink", shrink)
    arrays = [np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (verts, colors, mean_edge)]
    xyz, rgb, mean = arrays
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape or mean.shape != xyz.shape:
        raise ValueError(f"expected verts, colors and mean_edge [Nv, 3], got {[a.shape for a in arrays]}")
    N = xyz.shape[0]
    with np.errstate(divide="ignore"):
        scale = np.log(mean / shrink)
    rot = np.zeros((N, 4))
    rot[:, 0] = 1.0
    logit = np.full((N, 1), np.log(opacity / (1 - opacity)))
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1",
             "rot_2", "rot_3"]
    table = np.concatenate([xyz, np.zeros_like(xyz), (rgb - 0.5) / C0, logit, scale, rot], axis=1).astype("<f4")
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % N + "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())


def write_connected_vertices(path, graph: MeshGraph, edge_length: torch.Tensor):
    """The JSON of ``find_and_save_connected_vertices`` (:66-88): ``{"v": {"u": |x_v - x_u|, ...}, ...}`` with every vertex a key, rows in
    the graph's order; what ``prepare_arap_from_mesh_vertices`` and ``MeshGraph.from_connected_vertices`` read."""
    if edge_length.dim() != 1 or edge_length.shape[0] != graph.col.shape[0]:
        raise ValueError(f"edge_length: expected [{graph.col.shape[0]}] (one per entry of graph.col), got {tuple(edge_length.shape)}")
    start, col, dist = graph.row_start.cpu().tolist(), graph.col.cpu().tolist(), edge_length.detach().double().cpu().tolist()
    info = {str(v): {str(col[e]): dist[e] for e in range(start[v], start[v + 1])} for v in range(graph.Nv)}
    with open(path, "w") as f:
        json.dump(info, f, indent=2)


def _obj_index(token: str, n: int, what: str, line_no: int) -> int:
    i = int(token)
    i = i - 1 if i > 0 else n + i                                 # 1-based; negative: relative to the elements read so far
    if i < 0 or i >= n or int(token) == 0:
        raise ValueError(f"line {line_no}: {what} index {token} with {n} read so far")
    return i


def _map_kd(mtl_path: str) -> Optional[str]:
    materials, maps = 0, []
    with open(mtl_path) as f:
        for line in f:
            tok = line.split()
            if tok and tok[0] == "newmtl":
                materials += 1
            elif tok and tok[0] == "map_Kd":
                maps.append(tok[-1])
    if materials > 1 or len(maps) > 1:
        raise NotImplementedError(f"{mtl_path}: {materials} materials and {len(maps)} texture maps; one material with one map_Kd is read")
    return os.path.join(os.path.dirname(mtl_path), maps[0]) if maps else None


def load_obj(path, device=None) -> ObjMesh:
    """A Wavefront OBJ -> ``ObjMesh(verts [Nv, 3] f32, faces [F, 3] int64, colors)`` where ``colors`` holds one colour source of
    ``gaussians_from_mesh``: ``texture`` / ``uvs`` / ``faces_uvs`` when the file's material library names a ``map_Kd`` (read through
    PIL, ``/ 255``) and every face corner has a ``vt``, else ``vertex_colors`` from ``v x y z r g b`` lines (``ValueError`` when there
    is neither).  Read: ``v``, ``vt``, ``f`` with corners ``a``, ``a/b``, ``a/b/c`` and ``a//c``, negative (relative) indices, polygons
    as fans around their first corner, one ``mtllib`` with one material and one ``map_Kd`` (more: ``NotImplementedError``).  Normals,
    groups and smoothing are ignored.  The tensors are on ``device`` (default: the CPU)."""
    verts, rgb, vts, faces, faces_uv, mtllibs, used = [], [], [], [], [], [], set()
    with open(path) as f:
        for line_no, line in enumerate(f, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) not in (4, 5, 7):
                    raise ValueError(f"line {line_no}: a vertex has 3 coordinates (an optional w) or 3 coordinates and r g b")
                verts.append([float(t) for t in tok[1:4]])
                rgb.append([float(t) for t in tok[4:7]] if len(tok) == 7 else None)
            elif tok[0] == "vt":
                if len(tok) < 3:
                    raise ValueError(f"line {line_no}: a texture coordinate has u and v")
                vts.append([float(tok[1]), float(tok[2])])
            elif tok[0] == "f":
                if len(tok) < 4:
                    raise ValueError(f"line {line_no}: a face has at least 3 corners")
                corners = [t.split("/") for t in tok[1:]]
                vi = [_obj_index(c[0], len(verts), "vertex", line_no) for c in corners]
                has_uv = [len(c) > 1 and c[1] != "" for c in corners]
                ti = [_obj_index(c[1], len(vts), "texture", line_no) for c in corners] if all(has_uv) else None
                for k in range(1, len(vi) - 1):
                    faces.append([vi[0], vi[k], vi[k + 1]])
                    faces_uv.append(None if ti is None else [ti[0], ti[k], ti[k + 1]])
            elif tok[0] == "mtllib":
                mtllibs.extend(tok[1:])
            elif tok[0] == "usemtl":
                used.add(tok[1])
    if not verts or not faces:
        raise ValueError(f"{path}: {len(verts)} vertices and {len(faces)} faces")
    if len(set(mtllibs)) > 1 or len(used) > 1:
        raise NotImplementedError(f"{path}: {len(set(mtllibs))} material libraries, {len(used)} materials in use; one of each is read")
    out = dict(verts=torch.tensor(verts, dtype=torch.float32), faces=torch.tensor(faces, dtype=torch.int64))
    image = _map_kd(os.path.join(os.path.dirname(os.path.abspath(path)), mtllibs[0])) if mtllibs else None
    if image is not None and all(t is not None for t in faces_uv):
        from PIL import Image
        with Image.open(image) as im:
            texture = torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0)
        colors = dict(texture=texture, uvs=torch.tensor(vts, dtype=torch.float32), faces_uvs=torch.tensor(faces_uv, dtype=torch.int64))
    elif all(c is not None for c in rgb):
        colors = dict(vertex_colors=torch.tensor(rgb, dtype=torch.float32))
    else:
        raise ValueError(f"{path}: no colour source: neither a map_Kd with a vt at every face corner nor r g b on every vertex")
    if device is not None:
        out = {k: t.to(device) for k, t in out.items()}
        colors = {k: t.to(device) for k, t in colors.items()}
    return ObjMesh(out["verts"], out["faces"], colors)
