"""Mesh export: one animated, self-contained ``.glb`` (glTF 2.0) from ``stage4d.vertex_trajectory`` and the mesh it came from, with the
per-frame vertex normals computed on gfx950 by csrc/mesh_export.hip.

The reference ends its mesh-animation branch with ``tools/mesh_animation/export_animated_mesh.py``: inside Blender (``bpy``) it loads the
OBJ, undoes ``load_ply``'s transform on every ``mesh_trajectory/{i}.npy`` (:97-99), loops over every vertex of every frame in Python
(:103-104) to write one shape key per frame with linear keyframes, leaves the normals of the deformed surface to Blender and exports an
FBX.  Neither ``bpy`` nor an FBX writer exists on a ROCm machine.  ``export_animated_glb`` builds the same construction, one morph target
per frame with linear keys, in a format that is JSON plus raw arrays, and ships the normals in the file.

Timeline.  The reference's timeline also holds a "Basis" key, the OBJ's own vertices, shown at time 0, with frame k at time k + 1.  Here
frame 0 of the trajectory is the base mesh and frame k sits at ``k / fps``: frame 0 of the stage is the undeformed mesh (timestamp -1
bypasses the field), so the extra key would repeat it.

Contract

``NormalPlan(faces [F, 3] int32 / int64, Nv)``: built once per mesh.  ``ValueError`` for another dtype or shape, ``IndexError`` for an
index outside ``[0, Nv)``, ``ValueError`` for a vertex that is in no face (as ``gaussians_from_mesh``).  Keeps int32 ``faces [3 F]``
flat, and ``order [3 F]`` / ``starts [Nv + 1]`` = ``f32_stage.gather_plan(faces.reshape(-1), Nv)``: vertex v's corners, ascending.  The
checks synchronise with the host.

``vertex_normals(positions [T, Nv, 3] or [Nv, 3], plan_or_faces) -> the same shape``: fp32 CUDA only, CPU tensors raise (no torch
fallback).  ``n[t, v] = normalize(sum over v's corners c of (P_t[b] - P_t[a]) x (P_t[d] - P_t[a]))`` with a, b, d the corners of c's face
in cyclic order from c: area-weighted, summed in ascending corner order in fp64 and rounded to fp32 once, hence bitwise reproducible and
independent of the launch geometry; ``(0, 0, 1)`` where the sum has no length or is not finite (glTF requires unit normals).  One launch
of a3d_mesh_vertex_normals_f32; with a prebuilt ``NormalPlan`` no host synchronisation.

``split_vertices(faces [F, 3], faces_uvs [F, 3] or None) -> (split_vertex [Ng], split_uv [Ng] or None, indices [F, 3])``: glTF has one
index per corner where an OBJ has two, so the glTF vertices are the distinct ``(v, vt)`` pairs, sorted by ``(v, vt)``:
``split_vertex[indices] == faces`` and ``split_uv[indices] == faces_uvs``.  Without UVs it is the identity on ``Nv`` vertices (default:
``faces.max() + 1``).  Plain torch, on the device of ``faces``, CPU included.

``write_animated_glb(path, positions [T, Ng, 3], normals [T, Ng, 3], indices [F, 3], *, uvs [Ng, 2], texture [Ht, Wt, 3], colors [Ng, 3],
fps)``: host-side (numpy arrays or CPU tensors), the only place that knows the file format.  One mesh with one primitive: ``POSITION`` /
``NORMAL`` hold frame 0, ``TEXCOORD_0 = (u, 1 - v)`` with ``uvs``, else ``COLOR_0`` (float VEC3) with ``colors``, UNSIGNED_INT indices;
``targets[k - 1] = {POSITION: fl32(p_k - p_0), NORMAL: fl32(n_k - n_0)}`` for k = 1 .. T - 1 and zero ``mesh.weights``; one animation on
the node's ``weights`` with input times ``k / fps``, the ``[T, T - 1]`` output whose row 0 is zero and whose row k is one-hot at k - 1,
``LINEAR``.  ``T == 1`` has no ``targets``, ``weights`` or ``animations`` key.  ``texture`` in [0, 1] is embedded as a PNG of
``round(texture * 255)`` (through PIL) behind one material (``baseColorTexture``, ``metallicFactor`` 0, ``roughnessFactor`` 1); its sampler
clamps to the edge and filters linearly, the convention ``gaussians_from_mesh`` samples the texture under.  ``ValueError`` before the
file is opened for: non-finite positions, normals, uvs or colours, ``fps <= 0``, a shape mismatch, an index outside ``[0, Ng)``, ``uvs``
together with ``colors``, ``texture`` without ``uvs``.

``export_animated_glb(path, trajectory [T, Nv, 3], faces, *, uvs, faces_uvs, texture, vertex_colors, rot_x_degree, rot_z_degree,
scale_factor, fps)``: ``mesh.to_mesh_frame``, ``vertex_normals``, ``split_vertices``, the gather through the split, ``write_animated_glb``.
The colour arguments are ``ObjMesh.colors``: ``export_animated_glb(path, traj, m.faces, **m.colors, ...)`` for both kinds of ``load_obj``
result.  Returns the arrays it wrote."""
from __future__ import annotations

import io
import json
import struct
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from .f32_stage import gather_plan, launch, require_f32_cuda, require_index_cuda, require_shape
from .hip_ops import _p
from .mesh import to_mesh_frame

FLOAT, UNSIGNED_INT, ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 5126, 5125, 34962, 34963
LINEAR_FILTER, CLAMP_TO_EDGE = 9729, 33071
GLB_MAGIC, CHUNK_JSON, CHUNK_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942


class NormalPlan:
    """The corner list of one mesh for ``vertex_normals``; see the module docstring."""

    def __init__(self, faces: torch.Tensor, Nv: int):
        require_shape("faces", faces, ("F", 3), non_empty=True)
        if faces.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"faces: expected an int32 / int64 tensor, got {faces.dtype}")
        Nv, F = int(Nv), faces.shape[0]
        if Nv < 1 or Nv >= 2 ** 31 // 3 or F >= 2 ** 31 // 3:
            raise ValueError(f"{Nv} vertices, {F} faces: the mesh is indexed in 32 bits")
        flat = faces.detach().reshape(-1)
        lo, hi = torch.stack([flat.min(), flat.max()]).tolist()
        if lo < 0 or hi >= Nv:
            raise IndexError(f"faces: vertex indices must lie in [0, {Nv}), got [{lo}, {hi}]")
        unreferenced = int((torch.bincount(flat.long(), minlength=Nv) == 0).sum())
        if unreferenced:
            raise ValueError(f"{unreferenced} of {Nv} vertices are in no face: they would have no normal; remove them from the mesh first")
        self.Nv, self.F = Nv, F
        self.faces = flat.to(torch.int32).contiguous()
        self.order, self.starts = gather_plan(flat, Nv)

    @property
    def device(self) -> torch.device:
        return self.faces.device


def vertex_normals(positions: torch.Tensor, plan_or_faces: Union[NormalPlan, torch.Tensor]) -> torch.Tensor:
    """Area-weighted unit vertex normals of every frame of ``positions``; see the module docstring."""
    require_shape("positions", positions, ("T", "Nv", 3), ("Nv", 3), non_empty=True)
    Nv = positions.shape[-2]
    T = positions.shape[0] if positions.dim() == 3 else 1
    plan = plan_or_faces if isinstance(plan_or_faces, NormalPlan) else NormalPlan(plan_or_faces, Nv)
    if plan.Nv != Nv:
        raise ValueError(f"positions has {Nv} vertices, the plan {plan.Nv}")
    if T * Nv * 3 >= 2 ** 31:
        raise ValueError(f"{T} frames of {Nv} vertices: the trajectory is indexed in 32 bits; split the frames over several calls")
    require_f32_cuda("positions", positions)
    require_index_cuda("faces", plan.faces)
    if plan.device != positions.device:
        raise ValueError(f"faces is on {plan.device}, positions on {positions.device}")
    pos = positions.detach().contiguous()
    out = torch.empty_like(pos)
    launch("a3d_mesh_vertex_normals_f32", pos.device, T, Nv, 3 * plan.F, _p(pos), _p(plan.faces), _p(plan.order), _p(plan.starts), _p(out))
    return out


def split_vertices(faces: torch.Tensor, faces_uvs: Optional[torch.Tensor] = None, *,
                   Nv: Optional[int] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """The glTF vertices of a mesh indexed by position and by UV: the distinct ``(v, vt)`` pairs, ascending; see the module docstring."""
    require_shape("faces", faces, ("F", 3), non_empty=True)
    require_shape("faces_uvs", faces_uvs, tuple(faces.shape), optional=True)
    for name, t in (("faces", faces), ("faces_uvs", faces_uvs)):
        if t is not None and t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name}: expected an int32 / int64 tensor, got {t.dtype}")
    f = faces.detach().long()
    if int(f.min()) < 0 or (faces_uvs is not None and int(faces_uvs.min()) < 0):
        raise IndexError("faces, faces_uvs: indices must not be negative")
    if faces_uvs is None:
        n = int(f.max()) + 1 if Nv is None else int(Nv)
        if int(f.max()) >= n:
            raise IndexError(f"faces: vertex indices must lie in [0, {n}), got {int(f.max())}")
        return torch.arange(n, dtype=torch.int64, device=f.device), None, f
    if faces_uvs.device != f.device:
        raise ValueError(f"faces_uvs is on {faces_uvs.device}, faces on {f.device}")
    uv = faces_uvs.detach().long()
    Nt = int(uv.max()) + 1
    keys, inverse = torch.unique(f.reshape(-1) * Nt + uv.reshape(-1), sorted=True, return_inverse=True)
    split_vertex = torch.div(keys, Nt, rounding_mode="floor")
    return split_vertex, keys - split_vertex * Nt, inverse.reshape(f.shape)


# ---- the file

def _host(name: str, value, dtype, shape) -> Optional[np.ndarray]:
    """``value`` (array or tensor, ``None`` passes) as a contiguous array of ``dtype`` whose shape fits ``shape`` (``None``: any size)."""
    if value is None:
        return None
    a = np.ascontiguousarray(value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value))
    if a.ndim != len(shape) or any(want is not None and want != have for want, have in zip(shape, a.shape)) or 0 in a.shape:
        spelled = ", ".join("*" if s is None else str(s) for s in shape)
        raise ValueError(f"{name}: expected [{spelled}], got {list(a.shape)}")
    if np.issubdtype(np.dtype(dtype), np.floating):
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f"{name}: expected floating point values, got {a.dtype}")
        if not np.isfinite(a).all():
            raise ValueError(f"{name}: {int((~np.isfinite(a)).sum())} values are not finite")
    elif not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: expected integers, got {a.dtype}")
    return a if a.dtype == np.dtype(dtype) else a.astype(dtype)


class _Buffer:
    """The BIN chunk under construction: views, each 4-byte aligned, and the accessors over them."""

    def __init__(self):
        self.data, self.views, self.accessors = bytearray(), [], []

    def view(self, raw: bytes, target: Optional[int] = None) -> int:
        assert len(self.data) % 4 == 0
        v = {"buffer": 0, "byteOffset": len(self.data), "byteLength": len(raw)}
        if target is not None:
            v["target"] = target
        self.views.append(v)
        self.data += raw + b"\0" * (-len(raw) % 4)
        return len(self.views) - 1

    def accessor(self, array: np.ndarray, kind: str, target: Optional[int] = None, bounds: bool = False) -> int:
        component = {np.dtype("<f4"): FLOAT, np.dtype("<u4"): UNSIGNED_INT}[array.dtype]
        a = {"bufferView": self.view(array.tobytes(), target), "componentType": component, "count": int(array.shape[0]), "type": kind}
        if bounds:
            rows = array.reshape(array.shape[0], -1)
            a["min"], a["max"] = [float(x) for x in rows.min(0)], [float(x) for x in rows.max(0)]
        self.accessors.append(a)
        return len(self.accessors) - 1


def write_animated_glb(path, positions, normals, indices, *, uvs=None, texture=None, colors=None, fps: float = 8.0) -> None:
    """One animated ``.glb``: frame 0 as the mesh, one morph target per later frame, linear keys; see the module docstring."""
    fps = float(fps)
    if not (fps > 0.0 and np.isfinite(fps)):
        raise ValueError(f"fps = {fps}: expected a positive finite number")
    if uvs is not None and colors is not None:
        raise ValueError("uvs together with colors: a primitive is textured or vertex-coloured, not both")
    if texture is not None and uvs is None:
        raise ValueError("texture without uvs")
    p = _host("positions", positions, "<f4", (None, None, 3))
    T, Ng = p.shape[:2]
    n = _host("normals", normals, "<f4", (T, Ng, 3))
    idx = _host("indices", indices, np.int64, (None, 3))
    if int(idx.min()) < 0 or int(idx.max()) >= Ng:
        raise ValueError(f"indices: vertex indices must lie in [0, {Ng}), got [{int(idx.min())}, {int(idx.max())}]")
    uv = _host("uvs", uvs, "<f4", (Ng, 2))
    rgb = _host("colors", colors, "<f4", (Ng, 3))
    tex = _host("texture", texture, "<f4", (None, None, 3))

    buf = _Buffer()
    primitive = {"mode": 4, "indices": buf.accessor(idx.reshape(-1).astype("<u4"), "SCALAR", ELEMENT_ARRAY_BUFFER)}
    attributes = {"POSITION": buf.accessor(p[0], "VEC3", ARRAY_BUFFER, bounds=True), "NORMAL": buf.accessor(n[0], "VEC3", ARRAY_BUFFER)}
    if uv is not None:
        flipped = np.stack([uv[:, 0], np.float32(1.0) - uv[:, 1]], 1).astype("<f4")
        attributes["TEXCOORD_0"] = buf.accessor(flipped, "VEC2", ARRAY_BUFFER)
    elif rgb is not None:
        attributes["COLOR_0"] = buf.accessor(rgb, "VEC3", ARRAY_BUFFER)
    primitive["attributes"] = attributes
    mesh = {"primitives": [primitive]}
    gltf = {"asset": {"version": "2.0", "generator": "animate3d_amd.mesh_export"}, "scene": 0, "scenes": [{"nodes": [0]}],
            "nodes": [{"mesh": 0, "name": "animated_mesh"}], "meshes": [mesh]}
    if T > 1:
        primitive["targets"] = [{"POSITION": buf.accessor((p[k] - p[0]).astype("<f4"), "VEC3", ARRAY_BUFFER, bounds=True),
                                 "NORMAL": buf.accessor((n[k] - n[0]).astype("<f4"), "VEC3", ARRAY_BUFFER)} for k in range(1, T)]
        mesh["weights"] = [0.0] * (T - 1)
        times = (np.arange(T, dtype=np.float64) / fps).astype("<f4")
        weights = np.zeros((T, T - 1), dtype="<f4")
        weights[np.arange(1, T), np.arange(T - 1)] = 1.0
        sampler = {"input": buf.accessor(times, "SCALAR", bounds=True), "output": buf.accessor(weights.reshape(-1), "SCALAR"),
                   "interpolation": "LINEAR"}
        gltf["animations"] = [{"name": "trajectory", "samplers": [sampler], "channels": [{"sampler": 0, "target": {"node": 0, "path": "weights"}}]}]
    if tex is not None:
        from PIL import Image
        png = io.BytesIO()
        Image.fromarray(np.clip(np.round(tex * np.float32(255.0)), 0, 255).astype(np.uint8)).save(png, format="PNG")
        gltf["images"] = [{"bufferView": buf.view(png.getvalue()), "mimeType": "image/png"}]
        gltf["samplers"] = [{"magFilter": LINEAR_FILTER, "minFilter": LINEAR_FILTER, "wrapS": CLAMP_TO_EDGE, "wrapT": CLAMP_TO_EDGE}]
        gltf["textures"] = [{"source": 0, "sampler": 0}]
        gltf["materials"] = [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}]
        primitive["material"] = 0
    gltf["buffers"] = [{"byteLength": len(buf.data)}]
    gltf["bufferViews"], gltf["accessors"] = buf.views, buf.accessors

    text = json.dumps(gltf, separators=(",", ":")).encode("ascii")
    text += b" " * (-len(text) % 4)
    total = 12 + 8 + len(text) + 8 + len(buf.data)
    if total >= 2 ** 32:
        raise ValueError(f"{total} bytes: a .glb holds less than 4 GiB; export fewer frames per file")
    with open(path, "wb") as f:
        f.write(struct.pack("<III", GLB_MAGIC, 2, total))
        f.write(struct.pack("<II", len(text), CHUNK_JSON))
        f.write(text)
        f.write(struct.pack("<II", len(buf.data), CHUNK_BIN))
        f.write(bytes(buf.data))


def export_animated_glb(path, trajectory: torch.Tensor, faces: torch.Tensor, *, uvs: Optional[torch.Tensor] = None,
                        faces_uvs: Optional[torch.Tensor] = None, texture: Optional[torch.Tensor] = None,
                        vertex_colors: Optional[torch.Tensor] = None, rot_x_degree: float = 0.0, rot_z_degree: float = 0.0,
                        scale_factor: float = 1.0, fps: float = 8.0) -> Dict[str, np.ndarray]:
    """``stage4d.vertex_trajectory``'s rows and the mesh they came from -> one animated ``.glb``: what the reference's
    ``export_animated_mesh.py`` does inside Blender.  Returns the arrays written: ``positions`` / ``normals [T, Ng, 3]`` (the mesh's own
    frame), ``indices [F, 3]``, ``split_vertex [Ng]`` and, as given, ``split_uv [Ng]``, ``uvs [Ng, 2]`` (unflipped), ``texture``,
    ``colors [Ng, 3]``.  See the module docstring."""
    require_shape("trajectory", trajectory, ("T", "Nv", 3), non_empty=True)
    require_shape("faces", faces, ("F", 3), non_empty=True)
    Nv, F = trajectory.shape[1], faces.shape[0]
    textured = [t is not None for t in (texture, uvs, faces_uvs)]
    if any(textured) and not all(textured):
        raise ValueError("a textured mesh needs texture, uvs and faces_uvs together")
    if any(textured) and vertex_colors is not None:
        raise ValueError("2 colour sources: give at most one of vertex_colors and (texture, uvs, faces_uvs)")
    require_shape("uvs", uvs, ("Nt", 2), non_empty=True, optional=True)
    require_shape("faces_uvs", faces_uvs, (F, 3), optional=True)
    require_shape("texture", texture, ("Ht", "Wt", 3), non_empty=True, optional=True)
    require_shape("vertex_colors", vertex_colors, (Nv, 3), optional=True)
    require_f32_cuda("trajectory", trajectory)
    require_index_cuda("faces", faces)
    dev = trajectory.device
    if faces.device != dev:
        raise ValueError(f"faces is on {faces.device}, trajectory on {dev}")
    plan = NormalPlan(faces, Nv)
    if faces_uvs is not None:
        if faces_uvs.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"faces_uvs: expected an int32 / int64 tensor, got {faces_uvs.dtype}")
        faces_uvs = faces_uvs.to(dev)
        lo, hi = torch.stack([faces_uvs.min(), faces_uvs.max()]).tolist()
        if lo < 0 or hi >= uvs.shape[0]:
            raise IndexError(f"faces_uvs: uv indices must lie in [0, {uvs.shape[0]}), got [{lo}, {hi}]")
    own = to_mesh_frame(trajectory.detach(), rot_x_degree=rot_x_degree, rot_z_degree=rot_z_degree, scale_factor=scale_factor)
    normals = vertex_normals(own, plan)
    split_vertex, split_uv, indices = split_vertices(faces, faces_uvs, Nv=Nv)
    out = dict(positions=own[:, split_vertex], normals=normals[:, split_vertex], indices=indices, split_vertex=split_vertex)
    if split_uv is not None:
        out.update(split_uv=split_uv, uvs=uvs.detach().to(dev)[split_uv], texture=texture.detach())
    elif vertex_colors is not None:
        out["colors"] = vertex_colors.detach().to(dev)[split_vertex]
    arrays = {k: v.cpu().numpy() for k, v in out.items()}
    write_animated_glb(path, arrays["positions"], arrays["normals"], arrays["indices"], uvs=arrays.get("uvs"), texture=arrays.get("texture"),
                       colors=arrays.get("colors"), fps=fps)
    return arrays
