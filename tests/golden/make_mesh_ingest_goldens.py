"""Generate tests/golden/mesh_ingest.npz by running the REFERENCE's own mesh-to-Gaussian code on the CPU.

Run in the build container only (needs the reference tree and scipy):

    python -B tests/golden/make_mesh_ingest_goldens.py <path to the reference tree>

``convert_to_textureVertex_with_average``, ``compute_edge_distances``, ``find_and_save_connected_vertices`` and
``convert_point_cloud_to_gaussian`` with its helpers (tools/mesh_animation/mesh2gaussian.py), ``Gaussian4DModel.load_ply``
(custom/threestudio-animate3d/geometry/gaussian_4d.py) and ``build_rotation_np`` / ``extract_rotation_scipy`` (geometry/utils.py) are
compiled from the reference files as they lie; the modules import pytorch3d and plyfile at their tops, so only these definitions are
executed, and every ``"cuda"`` literal becomes ``"cpu"`` in the syntax tree.  Neither library is installed.  STAND-INS: ``Meshes`` (packed
vertices, faces, textures), ``TexturesVertex``, ``packed_to_list``; a ``TexturesUV`` whose ``faces_verts_textures_packed`` is the torch call
pytorch3d documents for it (``F.grid_sample`` on the row-flipped texture, bilinear, border, ``align_corners=True``), in float32 as
pytorch3d runs it; ``PlyData`` / ``PlyElement`` that keep the float32 record array in memory instead of a file.  Only data is written.

The mesh and the texture: tests/mesh_ingest_ref.golden_mesh (the 24 x 25 jittered curved sheet, a fan whose hub has degree 70, a
duplicated face, a UV seam; texture 5 x 3).  The transform: rot_x = rot_z = 90, scale_factor = 0.76 (the released config).  Recorded:
the inputs, the reference's vertex colours, mean edges, connectivity (CSR in dict order, with the distances), the PLY record and what
``load_ply`` makes of it; and a second PLY record of 100 Gaussians with random orientations, log-scales and ``max_sh_degree = 1``
through ``load_ply``."""
import ast
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import mesh_ingest_ref as ref  # noqa: E402

N2, SEED2 = 100, 5


class OnTheCpu(ast.NodeTransformer):
    def visit_Constant(self, node):
        return ast.Constant("cpu") if node.value == "cuda" else node

    def visit_FunctionDef(self, node):
        self.generic_visit(node)
        node.decorator_list = []
        return node


def extract(path, names):
    """The definitions ``names`` of a file, functions at the top level or methods of any class, as one module."""
    found = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in found:
            found[node.name] = node
    assert not set(names) - set(found), set(names) - set(found)
    return ast.fix_missing_locations(ast.Module(body=[OnTheCpu().visit(found[n]) for n in names], type_ignores=[]))


class TexturesUV:
    def __init__(self, texture, uvs, faces_uvs):
        self.texture, self.uvs, self.faces_uvs = texture, uvs, faces_uvs

    def faces_verts_textures_packed(self):
        grid = (self.uvs[self.faces_uvs] * 2.0 - 1.0)[None]                                    # [1, F, 3, 2]
        image = torch.flip(self.texture, [0]).permute(2, 0, 1)[None]
        return F.grid_sample(image, grid, mode="bilinear", padding_mode="border", align_corners=True)[0].permute(1, 2, 0)


class TexturesVertex:
    def __init__(self, verts_features):
        self.verts_features = verts_features

    def verts_features_packed(self):
        return torch.cat(list(self.verts_features))


class Meshes:
    def __init__(self, verts, faces, textures):
        self.verts, self.faces, self.textures = verts, faces, textures

    def verts_packed(self):
        return self.verts

    def faces_packed(self):
        return self.faces

    def num_verts_per_mesh(self):
        return torch.tensor([self.verts.shape[0]])


def packed_to_list(x, split_size):
    return list(x.split(torch.as_tensor(split_size).tolist(), dim=0))


FILES = {}                                                                                      # path -> the record array a file would hold


class PlyElement:
    def __init__(self, data):
        self.data = data
        self.properties = [types.SimpleNamespace(name=n) for n in data.dtype.names]

    @staticmethod
    def describe(data, name):
        assert name == "vertex"
        return PlyElement(data)

    def __getitem__(self, key):
        return self.data[key]


class PlyData:
    def __init__(self, elements):
        self.elements = elements

    def write(self, path):
        FILES[path] = self.elements[0].data.copy()

    @staticmethod
    def read(path):
        return PlyData([PlyElement(FILES[path])])


class Holder(torch.nn.Module):
    """What ``load_ply`` touches of a ``Gaussian4DModel``."""

    def __init__(self, max_sh_degree):
        super().__init__()
        self.cfg = types.SimpleNamespace(load_ply_cfg=types.SimpleNamespace(rot_x_degree=ref.ROT_X, rot_z_degree=ref.ROT_Z, scale_factor=ref.SCALE))
        self.max_sh_degree = max_sh_degree
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity"):
            self.register_buffer(name, torch.zeros(1))


def loaded(load_ply, path, max_sh_degree, tag):
    h = Holder(max_sh_degree)
    load_ply(h, path)
    return {f"{tag}_xyz": h._xyz, f"{tag}_features_dc": h._features_dc, f"{tag}_features_rest": h._features_rest, f"{tag}_opacity": h._opacity,
            f"{tag}_scaling": h._scaling.detach(), f"{tag}_rotation": h._rotation.detach()}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    geometry = os.path.join(root, "custom", "threestudio-animate3d", "geometry")
    m2g = {"torch": torch, "np": np, "json": json, "TexturesVertex": TexturesVertex, "packed_to_list": packed_to_list, "PlyData": PlyData,
           "PlyElement": PlyElement, "C0": ref.C0}
    names = ("convert_to_textureVertex_with_average", "compute_edge_distances", "find_and_save_connected_vertices",
             "construct_list_of_attributes", "RGB2SH", "inverse_sigmoid", "convert_point_cloud_to_gaussian")
    exec(compile(extract(os.path.join(root, "tools", "mesh_animation", "mesh2gaussian.py"), names), "mesh2gaussian.py", "exec"), m2g)
    utils = {"np": np, "R": Rotation}
    exec(compile(extract(os.path.join(geometry, "utils.py"), ("build_rotation_np", "extract_rotation_scipy")), "utils.py", "exec"), utils)
    g4d = {"np": np, "torch": torch, "nn": torch.nn, "PlyData": PlyData, "build_rotation_np": utils["build_rotation_np"],
           "extract_rotation_scipy": utils["extract_rotation_scipy"]}
    exec(compile(extract(os.path.join(geometry, "gaussian_4d.py"), ("load_ply",)), "gaussian_4d.py", "exec"), g4d)

    mesh = ref.golden_mesh()
    t = {k: torch.from_numpy(v) for k, v in mesh.items()}
    meshes = Meshes(t["verts"], t["faces"], TexturesUV(t["texture"], t["uvs"], t["faces_uvs"]))
    # main() of mesh2gaussian.py, :158-176
    colored = m2g["convert_to_textureVertex_with_average"](meshes)
    verts_pos = meshes.verts_packed().cpu().numpy()
    verts_colors = colored.verts_features_packed().cpu().numpy()
    mean_edge = m2g["compute_edge_distances"](meshes).cpu().numpy()
    m2g["convert_point_cloud_to_gaussian"](verts_pos, verts_colors, mean_edge / ref.SHRINK, "mesh.ply")
    with tempfile.TemporaryDirectory() as tmp:
        m2g["find_and_save_connected_vertices"](meshes, os.path.join(tmp, "mesh.json"))
        info = json.load(open(os.path.join(tmp, "mesh.json")))
    Nv = verts_pos.shape[0]
    assert sorted(info, key=int) == [str(v) for v in range(Nv)]
    rows = [[int(u) for u in info[str(v)]] for v in range(Nv)]
    dist = np.array([w for v in range(Nv) for w in info[str(v)].values()], dtype=np.float64)
    assert np.array_equal(dist.astype(np.float32).astype(np.float64), dist)                     # `.item()` of fp32 norms: fp32 values
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    record = FILES["mesh.ply"]
    out = dict(mesh, faces=mesh["faces"].astype(np.int32), faces_uvs=mesh["faces_uvs"].astype(np.int32), colors=verts_colors, mean_edge=mean_edge, row_start=row_start, col=np.array([u for r in rows for u in r], dtype=np.int32),
               distance=dist.astype(np.float32), ply_names=np.array(record.dtype.names), ply=np.stack([record[n] for n in record.dtype.names], 1),
               frame=np.array([ref.ROT_X, ref.ROT_Z, ref.SCALE, ref.SHRINK]))
    out.update({k: v.numpy() for k, v in loaded(g4d["load_ply"], "mesh.ply", 0, "loaded").items()})

    rng = np.random.default_rng(SEED2)
    names2 = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(9)] + ["opacity"] + \
             [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    table = rng.standard_normal((N2, len(names2))).astype(np.float32)
    table[:, names2.index("scale_0"):names2.index("scale_0") + 3] -= 4.0
    record2 = np.empty(N2, dtype=[(n, "f4") for n in names2])
    for i, n in enumerate(names2):
        record2[n] = table[:, i]
    FILES["random.ply"] = record2
    out.update(ply2_names=np.array(names2), ply2=table)
    out.update({k: v.numpy() for k, v in loaded(g4d["load_ply"], "random.ply", 1, "loaded2").items()})

    path = os.path.join(HERE, "mesh_ingest.npz")
    np.savez_compressed(path, **out)
    deg = np.diff(row_start)
    print(f"{Nv} vertices, {len(mesh['faces'])} faces, degrees {deg.min()} .. {deg.max()}, {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
