"""The mesh ingest without a GPU: the float64 restatement (tests/mesh_ingest_ref.py) against the reference's own results
(tests/golden/mesh_ingest.npz, written by tests/golden/make_mesh_ingest_goldens.py), the files (OBJ, PLY, the connectivity JSON), every
refusal of animate3d_amd/mesh.py that needs no device, and the C-ABI refusals of csrc/mesh_ingest.hip through ctypes."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from animate3d_amd import arap, mesh
from tests import mesh_ingest_ref as ref

A3D_EINVAL = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_ingest.npz")
FRAME = dict(rot_x_degree=ref.ROT_X, rot_z_degree=ref.ROT_Z, scale_factor=ref.SCALE)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def mesh_of(golden):
    return dict(verts=golden["verts"], faces=golden["faces"].astype(np.int64), texture=golden["texture"], uvs=golden["uvs"],
                faces_uvs=golden["faces_uvs"].astype(np.int64))


def grid_sample_error(texture, uvs, faces_uvs):
    """e32: torch's float32 ``grid_sample`` on the CPU against its float64 one, on the corner UVs of the mesh (the largest difference)."""
    def run(dtype):
        grid = (torch.from_numpy(np.asarray(uvs)).to(dtype)[torch.from_numpy(np.asarray(faces_uvs)).long()] * 2 - 1)[None]
        image = torch.flip(torch.from_numpy(np.asarray(texture)).to(dtype), [0]).permute(2, 0, 1)[None]
        return F.grid_sample(image, grid, mode="bilinear", padding_mode="border", align_corners=True)[0].permute(1, 2, 0)
    return float((run(torch.float32).double() - run(torch.float64)).abs().max()), run(torch.float64).numpy()


def restated(golden):
    m = mesh_of(golden)
    return ref.restate(m["verts"], m["faces"], texture=m["texture"], uvs=m["uvs"], faces_uvs=m["faces_uvs"], shrink=ref.SHRINK, **FRAME)


def golden_rows(golden):
    start, col = golden["row_start"], golden["col"]
    return [col[start[v]:start[v + 1]].tolist() for v in range(len(start) - 1)]


def test_golden_inputs_are_the_shared_mesh(golden):
    for k, v in ref.golden_mesh().items():
        assert np.array_equal(golden[k], v), k
    assert golden["verts"].shape == (671, 3) and golden["texture"].shape == (ref.TEX_H, ref.TEX_W, 3)
    assert tuple(golden["frame"]) == (ref.ROT_X, ref.ROT_Z, ref.SCALE, ref.SHRINK)
    m = mesh_of(golden)
    dup = [tuple(f) for f in m["faces"].tolist()]
    assert len(set(dup)) == len(dup) - 1                                                       # one duplicated face
    seam = m["faces_uvs"][m["faces"] == ref.SEAM_VERTEX]
    assert len(set(seam.tolist())) == 2                                                        # one vertex, two UVs
    uv = m["uvs"]
    assert (uv == 0).any() and (uv == 1).any() and (uv < 0).any() and (uv > 1).any()


def test_bilinear_restatement_is_grid_sample(golden):
    m = mesh_of(golden)
    e32, want = grid_sample_error(m["texture"], m["uvs"], m["faces_uvs"])
    got = ref.sample_texture(m["texture"], m["uvs"].astype(np.float64)[m["faces_uvs"]])
    assert np.abs(got - want).max() <= 4 * 2.0 ** -53 * 4 and 0 < e32 < 1e-5, (np.abs(got - want).max(), e32)


def test_restatement_reproduces_the_reference(golden):
    """The float64 restatement against what the reference computed in fp32 and stored as float32: its own rounding is of the kernel's
    kind (it sums the same terms, in fp32, in another order), so the kernel's bars hold for it, plus u for the file."""
    m, r = mesh_of(golden), restated(golden)
    e32, _ = grid_sample_error(m["texture"], m["uvs"], m["faces_uvs"])
    bar = ref.bars(r, m["verts"], scale_factor=ref.SCALE, textured_e32=e32, golden=True)
    rows = golden_rows(golden)
    assert [sorted(x) for x in rows] == r["rows"] and any(x != sorted(x) for x in rows)       # equal as sets, not in order
    deg = np.diff(r["row_start"])
    assert deg.max() == ref.FAN and deg.min() == 2 and int(r["corners"].max()) >= ref.FAN
    position = {(v, u): r["row_start"][v] + i for v, row in enumerate(r["rows"]) for i, u in enumerate(row)}
    at = np.array([position[(v, u)] for v, row in enumerate(rows) for u in row])
    names = golden["ply_names"].tolist()
    ply = {n: golden["ply"][:, i] for i, n in enumerate(names)}
    unrotated = ref.restate(m["verts"], m["faces"], vertex_colors=r["colors"], shrink=ref.SHRINK)
    checks = {"edge_length": (golden["distance"], r["edge_length"][at], bar["edge_length"][at]),
              "mean_edge": (golden["mean_edge"], r["mean_edge"], bar["mean_edge"]),
              "colors": (golden["colors"], r["colors"], bar["colors"]),
              "ply f_dc": (np.stack([ply[f"f_dc_{i}"] for i in range(3)], 1), r["shs"], bar["shs"]),
              "ply scale": (np.stack([ply[f"scale_{i}"] for i in range(3)], 1), unrotated["scaling"], bar["scaling"]),
              "loaded xyz": (golden["loaded_xyz"], r["xyz"], bar["xyz"]),
              "loaded scaling": (golden["loaded_scaling"], r["scaling"], bar["scaling"]),
              "loaded features_dc": (golden["loaded_features_dc"][:, 0], r["shs"], bar["shs"])}
    for name, (got, want, b) in checks.items():
        ratio, exact = ref.worst(got, want, b)
        print(f"[mesh ingest restatement vs reference] {name}: worst error / bar {ratio:.3f}")
        assert ratio <= 1.0 and exact, (name, ratio)
    assert np.array_equal(np.stack([ply[k] for k in "xyz"], 1), m["verts"])
    assert np.allclose(ply["opacity"], np.log(ref.OPACITY / (1 - ref.OPACITY)), rtol=1e-6)
    assert golden["loaded_features_rest"].shape == (671, 0, 3)
    R = ref.rotation_matrices(golden["loaded_rotation"])
    assert np.abs(R - r["R"][None]).max() <= 8 * ref.U
    q = mesh.quaternion_of(mesh.frame_rotation(ref.ROT_X, ref.ROT_Z))
    assert q[0] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-15 and np.abs(ref.rotation_matrices(q[None])[0] - r["R"]).max() < 1e-15
    assert np.array_equal(mesh.frame_rotation(ref.ROT_X, ref.ROT_Z), r["R"])


def test_quaternion_of_every_branch():
    rng = np.random.default_rng(0)
    qs = rng.standard_normal((50, 4))
    qs = np.concatenate([qs, np.eye(4), [[1e-9, 1, 0, 0], [0, 0.6, 0.8, 0], [-0.5, 0.5, 0.5, 0.5]]])
    for q in qs:
        R = ref.rotation_matrices(q[None])[0]
        got = mesh.quaternion_of(R)
        assert got[0] >= 0 and np.abs(ref.rotation_matrices(got[None])[0] - R).max() < 1e-14, q


# ---- files

OBJ_COLOURED = """# a square pyramid with vertex colours; a quad base, negative indices, every corner form
v 0 0 0 1 0 0
v 1 0 0 0 1 0
v 1 1 0 0 0 1
v 0 1 0 1 1 0
v 0.5 0.5 1 0.5 0.5 0.5
vn 0 0 1
vt 0 0
f 1 4 3 2
f 1/1 2/1 5/1
f 2/1/1 3/1/1 5/1/1
f 3//1 4//1 5//1
f -2 -5 -1
"""


def test_load_obj_vertex_colours(tmp_path):
    p = tmp_path / "pyramid.obj"
    p.write_text(OBJ_COLOURED)
    m = mesh.load_obj(str(p))
    assert m.verts.dtype == torch.float32 and m.verts.shape == (5, 3) and m.faces.dtype == torch.int64
    assert m.faces.tolist() == [[0, 3, 2], [0, 2, 1], [0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]]       # the quad as a fan
    assert list(m.colors) == ["vertex_colors"] and m.colors["vertex_colors"][4].tolist() == [0.5, 0.5, 0.5]
    (tmp_path / "bare.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="no colour source"):
        mesh.load_obj(str(tmp_path / "bare.obj"))
    (tmp_path / "bad.obj").write_text("v 0 0 0 1 1 1\nv 1 0 0 1 1 1\nv 0 1 0 1 1 1\nf 1 2 4\n")
    with pytest.raises(ValueError, match="vertex index 4"):
        mesh.load_obj(str(tmp_path / "bad.obj"))
    (tmp_path / "empty.obj").write_text("v 0 0 0\n")
    with pytest.raises(ValueError):
        mesh.load_obj(str(tmp_path / "empty.obj"))


def test_load_obj_textured(tmp_path):
    from PIL import Image
    pixels = (np.arange(5 * 3 * 3).reshape(5, 3, 3) * 5).astype(np.uint8)
    Image.fromarray(pixels).save(tmp_path / "skin.png")
    (tmp_path / "one.mtl").write_text("newmtl skin\nKd 1 1 1\nmap_Kd skin.png\n")
    body = "mtllib one.mtl\nusemtl skin\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvt 1 1\nvt 0.5 0.5\nf 1/1 2/2 3/3\nf 2/2 4/4 3/5\n"
    (tmp_path / "quad.obj").write_text(body)
    m = mesh.load_obj(str(tmp_path / "quad.obj"))
    assert sorted(m.colors) == ["faces_uvs", "texture", "uvs"]
    assert torch.equal(m.colors["texture"], torch.from_numpy(pixels.astype(np.float32) / 255.0))
    assert m.colors["faces_uvs"].tolist() == [[0, 1, 2], [1, 3, 4]] and m.colors["uvs"].shape == (5, 2)   # vertex 2 has two UVs
    assert m.faces.tolist() == [[0, 1, 2], [1, 3, 2]]
    (tmp_path / "two.mtl").write_text("newmtl a\nmap_Kd skin.png\nnewmtl b\nmap_Kd skin.png\n")
    (tmp_path / "two.obj").write_text(body.replace("one.mtl", "two.mtl"))
    with pytest.raises(NotImplementedError, match="2 materials"):
        mesh.load_obj(str(tmp_path / "two.obj"))
    (tmp_path / "libs.obj").write_text(body.replace("mtllib one.mtl", "mtllib one.mtl two.mtl"))
    with pytest.raises(NotImplementedError):
        mesh.load_obj(str(tmp_path / "libs.obj"))


def test_gaussian_ply_round_trip_and_the_reference_record(golden, tmp_path):
    """``write_gaussian_ply`` on the reference's own colours and mean edges gives the reference's PLY record (it computes in fp32 where
    this computes in float64 and rounds once: 3 u relative for f_dc, u absolute + 3 ulp for the logarithm), and the parser returns what
    was written."""
    path = str(tmp_path / "mesh.ply")
    mesh.write_gaussian_ply(path, torch.from_numpy(golden["verts"]), golden["colors"], golden["mean_edge"], shrink=ref.SHRINK, opacity=ref.OPACITY)
    rec = mesh.parse_gaussian_ply(path)
    names = golden["ply_names"].tolist()
    assert list(mesh.parse_ply_vertices(path)) == names
    ply = {n: golden["ply"][:, i] for i, n in enumerate(names)}
    want = {"xyz": np.stack([ply[k] for k in "xyz"], 1), "f_dc": np.stack([ply[f"f_dc_{i}"] for i in range(3)], 1),
            "scale": np.stack([ply[f"scale_{i}"] for i in range(3)], 1), "rot": np.stack([ply[f"rot_{i}"] for i in range(4)], 1),
            "opacity": ply["opacity"][:, None]}
    assert np.array_equal(rec["xyz"], want["xyz"]) and np.array_equal(rec["rot"], want["rot"]) and rec["f_rest"].shape == (671, 0)
    assert np.abs(rec["f_dc"] - want["f_dc"]).max() <= 3 * ref.U * np.abs(want["f_dc"]).max()
    assert (np.abs(rec["scale"].astype(np.float64) - want["scale"]) <= ref.U + 3 * ref.ulp32(want["scale"])).all()
    assert np.allclose(rec["opacity"], want["opacity"], rtol=1e-6)
    exact = np.log(golden["mean_edge"].astype(np.float64) / ref.SHRINK).astype(np.float32)
    assert np.array_equal(rec["scale"], exact)
    with pytest.raises(ValueError):
        mesh.write_gaussian_ply(path, golden["verts"], golden["colors"][:5], golden["mean_edge"])


def test_ply_parser_formats_and_refusals(golden, tmp_path):
    names, table = golden["ply2_names"].tolist(), golden["ply2"]
    ref.write_ply(str(tmp_path / "b.ply"), names, table)
    ref.write_ply(str(tmp_path / "a.ply"), names, table, ascii=True)
    b, a = mesh.parse_gaussian_ply(str(tmp_path / "b.ply")), mesh.parse_gaussian_ply(str(tmp_path / "a.ply"))
    for k in b:
        assert b[k].dtype == np.float32 and np.array_equal(b[k], a[k]), k
    assert b["f_rest"].shape == (100, 9) and np.array_equal(b["f_rest"][:, 4], table[:, names.index("f_rest_4")])
    assert np.array_equal(b["rot"], table[:, -4:]) and np.array_equal(b["opacity"][:, 0], table[:, names.index("opacity")])
    (tmp_path / "junk.ply").write_bytes(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        mesh.parse_ply_vertices(str(tmp_path / "junk.ply"))
    head = "ply\nformat binary_big_endian 1.0\nelement vertex 1\nproperty float x\nend_header\n"
    (tmp_path / "big.ply").write_bytes(head.encode() + b"\0\0\0\0")
    with pytest.raises(NotImplementedError):
        mesh.parse_ply_vertices(str(tmp_path / "big.ply"))
    (tmp_path / "list.ply").write_bytes(head.replace("big", "little").replace("float x", "list uchar int x").encode() + b"\0")
    with pytest.raises(ValueError, match="scalar"):
        mesh.parse_ply_vertices(str(tmp_path / "list.ply"))
    (tmp_path / "short.ply").write_bytes(head.replace("big", "little").replace("vertex 1", "vertex 2").encode() + b"\0\0\0\0")
    with pytest.raises(ValueError, match="do not fit"):
        mesh.parse_ply_vertices(str(tmp_path / "short.ply"))
    ref.write_ply(str(tmp_path / "xyz.ply"), ["x", "y", "z"], table[:, :3])
    with pytest.raises(ValueError, match="not a 3DGS PLY"):
        mesh.parse_gaussian_ply(str(tmp_path / "xyz.ply"))
    with pytest.raises(ValueError, match="f_rest"):                                            # 9 f_rest properties are max_sh_degree 1
        mesh.read_gaussian_ply(str(tmp_path / "b.ply"), max_sh_degree=2)
    with pytest.raises(ValueError):
        mesh.read_gaussian_ply(str(tmp_path / "b.ply"), max_sh_degree=1, scale_factor=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.read_gaussian_ply(str(tmp_path / "b.ply"), max_sh_degree=1, device="cpu")


def test_connected_vertices_round_trip(golden, tmp_path):
    m, r = mesh_of(golden), restated(golden)
    graph = arap.MeshGraph.from_faces(torch.from_numpy(m["faces"]), 671)
    assert graph.col.tolist() == r["col"].tolist()
    lengths = torch.from_numpy(r["edge_length"].astype(np.float32))
    path = str(tmp_path / "mesh.json")
    mesh.write_connected_vertices(path, graph, lengths)
    info = json.load(open(path))
    back = arap.MeshGraph.from_connected_vertices(info, "cpu")
    assert torch.equal(back.row_start, graph.row_start) and torch.equal(back.col, graph.col)
    rows = golden_rows(golden)
    assert all(set(int(u) for u in info[str(v)]) == set(rows[v]) for v in range(671))          # the reference's rows, as sets
    flat = [w for v in range(671) for w in info[str(v)].values()]
    assert flat == lengths.double().tolist()
    nn_idx, max_idx = arap.prepare_arap_from_mesh_vertices(info)
    assert nn_idx.shape == (671, ref.FAN) and int(max_idx.sum()) == graph.col.shape[0]
    with pytest.raises(ValueError):
        mesh.write_connected_vertices(path, graph, lengths[:-1])


# ---- refusals that need no device

def _cpu_mesh():
    verts, faces = ref.tetrahedron()
    return torch.from_numpy(verts), torch.from_numpy(faces)


def test_colour_sources_and_arguments():
    v, f = _cpu_mesh()
    vc, cc = torch.rand(4, 3), torch.rand(4, 3, 3)
    tex = dict(texture=torch.rand(5, 3, 3), uvs=torch.rand(6, 2), faces_uvs=torch.zeros(4, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="0 colour sources"):
        mesh.gaussians_from_mesh(v, f)
    with pytest.raises(ValueError, match="2 colour sources"):
        mesh.gaussians_from_mesh(v, f, vertex_colors=vc, corner_colors=cc)
    with pytest.raises(ValueError, match="2 colour sources"):
        mesh.gaussians_from_mesh(v, f, vertex_colors=vc, **tex)
    with pytest.raises(ValueError, match="3 colour sources"):
        mesh.gaussians_from_mesh(v, f, vertex_colors=vc, corner_colors=cc, uvs=tex["uvs"])
    with pytest.raises(ValueError, match="together"):
        mesh.gaussians_from_mesh(v, f, texture=tex["texture"], uvs=tex["uvs"])
    with pytest.raises(TypeError):
        mesh.gaussians_from_mesh(v.numpy(), f, vertex_colors=vc)
    with pytest.raises(TypeError):
        mesh.gaussians_from_mesh(v, f, vertex_colors=vc.tolist())
    for bad in (dict(vertex_colors=torch.rand(5, 3)), dict(corner_colors=torch.rand(4, 3)), dict(tex, texture=torch.rand(0, 3, 3)),
                dict(tex, texture=torch.rand(5, 3, 4)), dict(tex, uvs=torch.rand(6, 3)), dict(tex, faces_uvs=torch.zeros(3, 3, dtype=torch.int64)),
                dict(tex, faces_uvs=torch.zeros(4, 3))):
        with pytest.raises(ValueError):
            mesh.gaussians_from_mesh(v, f, **bad)
    with pytest.raises(ValueError):
        mesh.gaussians_from_mesh(v[:, :2], f, vertex_colors=vc)
    with pytest.raises(ValueError):
        mesh.gaussians_from_mesh(v, f.float(), vertex_colors=vc)
    for bad in (dict(shrink=0.0), dict(shrink=-1.1), dict(scale_factor=0.0), dict(scale_factor=float("nan")), dict(opacity=0.0), dict(opacity=1.5)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            mesh.gaussians_from_mesh(v, f, vertex_colors=vc, **bad)
    with pytest.raises(IndexError):
        mesh.gaussians_from_mesh(v, f + 1, vertex_colors=vc)
    with pytest.raises(IndexError, match="uv"):
        mesh.gaussians_from_mesh(v, f, **dict(tex, faces_uvs=tex["faces_uvs"] + 6))
    lonely = torch.cat([v, torch.ones(2, 3)])
    with pytest.raises(ValueError, match="2 of 6 vertices are in no face"):
        mesh.gaussians_from_mesh(lonely, f, vertex_colors=torch.rand(6, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                 # a valid call on CPU tensors
        mesh.gaussians_from_mesh(v, f, vertex_colors=vc)


def test_to_mesh_frame_inverts_the_transform():
    x = torch.randn(3, 50, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    R = torch.from_numpy(ref.frame(30.0, -70.0))
    moved = 0.76 * (x @ R.T)
    back = mesh.to_mesh_frame(moved, rot_x_degree=30.0, rot_z_degree=-70.0, scale_factor=0.76)
    assert back.dtype == torch.float64 and (back - x).abs().max() < 1e-14
    assert torch.equal(mesh.to_mesh_frame(x.float()), x.float() @ torch.eye(3))
    with pytest.raises(ValueError):
        mesh.to_mesh_frame(x[0])
    with pytest.raises(ValueError):
        mesh.to_mesh_frame(x, scale_factor=0.0)


# ---- the C-ABI of csrc/mesh_ingest.hip, as tests/test_cabi_contract.py holds the other entry points: made-up device addresses, every
# call differs from a valid launch in at least one operand, and never in none

BASE = 0x7F00_0010_0000
DEVICE = ("verts", "row_start", "col", "corner_order", "corner_start", "vertex_colors", "corner_colors", "texture", "uvs", "corner_uv", "xyz",
          "scaling", "shs", "colors", "mean_edge", "edge_length")
SOURCES = {"vertex": ("vertex_colors",), "corner": ("corner_colors",), "texture": ("texture",)}
VALID = dict(Nv=300, E=1800, C=1700, Ht=5, Wt=3, Nt=400, scale_factor=0.76, shrink=1.1)


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.load_library()


def _doubles(n):
    import ctypes
    return (ctypes.c_double * n)(*([1.0] + [0.0] * (n - 1)))


def _mesh_call(lib, source="texture", ptr=None, rot9="host", **scalars):
    """A call that would be valid for the colour source ``source`` but for ``ptr`` (operand -> another address or None), ``rot9`` and
    ``scalars``.  ``source`` may also be a tuple of colour operands to pass at once (none, or several)."""
    assert ptr or scalars or rot9 != "host" or not isinstance(source, str), "a fully valid call would launch a kernel on made-up addresses"
    p = {n: BASE + 0x10_0000 * i for i, n in enumerate(DEVICE)}
    for n in ("vertex_colors", "corner_colors", "texture"):
        if n not in (SOURCES[source] if isinstance(source, str) else source):
            p[n] = None
    p.update(ptr or {})
    g = dict(VALID, **scalars)
    return lib.a3d_mesh_vertex_gaussians_f32(None, g["Nv"], g["E"], g["C"], p["verts"], p["row_start"], p["col"], p["corner_order"],
                                             p["corner_start"], p["vertex_colors"], p["corner_colors"], p["texture"], g["Ht"], g["Wt"],
                                             p["uvs"], g["Nt"], p["corner_uv"], _doubles(9) if rot9 == "host" else None, g["scale_factor"],
                                             g["shrink"], p["xyz"], p["scaling"], p["shs"], p["colors"], p["mean_edge"], p["edge_length"])


def test_mesh_vertex_gaussians_refusals(lib):
    """Before any launch: a NULL required pointer, Nv <= 0, zero or two colour sources, a texture extent below 1, shrink <= 0 or
    scale_factor <= 0 (or not finite), a misaligned pointer."""
    for operand in ("verts", "row_start", "col", "xyz", "scaling", "shs", "colors", "mean_edge", "edge_length"):
        for source in SOURCES:
            assert _mesh_call(lib, source, ptr={operand: None}) == A3D_EINVAL, f"NULL {operand} ({source})"
        assert _mesh_call(lib, ptr={operand: BASE + 2}) == A3D_EINVAL, f"{operand} misaligned"
    for operand in ("corner_order", "corner_start"):
        for source in ("corner", "texture"):
            assert _mesh_call(lib, source, ptr={operand: None}) == A3D_EINVAL, f"NULL {operand} ({source})"
    for operand in ("uvs", "corner_uv"):
        assert _mesh_call(lib, "texture", ptr={operand: None}) == A3D_EINVAL, f"NULL {operand}"
    assert _mesh_call(lib, rot9=None) == A3D_EINVAL
    for source in SOURCES:
        for scalars in (dict(Nv=0), dict(Nv=-5), dict(E=-1), dict(shrink=0.0), dict(shrink=-1.1), dict(shrink=float("nan")),
                        dict(scale_factor=0.0), dict(scale_factor=-0.76), dict(scale_factor=float("inf"))):
            assert _mesh_call(lib, source, **scalars) == A3D_EINVAL, (source, scalars)
    for scalars in (dict(Ht=0), dict(Wt=0), dict(Ht=-1), dict(Nt=0), dict(C=0)):
        assert _mesh_call(lib, "texture", **scalars) == A3D_EINVAL, scalars
    assert _mesh_call(lib, "corner", C=0) == A3D_EINVAL
    for several in ((), ("vertex_colors", "corner_colors"), ("vertex_colors", "texture"), ("corner_colors", "texture"),
                    ("vertex_colors", "corner_colors", "texture")):
        assert _mesh_call(lib, several) == A3D_EINVAL, several


RIGID = ("xyz_in", "scaling_in", "rotation_in", "xyz", "scaling", "rotation")


def _rigid_call(lib, ptr=None, rot9="host", quat4="host", **scalars):
    assert ptr or scalars or rot9 != "host" or quat4 != "host", "a fully valid call would launch a kernel on made-up addresses"
    p = {n: BASE + 0x10_0000 * i for i, n in enumerate(RIGID)}
    p.update(ptr or {})
    g = dict(dict(N=300, scale_factor=0.76), **scalars)
    return lib.a3d_gaussians_rigid_f32(None, g["N"], p["xyz_in"], p["scaling_in"], p["rotation_in"], _doubles(9) if rot9 == "host" else None,
                                       _doubles(4) if quat4 == "host" else None, g["scale_factor"], p["xyz"], p["scaling"], p["rotation"])


def test_gaussians_rigid_refusals(lib):
    for operand in RIGID:
        assert _rigid_call(lib, ptr={operand: None}) == A3D_EINVAL, f"NULL {operand}"
        assert _rigid_call(lib, ptr={operand: BASE + 2}) == A3D_EINVAL, f"{operand} misaligned"
    assert _rigid_call(lib, rot9=None) == A3D_EINVAL and _rigid_call(lib, quat4=None) == A3D_EINVAL
    for scalars in (dict(N=0), dict(N=-1), dict(scale_factor=0.0), dict(scale_factor=-1.0), dict(scale_factor=float("nan"))):
        assert _rigid_call(lib, **scalars) == A3D_EINVAL, scalars
