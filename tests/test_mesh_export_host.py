"""The mesh export without a GPU (animate3d_amd/mesh_export.py): the vertex split, the GLB writer read back through the minimal reader of
tests/mesh_export_ref.py (every structural rule of the module docstring, every array bit for bit), the colour sources, every refusal that
needs no device, the restatement's own self-check, and the C-ABI refusals of csrc/mesh_export.hip through ctypes."""
import io
import os

import numpy as np
import pytest
import torch

from animate3d_amd import mesh_export
from tests import mesh_export_ref as ref

A3D_EINVAL = -1


# ---- splitting

def test_split_vertices_on_a_seamed_cube():
    verts, faces, uvs, faces_uvs = ref.seamed_cube()
    assert verts.shape == (8, 3) and uvs.shape == (14, 2) and set(faces.reshape(-1)) == set(range(8)) and set(faces_uvs.reshape(-1)) == set(range(14))
    pairs = sorted(set(zip(faces.reshape(-1).tolist(), faces_uvs.reshape(-1).tolist())))
    assert len(pairs) > 14                                                                    # a seam: more pairs than UVs or positions
    sv, su, idx = mesh_export.split_vertices(torch.from_numpy(faces), torch.from_numpy(faces_uvs))
    assert sv.dtype == su.dtype == idx.dtype == torch.int64 and idx.shape == (12, 3)
    assert list(zip(sv.tolist(), su.tolist())) == pairs                                       # Ng distinct pairs, ascending by (v, vt)
    assert torch.equal(sv[idx], torch.from_numpy(faces)) and torch.equal(su[idx], torch.from_numpy(faces_uvs))
    sv32, su32, idx32 = mesh_export.split_vertices(torch.from_numpy(faces).int(), torch.from_numpy(faces_uvs).int())
    assert torch.equal(sv32, sv) and torch.equal(su32, su) and torch.equal(idx32, idx)


def test_split_vertices_without_uvs_is_the_identity():
    _, faces, _, faces_uvs = ref.seamed_cube()
    sv, su, idx = mesh_export.split_vertices(torch.from_numpy(faces))
    assert su is None and sv.tolist() == list(range(8)) and torch.equal(idx, torch.from_numpy(faces))
    sv, _, _ = mesh_export.split_vertices(torch.from_numpy(faces), None, Nv=11)
    assert sv.tolist() == list(range(11))
    with pytest.raises(ValueError):
        mesh_export.split_vertices(torch.from_numpy(faces), torch.from_numpy(faces_uvs[:5]))
    with pytest.raises(ValueError):
        mesh_export.split_vertices(torch.from_numpy(faces).float())
    with pytest.raises(IndexError):
        mesh_export.split_vertices(torch.from_numpy(faces), None, Nv=7)
    with pytest.raises(IndexError):
        mesh_export.split_vertices(torch.from_numpy(faces) - 1)


# ---- the writer, read back

FPS = 7.0


def _case(T, seed=0):
    """The seamed cube, split, with T random frames and random unit normals."""
    verts, faces, uvs, faces_uvs = ref.seamed_cube()
    sv, su, idx = mesh_export.split_vertices(torch.from_numpy(faces), torch.from_numpy(faces_uvs))
    rng = np.random.default_rng(seed)
    p = (verts[sv.numpy()][None] + 0.1 * rng.standard_normal((T, len(sv), 3))).astype(np.float32)
    n = rng.standard_normal((T, len(sv), 3))
    n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    return dict(p=p, n=n, idx=idx.numpy(), uvs=uvs[su.numpy()].astype(np.float32), Ng=len(sv),
                texture=rng.random((6, 5, 3)).astype(np.float32), colors=rng.random((len(sv), 3)).astype(np.float32))


def _check_structure(g, T, Ng, F):
    """The rules of the glTF 2.0 specification the writer has to honour, whatever the colour source."""
    j, raw = g.json, g.raw
    assert raw["magic"] == 0x46546C67 and raw["version"] == 2 and raw["length"] == raw["size"] == raw["end"]   # header length = file size
    assert raw["json_type"] == 0x4E4F534A and raw["bin_type"] == 0x004E4942
    assert raw["json_length"] % 4 == 0 and raw["bin_length"] % 4 == 0
    stripped = raw["json_text"].rstrip(b" ")
    assert stripped.endswith(b"}") and b"\0" not in raw["json_text"]                                            # JSON padded with spaces
    assert j["asset"]["version"] == "2.0" and j["scene"] == 0 and j["scenes"] == [{"nodes": [0]}] and j["nodes"][0]["mesh"] == 0
    assert len(j["buffers"]) == 1 and "uri" not in j["buffers"][0] and j["buffers"][0]["byteLength"] == raw["bin_length"]
    assert len(j["meshes"]) == 1 and len(j["meshes"][0]["primitives"]) == 1
    prim = j["meshes"][0]["primitives"][0]
    covered = np.zeros(raw["bin_length"], dtype=bool)
    for v in j["bufferViews"]:
        assert v["buffer"] == 0 and v["byteOffset"] % 4 == 0 and v["byteOffset"] + v["byteLength"] <= raw["bin_length"]
        assert not covered[v["byteOffset"]:v["byteOffset"] + v["byteLength"]].any()
        covered[v["byteOffset"]:v["byteOffset"] + v["byteLength"]] = True
    assert not np.frombuffer(g.bin, dtype=np.uint8)[~covered].any()                                             # BIN padded with zeros
    vertex = list(prim["attributes"].values()) + [a for t in prim.get("targets", []) for a in t.values()]
    for i, a in enumerate(j["accessors"]):
        want = 34963 if i == prim["indices"] else 34962 if i in vertex else None
        assert j["bufferViews"][a["bufferView"]].get("target") == want, i
    for im in j.get("images", []):
        assert "target" not in j["bufferViews"][im["bufferView"]]
    ia = j["accessors"][prim["indices"]]
    assert prim["mode"] == 4 and ia["componentType"] == 5125 and ia["type"] == "SCALAR" and ia["count"] == 3 * F
    positions = [prim["attributes"]["POSITION"]] + [t["POSITION"] for t in prim.get("targets", [])]
    for i in positions:
        a, arr = j["accessors"][i], g.accessor(i)
        assert a["type"] == "VEC3" and a["componentType"] == 5126 and a["count"] == Ng
        assert a["min"] == arr.min(0).astype(np.float64).tolist() and a["max"] == arr.max(0).astype(np.float64).tolist()
    if T == 1:
        assert "targets" not in prim and "weights" not in j["meshes"][0] and "animations" not in j
    else:
        assert len(prim["targets"]) == T - 1 and all(sorted(t) == ["NORMAL", "POSITION"] for t in prim["targets"])
        assert j["meshes"][0]["weights"] == [0.0] * (T - 1)
        assert len(j["animations"]) == 1 and len(j["animations"][0]["samplers"]) == 1
        assert j["animations"][0]["channels"] == [{"sampler": 0, "target": {"node": 0, "path": "weights"}}]
        s = j["animations"][0]["samplers"][0]
        assert s["interpolation"] == "LINEAR"
        ta, times = j["accessors"][s["input"]], g.accessor(s["input"])
        assert ta["type"] == "SCALAR" and ta["min"] == [float(times.min())] and ta["max"] == [float(times.max())]
        assert j["accessors"][s["output"]]["count"] == T * (T - 1)
    return prim


@pytest.mark.parametrize("T", [1, 2, 4])
def test_writer_round_trip(T, tmp_path):
    c = _case(T)
    path = str(tmp_path / f"t{T}.glb")
    assert mesh_export.write_animated_glb(path, c["p"], torch.from_numpy(c["n"]), c["idx"], uvs=c["uvs"], texture=c["texture"], fps=FPS) is None
    g = ref.Glb(path)
    prim = _check_structure(g, T, c["Ng"], 12)
    assert np.array_equal(g.accessor(prim["indices"]), c["idx"].reshape(-1).astype(np.uint32))
    assert np.array_equal(g.accessor(prim["attributes"]["POSITION"]), c["p"][0])
    assert np.array_equal(g.accessor(prim["attributes"]["NORMAL"]), c["n"][0])
    for k in range(1, T):
        t = prim["targets"][k - 1]
        assert np.array_equal(g.accessor(t["POSITION"]), (c["p"][k] - c["p"][0]).astype(np.float32)), k
        assert np.array_equal(g.accessor(t["NORMAL"]), (c["n"][k] - c["n"][0]).astype(np.float32)), k
    if T > 1:
        s = g.json["animations"][0]["samplers"][0]
        assert np.array_equal(g.accessor(s["input"]), np.array([np.float32(k / FPS) for k in range(T)]))
        want = np.zeros((T, T - 1), dtype=np.float32)
        for k in range(1, T):
            want[k, k - 1] = 1.0
        assert np.array_equal(g.accessor(s["output"]).reshape(T, T - 1), want)


def test_colour_sources(tmp_path):
    from PIL import Image
    c = _case(2)
    path = str(tmp_path / "c.glb")
    # a texture: the PNG decodes to round(texture * 255), the UVs are flipped, one material
    mesh_export.write_animated_glb(path, c["p"], c["n"], c["idx"], uvs=c["uvs"], texture=c["texture"], fps=FPS)
    g = ref.Glb(path)
    prim = _check_structure(g, 2, c["Ng"], 12)
    assert sorted(prim["attributes"]) == ["NORMAL", "POSITION", "TEXCOORD_0"] and prim["material"] == 0
    assert np.array_equal(g.accessor(prim["attributes"]["TEXCOORD_0"]), np.stack([c["uvs"][:, 0], np.float32(1) - c["uvs"][:, 1]], 1))
    assert g.json["materials"] == [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}]
    assert g.json["textures"][0]["source"] == 0 and g.json["images"][0]["mimeType"] == "image/png"
    png = g.view(g.json["images"][0]["bufferView"])
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    with Image.open(io.BytesIO(png)) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), np.round(c["texture"] * 255).astype(np.uint8))
    # UVs alone: the coordinates without a material
    mesh_export.write_animated_glb(path, c["p"], c["n"], c["idx"], uvs=c["uvs"], fps=FPS)
    g = ref.Glb(path)
    prim = _check_structure(g, 2, c["Ng"], 12)
    assert "TEXCOORD_0" in prim["attributes"] and "material" not in prim and not any(k in g.json for k in ("materials", "textures", "images"))
    # vertex colours: COLOR_0 as float VEC3 and no material texture
    mesh_export.write_animated_glb(path, c["p"], c["n"], c["idx"], colors=c["colors"], fps=FPS)
    g = ref.Glb(path)
    prim = _check_structure(g, 2, c["Ng"], 12)
    assert sorted(prim["attributes"]) == ["COLOR_0", "NORMAL", "POSITION"]
    a = g.json["accessors"][prim["attributes"]["COLOR_0"]]
    assert a["type"] == "VEC3" and a["componentType"] == 5126 and np.array_equal(g.accessor(prim["attributes"]["COLOR_0"]), c["colors"])
    assert "material" not in prim and not any(k in g.json for k in ("materials", "textures", "images", "samplers"))
    # neither
    mesh_export.write_animated_glb(path, c["p"], c["n"], c["idx"], fps=FPS)
    g = ref.Glb(path)
    prim = _check_structure(g, 2, c["Ng"], 12)
    assert sorted(prim["attributes"]) == ["NORMAL", "POSITION"] and "material" not in prim
    assert not any(k in g.json for k in ("materials", "textures", "images", "samplers"))


def test_writer_refusals(tmp_path):
    c = _case(3)
    path = str(tmp_path / "refused.glb")
    good = dict(positions=c["p"], normals=c["n"], indices=c["idx"])

    def poisoned(a, value):
        a = a.copy()
        a[1, 2, 0] = value
        return a

    bad = [dict(good, positions=poisoned(c["p"], np.nan)), dict(good, positions=poisoned(c["p"], np.inf)),
           dict(good, normals=poisoned(c["n"], np.nan)), dict(good, normals=poisoned(c["n"], -np.inf)),
           dict(good, fps=0.0), dict(good, fps=-8.0), dict(good, fps=float("nan")),
           dict(good, normals=c["n"][:2]), dict(good, normals=c["n"][:, :-1]), dict(good, positions=c["p"][0]), dict(good, positions=c["p"][..., :2]),
           dict(good, indices=c["idx"].reshape(-1)), dict(good, indices=c["idx"][:, :2]), dict(good, indices=c["idx"].astype(np.float32)),
           dict(good, uvs=c["uvs"][:-1]), dict(good, colors=c["colors"][:-1]), dict(good, uvs=c["uvs"], texture=c["texture"][..., :2]),
           dict(good, indices=np.where(c["idx"] == 0, c["Ng"], c["idx"])), dict(good, indices=c["idx"] - 1),
           dict(good, uvs=c["uvs"], colors=c["colors"]), dict(good, texture=c["texture"]), dict(good, texture=c["texture"], colors=c["colors"])]
    for kw in bad:
        kw = dict(kw)
        args = [kw.pop(k) for k in ("positions", "normals", "indices")]
        with pytest.raises(ValueError):
            mesh_export.write_animated_glb(path, *args, **kw)
        assert not os.path.exists(path), sorted(kw)
    mesh_export.write_animated_glb(path, c["p"], c["n"], c["idx"])                           # and the unpoisoned call writes it
    assert os.path.exists(path)


def test_plan_and_normals_refusals_without_a_device():
    verts, faces = ref.regular_tetrahedron()
    f = torch.from_numpy(faces)
    plan = mesh_export.NormalPlan(f, 4)
    assert plan.faces.dtype == plan.order.dtype == plan.starts.dtype == torch.int32
    assert plan.faces.tolist() == faces.reshape(-1).tolist() and plan.starts.tolist() == [0, 3, 6, 9, 12]
    assert [sorted(plan.order[3 * v:3 * v + 3].tolist()) == plan.order[3 * v:3 * v + 3].tolist() for v in range(4)] == [True] * 4
    assert all(int(plan.faces[c]) == v for v in range(4) for c in plan.order[3 * v:3 * v + 3].tolist())
    with pytest.raises(ValueError, match="2 of 6 vertices are in no face"):
        mesh_export.NormalPlan(f, 6)
    with pytest.raises(IndexError):
        mesh_export.NormalPlan(f, 3)
    with pytest.raises(IndexError):
        mesh_export.NormalPlan(f - 1, 4)
    with pytest.raises(ValueError):
        mesh_export.NormalPlan(f.float(), 4)
    with pytest.raises(ValueError):
        mesh_export.NormalPlan(f.reshape(-1), 4)
    with pytest.raises(TypeError):
        mesh_export.NormalPlan(faces, 4)
    p = torch.from_numpy(verts).float()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_export.vertex_normals(p, plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_export.vertex_normals(p[None], f)
    with pytest.raises(ValueError):
        mesh_export.vertex_normals(p[:3], plan)
    with pytest.raises(ValueError):
        mesh_export.vertex_normals(p[:, :2], plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_export.export_animated_glb("unused.glb", p[None], f)
    for bad in (dict(texture=torch.rand(4, 4, 3)), dict(texture=torch.rand(4, 4, 3), uvs=torch.rand(5, 2), faces_uvs=f, vertex_colors=torch.rand(4, 3)),
                dict(vertex_colors=torch.rand(5, 3))):
        with pytest.raises(ValueError):
            mesh_export.export_animated_glb("unused.glb", p[None], f, **bad)
    assert not os.path.exists("unused.glb")


# ---- the restatement's self-check

def test_restatement_on_a_regular_tetrahedron():
    verts, faces = ref.regular_tetrahedron()
    for order in (False, True):
        n, q = ref.normals_f64(verts[None], faces, descending=order)
        assert np.abs(n[0] - verts / np.linalg.norm(verts, axis=1, keepdims=True)).max() <= 1e-15
        assert np.abs(q - np.sqrt(3.0) / 6.0).max() <= 1e-15          # sin 60 degrees per corner, a third of each face normal survives
    # the degenerate rule: a vertex whose faces have no area gets (0, 0, 1)
    flat = np.zeros((1, 4, 3))
    n, q = ref.normals_f64(flat, faces)
    assert np.array_equal(n[0], np.tile([0.0, 0.0, 1.0], (4, 1))) and not q.any()


def test_sphere_recipe():
    """The GPU parity mesh, checked here: 514 vertices, 1 024 faces, two poles of degree 64, every vertex's q above the precondition, and
    the restatement summed in ascending and in descending corner order rounds to identical fp32 in all 6 168 components."""
    pos, faces = ref.sphere_trajectory()
    assert pos.shape == (4, 514, 3) and pos.dtype == np.float32 and faces.shape == (1024, 3)
    deg = np.bincount(faces.reshape(-1), minlength=514)
    assert deg[0] == deg[513] == 64 and (deg[65:449] == 6).all() and (deg[1:65] == 5).all() and (deg[449:513] == 5).all()   # corners per vertex
    up, q = ref.normals_f64(pos, faces)
    down, _ = ref.normals_f64(pos, faces, descending=True)
    print(f"[mesh export sphere] min q {q.min():.3f}; ascending vs descending corner order, float64: {np.abs(up - down).max():.3e}")
    assert q.min() >= ref.Q_MIN
    assert np.array_equal(up.astype(np.float32), down.astype(np.float32)) and up.size == 6168
    unit, _ = ref.normals_f64(ref.sphere()[0][None], faces)
    assert (np.einsum("vk,vk->v", unit[0], ref.sphere()[0]) > 0.97).all()                     # wound outwards


# ---- the C-ABI of csrc/mesh_export.hip, as test_mesh_vertex_gaussians_refusals holds the ingest's: made-up device addresses, every call
# differs from a valid launch in at least one operand, and never in none

BASE = 0x7F00_0010_0000
DEVICE = ("pos", "faces", "order", "starts", "nrm")
VALID = dict(T=4, Nv=514, C=3072)


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.load_library()


def _normals_call(lib, ptr=None, **scalars):
    assert ptr or scalars, "a fully valid call would launch a kernel on made-up addresses"
    p = {n: BASE + 0x100_0000 * i for i, n in enumerate(DEVICE)}
    p.update(ptr or {})
    g = dict(VALID, **scalars)
    return lib.a3d_mesh_vertex_normals_f32(None, g["T"], g["Nv"], g["C"], p["pos"], p["faces"], p["order"], p["starts"], p["nrm"])


def test_mesh_vertex_normals_refusals(lib):
    """Before any launch: T < 1, Nv < 1, C < 3, C % 3 != 0, T Nv 3 >= 2^31, a NULL pointer, a misaligned pointer."""
    for operand in DEVICE:
        assert _normals_call(lib, ptr={operand: None}) == A3D_EINVAL, f"NULL {operand}"
        assert _normals_call(lib, ptr={operand: BASE + 2}) == A3D_EINVAL, f"{operand} misaligned"
    for scalars in (dict(T=0), dict(T=-1), dict(Nv=0), dict(Nv=-514), dict(C=0), dict(C=2), dict(C=-3), dict(C=3071), dict(C=3073),
                    dict(T=2 ** 16, Nv=2 ** 14), dict(T=1, Nv=715827883), dict(T=3, Nv=238609295), dict(T=2 ** 30, Nv=2 ** 30)):
        assert _normals_call(lib, **scalars) == A3D_EINVAL, scalars
