"""The mesh export on the GPU (animate3d_amd/mesh_export.py, csrc/mesh_export.hip): the vertex normals against the float64 restatement
of tests/mesh_export_ref.py on the same fp32 positions, the degenerate rule, bitwise reproducibility, the absence of a host
synchronisation, and one export of a deformed golden ingest mesh read back from the file.

The parity bar is 2^-24 absolute on every component of every vertex, nothing excluded, under the precondition the tests assert on the
restatement itself: every vertex has q(v) >= 1/64 (tests/mesh_export_ref.py derives the bar from it).  A mesh that misses the
precondition is changed, never the bar."""
import functools
import math

import numpy as np
import pytest
import torch

from animate3d_amd import deform4d, mesh, mesh_export, stage4d
from tests import mesh_export_ref as ref
from tests.test_mesh_ingest_host import FRAME, GOLDEN, mesh_of

pytestmark = pytest.mark.gpu


def _tetrahedron():
    verts, faces = ref.regular_tetrahedron()
    return verts[None].astype(np.float32), faces


def _two_components():
    return ref.with_tetrahedron_first(*ref.sphere_trajectory())


MESHES = {"tetrahedron": _tetrahedron, "sphere": ref.sphere_trajectory, "strip": ref.strip, "two components": _two_components}


@functools.lru_cache(maxsize=None)
def case(name):
    """(positions [T, Nv, 3] float32, faces [F, 3] int64, restated normals float64, q): computed once, read by several tests."""
    pos, faces = MESHES[name]()
    want, q = ref.normals_f64(pos, faces)
    for a in (pos, faces, want, q):
        a.setflags(write=False)
    return pos, faces, want, q


def _normals(pos, faces, dtype=torch.int64):
    out = mesh_export.vertex_normals(torch.tensor(pos).cuda(), torch.tensor(faces).to(dtype).cuda())      # copies: the shared arrays are read-only
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == pos.shape
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("name", list(MESHES))
def test_normals_against_the_restatement(name, dtype):
    pos, faces, want, q = case(name)
    assert q.min() >= ref.Q_MIN, (name, q.min())                                              # the precondition of the bar
    got = _normals(pos, faces, dtype)
    err = np.abs(got.astype(np.float64) - want)
    print(f"[mesh export normals {name} {str(dtype)[6:]}] {pos.shape[0]} x {pos.shape[1]} vertices, min q {q.min():.3f}, "
          f"worst error / bar {err.max() / ref.U:.3f}")
    assert (err <= ref.U).all(), (name, err.max() / ref.U)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=2) - 1).max() <= 2.0 ** -23
    if pos.shape[0] == 1:                                                                     # [Nv, 3] is one frame
        assert np.array_equal(_normals(pos[0], faces, dtype), got[0])


def test_degenerate_faces():
    """A new vertex at the position of vertex 5 and two faces (it, 5, 9): every face at the new vertex has no area, so it gets exactly
    (0, 0, 1); vertices 5 and 9 gain corners that add exactly 0 (an edge of length 0; two equal edges, which a contracted product would
    not cancel), and a face with a repeated corner does the same at 100 and 101: every other normal is bitwise what it was."""
    pos, faces, want, _ = case("sphere")
    Nv = pos.shape[1]
    more_pos = np.concatenate([pos, pos[:, 5:6]], 1)
    more_faces = np.concatenate([faces, [[Nv, 5, 9], [Nv, 9, 5], [100, 101, 100]]])
    restated, _ = ref.normals_f64(more_pos, more_faces)
    assert np.array_equal(restated[:, :Nv], want) and np.array_equal(restated[:, Nv], np.tile([0.0, 0.0, 1.0], (pos.shape[0], 1)))
    plain, got = _normals(pos, faces), _normals(more_pos, more_faces)
    assert np.array_equal(got[:, Nv], np.tile(np.float32([0, 0, 1]), (pos.shape[0], 1)))
    assert np.array_equal(got[:, :Nv], plain)
    collapsed = _normals(np.zeros((2, 4, 3), dtype=np.float32), ref.regular_tetrahedron()[1])  # a mesh of no extent at all
    assert np.array_equal(collapsed, np.tile(np.float32([0, 0, 1]), (2, 4, 1)))


def test_reproducibility():
    """Two calls; T frames in one call against T calls of one frame; and the sphere's rows when the tetrahedron comes first (vertex v
    becomes v + 4: another lane, for 4 of every 256 another block, other frames' offsets): all bitwise equal."""
    pos, faces, _, _ = case("sphere")
    first = _normals(pos, faces)
    assert np.array_equal(first, _normals(pos, faces))
    dev_faces = torch.tensor(faces).cuda()
    plan = mesh_export.NormalPlan(dev_faces, pos.shape[1])
    dev_pos = torch.tensor(pos).cuda()
    frames = torch.stack([mesh_export.vertex_normals(dev_pos[t:t + 1], plan)[0] for t in range(pos.shape[0])])
    assert np.array_equal(frames.cpu().numpy(), first)
    both, both_faces, _, _ = case("two components")
    assert np.array_equal(_normals(both, both_faces)[:, 4:], first)


def test_no_host_synchronisation_with_a_plan():
    pos, faces, _, _ = case("sphere")
    plan = mesh_export.NormalPlan(torch.tensor(faces).cuda(), pos.shape[1])
    dev_pos = torch.tensor(pos).cuda()
    first = mesh_export.vertex_normals(dev_pos, plan)                  # also loads the library and the kernel outside the guarded region
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        second = mesh_export.vertex_normals(dev_pos, plan)
        single = mesh_export.vertex_normals(dev_pos[0], plan)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(single, first[0])


def test_refusals_on_the_device():
    pos, faces, _, _ = case("tetrahedron")
    p, f = torch.tensor(pos).cuda(), torch.tensor(faces).cuda()
    plan = mesh_export.NormalPlan(f, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_export.vertex_normals(p.double(), plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_export.vertex_normals(p.cpu(), plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_export.vertex_normals(p, mesh_export.NormalPlan(f.cpu(), 4))
    with pytest.raises(ValueError, match="no face"):
        mesh_export.vertex_normals(torch.zeros(1, 5, 3, device="cuda"), f)


def test_export_of_a_deformed_golden_mesh(tmp_path):
    """The golden ingest mesh under the released frame, a field whose last layers are small seeded values (so frames differ),
    ``vertex_trajectory``, ``export_animated_glb``, and the file read back."""
    from PIL import Image
    import io
    m = mesh_of(dict(np.load(GOLDEN)))
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in m.items()}
    mg = mesh.gaussians_from_mesh(dev["verts"], dev["faces"], texture=dev["texture"], uvs=dev["uvs"], faces_uvs=dev["faces_uvs"], **FRAME)
    g = torch.Generator().manual_seed(12)
    field = deform4d.HexPlaneDeformation()
    with torch.no_grad():
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    T, Nv = 4, 671
    traj = stage4d.vertex_trajectory(field.cuda(), mg.gaussians, torch.linspace(-1, 1, T).cuda())
    assert traj.shape == (T, Nv, 3) and not torch.equal(traj[1], traj[0]) and not torch.equal(traj[3], traj[1])
    path = str(tmp_path / "golden.glb")
    arrays = mesh_export.export_animated_glb(path, traj, dev["faces"], texture=dev["texture"], uvs=dev["uvs"], faces_uvs=dev["faces_uvs"],
                                             fps=8.0, **FRAME)
    sv, su, idx = arrays["split_vertex"], arrays["split_uv"], arrays["indices"]
    Ng = len(sv)
    assert Ng == Nv + 1 and np.array_equal(sv[idx], m["faces"]) and np.array_equal(su[idx], m["faces_uvs"])   # the seam vertex, twice
    assert arrays["positions"].shape == arrays["normals"].shape == (T, Ng, 3) and arrays["positions"].dtype == np.float32
    # the positions: R^T (p / s) in float64 on the fp32 trajectory, with the 6 u of to_mesh_frame's own fp32 arithmetic
    R = mesh.frame_rotation(FRAME["rot_x_degree"], FRAME["rot_z_degree"])
    exact = ((traj.cpu().numpy().astype(np.float64) / FRAME["scale_factor"]) @ R)[:, sv]
    bar = math.sqrt(3.0) * 6 * ref.U * np.abs(exact).sum(2, keepdims=True)
    err = np.abs(arrays["positions"] - exact)
    print(f"[mesh export golden] {T} frames, {Ng} glTF vertices, positions: worst error / bar {float((err / bar).max()):.3f}")
    assert (err <= bar).all()
    assert np.abs(np.linalg.norm(arrays["normals"].astype(np.float64), axis=2) - 1).max() <= 2.0 ** -23
    # the file
    glb = ref.Glb(path)
    prim = glb.json["meshes"][0]["primitives"][0]
    assert glb.raw["length"] == glb.raw["size"] and len(prim["targets"]) == T - 1
    assert np.array_equal(glb.accessor(prim["indices"]).reshape(-1, 3), idx.astype(np.uint32))
    assert np.array_equal(sv[glb.accessor(prim["indices"]).reshape(-1, 3).astype(np.int64)], m["faces"])
    assert np.array_equal(glb.accessor(prim["attributes"]["POSITION"]), arrays["positions"][0])
    assert np.array_equal(glb.accessor(prim["attributes"]["NORMAL"]), arrays["normals"][0])
    for k in range(1, T):
        assert np.array_equal(glb.accessor(prim["targets"][k - 1]["POSITION"]), (arrays["positions"][k] - arrays["positions"][0]).astype(np.float32))
        assert np.array_equal(glb.accessor(prim["targets"][k - 1]["NORMAL"]), (arrays["normals"][k] - arrays["normals"][0]).astype(np.float32))
        assert np.abs(glb.accessor(prim["targets"][k - 1]["POSITION"])).max() > 0
    uv = m["uvs"][su]
    assert np.array_equal(glb.accessor(prim["attributes"]["TEXCOORD_0"]), np.stack([uv[:, 0], np.float32(1) - uv[:, 1]], 1))
    sampler = glb.json["animations"][0]["samplers"][0]
    assert np.array_equal(glb.accessor(sampler["input"]), np.arange(T, dtype=np.float32) / np.float32(8.0))
    with Image.open(io.BytesIO(glb.view(glb.json["images"][0]["bufferView"]))) as im:
        assert np.array_equal(np.asarray(im), np.round(m["texture"] * 255).astype(np.uint8))
    assert np.array_equal(arrays["texture"], m["texture"])
    # the normals in the file are the kernel's on the exported positions
    own = mesh.to_mesh_frame(traj, **FRAME)
    assert np.array_equal(mesh_export.vertex_normals(own, dev["faces"]).cpu().numpy()[:, sv], arrays["normals"])
    # vertex colours through the same call: ObjMesh.colors' other kind
    colours = mesh_export.export_animated_glb(path, traj, dev["faces"], vertex_colors=mg.colors, **FRAME)
    glb = ref.Glb(path)
    prim = glb.json["meshes"][0]["primitives"][0]
    assert len(colours["split_vertex"]) == Nv and np.array_equal(glb.accessor(prim["attributes"]["COLOR_0"]), mg.colors.cpu().numpy())
    assert "materials" not in glb.json and "split_uv" not in colours
