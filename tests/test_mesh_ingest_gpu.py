"""The mesh ingest on the GPU (animate3d_amd/mesh.py, csrc/mesh_ingest.hip) against its float64 restatement on the same fp32 inputs and
against the reference's own results (tests/golden/mesh_ingest.npz), with the derived bars of tests/mesh_ingest_ref.py: no quantity here
has a discontinuity, so every element is compared.  Then determinism, independence of the block a vertex lands in, ``read_gaussian_ply``
against the reference's ``load_ply``, ``to_mesh_frame`` and one training step on the ingested mesh.

logf: the bar of ``scaling`` allows 4 ulp of the result for the device's ``logf``.  Measured on these inputs against float64 ``log`` of
the kernel's own fp32 argument (printed by the golden test as "logf"): 2.07 ulp at worst on an MI355X
(profiles/pytest_gpu_mesh_ingest.log), so the 4 ulp stand."""
import math
import random

import numpy as np
import pytest
import torch

from animate3d_amd import arap, deform4d, mesh, stage4d
from tests import gs_ref
from tests import mesh_ingest_ref as ref
from tests.test_mesh_ingest_host import FRAME, GOLDEN, golden_rows, grid_sample_error, mesh_of

pytestmark = pytest.mark.gpu

QUANTITIES = ("edge_length", "mean_edge", "xyz", "scaling", "colors", "shs")


def _cuda(arrays):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}


def _outputs(mg):
    g = mg.gaussians
    out = dict(edge_length=mg.edge_length, mean_edge=mg.mean_edge, xyz=g.xyz, scaling=g.scaling, colors=mg.colors, shs=g.shs[:, 0])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(tag, got, want, bar, quantities=QUANTITIES):
    worst = {}
    for q in quantities:
        ratio, exact = ref.worst(got[q], want[q], bar[q])
        worst[q] = ratio
        assert exact, f"{tag}: {q} differs where the bar is zero"
    print(f"[mesh ingest {tag}] worst error / bar: " + " ".join(f"{q} {r:.3f}" for q, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), (tag, worst)


def _check_gaussians(mg, Nv, R, opacity=1 - 1e-5):
    g = mg.gaussians
    assert g.sh_degree == 0 and g.shs.shape == (Nv, 1, 3) and g.opacity.shape == (Nv, 1) and g.rotation.shape == (Nv, 4)
    assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (g.xyz, g.scaling, g.rotation, g.opacity, g.shs))
    assert torch.equal(g.opacity, torch.full((Nv, 1), opacity).cuda())
    q = mesh.quaternion_of(R)
    assert torch.equal(g.rotation.cpu(), torch.tensor(q, dtype=torch.float32).expand(Nv, 4)) and float(g.rotation[0, 0]) >= 0


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def golden_case(golden):
    """The golden mesh on the device, its ingest, the float64 restatement and e32: computed once, read by several tests."""
    m = mesh_of(golden)
    e32, _ = grid_sample_error(m["texture"], m["uvs"], m["faces_uvs"])
    want = ref.restate(m["verts"], m["faces"], texture=m["texture"], uvs=m["uvs"], faces_uvs=m["faces_uvs"], shrink=ref.SHRINK, **FRAME)
    dev = _cuda(m)
    mg = mesh.gaussians_from_mesh(dev.pop("verts"), dev.pop("faces"), shrink=ref.SHRINK, **dev, **FRAME)
    torch.cuda.synchronize()
    return dict(m=m, e32=e32, want=want, mg=mg)


def test_tetrahedron_every_colour_source():
    """Four vertices, every one in three faces.  The UVs: exactly 0 and 1, and outside [0, 1] on both sides (border padding)."""
    verts, faces = ref.tetrahedron()
    rng = np.random.default_rng(1)
    vc, cc = rng.random((4, 3)).astype(np.float32), rng.random((4, 3, 3)).astype(np.float32)
    texture = rng.random((4, 7, 3)).astype(np.float32)
    uvs = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [-0.25, 0.4], [1.5, 0.6], [0.3, -2.0], [0.7, 1.001], [0.37, 0.81]], dtype=np.float32)
    faces_uvs = np.array([[0, 4, 1], [2, 5, 8], [6, 3, 7], [8, 1, 0]], dtype=np.int64)
    e32, _ = grid_sample_error(texture, uvs, faces_uvs)
    frame = dict(rot_x_degree=30.0, rot_z_degree=-70.0, scale_factor=1.3)
    sources = {"vertex": dict(vertex_colors=vc), "corner": dict(corner_colors=cc), "texture": dict(texture=texture, uvs=uvs, faces_uvs=faces_uvs)}
    for tag, source in sources.items():
        want = ref.restate(verts, faces, shrink=1.1, **source, **frame)
        mg = mesh.gaussians_from_mesh(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).int().cuda(), **_cuda(source), **frame)
        e = e32 if tag == "texture" else None
        print(f"[mesh ingest tetrahedron {tag}] e32 {0.0 if e is None else e:.3e}")
        _compare(f"tetrahedron {tag}", _outputs(mg), want, ref.bars(want, verts, scale_factor=1.3, textured_e32=e))
        _check_gaussians(mg, 4, want["R"])
        assert mg.graph.Nv == 4 and mg.graph.col.tolist() == want["col"].tolist()
        if tag == "vertex":
            assert np.array_equal(mg.colors.cpu().numpy(), vc)                                 # passed through unchanged


def test_golden_mesh_against_the_restatement_and_the_reference(golden, golden_case):
    """600 + 71 vertices (three blocks, the last partial), valence 2 to 70, the duplicated face, the UV seam, UVs on and outside the
    border; rot_x = rot_z = 90, scale_factor = 0.76."""
    m, want, mg, e32 = golden_case["m"], golden_case["want"], golden_case["mg"], golden_case["e32"]
    got = _outputs(mg)
    bar = ref.bars(want, m["verts"], scale_factor=ref.SCALE, textured_e32=e32)
    err = np.abs(got["colors"] - want["colors"]).max()
    print(f"[mesh ingest golden] e32 {e32:.3e} colour error {err:.3e} colour bar {bar['colors'].min():.3e} .. {bar['colors'].max():.3e}")
    _compare("golden mesh vs float64", got, want, bar)
    _check_gaussians(mg, 671, want["R"], ref.OPACITY)
    arg = (got["mean_edge"].astype(np.float64) / ref.SHRINK * ref.SCALE).astype(np.float32).astype(np.float64)
    ulps = np.abs(got["scaling"] - np.log(arg)) / ref.ulp32(np.log(arg))
    print(f"[mesh ingest golden] logf: {ulps.max():.3f} ulp at worst against float64 log of the kernel's own argument")
    assert ulps.max() <= 4.0
    # the graph: from_faces' rows, the reference's as sets
    rows = golden_rows(golden)
    start, col = mg.graph.row_start.cpu().numpy(), mg.graph.col.cpu().numpy()
    assert np.array_equal(start, want["row_start"]) and np.array_equal(col, want["col"])
    assert all(set(col[start[v]:start[v + 1]].tolist()) == set(rows[v]) for v in range(671)) and mg.graph.max_degree == ref.FAN
    # the reference's own numbers, at the positions of its rows
    position = {(v, u): want["row_start"][v] + i for v, row in enumerate(want["rows"]) for i, u in enumerate(row)}
    at = np.array([position[(v, u)] for v, row in enumerate(rows) for u in row])
    bar = ref.bars(want, m["verts"], scale_factor=ref.SCALE, textured_e32=e32, golden=True)
    reference = dict(edge_length=golden["distance"], mean_edge=golden["mean_edge"], xyz=golden["loaded_xyz"], scaling=golden["loaded_scaling"],
                     colors=golden["colors"], shs=golden["loaded_features_dc"][:, 0])
    _compare("golden mesh vs the reference", dict(got, edge_length=got["edge_length"][at]), reference, dict(bar, edge_length=bar["edge_length"][at]))
    R = ref.rotation_matrices(mg.gaussians.rotation.cpu().numpy())
    assert np.abs(R - ref.rotation_matrices(golden["loaded_rotation"])).max() <= 8 * ref.U    # scipy's sign is not canonical: as matrices


def test_flat_grid_has_minus_infinity_on_its_axis():
    """Every neighbour shares z with its vertex: ``mean_edge[:, 2]`` is exactly 0 and the log-scale exactly -inf, as the reference's
    ``np.log(0)``; every other element is finite and within its bar.  The spacings are powers of two, so the positions and the edge
    lengths are exact in fp32."""
    verts, faces = ref.flat_grid()
    vc = np.linspace(0, 1, 27, dtype=np.float32).reshape(9, 3)
    want = ref.restate(verts, faces, vertex_colors=vc, shrink=1.1)
    mg = mesh.gaussians_from_mesh(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), vertex_colors=torch.from_numpy(vc).cuda())
    got = _outputs(mg)
    assert np.isneginf(want["scaling"][:, 2]).all() and np.isfinite(want["scaling"][:, :2]).all()
    assert np.array_equal(np.isneginf(got["scaling"]), np.isneginf(want["scaling"])) and not np.isnan(got["scaling"]).any()
    assert np.array_equal(got["mean_edge"][:, 2], np.zeros(9, dtype=np.float32))
    assert np.array_equal(got["xyz"], verts) and np.array_equal(got["edge_length"], want["edge_length"].astype(np.float32))   # exact in fp32
    _compare("flat grid", got, want, ref.bars(want, verts, scale_factor=1.0))


def test_two_calls_are_bitwise_equal(golden_case):
    m = golden_case["m"]
    dev = _cuda(m)
    again = mesh.gaussians_from_mesh(dev.pop("verts"), dev.pop("faces"), shrink=ref.SHRINK, **dev, **FRAME)
    first, second = _outputs(golden_case["mg"]), _outputs(again)
    for q in QUANTITIES:
        assert np.array_equal(first[q], second[q], equal_nan=True), q
    assert torch.equal(again.gaussians.rotation, golden_case["mg"].gaussians.rotation)


def test_a_vertex_does_not_depend_on_its_block(golden_case):
    """300 unrelated vertices and their faces, appended (the vertices keep their blocks) and prepended (vertex v becomes v + 300: another
    block, another lane): every output of the original vertices is bitwise what it was."""
    m, first = golden_case["m"], _outputs(golden_case["mg"])
    extra_verts, extra_faces = 5.0 + ref.golden_mesh()["verts"][:300], np.stack([np.arange(300), (np.arange(300) + 1) % 300, (np.arange(300) + 7) % 300], 1)
    n_uv = len(m["uvs"])
    extra_uv = np.full((300, 3), n_uv - 1, dtype=np.int64)
    E = len(first["edge_length"])
    for tag, shift in (("appended", 0), ("prepended", 300)):
        other = 671 if shift == 0 else 0
        parts = [m["verts"], extra_verts] if shift == 0 else [extra_verts, m["verts"]]
        face_parts = [m["faces"] + shift, extra_faces + other]
        dev = _cuda(dict(verts=np.concatenate(parts), faces=np.concatenate(face_parts), texture=m["texture"], uvs=m["uvs"],
                         faces_uvs=np.concatenate([m["faces_uvs"], extra_uv])))
        mg = mesh.gaussians_from_mesh(dev.pop("verts"), dev.pop("faces"), shrink=ref.SHRINK, **dev, **FRAME)
        got = _outputs(mg)
        start = mg.graph.row_start.cpu().numpy()
        e0 = int(start[shift])
        assert int(start[shift + 671]) - e0 == E, tag
        for q in QUANTITIES:
            mine = got[q][e0:e0 + E] if q == "edge_length" else got[q][shift:shift + 671]
            assert np.array_equal(mine, first[q]), (tag, q)


def test_read_gaussian_ply_against_load_ply(golden, golden_case, tmp_path):
    """100 Gaussians with random orientations and ``max_sh_degree = 1`` through the reference's ``load_ply`` (float64 on the host, stored
    as float32), and the mesh's own PLY.  xyz: the ingest's bar; scaling: ``s + log(scale_factor)`` rounded once against
    ``log(exp(s) scale_factor)`` in float64, 2 u relative; rotations as matrices (scipy's quaternion sign is not canonical), 8 u;
    opacity: sigmoid in fp32, 4 u; the SH coefficients are copied."""
    names, table = golden["ply2_names"].tolist(), golden["ply2"]
    path = str(tmp_path / "random.ply")
    ref.write_ply(path, names, table)
    g = mesh.read_gaussian_ply(path, max_sh_degree=1, **FRAME)
    assert g.sh_degree == 1 and g.shs.shape == (100, 4, 3) and g.opacity.shape == (100, 1) and all(t.is_cuda for t in g[:5])
    xyz_in = table[:, :3].astype(np.float64)
    assert (np.abs(g.xyz.cpu().numpy() - golden["loaded2_xyz"]) <= (8 * ref.U * ref.SCALE) * np.abs(xyz_in).sum(1, keepdims=True)
            + ref.U * np.abs(golden["loaded2_xyz"])).all()
    assert (np.abs(g.scaling.cpu().numpy() - golden["loaded2_scaling"]) <= 2 * ref.U * np.abs(golden["loaded2_scaling"])).all()
    R = ref.rotation_matrices(g.rotation.cpu().numpy())
    assert np.abs(R - ref.rotation_matrices(golden["loaded2_rotation"])).max() <= 8 * ref.U
    assert np.abs(np.linalg.norm(g.rotation.cpu().numpy().astype(np.float64), axis=1) - 1).max() <= 4 * ref.U
    shs = np.concatenate([golden["loaded2_features_dc"], golden["loaded2_features_rest"]], 1)
    assert np.array_equal(g.shs.cpu().numpy(), shs)
    sig = 1 / (1 + np.exp(-golden["loaded2_opacity"].astype(np.float64)))
    assert np.abs(g.opacity.cpu().numpy() - sig).max() <= 4 * ref.U
    # the mesh's own file: write_gaussian_ply -> read_gaussian_ply is gaussians_from_mesh
    m, want, mg = golden_case["m"], golden_case["want"], golden_case["mg"]
    path = str(tmp_path / "mesh.ply")
    mesh.write_gaussian_ply(path, m["verts"], mg.colors, mg.mean_edge, shrink=ref.SHRINK, opacity=ref.OPACITY)
    back = mesh.read_gaussian_ply(path, max_sh_degree=0, **FRAME)
    assert torch.equal(back.xyz, mg.gaussians.xyz) and torch.equal(back.shs, mg.gaussians.shs) and back.shs.shape == (671, 1, 3)
    bar = ref.bars(want, m["verts"], scale_factor=ref.SCALE)["scaling"] + 2 * ref.U * np.abs(want["scaling"])
    assert (np.abs(back.scaling.cpu().numpy() - want["scaling"]) <= bar).all()
    assert (back.opacity.cpu() - ref.OPACITY).abs().max() <= 4 * ref.U
    assert np.abs(ref.rotation_matrices(back.rotation.cpu().numpy()) - want["R"][None]).max() <= 8 * ref.U


def test_trajectory_of_an_identity_field_is_the_mesh(golden_case):
    """A freshly initialised field deforms nothing (its last layers are zero): ``vertex_trajectory`` returns ``xyz`` in every frame, and
    ``to_mesh_frame`` takes it back to the vertices.  The bar: the ingest's 8 u on ``xyz`` plus 6 u for the inverse's own fp32 arithmetic
    (R rounded to fp32, a division, three products, two additions), each at most sqrt(3) (|x| + |y| + |z|) through a rotation."""
    m, mg = golden_case["m"], golden_case["mg"]
    field = deform4d.HexPlaneDeformation().cuda()
    traj = stage4d.vertex_trajectory(field, mg.gaussians, torch.linspace(-1, 1, 3).cuda())
    assert traj.shape == (3, 671, 3) and all(torch.equal(traj[t], mg.gaussians.xyz) for t in range(3))
    back = mesh.to_mesh_frame(traj, **FRAME).cpu().numpy()
    bar = math.sqrt(3.0) * 14 * ref.U * np.abs(m["verts"].astype(np.float64)).sum(1, keepdims=True)
    err = np.abs(back - m["verts"][None].astype(np.float64))
    print(f"[mesh ingest to_mesh_frame] worst error / bar {float((err / bar[None]).max()):.3f}")
    assert (err <= bar[None]).all()


N_VIEW, N_FRAME, SIDE, PROGRESSIVE = 2, 4, 32, 10
LOSS = dict(lambda_rgb=100.0, lambda_mask=100.0, lambda_arap=4.0, arap_K=3, arap_sample_num=512)


def test_training_step_on_the_ingested_mesh(golden_case):
    """The released mesh-animation config's step (``sample_strategy: light``, ``use_global_trans``, ``lambda_arap``, ``arap_K: 3``) on the
    Gaussians and the graph of one ``gaussians_from_mesh`` call, through the real renderer."""
    mg = golden_case["mg"]
    g = torch.Generator().manual_seed(12)
    field = deform4d.HexPlaneDeformation(use_global_trans=True)
    with torch.no_grad():                                       # the reference's zero last layers give zero gradient to everything before them
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    field = field.cuda()
    S = N_VIEW * N_FRAME
    views = torch.stack([gs_ref.look_at((3.5 * math.cos(a), 3.5 * math.sin(a), 0.3)) for a in (0.0, math.pi / 2)])
    batch = dict(c2w=views[:, None].expand(N_VIEW, N_FRAME, 4, 4).reshape(S, 4, 4).cuda().contiguous(),
                 fovy=torch.full((S,), math.radians(40.0), device="cuda"), timestamps=torch.linspace(-1, 1, N_FRAME).repeat(N_VIEW).cuda(),
                 rgb=torch.rand(S, SIDE, SIDE, 3, generator=g).cuda(), mask=(torch.rand(S, SIDE, SIDE, 1, generator=g) > 0.5).cuda())
    assert isinstance(mg.graph, arap.MeshGraph) and bool(torch.isfinite(mg.gaussians.scaling).all())
    out = stage4d.training_step(field, mg.gaussians, batch, loss=LOSS, global_step=2 * PROGRESSIVE + 5, n_view=N_VIEW, n_frame=N_FRAME,
                                progressive_iter_per_frame=PROGRESSIVE, bg=torch.ones(3, device="cuda"), graph=mg.graph,
                                sample_strategy="light", generator=torch.Generator(device="cuda").manual_seed(9), rng=random.Random(3))
    assert set(out) == {"loss", "loss_rgb", "loss_mask", "loss_arap"} and all(bool(torch.isfinite(v)) for v in out.values())
    assert float(out["loss_arap"]) > 0.0
    out["loss"].backward()
    grads = {n: p.grad for n, p in field.named_parameters()}
    assert all(x is not None and bool(torch.isfinite(x).all()) for x in grads.values()), [n for n, x in grads.items() if x is None]
    assert any(float(x.abs().max()) > 0 for n, x in grads.items() if n.startswith(("delta_xyz", "global")))
