"""The mesh branch of the ARAP loss on the GPU: ``MeshGraph.sample`` (csrc/arap.hip, mesh_sample_kernel) bit for bit against its numpy
restatement (tests/mesh_ref.py), the sampling contract from the output alone, determinism and host independence, the reference's recorded
draw through the energy kernels against the reference's own results (tests/golden/mesh_arap.npz; the bars are the project's for the
reference's ARAP golden, tests/test_arap_host.py), ``training_step`` with a ``MeshGraph``, and ``vertex_trajectory``."""
import math
import random

import numpy as np
import pytest
import torch

from animate3d_amd import arap, deform4d, stage4d
from tests import gs_ref, mesh_ref
from tests.test_arap_host import ROT_BAR, SUM_BAR
from tests.test_mesh_arap_host import GOLDEN, golden_rows, info_of

pytestmark = pytest.mark.gpu

SEEDS = (0, 12345, 2 ** 61 + 2 ** 33 + 7)            # the last: bits in the key's high word
KS = (1, 3, 4, 16)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def _graph_of(rows):
    row_start, col = mesh_ref.csr_of(rows)
    return arap.MeshGraph(torch.from_numpy(row_start).cuda(), torch.from_numpy(col).cuda()), row_start, col


def _clone(gen):
    other = torch.Generator(device="cuda")
    other.set_state(gen.get_state())
    return other


@pytest.fixture(scope="module")
def zoo():
    return _graph_of(mesh_ref.zoo_rows())


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def golden_graph(golden):
    return arap.MeshGraph.from_connected_vertices(info_of(golden_rows(golden)))


def test_sample_equals_the_restatement_bit_for_bit(zoo):
    """Nv = 1000: the last block is partial; degrees 0, 1, 2, 3, 4, 7, 16, 17, 40 in shuffled order, rows not ascending."""
    graph, row_start, col = zoo
    assert graph.Nv == 1000 and graph.max_degree == 40
    for K in KS:
        for seed in SEEDS:
            got = graph.sample(K, seed=_seed(seed))
            assert got.dtype == torch.int32 and got.shape == (1000, K) and got.is_cuda
            want = mesh_ref.sample(row_start, col, K, seed)
            wrong = int((got.cpu().numpy() != want).any(1).sum())
            assert wrong == 0, f"K {K} seed {seed}: {wrong} rows differ"


def test_sample_meets_the_contract_from_its_output_alone(zoo):
    graph, row_start, col = zoo
    grid = arap.MeshGraph.from_faces(torch.from_numpy(mesh_ref.grid_faces(40, 40)).cuda(), 1600)
    want = mesh_ref.adjacency_from_faces(mesh_ref.grid_faces(40, 40), 1600)
    grid_start, grid_col = mesh_ref.csr_of(want)
    assert np.array_equal(grid.row_start.cpu().numpy(), grid_start) and np.array_equal(grid.col.cpu().numpy(), grid_col)
    assert grid.max_degree == 6 and grid.col.is_cuda
    for g, rs, c in ((graph, row_start, col), (grid, grid_start, grid_col)):
        for K in KS:
            mesh_ref.check_invariants(rs, c, g.sample(K, seed=_seed(99)).cpu().numpy(), K)
    nn_idx, max_idx = grid.padded()                                                            # the drop-in, on the padded form
    drop_in = arap.sample_matrix_vectorized(nn_idx, 3, max_idx, seed=_seed(99))
    assert drop_in.dtype == torch.int64 and torch.equal(drop_in, grid.sample(3, seed=_seed(99)).long())


def test_sample_is_deterministic_follows_the_generator_and_does_not_synchronise(zoo):
    graph = zoo[0]
    a, b, c = graph.sample(3, seed=_seed(5)), graph.sample(3, seed=_seed(5)), graph.sample(3, seed=_seed(6))
    assert torch.equal(a, b) and not torch.equal(a, c)
    gen = torch.Generator(device="cuda").manual_seed(21)
    twin = _clone(gen)
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=twin, device="cuda")
    assert torch.equal(graph.sample(3, generator=gen), graph.sample(3, seed=seed))
    assert torch.equal(gen.get_state(), twin.get_state())                                      # one draw of [1], nothing else
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        again = graph.sample(3, seed=seed)
        drawn = graph.sample(16, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.equal(again, graph.sample(3, seed=seed)) and drawn.shape == (1000, 16)
    with pytest.raises(ValueError):
        graph.sample(3, seed=torch.tensor([5]))                                                # a CPU seed: it is read on the device
    with pytest.raises(ValueError):
        graph.sample(3, seed=_seed(5).int())


def test_reference_draw_through_the_energy_against_the_reference(golden):
    """The reference's own draw (K = 3, -1 in its degree-1 and degree-2 rows) and its edge list through ``cal_arap_error``."""
    K = int(golden["K"])
    assert int((golden["draw"] == -1).sum()) > 0
    ii, jj, nn = (torch.from_numpy(golden[k]).long().cuda() for k in ("ii", "jj", "nn"))
    assert torch.equal(arap.edges_to_dense(ii, jj, nn, 600, K).cpu(), torch.from_numpy(golden["draw"]))
    nodes = torch.from_numpy(golden["nodes"]).cuda().requires_grad_(True)
    err, R = arap.cal_arap_error(nodes, ii, jj, nn, K=K, sample_idx=torch.from_numpy(golden["sample_idx"]).cuda(), return_rotations=True)
    (grad,) = torch.autograd.grad(err, [nodes])
    errs = {"R": _rel(R, torch.from_numpy(golden["rotations"])), "loss": _rel(err, torch.from_numpy(golden["error"])),
            "grad": _rel(grad, torch.from_numpy(golden["grad"]))}
    print("[mesh arap golden on the GPU] " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["R"] <= ROT_BAR and errs["loss"] <= SUM_BAR and errs["grad"] <= SUM_BAR, errs


N_VIEW, N_FRAME, SIDE, PROGRESSIVE = 2, 4, 8, 10
LOSS = dict(lambda_rgb=100.0, lambda_mask=100.0, lambda_arap=4.0, arap_K=3, arap_sample_num=64)


def _batch(side, g):
    S = N_VIEW * N_FRAME
    views = torch.stack([gs_ref.look_at((3.5 * math.cos(a), 3.5 * math.sin(a), 0.3)) for a in (0.0, math.pi / 2)])
    return dict(c2w=views[:, None].expand(N_VIEW, N_FRAME, 4, 4).reshape(S, 4, 4).cuda().contiguous(),
                fovy=torch.full((S,), math.radians(40.0), device="cuda"), timestamps=torch.linspace(-1, 1, N_FRAME).repeat(N_VIEW).cuda(),
                rgb=torch.rand(S, side, side, 3, generator=g).cuda(), mask=(torch.rand(S, side, side, 1, generator=g) > 0.5).cuda())


def test_training_step_with_a_mesh_graph(golden, golden_graph):
    """2 views x 4 frames, 600 Gaussians on the golden's graph, a render stand-in that returns fixed tensors and draws nothing."""
    g = torch.Generator().manual_seed(4)
    xyz = torch.from_numpy(golden["nodes"][0]).cuda()
    gaussians = stage4d.Gaussians(xyz, None, None, None, None, 0)
    batch = _batch(SIDE, g)
    step = 2 * PROGRESSIVE + 5
    frames = stage4d.sampled_frames(step, N_FRAME, PROGRESSIVE, do_guidance=False)
    assert frames == [1, 2, 3]
    B = N_VIEW * len(frames)
    image, alpha = torch.rand(B, 3, SIDE, SIDE, generator=g).cuda(), torch.rand(B, 1, SIDE, SIDE, generator=g).cuda()
    moved = torch.from_numpy(golden["nodes"][[2, 3, 4, 2, 3, 4]]).cuda() + 0.01 * torch.randn(B, 600, 3, generator=g).cuda()
    leaves = []

    def render(field, gs, c2w, fovy, timestamps, height, width, bg, **kwargs):
        means = moved.clone().requires_grad_(True)
        leaves.append(means)
        return stage4d.RenderOutput(image=image.clone().requires_grad_(True), alpha=alpha.clone().requires_grad_(True), means3D=means)

    def run(graph, gen):
        return stage4d.training_step(None, gaussians, batch, loss=LOSS, global_step=step, n_view=N_VIEW, n_frame=N_FRAME,
                                     progressive_iter_per_frame=PROGRESSIVE, bg=(1.0, 1.0, 1.0), graph=graph, generator=gen,
                                     rng=random.Random(0), render=render)
    gen = torch.Generator(device="cuda").manual_seed(17)
    twin, start = _clone(gen), _clone(gen)
    out = run(golden_graph, gen)
    nn_idx = golden_graph.sample(3, generator=twin)                                            # the seed first, then sample_idx
    want = 4.0 * arap.arap_energy(xyz, moved[:len(frames)], nn_idx, sample_num=64, generator=twin)
    assert torch.equal(out["loss_arap"], want) and float(want) > 0.0
    assert torch.equal(gen.get_state(), twin.get_state())
    out["loss"].backward()
    grad = leaves[-1].grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad[:len(frames)].abs().max()) > 0.0
    assert float(grad[len(frames):].abs().max()) == 0.0                                        # ARAP reads the first len(frames) means only
    # the k-NN branch draws exactly one [1] fewer: sample_idx alone
    knn_gen = _clone(start)
    out_knn = run(arap.ArapGraph(xyz, K=3), knn_gen)
    assert "loss_arap" in out_knn and not torch.equal(knn_gen.get_state(), gen.get_state())
    torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=knn_gen, device="cuda")
    assert torch.equal(knn_gen.get_state(), gen.get_state())
    with pytest.raises(ValueError):                                                            # a mesh of another size
        run(arap.MeshGraph.from_faces(torch.from_numpy(mesh_ref.grid_faces(7, 5)).cuda(), 35), _clone(start))


@pytest.fixture(scope="module")
def scene(golden):
    g = torch.Generator().manual_seed(12)
    N = 600
    gaussians = stage4d.Gaussians(xyz=(torch.from_numpy(golden["nodes"][0]) * 1.5).cuda().contiguous(),
                                  scaling=(torch.rand(N, 3, generator=g) * 2.0 - 4.2).cuda(), rotation=torch.randn(N, 4, generator=g).cuda(),
                                  opacity=torch.sigmoid(torch.randn(N, 1, generator=g) * 1.5).cuda(),
                                  shs=(torch.randn(N, 16, 3, generator=g) * 0.3).cuda(), sh_degree=3)
    field = deform4d.HexPlaneDeformation(use_global_trans=True)                                # mesh_animation_frame_16.yaml: use_global_trans
    with torch.no_grad():                                       # the reference's zero last layers give zero gradient to everything before them
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return dict(gaussians=gaussians, field=field.cuda(), batch=_batch(32, g), bg=torch.ones(3, device="cuda"))


def test_vertex_trajectory_is_the_renders_means(scene):
    gs, field, batch, bg = scene["gaussians"], scene["field"], scene["batch"], scene["bg"]
    ts = batch["timestamps"][:N_FRAME]
    traj = stage4d.vertex_trajectory(field, gs, ts)
    out = stage4d.render_batch(field, gs, batch["c2w"][:N_FRAME], batch["fovy"][:N_FRAME], ts, 32, 32, bg, do_guidance=False,
                               generator=torch.Generator(device="cuda").manual_seed(1))
    assert traj.shape == (N_FRAME, 600, 3) and not traj.requires_grad and out["means3D"].requires_grad
    assert torch.equal(traj, out["means3D"].detach()) and torch.equal(traj[0], gs.xyz) and not torch.equal(traj[1], gs.xyz)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.vertex_trajectory(field, gs, ts.cpu())


def test_mesh_animation_step_end_to_end(scene, golden_graph):
    """The released mesh-animation config's step (``sample_strategy: light``, ``use_global_trans``, ``lambda_arap: 4.0``, ``arap_K: 3``)
    through the real renderer: every term finite, and the ARAP term's gradient reaches the field."""
    gs, field, batch, bg = scene["gaussians"], scene["field"], scene["batch"], scene["bg"]
    for p in field.parameters():
        p.grad = None
    out = stage4d.training_step(field, gs, batch, loss=dict(LOSS, arap_sample_num=512), global_step=2 * PROGRESSIVE + 5, n_view=N_VIEW,
                                n_frame=N_FRAME, progressive_iter_per_frame=PROGRESSIVE, bg=bg, graph=golden_graph, sample_strategy="light",
                                generator=torch.Generator(device="cuda").manual_seed(9), rng=random.Random(3))
    assert set(out) == {"loss", "loss_rgb", "loss_mask", "loss_arap"} and all(bool(torch.isfinite(v)) for v in out.values())
    assert float(out["loss_arap"]) > 0.0
    out["loss"].backward()
    grads = [p.grad for n, p in field.named_parameters() if n.startswith(("delta_xyz", "global")) and p.grad is not None]
    assert grads and all(bool(torch.isfinite(x).all()) for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
