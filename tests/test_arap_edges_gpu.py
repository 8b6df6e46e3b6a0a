"""The ARAP kernels (csrc/arap.hip) at their seams, under the acceptance rules of tests/test_arap_gpu.py unchanged: ``nn_idx`` equal to
the float64 oracle's and the distances within 8 * 2^-24 (``_check_graph``); per energy tensor the relative L2 against the float64
restatement at most max(4 e32, 16 * 2^-24) (``check_against_float64``).  That file's scenes are two large random clouds at K = 1, 3, 10,
16 and two random energy scenes at K = 3 and 8; the clouds and scenes here (arap_ref.EDGE_SCENES and the graph makers beside it, whose
features tests/test_arap_host.py counts on the CPU) are the smallest that have

* every list length 1 ... 16, the rounded-up ones included, and N at the edges of a block of 256 queries and a tile of 1024 candidates;
* exact ties: bitwise twins on both sides of a tile boundary, and a lattice whose 6- and 12-fold tie shells the K-th column cuts
  through, with distances exact in fp32 (so they are compared for equality) and some exactly at ``radius ** 2`` (the cut is strict);
* each axis of the unchanged rule alone, an exact translation, samples without any edge, exactly diagonal covariances in every column
  order, rank-1 covariances (K = 1), near-rigid motion (where only an fp64 interior meets the 16 * 2^-24 floor), a vertex with hundreds
  of inverse-list entries;
* F S at the edges of the forward's blocks of 128 and the reduction's stride of 256, Nv at the backward's block of 256, F = 1, S = 1, Nv = 2;
* the host contract of arap.py's docstring: out-of-range indices are absent edges / empty samples, nothing synchronises with the host,
  forward and backward capture into a graph.

No comparison leaves an element out.  Where R is not unique (K = 1) it is held to the properties that define it instead."""
import functools

import pytest
import torch

from animate3d_amd import arap
from tests import arap_ref
from tests.test_arap_gpu import FLOOR, _check_graph, _rel, _run_hip, check_against_float64

pytestmark = pytest.mark.gpu

EYE = torch.eye(3)
ENERGY_SCENES = sorted(set(arap_ref.EDGE_SCENES) - set(arap_ref.RANK_ONE) - {"near_rigid"})


# ---- the graph

def _radius(N):
    return round(1.2 * N ** (-1.0 / 3.0), 3)          # about the 8th neighbour's distance: some columns are cut, some kept


@functools.lru_cache(maxsize=None)
def _cloud(N, K=16, duplicates=6):
    """One cloud per size, searched once for K + 2 neighbours and sliced for every smaller K (the near-tie guard covers them all)."""
    return arap_ref.make_points(N, K, 1000 + N, radius=_radius(N), duplicates=duplicates)


@pytest.mark.parametrize("K", range(1, 17))
def test_knn_every_list_length(K):
    """N = 1025: two tiles, five blocks, a ragged last block; the planted duplicates stay in."""
    pts, rounds, idx, dist = _cloud(1025)
    assert int((dist[:, 0] == 0).sum()) == 11
    _check_graph(pts, idx, dist, _radius(1025), f"N 1025, {rounds} rounds", Ks=(K,))


@pytest.mark.parametrize("N", [255, 256, 257, 1023, 1024, 1025, 2049])
def test_knn_block_and_tile_seams(N):
    pts, rounds, idx, dist = _cloud(N)
    _check_graph(pts, idx, dist, _radius(N), f"N {N}, {rounds} rounds", Ks=(1, 3, 16))


@pytest.mark.parametrize("K,duplicates", [(1, 0), (5, 2), (16, 2)])
def test_knn_of_everybody_else(K, duplicates):
    """N = K + 1: every other point is a neighbour, in (distance, index) order."""
    pts, rounds, idx, dist = _cloud(K + 1, K, duplicates)
    assert idx.shape[1] == K
    _check_graph(pts, idx, dist, _radius(K + 1), f"N {K + 1}, {rounds} rounds", Ks=(K,))


def test_knn_twins_across_the_tile_boundary():
    """Points 1023 and 1024 are bitwise equal and the nearest of point 0: the lower index comes first although it is met in another tile."""
    pts, idx, dist = arap_ref.tile_boundary_points()
    assert torch.equal(pts[1023], pts[1024]) and idx[0, :3].tolist() == [1023, 1024, 2048] and float(dist[0, 0]) == float(dist[0, 1])
    _check_graph(pts, idx, dist, None, "tile boundary", Ks=(1, 2, 3, 16))


@pytest.mark.parametrize("K", [1, 6, 7, 16])
def test_knn_lattice_ties_and_strict_radius_cut(K):
    """The cut after column K falls inside the 6-fold (K = 1), between the shells (6), and inside the 12-fold shell (7, 16).  With
    ``radius = 0.125`` the fourth shell is exactly at r^2 and is cut, the third is kept, from column ``least_edge_num`` on."""
    pts = arap_ref.lattice_points()
    idx, dist = arap_ref.knn_exact(pts, 17)
    assert int((dist[:, :16] == arap_ref.LATTICE_RADIUS ** 2).sum()) > 0 and int((dist[:, K - 1] == dist[:, K]).sum()) > 0
    for least in (0, 3, K, K + 4):
        _check_graph(pts, idx, dist, arap_ref.LATTICE_RADIUS, "lattice", Ks=(K,), least_edge_num=least, exact=True)


def test_knn_radius_zero_cuts_every_column():
    """``0 < 0`` fails for the twins at distance 0 as for everybody else: with ``least_edge_num = 0`` nothing is left."""
    pts, _, _, dist = _cloud(1025)
    assert int((dist[:, 0] == 0).sum()) == 11
    nn_idx, nn_dist = arap.knn_graph(pts.float().cuda(), 4, radius=0.0, least_edge_num=0)
    assert bool((nn_idx == -1).all()) and bool((nn_dist == float("inf")).all())


# ---- the energy

@functools.lru_cache(maxsize=None)
def _scene(name):
    return arap_ref.named_scene(name)


def _references(scene, weighted, need_source_grad=True):
    return (arap_ref.run(scene, torch.float64, weighted=weighted, need_source_grad=need_source_grad),
            arap_ref.run(scene, torch.float32, weighted=weighted, need_source_grad=need_source_grad))


def _parity(tag, scene, weighted, need_source_grad=True, **rule):
    """One forward + backward of the kernels on ``scene`` under the acceptance rule; where the unchanged rule holds R is exactly I."""
    r64, r32 = _references(scene, weighted, need_source_grad)
    got, _ = _run_hip(scene, weighted, need_source_grad=need_source_grad)
    torch.cuda.synchronize()
    got = {k: None if v is None else v.cpu() for k, v in got.items()}
    assert got["loss"].dim() == 0 and got["loss"].dtype == torch.float32 and got["R"].shape == r64["R"].shape
    worst = check_against_float64(tag, got, r64, r32, **rule)
    print(f"[arap {tag}] worst tensor at {worst:.3f} of its bar")
    assert torch.equal(got["R"][r64["unchanged"]], EYE.expand(int(r64["unchanged"].sum()), 3, 3))
    return got, r64


def _bitwise(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ENERGY_SCENES)
def test_energy_edge_scene_against_float64(name, weighted):
    scene = _scene(name)
    got, r64 = _parity(f"{name} w{int(weighted)}", scene, weighted)
    if name == "axes":                                      # frames 0, 1: one axis copied; 2: x copied off the marked set; 3: translated
        un = r64["unchanged"]
        assert bool(un[[0, 1, 3]].all()) and 0 < int(un[2].sum()) < un.shape[1]
        assert float(got["d_targets"][3].abs().max()) == 0.0
    if name == "diagonal":
        err = float((got["R"].double() - scene["R_closed"]).abs().max())
        print(f"[arap diagonal w{int(weighted)}] R against the closed form: max abs {err:.3e}")
        assert err <= FLOOR
    if name == "isolated":
        alone = torch.isin(scene["sample_idx"], scene["isolated"])
        assert int(alone.sum()) >= len(scene["isolated"])
        assert torch.equal(got["R"][:, alone], EYE.expand(got["R"].shape[0], int(alone.sum()), 3, 3))
        assert float(got["d_targets"][:, scene["isolated"]].abs().max()) == 0.0 and float(got["d_source"][scene["isolated"]].abs().max()) == 0.0


def test_translated_frame_alone_costs_exactly_nothing():
    """F = 1: the frame that is the quantised source translated.  Every edge is equal exactly, so R = I, the loss and the gradients are 0."""
    scene = _scene("axes")
    got, _ = _parity("axes, translated frame alone", dict(scene, targets=scene["targets"][3:]), True)
    assert float(got["loss"]) == 0.0 and float(got["d_targets"].abs().max()) == 0.0 and float(got["d_source"].abs().max()) == 0.0
    assert torch.equal(got["R"], EYE.expand_as(got["R"]))


def test_weight_on_absent_edges_is_ignored():
    """``weight`` non-zero where ``nn_idx`` is -1 gives bitwise what the masked weight gives."""
    scene = _scene("isolated")
    assert float(scene["weight"][scene["nn_idx"] < 0].min()) > 0.0
    a, _ = _run_hip(scene, True)
    b, _ = _run_hip(dict(scene, weight=scene["weight_masked"]), True)
    _bitwise(a, b)


@pytest.mark.parametrize("need_source_grad", [True, False])
@pytest.mark.parametrize("name", arap_ref.RANK_ONE)
def test_rank_one_covariances(name, need_source_grad):
    """K = 1 (``k1_nv2``: Nv = 2 as well): the loss and the gradients under the usual rule; R is not unique, so it is held to what
    defines it: a proper rotation that takes the source edge's direction to the target edge's, within 16 * 2^-24 (an fp64 result rounded
    once to fp32), and exactly I on frame 0, which is bitwise the source."""
    scene = _scene(name)
    got, r64 = _parity(f"{name} src{int(need_source_grad)}", scene, True, need_source_grad, keys=("loss", "d_targets", "d_source"))
    R, un = got["R"].double(), r64["unchanged"]
    assert bool(un[0].all()) and not bool(un[1:].any())
    se = arap_ref.edges(scene["source"], scene["nn_idx"])[scene["sample_idx"]][:, 0]
    te = arap_ref.edges(scene["targets"], scene["nn_idx"])[:, scene["sample_idx"]][:, :, 0]
    unit = lambda e: e / e.norm(dim=-1, keepdim=True)
    ortho = float((R.transpose(-1, -2) @ R - EYE.double()).abs().max())
    det = float((torch.det(R) - 1.0).abs().max())
    maps = float((torch.einsum("fsab,sb->fsa", R, unit(se)) - unit(te))[1:].abs().max())
    print(f"[arap {name}] R^T R - I {ortho:.3e}, det - 1 {det:.3e}, R s^ - t^ {maps:.3e}; bar {FLOOR:.3e}")
    assert ortho <= FLOOR and det <= FLOOR and maps <= FLOOR


@pytest.mark.parametrize("weighted", [False, True])
def test_near_rigid_motion_needs_the_fp64_interior(weighted):
    """A rotation plus 1e-4 noise: every output is an fp64 result rounded once to fp32, so the bar is the floor 16 * 2^-24 alone, not
    4 e32 (e32 of ``d_targets`` is about 1e-4 here, printed beside it: an fp32 interior would pass the usual rule)."""
    _parity(f"near_rigid w{int(weighted)}", _scene("near_rigid"), weighted, floor_only=True)


def test_hub_and_a_sample_repeated_300_times():
    """``hub`` itself (vertex 0 has about 2 Nv inverse-list entries) is among the scenes above; here one sample 300 times: the gradients
    are 300 x the single sample's (an fp64 sum of equal terms, rounded once)."""
    scene = _scene("hub")
    one, _ = _run_hip(dict(scene, sample_idx=torch.tensor([7])), True)
    many, _ = _run_hip(dict(scene, sample_idx=torch.full((300,), 7)), True)
    assert torch.equal(many["R"], one["R"].expand_as(many["R"]))
    for k in ("loss", "d_targets", "d_source"):
        err = _rel(many[k], 300.0 * one[k].double())
        print(f"[arap hub x 300] {k}: {err:.3e}")
        assert err <= 2.0 ** -22, k
    assert float(one["d_targets"][:, 0].abs().max()) > 0.0


@pytest.mark.parametrize("need_source_grad", [True, False])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("S", [1, 127, 128, 129, 257])
def test_launch_seams_in_frames_and_samples(S, F, need_source_grad):
    """F S around the forward's blocks of 128 and the reduction's stride of 256.  The last F frames: the generic one; with F = 3 also the
    one with x copied and the mirrored one."""
    scene = _scene("k5_nv257")
    sub = dict(scene, targets=scene["targets"][-F:], sample_idx=scene["sample_idx"].repeat(3)[:S])
    _parity(f"k5_nv257 F {F} S {S} src{int(need_source_grad)}", sub, True, need_source_grad)


@pytest.mark.parametrize("name", ["k5_nv255", "k5_nv256", "k5_nv257"])
def test_launch_seams_in_vertices_without_source_gradient(name):
    """Nv around the backward's block of 256 (with ``source.requires_grad``: among the scenes above; Nv = 2: ``k1_nv2``)."""
    _parity(f"{name} src0", _scene(name), True, need_source_grad=False)


def test_out_of_range_indices_are_absent_edges_and_empty_samples():
    """The docstring's contract: an ``nn_idx`` entry outside [0, Nv) is an absent edge, a ``sample_idx`` entry outside contributes nothing.
    Every kernel and ``inverse_list`` test the range before they use such an index.  Bitwise equal to the call with -1 in the graph and,
    at the same position of ``sample_idx`` (the reduction order stays), a vertex without edges; int64 indices give what int32 gives."""
    scene = _scene("isolated")
    Nv, S = scene["source"].shape[0], len(scene["sample_idx"])
    live = torch.nonzero(~torch.isin(scene["sample_idx"], scene["isolated"]))[:, 0]
    rows, where = scene["sample_idx"][live[:6]], live[6:14]
    assert bool((scene["nn_idx"][rows, 0] >= 0).all())
    dirty_nn, clean_nn = scene["nn_idx"].clone(), scene["nn_idx"].clone()
    dirty_nn[rows, 0] = torch.tensor([Nv, Nv + 5, -7, Nv, Nv + 5, -7])
    clean_nn[rows, 0] = -1
    dirty_s, clean_s = scene["sample_idx"].clone(), scene["sample_idx"].clone()
    dirty_s[where] = torch.tensor([-1, -5, Nv, Nv + 3, -1, -5, Nv, Nv + 3])
    clean_s[where] = scene["isolated"][:8]
    base, _ = _run_hip(scene, True)
    clean, _ = _run_hip(dict(scene, nn_idx=clean_nn, sample_idx=clean_s), True)
    dirty, _ = _run_hip(dict(scene, nn_idx=dirty_nn, sample_idx=dirty_s), True)
    dirty32, _ = _run_hip(dict(scene, nn_idx=dirty_nn.int(), sample_idx=dirty_s.int()), True)
    torch.cuda.synchronize()
    assert not torch.equal(base["loss"], clean["loss"])                                  # the entries that were replaced were live
    _bitwise(clean, dirty)
    _bitwise(dirty, dirty32)
    assert S == len(dirty_s) and bool(torch.isfinite(dirty["d_targets"]).all())


def _step(src, tgt, nn_idx, weight, sample_idx):
    loss, R = arap.arap_energy(src, tgt, nn_idx, weight=weight, sample_idx=sample_idx, return_rotations=True)
    d_tgt, d_src = torch.autograd.grad(loss, [tgt, src])
    return loss.detach(), R, d_tgt, d_src


def _device_inputs(scene):
    return (scene["source"].float().cuda().requires_grad_(True), scene["targets"].float().cuda().requires_grad_(True),
            scene["nn_idx"].cuda(), scene["weight"].float().cuda(), scene["sample_idx"].cuda())


def test_forward_and_backward_do_not_synchronise_with_the_host():
    args = _device_inputs(_scene("k5_nv257"))
    first = _step(*args)                                     # also loads the library and the kernels outside the guarded region
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        second = _step(*args)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_forward_and_backward_capture_into_a_graph():
    """One forward + ``torch.autograd.grad`` captured as a single chain; new targets copied into the static input and replayed give
    bitwise what an eager call on them gives."""
    scene = _scene("k5_nv257")
    src, tgt, nn_idx, weight, sample_idx = _device_inputs(scene)
    _step(src, tgt, nn_idx, weight, sample_idx)              # loads the library, warms the allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(src, tgt, nn_idx, weight, sample_idx)
    other = scene["targets"].flip(0).float().cuda()
    with torch.no_grad():
        tgt.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    eager = _step(src, other.clone().requires_grad_(True), nn_idx, weight, sample_idx)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
    assert not torch.equal(eager[2], _step(src, scene["targets"].float().cuda().requires_grad_(True), nn_idx, weight, sample_idx)[2])
