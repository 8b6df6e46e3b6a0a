"""CPU checks of the ARAP feature: the torch restatement tests/arap_ref.py against the golden recorded from the reference's own functions
(tests/golden/arap.npz), the scene makers, and the host logic of animate3d_amd/arap.py (no kernel runs: there is no GPU here).

Golden bars.  The golden is the reference in float32: its SVD leaves a rotation error of about c * 2^-24 / COND with COND = 0.05 the
conditioning the scenes are resampled to and c < 10 for a 3 x 3 LAPACK SVD: 1e-5.  The residual ``tgt - R src`` then carries
``dR |src|``, against ``|tgt - R src|`` itself, which for these deformations (strain of 0.1 and more) is at least a tenth of ``|src|``:
1e-4 per term for the gradient, twice that for the squared terms of the loss: 2e-4 for both."""
import os

import numpy as np
import pytest
import torch

from animate3d_amd import arap
from tests import arap_ref

ROT_BAR, SUM_BAR = 1e-5, 2e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arap.npz")


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def golden_case(g, tag):
    K, Nv = int(g[f"{tag}_K"]), g["nodes"].shape[1]
    ii, jj, nn = (torch.from_numpy(g[f"{tag}_{k}"]).long() for k in ("ii", "jj", "nn"))
    return K, Nv, ii, jj, nn, arap.edges_to_dense(ii, jj, nn, Nv, K).long()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tag,variant", [("k3", "unit"), ("k3", "weighted"), ("k8", "unit")])
def test_restatement_reproduces_the_reference_golden(dtype, tag, variant):
    g = np.load(GOLDEN)
    assert np.array_equal(g["rotation_of_zero_S"], np.broadcast_to(np.eye(3, dtype=np.float32), (4, 3, 3)))     # the reference's svd(0): R = I
    K, Nv, ii, jj, nn, dense = golden_case(g, tag)
    nodes = torch.from_numpy(g["nodes"]).to(dtype)
    w = torch.from_numpy(g[f"{tag}_weight"]).to(dtype) if variant == "weighted" else None
    src, tgt = nodes[0].clone().requires_grad_(True), nodes[1:].clone().requires_grad_(True)
    loss, R, unchanged = arap_ref.energy(src, tgt, dense, w, torch.from_numpy(g["sample_idx"]).long())
    d_tgt, d_src = torch.autograd.grad(loss, [tgt, src])
    assert bool(unchanged[0].all()) and bool(unchanged[3].all()) and not bool(unchanged[1].any()) and not bool(unchanged[2].any())
    want_R, want_grad = torch.from_numpy(g[f"{tag}_{variant}_rotations"]), torch.from_numpy(g[f"{tag}_{variant}_grad"])
    assert float(torch.det(want_R[2].double()).min()) > 0.99                                 # the mirrored frame: flipped to proper rotations
    errs = {"R": _rel(R, want_R), "loss": _rel(loss.detach(), torch.from_numpy(g[f"{tag}_{variant}_error"])),
            "d_targets": _rel(d_tgt, want_grad[1:]), "d_source": _rel(d_src, want_grad[0])}
    print(f"[arap golden {tag} {variant} {dtype}] " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["R"] <= ROT_BAR and errs["loss"] <= SUM_BAR and errs["d_targets"] <= SUM_BAR and errs["d_source"] <= SUM_BAR, errs


def test_restatement_of_the_graph_matches_the_golden():
    g = np.load(GOLDEN)
    K, Nv, ii, jj, nn, dense = golden_case(g, "k3")
    pts = torch.from_numpy(g["nodes"][0])
    for dtype in (torch.float32, torch.float64):
        idx, dist = arap_ref.knn_bruteforce(pts.to(dtype), K)
        idx, dist = arap_ref.mask_radius(idx, dist, float(g["k3_radius"]))                   # K = least_edge_num: nothing is cut
        assert torch.equal(idx, dense)
    assert int((golden_case(g, "k8")[5] < 0).sum()) > 0


def test_edge_list_and_dense_graph_round_trip():
    g = torch.Generator().manual_seed(0)
    dense = torch.randint(0, 50, (50, 5), generator=g).to(torch.int32)
    dense[torch.rand(50, 5, generator=g) < 0.3] = -1
    ii, jj, nn = arap.dense_to_edges(dense)
    assert ii.dtype == torch.int64 and len(ii) == int((dense >= 0).sum()) and bool((jj >= 0).all())
    assert torch.equal(arap.edges_to_dense(ii, jj, nn, 50, 5), dense)
    i2, j2, n2 = arap.dense_to_edges(arap.edges_to_dense(ii, jj, nn, 50, 5))
    assert torch.equal(i2, ii) and torch.equal(j2, jj) and torch.equal(n2, nn)


def test_inverse_list_lists_every_pair_of_a_vertex_in_order():
    g = torch.Generator().manual_seed(1)
    Nv, K, S = 40, 3, 25
    nn_idx = torch.randint(0, Nv, (Nv, K), generator=g).to(torch.int32)
    nn_idx[torch.rand(Nv, K, generator=g) < 0.2] = -1
    sample_idx = torch.randint(0, Nv, (S,), generator=g)
    order, starts = arap.inverse_list(sample_idx, nn_idx)
    assert order.shape == (S * (K + 1),) and starts.shape == (Nv + 1,) and order.dtype == starts.dtype == torch.int32
    for v in range(Nv):
        want = [s * (K + 1) + c for s in range(S) for c in range(K + 1)
                if (int(sample_idx[s]) if c == 0 else int(nn_idx[sample_idx[s], c - 1])) == v]
        assert order[starts[v]:starts[v + 1]].tolist() == want, v
    assert int(starts[Nv]) == S * (K + 1) - int((nn_idx[sample_idx] < 0).sum())


def test_cpu_tensors_raise_and_limits_hold():
    pts = torch.rand(100, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        arap.knn_graph(pts, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        arap.arap_energy(pts, pts[None], torch.zeros(100, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        arap.cal_connectivity_from_points(pts[None], radius=0.1, K=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        arap.cal_arap_error(pts[None].repeat(2, 1, 1), *[torch.zeros(1, dtype=torch.long)] * 3, K=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        arap.ArapGraph(pts, K=3)
    for K in (0, 17, 64):
        with pytest.raises(NotImplementedError):
            arap.knn_graph(pts, K)
    with pytest.raises(ValueError):
        arap.knn_graph(pts[:3], 3)
    with pytest.raises(ValueError):
        arap.knn_graph(torch.rand(100, 2), 3)
    with pytest.raises(NotImplementedError):
        arap.cal_connectivity_from_points(pts[None], mode="floyd")
    with pytest.raises(NotImplementedError):
        arap.cal_connectivity_from_points(pts[None], trajectory=pts[:, None])


def test_graph_key_follows_the_tensor_its_version_and_the_settings():
    xyz = torch.rand(30, 3)
    nn_idx = torch.zeros(30, 3, dtype=torch.int32)
    graph = arap.ArapGraph.from_neighbours(xyz, nn_idx, radius=0.01)
    assert graph.matches(xyz) and graph.K == 3 and graph.builds == 1
    assert graph.refresh(xyz) is graph and graph.builds == 1                                 # nothing to search again
    assert not graph.matches(xyz.clone())                                                    # equal values, another tensor
    assert not graph.matches(xyz[:20])
    other = arap.ArapGraph.from_neighbours(xyz, nn_idx, radius=0.02)
    assert other.key != graph.key
    assert arap.ArapGraph.from_neighbours(xyz, nn_idx, radius=0.01, least_edge_num=2).key != graph.key
    assert arap.ArapGraph.from_neighbours(xyz, torch.zeros(30, 4, dtype=torch.int32), radius=0.01).key != graph.key
    xyz.add_(0.5)                                                                            # an in-place change invalidates the graph
    assert not graph.matches(xyz)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        graph.refresh(xyz)                                                                   # it would search again, on the GPU


@pytest.mark.parametrize("name", sorted(arap_ref.SCENES))
def test_scenes_terminate_and_float32_separates_every_case(name):
    """The scene maker ends within its rounds, the scene has every case the GPU comparison needs, and the float32 restatement decides
    every discrete choice (the unchanged rule, the sign of det) as float64 does, so its error e32 is rounding only."""
    sc = arap_ref.named_scene(name)
    assert 1 <= sc["rounds"] <= 40
    assert int((sc["nn_idx"] < 0).sum()) > 0 and len(torch.unique(sc["sample_idx"])) < len(sc["sample_idx"])
    assert torch.equal(sc["targets"][0], sc["source"]) and torch.equal(sc["targets"][1][:, 0], sc["source"][:, 0])
    assert torch.equal(sc["source"].float().double(), sc["source"]) and torch.equal(sc["targets"].float().double(), sc["targets"])
    for weighted in (True, False):
        r64, r32 = arap_ref.run(sc, torch.float64, weighted=weighted), arap_ref.run(sc, torch.float32, weighted=weighted)
        assert torch.equal(r64["unchanged"], r32["unchanged"])
        assert bool(r64["unchanged"][:2].all()) and not bool(r64["unchanged"][2:].any())
        assert float(torch.det(r64["R"]).min()) > 0.99
        w = sc["weight"] if weighted else arap_ref.default_weight(sc["nn_idx"], torch.float64)
        S2 = arap_ref.covariances(sc["source"], sc["targets"][2], sc["nn_idx"], w, sc["sample_idx"])[0]
        sig1 = torch.linalg.svdvals(S2)[:, 0]                                                # the mirrored frame: det <= 0 everywhere (a vertex
        assert bool((torch.det(S2) <= 1e-5 * sig1 ** 3).all())                              # with two edges, or a twin for a neighbour, has rank 2)
        for k in ("loss", "R", "d_targets", "d_source"):
            e32 = _rel(r32[k], r64[k])
            print(f"[arap scene {name} w{int(weighted)}] {k}: e32 {e32:.3e}")
            assert e32 < 1e-5, (k, e32)


def test_points_have_no_near_ties_so_float32_finds_the_float64_graph():
    pts, rounds, idx64, dist64 = arap_ref.make_points(6000, 16, 3, radius=0.05)
    assert rounds <= 40 and int((dist64[:, 0] == 0).sum()) == 11                             # six copies of five points: a triple among them
    idx32, dist32 = arap_ref.knn_bruteforce(pts.float(), 16)
    assert torch.equal(idx32, idx64[:, :16])
    m32, m64 = arap_ref.mask_radius(idx32, dist32, 0.05), arap_ref.mask_radius(idx64[:, :16], dist64[:, :16], 0.05)
    assert torch.equal(m32[0], m64[0]) and int((m64[0] < 0).sum()) > 0 and int((m64[0][:, 3:] >= 0).sum()) > 0


# ---- the scenes and clouds of tests/test_arap_edges_gpu.py: each terminates and holds the feature it is named for
FLOOR = 16 * 2.0 ** -24


def _inverse_entries(scene, v):
    pairs = torch.cat([scene["sample_idx"][:, None], scene["nn_idx"][scene["sample_idx"]]], dim=1)
    return int((pairs == v).sum())


@pytest.mark.parametrize("name", sorted(arap_ref.EDGE_SCENES))
def test_edge_scenes_terminate_and_hold_their_feature(name):
    sc = arap_ref.named_scene(name)
    src, tgt, nn, w, sidx = sc["source"], sc["targets"], sc["nn_idx"], sc["weight"], sc["sample_idx"]
    Nv, K, (F, S) = src.shape[0], nn.shape[1], (tgt.shape[0], len(sidx))
    assert 1 <= sc["rounds"] <= 5 and Nv <= 700 and S <= 300 and F <= 6
    assert all(torch.equal(t.float().double(), t) for t in (src, tgt, w))                  # fp32 values
    runs = {}
    for weighted in (True, False):
        r64, r32 = arap_ref.run(sc, torch.float64, weighted=weighted), arap_ref.run(sc, torch.float32, weighted=weighted)
        assert torch.equal(r64["unchanged"], r32["unchanged"])
        runs[weighted] = (r64, r32)
    r64, r32 = runs[True]
    un = r64["unchanged"]
    if name not in arap_ref.RANK_ONE:                                                        # wherever R is compared with the oracle
        assert float(arap_ref.worst_conditioning(src, tgt, nn, w, sidx).min()) >= arap_ref.COND
    if name in arap_ref.RANK_ONE:
        rank_one, closed = 0, 0.0
        for f in range(F):
            M, _, se, te, ws = arap_ref.covariances(src, tgt[f], nn, w, sidx)
            sig = torch.linalg.svdvals(M)
            rank_one += int(((sig[:, 0] > 0) & (sig[:, 1] <= 1e-12 * sig[:, 0])).sum())
            closed += float((ws[:, 0] * (te[:, 0].norm(dim=-1) - se[:, 0].norm(dim=-1)) ** 2).sum())
        assert K == 1 and rank_one == S * (F - 1) and bool(un[0].all()) and not bool(un[1:].any())
        assert abs(float(r64["loss"]) - closed) <= 1e-12 * closed                           # R s^ = t^: the loss is sum w (|t| - |s|)^2
        for k in ("loss", "d_targets", "d_source"):
            assert _rel(r32[k], r64[k]) < 1e-5, k
    elif name == "axes":
        assert torch.equal(src * 4096.0, torch.round(src * 4096.0))
        touch = torch.isin(torch.cat([sidx[:, None], nn[sidx]], dim=1), sc["marked"]).any(1)
        assert bool(un[[0, 1, 3]].all()) and torch.equal(un[2], ~touch) and 0 < int(touch.sum()) < S
        e_s, e_t = arap_ref.edges(src.float(), nn), arap_ref.edges(tgt[3].float(), nn)
        assert torch.equal(e_s, e_t) and torch.equal(arap_ref.edges(src, nn), arap_ref.edges(tgt[3], nn))
        assert not torch.equal(tgt[0][:, 0], src[:, 0]) and torch.equal(tgt[0][:, 1], src[:, 1]) and torch.equal(tgt[1][:, 2], src[:, 2])
    elif name == "isolated":
        iso = sc["isolated"]
        assert bool((nn[iso] == -1).all()) and not bool(torch.isin(nn, iso).any()) and bool(torch.isin(iso, sidx).all())
        assert torch.equal(sidx[sc["planted"]], iso) and float(w[nn < 0].min()) > 0.0 and int((nn[~torch.isin(torch.arange(Nv), iso)] < 0).sum()) > 0
        assert torch.equal(sc["weight_masked"], w * (nn >= 0))
    elif name == "diagonal":
        seen = set()
        for f in range(F):
            M = arap_ref.covariances(src, tgt[f], nn, w, sidx)[0]
            d = torch.diagonal(M, dim1=1, dim2=2)
            assert torch.equal(torch.diag_embed(d), M)                                       # exactly diagonal: nothing for Jacobi to rotate
            seen |= {(tuple(o), tuple(n)) for o, n in zip(d.abs().argsort(1).tolist(), (d < 0).tolist())}
        assert len(seen) == 6 * 4 and not bool(un.any())                                     # six orderings x (none, x, y or z negative)
        assert float((r64["R"] - sc["R_closed"]).abs().max()) <= 1e-12
    elif name == "near_rigid":
        e32 = _rel(r32["d_targets"], r64["d_targets"])
        print(f"[arap scene near_rigid] d_targets: e32 {e32:.3e}, floor {FLOOR:.3e}")
        assert e32 > 10 * FLOOR and not bool(un.any())                                       # the floor-only bar discriminates: fp32 inside fails it
    elif name == "hub":
        assert bool((nn[1:, 0] == 0).all()) and torch.equal(sidx, torch.arange(Nv).repeat(2)) and _inverse_entries(sc, 0) >= 2 * Nv
    else:
        want = {"k2": (600, 2, 129), "k16_radius": (700, 16, 257), "k5_nv255": (255, 5, 127), "k5_nv256": (256, 5, 127), "k5_nv257": (257, 5, 127)}
        assert (Nv, K, S) == want[name] and bool(un[:2].all())
        if name == "k16_radius":
            assert 0.5 < float((nn < 0).double().mean()) < 0.9


def test_lattice_and_tile_boundary_clouds_hold_their_ties():
    pts = arap_ref.lattice_points()
    assert pts.shape == (1331, 3) and torch.equal(pts * 16.0, torch.round(pts * 16.0)) and len(torch.unique(pts, dim=0)) == 1331
    idx, dist = arap_ref.knn_exact(pts, 17)
    assert torch.equal(dist * 256.0, torch.round(dist * 256.0))
    assert torch.equal(arap_ref.knn_exact(pts.float(), 17)[1], dist)                         # exact in fp32 too
    inner = int(torch.nonzero((pts.abs() <= 0.125).all(1))[0])
    assert (dist[inner] * 256.0).tolist() == [1.0] * 6 + [2.0] * 11                          # the 6-fold shell, then the 12-fold one
    for K in (1, 6, 7, 16):                                                                  # the cut falls inside a tie, in both tiles
        tied = (dist == dist[:, K - 1:K]) & (torch.arange(17) >= K - 1)
        assert int((tied.sum(1) > 1).sum()) > 0
        assert int((tied & (idx < 1024)).sum()) > 0 and int((tied & (idx >= 1024)).sum()) > 0
    r2 = arap_ref.LATTICE_RADIUS ** 2
    assert r2 == 4.0 / 256.0 and int((dist[:, :16] == r2).sum()) > 0 and int((dist[:, 3:16] < r2).sum()) > 0
    cut = arap_ref.mask_radius(idx[:, :16], dist[:, :16], arap_ref.LATTICE_RADIUS, 0)[0]
    assert bool((cut[dist[:, :16] == r2] == -1).all()) and bool((cut[dist[:, :16] < r2] >= 0).all())
    pts, idx, dist = arap_ref.tile_boundary_points()
    assert pts.shape == (2049, 3) and torch.equal(pts[1023], pts[1024]) and torch.equal(pts.float().double(), pts)
    assert idx[0, :3].tolist() == [1023, 1024, 2048] and float(dist[0, 0]) == float(dist[0, 1]) < float(dist[0, 2])
    assert torch.equal(arap_ref.knn_exact(pts.float(), 18)[0], idx)


def test_knn_exact_agrees_with_the_bruteforce_on_a_tie_free_cloud():
    pts, _, idx, dist = arap_ref.make_points(1500, 16, 4, duplicates=0)
    want_i, want_d = arap_ref.knn_exact(pts, 18)
    assert torch.equal(want_i, idx) and torch.equal(want_d, dist)
    pts, _, idx, dist = arap_ref.make_points(1025, 16, 2025, radius=0.119)                   # with the planted duplicates
    assert torch.equal(arap_ref.knn_exact(pts, 18)[0], idx)
