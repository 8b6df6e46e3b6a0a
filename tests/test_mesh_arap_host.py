"""CPU checks of the mesh branch of the ARAP loss (animate3d_amd/arap.py, ``MeshGraph``): the host constructors against the golden
recorded from the reference's own functions (tests/golden/mesh_arap.npz, made by tests/golden/make_mesh_arap_goldens.py) and against a
set-based brute force, the reference's recorded draw against our sampling contract, the uniformity of the sampler's restatement
(tests/mesh_ref.py: the generator and the integer acceptance rule of the kernel), and the refusals.  No kernel runs: there is no GPU here.

Uniformity bars.  One seed and a ring graph of 20 000 equal rows give 20 000 independent draws.  d = 7, K = 3: the chi-square statistic
over the 35 subsets against the uniform expectation has 34 degrees of freedom; the bar is its 1 - 1e-4 quantile (73.5).  d = 40, K = 3: the
per-position inclusion counts against 20 000 * 3 / 40; a draw fills three distinct cells, so the statistic is (40 - 3) / (40 - 1) of a
chi-square with 39 degrees of freedom in distribution: its 1 - 1e-4 quantile (80.6) is a bar on the safe side.  The seeds are fixed."""
import os

import numpy as np
import pytest
import scipy.stats
import torch

from animate3d_amd import arap, stage4d
from tests import mesh_ref

A3D_EINVAL, A3D_EUNSUPPORTED = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_arap.npz")
RING = 20000


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def golden_rows(g):
    return [g["col"][a:b].tolist() for a, b in zip(g["row_start"][:-1], g["row_start"][1:])]


def info_of(rows, order=None):
    """The parsed JSON of ``connected_vertices_info_path`` for these rows, its keys in ``order``."""
    return {str(v): {str(u): 1.0 for u in rows[v]} for v in (range(len(rows)) if order is None else order)}


def test_golden_graph_holds_the_cases_it_is_made_for(golden):
    deg = np.diff(golden["row_start"])
    K = int(golden["K"])
    assert len(deg) == 600 and int((deg == 1).sum()) == 3 and int((deg == 2).sum()) >= 3 and int(deg.max()) == 24 and K == 3
    rows = golden_rows(golden)
    assert sum(r != sorted(r) for r in rows) > 500                                             # neighbour order is not ascending
    drawn = set(golden["sample_idx"].tolist())
    assert int(np.argmax(deg)) in drawn and drawn & set(np.nonzero(deg == 2)[0].tolist()) and not drawn & set(np.nonzero(deg == 1)[0].tolist())
    assert len(drawn) < len(golden["sample_idx"])                                              # repeats


def test_from_connected_vertices_reproduces_the_reference_padded_form(golden):
    rows = golden_rows(golden)
    order = np.random.default_rng(0).permutation(len(rows)).tolist()                           # the keys in any order
    for info in (info_of(rows), info_of(rows, order)):
        graph = arap.MeshGraph.from_connected_vertices(info, "cpu")
        nn_idx, max_idx = graph.padded()
        assert nn_idx.dtype == torch.int64 and max_idx.dtype == torch.bool
        assert np.array_equal(nn_idx.numpy(), golden["nn_idx"]) and np.array_equal(max_idx.numpy(), golden["max_idx"])
        assert graph.Nv == 600 and graph.max_degree == 24 and np.array_equal(graph.degrees.numpy(), np.diff(golden["row_start"]))
        assert graph.row_start.dtype == graph.col.dtype == torch.int32
        assert np.array_equal(graph.row_start.numpy(), golden["row_start"]) and np.array_equal(graph.col.numpy(), golden["col"])
    nn_idx, max_idx = arap.prepare_arap_from_mesh_vertices(info_of(rows))                      # the drop-in: on the CPU, as the reference's
    assert np.array_equal(nn_idx.numpy(), golden["nn_idx"]) and np.array_equal(max_idx.numpy(), golden["max_idx"])


def test_from_padded_round_trips_and_takes_holes_anywhere(golden):
    dense = torch.from_numpy(golden["nn_idx"]).long()
    graph = arap.MeshGraph.from_padded(dense)
    nn_idx, max_idx = graph.padded()
    assert torch.equal(nn_idx, dense) and np.array_equal(max_idx.numpy(), golden["max_idx"])
    assert np.array_equal(graph.col.numpy(), golden["col"])
    again = arap.MeshGraph.from_padded(dense.int(), torch.from_numpy(golden["max_idx"]))       # int32, and the reference's mask given
    assert torch.equal(again.row_start, graph.row_start) and torch.equal(again.col, graph.col)
    holes = torch.tensor([[-1, 4, -1, 2, 2], [-1, -1, -1, -1, -1], [0, -1, 3, -1, 1], [1, 0, 2, 4, 0], [-1, -1, -1, -1, 3]])
    g = arap.MeshGraph.from_padded(holes)
    assert g.row_start.tolist() == [0, 3, 3, 6, 11, 12] and g.col.tolist() == [4, 2, 2, 0, 3, 1, 1, 0, 2, 4, 0, 3]     # duplicates kept
    assert g.degrees.tolist() == [3, 0, 3, 5, 1] and g.max_degree == 5
    assert g.padded()[0].tolist() == [[4, 2, 2, -1, -1], [-1] * 5, [0, 3, 1, -1, -1], [1, 0, 2, 4, 0], [3, -1, -1, -1, -1]]


def test_the_reference_draw_satisfies_the_sampling_contract(golden):
    """Every entry a neighbour of its row, entries distinct, min(P, deg) of them, then -1: the contract is what the reference does, up
    to the order inside a row (a random tuple there, row order here)."""
    rows, draw, K = golden_rows(golden), golden["draw"], int(golden["K"])
    assert draw.shape == (600, K)
    in_row_order = 0
    for v, r in enumerate(rows):
        got = draw[v].tolist()
        n = min(K, len(r))
        assert all(u in r for u in got[:n]) and len(set(got[:n])) == n and got[n:] == [-1] * (K - n), (v, got, r)
        in_row_order += [r.index(u) for u in got[:n]] == sorted(r.index(u) for u in got[:n])
    assert int((draw == -1).sum()) == sum(max(0, K - len(r)) for r in rows) > 0
    assert in_row_order < 300                                                                  # the reference's order is random
    ii, jj, nn = golden["ii"], golden["jj"], golden["nn"]                                      # animate3d.py:227-234
    assert np.array_equal(draw[ii, nn], jj) and len(jj) == int((draw != -1).sum())


def test_restatement_reproduces_the_reference_energy_on_its_own_draw(golden):
    """tests/arap_ref.energy in float64 on the recorded draw against the reference's fp32 rotations, error and gradient: the golden is
    well conditioned enough for the project's bars (tests/test_arap_host.py) to apply, -1 columns included."""
    from tests import arap_ref
    from tests.test_arap_host import ROT_BAR, SUM_BAR, _rel
    nodes = torch.from_numpy(golden["nodes"]).double()
    src, tgt = nodes[0].clone().requires_grad_(True), nodes[1:].clone().requires_grad_(True)
    loss, R, unchanged = arap_ref.energy(src, tgt, torch.from_numpy(golden["draw"]).long(), None, torch.from_numpy(golden["sample_idx"]).long())
    d_tgt, d_src = torch.autograd.grad(loss, [tgt, src])
    want_grad = torch.from_numpy(golden["grad"])
    errs = {"R": _rel(R, torch.from_numpy(golden["rotations"])), "loss": _rel(loss.detach(), torch.from_numpy(golden["error"])),
            "d_targets": _rel(d_tgt, want_grad[1:]), "d_source": _rel(d_src, want_grad[0])}
    print("[mesh arap golden] " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert bool(unchanged[0].all()) and not bool(unchanged[1:].any())
    assert errs["R"] <= ROT_BAR and max(errs["loss"], errs["d_targets"], errs["d_source"]) <= SUM_BAR, errs


CASES = {
    "tetrahedron": (np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]]), 4),
    "grid_7x5": (mesh_ref.grid_faces(7, 5), 35),
    "repeated_degenerate_unreferenced": (np.array([[0, 1, 2], [2, 1, 0], [0, 1, 2], [3, 3, 4], [5, 5, 5], [4, 2, 6]]), 9),   # 7, 8: no face
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_from_faces_equals_the_set_based_brute_force(name):
    faces, Nv = CASES[name]
    want = mesh_ref.adjacency_from_faces(faces, Nv)
    for dtype in (torch.int64, torch.int32):
        graph = arap.MeshGraph.from_faces(torch.from_numpy(faces).to(dtype), Nv)
        got = [graph.col[a:b].tolist() for a, b in zip(graph.row_start[:-1].tolist(), graph.row_start[1:].tolist())]
        assert got == want and graph.Nv == Nv and graph.max_degree == max(len(r) for r in want)
        assert all(v not in r for v, r in enumerate(got))                                       # no self-edge
        assert all(v in got[u] for v, r in enumerate(got) for u in r)                           # both directions
    if name != "grid_7x5":
        return
    assert sorted(set(map(len, want))) == [2, 3, 4, 6]
    with pytest.raises(IndexError):
        arap.MeshGraph.from_faces(torch.from_numpy(faces), Nv - 1)
    with pytest.raises(IndexError):
        arap.MeshGraph.from_faces(torch.tensor([[0, 1, -1]]), Nv)


def test_restatement_meets_the_contract_on_the_zoo():
    rows = mesh_ref.zoo_rows()
    row_start, col = mesh_ref.csr_of(rows)
    deg = np.diff(row_start)
    assert len(rows) == 1000 and sorted(set(deg.tolist())) == sorted(mesh_ref.ZOO_DEGREES) and sum(r != sorted(r) for r in rows) > 500
    for K in (1, 3, 4, 16):
        a, b = mesh_ref.sample(row_start, col, K, 12345), mesh_ref.sample(row_start, col, K, 12345 + 2 ** 32)
        mesh_ref.check_invariants(row_start, col, a, K)
        mesh_ref.check_invariants(row_start, col, b, K)
        assert not np.array_equal(a, b)                                                        # the seed's high word is part of the key
        whole = deg <= K
        assert np.array_equal(a[whole], mesh_ref.padded_of(rows + [[0] * K])[:-1, :K][whole])  # rows with d <= K are copied whole


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32_10 that have counter words 2 and 3 zero."""
    got = [int(w[0]) for w in mesh_ref.philox4x32_10(0, np.array([0]), np.array([0]))]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_draws_uniform_subsets(seed):
    K, d = 3, 7
    row_start, col = mesh_ref.csr_of(mesh_ref.ring_rows(RING, d))
    pos = mesh_ref.positions(row_start, col, mesh_ref.sample(row_start, col, K, seed))
    index = mesh_ref.subset_index(d, K)
    counts = np.bincount([index[tuple(p)] for p in pos.tolist()], minlength=len(index)).astype(np.float64)
    expect = RING / len(index)
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    bar = float(scipy.stats.chi2.ppf(1 - 1e-4, len(index) - 1))
    print(f"[mesh sampler d {d} K {K} seed {seed}] chi-square over {len(index)} subsets {chi2:.1f}, bar {bar:.1f}")
    assert len(index) == 35 and chi2 <= bar


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_includes_every_position_equally_often(seed):
    K, d = 3, 40
    row_start, col = mesh_ref.csr_of(mesh_ref.ring_rows(RING, d))
    pos = mesh_ref.positions(row_start, col, mesh_ref.sample(row_start, col, K, seed))
    counts = np.bincount(pos.reshape(-1), minlength=d).astype(np.float64)
    expect = RING * K / d
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    bar = float(scipy.stats.chi2.ppf(1 - 1e-4, d - 1))
    print(f"[mesh sampler d {d} K {K} seed {seed}] chi-square over {d} positions {chi2:.1f}, bar {bar:.1f}")
    assert int(counts.sum()) == RING * K and chi2 <= bar


def test_validation_errors(golden):
    rows = golden_rows(golden)
    missing = info_of(rows)
    missing["600"] = missing.pop("17")                                                         # 600 keys, vertex 17 not among them
    with pytest.raises(ValueError, match="vertex 17"):
        arap.MeshGraph.from_connected_vertices(missing, "cpu")
    with pytest.raises(ValueError):
        arap.MeshGraph.from_connected_vertices({}, "cpu")
    for bad in (600, -2):
        outside = info_of(rows)
        outside["5"] = {str(bad): 1.0, **outside["5"]}
        with pytest.raises(IndexError):
            arap.MeshGraph.from_connected_vertices(outside, "cpu")
    with pytest.raises(IndexError):
        arap.MeshGraph.from_padded(torch.tensor([[1, -1], [2, 0]]))
    with pytest.raises(ValueError):
        arap.MeshGraph.from_padded(torch.zeros(3, 2))
    graph = arap.MeshGraph.from_connected_vertices(info_of(rows), "cpu")
    for K in (0, 17, -1):
        with pytest.raises(NotImplementedError):
            graph.sample(K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        graph.sample(3)                                                                        # a graph on the CPU: there is no torch fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        arap.sample_matrix_vectorized(torch.from_numpy(golden["nn_idx"]).long(), 3, torch.from_numpy(golden["max_idx"]))


def test_training_step_refuses_a_mismatched_mesh_before_anything_touches_a_device(golden):
    graph = arap.MeshGraph.from_connected_vertices(info_of(golden_rows(golden)), "cpu")

    def untouched(*args, **kwargs):
        raise AssertionError("the step went on")
    common = dict(global_step=0, n_view=2, n_frame=4, progressive_iter_per_frame=10, bg=(1.0, 1.0, 1.0), graph=graph, render=untouched)
    loss = dict(lambda_rgb=1.0, lambda_mask=1.0, lambda_arap=4.0, arap_K=3)
    few = stage4d.Gaussians(torch.zeros(599, 3), None, None, None, None, 0)
    with pytest.raises(ValueError, match="600 vertices for 599 Gaussians"):
        stage4d.training_step(None, few, {}, loss=loss, **common)
    right = stage4d.Gaussians(torch.zeros(600, 3), None, None, None, None, 0)
    with pytest.raises(ValueError, match="arap_K"):
        stage4d.training_step(None, right, {}, loss={k: v for k, v in loss.items() if k != "arap_K"}, **common)


# ---- the C-ABI of a3d_mesh_sample_neighbours, as tests/test_cabi_contract.py holds the other entry points: made-up device addresses,
# every call differs from a valid launch in exactly one operand, and never in none
BASE = 0x7F00_0010_0000
OPERANDS = ("row_start", "col", "seed", "nn_idx")
VALID = dict(Nv=300, E=1800, K=3)


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.load_library()


def _call(lib, ptr=None, **geometry):
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = {n: BASE + 0x10_0000 * i for i, n in enumerate(OPERANDS)}
    p.update(ptr or {})
    g = dict(VALID, **geometry)
    return lib.a3d_mesh_sample_neighbours(None, g["Nv"], g["E"], p["row_start"], p["col"], g["K"], p["seed"], p["nn_idx"])


def test_mesh_sample_refusals(lib):
    """A missing or misaligned operand (the int32 operands 2 bytes off, the int64 seed 4 bytes off), no vertices and a negative edge
    count are A3D_EINVAL; a K outside 1 .. 16 is A3D_EUNSUPPORTED."""
    base = {n: BASE + 0x10_0000 * i for i, n in enumerate(OPERANDS)}
    for operand in OPERANDS:
        assert _call(lib, ptr={operand: None}) == A3D_EINVAL, f"NULL {operand}"
        off = 4 if operand == "seed" else 2
        assert _call(lib, ptr={operand: base[operand] + off}) == A3D_EINVAL, f"{operand} at +{off} bytes"
    for g in (dict(Nv=0), dict(Nv=-1), dict(E=-1)):
        assert _call(lib, **g) == A3D_EINVAL, g
    for K in (0, 17, -1):
        assert _call(lib, K=K) == A3D_EUNSUPPORTED, K
