"""CPU checks of the deformation field's host side: the dense restatement tests/deform_ref.py (the GPU tests' oracle) against the
reference's own outputs (tests/golden/deform4d.npz), its gradcheck, the module's parameter names / shapes / initialisation against
the reference's, the refusals, the binning plan against a brute-force cell assignment, the scene generator's two input conditions,
and the hot kernels of csrc/deform4d.hip free of scratch."""
import os

import numpy as np
import pytest
import torch

from animate3d_amd import deform4d
from tests import deform_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELEASED = deform_ref.RELEASED


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "deform4d.npz"))


def _golden_scene(g):
    t = lambda k: torch.from_numpy(g[k])
    grids = [[t(f"grids.{s}.{p}") for p in range(6)] for s in range(2)]
    nets = {n: (t(f"{n}.layers.0.weight"), t(f"{n}.layers.2.weight")) for n in deform_ref.LOCAL + deform_ref.GLOBAL}
    return dict(xyz=t("xyz"), scaling=t("scaling"), rotation=t("rotation"), timestamps=t("timestamps"), grids=grids, nets=nets)


@pytest.mark.parametrize("use_global", [False, True])
@pytest.mark.parametrize("deform_scales", [False, True])
@pytest.mark.parametrize("fft", [False, True])
def test_restatement_reproduces_reference(golden, use_global, deform_scales, fft):
    s = _golden_scene(golden)
    assert float(s["timestamps"][0]) == -1.0 and bool((s["xyz"].abs() > 1).any())          # first frame and border clamp are in the golden
    means, scales, rots = deform_ref.deform(s["xyz"], s["scaling"], s["rotation"], s["timestamps"], s["grids"], s["nets"],
                                            use_global_trans=use_global, deform_scales=deform_scales, first_frame_trainable=fft)
    key = f"{'global' if use_global else 'local'}_ds{int(deform_scales)}_fft{int(fft)}"
    for name, got in (("means", means), ("scales", scales), ("rotations", rots)):
        torch.testing.assert_close(got, torch.from_numpy(golden[f"{name}_{key}"]), rtol=1e-5, atol=1e-5)


def test_restatement_gradcheck():
    scene = deform_ref.named_scene("gradcheck")
    s = deform_ref.cast(scene, torch.float64)
    leaves = [s["scaling"], s["rotation"]] + [p for g in s["grids"] for p in g] + [w for pair in s["nets"].values() for w in pair]
    for t in leaves:
        t.requires_grad_(True)
    i2t = torch.tensor([2, 0, 1, 2])

    def fn(*_):
        return deform_ref.deform(s["xyz"], s["scaling"], s["rotation"], s["timestamps"], s["grids"], s["nets"], image_to_time=i2t,
                                 use_global_trans=True)
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6, rtol=1e-4, nondet_tol=0.0)


@pytest.mark.parametrize("use_global", [False, True])
def test_module_matches_reference_state_dict_and_init(golden, use_global):
    tag = "global" if use_global else "local"
    grid_size = tuple(tuple(int(v) for v in r) for r in golden["grid_size"])
    torch.manual_seed(0)
    m = deform4d.HexPlaneDeformation(grid_size=grid_size, n_grid_dims=16, use_global_trans=use_global)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in golden[f"keys_{tag}"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(v) for v in golden[f"shapes_{tag}"]]
    planes = [p for g in m.grids for p in g]
    for k, p in enumerate(planes):
        if k % 6 in (2, 4, 5):                        # time planes: ones, in the reference too
            assert float(golden["init_min"][k]) == 1.0 == float(golden["init_max"][k])
            assert bool((p == 1).all())
        else:                                         # U(0.1, 0.5)
            assert 0.1 <= float(golden["init_min"][k]) and float(golden["init_max"][k]) <= 0.5
            assert 0.1 <= float(p.min()) and float(p.max()) <= 0.5 and abs(float(p.mean()) - 0.3) < 0.03
    for name in deform_ref.LOCAL + (deform_ref.GLOBAL if use_global else ()):
        net = getattr(m, name)
        assert bool((net.layers[2].weight == 0).all()) and float(net.layers[0].weight.abs().max()) > 0
    big = deform4d.HexPlaneDeformation()
    assert big.grid_size == RELEASED and tuple(big.grids[1][5].shape) == (1, 16, 16, 100)
    state = {k: torch.from_numpy(golden[k]) for k in sd}
    assert m.load_state_dict(state, strict=False).missing_keys == []


def test_refusals():
    m = deform4d.HexPlaneDeformation(grid_size=((3, 3, 3, 2), (4, 4, 4, 3)))
    with pytest.raises(RuntimeError):
        m(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4, 4), torch.zeros(2))
    nets = {n: getattr(m, n).weights() for n in deform_ref.LOCAL}
    with pytest.raises(RuntimeError):
        deform4d.deform_gaussians(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4, 4), torch.zeros(2), [list(g) for g in m.grids], nets)
    for kw, field in ((dict(n_grid_dims=8), "n_grid_dims"), (dict(n_neurons=64), "n_neurons"), (dict(n_hidden_layers=2), "n_hidden_layers"),
                      (dict(grid_size=((4, 4, 4, 2),)), "grid_size"), (dict(grid_size=((4, 4, 4, 1), (4, 4, 4, 2))), "grid_size")):
        with pytest.raises(NotImplementedError, match=field):
            deform4d.HexPlaneDeformation(**kw)


def test_binning_plan_against_brute_force():
    grid_size = ((6, 5, 7, 3), (12, 10, 14, 6))
    g = torch.Generator().manual_seed(5)
    xyz = torch.randn(300, 3, generator=g) * 0.8
    xyz[:4] = torch.tensor([[1.0, -1.0, 0.0], [-1.0, 1.0, 1.0], [3.0, -3.0, 0.5], [0.0, 0.0, 0.0]])
    cells = deform_ref.cell_ids(xyz, grid_size)
    n_cells = deform4d.plane_cells(grid_size)
    order, starts = deform4d.build_plan(cells, n_cells)
    dims = deform4d.plane_dims(grid_size)
    off = 0
    for k, ((W, H), (a, b)) in enumerate(zip(dims, deform4d.PAIRS * 2)):
        st = starts[off:off + n_cells[k] + 1].tolist()
        off += n_cells[k] + 1
        assert st[0] == 0 and st[-1] == xyz.shape[0]
        for n in range(xyz.shape[0]):                                  # brute force: the cell from the definition, in float64
            def cell(u, R):
                x = min(max((float(u) + 1) / 2 * (R - 1), 0.0), R - 1.0)
                return min(int(x), R - 2)
            want = cell(xyz[n, a], W) if b == 3 else cell(xyz[n, b], H) * (W - 1) + cell(xyz[n, a], W)
            assert int(cells[k, n]) == want, (k, n)
        for c in range(n_cells[k]):
            members = order[k, st[c]:st[c + 1]].tolist()
            assert members == [n for n in range(xyz.shape[0]) if int(cells[k, n]) == c]      # stable: ascending Gaussian index


@pytest.mark.parametrize("name,use_global", [("gpu_parity", False), ("gpu_parity", True), ("golden", False), ("golden", True),
                                             ("gradcheck", True)] + [(n, g) for n in deform_ref.EDGE_SCENES for g in (False, True)])
def test_scene_conditions_hold_in_both_precisions(golden, name, use_global):
    """Every scene a deform4d test compares on (deform_ref.SCENES, the golden one as stored, and deform_ref.EDGE_SCENES): float32 and
    float64 choose the same ReLU pattern and the same quaternion branch everywhere, and all four branches occur (the five-Gaussian
    gradcheck scene is too small for that; it is used with use_global_trans only and in float64 only).  An edge scene says in its table
    row whether it is large enough for all four branches and wide enough for a point outside [-1, 1]."""
    edge = deform_ref.EDGE_SCENES.get(name)
    want_branches = name != "gradcheck" if edge is None else edge["branches"]
    want_outside = name != "gradcheck" if edge is None else edge["outside"]
    if name == "golden":
        scene = _golden_scene(golden)
        gen = deform_ref.named_scene("golden")                        # the generator's scene is the stored one
        assert torch.equal(gen["xyz"], scene["xyz"]) and torch.equal(gen["nets"]["delta_rot_network"][0], scene["nets"]["delta_rot_network"][0])
    else:
        scene = deform_ref.named_scene(name, use_global)
    r32, b32 = deform_ref.patterns(scene, torch.float32, use_global)
    r64, b64 = deform_ref.patterns(scene, torch.float64, use_global)
    assert set(r64) == set(deform_ref.LOCAL + (deform_ref.GLOBAL if use_global else ()))
    for net in r64:
        assert torch.equal(r32[net], r64[net]), net
    if use_global:
        assert torch.equal(b32, b64)
        if want_branches:
            assert sorted(b64.unique().tolist()) == [0, 1, 2, 3]
    if want_outside:
        assert bool((scene["xyz"].abs() > 1).any())
    if edge is not None:
        assert scene["xyz"].shape[0] == edge["N"] and torch.equal(scene["timestamps"], torch.tensor(edge["timestamps"]))
        if edge["fixed"] is not None:                                  # planted before the resampling, and still there
            fixed = torch.tensor(edge["fixed"], dtype=torch.float32)
            assert torch.equal(scene["xyz"][:len(fixed)], fixed)
        if edge["center"] is not None:
            assert float((scene["xyz"] - torch.tensor(edge["center"])).abs().max()) < 6 * edge["spread"]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_hot_kernels_do_not_touch_scratch(tmp_path):
    """The per-(frame, Gaussian) kernels and the gathers keep their 32-wide vectors in registers: no scratch instruction in them."""
    from animate3d_amd import build
    from tests.test_cabi import _device_kernels
    lib = build.build(verbose=False)
    kernels = _device_kernels(os.path.join(os.path.dirname(lib), "obj", "deform4d.o"), str(tmp_path))
    hot = ("dg_spatial_kernel", "dg_mean_partial_kernel", "dg_deform_kernel", "dg_bwd_global_partial_kernel", "dg_bwd_kernel",
           "dg_bwd_spatial_kernel", "dg_sgather_kernel", "dg_tgather_kernel")
    for stem in hot:
        found = [n for n in kernels if stem in n]
        assert len(found) == 1, (stem, list(kernels))
        scratch = [t for _, t, _ in kernels[found[0]]["ins"] if t.startswith("scratch_") or "buffer_store_dword" in t and "off, s[0:3]" in t]
        assert not scratch, (stem, scratch[:3])
