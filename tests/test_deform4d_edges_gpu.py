"""The deformation-field kernels (csrc/deform4d.hip) at their seams, under the acceptance rule of tests/test_deform4d_gpu.py unchanged
(per tensor: relative L2 against the float64 restatement at most max(4 e32, 16 * 2^-24); a tensor whose reference is exactly zero is
exactly zero).  That file's one float64 scene has cubic spatial planes, N = 4000 and every frame shown; the scenes here
(deform_ref.EDGE_SCENES, whose two input conditions tests/test_deform4d_host.py checks on the CPU) are the smallest that have

* W != H in every plane (``noncubic``), where a swapped W / H in the cell formula, the gathers' texel decomposition or the unpacking of
  d_grid would show; the reference's own recorded outputs on such a grid (tests/golden/deform4d.npz);
* Gaussians and timestamps exactly on lattice points and borders (``lattice``), resolution 2 (``min_res``: one cell per axis, gather
  lists of length N), all Gaussians in a few cells (``cluster``: every other texel's gradient exactly zero);
* N = 1, exact multiples of the 128-row tile / 512-row slab (and of the 4 / 16 gather slices) and one past them (``seam_N``);
* frame / image states: T = 1, every frame bypassed, duplicate timestamps, an int32 image_to_time, frames shown in no image;
* losses on one output only, and inputs / cotangents that are non-contiguous or contiguous at an address that is not a multiple of 16.
"""
import functools
import os

import numpy as np
import pytest
import torch

from animate3d_amd import deform4d
from tests import deform_ref
from tests.test_deform4d_gpu import _assert_parity, _run_hip, _run_ref
from tests.test_deform4d_host import ROOT, _golden_scene

pytestmark = pytest.mark.gpu

UG = pytest.mark.parametrize("use_global", [False, True])


@functools.lru_cache(maxsize=None)
def _scene(name, use_global):
    """Built once per session and never written to (every run casts it into fresh tensors)."""
    return deform_ref.named_scene(name, use_global)


def _names(use_global):
    return deform_ref.LOCAL + (deform_ref.GLOBAL if use_global else ())


def _cots(B, N, which=(True, True, True)):
    g = torch.Generator().manual_seed(4)
    cots = [torch.randn(B, N, k, generator=g) for k in (3, 3, 4)]
    return [c if w else None for c, w in zip(cots, which)]


def _parity(tag, scene, use_global, i2t="scene", which=(True, True, True), **kw):
    """Outputs and the gradient of every leaf of ``scene`` against float64 under the acceptance rule -> the kernels' (outputs, gradients)."""
    if isinstance(i2t, str):
        i2t = scene.get("image_to_time")
    if i2t is not None and not torch.is_tensor(i2t):
        i2t = torch.tensor(i2t)
    N, T = scene["xyz"].shape[0], scene["timestamps"].shape[0]
    cots = _cots(T if i2t is None else len(i2t), N, which)
    kw = dict(use_global_trans=use_global, **kw)
    ref64 = _run_ref(scene, torch.float64, _names(use_global), i2t, cots, **kw)
    ref32 = _run_ref(scene, torch.float32, _names(use_global), i2t, cots, **kw)
    got = _run_hip(scene, _names(use_global), i2t, cots, **kw)
    torch.cuda.synchronize()
    _assert_parity(tag, ref64, ref32, got)
    return ref64, got


def _assert_equal(a, b):
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k


# ---------------------------------------------------------------------------------------------------------------- scenes against float64
@UG
@pytest.mark.parametrize("deform_scales", [False, True])
@pytest.mark.parametrize("fft", [False, True])
def test_noncubic_planes(use_global, deform_scales, fft):
    _parity(f"noncubic g{int(use_global)} s{int(deform_scales)} f{int(fft)}", _scene("noncubic", use_global), use_global,
            deform_scales=deform_scales, first_frame_trainable=fft)


@UG
@pytest.mark.parametrize("fft", [False, True])
@pytest.mark.parametrize("name", ["lattice", "min_res"])
def test_lattice_points_and_minimum_resolution(name, use_global, fft):
    scene = _scene(name, use_global)
    if name == "lattice":                       # the planted points are where they were put, and the cells of both precisions agree
        fixed = torch.tensor(deform_ref.LATTICE_POINTS, dtype=torch.float32)
        assert torch.equal(scene["xyz"][:len(fixed)], fixed)
        grid_size = deform_ref.EDGE_SCENES[name]["grid_size"]
        plan = deform4d.BinningPlan(scene["xyz"].cuda(), grid_size)
        assert torch.equal(plan.cells.cpu(), deform_ref.cell_ids(scene["xyz"], grid_size))
    _parity(f"{name} g{int(use_global)} f{int(fft)}", scene, use_global, first_frame_trainable=fft)


@UG
@pytest.mark.parametrize("name", ["seam_1", "seam_128", "seam_129", "seam_512", "seam_513", "cluster"])
def test_tile_seams_and_cluster(name, use_global):
    ref64, got = _parity(f"{name} g{int(use_global)}", _scene(name, use_global), use_global)
    if name == "cluster":                       # a texel no Gaussian touches: exactly zero, not merely small
        for k, g in ref64[1].items():
            if k.startswith("grids.") and k[-1] in "013":
                zero = g == 0
                assert 0.9 < zero.float().mean().item() < 1.0, k
                assert bool((got[1][k].cpu()[zero] == 0).all()), k


# ---------------------------------------------------------------------------------------------------------------- the reference's outputs
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "deform4d.npz"))


@UG
@pytest.mark.parametrize("deform_scales", [False, True])
@pytest.mark.parametrize("fft", [False, True])
def test_kernels_reproduce_reference_outputs(golden, use_global, deform_scales, fft):
    """The stored scene (N = 64, non-cubic grid, T = 4) through the kernels against what the reference itself computed, with the
    tolerance tests/test_deform4d_host.py gives the restatement."""
    s = deform_ref.cast(_golden_scene(golden), torch.float32, "cuda")
    with torch.no_grad():
        outs = deform4d.deform_gaussians(s["xyz"], s["scaling"], s["rotation"], s["timestamps"], s["grids"],
                                         {n: s["nets"][n] for n in _names(use_global)}, use_global_trans=use_global,
                                         deform_scales=deform_scales, first_frame_trainable=fft)
    key = f"{'global' if use_global else 'local'}_ds{int(deform_scales)}_fft{int(fft)}"
    for name, got in zip(("means", "scales", "rotations"), outs):
        want = torch.from_numpy(golden[f"{name}_{key}"])
        print(f"[deform4d golden {key}] {name}: max abs difference {(got.cpu() - want).abs().max().item():.3e}")
        torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- frames and images
@UG
@pytest.mark.parametrize("B", [1, 3])
def test_one_frame(use_global, B):
    _parity(f"one_frame B{B} g{int(use_global)}", _scene("one_frame", use_global), use_global, i2t=None if B == 1 else (0,) * B)


@UG
def test_every_frame_is_the_bypassed_first_frame(use_global):
    ref64, got = _parity(f"first_frame_only g{int(use_global)}", _scene("first_frame_only", use_global), use_global)
    for k, g in got[1].items():                 # no path to any plane or network; scaling and rotation get the bypass formulas
        assert (float(g.abs().max()) == 0.0) == (k not in ("scaling", "rotation")), k


@UG
@pytest.mark.parametrize("fft", [False, True])
def test_duplicate_timestamps(use_global, fft):
    _, got = _parity(f"duplicate_frames g{int(use_global)} f{int(fft)}", _scene("duplicate_frames", use_global), use_global,
                     first_frame_trainable=fft)
    for o in got[0].values():                   # equal timestamps, equal frames
        assert torch.equal(o[0], o[1]) and torch.equal(o[2], o[3])


@UG
def test_int32_image_to_time(use_global):
    scene = _scene("noncubic", use_global)
    i2t = torch.tensor(scene["image_to_time"])
    _, got32 = _parity(f"int32 image_to_time g{int(use_global)}", scene, use_global, i2t=i2t.to(torch.int32))
    got64 = _run_hip(scene, _names(use_global), i2t, _cots(len(i2t), scene["xyz"].shape[0]), use_global_trans=use_global)
    _assert_equal(got32, got64)


@UG
def test_frames_shown_in_no_image(use_global):
    """Frames 1, 2, 3 (the first frame among them) are in no image: img_start[f] == img_start[f + 1].  Such a frame contributes only
    exact-zero terms, added in frame order, so the call equals, bit for bit, the one that never had those frames."""
    scene = _scene("unshown_frames", use_global)
    assert scene["image_to_time"] == (4, 0, 0)
    _, got = _parity(f"unshown_frames g{int(use_global)}", scene, use_global)
    twin = dict(scene, timestamps=scene["timestamps"][[0, 4]])
    cots = _cots(3, scene["xyz"].shape[0])
    want = _run_hip(twin, _names(use_global), torch.tensor([1, 0, 0]), cots, use_global_trans=use_global)
    _assert_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- partial cotangents
@UG
@pytest.mark.parametrize("output", ["means", "rotations", "scales"])
def test_loss_on_one_output(use_global, output, monkeypatch):
    """The other two outputs take no part in the loss, and ``backward`` receives None for them (the function does not let autograd
    materialise zeros): asserted on what it was called with.  From ``scales`` with deform_scales=False no path leads to a plane or a
    network."""
    outputs = ("means", "scales", "rotations")
    which = tuple(output == o for o in outputs)
    received = []
    backward = deform4d._DeformGaussians.backward

    def spy(ctx, *cotangents):
        received.append(tuple(c is not None for c in cotangents))
        return backward(ctx, *cotangents)
    monkeypatch.setattr(deform4d._DeformGaussians, "backward", staticmethod(spy))
    kw = dict(deform_scales=False) if output == "scales" else {}
    ref64, got = _parity(f"loss on {output} g{int(use_global)}", _scene("noncubic", use_global), use_global, which=which, **kw)
    assert received == [which]                  # one backward pass, the two unused cotangents None
    if output == "scales":
        for k, g in got[1].items():
            assert (float(g.abs().max()) == 0.0) == (k != "scaling"), k


# ---------------------------------------------------------------------------------------------------------------- views
def _offset_view(t):
    """``t``'s values in a contiguous tensor 4 bytes past an allocation's start: what a parameter is inside a flat buffer."""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t.detach())
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class _OffsetCotangent(torch.autograd.Function):
    """Identity whose backward hands its cotangent on as a contiguous view at a 4-byte offset."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return _offset_view(g)


def _column_slice(name, t):
    wide = torch.zeros(t.shape[0], t.shape[1] + 3, device=t.device)
    v = wide[:, 2:2 + t.shape[1]]
    v.copy_(t)
    assert not v.is_contiguous()
    return v


@UG
@pytest.mark.parametrize("case", ["column_slices", "rotation_at_4_bytes", "cotangent_at_4_bytes"])
def test_views_equal_fresh_contiguous_tensors(use_global, case):
    """Bitwise against the same call on freshly allocated tensors.  ``rotation`` and the ``rotations`` cotangent are read 16 bytes at a
    time: a contiguous view that does not start on a multiple of 16 is copied by the host layer, not refused."""
    scene = _scene("noncubic", use_global)
    i2t = torch.tensor(scene["image_to_time"])
    hooks = {"column_slices": dict(make=_column_slice),
             "rotation_at_4_bytes": dict(make=lambda k, t: _offset_view(t) if k == "rotation" else t),
             "cotangent_at_4_bytes": dict(after=lambda outs: (outs[0], outs[1], _OffsetCotangent.apply(outs[2])))}[case]
    run = lambda **kw: _run_hip(scene, _names(use_global), i2t, _cots(len(i2t), scene["xyz"].shape[0]), use_global_trans=use_global, **kw)
    _assert_equal(run(**hooks), run())
