"""CPU checks of the splat rasterizer's host side: the batched camera helpers against the reference's own (tests/golden/gs_camera.npz),
closed-form checks of the dense restatement tests/gs_ref.py (the GPU tests' oracle), the sort-key packing and the tile rectangle, and
the render loops of csrc/splat.hip free of scratch; and, for the constructed scenes of tests/splat_scenes.py, the decision margins, the
branch predicates, fp32 / float64 agreement of every decision and the oracle's derivative against finite differences."""
import math
import os

import numpy as np
import pytest
import torch

from animate3d_amd import splat
from tests import gs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cam_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "gs_camera.npz"))


def test_camera_helpers_match_reference(cam_golden):
    g = cam_golden
    c2w, fovy = torch.from_numpy(g["c2w"]), torch.from_numpy(g["fovy"])
    w2c, full, center = splat.get_cam_info_gaussian(c2w, fovy, fovy, float(g["znear"]), float(g["zfar"]))
    torch.testing.assert_close(w2c, torch.from_numpy(g["world_view_transform"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(full, torch.from_numpy(g["full_proj_transform"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(center, torch.from_numpy(g["camera_center"]), rtol=1e-5, atol=1e-5)
    P = splat.get_projection_matrix_gaussian(float(g["znear"]), float(g["zfar"]), fovy, fovy)
    torch.testing.assert_close(P, torch.from_numpy(g["projection"]), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(splat.convert_pose(c2w), torch.from_numpy(g["converted_pose"]))
    a, b, c = splat.get_cam_info_gaussian(c2w[2], float(fovy[2]), float(fovy[2]), 0.1, 100.0)          # unbatched form
    torch.testing.assert_close(a, w2c[2]) and torch.testing.assert_close(c, center[2])


H = W = 33          # the pixel centre of p_proj.xy = 0 is pixel 16: power 0 there


def _cam(tan=0.5):
    view = torch.eye(4, dtype=torch.float64)[None]          # camera at the origin looking along +z (row-vector convention)
    P = splat.get_projection_matrix_gaussian(0.1, 100.0, 2 * math.atan(tan), 2 * math.atan(tan)).double().t()[None]
    return dict(viewmatrix=view, projmatrix=view @ P, campos=torch.zeros(1, 3, dtype=torch.float64), tanfovx=tan, tanfovy=tan,
                image_height=H, image_width=W)


def _g(means, scales, opac, colors=None, shs=None, bg=(0.0, 0.0, 0.0), deg=0, smod=1.0):
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    n = len(means)
    rots = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * n, dtype=torch.float64)
    return gs_ref.rasterize(t(means), t(scales), rots, t(opac)[:, None], colors_precomp=None if colors is None else t(colors),
                            shs=None if shs is None else t(shs), bg=t(bg), sh_degree=deg, scale_modifier=smod, **_cam())


def test_single_isotropic_gaussian_closed_form():
    z, s, o = 5.0, 0.2, 0.7
    img, radii, dep, alp = _g([[0.0, 0.0, z]], [[s, s, s]], [o], colors=[[0.2, 0.4, 0.6]], bg=(0.1, 0.1, 0.1))
    f = W / (2 * 0.5)
    var = (f * s / z) ** 2 + 0.3
    assert int(radii[0, 0]) == math.ceil(3 * math.sqrt(var))
    for (py, px) in ((16, 16), (16, 18), (13, 17)):
        a = o * math.exp(-0.5 * ((px - 16) ** 2 + (py - 16) ** 2) / var)
        a = a if a >= 1 / 255 else 0.0
        assert abs(float(alp[0, 0, py, px]) - a) < 1e-12
        assert abs(float(dep[0, 0, py, px]) - z * a) < 1e-12
        assert abs(float(img[0, 1, py, px]) - (0.4 * a + 0.1 * (1 - a))) < 1e-12


def test_alpha_clamp_skip_and_stop():
    big = [[30.0, 30.0, 30.0]]
    _, _, _, alp = _g([[0.0, 0.0, 4.0]], big, [1.0], colors=[[1.0, 1.0, 1.0]])
    assert abs(float(alp[0, 0, 16, 16]) - 0.99) < 1e-12                      # min(0.99, o G)
    _, _, _, alp = _g([[0.0, 0.0, 4.0]], big, [0.9 / 255], colors=[[1.0, 1.0, 1.0]])
    assert float(alp.abs().max()) == 0.0                                         # alpha < 1/255: skipped everywhere
    # 0.99, then 0.9 (T 0.01 -> 0.001), then 0.95 would take T to 5e-5 < 1e-4: stop before it
    img, _, dep, alp = _g([[0.0, 0.0, 2.0], [0.0, 0.0, 3.0], [0.0, 0.0, 4.0]], big * 3, [1.0, 0.9, 0.95],
                          colors=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], bg=(0.0, 0.0, 0.0))
    assert abs(float(alp[0, 0, 16, 16]) - (1 - 0.01 * 0.1)) < 1e-12
    assert abs(float(img[0, 0, 16, 16]) - 0.99) < 1e-12 and abs(float(img[0, 1, 16, 16]) - 0.009) < 1e-12
    assert float(img[0, 2, 16, 16]) == 0.0
    assert abs(float(dep[0, 0, 16, 16]) - (2 * 0.99 + 3 * 0.009)) < 1e-12


def test_culling_rules():
    _, radii, _, _ = _g([[0.0, 0.0, 0.2], [0.0, 0.0, 0.21], [0.0, 0.0, -3.0], [40.0, 0.0, 2.0], [0.0, 0.0, 3.0]],
                        [[0.01] * 3] * 5, [0.5] * 5, colors=[[1.0, 1.0, 1.0]] * 5)
    assert radii[0].tolist()[:4] == [0, radii[0, 1].item(), 0, 0] and int(radii[0, 1]) > 0 and int(radii[0, 4]) > 0


def test_sh_degree0_is_c0_fdc_plus_half():
    fdc = [[0.3, -0.2, -3.0]]
    pre = gs_ref.preprocess(torch.tensor([[0.0, 0.5, 3.0]], dtype=torch.float64), torch.full((1, 3), 0.1, dtype=torch.float64),
                            torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64), torch.full((1, 1), 0.5, dtype=torch.float64),
                            torch.tensor([fdc], dtype=torch.float64), None, _cam()["viewmatrix"], _cam()["projmatrix"],
                            torch.zeros(1, 3, dtype=torch.float64), 0.5, 0.5, H, W)
    want = [max(0.0, gs_ref.SH_C0 * v + 0.5) for v in fdc[0]]
    assert torch.allclose(pre["rgb"][0, 0], torch.tensor(want, dtype=torch.float64))
    assert want[2] == 0.0


def test_sort_key_packing_and_tile_rect():
    tiles = 3 * 4
    keys = [splat.sort_key(img, tile, tiles, d) for img, tile, d in ((1, 0, 0.5), (0, 5, 2.0), (0, 5, 1.0), (0, 2, 7.0))]
    assert keys[0] == ((1 * tiles + 0) << 32) | 0x3F000000
    assert sorted(range(4), key=lambda i: keys[i]) == [3, 2, 1, 0]            # (image, tile) major, then ascending depth
    assert all(0 <= k < 2 ** 63 for k in keys)
    assert splat.tile_grid(37, 53) == (4, 3)
    assert splat.tile_rect(15.5, 15.5, 3, 33, 33) == (0, 2, 0, 2)
    assert splat.tile_rect(-30.0, 10.0, 5, 33, 33) == (0, 0, 0, 1)         # off to the left: no tile column
    assert splat.tile_rect(100.0, 100.0, 500, 40, 60) == (0, 4, 0, 3)      # clipped to the grid
    pre = gs_ref.preprocess(torch.tensor([[0.0, 0.0, 5.0]], dtype=torch.float64), torch.full((1, 3), 0.2, dtype=torch.float64),
                            torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64), torch.full((1, 1), 0.5, dtype=torch.float64),
                            None, torch.ones(1, 3, dtype=torch.float64), _cam()["viewmatrix"], _cam()["projmatrix"],
                            torch.zeros(1, 3, dtype=torch.float64), 0.5, 0.5, H, W)
    x, y = pre["xy"][0, 0].tolist()
    assert tuple(pre["rect"][0, 0].tolist()) == (lambda r: (r[0], r[1], r[2], r[3]))(splat.tile_rect(x, y, int(pre["radii"][0, 0]), H, W))


def test_entry_points_refuse_cpu_tensors():
    with pytest.raises(RuntimeError):
        splat.rasterize_gaussians(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 4), torch.ones(4, 1), colors_precomp=torch.ones(4, 3),
                                  viewmatrix=torch.eye(4)[None], projmatrix=torch.eye(4)[None], campos=torch.zeros(1, 3), tanfovx=0.5,
                                  tanfovy=0.5, image_height=16, image_width=16, bg=torch.zeros(3))
    with pytest.raises(NotImplementedError):
        splat.rasterize_gaussians(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 4), torch.ones(4, 1), colors_precomp=torch.ones(4, 3),
                                  viewmatrix=torch.eye(4)[None], projmatrix=torch.eye(4)[None], campos=torch.zeros(1, 3), tanfovx=0.5,
                                  tanfovy=0.5, image_height=16, image_width=16, bg=torch.zeros(3), cov3D_precomp=torch.zeros(4, 6))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_render_loops_do_not_touch_scratch(tmp_path):
    """The forward and backward render kernels keep every per-pixel value in registers: no scratch instruction anywhere in them."""
    from animate3d_amd import build
    from tests.test_cabi import _device_kernels
    lib = build.build(verbose=False)
    kernels = _device_kernels(os.path.join(os.path.dirname(lib), "obj", "splat.o"), str(tmp_path))
    found = [n for n in kernels if "gs_render" in n]
    assert len(found) == 2, list(kernels)
    for n in found:
        scratch = [t for _, t, _ in kernels[n]["ins"] if t.startswith("scratch_") or "buffer_store_dword" in t and "off, s[0:3]" in t]
        assert not scratch, (n, scratch[:3])


# ---- the constructed scenes of tests/splat_scenes.py: what the GPU parity tests (tests/test_splat_edges_gpu.py) rely on, proved on the CPU
from tests import splat_scenes  # noqa: E402

ALL_SCENES = sorted(splat_scenes.SCENES)
_ORACLE = {}


def _oracle(name, dtype=torch.float64):
    if (name, dtype) not in _ORACLE:
        _ORACLE[name, dtype] = splat_scenes.oracle(splat_scenes.SCENES[name], dtype=dtype)
    return _ORACLE[name, dtype]


def test_scene_table_rules():
    """At most 8 Gaussians outside the seam scenes, at most 700 and 40 x 56 anywhere, non-square tanfov in at least half of the scenes,
    anisotropic scales, rotations off every axis, centres off the pixel grid."""
    sc = splat_scenes.SCENES
    assert all(sc[n]["inputs"]["means3D"].shape[-2] <= (700 if n.startswith("seam_") else 8) for n in sc)
    assert all(sc[n]["H"] <= 40 and sc[n]["W"] <= 56 for n in sc)
    assert sum(bool((s["cam"]["tanfovx"] != s["cam"]["tanfovy"]).all()) for s in sc.values()) * 2 >= len(sc)
    for n, s in sc.items():
        scales, q = s["inputs"]["scales"].reshape(-1, 3), s["inputs"]["rotations"].reshape(-1, 4)
        assert bool((scales.max(1).values / scales.min(1).values > 1.02).float().mean() > 0.9), n
        assert bool(((q / q.norm(dim=1, keepdim=True)).abs().max(1).values < 0.999).float().mean() > 0.99), n
        xy = _oracle(n)[0]["xy"]                                  # the seam scenes scatter hundreds of centres at random
        assert n.startswith("seam_") or float((xy - xy.round()).abs().min()) > 1e-3, n


@pytest.mark.parametrize("name", ALL_SCENES)
def test_scene_keeps_its_margins_and_takes_its_branch(name):
    """Every decision of the contract is at least gs_ref.MIN_MARGINS away from its threshold in float64, the conics are well conditioned,
    and the branch the scene is for is taken."""
    sc = splat_scenes.SCENES[name]
    pre, ex = _oracle(name)
    m = gs_ref.decision_margins(pre, sc["H"], sc["W"])
    for k, least in gs_ref.MIN_MARGINS.items():
        assert m[k] >= least, (name, k, m[k], least)
    assert m["conic_condition"] <= gs_ref.MAX_CONIC_CONDITION, (name, m["conic_condition"])
    assert sc["active"](pre, ex), (name, sc["branch"])


@pytest.mark.parametrize("name", sorted(splat_scenes.ordinary_counterparts()))
def test_scene_predicate_fails_on_the_ordinary_counterpart(name):
    """Centre moved on-screen, opacity 0.5, SH coefficients positive, depths apart: the predicate that proves the branch sees it idle."""
    sc = splat_scenes.ordinary_counterparts()[name]
    pre, ex = splat_scenes.oracle(sc)
    assert not sc["active"](pre, ex), name


@pytest.mark.parametrize("name", ALL_SCENES)
def test_scene_decisions_agree_between_fp32_and_float64(name):
    """The oracle evaluated in fp32 takes every decision the way float64 does: radii, rectangles, visibility and the per-(pixel,
    Gaussian) blend mask are identical.  This is what the margins are for, and what makes the fp32 oracle's error a fair yardstick."""
    (pre64, ex64), (pre32, ex32) = _oracle(name), _oracle(name, torch.float32)
    assert torch.equal(pre64["radii"], pre32["radii"]), name
    assert torch.equal(pre64["rect"][pre64["visible"]], pre32["rect"][pre32["visible"]]) and torch.equal(pre64["visible"], pre32["visible"]), name
    assert torch.equal(ex64["use"], ex32["use"]), (name, int((ex64["use"] != ex32["use"]).sum()))
    assert torch.equal(ex64["counts"], ex32["counts"]), name


def _scene_loss(sc, kw, rest, cot):
    img, _, dep, alp = gs_ref.rasterize(**kw, **rest)
    return (img * cot[0]).sum() + (dep * cot[1]).sum() + (alp * cot[2]).sum()


@pytest.mark.parametrize("name", ["ewa_clamp_x", "ewa_clamp_y", "ewa_clamp_xy", "alpha_clamp", "sh_clamp", "depth_tie"])
def test_oracle_gradient_matches_finite_differences(name):
    """The float64 oracle's autograd is the exact derivative of the contract at the clamps: along two seeded random directions per input
    (means2D included) it agrees with a central difference of step 1e-6 within 1e-6 relative.  (depth_tie: the two Gaussians of a
    tied pair move together, since the blending order is not differentiable in their depth difference.)"""
    sc = splat_scenes.SCENES[name]
    kw, rest = splat_scenes.to(sc, "cpu", torch.float64, means2D="per_image")
    B = rest["viewmatrix"].shape[0]
    g = torch.Generator().manual_seed(7)
    cot = (torch.randn(B, 3, sc["H"], sc["W"], generator=g, dtype=torch.float64), torch.randn(B, 1, sc["H"], sc["W"], generator=g, dtype=torch.float64) * 0.1,
           torch.randn(B, 1, sc["H"], sc["W"], generator=g, dtype=torch.float64))
    grads = dict(zip(kw, torch.autograd.grad(_scene_loss(sc, kw, rest, cot), list(kw.values()))))
    h = 1e-6
    with torch.no_grad():
        for k in kw:
            for _ in range(2):
                d = torch.randn(kw[k].shape, generator=g, dtype=torch.float64)
                if k == "means2D":
                    d[..., 2] = 0.0
                if k == "means3D" and name == "depth_tie":
                    d[:, 1], d[:, 3] = d[:, 0], d[:, 2]
                plus, minus = dict(kw, **{k: kw[k] + h * d}), dict(kw, **{k: kw[k] - h * d})
                fd = float(_scene_loss(sc, plus, rest, cot) - _scene_loss(sc, minus, rest, cot)) / (2 * h)
                an = float((grads[k] * d).sum())
                assert abs(fd - an) <= 1e-6 * abs(an), (name, k, fd, an)


def test_oracle_means2d_gradient_closed_form():
    """One isotropic Gaussian on the optical axis, loss = sum over pixels of x_pixel * alpha: d loss / d p_proj.x = (W / 2) sum x_pixel
    alpha (x_pixel - c_x) / var over the blended pixels (alpha >= 1/255; the radius covers every tile), and the third component is 0."""
    z, s, o = 5.0, 1.0, 0.7
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    m2 = torch.zeros(1, 3, dtype=torch.float64, requires_grad=True)
    img, radii, dep, alp = gs_ref.rasterize(t([[0.0, 0.0, z]]), t([[s, s, s]]), t([[1.0, 0.0, 0.0, 0.0]]), t([[o]]), colors_precomp=t([[0.2, 0.4, 0.6]]),
                                            bg=t([0.0, 0.0, 0.0]), means2D=m2, **_cam())
    xs = torch.arange(W, dtype=torch.float64)
    (alp[0, 0] * xs[None, :]).sum().backward()
    var = (W / (2 * 0.5) * s / z) ** 2 + 0.3
    assert int(radii[0, 0]) >= 17
    want_x = want_y = 0.0
    for py in range(H):
        for px in range(W):
            a = o * math.exp(-0.5 * ((px - 16) ** 2 + (py - 16) ** 2) / var)
            if a >= 1 / 255:
                want_x += px * a * (px - 16) / var * W / 2
                want_y += px * a * (py - 16) / var * H / 2
    assert abs(want_x) > 1.0 and abs(float(m2.grad[0, 0]) - want_x) <= 1e-10 * abs(want_x)
    assert abs(float(m2.grad[0, 1]) - want_y) <= 1e-10 * abs(want_x) and float(m2.grad[0, 2]) == 0.0
