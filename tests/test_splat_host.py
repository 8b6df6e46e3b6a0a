"""CPU checks of the splat rasterizer's host side: the batched camera helpers against the reference's own (tests/golden/gs_camera.npz),
closed-form checks of the dense restatement tests/gs_ref.py (the GPU tests' oracle), the sort-key packing and the tile rectangle, and
the render loops of csrc/splat.hip free of scratch."""
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
