"""GPU checks of the camera layer (animate3d_amd/cameras.py on csrc/camera_batch.hip) against tests/golden/cameras.npz, which
tests/golden/make_camera_goldens.py takes from the reference's own data modules, and against the float64 restatement of tests/cameras_ref.py.

The bound.  The kernels compute in fp64 from the fp32 values of the interface and round every output to fp32 once, so an output lies
within half an fp32 ulp of the exact value plus the fp64 error of a few dozen operations (below 1e-14 relative to the largest operand).
Every entry must therefore lie within ONE fp32 ulp taken at the largest magnitude in its own matrix row or vector
(``cameras_ref.ulp_bound``: ``spacing(float32(max |row|))``; a per-camera scalar: at its own magnitude).  Derived, not measured."""
import json
import os
import random

import numpy as np
import pytest
import torch

from animate3d_amd import cameras, deform4d, splat, stage4d
from tests import cameras_ref as R
from tests import stage4d_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cameras.npz")
FIELDS = R.RANDOM_FIELDS


@pytest.fixture(scope="module")
def golden():
    data = dict(np.load(GOLDEN))
    return data, json.loads(str(data["meta"]))


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _within(tag, got, exact):
    """Every entry of ``got`` within ``ulp_bound(exact)`` of ``exact``; prints the figure first and returns the largest deviation."""
    got, exact = _f64(got) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64), np.asarray(exact, np.float64)
    assert got.shape == exact.shape, (tag, got.shape, exact.shape)
    dev, bound = np.abs(got - exact), R.ulp_bound(exact)
    print(f"[cameras] {tag}: max deviation {dev.max():.3e}, max deviation / bound {(dev / bound).max():.3f}")
    assert (dev <= bound).all(), (tag, float(dev.max()), float((dev / bound).max()))
    return float(dev.max())


def _random_case(golden, i):
    data, meta = golden
    case = R.RANDOM_CASES[i]
    sampler = cameras.RandomCameraSampler(**case["cfg"], device="cuda")
    sampler.update_step(case["step"])
    draws = [torch.from_numpy(data[f"random{i}_{k}"]).cuda() for k in ("obj", "pert_u", "pert_n")]
    cb = sampler.from_draws(*draws, case["elev_mode"])
    exact = R.random_from_draws(case["cfg"], case["step"], *(data[f"random{i}_{k}"] for k in ("obj", "pert_u", "pert_n")), case["elev_mode"])
    return case, meta["random"][i], cb, exact


def _fixed_sets(golden):
    """(tag, golden prefix, batch, meta) of the data views, the orbit sets and the test set."""
    _, meta = golden
    out = [("data", "data", cameras.data_view_cameras(**R.DATA_VIEW_CASE, device="cuda"), meta["data"])]
    for i, case in enumerate(R.ORBIT_CASES):
        cfg = dict(R.ORBIT_CFG, n_val_views=case["n_val_views"], n_test_views=case["n_test_views"])
        out.append((f"orbit{i}", f"orbit{i}", cameras.orbit_cameras(cfg, case["split"], device="cuda"), meta["orbit"][i]))
    out.append(("testset", "testset", cameras.testset_cameras(dict(R.TESTSET_CFG), "test", device="cuda"), meta["testset"]))
    return out


def _fixed_exact(data, prefix, cb):
    fovy_deg = {"data": R.DATA_VIEW_CASE["default_fovy_deg"], "testset": R.TESTSET_CFG["eval_fovy_deg"]}.get(prefix, R.ORBIT_CFG["eval_fovy_deg"])
    return R.spherical(data[f"{prefix}_elevation"], data[f"{prefix}_azimuth"], data[f"{prefix}_camera_distances"],
                       [fovy_deg] * cb.c2w.shape[0])


@pytest.mark.parametrize("i", range(len(R.RANDOM_CASES)), ids=[c["name"] for c in R.RANDOM_CASES])
def test_from_draws_against_float64_and_the_reference(golden, i):
    """Tests 1 and 2 of the camera layer.  1: every output of ``from_draws`` on the recorded draws within the derived bound of the float64
    restatement.  2: per field the kernel is no further from float64 than ``max(ref_err, bound)``, hence within ``ref_err + bound`` of the
    reference's own fp32 values; timestamps, sizes and the repeat structure are equal."""
    data, _ = golden
    case, meta, cb, exact = _random_case(golden, i)
    n_view, F = case["cfg"]["n_view"], case["cfg"]["total_frame"]
    B = meta["batch_size"]
    assert cb.c2w.shape == (B, 4, 4) and (cb.height, cb.width) == (meta["height"], meta["width"]) == (cb["height"], cb["width"])
    for f in FIELDS:
        dev = _within(f"{case['name']} {f}", cb[f], exact[f])                                                   # test 1
        bound = float(R.ulp_bound(exact[f]).max())
        assert dev <= max(meta["ref_err"][f], bound), (f, dev, meta["ref_err"][f])                              # test 2
        vs_ref = np.abs(_f64(cb[f]) - data[f"random{i}_{f}"].astype(np.float64))
        print(f"[cameras] {case['name']} {f}: against the reference {vs_ref.max():.3e}, the reference's own error {meta['ref_err'][f]:.3e}")
        assert (vs_ref <= meta["ref_err"][f] + R.ulp_bound(exact[f])).all(), f
    # the reference's timestamps have n_view * total_frame rows whatever the batch size (uncond_hybrid.py:400-404 never repeats them over
    # the objects): ours are per image, the reference's rows once per object
    stamps = data[f"random{i}_timestamps"]
    assert stamps.shape == (n_view * F, 1) and cb["timestamps"].shape == (B, 1)
    assert np.array_equal(cb["timestamps"].cpu().numpy(), np.tile(stamps, (B // (n_view * F), 1)))
    assert cb.frame_ids == tuple(range(F)) * (B // F) and torch.equal(cb.frames.cpu(), torch.linspace(-1, 1, F))
    per_object = lambda t: t.reshape(B // (n_view * F), n_view * F, -1)                 # noqa: E731
    per_view = lambda t: t.reshape(B // F, F, -1)                                        # noqa: E731
    for f in ("elevation", "fovy", "camera_distances"):                                   # one draw per object
        assert bool((per_object(cb[f]) == per_object(cb[f])[:, :1]).all()), f
        assert not bool((per_object(cb[f])[0, 0] == per_object(cb[f])[1, 0]).all()), f
    az = per_view(cb["azimuth"])                                                          # one per (object, view)
    assert bool((az == az[:, :1]).all()) and len(set(az[:, 0, 0].tolist())) == B // F
    pos = per_view(cb["camera_positions"])                                                # the perturbation is per image
    assert not bool((pos[:, 0] == pos[:, 1]).all(dim=-1).any())
    with pytest.raises(KeyError, match="not built"):
        cb["rays_d"]


def test_fixed_sets_against_float64_and_the_reference(golden):
    data, _ = golden
    for tag, prefix, cb, meta in _fixed_sets(golden):
        exact = _fixed_exact(data, prefix, cb)
        for f in FIELDS:
            # fovy is rounded on the host from the float64 product of the fp32 degrees: half an ulp, inside the same bound
            dev = _within(f"{tag} {f}", cb[f], exact[f])
            assert dev <= max(meta["ref_err"][f], float(R.ulp_bound(exact[f]).max())), (tag, f)
            vs_ref = np.abs(_f64(cb[f]) - data[f"{prefix}_{f}"].astype(np.float64))
            assert (vs_ref <= meta["ref_err"][f] + R.ulp_bound(exact[f])).all(), (tag, f)
        for f in ("elevation", "azimuth", "camera_distances"):
            assert np.array_equal(cb[f].cpu().numpy(), data[f"{prefix}_{f}"]), (tag, f)
        assert np.array_equal(cb["timestamps"].cpu().numpy(), data[f"{prefix}_timestamps"]), tag
        assert (cb.height, cb.width) == (meta["height"], meta["width"]), tag
    cb = _fixed_sets(golden)[3][2]                                                        # 7 test views, F = 3: the (i // F) * F hold
    assert cb.frame_ids == (0, 1, 2, 0, 1, 2, 0)
    assert torch.equal(cb.c2w[0], cb.c2w[1]) and torch.equal(cb.c2w[0], cb.c2w[2]) and torch.equal(cb.c2w[3], cb.c2w[5])
    assert not torch.equal(cb.c2w[0], cb.c2w[3]) and not torch.equal(cb.c2w[3], cb.c2w[6])


def test_rasterizer_inputs_against_float64(golden):
    """Test 3: ``w2c``, ``full_proj``, ``campos``, ``tanfov`` of all three kernels against ``get_cam_info_gaussian`` restated in float64."""
    data, _ = golden
    names = ("w2c", "full_proj", "campos", "tanfov")
    for i in range(len(R.RANDOM_CASES)):
        case, _, cb, exact = _random_case(golden, i)
        for name, want in zip(names, R.cam_info(exact["c2w"], exact["fovy"])):
            _within(f"{case['name']} {name}", getattr(cb, name), want)
    for tag, prefix, cb, _ in _fixed_sets(golden):
        exact = _fixed_exact(data, prefix, cb)
        for name, want in zip(names, R.cam_info(exact["c2w"], exact["fovy"])):
            _within(f"{tag} {name}", getattr(cb, name), want)
    for prefix in ("random0", "random2", "data", "testset"):                              # any c2w: the reference's own fp32 matrices
        c2w, fovy = data[f"{prefix}_c2w"], data[f"{prefix}_fovy"]
        B = c2w.shape[0]
        stamps = [float(t) for t in np.resize(data[f"{prefix}_timestamps"].reshape(-1), B)]      # random: one object's rows, tiled
        cb = cameras.CameraBatch.from_c2w(torch.from_numpy(c2w).cuda(), torch.from_numpy(fovy).cuda(), stamps, 16, 16)
        for name, want in zip(names, R.cam_info(c2w, fovy)):                              # numpy.linalg.inv in float64
            _within(f"from_c2w {prefix} {name}", getattr(cb, name), want)
        assert torch.equal(cb.c2w.cpu(), torch.from_numpy(c2w)) and np.array_equal(cb.timestamps.cpu().numpy().reshape(-1), np.float32(stamps))
        frames, i2t = stage4d.frames_of_images(cb.timestamps)
        assert torch.equal(frames, cb.frames) and torch.equal(i2t, cb.image_to_time)
        assert "elevation" not in cb and set(cb.keys()) == {"c2w", "fovy", "timestamps", "camera_positions", "height", "width"}
    general = torch.from_numpy(data["random1_c2w"]).clone()                               # not rigid: scaled, sheared
    general[:, :3, :3] = general[:, :3, :3] @ torch.tensor([[1.5, 0.2, 0.0], [0.0, 0.7, 0.1], [0.3, 0.0, 1.1]])
    fovy = torch.from_numpy(data["random1_fovy"])
    cb = cameras.CameraBatch.from_c2w(general.cuda(), fovy.cuda(), [0.0] * general.shape[0], 16, 16)
    for name, want in zip(names, R.cam_info(general.numpy(), fovy.numpy())):
        _within(f"from_c2w general {name}", getattr(cb, name), want)


# ---- the render path and the step

N_GAUSS, SIDE = 64, 16


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(21)
    gaussians = stage4d.Gaussians(xyz=(torch.randn(N_GAUSS, 3, generator=g) * 0.25).cuda(),
                                  scaling=(torch.rand(N_GAUSS, 3, generator=g) * 1.0 - 2.6).cuda(),
                                  rotation=torch.randn(N_GAUSS, 4, generator=g).cuda(),
                                  opacity=torch.sigmoid(torch.randn(N_GAUSS, 1, generator=g) + 1.0).cuda(),
                                  shs=(torch.randn(N_GAUSS, 1, 3, generator=g) * 0.5).cuda(), sh_degree=0)
    field = deform4d.HexPlaneDeformation(use_global_trans=True)
    with torch.no_grad():
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return dict(gaussians=gaussians, field=field.cuda(), bg=torch.tensor(stage4d_ref.BG, device="cuda"))


def _sampler(**over):
    cfg = dict(R.RANDOM_CASES[3]["cfg"], height=SIDE, width=SIDE)                         # n_view 2, total_frame 3, 12 cameras
    cfg.update(over)
    s = cameras.RandomCameraSampler(**cfg, device="cuda")
    s.update_step(100)
    return s


def test_render_batch_with_cameras_is_the_direct_call_bitwise(scene):
    """Test 4, first half: the wiring.  No tolerance arises."""
    g, field, bg = scene["gaussians"], scene["field"], scene["bg"]
    cb = _sampler().sample(generator=torch.Generator(device="cuda").manual_seed(4), rng=random.Random(1))
    out = stage4d.render_batch(field, g, None, None, None, None, None, bg, do_guidance=True, cameras=cb)
    with torch.no_grad():
        means, scales, rots = field(g.xyz, g.scaling, g.rotation, cb.frames, cb.image_to_time, deform_scales=True)
        image, radii, depth, alpha = splat.rasterize_gaussians(means, scales, rots, g.opacity, shs=g.shs, viewmatrix=cb.w2c, projmatrix=cb.full_proj,
                                                               campos=cb.campos, tanfovx=cb.tanfov, tanfovy=cb.tanfov, image_height=SIDE,
                                                               image_width=SIDE, bg=bg, sh_degree=0)
    assert torch.equal(out["image"], image) and torch.equal(out["alpha"], alpha) and torch.equal(out["radii"], radii)
    assert torch.equal(out["comp_depth"], depth.permute(0, 2, 3, 1)) and torch.equal(out["means3D"], means)
    assert float(image.std()) > 0.01 and bool((radii > 0).any())                          # a picture, not the background
    same = stage4d.render_batch(field, g, None, None, None, SIDE, SIDE, bg, do_guidance=True, cameras=cb)
    assert torch.equal(same["image"], image)
    tensors = stage4d.render_batch(field, g, cb.c2w, cb.fovy, cb.timestamps, SIDE, SIDE, bg, do_guidance=True)
    assert torch.equal(tensors["means3D"], means) and torch.equal(tensors["scales"], scales)   # the same frames: the field's output is bit-equal
    with pytest.raises(ValueError, match="cameras="):
        stage4d.render_batch(field, g, cb.c2w, None, None, SIDE, SIDE, bg, do_guidance=True, cameras=cb)
    out["image"].sum().backward()
    assert all(p.grad is not None for p in field.parameters())
    for p in field.parameters():
        p.grad = None


def test_no_host_synchronisation_before_the_rasterizer(scene, monkeypatch):
    """Test 4, second half: under torch's sync debug mode ``sample()`` and everything ``render_batch(cameras=)`` does before the
    rasterizer call complete; the tensor path (two solver calls, a ``torch.unique``) raises under the same mode."""
    g, field, bg = scene["gaussians"], scene["field"], scene["bg"]
    sampler, gen = _sampler(), torch.Generator(device="cuda").manual_seed(4)
    warm = sampler.sample(generator=gen, rng=random.Random(1))                            # the field's plan and the library are ready
    stage4d.render_batch(field, g, None, None, None, None, None, bg, do_guidance=False, cameras=warm, generator=gen)
    seen = []

    def fake_rasterizer(means, scales, rots, opacity, **kw):
        seen.append(kw)
        B = means.shape[0]
        z = torch.zeros(B, 3, SIDE, SIDE, device=means.device)
        return z, torch.zeros(B, N_GAUSS, dtype=torch.int32, device=means.device), z[:, :1], z[:, :1]
    monkeypatch.setattr(stage4d, "rasterize_gaussians", fake_rasterizer)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    raised = None
    try:
        torch.cuda.set_sync_debug_mode("error")
        cb = sampler.sample(generator=gen, rng=random.Random(2))
        sub = cb.take([0, 1, 3, 4])
        stage4d.render_batch(field, g, None, None, None, None, None, bg, do_guidance=False, cameras=cb, generator=gen)
        stage4d.render_batch(field, g, None, None, None, None, None, bg, do_guidance=True, cameras=sub)
        try:
            stage4d.render_batch(field, g, cb.c2w, cb.fovy, cb.timestamps, SIDE, SIDE, bg, do_guidance=True)
        except RuntimeError as e:
            raised = e
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert len(seen) == 2 and seen[0]["viewmatrix"] is cb.w2c and seen[0]["projmatrix"] is cb.full_proj and seen[0]["tanfovx"] is cb.tanfov
    assert seen[1]["viewmatrix"].shape == (4, 4, 4) and torch.equal(seen[1]["campos"], cb.campos[[0, 1, 3, 4]])
    assert raised is not None, "the tensor path synchronises (linalg.inv, unique): the mode must raise, or this test cannot fail"


def test_training_step_with_camera_batches(scene):
    """Test 5: 2 views x 4 frames at 8 x 8.  A step whose batch carries ``CameraBatch``es hands the render the same images in the same
    order, and draws the same values from the generator, as the step on the same cameras given as tensors."""
    g, field = scene["gaussians"], scene["field"]
    n_view, n_frame, side = 2, 4, 8
    S = n_view * n_frame
    data = cameras.data_view_cameras(default_elevation_deg=12.0, default_azimuth_deg=[0.0, 95.0], default_camera_distance=2.2, default_fovy_deg=45.0,
                                     n_view=n_view, total_frame=n_frame, height=side, width=side, device="cuda")
    sampler = cameras.RandomCameraSampler(**dict(R.RANDOM_CASES[3]["cfg"], height=side, width=side, total_frame=n_frame, batch_size=S), device="cuda")
    sampler.update_step(100)
    rand = sampler.sample(generator=torch.Generator(device="cuda").manual_seed(6), rng=random.Random(3))
    gen0 = torch.Generator().manual_seed(8)
    rgb, mask = torch.rand(S, side, side, 3, generator=gen0).cuda(), (torch.rand(S, side, side, 1, generator=gen0) > 0.5).cuda()
    with_batches = dict(rgb=rgb, mask=mask, cameras=data, random_camera=rand)
    with_tensors = dict(rgb=rgb, mask=mask, c2w=data.c2w, fovy=data.fovy, timestamps=data.timestamps,
                        random_camera=dict(c2w=rand.c2w, fovy=rand.fovy, timestamps=rand.timestamps, height=side, width=side))
    loss = dict(stage4d_ref.LOSS, lambda_arap=0.0, lambda_tv_loss=0.5)
    step = 25
    kw = dict(loss=loss, global_step=step, n_view=n_view, n_frame=n_frame, progressive_iter_per_frame=10, bg=stage4d_ref.BG,
              guidance=lambda rgb: (rgb ** 2).mean())

    def recording(log):
        def render(field_, gaussians, c2w, fovy, timestamps, height, width, bg, *, do_guidance, first_frame_trainable, keep_prob, generator,
                   **extra):
            assert set(extra) <= {"cameras"}
            cams = extra.get("cameras")
            if cams is not None:
                assert c2w is None and fovy is None and timestamps is None
                c2w, fovy, timestamps, height, width = cams.c2w, cams.fovy, cams.timestamps, cams.height, cams.width
            B = c2w.shape[0]
            log.append(dict(c2w=c2w.clone(), fovy=fovy.clone(), timestamps=timestamps.reshape(-1).clone(), size=(int(height), int(width)),
                            do_guidance=do_guidance, drawn=torch.rand(B, 3, generator=generator, device="cuda"), batch=cams is not None))
            image = (torch.rand(B, 3, height, width, generator=generator, device="cuda") * 1.4 - 0.2).requires_grad_(True)
            alpha = torch.rand(B, 1, height, width, generator=generator, device="cuda").requires_grad_(True)
            return stage4d.RenderOutput(image=image, alpha=alpha, comp_depth=alpha.permute(0, 2, 3, 1), means3D=None, scales=None)
        return render

    def fixed_signature(field_, gaussians, c2w, fovy, timestamps, height, width, bg, *, do_guidance, first_frame_trainable, keep_prob, generator):
        return recording(fixed_log)(field_, gaussians, c2w, fovy, timestamps, height, width, bg, do_guidance=do_guidance,
                                    first_frame_trainable=first_frame_trainable, keep_prob=keep_prob, generator=generator)
    a_log, b_log, fixed_log = [], [], []
    gen_a, gen_b, gen_c = (torch.Generator(device="cuda").manual_seed(17) for _ in range(3))
    out_a = stage4d.training_step(field, g, with_batches, generator=gen_a, render=recording(a_log), **kw)
    out_b = stage4d.training_step(field, g, with_tensors, generator=gen_b, render=recording(b_log), **kw)
    stage4d.training_step(field, g, with_tensors, generator=gen_c, render=fixed_signature, **kw)      # cameras= is passed only with a batch
    assert len(a_log) == len(b_log) == len(fixed_log) == 2 and [c["batch"] for c in a_log + b_log] == [True, True, False, False]
    frames = stage4d.sampled_frames(step, n_frame, 10, do_guidance=True)
    assert a_log[0]["c2w"].shape[0] == n_view * len(frames) and a_log[1]["c2w"].shape[0] == S
    for a, b in zip(a_log, b_log):
        for key in ("c2w", "fovy", "timestamps", "drawn"):
            assert torch.equal(a[key], b[key]), key
        assert a["size"] == b["size"] == (side, side) and a["do_guidance"] is b["do_guidance"] is True
    assert torch.equal(gen_a.get_state(), gen_b.get_state()) and torch.equal(gen_a.get_state(), gen_c.get_state())
    assert set(out_a) == set(out_b) and all(torch.equal(out_a[k], out_b[k]) for k in out_a)
    # the real renderer
    for p in field.parameters():
        p.grad = None
    out = stage4d.training_step(field, g, with_batches, generator=torch.Generator(device="cuda").manual_seed(17), **kw)
    out["loss"].backward()
    assert {"loss", "loss_rgb", "loss_mask", "loss_sds", "loss_tv"} <= set(out) and all(bool(torch.isfinite(v)) for v in out.values())
    for name, p in field.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        p.grad = None
    small = cameras.RandomCameraSampler(batch_size=S, n_view=n_view, total_frame=n_frame, height=1, width=8, device="cuda").sample()
    with pytest.raises(ValueError, match="total-variation"):                              # the guard reads height / width from the batch
        stage4d.training_step(field, g, dict(with_batches, random_camera=small), **kw)


# ---- the sampler

# The device generator's stream cannot be drawn on a CPU, so what was checked there, with the float64 restatement on 4096 CPU draws of
# this seed, is the statistic itself (mean sin(elevation) 1.8 standard errors below the midpoint).  A uniform variable's mean over 4096
# draws leaves 5 standard errors with probability 6e-7, and the seed fixes the outcome: the figure is printed before it is asserted.
STAT_SEED = 5


def test_sample_statistics():
    """Test 6: 4096 objects in one call, n_view 4, total_frame 1."""
    n = 4096
    cfg = dict(batch_size=4 * n, n_view=4, total_frame=1, elevation_range=(-10.0, 80.0), azimuth_range=(-180.0, 180.0),
               camera_distance_range=(1.0, 1.5), fovy_range=(40.0, 70.0), relative_radius=False, height=16, width=16)
    sampler = cameras.RandomCameraSampler(**cfg, device="cuda")
    sampler.update_step(100)

    class Coin:                                                                           # the sphere branch
        def random(self):
            return 0.75
    cb = sampler.sample(generator=torch.Generator(device="cuda").manual_seed(STAT_SEED), rng=Coin())
    elev, azim, fovy, dist = (_f64(cb[k]) for k in ("elevation", "azimuth", "fovy", "camera_distances"))
    eps = 1e-4                                                                            # one fp32 rounding at the ends of the ranges
    assert elev.min() >= -10.0 - eps and elev.max() <= 80.0 + eps and azim.min() >= -180.0 - eps and azim.max() <= 180.0 + eps
    assert fovy.min() >= np.deg2rad(40.0) - eps and fovy.max() <= np.deg2rad(70.0) + eps and dist.min() >= 1.0 - eps and dist.max() <= 1.5 + eps
    first = -180.0 + 90.0 * np.arange(4)[None]                                            # view v in quarter v: four different quarters
    assert (azim.reshape(n, 4) >= first - eps).all() and (azim.reshape(n, 4) <= first + 90.0 + eps).all()
    s = np.sin(np.deg2rad(elev.reshape(n, 4)[:, 0]))
    lo, hi = np.sin(np.deg2rad(-10.0)), np.sin(np.deg2rad(80.0))
    stderr = (hi - lo) / np.sqrt(12 * n)
    print(f"[cameras] mean sin(elevation) {s.mean():.5f}, midpoint {(lo + hi) / 2:.5f}, in standard errors {(s.mean() - (lo + hi) / 2) / stderr:.2f}")
    assert abs(s.mean() - (lo + hi) / 2) <= 5 * stderr
    assert len(np.unique(fovy)) > n // 2
    uniform = sampler.sample(generator=torch.Generator(device="cuda").manual_seed(STAT_SEED), rng=random.Random(1))   # random() = 0.134: uniform
    e = _f64(uniform["elevation"]).reshape(n, 4)[:, 0]
    assert abs(e.mean() - 35.0) <= 5 * 90.0 / np.sqrt(12 * n)


def test_reproducible_and_independent_of_total_frame():
    """Test 7."""
    a = _sampler().sample(generator=torch.Generator(device="cuda").manual_seed(9), rng=random.Random(4))
    b = _sampler().sample(generator=torch.Generator(device="cuda").manual_seed(9), rng=random.Random(4))
    for name in ("c2w", "fovy", "w2c", "full_proj", "campos", "tanfov", "elevation", "azimuth", "camera_distances", "timestamps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.frame_ids == b.frame_ids
    c = _sampler(total_frame=5, batch_size=20).sample(generator=torch.Generator(device="cuda").manual_seed(9), rng=random.Random(4))
    assert c.c2w.shape[0] == 20 and a.c2w.shape[0] == 12
    for name in ("elevation", "fovy", "camera_distances"):                                # per object: R = 2 in both
        assert torch.equal(getattr(a, name).reshape(2, -1)[:, 0], getattr(c, name).reshape(2, -1)[:, 0]), name
    assert torch.equal(a.azimuth.reshape(4, 3)[:, 0], c.azimuth.reshape(4, 5)[:, 0])      # per (object, view)
