"""animate3d_amd.stage4d on the GPU: the loss kernel (csrc/recon_loss.hip) against the reference's formulas in float64 (tests/stage4d_ref.py),
its bitwise and host-independence guarantees, the renderer's keep-mask against the blend it replaces, ``training_step`` against the golden
the reference's own ``training_step`` produced (tests/golden/make_stage4d_goldens.py), and one small step end to end.

Bars.  Gradient of the loss kernel, derived: every element of d_image / d_alpha is within 4 * 2^-24 relative of the float64 value computed
from the same fp32 inputs (one rounding in the difference, two in the coefficient, one in the product; the compositing is an exact
select), and exactly 0 outside the clamp.  Loss values and chained gradients, the project's rule (tests/test_arap_gpu.py): e32 is the
error of torch's own fp32 evaluation of the reference formula against float64 on the same inputs, the kernel's error must be at most
max(4 e32, 2^-20) (the factor covers another summation order, the floor inputs on which torch happens to be exact)."""
import math
import os
import random

import numpy as np
import pytest
import torch

from animate3d_amd import arap, deform4d, splat, stage4d
from tests import gs_ref
from tests import stage4d_ref as R
from tests.golden.seeded import seeded_tensor

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
GRAD_BOUND = 4 * 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage4d.npz")
BG32 = float(torch.tensor(R.BG[0], dtype=torch.float32))          # the background as the kernel gets it: an fp32 number


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _loss_bar(tag, got, r32, r64, failures):
    e32, err = _rel(r32, r64), _rel(got, r64)
    bar = max(4 * e32, FLOOR)
    print(f"[stage4d {tag}] e32 {e32:.3e} kernel {err:.3e} bar {bar:.3e}")
    if not err <= bar:
        failures.append((tag, e32, err, bar))


def _grad_within_bound(got, want64, raw=None):
    """Elementwise 4 * 2^-24 relative; with ``raw`` (the unclamped render) also exactly 0 outside the clamp."""
    got, want64 = got.detach().double().cpu(), want64.detach().cpu()
    ok = bool(((got - want64).abs() <= GRAD_BOUND * want64.abs()).all())
    if raw is not None:
        outside = ((raw < 0) | (raw > 1)).cpu()
        ok = ok and bool((got[outside] == 0).all())
    worst = float(((got - want64).abs() / want64.abs().clamp_min(1e-300))[want64 != 0].max()) if bool((want64 != 0).any()) else 0.0
    return ok, worst


def _reference(image, alpha, gt, mask, index, lam, dtype, scale=1.0):
    """(loss, loss_rgb, loss_mask, d_image, d_alpha) of the reference's formulas in ``dtype`` on the device, from the same fp32 inputs."""
    i, a = image.detach().to(dtype).requires_grad_(True), alpha.detach().to(dtype).requires_grad_(True)
    idx = None if index is None else torch.as_tensor(index, device=image.device).long()
    loss, l_rgb, l_mask = R.recon_loss_ref(i, a, gt, mask, idx, BG32, lam[0], lam[1], dtype)
    (scale * loss).backward()
    return loss.detach(), l_rgb.detach(), l_mask.detach(), i.grad, a.grad.reshape(alpha.shape)


def _index_for(B):
    return {1: [5], 2: [3, 3], 3: [5, 0, 0], 4: [5, 0, 0, 3]}[B]


SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 16), (2, 33, 65), (4, 128, 160)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_against_float64(shape):
    B, H, W = shape
    S, lam = 6, (100.0, 30.0)
    image, alpha = (t.cuda() for t in R.make_render(f"gpu/{shape}", B, H, W))
    assert H * W < 3 or (bool((image < 0).any()) and bool((image > 1).any()) and bool((image == 0).any()) and bool((image == 1).any()))
    gt = (seeded_tensor(f"stage4d/gpu/{shape}/gt", (S, H, W, 3), 0.3) + 0.5).cuda()
    masks = {"false": torch.zeros(S, H, W, 1, dtype=torch.bool), "true": torch.ones(S, H, W, 1, dtype=torch.bool),
             "random": seeded_tensor(f"stage4d/gpu/{shape}/mask", (S, H, W, 1)) > 0.2}
    failures, combos = [], 0
    for mask_kind, mask in masks.items():
        for mask_dtype in (torch.bool, torch.uint8):
            for index_kind in ("identity", "list", "device"):
                m = mask.to(mask_dtype).cuda()
                if mask_dtype == torch.uint8 and mask_kind == "random":
                    m = m * 255                                       # any non-zero byte is inside
                index = None if index_kind == "identity" else _index_for(B)
                gt_i, m_i = (gt[:B], m[:B]) if index is None else (gt, m)
                if index_kind == "device":
                    index = torch.tensor(index, device="cuda", dtype=torch.int64 if mask_dtype == torch.bool else torch.int32)
                    m_i = m_i.reshape(S, H, W)                        # the mask without its channel axis
                scale = 3.0 if index_kind == "list" else 1.0          # a non-unit upstream gradient
                a_in = alpha.reshape(B, H, W) if index_kind == "list" else alpha
                r64 = _reference(image, a_in, gt_i, m_i != 0, index, lam, torch.float64, scale)
                r32 = _reference(image, a_in, gt_i, m_i != 0, index, lam, torch.float32, scale)
                img, alp = image.clone().requires_grad_(True), a_in.clone().requires_grad_(True)
                got = stage4d.masked_recon_loss(img, alp, gt_i, m_i, index, bg=BG32, lambda_rgb=lam[0], lambda_mask=lam[1])
                (scale * got[0]).backward()
                torch.cuda.synchronize()
                tag = f"{shape} mask {mask_kind}/{str(mask_dtype)[6:]} index {index_kind}"
                assert got[0].requires_grad and not got[1].requires_grad and not got[2].requires_grad and got[0].dim() == 0
                for name, g, a32, a64 in zip(("loss", "loss_rgb", "loss_mask"), got, r32, r64):
                    _loss_bar(f"{tag} {name}", g, a32, a64, failures)
                ok_i, worst_i = _grad_within_bound(img.grad, r64[3], image)
                ok_a, worst_a = _grad_within_bound(alp.grad, r64[4])
                print(f"[stage4d {tag}] d_image worst {worst_i / 2.0 ** -24:.2f} ulp, d_alpha worst {worst_a / 2.0 ** -24:.2f} ulp (bound 4)")
                if not (ok_i and ok_a):
                    failures.append((tag, "gradient", worst_i, worst_a))
                assert alp.grad.shape == a_in.shape
                combos += 1
    assert combos == 18 and not failures, failures


def test_bitwise_reproducible_no_host_sync_and_inputs_unchanged():
    for B, H, W in ((4, 128, 160), (2, 5, 7)):
        S = 6
        image, alpha = (t.cuda() for t in R.make_render(f"gpu/det/{H}", B, H, W))
        gt = (seeded_tensor(f"stage4d/gpu/det/{H}/gt", (S, H, W, 3), 0.3) + 0.5).cuda()
        mask = (seeded_tensor(f"stage4d/gpu/det/{H}/mask", (S, H, W, 1)) > 0.2).cuda()
        index = torch.tensor(_index_for(B), device="cuda", dtype=torch.int32)
        keep = [t.clone() for t in (image, alpha, gt, mask, index)]

        def run():
            img, alp = image.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
            out = stage4d.masked_recon_loss(img, alp, gt, mask, index, bg=BG32, lambda_rgb=100.0, lambda_mask=100.0)
            out[0].backward()
            return [t.detach().clone() for t in (*out, img.grad, alp.grad)]
        first = run()                                                  # also loads the library and the kernels outside the guarded region
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        try:
            torch.cuda.set_sync_debug_mode("error")
            second = run()
        finally:
            torch.cuda.set_sync_debug_mode(before)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, second))
        assert all(torch.equal(a, b) for a, b in zip(keep, (image, alpha, gt, mask, index)))


def test_nothing_is_saved_without_a_gradient_and_host_indices_are_checked():
    B, H, W, S = 2, 5, 7, 6
    image, alpha = (t.cuda() for t in R.make_render("gpu/nograd", B, H, W))
    gt = torch.rand(S, H, W, 3, device="cuda")
    mask = torch.rand(S, H, W, 1, device="cuda") > 0.5
    kw = dict(bg=BG32, lambda_rgb=1.0, lambda_mask=1.0)
    loss, _, _ = stage4d.masked_recon_loss(image, alpha, gt, mask, [0, 5], **kw)
    assert not loss.requires_grad and loss.grad_fn is None
    only_alpha = alpha.clone().requires_grad_(True)
    stage4d.masked_recon_loss(image, only_alpha, gt, mask, [0, 5], **kw)[0].backward()
    assert only_alpha.grad is not None and bool(torch.isfinite(only_alpha.grad).all())
    for bad in ([0, 6], [-1, 0], torch.tensor([0, 6])):
        with pytest.raises(IndexError):
            stage4d.masked_recon_loss(image, alpha, gt, mask, bad, **kw)
    with pytest.raises(ValueError):
        stage4d.masked_recon_loss(image, alpha, gt, mask, [0, 1, 2], **kw)
    with pytest.raises(TypeError):
        stage4d.masked_recon_loss(image, alpha, gt, mask.float(), [0, 5], **kw)


# ---- the renderer and the step on a small scene

N_VIEW, N_FRAME, SIDE, N_GAUSS = 2, 4, 32, 2000


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(12)
    xyz = (torch.randn(N_GAUSS, 3, generator=g) * 0.6).cuda()
    gaussians = stage4d.Gaussians(xyz=xyz, scaling=(torch.rand(N_GAUSS, 3, generator=g) * 2.0 - 4.2).cuda(),
                                  rotation=torch.randn(N_GAUSS, 4, generator=g).cuda(),
                                  opacity=torch.sigmoid(torch.randn(N_GAUSS, 1, generator=g) * 1.5).cuda(),
                                  shs=(torch.randn(N_GAUSS, 16, 3, generator=g) * 0.3).cuda(), sh_degree=3)
    field = deform4d.HexPlaneDeformation(use_global_trans=True)
    with torch.no_grad():                                       # the reference's zero last layers give zero gradient to everything before them
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    field = field.cuda()
    views = torch.stack([gs_ref.look_at((3.5 * math.cos(a), 3.5 * math.sin(a), 0.3)) for a in (0.0, math.pi / 2)])
    S = N_VIEW * N_FRAME
    batch = dict(c2w=views[:, None].expand(N_VIEW, N_FRAME, 4, 4).reshape(S, 4, 4).cuda().contiguous(),
                 fovy=torch.full((S,), math.radians(40.0), device="cuda"),
                 timestamps=torch.linspace(-1, 1, N_FRAME).repeat(N_VIEW).cuda(),
                 rgb=torch.rand(S, SIDE, SIDE, 3, generator=g).cuda(), mask=(torch.rand(S, SIDE, SIDE, 1, generator=g) > 0.5).cuda())
    return dict(gaussians=gaussians, field=field, batch=batch, bg=torch.tensor(R.BG, device="cuda"))


def _field_grads(field):
    out = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in field.named_parameters()}
    for p in field.parameters():
        p.grad = None
    return out


def test_render_batch_policy_and_keep_mask(scene):
    g, field, batch, bg = scene["gaussians"], scene["field"], scene["batch"], scene["bg"]
    cams = (batch["c2w"], batch["fovy"], batch["timestamps"][:, None])                 # [B, 1] timestamps, as the data module hands them over
    B = batch["c2w"].shape[0]
    frames, i2t = stage4d.frames_of_images(batch["timestamps"])
    assert frames.shape == (N_FRAME,) and i2t.tolist() == list(range(N_FRAME)) * N_VIEW
    w_img, w_alpha = torch.randn(B, 3, SIDE, SIDE, device="cuda"), torch.randn(B, 1, SIDE, SIDE, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    state = gen.get_state()
    out = stage4d.render_batch(field, g, *cams, SIDE, SIDE, bg, do_guidance=False, generator=gen)
    assert not torch.equal(gen.get_state(), state)
    with torch.no_grad():
        want = field(g.xyz, g.scaling, g.rotation, frames, i2t, deform_scales=False)
    for key, w in zip(("means3D", "scales", "rotations"), want):                      # the unmasked tensors, bit-equal to the field's output
        assert torch.equal(out[key], w) and out[key].requires_grad, key
    assert "comp_rgb" not in out.keys() and "comp_rgb" in out
    assert torch.equal(out["comp_rgb"], out["image"].clamp(0, 1).permute(0, 2, 3, 1)) and "comp_rgb" in out.keys()
    assert out["comp_mask"].shape == (B, SIDE, SIDE, 1) and out["comp_depth"].shape == (B, SIDE, SIDE, 1)
    assert torch.equal(out["visibility_filter"], out["radii"] > 0) and bool(out["visibility_filter"].any()) and out["opacities"] is g.opacity
    assert float(out["image"].detach().std()) > 0.01                                           # a picture, not the background
    ((out["image"] * w_img).sum() + (out["alpha"] * w_alpha).sum()).backward()
    fused = _field_grads(field)

    def explicit():                                                                    # the blend of advanced_4d.py:147-154 with the same mask
        keep = (torch.rand(B, N_GAUSS, 1, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda") < 0.1).float()
        means, scales, rots = field(g.xyz, g.scaling, g.rotation, frames, i2t, deform_scales=False)
        means, scales, rots = (t * keep + t.detach().clone() * (1 - keep) for t in (means, scales, rots))
        w2c, proj, cam_p = splat.get_cam_info_gaussian(batch["c2w"], batch["fovy"], batch["fovy"], znear=0.1, zfar=100)
        tan = torch.tan(batch["fovy"] / 2)
        img, _, _, alp = splat.rasterize_gaussians(means, scales, rots, g.opacity, shs=g.shs, viewmatrix=w2c, projmatrix=proj, campos=cam_p,
                                                   tanfovx=tan, tanfovy=tan, image_height=SIDE, image_width=SIDE, bg=bg, sh_degree=3)
        ((img * w_img).sum() + (alp * w_alpha).sum()).backward()
        return img.detach(), _field_grads(field), keep
    img_a, blend_a, keep = explicit()
    img_b, blend_b, _ = explicit()
    assert 0.05 < float(keep.mean()) < 0.15 and torch.equal(img_a, out["image"])
    for k in fused:
        run_to_run = float((blend_a[k] - blend_b[k]).abs().max())
        diff = float((fused[k] - blend_a[k]).abs().max())
        print(f"[stage4d keep-mask] {k}: |grad| max {float(blend_a[k].abs().max()):.3e}, against the blend {diff:.3e}, "
              f"the blend run to run {run_to_run:.3e}")
        assert float(blend_a[k].abs().max()) > 0 or k.startswith("delta_scaling_network"), k     # scales are not deformed in this step
        assert torch.equal(fused[k], blend_a[k]) if run_to_run == 0.0 else diff <= run_to_run, k
    # a guidance step: deformed scales, no mask, no draw
    gen = torch.Generator(device="cuda").manual_seed(3)
    state = gen.get_state()
    out = stage4d.render_batch(field, g, *cams, SIDE, SIDE, bg, do_guidance=True, generator=gen)
    assert torch.equal(gen.get_state(), state)
    with torch.no_grad():
        want = field(g.xyz, g.scaling, g.rotation, frames, i2t, deform_scales=True)
    assert all(torch.equal(out[key], w) for key, w in zip(("means3D", "scales", "rotations"), want))
    out["image"].sum().backward()
    full = _field_grads(field)
    assert float(full["delta_scaling_network.layers.0.weight"].abs().max()) > 0


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("load_guidance", [False, True])
def test_training_step_against_the_reference_golden(golden, load_guidance):
    """``training_step`` with the golden's seeded render outputs injected in place of ``render_batch``: the sampled index, what each render
    call is handed and its ``do_guidance``, the losses, the gradients that reach the raw render and alpha, and which means ARAP receives."""
    xyz = R.make_means("xyz", 1)[0].cuda()
    gaussians = stage4d.Gaussians(xyz, None, None, None, None, 0)
    graph = arap.ArapGraph(xyz, K=3)
    failures, numeric = [], 0
    for i, c in enumerate(R.cases()):
        if c["guidance"] != load_guidance:
            continue
        batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in R.make_batch(c["n_view"], c["n_frame"]).items()}
        if load_guidance:
            batch["random_camera"] = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in R.make_random_camera().items()}
        calls = []

        def render(field, gs, c2w, fovy, timestamps, height, width, bg, *, do_guidance, **kwargs):
            nb = c2w.shape[0]
            key = f"{R.case_key(c)}/r{len(calls)}"
            image, alpha = (t.cuda().requires_grad_(True) for t in R.make_render(key, nb))
            means = R.make_means(key, nb).cuda().requires_grad_(True)
            assert (height, width) == (R.H, R.W) and fovy.shape == timestamps.shape == (nb,)
            calls.append(dict(do_guidance=do_guidance, ids=c2w[:, 0, 3].int().tolist(), image=image, alpha=alpha, means=means))
            return stage4d.RenderOutput(image=image, alpha=alpha, means3D=means)
        tag = f"{R.case_key(c)} arap {int(c['arap'])}"
        out = stage4d.training_step(None, gaussians, batch, loss=dict(R.LOSS, lambda_arap=R.LOSS["lambda_arap"] if c["arap"] else 0.0),
                                    global_step=c["step"], n_view=c["n_view"], n_frame=c["n_frame"], progressive_iter_per_frame=R.PROGRESSIVE,
                                    bg=R.BG, graph=graph, guidance=R.guidance_stub if load_guidance else None, sample_strategy=c["strategy"],
                                    rng=random.Random(c["seed"]), render=render)
        out["loss"].backward()
        want_idx = golden["sampled_idx"][i][golden["sampled_idx"][i] >= 0].tolist()
        assert len(calls) == 1 + load_guidance and calls[0]["ids"] == want_idx, tag
        for r, call in enumerate(calls):
            want_ids = golden["render_ids"][i, r][golden["render_ids"][i, r] >= 0].tolist()
            assert call["ids"] == want_ids and int(call["do_guidance"]) == int(golden["render_flags"][i, r]), (tag, r)
            got_sel = [] if call["means"].grad is None else torch.nonzero(call["means"].grad.abs().sum((1, 2)) > 0).flatten().tolist()
            want_sel = np.nonzero(golden["arap_pos"][i, r] >= 0)[0].tolist()
            assert got_sel == want_sel, (tag, r, got_sel, want_sel)                      # the ARAP selection, exactly
        assert set(out) == {"loss", "loss_rgb", "loss_mask"} | ({"loss_sds"} if load_guidance else set()) | ({"loss_arap"} if c["arap"] else set())
        # the losses: float64 restatement on the same inputs; e32 is the reference's own fp32 result
        first, index = calls[0], torch.tensor(want_idx, device="cuda")
        lam = (R.LOSS["lambda_rgb"], R.LOSS["lambda_mask"])
        r64 = _reference(first["image"], first["alpha"], batch["rgb"], batch["mask"], index, lam, torch.float64)
        ref64 = {"loss_rgb": lam[0] * r64[1], "loss_mask": lam[1] * r64[2], "loss": r64[0]}
        if load_guidance:
            ref64["loss_sds"] = R.LOSS["lambda_sds"] * R.guidance_stub(calls[1]["image"].detach().double().clamp(0, 1).permute(0, 2, 3, 1))
            ref64["returned"] = ref64["loss"] + ref64["loss_sds"]
        names = ("loss", "loss_rgb", "loss_mask", "loss_sds", "loss_arap")
        logged = {n: torch.tensor(float(golden["losses"][i, j])) for j, n in enumerate(names)}
        for name in ("loss_rgb", "loss_mask") + (("loss_sds",) if load_guidance else ()):
            _loss_bar(f"{tag} {name}", out[name], logged[name], ref64[name], failures)
        if not c["arap"]:                                                                # with ARAP the golden's total holds the stub's term
            _loss_bar(f"{tag} loss", out["loss"], torch.tensor(float(golden["returned"][i])), ref64["returned" if load_guidance else "loss"],
                      failures)
        if golden["numeric_at"][i, 0, 0] >= 0:
            numeric += 1
            at, rows = golden["numeric_at"][i, 0]
            for name, leaf, want64, raw in (("d_image", first["image"], r64[3], first["image"].detach()), ("d_alpha", first["alpha"], r64[4], None)):
                gold = torch.from_numpy(golden[name][at:at + rows])
                ok, worst = _grad_within_bound(leaf.grad, want64, raw)
                ok_gold, worst_gold = _grad_within_bound(gold, want64, raw)
                print(f"[stage4d {tag}] {name}: kernel worst {worst / 2.0 ** -24:.2f} ulp, the reference's fp32 {worst_gold / 2.0 ** -24:.2f} ulp "
                      "of float64 (bound 4)")
                if not (ok and ok_gold):
                    failures.append((tag, name, worst, worst_gold))
            if load_guidance:                                                            # the guidance render: torch on both sides
                at, rows = golden["numeric_at"][i, 1]
                gold = torch.from_numpy(golden["d_image"][at:at + rows]).cuda()
                assert torch.allclose(calls[1]["image"].grad, gold, rtol=8 * 2.0 ** -24, atol=0), tag
                assert calls[1]["alpha"].grad is None and not golden["d_alpha"][at:at + rows].any()
    assert numeric == (9 if not load_guidance else 8) and not failures, failures


def test_one_step_end_to_end_against_the_composed_pieces(scene):
    """The gradients of every field parameter after one ``training_step(...)["loss"].backward()`` against the same step composed from the
    public pieces with torch glue (the index copies, the blend, clamp / permute, F.mse_loss).  Gradients, not parameters after Adam: with
    eps = 1e-15 the update of an element whose gradient is rounding noise is +-lr either way.  e32: the torch-glue path against the same
    path with the loss gradient computed in float64 and cast."""
    g, field, batch, bg = scene["gaussians"], scene["field"], scene["batch"], scene["bg"]
    loss_cfg = dict(R.LOSS)
    graph = arap.ArapGraph(g.xyz, K=3)
    step = 2 * R.PROGRESSIVE + 5                                                         # frames 1, 2, 3
    frames = stage4d.sampled_frames(step, N_FRAME, R.PROGRESSIVE, do_guidance=False)
    assert frames == [1, 2, 3]
    for p in field.parameters():
        p.grad = None
    out = stage4d.training_step(field, g, batch, loss=loss_cfg, global_step=step, n_view=N_VIEW, n_frame=N_FRAME,
                                progressive_iter_per_frame=R.PROGRESSIVE, bg=R.BG, graph=graph,
                                generator=torch.Generator(device="cuda").manual_seed(9))
    out["loss"].backward()
    kernel = _field_grads(field)
    assert graph.builds == 1 and all(bool(torch.isfinite(v)) for v in out.values())

    def glue(dtype):
        gen = torch.Generator(device="cuda").manual_seed(9)
        index = stage4d.sampled_image_index(frames, N_VIEW, N_FRAME, "cuda").long()
        sub = {k: v[index] for k, v in batch.items()}                                    # batch[key] = val[sampled_idx]
        ts, i2t = stage4d.frames_of_images(sub["timestamps"])
        means, scales, rots = field(g.xyz, g.scaling, g.rotation, ts, i2t, deform_scales=False)
        keep = (torch.rand(len(index), N_GAUSS, 1, generator=gen, device="cuda") < 0.1).float()
        m_in, s_in, r_in = (t * keep + t.detach().clone() * (1 - keep) for t in (means, scales, rots))
        w2c, proj, cam_p = splat.get_cam_info_gaussian(sub["c2w"], sub["fovy"], sub["fovy"], znear=0.1, zfar=100)
        tan = torch.tan(sub["fovy"] / 2)
        img, _, _, alp = splat.rasterize_gaussians(m_in, s_in, r_in, g.opacity, shs=g.shs, viewmatrix=w2c, projmatrix=proj, campos=cam_p,
                                                   tanfovx=tan, tanfovy=tan, image_height=SIDE, image_width=SIDE, bg=bg, sh_degree=3)
        total, l_rgb, l_mask = R.recon_loss_ref(img, alp, sub["rgb"], sub["mask"], None, BG32, loss_cfg["lambda_rgb"], loss_cfg["lambda_mask"],
                                                dtype)
        term = arap.arap_energy(g.xyz, means[:len(frames)], graph.refresh(g.xyz).nn_idx, sample_num=loss_cfg["arap_sample_num"], generator=gen)
        total = total.float() + loss_cfg["lambda_arap"] * term
        total.backward()
        return total.detach(), _field_grads(field)
    l32, g32 = glue(torch.float32)
    l64, g64 = glue(torch.float64)
    failures = []
    _loss_bar("step loss", out["loss"], l32, l64, failures)
    for k in kernel:
        assert float(g64[k].abs().max()) > 0 or k.startswith("delta_scaling_network"), k
        if float(g64[k].abs().max()) == 0.0:
            assert float(kernel[k].abs().max()) == 0.0, k
            continue
        _loss_bar(f"step grad {k}", kernel[k], g32[k], g64[k], failures)
    assert not failures, failures
