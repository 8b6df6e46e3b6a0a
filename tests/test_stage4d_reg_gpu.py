"""The regularisers of the 4-D stage's step on the GPU (csrc/stage_reg.hip): ``image_regularizers`` and ``gaussian_regularizers`` against the
reference's formulas in float64 (tests/stage4d_reg_ref.py), their bitwise and host-independence guarantees, ``training_step`` against the
golden the reference's own ``training_step`` and ``tv_loss`` produced (tests/golden/make_stage4d_reg_goldens.py), and one small step end
to end through the real renderer.

Bar, the project's rule (tests/test_stage4d_gpu.py): e32 is the error of torch's own fp32 evaluation of the reference formula against
float64 on the same inputs; the kernel's error, as a relative norm, must be at most max(4 e32, 2^-20).  A TV gradient is a difference of
differences, so no elementwise relative bound holds for it; where the raw render is outside [0, 1] d_image is exactly 0."""
import math
import os
import random

import numpy as np
import pytest
import torch

from animate3d_amd import arap, deform4d, stage4d
from tests import gs_ref
from tests import stage4d_ref as R
from tests import stage4d_reg_ref as G

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage4d_reg.npz")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _bar(tag, got, r32, r64, failures):
    e32, err = _rel(r32, r64), _rel(got, r64)
    bar = max(4 * e32, FLOOR)
    print(f"[stage4d_reg {tag}] e32 {e32:.3e} kernel {err:.3e} bar {bar:.3e}")
    if not err <= bar:
        failures.append((tag, e32, err, bar))


def _offset_view(t):
    """The same values in storage that starts one element (4 bytes) after a 16-byte boundary: the unaligned path."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    view = flat[1:].view(t.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _torch_reference(fn, tensors, lambdas, dtype, scale):
    """(values, gradients) of ``fn`` in ``dtype`` from the same fp32 inputs; the gradient of an operand whose weight is 0 is None."""
    leaves = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in tensors]
    out = fn(*leaves, lambdas, dtype)
    (scale * out[0]).backward()
    return [o.detach() for o in out], [None if t is None else t.grad for t in leaves]


# ---- the image terms

# 96 x 100 and 95 x 101: more pixels than one block covers (8192) and no multiple of it; the block boundary lies inside row 81, and the
# blocks hold many row boundaries; the first takes the 16-byte path, the second (odd width) the 4-byte one
IMAGE_SIZES = [(2, 2), (2, 5), (5, 2), (3, 7), (16, 16), (17, 33), (96, 100), (95, 101)]
IMAGE_LAMBDAS = (2.0, 0.5, 3.0)


def _image_inputs(B, H, W):
    image, alpha = R.make_render(f"reg/{B}x{H}x{W}", B, H, W)
    if image.numel() >= 9:
        assert all(bool(c.any()) for c in (image < 0, image > 1, image == 0, image == 1))
    return image.cuda(), G.make_depth(f"gpu/{B}x{H}x{W}", B, H, W).cuda(), alpha.cuda()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", IMAGE_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_image_terms_and_gradients_against_float64(size, B):
    H, W = size
    image, depth, alpha = _image_inputs(B, H, W)
    variants = [("all", IMAGE_LAMBDAS, False, False, 1.0), ("all/alpha3d/offset", IMAGE_LAMBDAS, True, True, 3.0)]
    for off in range(3):
        variants.append((f"zero{off}", tuple(0.0 if i == off else v for i, v in enumerate(IMAGE_LAMBDAS)), off == 1, off == 2, 1.0))
    failures = []
    for tag, lam, alpha3d, offset, scale in variants:
        ops = [image, depth, alpha.reshape(B, H, W) if alpha3d else alpha]
        if offset:
            ops = [_offset_view(t) for t in ops]
        ref_ops = [t if v else None for t, v in zip(ops, lam)]
        v64, g64 = _torch_reference(G.image_reg_ref, ref_ops, lam, torch.float64, scale)
        v32, g32 = _torch_reference(G.image_reg_ref, ref_ops, lam, torch.float32, scale)
        # an operand whose weight is 0 is a tensor of NaN: read, it would poison every sum
        leaves = [(t.clone() if v else torch.full_like(t, float("nan"))) for t, v in zip(ops, lam)]
        if offset:
            leaves = [_offset_view(t) for t in leaves]
        for t in leaves:
            t.requires_grad_(True)
        got = stage4d.image_regularizers(*leaves, lambda_tv=lam[0], lambda_depth_tv=lam[1], lambda_sparsity=lam[2])
        (scale * got[0]).backward()
        torch.cuda.synchronize()
        assert got[0].requires_grad and got[0].dim() == 0 and not any(t.requires_grad for t in got[1:])
        name = f"{B}x{H}x{W} {tag}"
        for term, g, a32, a64 in zip(("loss", "tv", "depth_tv", "sparsity"), got, v32, v64):
            _bar(f"{name} {term}", g, a32, a64, failures)
        for term, leaf, a32, a64, v in zip(("d_image", "d_depth", "d_alpha"), leaves, g32, g64, lam):
            if not v:
                assert leaf.grad is None, (name, term)
                continue
            assert leaf.grad.shape == leaf.shape
            _bar(f"{name} {term}", leaf.grad, a32, a64, failures)
        if lam[0]:
            outside = (ops[0] < 0) | (ops[0] > 1)
            assert bool((leaves[0].grad[outside] == 0).all()), name
            assert bool((leaves[0].grad[~outside] != 0).any()), name
    assert not failures, failures


# ---- the per-Gaussian terms

GAUSS_LAMBDAS = (0.7, 0.3, 0.05)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1025])           # around a block's 256 threads, and more pairs than one block's 1024
def test_gaussian_terms_and_gradients_against_float64(N, B):
    means = R.make_means(f"reg/{B}x{N}", B, N).cuda()
    zero_at = (B - 1, N // 2)
    if B * N > 1:
        means[zero_at] = 0.0                                                            # a zero-length mean
    scales_full = G.make_scales(f"gpu/{B}x{N}", B, N).cuda()
    scaling, opacity = (t.cuda() for t in G.make_static(N))
    variants = [("all/per-image", GAUSS_LAMBDAS, False, False, 1.0), ("all/shared/offset/opacity1d", GAUSS_LAMBDAS, True, True, 3.0)]
    for off in range(3):
        variants.append((f"zero{off}", tuple(0.0 if i == off else v for i, v in enumerate(GAUSS_LAMBDAS)), off == 0, False, 1.0))
    failures = []
    for tag, lam, shared, offset, scale in variants:
        lam4 = (lam[0], lam[1], lam[2], lam[2])
        base = [means, scales_full[0].contiguous() if shared else scales_full, scaling, opacity.reshape(N) if offset else opacity]
        if offset:
            base = [_offset_view(t) for t in base]
        leaves = [(t.clone() if v else torch.full_like(t, float("nan"))) for t, v in zip(base, lam4)]
        leaves = [(_offset_view(t) if offset else t).requires_grad_(True) for t in leaves]
        expand = (lambda t: t[None].expand(B, N, 3)) if shared else (lambda t: t)      # one [N, 3] counted B times
        ref_ops = [t if v else None for t, v in zip(base, lam4)]

        def ref(m, s, sg, op, lambdas, dtype):
            return G.gaussian_reg_ref(m, None if s is None else expand(s), sg, op, lambdas, dtype)
        v64, g64 = _torch_reference(ref, ref_ops, lam, torch.float64, scale)
        v32, g32 = _torch_reference(ref, ref_ops, lam, torch.float32, scale)
        got = stage4d.gaussian_regularizers(leaves[0], expand(leaves[1]), leaves[2], leaves[3], lambda_position=lam[0], lambda_scales=lam[1],
                                            lambda_opacity=lam[2])
        (scale * got[0]).backward()
        torch.cuda.synchronize()
        assert got[0].requires_grad and got[0].dim() == 0 and not any(t.requires_grad for t in got[1:])
        name = f"{B}x{N} {tag}"
        for term, g, a32, a64 in zip(("loss", "position", "scale_sum", "opacity"), got, v32, v64):
            if float(a64) == 0.0:
                assert float(g) == 0.0, (name, term)                                    # a term that is off, or the norm of one zero mean
            else:
                _bar(f"{name} {term}", g, a32, a64, failures)
        assert leaves[2].grad is None                                                   # the opacity term detaches the scales
        for term, leaf, a32, a64, v in zip(("d_means", "d_scales", "", "d_opacity"), leaves, g32, g64, lam4):
            if term == "":
                continue
            if not v:
                assert leaf.grad is None, (name, term)
            elif float(a64.abs().max()) == 0.0:
                assert float(leaf.grad.abs().max()) == 0.0, (name, term)
            else:
                assert leaf.grad.shape == leaf.shape
                _bar(f"{name} {term}", leaf.grad, a32, a64, failures)
        if lam[0] and B * N > 1:                                                        # what torch.norm's backward gives at |m| = 0
            assert bool((g64[0][zero_at] == 0).all()) and bool((g32[0][zero_at] == 0).all())
            assert bool((leaves[0].grad[zero_at] == 0).all()) and bool(torch.isfinite(leaves[0].grad).all())
    assert not failures, failures


# ---- behaviour

def _both_calls(B, H, W, N):
    image, depth, alpha = _image_inputs(B, H, W)
    means, scales = R.make_means(f"reg/det/{N}", B, N).cuda(), G.make_scales(f"gpu/det/{N}", B, N).cuda()
    scaling, opacity = (t.cuda() for t in G.make_static(N))
    inputs = (image, depth, alpha, means, scales, scaling, opacity)

    def run(grad=True):
        leaves = [t.clone().requires_grad_(grad) for t in inputs]
        img = stage4d.image_regularizers(*leaves[:3], lambda_tv=2.0, lambda_depth_tv=0.5, lambda_sparsity=3.0)
        gs = stage4d.gaussian_regularizers(*leaves[3:], lambda_position=0.7, lambda_scales=0.3, lambda_opacity=0.05)
        if not grad:
            return img, gs
        (img[0] + gs[0]).backward()
        return [t.detach().clone() for t in (*img, *gs, *(leaf.grad for i, leaf in enumerate(leaves) if i != 5))]
    return inputs, run


@pytest.mark.parametrize("shape", [(3, 96, 100, 1025), (2, 5, 7, 5)], ids=["blocks", "small"])
def test_bitwise_reproducible_no_host_sync_and_inputs_unchanged(shape):
    inputs, run = _both_calls(*shape)
    keep = [t.clone() for t in inputs]
    first = run()                                                      # also loads the library and the kernels outside the guarded region
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert len(first) == 14 and all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(torch.equal(a, b) for a, b in zip(keep, inputs))


def test_nothing_is_saved_without_a_gradient():
    inputs, run = _both_calls(2, 5, 7, 5)
    img, gs = run(grad=False)
    assert all(t.grad_fn is None and not t.requires_grad for t in (*img, *gs))
    with torch.no_grad():
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        out = stage4d.image_regularizers(*leaves[:3], lambda_tv=1.0, lambda_depth_tv=1.0, lambda_sparsity=1.0)
        out_g = stage4d.gaussian_regularizers(*leaves[3:], lambda_position=1.0, lambda_scales=1.0, lambda_opacity=1.0)
    assert out[0].grad_fn is None and out_g[0].grad_fn is None
    only_depth = inputs[1].clone().requires_grad_(True)                # a gradient for one operand only
    stage4d.image_regularizers(inputs[0], only_depth, inputs[2], lambda_tv=1.0, lambda_depth_tv=1.0, lambda_sparsity=1.0)[0].backward()
    assert only_depth.grad is not None and bool(torch.isfinite(only_depth.grad).all())


# ---- training_step against the reference's own

@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("load_guidance", [False, True])
def test_training_step_against_the_reference_golden(golden, load_guidance):
    """``training_step`` with the golden's seeded render outputs injected in place of ``render_batch``: which terms the step returns, each
    term and the total against the float64 restatement with the reference's own fp32 value as e32, and the gradients that reach the raw
    render, depth, alpha, means, scales and opacity against the reference's."""
    xyz = R.make_means("xyz", 1)[0].cuda()
    graph = arap.ArapGraph(xyz, K=3)
    cases, failures, checked = G.cases(), [], 0
    assert len(cases) == int(golden["n_cases"])
    for i, c in enumerate(cases):
        if c["guidance"] != load_guidance:
            continue
        scaling, opacity = (t.cuda().requires_grad_(True) for t in G.make_static())
        gaussians = stage4d.Gaussians(xyz, scaling, None, opacity, None, 0)
        batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in R.make_batch(c["n_view"], c["n_frame"]).items()}
        if load_guidance:
            batch["random_camera"] = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in R.make_random_camera().items()}
        calls = []

        def render(field, gs, c2w, fovy, timestamps, height, width, bg, *, do_guidance, **kwargs):
            nb = c2w.shape[0]
            key = f"{G.case_key(c)}/r{len(calls)}"
            image, alpha = R.make_render(key, nb)
            leaves = dict(image=image, alpha=alpha, depth=G.make_depth(key, nb), means=R.make_means(key, nb), scales=G.make_scales(key, nb))
            leaves = {k: v.cuda().requires_grad_(True) for k, v in leaves.items()}
            calls.append(leaves)
            return stage4d.RenderOutput(image=leaves["image"], alpha=leaves["alpha"], comp_depth=leaves["depth"].permute(0, 2, 3, 1),
                                        means3D=leaves["means"], scales=leaves["scales"])
        loss_cfg = G.case_loss(c)
        tag = G.case_key(c)
        out = stage4d.training_step(None, gaussians, batch, loss=loss_cfg, global_step=c["step"], n_view=c["n_view"], n_frame=c["n_frame"],
                                    progressive_iter_per_frame=R.PROGRESSIVE, bg=R.BG, graph=graph,
                                    guidance=R.guidance_stub if load_guidance else None, sample_strategy=c["strategy"],
                                    rng=random.Random(c["seed"]), render=render)
        out["loss"].backward()
        torch.cuda.synchronize()
        assert len(calls) == 1 + load_guidance and [int(b) for b in golden["render_b"][i] if b] == [call["image"].shape[0] for call in calls]
        want_keys = {"loss", "loss_rgb", "loss_mask"} | ({"loss_sds"} if load_guidance else set()) | ({"loss_arap"} if c["arap"] else set())
        assert set(out) == want_keys | {G.RETURNED[k] for k in c["on"]}, tag
        last = calls[-1]
        lam_i = tuple(loss_cfg[k] for k in stage4d.IMAGE_REG_LAMBDAS)
        lam_g = tuple(loss_cfg[k] for k in stage4d.GAUSSIAN_REG_LAMBDAS)
        img64 = G.image_reg_ref(last["image"].detach(), last["depth"].detach(), last["alpha"].detach(), lam_i, torch.float64)
        gs64 = G.gaussian_reg_ref(last["means"].detach(), last["scales"].detach(), scaling.detach(), opacity.detach(), lam_g, torch.float64)
        term64 = dict(zip(stage4d.IMAGE_REG_LAMBDAS + stage4d.GAUSSIAN_REG_LAMBDAS, (*img64[1:], *gs64[1:])))
        for j, name in enumerate(G.LAMBDAS):                                            # the golden's column order
            if name not in c["on"]:
                assert np.isnan(golden["logged"][i, j])
                continue
            logged = torch.tensor(float(golden["logged"][i, j])) * (1.0 if G.LOGGED[name][1] else loss_cfg[name])
            _bar(f"{tag} {G.RETURNED[name]}", out[G.RETURNED[name]], logged, loss_cfg[name] * term64[name], failures)
        # the gradients of the last render's leaves and of the opacity: the reference's own fp32 values are e32.  The first render of a
        # guidance step sees the reconstruction loss only, the means with ARAP the stub's weights: both are tests/test_stage4d_gpu.py's
        r = len(calls) - 1
        i64 = [t.detach().double().requires_grad_(True) for t in (last["image"], last["depth"], last["alpha"], last["means"], last["scales"])]
        o64 = opacity.detach().double().requires_grad_(True)
        total64 = G.image_reg_ref(*i64[:3], lam_i)[0] + G.gaussian_reg_ref(*i64[3:], scaling.detach(), o64, lam_g)[0]
        index = stage4d.sampled_image_index(stage4d.sampled_frames(c["step"], c["n_frame"], R.PROGRESSIVE, do_guidance=load_guidance),
                                            c["n_view"], c["n_frame"], "cuda").long()
        bg32 = float(torch.tensor(R.BG[0], dtype=torch.float32))

        def recon64(image, alpha):
            return R.recon_loss_ref(image, alpha, batch["rgb"], batch["mask"], index, bg32, R.LOSS["lambda_rgb"], R.LOSS["lambda_mask"])[0]
        if load_guidance:                                                               # the first render: the reconstruction loss only
            total64 = total64 + R.LOSS["lambda_sds"] * R.guidance_stub(i64[0].clamp(0, 1).permute(0, 2, 3, 1))
            full64 = total64.detach() + recon64(calls[0]["image"].detach().double(), calls[0]["alpha"].detach().double())
        else:
            total64 = total64 + recon64(i64[0], i64[2])
            full64 = total64.detach()
        total64.backward()
        for name, leaf, want in zip(("image", "depth", "alpha", "means", "scales"), (last[k] for k in ("image", "depth", "alpha", "means", "scales")),
                                    i64):
            gold = torch.from_numpy(golden[f"d_{name}"][i, r, :leaf.shape[0]])
            if name == "means" and c["arap"]:
                continue
            if want.grad is None or float(want.grad.abs().max()) == 0.0:
                assert not gold.any() and (leaf.grad is None or not bool(leaf.grad.any())), (tag, name)
                continue
            _bar(f"{tag} d_{name}", leaf.grad, gold, want.grad, failures)
        if "lambda_opacity" in c["on"]:
            _bar(f"{tag} d_opacity", opacity.grad, torch.from_numpy(golden["d_opacity"][i]), o64.grad, failures)
        else:
            assert opacity.grad is None and not golden["d_opacity"][i].any()
        assert scaling.grad is None
        if not c["arap"]:                                                               # with ARAP the golden's total holds the stub's term
            _bar(f"{tag} loss", out["loss"], torch.tensor(float(golden["returned"][i])), full64, failures)
        checked += 1
    assert checked == 14 and not failures, failures


# ---- one step through the real renderer

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


@pytest.mark.parametrize("which", ["all", "depth_tv", "position"])
def test_one_step_end_to_end_against_the_composed_pieces(scene, which):
    """The gradients of every field parameter after one ``training_step(...)["loss"].backward()`` with the regularisers on against the same
    step composed from the public pieces: the same render and reconstruction kernels, the torch restatement of the six terms applied to
    the render's outputs.  ``depth_tv`` and ``position`` switch everything else off (``lambda_rgb = lambda_mask = 0``): what reaches the
    field then came through d_depth, or through the unmasked means, alone.  e32: the composed step in fp32 against it in float64."""
    g, field, batch, bg = scene["gaussians"], scene["field"], scene["batch"], scene["bg"]
    only = {"depth_tv": "lambda_depth_tv_loss", "position": "lambda_position"}
    loss_cfg = dict(R.LOSS, lambda_arap=0.0, **G.LAMBDAS)
    if which != "all":
        loss_cfg = dict(R.LOSS, lambda_arap=0.0, lambda_rgb=0.0, lambda_mask=0.0, **{only[which]: G.LAMBDAS[only[which]]})
    step = 2 * R.PROGRESSIVE + 5                                                         # frames 1, 2, 3
    frames = stage4d.sampled_frames(step, N_FRAME, R.PROGRESSIVE, do_guidance=False)
    index = stage4d.sampled_image_index(frames, N_VIEW, N_FRAME, "cuda")
    opacity = g.opacity.clone().requires_grad_(True)
    gs = g._replace(opacity=opacity)
    for p in field.parameters():
        p.grad = None
    out = stage4d.training_step(field, gs, batch, loss=loss_cfg, global_step=step, n_view=N_VIEW, n_frame=N_FRAME,
                                progressive_iter_per_frame=R.PROGRESSIVE, bg=R.BG, generator=torch.Generator(device="cuda").manual_seed(9))
    out["loss"].backward()
    kernel, kernel_opacity = _field_grads(field), opacity.grad.clone()
    opacity.grad = None
    assert all(bool(torch.isfinite(v)) for v in out.values())
    lam_i = tuple(loss_cfg[k] for k in stage4d.IMAGE_REG_LAMBDAS)
    lam_g = tuple(loss_cfg[k] for k in stage4d.GAUSSIAN_REG_LAMBDAS)

    def composed(dtype):
        sel = index.long()
        r = stage4d.render_batch(field, gs, batch["c2w"][sel], batch["fovy"][sel], batch["timestamps"][sel], SIDE, SIDE, bg, do_guidance=False,
                                 generator=torch.Generator(device="cuda").manual_seed(9))
        total = stage4d.masked_recon_loss(r["image"], r["alpha"], batch["rgb"], batch["mask"], index, bg=float(bg[0]),
                                          lambda_rgb=loss_cfg["lambda_rgb"], lambda_mask=loss_cfg["lambda_mask"])[0]
        reg = G.gaussian_reg_ref(r["means3D"], r["scales"], gs.scaling, opacity, lam_g, dtype)[0] + \
            G.image_reg_ref(r["image"], r["comp_depth"].permute(0, 3, 1, 2), r["alpha"], lam_i, dtype)[0]
        total = total + reg.float()
        total.backward()
        grads, d_op = _field_grads(field), opacity.grad.clone()
        opacity.grad = None
        return total.detach(), grads, d_op
    l32, g32, o32 = composed(torch.float32)
    l64, g64, o64 = composed(torch.float64)
    failures = []
    _bar(f"step {which} loss", out["loss"], l32, l64, failures)
    moved = 0
    for k in kernel:
        if float(g64[k].abs().max()) == 0.0:
            assert float(kernel[k].abs().max()) == 0.0, k
            continue
        moved += 1
        _bar(f"step {which} grad {k}", kernel[k], g32[k], g64[k], failures)
    assert moved >= 10, moved                                                            # the grids and the position / rotation networks
    if float(o64.abs().max()) > 0:
        _bar(f"step {which} d_opacity", kernel_opacity, o32, o64, failures)
    assert not failures, failures
