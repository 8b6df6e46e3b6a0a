"""The SDS-side glue kernels (csrc/sds_glue.hip, ``sds.sds_recon_loss_fused``) and ``guidance.AnimateMVGuidance`` on the GPU.

* Against the reference's own function: the golden of tests/test_sds.py (``compute_mvdream_recon_loss`` with tests/sds_stub.py's UNet), both
  tags, under that test's bars.
* Against float64 (tests/guidance_ref.py) at the smallest shapes at which each seam can go wrong, with fp16 and bf16 ``eps``.  The UNet
  there is a fixed, pre-drawn ``eps``: what is measured is the glue's arithmetic, not the luck of a 16-bit rounding boundary in front of a
  stand-in network.  The bar is not a constant: on the same inputs ``sds.sds_recon_loss`` (the fp32 torch chain, pinned to the reference)
  is measured against the same float64, and the fused path's maximum element-wise error per output may be at most twice that (one factor
  of two for another, equally valid rounding order).  Both figures are printed before they are compared.
* Reproducibility: two runs are bit-identical; b = 2 is two b = 1 calls bit for bit (the gradient's coefficient holds 1 / b: a power of
  two, so the rows of the b = 2 gradient times 2 are the b = 1 rows exactly).
* The object end to end on small models, and its timestep draws."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from animate3d_amd import deform4d, sds, stage4d
from animate3d_amd.denoise import ddim_schedule, randn_like_reference
from animate3d_amd.guidance import AnimateMVGuidance
from tests import guidance_ref, gs_ref
from tests.sds_stub import StubDDIM, stub_unet

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sds.npz")
OUTPUTS = ("latents_noisy", "noise_pred", "latents_recon", "loss", "grad")


def stub_unet_on_device(sample, timestep, **kw):
    with torch.device(sample.device):                            # the stub builds its constants where the default device is
        return stub_unet(sample, timestep, **kw)


# ---- the reference's own function

@pytest.mark.parametrize("tag", ["rescale", "plain"])
def test_fused_step_matches_the_reference(tag):
    golden = np.load(GOLD)
    G = {k.split("/", 1)[1]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith(tag + "/")}
    n, f, scale, rescale, tz = G["cfg"].tolist()
    seen = {}

    def unet(sample, timestep, **kw):
        seen.update(sample=sample.clone(), t=timestep.clone(), camera=kw["camera"].clone(), image_embeds=kw["added_cond_kwargs"]["image_embeds"].clone())
        return stub_unet_on_device(sample, timestep, **kw)

    dev = lambda v: v.cuda()
    lat = G["latents"].clone().cuda().requires_grad_(True)
    loss, aux = sds.sds_recon_loss_fused(unet, lat, dev(G["t"]), dev(G["text"]), dev(G["image_embeds"]), dev(G["c2w"]), n_view=int(n),
                                         n_frame=int(f), guidance_scale=scale, recon_std_rescale=rescale, i2v_cond_time_zero=bool(tz),
                                         alphas_cumprod=StubDDIM().alphas_cumprod, noise=dev(G["noise"]))
    loss.backward()
    cpu = lambda v: v.detach().cpu()
    torch.testing.assert_close(cpu(seen["sample"]), G["unet_sample"], rtol=1e-6, atol=1e-6)
    assert torch.equal(cpu(seen["t"]).long(), G["unet_t"].long())
    torch.testing.assert_close(cpu(seen["camera"]), G["unet_camera"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(cpu(seen["image_embeds"]), G["unet_image_embeds"], rtol=0, atol=0)
    torch.testing.assert_close(cpu(aux["latents_noisy"]), G["latents_noisy"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(cpu(aux["noise_pred"]), G["noise_pred"], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(cpu(aux["latents_recon"]), G["latents_recon"], rtol=1e-5, atol=2e-4)
    torch.testing.assert_close(cpu(loss), G["loss"], rtol=1e-5, atol=0)
    torch.testing.assert_close(cpu(lat.grad), G["grad"], rtol=1e-5, atol=1e-5)
    g6 = lat.grad.reshape(-1, int(f), *lat.shape[1:])
    assert float(g6[:, 0].abs().max()) == 0.0 and float(g6[:, 1:].abs().max()) > 0.0


# ---- float64, at the seams

# (b, n, f, c, h, w), t: per-b timesteps that differ, both ends of the table; one diffused frame (f = 2, f / (f - 1) = 2) and two; a
# non-square image; 5 x 7 (no multiple of any block); 16 x 16 with n = 4, f = 5: 10 blocks per b in the loss, 8 in the statistics
SHAPES = [((1, 2, 2, 4, 2, 3), [999]), ((1, 2, 3, 4, 5, 7), [0]), ((2, 2, 3, 4, 5, 7), [0, 999]), ((2, 2, 2, 4, 2, 3), [431, 20]),
          ((2, 4, 5, 4, 16, 16), [20, 700])]
TABLE = ddim_schedule(1)[1].float()


def _inputs(shape, t, dtype, seed=0):
    b, n, f, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    lat = (0.5 * torch.randn(b * n * f, c, h, w, generator=g)).cuda()
    noise = torch.randn(b, n, f - 1, c, h, w, generator=g).cuda()
    eps = torch.randn(2 * b * n, c, f, h, w, generator=g).to(dtype).cuda()
    text, emb = torch.zeros(2 * b * n, 3, 8, device="cuda"), torch.zeros(b * n, 6, device="cuda")
    return lat, noise, eps, torch.tensor(t, device="cuda"), text, emb


def _run(fn, shape, lat, noise, eps, t, text, emb, dtype, scale, rescale, table=TABLE):
    seen = {}

    def unet(sample, timestep, **kw):
        seen.update(sample=sample.clone(), t=timestep.clone())
        return SimpleNamespace(sample=eps)

    x = lat.clone().requires_grad_(True)
    # where c == f - 1 a [b, n, f - 1, c, h, w] noise has the shape of the reference's "b n c f h w" order as well, and both functions
    # read it as that: hand it over in that order, so that what they diffuse with is `noise`
    given = noise.permute(0, 1, 3, 2, 4, 5).contiguous() if shape[3] == shape[2] - 1 else noise
    loss, aux = fn(unet, x, t, text, emb, None, n_view=shape[1], n_frame=shape[2], guidance_scale=scale, recon_std_rescale=rescale,
                   alphas_cumprod=table, noise=given, weights_dtype=dtype)
    loss.backward()
    return dict(aux, loss=loss.detach(), grad=x.grad), seen


@pytest.mark.parametrize("scale,rescale", [(5.0, 0.25), (100.0, 0.25), (5.0, 0.0), (100.0, 0.0)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape,t", SHAPES, ids=["f2-2x3", "b1-5x7-t0", "b2-5x7-ends", "b2-f2", "blocks"])
def test_fused_glue_against_float64(shape, t, dtype, scale, rescale):
    b, n, f = shape[:3]
    lat, noise, eps, tt, text, emb = _inputs(shape, t, dtype)
    table = TABLE.cuda()
    want = guidance_ref.glue(lat, noise, tt, TABLE, eps, n, f, scale, rescale)
    fused, seen = _run(sds.sds_recon_loss_fused, shape, lat, noise, eps, tt, text, emb, dtype, scale, rescale, table)
    torch_path, _ = _run(sds.sds_recon_loss, shape, lat, noise, eps, tt, text, emb, dtype, scale, rescale, table)
    err = lambda got, key: float((got[key].double().cpu() - want[key]).abs().max())
    report, failed = [], []
    for key in OUTPUTS:
        e_fused, e_torch = err(fused, key), err(torch_path, key)
        report.append(f"{key} {e_fused:.3e} / {e_torch:.3e}")
        if not e_fused <= 2.0 * e_torch:
            failed.append(key)
    print(f"[parity] sds glue {tuple(shape)} t={t} {str(dtype)[6:]} s={scale} r={rescale}: fused / torch max error vs float64: " + "; ".join(report))
    # what the UNet is handed: the noisy latents in its layout, rounded once to its storage type, twice; the timestep per (half, b, view)
    half = seen["sample"].shape[0] // 2
    assert seen["sample"].dtype == dtype and torch.equal(seen["sample"][:half], seen["sample"][half:])
    ulp = 2.0 ** (-8 if dtype == torch.bfloat16 else -11)
    assert bool(((seen["sample"][:half].double().cpu() - want["sample"]).abs() <= ulp * want["sample"].abs() + 1e-6).all())
    assert torch.equal(seen["t"], torch.cat([tt.repeat_interleave(n)] * 2).to(dtype))
    # frame 0: the target is the input, bit for bit, and carries no gradient
    frame0 = lambda z: z.reshape(b * n, f, *shape[3:])[:, 0]
    assert torch.equal(frame0(fused["latents_recon"]), frame0(lat)) and torch.equal(frame0(fused["latents_noisy"]), frame0(lat))
    assert float(frame0(fused["grad"]).abs().max()) == 0.0 and float(fused["grad"].abs().max()) > 0.0
    assert not failed, failed


# ---- reproducibility

def test_bitwise_reproducible_and_batch_independent():
    shape, t = SHAPES[-1]
    b, n, f = shape[:3]
    lat, noise, eps, tt, text, emb = _inputs(shape, t, torch.float16, seed=3)
    args = (torch.float16, 100.0, 0.25, TABLE.cuda())
    first, _ = _run(sds.sds_recon_loss_fused, shape, lat, noise, eps, tt, text, emb, *args)
    second, _ = _run(sds.sds_recon_loss_fused, shape, lat, noise, eps, tt, text, emb, *args)
    for key in ("loss", "latents_recon", "grad", "latents_noisy", "noise_pred"):
        assert torch.equal(first[key], second[key]), key
    rows = n * f
    eps2 = eps.reshape(2, b, n, *eps.shape[1:])
    for i in range(b):
        one, _ = _run(sds.sds_recon_loss_fused, (1, *shape[1:]), lat[i * rows:(i + 1) * rows], noise[i:i + 1],
                      eps2[:, i].reshape(2 * n, *eps.shape[1:]).contiguous(), tt[i:i + 1], text[:2 * n], emb[:n], *args)
        assert torch.equal(one["latents_recon"], first["latents_recon"][i * rows:(i + 1) * rows])
        assert torch.equal(one["grad"], first["grad"][i * rows:(i + 1) * rows] * b)      # the coefficient holds 1 / b, b = 2: exact
    # an upstream gradient is read on the device and scales the result
    x = lat.clone().requires_grad_(True)
    loss, _ = sds.sds_recon_loss_fused(lambda s, ts, **kw: SimpleNamespace(sample=eps), x, tt, text, emb, None, n_view=n, n_frame=f,
                                       alphas_cumprod=args[3], noise=noise, weights_dtype=torch.float16)
    (loss * 4.0).backward()
    y = lat.clone().requires_grad_(True)
    sds.sds_recon_loss_fused(lambda s, ts, **kw: SimpleNamespace(sample=eps), y, tt, text, emb, None, n_view=n, n_frame=f,
                             alphas_cumprod=args[3], noise=noise, weights_dtype=torch.float16)[0].backward()
    assert torch.equal(x.grad, y.grad * 4.0)


def test_no_host_synchronisation():
    """The glue, forward and backward, and a whole call of the object (latents given, a device generator: the draws of ``t`` and of the
    noise included) under torch's synchronisation guard; the first run loads the kernels and copies the table outside of it."""
    shape, t = SHAPES[2]
    lat, noise, eps, tt, text, emb = _inputs(shape, t, torch.float16, seed=4)
    args = (torch.float16, 5.0, 0.25, TABLE.cuda())
    pair = (torch.zeros(3, 8, device="cuda"), torch.zeros(3, 8, device="cuda"))
    guidance = AnimateMVGuidance(None, lambda sample, timestep, **kw: SimpleNamespace(sample=sample), text_embeddings=pair, n_view=shape[1],
                                 n_frame=shape[2], image_size=8 * shape[4], fused=True)
    guidance.min_step, guidance.max_step = 20, 200
    rgb = torch.rand(lat.shape[0], shape[4], shape[4], 4, device="cuda")
    c2w = torch.eye(4, device="cuda").repeat(lat.shape[0], 1, 1)

    def run(seed):
        out, _ = _run(sds.sds_recon_loss_fused, shape, lat, noise, eps, tt, text, emb, *args)
        x = rgb.clone().requires_grad_(True)
        loss = guidance(x, None, c2w=c2w, rgb_as_latents=True, generator=torch.Generator(device="cuda").manual_seed(seed),
                        image_embeds=emb)["loss_sds"]
        loss.backward()
        return out["loss"], out["grad"], loss.detach(), x.grad

    first = run(1)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        second = run(1)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and float(second[3].abs().max()) > 0.0


# ---- the object

N_VIEW, N_FRAME, SIDE, N_GAUSS, LATENT = 2, 2, 64, 300, 16


@pytest.fixture(scope="module")
def models():
    from animate3d_amd.config import UNetConfig
    from animate3d_amd.unet import MVUNetMotionModel
    from animate3d_amd.vae import AutoencoderKLEncoder
    vae = AutoencoderKLEncoder(device="cuda")
    vae.init_synthetic(seed=1)
    vae = vae.half().eval()
    unet = MVUNetMotionModel(UNetConfig(block_out_channels=(320, 640), down_has_attn=(True, False), layers_per_block=1), num_views=N_VIEW,
                             device="cuda")
    unet.init_synthetic(seed=0)
    return vae, unet.half().eval()


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(12)
    xyz = (torch.randn(N_GAUSS, 3, generator=g) * 0.6).cuda()
    gaussians = stage4d.Gaussians(xyz=xyz, scaling=(torch.rand(N_GAUSS, 3, generator=g) * 1.5 - 3.0).cuda(),
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
    cams = dict(c2w=views[:, None].expand(N_VIEW, N_FRAME, 4, 4).reshape(S, 4, 4).cuda().contiguous(),
                fovy=torch.full((S,), math.radians(40.0), device="cuda"), timestamps=torch.linspace(-1, 1, N_FRAME).repeat(N_VIEW).cuda())
    batch = dict(cams, rgb=torch.rand(S, SIDE, SIDE, 3, generator=g).cuda(), mask=(torch.rand(S, SIDE, SIDE, 1, generator=g) > 0.5).cuda())
    views2 = torch.stack([gs_ref.look_at((3.0 * math.cos(a), 3.0 * math.sin(a), 0.8)) for a in (0.4, 2.0)])
    batch["random_camera"] = dict(cams, c2w=views2[:, None].expand(N_VIEW, N_FRAME, 4, 4).reshape(S, 4, 4).cuda().contiguous(), height=SIDE,
                                  width=SIDE, elevation=torch.full((S,), 15.0, device="cuda"), azimuth=torch.arange(S, device="cuda") * 20.0,
                                  camera_distances=torch.full((S,), 3.1, device="cuda"))
    return dict(gaussians=gaussians, field=field, batch=batch, bg=torch.tensor([1.0, 1.0, 1.0], device="cuda"))


def _guidance(models, seen, fused, **kw):
    vae, unet = models

    def watched(sample, timestep, **cond):
        out = unet(sample, timestep, **cond)
        seen.update(sample=sample.clone(), t=timestep.clone(), camera=cond["camera"].clone(), eps=out.sample.clone())
        return out

    g = torch.Generator().manual_seed(5)
    pair = (torch.randn(77, 768, generator=g).cuda(), torch.randn(77, 768, generator=g).cuda())
    guidance = AnimateMVGuidance(vae, watched, text_embeddings=pair, n_view=N_VIEW, n_frame=N_FRAME, guidance_scale=5.0, recon_std_rescale=0.25,
                                 min_step_percent=0.02, max_step_percent=0.2, image_size=8 * LATENT, fused=fused, **kw)
    guidance.update_step(0, 0)
    return guidance, torch.randn(N_VIEW, 1024, generator=g).cuda()


def _field_grads(field):
    out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in field.named_parameters()}
    for p in field.parameters():
        p.grad = None
    return out


def test_guidance_object_end_to_end(models, scene):
    field, gaussians, batch, bg = scene["field"], scene["gaussians"], scene["batch"], scene["bg"]
    cam = batch["random_camera"]
    seen = {}
    guidance, emb = _guidance(models, seen, fused=True)
    bound = lambda rgb, prompt_utils=None, **kw: guidance(rgb, prompt_utils, image_embeds=emb, **kw)
    bound.takes_batch = True
    kw = dict(loss=dict(lambda_rgb=1.0, lambda_mask=1.0, lambda_sds=0.01), global_step=0, n_view=N_VIEW, n_frame=N_FRAME,
              progressive_iter_per_frame=10, bg=bg, guidance=bound)

    def step(seed):
        out = stage4d.training_step(field, gaussians, batch, generator=torch.Generator(device="cuda").manual_seed(seed), **kw)
        out["loss"].backward()
        return out["loss_sds"].clone(), _field_grads(field), {k: v.clone() for k, v in seen.items()}

    loss_a, grads_a, seen_a = step(3)
    assert torch.isfinite(loss_a) and float(loss_a) > 0.0
    filled = [k for k, g in grads_a.items() if g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0]
    assert any(k.startswith("grids.") for k in filled) and any("delta_xyz" in k for k in filled), filled
    # the camera the UNet received: normalize_camera of this step's frame-0 c2w per view, for both CFG halves, in the UNet's dtype
    want = sds.normalize_camera(cam["c2w"].reshape(N_VIEW, N_FRAME, 4, 4)[:, 0]).half()
    assert torch.equal(seen_a["camera"], torch.cat([want, want]))
    assert seen_a["sample"].shape == (2 * N_VIEW, 4, N_FRAME, LATENT, LATENT) and seen_a["sample"].dtype == torch.float16
    t_a = seen_a["t"].long()
    assert bool((t_a == t_a[0]).all()) and 20 <= int(t_a[0]) <= 200
    # the same seed gives the same bits, another seed another timestep
    loss_b, grads_b, seen_b = step(3)
    assert torch.equal(loss_a, loss_b) and torch.equal(seen_a["t"], seen_b["t"]) and torch.equal(seen_a["sample"], seen_b["sample"])
    loss_c, _, seen_c = step(4)
    print(f"[guidance] loss_sds {float(loss_a):.6e} at t = {int(t_a[0])}; another seed: {float(loss_c):.6e} at t = {int(seen_c['t'][0])}")
    assert int(seen_c["t"][0]) != int(t_a[0]) and torch.isfinite(loss_c)


def test_guidance_object_fused_and_torch_paths_agree(models, scene):
    """The object on one render, ``fused=True`` against ``fused=False``, both against float64 of the same draws (replayed from the seed:
    posterior noise, t, diffusion noise) and the ``eps`` the UNet returned: the fused loss's error may be at most twice the torch path's."""
    field, gaussians, batch, bg = scene["field"], scene["gaussians"], scene["batch"], scene["bg"]
    cam = batch["random_camera"]
    with torch.no_grad():
        rgb = stage4d.render_batch(field, gaussians, cam["c2w"], cam["fovy"], cam["timestamps"], SIDE, SIDE, bg, do_guidance=True)["comp_rgb"]
    rgb = rgb.contiguous()
    results = {}
    for fused in (True, False):
        seen = {}
        guidance, emb = _guidance(models, seen, fused=fused)
        x = rgb.clone().requires_grad_(True)
        out = guidance(x, None, **cam, generator=torch.Generator(device="cuda").manual_seed(9), image_embeds=emb)
        out["loss_sds"].backward()
        results[fused] = (out["loss_sds"].detach(), x.grad, seen)
    gen = torch.Generator(device="cuda").manual_seed(9)
    imgs = torch.nn.functional.interpolate(rgb.permute(0, 3, 1, 2), (8 * LATENT, 8 * LATENT), mode="bilinear", align_corners=False)
    lat = models[0].encode_images(imgs, generator=gen)
    t = torch.randint(20, 201, [1], dtype=torch.long, generator=gen, device="cuda")
    noise = randn_like_reference((1, N_VIEW, N_FRAME - 1, 4, LATENT, LATENT), gen, "cuda", torch.float32)
    (loss_f, grad_f, seen_f), (loss_t, grad_t, seen_t) = results[True], results[False]
    assert torch.equal(seen_f["t"], seen_t["t"]) and int(seen_f["t"][0]) == int(t)
    assert torch.equal(seen_f["sample"], seen_t["sample"]) and torch.equal(seen_f["eps"], seen_t["eps"])
    want = guidance_ref.glue(lat, noise, t, ddim_schedule(1)[1].float(), seen_f["eps"], N_VIEW, N_FRAME, 5.0, 0.25)
    e_fused, e_torch = abs(float(loss_f.double()) - float(want["loss"])), abs(float(loss_t.double()) - float(want["loss"]))
    g_diff = float((grad_f - grad_t).abs().max() / grad_t.abs().max())
    print(f"[parity] guidance object, loss_sds {float(loss_f):.6e}: fused / torch error vs float64 {e_fused:.3e} / {e_torch:.3e}; "
          f"rgb.grad fused vs torch, max difference / max {g_diff:.3e}")
    assert float(grad_t.abs().max()) > 0.0 and torch.isfinite(grad_f).all()
    assert e_fused <= 2.0 * e_torch


# ---- the timestep

def test_timestep_draws_cover_the_closed_range():
    seen = []

    def unet(sample, timestep, **kw):
        seen.append(timestep[:timestep.shape[0] // 2].clone())
        return SimpleNamespace(sample=torch.zeros_like(sample))

    b, n, f = 100, 1, 2
    pair = (torch.zeros(3, 8, device="cuda"), torch.zeros(3, 8, device="cuda"))
    g = AnimateMVGuidance(None, unet, text_embeddings=pair, n_view=n, n_frame=f, image_size=32, fused=True)
    g.min_step, g.max_step = 20, 22
    rgb = torch.rand(b * n * f, 4, 4, 4, device="cuda")
    cam = dict(c2w=torch.eye(4, device="cuda").repeat(b * n * f, 1, 1))
    emb = torch.zeros(b * n, 6, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(2):
        out = g(rgb, None, **cam, rgb_as_latents=True, generator=gen, image_embeds=emb)
        assert (out["min_step"], out["max_step"]) == (20, 22)
    draws = torch.cat(seen).long().cpu()
    assert draws.numel() == 200 and int(draws.min()) >= 20 and int(draws.max()) <= 22
    assert sorted(draws.unique().tolist()) == [20, 21, 22]
    seen.clear()
    g.min_step = g.max_step = 137
    g(rgb, None, **cam, rgb_as_latents=True, generator=gen, image_embeds=emb)
    assert bool((seen[0].long() == 137).all())
