"""animate3d_amd.guidance on the host: the timestep range against what the reference's own ``update_step`` / ``set_min_max_steps`` left
behind (tests/golden/guidance.json, written by tests/golden/make_guidance_goldens.py), the conditions a call assembles (text embeddings,
the frame-0 values handed to ``prompt_utils``, the camera the UNet receives, the order of the random draws), the refusals, and the way
``stage4d.training_step`` / ``fit`` hand this step's cameras to a guidance object.  No GPU: the call runs with ``fused=False`` on CPU
tensors over stand-ins (tests/sds_stub.py's UNet, an identity-like VAE), the step over a stand-in ``render`` and reconstruction loss."""
import json
import os
import random
from types import SimpleNamespace

import pytest
import torch

from animate3d_amd import cameras, sds, stage4d
from animate3d_amd.guidance import AnimateMVGuidance
from tests.sds_stub import stub_unet

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guidance.json")))


# ---- the timestep range

def test_update_step_matches_the_reference():
    assert len(GOLD["update_step"]) >= 60
    for case in GOLD["update_step"]:
        g = AnimateMVGuidance(None, None, min_step_percent=case["min_step_percent"], max_step_percent=case["max_step_percent"],
                              sqrt_anneal=case["sqrt_anneal"], trainer_max_steps=case["trainer_max_steps"],
                              num_train_timesteps=GOLD["num_train_timesteps"])
        assert (g.min_step, g.max_step) == (GOLD["defaults"]["min_step"], GOLD["defaults"]["max_step"])     # until the first update_step
        g.update_step(case["epoch"], case["step"])
        assert type(g.min_step) is int and type(g.max_step) is int
        assert (g.min_step, g.max_step) == (case["min_step"], case["max_step"]), case
    # the list schedule moves, and int() truncates its interpolated values
    moved = {c["step"]: c["min_step"] for c in GOLD["update_step"]
             if c["min_step_percent"] == [0, 0.98, 0.02, 10000] and c["max_step_percent"] == 0.98 and not c["sqrt_anneal"]}
    assert moved[0] == 980 and moved[10000] == moved[20000] == 20 and moved[0] > moved[1] >= moved[5000] > moved[9999] >= 20


def test_set_min_max_steps_matches_the_reference():
    g = AnimateMVGuidance(None, None, num_train_timesteps=GOLD["num_train_timesteps"])
    for case in GOLD["set_min_max_steps"]:
        g.set_min_max_steps(case["min_step_percent"], case["max_step_percent"])
        assert (g.min_step, g.max_step) == (case["min_step"], case["max_step"]), case
    g.set_min_max_steps()
    assert (g.min_step, g.max_step) == (GOLD["defaults"]["min_step"], GOLD["defaults"]["max_step"])


# ---- what a call assembles

class IdentityVAE:
    """``encode_images`` stand-in: 4 channels out of the 3 colours at 1/8 size, plus posterior noise from ``generator``."""

    def __init__(self):
        self.calls = 0

    def encode_images(self, imgs, generator=None, noise=None):
        self.calls += 1
        z = torch.nn.functional.avg_pool2d(torch.cat([imgs, imgs[:, :1]], dim=1), 8)
        return z + 0.1 * torch.randn(z.shape, generator=generator)


class RecordingPrompts:
    def __init__(self, L=5, D=16):
        self.calls, self.L, self.D = [], L, D

    def get_text_embeddings(self, elevation, azimuth, camera_distances, view_dependent_prompting):
        self.calls.append((elevation.clone(), azimuth.clone(), camera_distances.clone(), view_dependent_prompting))
        rows = elevation.shape[0]
        text = elevation.reshape(rows, 1, 1).expand(rows, self.L, self.D) * 0.01
        return torch.cat([text, -torch.ones(rows, self.L, self.D)])


def _camera_fields(b, n, f, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = b * n * f
    c2w = torch.eye(4).repeat(B, 1, 1)
    c2w[:, :3, :] += 0.3 * torch.randn(B, 3, 4, generator=g)
    return dict(elevation=torch.arange(B, dtype=torch.float32), azimuth=100.0 + torch.arange(B, dtype=torch.float32),
                camera_distances=200.0 + torch.arange(B, dtype=torch.float32), c2w=c2w, fovy=torch.full((B,), 0.7), height=64, width=64,
                timestamps=torch.zeros(B, 1))


def test_call_assembles_the_reference_conditions():
    b, n, f = 2, 2, 3
    seen = {}

    def unet(sample, timestep, **kw):
        seen.update(sample=sample, t=timestep, camera=kw["camera"], text=kw["encoder_hidden_states"],
                    image_embeds=kw["added_cond_kwargs"]["image_embeds"], tz=kw["i2v_cond_time_zero"])
        return stub_unet(sample, timestep, **kw)

    vae, prompts = IdentityVAE(), RecordingPrompts()
    g = AnimateMVGuidance(vae, unet, n_view=n, n_frame=f, guidance_scale=5.0, recon_std_rescale=0.25, min_step_percent=0.02,
                          max_step_percent=0.2, half_precision_weights=False, image_size=64, fused=False)
    g.update_step(0, 0)
    cam = _camera_fields(b, n, f)
    rgb = torch.rand(b * n * f, 16, 16, 3, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    emb = torch.randn(b * n, 12, generator=torch.Generator().manual_seed(2))
    out = g(rgb, prompts, **cam, rgb_as_latents=False, generator=torch.Generator().manual_seed(7), image_embeds=emb)
    assert set(out) == {"loss_sds", "min_step", "max_step"} and (out["min_step"], out["max_step"]) == (20, 200)
    assert torch.isfinite(out["loss_sds"]) and out["loss_sds"].requires_grad
    out["loss_sds"].backward()
    grad = rgb.grad.reshape(b * n, f, -1)
    assert float(grad[:, 0].abs().max()) == 0.0 and float(grad[:, 1:].abs().max()) > 0.0
    # prompt_utils got the frame-0 values per (b, view), in that order, and the config's view_dependent_prompting
    first = torch.arange(b * n) * f
    (elev, azim, dist, vdp), = prompts.calls
    assert torch.equal(elev, cam["elevation"][first]) and torch.equal(azim, cam["azimuth"][first])
    assert torch.equal(dist, cam["camera_distances"][first]) and vdp is False
    assert torch.equal(seen["text"], prompts.get_text_embeddings(elev, azim, dist, False))
    # the UNet's camera: normalize_camera of frame 0's c2w per (b, view), for both CFG halves
    want = sds.normalize_camera(cam["c2w"][first])
    assert torch.equal(seen["camera"], torch.cat([want, want]))
    assert torch.equal(seen["image_embeds"], torch.cat([emb, torch.zeros_like(emb)])) and seen["tz"] is False
    assert seen["sample"].shape == (2 * b * n, 4, f, 8, 8) and seen["sample"].dtype == torch.float32
    # the draws, in the reference's order from one generator: posterior noise, t, diffusion noise
    gen = torch.Generator().manual_seed(7)
    torch.randn(b * n * f, 4, 8, 8, generator=gen)
    t = torch.randint(20, 201, [b], dtype=torch.long, generator=gen)
    assert torch.equal(seen["t"].long(), torch.cat([t.repeat_interleave(n)] * 2))
    noise = torch.randn(b, n, f - 1, 4, 8, 8, generator=gen)
    a = g.alphas_cumprod[t].reshape(b, 1, 1, 1, 1, 1)
    lat = seen["sample"][:b * n].reshape(b, n, 4, f, 8, 8).permute(0, 1, 3, 2, 4, 5)
    torch.testing.assert_close(lat[:, :, 1:], a.sqrt() * _latents_of(rgb, gen_seed=7).reshape(b, n, f, 4, 8, 8)[:, :, 1:] + (1 - a).sqrt() * noise,
                               rtol=1e-6, atol=1e-6)
    # the same seed gives the same bits
    again = g(rgb.detach(), prompts, **cam, generator=torch.Generator().manual_seed(7), image_embeds=emb)
    assert torch.equal(again["loss_sds"], out["loss_sds"].detach())


def _latents_of(rgb, gen_seed):
    x = torch.nn.functional.interpolate(rgb.detach().permute(0, 3, 1, 2), (64, 64), mode="bilinear", align_corners=False)
    return IdentityVAE().encode_images(x, generator=torch.Generator().manual_seed(gen_seed))


def test_text_pair_expansion_and_camera_batch_fields():
    """Without ``prompt_utils`` the pair given at construction is expanded to (text for every (b, view), then uncond); a
    ``cameras.CameraBatch`` unpacks into the call as ``**batch["random_camera"]`` does in the reference."""
    b, n, f = 2, 3, 2
    text, uncond = torch.full((5, 16), 2.0), torch.full((1, 5, 16), -3.0)
    g = AnimateMVGuidance(IdentityVAE(), stub_unet, text_embeddings=(text, uncond), n_view=n, n_frame=f, half_precision_weights=False,
                          image_size=64, fused=False)
    e = g.get_text_embeddings(None, None, None, None, b)
    assert e.shape == (2 * b * n, 5, 16) and bool((e[:b * n] == 2.0).all()) and bool((e[b * n:] == -3.0).all())
    with pytest.raises(ValueError):
        AnimateMVGuidance(IdentityVAE(), stub_unet, n_view=n, n_frame=f).get_text_embeddings(None, None, None, None, b)
    fields = _camera_fields(b, n, f)
    B = b * n * f
    z = torch.zeros(B, 4, 4)
    cb = cameras.CameraBatch(c2w=fields["c2w"], fovy=fields["fovy"], w2c=z, full_proj=z, campos=torch.zeros(B, 3), tanfov=torch.zeros(B),
                             height=64, width=64, frame_ids=tuple(i % f for i in range(B)), frame_times=tuple(float(i) for i in range(f)),
                             elevation=fields["elevation"], azimuth=fields["azimuth"], camera_distances=fields["camera_distances"])
    rgb = torch.rand(B, 16, 16, 3, generator=torch.Generator().manual_seed(1))
    emb = torch.zeros(b * n, 12)
    a = g(rgb, None, **cb, rgb_as_latents=False, generator=torch.Generator().manual_seed(3), image_embeds=emb)
    want = g(rgb, None, **fields, rgb_as_latents=False, generator=torch.Generator().manual_seed(3), image_embeds=emb)
    assert torch.isfinite(a["loss_sds"]) and torch.equal(a["loss_sds"], want["loss_sds"])


def test_refusals():
    for bad in (dict(camera_condition_type="extrinsics"), dict(grad_clip=[0, 2.0, 8.0, 1000]), dict(token_merging=True),
                dict(guidance_eval=True), dict(recon_loss=False)):
        with pytest.raises(NotImplementedError):
            AnimateMVGuidance(None, None, **bad)
    vae = IdentityVAE()
    g = AnimateMVGuidance(vae, stub_unet, text_embeddings=(torch.zeros(5, 16), torch.zeros(5, 16)), n_view=2, n_frame=2,
                          half_precision_weights=False, image_size=64, fused=False)
    cam = _camera_fields(1, 2, 2)
    rgb, emb = torch.rand(4, 16, 16, 3), torch.zeros(2, 12)
    with pytest.raises(NotImplementedError):
        g(rgb, None, **cam, guidance_eval=True, image_embeds=emb)
    g.min_step, g.max_step = 300, 200
    with pytest.raises(ValueError, match="min_step"):
        g(rgb, None, **cam, image_embeds=emb)
    assert vae.calls == 0                                        # before anything is launched
    g.set_min_max_steps()
    with pytest.raises(ValueError):
        g(rgb, None, **cam)                                      # neither image_embeds nor an image encoder
    with pytest.raises(ValueError):
        g(rgb[:3], None, **cam, image_embeds=emb)
    assert vae.calls == 0
    # the fused path has no torch fallback: CPU tensors raise
    g.fused = True
    with pytest.raises(RuntimeError, match="CUDA"):
        g(rgb, None, **cam, image_embeds=emb)
    lat = torch.zeros(4, 4, 8, 8)
    with pytest.raises(RuntimeError, match="CUDA"):
        sds.sds_recon_loss_fused(stub_unet, lat, torch.tensor([5]), torch.zeros(4, 5, 16), emb, n_view=2, n_frame=2)


# ---- the step hands this step's cameras to the guidance object

N_VIEW, N_FRAME, SIDE = 2, 3, 4


class RecordingGuidance:
    takes_batch = True

    def __init__(self):
        self.calls, self.updates = [], []

    def update_step(self, epoch, global_step):
        self.updates.append((epoch, global_step, len(self.calls)))

    def __call__(self, rgb, prompt_utils=None, **kw):
        self.calls.append(dict(rgb=rgb, prompt_utils=prompt_utils, **kw))
        return {"loss_sds": (rgb ** 2).mean(), "min_step": 20, "max_step": 200}


@pytest.fixture
def step(monkeypatch):
    """``training_step``'s arguments over stand-ins: a ``render`` whose image is one parameter broadcast, and a reconstruction loss in
    torch ops (the kernel's needs a GPU)."""
    weight = torch.nn.Parameter(torch.tensor(0.5))

    def render(field, gs, c2w, fovy, timestamps, height, width, bg, *, cameras=None, **kw):
        B = cameras.c2w.shape[0] if cameras is not None else c2w.shape[0]
        image = weight * torch.ones(B, 3, int(height), int(width))
        return stage4d.RenderOutput(image=image, alpha=image[:, :1], means3D=torch.zeros(B, 1, 3))

    def recon(image, alpha, rgb, mask, index, *, bg, lambda_rgb, lambda_mask):
        value = lambda_rgb * (image ** 2).mean() + lambda_mask * (alpha ** 2).mean()
        return value, value.detach(), value.detach()

    monkeypatch.setattr(stage4d, "masked_recon_loss", recon)
    S = N_VIEW * N_FRAME
    batch = dict(rgb=torch.zeros(S, SIDE, SIDE, 3), mask=torch.ones(S, SIDE, SIDE, 1, dtype=torch.bool), c2w=torch.eye(4).repeat(S, 1, 1),
                 fovy=torch.full((S,), 0.7), timestamps=torch.zeros(S), prompt_utils="the prompts")
    kw = dict(loss=dict(lambda_rgb=1.0, lambda_mask=1.0, lambda_sds=0.5), n_view=N_VIEW, n_frame=N_FRAME, progressive_iter_per_frame=10,
              bg=(1.0, 1.0, 1.0), render=render)
    return SimpleNamespace(weight=weight, batch=batch, kw=kw, gaussians=SimpleNamespace(xyz=torch.zeros(5, 3)))


def _random_camera(seed, as_batch):
    fields = _camera_fields(1, N_VIEW, N_FRAME, seed=seed)
    fields.update(height=SIDE, width=SIDE)
    if not as_batch:
        return fields
    B = N_VIEW * N_FRAME
    z = torch.zeros(B, 4, 4)
    return cameras.CameraBatch(c2w=fields["c2w"], fovy=fields["fovy"], w2c=z, full_proj=z, campos=torch.zeros(B, 3), tanfov=torch.zeros(B),
                               height=SIDE, width=SIDE, frame_ids=tuple(i % N_FRAME for i in range(B)),
                               frame_times=tuple(float(i) for i in range(N_FRAME)), elevation=fields["elevation"],
                               azimuth=fields["azimuth"], camera_distances=fields["camera_distances"])


@pytest.mark.parametrize("as_batch", [False, True])
def test_training_step_hands_the_guidance_this_steps_cameras(step, as_batch):
    cam = _random_camera(4, as_batch)
    guidance, gen = RecordingGuidance(), torch.Generator().manual_seed(0)
    out = stage4d.training_step(None, step.gaussians, dict(step.batch, random_camera=cam), global_step=3, guidance=guidance, generator=gen,
                                **step.kw)
    (call,) = guidance.calls
    assert call["rgb"].shape == (N_VIEW * N_FRAME, SIDE, SIDE, 3) and call["prompt_utils"] == "the prompts"
    assert call["rgb_as_latents"] is False and call["generator"] is gen
    for key in ("elevation", "azimuth", "camera_distances", "c2w"):
        assert call[key] is cam[key], key                        # exactly this step's tensors
    assert set(call) - {"rgb", "prompt_utils", "rgb_as_latents", "generator"} == set(cam.keys())
    torch.testing.assert_close(out["loss_sds"], 0.5 * (step.weight.detach() ** 2), rtol=1e-6, atol=0)
    out["loss"].backward()
    assert step.weight.grad is not None and float(step.weight.grad) != 0.0


def test_a_plain_callable_still_gets_comp_rgb_alone(step):
    got = []

    def plain(*args, **kw):
        got.append((args, kw))
        return (args[0] ** 2).mean()

    out = stage4d.training_step(None, step.gaussians, dict(step.batch, random_camera=_random_camera(4, False)), global_step=0,
                                guidance=plain, **step.kw)
    ((args, kw),) = got
    assert len(args) == 1 and kw == {} and args[0].shape == (N_VIEW * N_FRAME, SIDE, SIDE, 3)
    torch.testing.assert_close(out["loss_sds"], 0.5 * (step.weight.detach() ** 2), rtol=1e-6, atol=0)


def test_fit_draws_cameras_and_updates_the_guidance_every_step(step):
    class Sampler:
        def __init__(self):
            self.steps, self.drawn = [], []

        def update_step(self, s):
            self.steps.append(s)

        def sample(self, generator, rng=random):
            self.drawn.append(_random_camera(100 + len(self.drawn), as_batch=len(self.drawn) % 2 == 1))
            return self.drawn[-1]

    guidance, sampler = RecordingGuidance(), Sampler()
    opt = torch.optim.SGD([step.weight], lr=0.1)
    logs = stage4d.fit(None, step.gaussians, step.batch, opt, steps=3, start_step=5, sampler=sampler, guidance=guidance, **step.kw)
    assert sampler.steps == [5, 6, 7] and len(guidance.calls) == 3
    assert guidance.updates == [(0, 5, 0), (0, 6, 1), (0, 7, 2)]            # update_step(0, s) before step s's call
    for call, cam in zip(guidance.calls, sampler.drawn):
        assert call["c2w"] is cam["c2w"] and call["elevation"] is cam["elevation"]
    assert not torch.equal(guidance.calls[0]["c2w"], guidance.calls[1]["c2w"]) and not torch.equal(guidance.calls[1]["c2w"], guidance.calls[2]["c2w"])
    assert logs["loss_sds"].shape == (3,) and bool(torch.isfinite(logs["loss_sds"]).all())
    assert logs["loss_sds"][2] < logs["loss_sds"][0]                        # the optimiser stepped
