#!/usr/bin/env python
"""Time the SDS-side glue and the guidance object at BASELINE config 5 (b = 1, 4 views x 16 frames, 256^2 renders, 32 x 32 latents, fp16).

1. The glue alone: everything of ``sds.sds_recon_loss`` but the UNet call, forward and backward, the kernels of csrc/sds_glue.hip
   (``sds.sds_recon_loss_fused``) against the torch chain.  The UNet is a callable that returns a fixed fp16 ``eps``.
2. One whole ``guidance.AnimateMVGuidance`` call with ``backward()`` to the rendered pixels (resize, VAE encode, UNet, glue, the encoder's
   input gradient), ``fused=True`` against ``fused=False``, on synthetic weights; ``image_embeds`` are given (no CLIP tower in the timing).

One process, the variants alternating, every call between two HIP events after a warm-up; per variant the median with its range, and for
the glue the host's time to enqueue a call (a clock around the call, without a synchronise).

    python tools/bench_guidance.py [--calls 200] [--block 10] [--rounds 7] [--iters 3]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import sds
from animate3d_amd.denoise import ddim_schedule
from animate3d_amd.guidance import AnimateMVGuidance
from tools._timing import timed

B, N, F, C, HW, SIDE = 1, 4, 16, 4, 32, 256
SCALE, RESCALE = 5.0, 0.25                                      # refine_frame_16.yaml


def summary(ts):
    s = sorted(ts)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "calls": len(s)}


def bench_glue(calls, block):
    g = torch.Generator(device="cuda").manual_seed(0)
    lat = torch.randn(B * N * F, C, HW, HW, generator=g, device="cuda").requires_grad_(True)
    noise = torch.randn(B, N, F - 1, C, HW, HW, generator=g, device="cuda")
    eps = torch.randn(2 * B * N, C, F, HW, HW, generator=g, device="cuda").half()
    t = torch.tensor([120], device="cuda")
    text, emb = torch.zeros(2 * B * N, 77, 768, device="cuda", dtype=torch.float16), torch.zeros(B * N, 1024, device="cuda", dtype=torch.float16)
    table = ddim_schedule(1)[1].float().cuda()
    unet = lambda sample, timestep, **kw: SimpleNamespace(sample=eps)
    kw = dict(n_view=N, n_frame=F, guidance_scale=SCALE, recon_std_rescale=RESCALE, alphas_cumprod=table, noise=noise, weights_dtype=torch.float16)
    variants = {"fused": sds.sds_recon_loss_fused, "torch": sds.sds_recon_loss}

    def one(fn):
        lat.grad = None
        fn(unet, lat, t, text, emb, None, **kw)[0].backward()

    for fn in variants.values():
        for _ in range(10):
            one(fn)
    torch.cuda.synchronize()
    device_ms, host_us = {k: [] for k in variants}, {k: [] for k in variants}
    for r in range(-(-calls // block)):
        for name, fn in variants.items():                       # alternating: a block of calls of each variant per round
            for _ in range(block):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                t0 = time.perf_counter()
                one(fn)
                host_us[name].append((time.perf_counter() - t0) * 1e6)
                e.record()
                torch.cuda.synchronize()
                device_ms[name].append(s.elapsed_time(e))
        if r % 5 == 0:
            print(f"[glue round {r}] " + "  ".join(f"{k} {sorted(v[-block:])[block // 2] * 1e3:.1f} us" for k, v in device_ms.items()), flush=True)
    res = {"what": "SDS glue alone, forward + backward", "device": torch.cuda.get_device_name(0), "shape": [B, N, F, C, HW, HW], "eps": "float16"}
    for name in variants:
        res[name + "_ms"] = summary(device_ms[name])
        res[name + "_host_enqueue_us"] = summary(host_us[name])
    return res


def bench_call(rounds, iters):
    from animate3d_amd.config import UNetConfig
    from animate3d_amd.unet import MVUNetMotionModel
    from animate3d_amd.vae import AutoencoderKLEncoder
    vae = AutoencoderKLEncoder(device="cuda")
    vae.init_synthetic(seed=1)
    vae = vae.half().eval()
    unet = MVUNetMotionModel(UNetConfig(), num_views=N, device="cuda")
    unet.init_synthetic(seed=0)
    unet = unet.half().eval()
    g = torch.Generator(device="cuda").manual_seed(2)
    rgb = torch.rand(B * N * F, SIDE, SIDE, 3, generator=g, device="cuda").requires_grad_(True)
    pair = (torch.randn(77, 768, generator=g, device="cuda"), torch.randn(77, 768, generator=g, device="cuda"))
    emb = torch.randn(B * N, 1024, generator=g, device="cuda")
    c2w = torch.eye(4, device="cuda").repeat(B * N * F, 1, 1)
    c2w[:, :3, 3] = torch.randn(B * N * F, 3, generator=g, device="cuda") * 2
    made = {}
    for name, fused in (("fused", True), ("torch", False)):
        obj = AnimateMVGuidance(vae, unet, text_embeddings=pair, n_view=N, n_frame=F, guidance_scale=SCALE, recon_std_rescale=RESCALE,
                                min_step_percent=0.02, max_step_percent=0.2, fused=fused)
        obj.update_step(0, 0)
        made[name] = (obj, torch.Generator(device="cuda").manual_seed(3))

    def one(name):
        obj, gen = made[name]

        def call():
            rgb.grad = None
            obj(rgb, None, c2w=c2w, generator=gen, image_embeds=emb)["loss_sds"].backward()
        return call

    series = {k: [] for k in made}
    for r in range(rounds):
        for name in made:
            series[name].append(round(timed(one(name), iters), 3))
        print(f"[call round {r}] " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in series.items()), flush=True)
    res = {"what": "one guidance call + backward to rgb, BASELINE config 5", "renders": [B * N * F, SIDE, SIDE, 3], "dtype": "float16"}
    for name, ts in series.items():
        s = sorted(ts)
        res[name + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": ts}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance.py needs the GPU: there is no CPU fallback and a CPU time would say nothing")
    print(json.dumps(bench_glue(a.calls, a.block)), flush=True)
    torch.cuda.empty_cache()
    print(json.dumps(bench_call(a.rounds, a.iters)), flush=True)


if __name__ == "__main__":
    main()
