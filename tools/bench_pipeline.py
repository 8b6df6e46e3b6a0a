#!/usr/bin/env python
"""Time the generation pipeline's byte tail (``animate3d_amd/video.py``, ``AutoencoderKLDecoder.decode_frames_u8``) against the chain it stands
in for, and one whole ``MVVideoPipeline`` call, in one process, the variants alternating:

* the conversion alone at 64 x 512^2 (4 views x 16 frames), from fixed conv_out rows, with HIP events: ``video_to_u8`` on the 16-bit rows
  against ``unpack_out`` + the reference's torch chain on the device (``/ 2 + 0.5``, ``clamp``, ``* 255``, ``round``, ``to(uint8)``, permute);
* the whole tail from the latents to bytes on the host, by the wall clock, synchronised: ``decode_frames_u8`` + D2H against
  ``decode_latents`` + the reference's chain as it runs it (``(x / 2 + 0.5).clamp(0, 1)`` on the device, D2H of the fp32 frames, numpy
  ``(x * 255).round().astype(uint8)`` on the host), with the peak device memory of each and whether the bytes are equal;
* one whole call (prompt ids and four 512^2 images in, ``VideoFrames`` out) at a reduced step count, full-size models with synthetic weights.

    python tools/bench_pipeline.py [--rounds 5] [--iters 3] [--steps 2] [--side 512] [--frames 16] [--no-call]

Per measurement the rounds are printed one by one: their spread is what a difference between the variants has to be read against."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from animate3d_amd import clip, video
from animate3d_amd.config import UNetConfig
from animate3d_amd.pipeline import MVVideoPipeline
from animate3d_amd.unet import MVUNetMotionModel
from animate3d_amd.vae import AutoencoderKLDecoder, AutoencoderKLEncoder
from tools._timing import peak_mib, timed

N_VIEW = 4


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ts):
    s = sorted(ts)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": ts}


def reference_bytes_on_host(vid):
    """tensor2vid(video, processor, "pil") up to the bytes: per view, denormalise on the device, copy, numpy."""
    out = []
    for v in vid:
        images = (v.permute(1, 0, 2, 3) / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
        out.append((images * 255).round().astype("uint8"))
    return np.stack(out)


def bench_tail(dec, side, frames, rounds, iters):
    h = side // 8
    g = torch.Generator(device="cuda").manual_seed(0)
    latents = 0.18215 * torch.randn(N_VIEW, 4, frames, h, h, generator=g, device="cuda")
    z = latents.permute(0, 2, 1, 3, 4).reshape(N_VIEW * frames, 4, h, h)
    with torch.no_grad():
        rows, H, W = dec._decode_rows(z, 1.0 / dec.config.scaling_factor)
    ops = dec.ops
    pixels = N_VIEW * frames * H * W
    res = {"views": N_VIEW, "frames": frames, "side": side, "pixels": pixels, "storage": str(ops.act_dtype), "device": torch.cuda.get_device_name(0)}

    def conv_u8():
        return video.video_to_u8(rows, (N_VIEW, frames, H, W))

    def conv_torch():
        img = ops.unpack_out(rows, N_VIEW * frames, 4, 1, H, W, torch.float32)[:, :3, 0]
        return ((img / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    res["conversion_bytes_equal"] = bool(torch.equal(conv_u8().view(-1, H, W, 3), conv_torch()))

    def tail_u8():
        return dec.decode_frames_u8(latents).cpu().numpy()

    def tail_ref():
        return reference_bytes_on_host(dec.decode_latents(latents))

    res["tail_bytes_equal"] = bool(np.array_equal(tail_u8(), tail_ref()))
    series = {"conversion_u8": [], "conversion_torch": [], "tail_u8": [], "tail_reference": []}
    for r in range(rounds):                                          # alternating: every round times all four, in this order
        series["conversion_u8"].append(round(timed(conv_u8, iters), 4))
        series["conversion_torch"].append(round(timed(conv_torch, iters), 4))
        series["tail_u8"].append(round(min(wall_ms(tail_u8)[0] for _ in range(iters)), 2))
        series["tail_reference"].append(round(min(wall_ms(tail_ref)[0] for _ in range(iters)), 2))
        print(f"[tail round {r}] " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in series.items()), flush=True)
    for name, ts in series.items():
        res[name + "_ms"] = summary(ts)
    moved = pixels * (8 + 3)                                         # the kernel reads 8 bytes of rows and writes 3 bytes per pixel
    res["conversion_u8_GBps"] = round(moved / (res["conversion_u8_ms"]["median"] * 1e-3) / 1e9, 1)
    torch.cuda.empty_cache()
    res["peak_mib_tail_u8"], res["peak_mib_tail_reference"] = round(peak_mib(tail_u8), 1), round(peak_mib(tail_ref), 1)
    res["fp32_video_mib"] = round(pixels * 3 * 4 / 2 ** 20, 1)
    return res


def bench_call(enc, dec, side, frames, steps, rounds):
    unet = MVUNetMotionModel(UNetConfig(), num_views=N_VIEW, device="cuda").init_synthetic(seed=1).to(torch.bfloat16).eval()
    torch.manual_seed(0)
    text = clip.CLIPTextEncoder(device="cuda").to(torch.bfloat16).eval()
    vision = clip.CLIPVisionEncoderWithProjection(device="cuda").to(torch.bfloat16).eval()
    pipe = MVVideoPipeline(unet, enc, dec, text, vision)
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (N_VIEW, side, side, 3), generator=g, dtype=torch.uint8)
    ids, neg = torch.randint(1, 49000, (1, 77), generator=g), torch.randint(1, 49000, (1, 77), generator=g)

    def call(kind):
        return pipe(prompt_ids=ids, negative_prompt_ids=neg, ip_adapter_image=images, num_frames=frames, num_inference_steps=steps,
                    generator=torch.Generator().manual_seed(5), output_type=kind).frames
    call("u8")                                                       # warm-up: packs the weights, plans the resize
    series = {"call_u8": [], "call_latent": []}
    for r in range(rounds):
        series["call_u8"].append(round(wall_ms(lambda: call("u8").numpy())[0], 1))
        series["call_latent"].append(round(wall_ms(lambda: call("latent"))[0], 1))
        print(f"[call round {r}] " + "  ".join(f"{k} {v[-1]:.1f} ms" for k, v in series.items()), flush=True)
    res = {"call_steps": steps, "free_init": False, "views": N_VIEW, "frames": frames, "side": side}
    for name, ts in series.items():
        res[name + "_wall_ms"] = summary(ts)
    res["peak_mib_call_u8"] = round(peak_mib(lambda: call("u8")), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--no-call", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pipeline.py needs the GPU: there is no CPU fallback and a CPU time would say nothing")
    dec = AutoencoderKLDecoder(device="cuda").init_synthetic(seed=3).eval()
    print(json.dumps(bench_tail(dec, a.side, a.frames, a.rounds, a.iters)), flush=True)
    if not a.no_call:
        enc = AutoencoderKLEncoder(device="cuda").init_synthetic(seed=2).eval()
        torch.cuda.empty_cache()
        print(json.dumps(bench_call(enc, dec, a.side, a.frames, a.steps, max(2, a.rounds // 2))), flush=True)


if __name__ == "__main__":
    main()
