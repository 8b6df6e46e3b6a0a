#!/usr/bin/env python
"""Time the CLIP image condition of one 4D-SDS step with HIP events: ``clip.encode_image_from_frames`` (the pre-processing kernel writing
the patch rows + the ViT-H/14 tower, bf16) and ``clip.preprocess_frames`` alone, against the reference's pattern on the same GPU and in the
same process (animatemv_guidance.py:546-555): the first frames to the host, ``(image * 255).astype(np.uint8)``, PIL images,
``CLIPImageProcessor``, the copy back, the same tower.  Without Pillow or transformers the pattern is timed as its two copies alone, and
the line says so.  Shapes: 4 and 8 first frames of 256^2, 4 of 512^2, each out of videos of ``--frames`` frames.

    python tools/bench_clip_preprocess.py [--iters 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from animate3d_amd import clip
from animate3d_amd.sds import first_frame_index
from tools._timing import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    try:
        import transformers
        from PIL import Image
        processor = transformers.CLIPImageProcessor()
    except Exception:                                                 # the pattern's host libraries are optional on the GPU box
        processor = None
    torch.manual_seed(0)
    enc = clip.CLIPVisionEncoderWithProjection(device="cuda").to(torch.bfloat16).eval()
    res = {"device": torch.cuda.get_device_name(0), "tower": "ViT-H/14 bf16", "frames_per_video": a.frames,
           "reference_pattern": "cpu copy + PIL + CLIPImageProcessor + copy back + tower" if processor else "copies only + tower (no Pillow / transformers)"}
    for n, side in ((4, 256), (8, 256), (4, 512)):
        rgb = torch.rand(n * a.frames, side, side, 3, device="cuda")
        first = first_frame_index(1, n, a.frames, "cuda")

        def ours():
            return clip.encode_image_from_frames(enc, rgb, first)[0]

        def pre():
            return clip.preprocess_frames(rgb, first)

        def pattern_pre():
            frames = rgb.reshape(n, a.frames, side, side, 3)[:, 0]
            host = [im.detach().cpu().numpy() for im in frames]
            if processor is None:
                px = torch.from_numpy(np.stack(host)[:, :224, :224].transpose(0, 3, 1, 2).copy())
            else:
                px = processor([Image.fromarray((im * 255).astype(np.uint8)) for im in host], return_tensors="pt").pixel_values
            return px.to(device="cuda", dtype=torch.bfloat16)

        def pattern():
            return enc(pattern_pre()).image_embeds

        tag = f"{n}x{side}"
        res[f"{tag}_preprocess_ms"] = round(timed(pre, a.iters), 4)
        res[f"{tag}_preprocess_tower_ms"] = round(timed(ours, a.iters), 3)
        res[f"{tag}_pattern_preprocess_ms"] = round(timed(pattern_pre, a.iters), 3)
        res[f"{tag}_pattern_tower_ms"] = round(timed(pattern, a.iters), 3)
        if processor is not None:
            diff = (ours().float() - pattern().float()).abs().max().item()
            res[f"{tag}_embeds_max_abs_diff"] = diff
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
