#!/usr/bin/env python
"""Time the camera layer (animate3d_amd/cameras.py) on the GPU, with the contenders alternating in one process.

(a) ``RandomCameraSampler.sample()`` for 64 cameras at 256^2 (4 views x 16 frames, one object) against our own torch restatement of the
    same formulas (no rays, no lights) on the device, and against that restatement on the CPU followed by the copies to the device, which
    is the reference's pattern without its rays.  ``sample()`` also produces the rasterizer's inputs and the frame structure; what the
    tensor path pays for those in ``render_batch`` (``get_cam_info_gaussian`` and ``frames_of_images``) is timed as a row of its own.
(b) One ``stage4d.training_step`` with ``backward()`` at the shape of tools/bench_stage4d.py (100 000 Gaussians, 60 images at 256^2), the
    cameras handed over as a ``CameraBatch`` and as tensors.

Host clock around work that ends in a device synchronise: the calls are launch- and synchronisation-bound, which device events would not
show.  Per round every contender is timed once, in a fixed order; medians over the rounds, and the rounds themselves, are printed.

    python tools/bench_cameras.py [--rounds 7] [--iters 20] [--step-iters 3] [--n 100000] [--side 256]
"""
import argparse
import json
import math
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from animate3d_amd import arap, cameras, splat, stage4d
from tools import bench_stage4d as S

CFG = dict(height=256, width=256, batch_size=64, n_view=4, total_frame=16)       # refine_frame_16.yaml's random_camera sizes


def wall(fn, iters):
    """Median over ``iters`` of the host time of ``fn()`` followed by a device synchronise, in ms, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def torch_collate(s, device, generator=None, rng=random):
    """uncond_hybrid.py:195-304, 367-377, 399-406 in torch on ``device``, fp32, without rays and lights."""
    B, n_view, Fr = s.batch_size, s.n_view, s.total_frame
    R, per = B // (n_view * Fr), n_view * Fr
    rand = lambda *shape: torch.rand(*shape, generator=generator, device=device)            # noqa: E731
    er, ar = s.elevation_range, s.azimuth_range
    if rng.random() < 0.5:
        elevation_deg = (rand(R) * (er[1] - er[0]) + er[0]).repeat_interleave(per)
        elevation = elevation_deg * math.pi / 180
    else:
        lo, hi = math.sin(er[0] / 180.0 * math.pi), math.sin(er[1] / 180.0 * math.pi)
        elevation = torch.asin(rand(R) * (hi - lo) + lo).repeat_interleave(per)
        elevation_deg = elevation / math.pi * 180.0
    azimuth_deg = (rand(R).reshape(-1, 1) + torch.arange(n_view, device=device).reshape(1, -1)).reshape(-1) / n_view * (ar[1] - ar[0]) + ar[0]
    azimuth_deg = azimuth_deg.repeat_interleave(Fr)
    azimuth = azimuth_deg * math.pi / 180
    fovy = (rand(R) * (s.fovy_range[1] - s.fovy_range[0]) + s.fovy_range[0]).repeat_interleave(per) * math.pi / 180
    dist = (rand(R) * (s.camera_distance_range[1] - s.camera_distance_range[0]) + s.camera_distance_range[0]).repeat_interleave(per)
    if s.relative_radius:
        dist = dist / torch.tan(0.5 * fovy)
    fovy = fovy * (rand(R) * (s.zoom_range[1] - s.zoom_range[0]) + s.zoom_range[0]).repeat_interleave(per)
    pos = torch.stack([dist * torch.cos(elevation) * torch.cos(azimuth), dist * torch.cos(elevation) * torch.sin(azimuth),
                       dist * torch.sin(elevation)], dim=-1)
    pos = pos + rand(B, 3) * 2 * s.camera_perturb - s.camera_perturb
    center = torch.randn(B, 3, generator=generator, device=device) * s.center_perturb
    up = torch.tensor([0.0, 0.0, 1.0], device=device)[None] + torch.randn(B, 3, generator=generator, device=device) * s.up_perturb
    lookat = F.normalize(center - pos, dim=-1)
    right = F.normalize(torch.linalg.cross(lookat, up), dim=-1)
    up = F.normalize(torch.linalg.cross(right, lookat), dim=-1)
    c2w = torch.cat([torch.cat([torch.stack([right, up, -lookat], dim=-1), pos[:, :, None]], dim=-1),
                     torch.tensor([0.0, 0.0, 0.0, 1.0], device=device).expand(B, 1, 4)], dim=1)
    timestamps = torch.linspace(-1, 1, Fr, device=device).repeat(R * n_view)[:, None]
    return dict(c2w=c2w, fovy=fovy, timestamps=timestamps, elevation=elevation_deg, azimuth=azimuth_deg, camera_distances=dist,
                camera_positions=pos, height=s.height, width=s.width)


def bench_sample(rounds, iters):
    s = cameras.RandomCameraSampler(**CFG, device="cuda")
    s.update_step(100)
    gen, cpu_gen = torch.Generator(device="cuda").manual_seed(0), torch.Generator().manual_seed(0)
    batch = torch_collate(s, "cuda", gen)

    def on_cpu():
        out = torch_collate(s, "cpu", cpu_gen)
        return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}

    def tensor_path_extras():
        stage4d.frames_of_images(batch["timestamps"])
        splat.get_cam_info_gaussian(batch["c2w"], batch["fovy"], batch["fovy"], znear=0.1, zfar=100)
        torch.tan(batch["fovy"] / 2)
    contenders = (("sample_kernel", lambda: s.sample(gen)), ("torch_device", lambda: torch_collate(s, "cuda", gen)), ("torch_cpu_plus_copy", on_cpu),
                  ("tensor_path_cam_info_and_frames", tensor_path_extras))
    series = {name: [] for name, _ in contenders}
    for r in range(rounds):
        for name, fn in contenders:
            series[name].append(round(wall(fn, iters), 4))
        print(f"[sample round {r}] " + "  ".join(f"{k} {v[-1]:.4f} ms" for k, v in series.items()), flush=True)
    res = {"what": "sample, 64 cameras at 256^2", "device": torch.cuda.get_device_name(0)}
    for name, ts in series.items():
        srt = sorted(ts)
        res[name + "_ms"] = {"median": srt[len(srt) // 2], "min": srt[0], "max": srt[-1], "rounds": ts}
    return res


def bench_step(n, side, rounds, iters):
    gaussians, field, batch = S.make_scene(n, side)
    graph = arap.ArapGraph(gaussians.xyz, K=3, radius=0.01)
    cams = cameras.CameraBatch.from_c2w(batch["c2w"], batch["fovy"], batch["timestamps"].tolist(), side, side)
    with_cameras = dict(rgb=batch["rgb"], mask=batch["mask"], cameras=cams)
    gen = torch.Generator(device="cuda")

    def step(b):
        for p in field.parameters():
            p.grad = None
        out = stage4d.training_step(field, gaussians, b, loss=S.LOSS, global_step=S.STEP, n_view=S.N_VIEW, n_frame=S.N_FRAME,
                                    progressive_iter_per_frame=S.PROGRESSIVE, bg=S.BG, graph=graph, generator=gen.manual_seed(1))
        out["loss"].backward()
        return out["loss"]
    l_cam, l_ten = float(step(with_cameras).detach()), float(step(batch).detach())
    series = {"step_cameras": [], "step_tensors": []}
    for r in range(rounds):
        series["step_cameras"].append(round(wall(lambda: step(with_cameras), iters), 3))
        series["step_tensors"].append(round(wall(lambda: step(batch), iters), 3))
        print(f"[step round {r}] " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in series.items()), flush=True)
    res = {"what": f"training_step + backward, {n} Gaussians, {S.N_VIEW * (S.N_FRAME - 1)} images at {side}^2", "loss_cameras": l_cam,
           "loss_tensors": l_ten}
    for name, ts in series.items():
        srt = sorted(ts)
        res[name + "_ms"] = {"median": srt[len(srt) // 2], "min": srt[0], "max": srt[-1], "rounds": ts}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--side", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cameras.py needs the GPU: there is no CPU fallback and a CPU time would say nothing")
    print(json.dumps(bench_sample(a.rounds, a.iters)), flush=True)
    print(json.dumps(bench_step(a.n, a.side, a.rounds, a.step_iters)), flush=True)


if __name__ == "__main__":
    main()
