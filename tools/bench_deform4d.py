#!/usr/bin/env python
"""Time the fused deformation field at the 4D-SDS shape: released grid sizes, 16 frames shown in 64 images (4 views), N Gaussians,
forward and forward + backward, with peak memory.  Baseline, same process and GPU: the dense torch restatement of the contract run the
way the reference runs it, one image at a time in a 64-iteration loop, fp32, with autograd (not the code under test).

    python tools/bench_deform4d.py [--n 100000] [--iters 10]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import deform4d
from tests import deform_ref
from tools._timing import peak_mib, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--raster-ms", default="6.2,11.5", help="the rasterizer's forward,backward ms for the same N and images "
                    "(profiles/bench_splat.log), quoted in the output: the other half of the render leg")
    ap.add_argument("--no-baseline", action="store_true", help="time the fused path only (for a kernel trace)")
    a = ap.parse_args()
    N, T, V = a.n, a.frames, a.views
    raster_fwd, raster_bwd = (float(v) for v in a.raster_ms.split(","))
    B = T * V
    torch.manual_seed(0)
    field = deform4d.HexPlaneDeformation(use_global_trans=True).cuda()
    with torch.no_grad():
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.normal_(0.0, 0.05)
    g = torch.Generator().manual_seed(0)
    xyz = (torch.randn(N, 3, generator=g) * 0.5).cuda()
    scaling = (torch.rand(N, 3, generator=g) * 2 - 5).cuda().requires_grad_(True)
    rotation = torch.randn(N, 4, generator=g).cuda().requires_grad_(True)
    ts = torch.linspace(-1, 1, T).cuda()
    i2t = (torch.arange(B) % T).cuda()
    cots = [torch.randn(B, N, k, generator=g).cuda() for k in (3, 3, 4)]
    leaves = [scaling, rotation] + list(field.parameters())
    grids = [list(p) for p in field.grids]
    nets = {n: getattr(field, n).weights() for n in deform_ref.LOCAL + deform_ref.GLOBAL}

    def fused_fwd():
        return field(xyz, scaling, rotation, ts, i2t)

    def fused_fb():
        outs = field(xyz, scaling, rotation, ts, i2t)
        torch.autograd.grad(outs, leaves, cots)

    def loop(backward):
        # one image per iteration, with autograd recording (the forward builds the graph), as gaussian_batch_renderer_4d.py:27-60 runs it
        total = 0.0
        for b in range(B):
            f = b % T
            outs = deform_ref.deform_frame(xyz, scaling, rotation, ts[f], grids, nets, True, True, f == 0)
            if backward:
                total = total + sum((o * c[b]).sum() for o, c in zip(outs, cots))
        if backward:
            torch.autograd.grad(total, leaves, allow_unused=True)

    t_fwd, t_fb = timed(fused_fwd, a.iters), timed(fused_fb, a.iters)
    if a.no_baseline:
        print(json.dumps({"N": N, "frames": T, "images": B, "fused_forward_ms": round(t_fwd, 3), "fused_fwd_bwd_ms": round(t_fb, 3)}), flush=True)
        return
    l_fwd, l_fb = timed(lambda: loop(False), max(3, a.iters // 3)), timed(lambda: loop(True), max(3, a.iters // 3))
    res = {"N": N, "frames": T, "images": B, "grid_size": field.grid_size, "fused_forward_ms": round(t_fwd, 3), "fused_fwd_bwd_ms": round(t_fb, 3),
           "fused_backward_ms": round(t_fb - t_fwd, 3), "torch_loop_forward_ms": round(l_fwd, 3), "torch_loop_fwd_bwd_ms": round(l_fb, 3),
           "speedup_forward": round(l_fwd / t_fwd, 2), "speedup_fwd_bwd": round(l_fb / t_fb, 2),
           "fused_peak_MiB_fwd_bwd": round(peak_mib(fused_fb), 1), "torch_loop_peak_MiB_fwd_bwd": round(peak_mib(lambda: loop(True)), 1),
           "share_of_render_leg_forward": round(t_fwd / (t_fwd + raster_fwd), 3),
           "share_of_render_leg_backward": round((t_fb - t_fwd) / (t_fb - t_fwd + raster_bwd), 3),
           "rasterizer_forward_ms_quoted": raster_fwd, "rasterizer_backward_ms_quoted": raster_bwd,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
