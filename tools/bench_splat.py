#!/usr/bin/env python
"""Time the splat rasterizer at the 4D-SDS shape: 64 images (4 views x 16 frames) at 256^2, per-image deformed means, shared scales /
rotations / opacities / degree-3 SH, for N Gaussians.  Prints one line per N: forward, backward, the stable key sort's share of the
forward, the tile instances, and the reference's pattern (64 single-image calls, forward + backward).

    python tools/bench_splat.py [--n 20000,100000,300000] [--iters 10]

The number of Gaussians in the reference's GRM .ply inputs is not known here (none is available); N spans a small to a large scene."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import splat
from tools._timing import timed


def scene(N, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    means = (torch.randn(N, 3, generator=g) * 0.6).cuda()
    offs = (torch.randn(B, 1, 3, generator=g) * 0.02).cuda()
    p = dict(means3D=(means[None] + offs).contiguous().requires_grad_(True),
             scales=torch.exp(torch.rand(N, 3, generator=g) * 2.0 - 5.0).cuda().requires_grad_(True),
             rotations=torch.randn(N, 4, generator=g).cuda().requires_grad_(True),
             opacities=torch.sigmoid(torch.randn(N, 1, generator=g)).cuda().requires_grad_(True),
             shs=(torch.randn(N, 16, 3, generator=g) * 0.3).cuda().requires_grad_(True))
    views = []
    for v in range(4):
        a = v * math.pi / 2
        eye = torch.tensor([3.0 * math.cos(a), 3.0 * math.sin(a), 0.5])
        f = -eye / eye.norm()
        r = torch.linalg.cross(f, torch.tensor([0.0, 0.0, 1.0]))
        r = r / r.norm()
        u = torch.linalg.cross(r, f)
        c2w = torch.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, u, -f, eye
        views.append(c2w)
    c2w = torch.stack(views)[:, None].expand(4, B // 4, 4, 4).reshape(B, 4, 4).cuda()
    fovy = torch.full((B,), math.radians(40.0), device="cuda")
    w2c, full, center = splat.get_cam_info_gaussian(c2w, fovy, fovy, 0.1, 100.0)
    cam = dict(viewmatrix=w2c, projmatrix=full, campos=center, tanfovx=torch.tan(fovy / 2), tanfovy=torch.tan(fovy / 2),
               image_height=256, image_width=256, bg=torch.ones(3, device="cuda"), sh_degree=3)
    return p, cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="20000,100000,300000")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--images", type=int, default=64)
    a = ap.parse_args()
    B = a.images
    for N in [int(x) for x in a.n.split(",")]:
        p, cam = scene(N, B)
        fwd = lambda: splat.rasterize_gaussians(**p, **cam)
        t_fwd = timed(lambda: [t.detach() for t in fwd()], a.iters)
        L = splat.last_instance_count()

        def fwd_bwd():
            img, _, dep, alp = fwd()
            torch.autograd.grad((img.sum() + dep.sum() * 0.01 + alp.sum()), list(p.values()))
        t_fb = timed(fwd_bwd, a.iters)
        keys = torch.randint(0, 2 ** 62, (L,), device="cuda", dtype=torch.int64)
        t_sort = timed(lambda: torch.sort(keys, stable=True), a.iters)

        def single_calls():
            for b in range(B):
                pb = dict(p, means3D=p["means3D"][b])
                cb = dict(cam, viewmatrix=cam["viewmatrix"][b:b + 1], projmatrix=cam["projmatrix"][b:b + 1], campos=cam["campos"][b:b + 1],
                          tanfovx=cam["tanfovx"][b:b + 1], tanfovy=cam["tanfovy"][b:b + 1])
                img, _, dep, alp = splat.rasterize_gaussians(**pb, **cb)
                torch.autograd.grad((img.sum() + dep.sum() * 0.01 + alp.sum()), list(pb.values()))
        t_single = timed(single_calls, max(2, a.iters // 3))
        print(json.dumps({"N": N, "images": B, "hw": 256, "instances": L, "rows_MiB": round(L * 48 / 2 ** 20, 1),
                          "forward_ms": round(t_fwd, 3), "backward_ms": round(t_fb - t_fwd, 3), "fwd_bwd_ms": round(t_fb, 3),
                          "sort_ms": round(t_sort, 3), "sort_share_of_forward": round(t_sort / t_fwd, 3),
                          "single_image_calls_fwd_bwd_ms": round(t_single, 3), "device": torch.cuda.get_device_name(0)}), flush=True)
        del p, cam
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
