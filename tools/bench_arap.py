#!/usr/bin/env python
"""Time the ARAP kernels at the 4D-SDS shape with HIP events: the exact k-NN search at Nv points for K = 3 and K = 10, and the energy
forward and forward + backward at F frames, S samples, K = 3.  Beside each, on the same GPU and in the same process, the reference's
pattern restated in torch (not the code under test): a chunked ``cdist`` + ``topk`` of K + 1 (what knn_points stands for, run every step),
and the per-frame loop of tests/arap_ref.energy with ``torch.linalg.svd``, fp32, with autograd.

    python tools/bench_arap.py [--n 100000] [--iters 10]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import arap
from tests import arap_ref
from tools._timing import timed


def torch_knn(x, K, chunk=4096):
    idx = []
    for b in range(0, x.shape[0], chunk):
        d = torch.cdist(x[b:b + chunk], x)
        idx.append(torch.topk(d, K + 1, dim=1, largest=False).indices[:, 1:])
    return torch.cat(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--samples", type=int, default=512)
    a = ap.parse_args()
    N, F, S = a.n, a.frames, a.samples
    g = torch.Generator().manual_seed(0)
    xyz = ((torch.rand(N, 3, generator=g) - 0.5)).cuda()
    res = {"Nv": N, "frames": F, "samples": S, "device": torch.cuda.get_device_name(0)}
    for K in (3, 10):
        res[f"knn_K{K}_ms"] = round(timed(lambda: arap.knn_graph(xyz, K, radius=0.01), a.iters), 3)
        res[f"torch_cdist_topk_K{K}_ms"] = round(timed(lambda: torch_knn(xyz, K), max(3, a.iters // 3)), 3)
    nn_idx, _ = arap.knn_graph(xyz, 3, radius=0.01)
    nn64 = nn_idx.long()
    targets = torch.stack([arap_ref.deform(xyz.double(), 50 + f, amplitude=0.01).float() for f in range(F)]).requires_grad_(True)
    targets.data[0] = xyz                                            # the first frame's means are xyz
    sample_idx = torch.randint(N, (S,), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")

    def fused_fwd():
        return arap.arap_energy(xyz, targets, nn_idx, sample_idx=sample_idx)

    def fused_fb():
        torch.autograd.grad(fused_fwd(), [targets])

    def loop_fwd():
        return arap_ref.energy(xyz, targets, nn64, None, sample_idx)[0]

    def loop_fb():
        torch.autograd.grad(loop_fwd(), [targets])

    t_f, t_fb = timed(fused_fwd, a.iters), timed(fused_fb, a.iters)
    l_f, l_fb = timed(loop_fwd, max(3, a.iters // 3)), timed(loop_fb, max(3, a.iters // 3))
    res.update({"energy_forward_ms": round(t_f, 3), "energy_fwd_bwd_ms": round(t_fb, 3), "energy_backward_ms": round(t_fb - t_f, 3),
                "torch_loop_forward_ms": round(l_f, 3), "torch_loop_fwd_bwd_ms": round(l_fb, 3),
                "loss_fused": float(fused_fwd().detach()), "loss_torch_loop_fp32": float(loop_fwd().detach())})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
