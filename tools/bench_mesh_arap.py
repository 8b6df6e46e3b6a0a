#!/usr/bin/env python
"""Time the mesh branch's per-step neighbour draw with HIP events: ``MeshGraph.sample`` (one launch of a3d_mesh_sample_neighbours) beside
the reference's pattern restated in torch on the same GPU and in the same process (not the code under test): a ``rand(Nv, Dmax)``, a masked
add, a full sort along ``Dmax`` and an advanced-index gather, on the padded ``[Nv, Dmax]`` table the reference holds.  The two alternate,
round by round.  Then each sampler followed by the ARAP energy, forward and backward, at F frames and S samples, and the peak device
memory of both samplers.

The mesh: a triangulated grid of about ``--n`` vertices (valence about 6) plus one hub row of degree ``--hub``, which sets Dmax; K = 3.

    python tools/bench_mesh_arap.py [--n 100000] [--hub 64] [--iters 20] [--rounds 5]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import arap
from tools._timing import peak_mib, timed

REPS = 20        # sampler calls per timed window: one call is a few microseconds of device work


def grid_faces(nx, ny, device):
    y, x = torch.meshgrid(torch.arange(ny - 1, device=device), torch.arange(nx - 1, device=device), indexing="ij")
    a = (y * nx + x).reshape(-1)
    return torch.cat([torch.stack([a, a + 1, a + nx + 1], 1), torch.stack([a, a + nx + 1, a + nx], 1)])


def torch_sampler(table, P, mask):
    """Uniform keys, +1000 on the padding, a sort along the row, the first P columns gathered (a -1 column picks the padded last one)."""
    N, D = table.shape
    keys = torch.rand(N, D, device=table.device)
    keys[~mask] += 1000.0
    val, index = torch.sort(keys, dim=1)
    index[val >= 1000.0] = -1
    rows = torch.arange(N, device=table.device).unsqueeze(1).expand(-1, P)
    return table[rows, index[:, :P]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--hub", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--samples", type=int, default=512)
    a = ap.parse_args()
    K, F, S = 3, a.frames, a.samples
    nx = int(math.isqrt(a.n))
    ny = (a.n + nx - 1) // nx
    Nv = nx * ny
    g = torch.Generator().manual_seed(0)
    base, mask = arap.MeshGraph.from_faces(grid_faces(nx, ny, "cuda"), Nv).padded()
    table = torch.full((Nv, a.hub), -1, dtype=torch.int64, device="cuda")
    table[:, :base.shape[1]] = base
    hub = Nv // 2 + nx // 2
    others = torch.randperm(Nv - 1, generator=g)[:a.hub]
    table[hub] = (others + (others >= hub)).cuda()                                # the hub row: `--hub` other vertices, never itself
    mask = table != -1
    graph = arap.MeshGraph.from_padded(table, mask)
    res = {"Nv": Nv, "edges": int(graph.col.shape[0]), "max_degree": graph.max_degree, "K": K, "frames": F, "samples": S,
           "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda").manual_seed(1)

    def kernel_draw():
        return graph.sample(K, generator=gen)

    def torch_draw():
        return torch_sampler(table, K, mask)

    ours, theirs = [], []
    for _ in range(a.rounds):                                                     # alternating rounds in one process
        ours.append(timed(lambda: [kernel_draw() for _ in range(REPS)], a.iters) / REPS)
        theirs.append(timed(lambda: [torch_draw() for _ in range(REPS)], a.iters) / REPS)
    res.update({"sample_ms": round(sorted(ours)[len(ours) // 2], 4), "sample_ms_rounds": [round(t, 4) for t in ours],
                "torch_pattern_ms": round(sorted(theirs)[len(theirs) // 2], 4), "torch_pattern_ms_rounds": [round(t, 4) for t in theirs]})

    xyz = (torch.rand(Nv, 3, generator=g) - 0.5).cuda()
    targets = (xyz[None] + 0.01 * torch.randn(F, Nv, 3, generator=g).cuda()).requires_grad_(True)

    def step(draw):
        loss = arap.arap_energy(xyz, targets, draw(), sample_num=S, generator=gen)
        torch.autograd.grad(loss, [targets])

    ours, theirs = [], []
    for _ in range(a.rounds):
        ours.append(timed(lambda: step(kernel_draw), a.iters))
        theirs.append(timed(lambda: step(torch_draw), a.iters))
    res.update({"sample_energy_fwd_bwd_ms": round(sorted(ours)[len(ours) // 2], 3),
                "torch_pattern_energy_fwd_bwd_ms": round(sorted(theirs)[len(theirs) // 2], 3),
                "sample_peak_mib": round(peak_mib(kernel_draw), 2), "torch_pattern_peak_mib": round(peak_mib(torch_draw), 2),
                "sample_energy_peak_mib": round(peak_mib(lambda: step(kernel_draw)), 2),
                "torch_pattern_energy_peak_mib": round(peak_mib(lambda: step(torch_draw)), 2)})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
