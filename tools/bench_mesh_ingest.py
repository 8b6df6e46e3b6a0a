#!/usr/bin/env python
"""Time the mesh ingest with HIP events: ``mesh.gaussians_from_mesh`` (``MeshGraph.from_faces``, the corner list and one launch of
a3d_mesh_vertex_gaussians_f32) beside a vectorised torch restatement of the same quantities on the same GPU and in the same process (not
the code under test): the same ``from_faces``, then gathers, ``index_add_`` for the per-vertex sums and ``F.grid_sample`` for the
texture.  The two alternate, round by round, with ``from_faces`` alone (both sides pay it) and the corner list alone (the sort behind
the kernel's fixed summation order) in the same rounds; then the peak device memory, and each side's largest error against the same
restatement in float64.

What the reference itself costs is not measured here: ``tools/mesh_animation/mesh2gaussian.py`` loops over faces and vertices in Python
with an ``.item()`` per edge, needs pytorch3d (no ROCm build), and is not part of this repository.  There is no pass/fail time: the
ingest runs once per asset.

The mesh: a textured triangulated grid of about ``--n`` vertices (valence about 6) plus one hub whose degree is raised to ``--hub`` by a
fan over far vertices, as in tools/bench_mesh_arap.py; a ``--texture`` x ``--texture`` image.

    python tools/bench_mesh_ingest.py [--n 100000] [--hub 64] [--texture 1024] [--iters 20] [--rounds 5]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from animate3d_amd import arap, mesh
from animate3d_amd.f32_stage import gather_plan
from tools._timing import peak_mib, timed
from tools.bench_mesh_arap import grid_faces

FRAME = dict(rot_x_degree=90.0, rot_z_degree=90.0, scale_factor=0.76)


def torch_ingest(verts, faces, texture, uvs, faces_uvs, R, scale_factor, shrink):
    """The outputs of ``gaussians_from_mesh`` with torch ops: sums by ``index_add_`` (atomics: not reproducible bit for bit)."""
    Nv = verts.shape[0]
    graph = arap.MeshGraph.from_faces(faces, Nv)
    col = graph.col.long()
    src = torch.repeat_interleave(torch.arange(Nv, device=verts.device), graph.degrees.long())
    delta = verts[col] - verts[src]
    edge_length = delta.norm(dim=1)
    mean_edge = torch.zeros_like(verts).index_add_(0, src, delta.abs()) / graph.degrees[:, None]
    grid = (uvs[faces_uvs] * 2 - 1)[None]
    corner = F.grid_sample(torch.flip(texture, [0]).permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border", align_corners=True)
    flat = faces.reshape(-1)
    colors = torch.zeros_like(verts).index_add_(0, flat, corner[0].permute(1, 2, 0).reshape(-1, 3))
    colors = colors / torch.bincount(flat, minlength=Nv).clamp(min=1)[:, None]
    xyz = scale_factor * (verts @ R.T)
    return xyz, torch.log(mean_edge / shrink * scale_factor), (colors - 0.5) / mesh.C0, colors, mean_edge, edge_length, graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--hub", type=int, default=64)
    ap.add_argument("--texture", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    nx = int(math.isqrt(a.n))
    ny = (a.n + nx - 1) // nx
    Nv = nx * ny
    g = torch.Generator().manual_seed(0)
    hub = (ny // 2) * nx + nx // 2                                                # an interior vertex: grid valence 6
    near = {hub + dx + dy * nx for dx in (-1, 0, 1) for dy in (-1, 0, 1)}
    others = [int(u) for u in torch.randperm(Nv, generator=g).tolist() if int(u) not in near][:a.hub - 6]       # the hub's grid valence is 6
    rim = torch.tensor(others, device="cuda")
    fan = torch.stack([torch.full_like(rim, hub), rim, rim.roll(-1)], 1)
    faces = torch.cat([grid_faces(nx, ny, "cuda"), fan])
    y, x = torch.meshgrid(torch.linspace(0, 1, ny), torch.linspace(0, 1, nx), indexing="ij")
    uvs = torch.stack([x, y], -1).reshape(Nv, 2).cuda()
    verts = torch.cat([uvs - 0.5, 0.1 * torch.sin(6.0 * uvs[:, :1])], 1) + 0.002 * torch.randn(Nv, 3, generator=g).cuda()
    texture = torch.rand(a.texture, a.texture, 3, generator=g).cuda()
    R = torch.tensor(mesh.frame_rotation(FRAME["rot_x_degree"], FRAME["rot_z_degree"]), dtype=torch.float32, device="cuda")

    def kernel():
        return mesh.gaussians_from_mesh(verts, faces, texture=texture, uvs=uvs, faces_uvs=faces, **FRAME)

    def restatement():
        return torch_ingest(verts, faces, texture, uvs, faces, R, FRAME["scale_factor"], 1.1)

    def graph_alone():
        return arap.MeshGraph.from_faces(faces, Nv)

    def corner_list_alone():
        return gather_plan(faces.reshape(-1), Nv)

    mg, theirs = kernel(), restatement()
    assert mg.graph.max_degree == a.hub, (mg.graph.max_degree, a.hub)
    exact = torch_ingest(verts.double(), faces, texture.double(), uvs.double(), faces, R.double(), FRAME["scale_factor"], 1.1)
    worst = lambda t, k: float((t.double() - exact[k]).abs().max())
    res = {"Nv": Nv, "faces": int(faces.shape[0]), "edges": int(mg.graph.col.shape[0]), "max_degree": mg.graph.max_degree,
           "texture": a.texture, "device": torch.cuda.get_device_name(0),
           "gaussians_from_mesh_error_vs_float64": {"xyz": worst(mg.gaussians.xyz, 0), "scaling": worst(mg.gaussians.scaling, 1),
                                                    "colors": worst(mg.colors, 3), "edge_length": worst(mg.edge_length, 5)},
           "torch_restatement_error_vs_float64": {"xyz": worst(theirs[0], 0), "scaling": worst(theirs[1], 1), "colors": worst(theirs[3], 3),
                                                  "edge_length": worst(theirs[5], 5)}}
    ours, torch_ms, graph_ms, plan_ms = [], [], [], []
    for _ in range(a.rounds):                                                     # alternating rounds in one process
        ours.append(timed(kernel, a.iters))
        torch_ms.append(timed(restatement, a.iters))
        graph_ms.append(timed(graph_alone, a.iters))
        plan_ms.append(timed(corner_list_alone, a.iters))
    med = lambda ts: round(sorted(ts)[len(ts) // 2], 3)
    res.update({"gaussians_from_mesh_ms": med(ours), "gaussians_from_mesh_ms_rounds": [round(t, 3) for t in ours],
                "torch_restatement_ms": med(torch_ms), "torch_restatement_ms_rounds": [round(t, 3) for t in torch_ms],
                "from_faces_alone_ms": med(graph_ms), "from_faces_alone_ms_rounds": [round(t, 3) for t in graph_ms],
                "corner_list_alone_ms": med(plan_ms), "corner_list_alone_ms_rounds": [round(t, 3) for t in plan_ms],
                "gaussians_from_mesh_peak_mib": round(peak_mib(kernel), 2), "torch_restatement_peak_mib": round(peak_mib(restatement), 2),
                "from_faces_alone_peak_mib": round(peak_mib(graph_alone), 2)})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
