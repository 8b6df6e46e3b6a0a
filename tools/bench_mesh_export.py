#!/usr/bin/env python
"""Time the mesh export's vertex normals with HIP events: ``mesh_export.vertex_normals`` with a prebuilt ``NormalPlan`` (one launch of
a3d_mesh_vertex_normals_f32) beside a vectorised torch restatement on the same GPU and in the same process (not the code under test):
``torch.cross`` per face, three ``index_add_`` for the per-vertex sums (atomics: not reproducible bit for bit), then a normalisation, all
in fp32.  The two alternate, round by round, with the plan's construction alone (once per mesh) in the same rounds; then the peak device
memory and each side's largest error against the same torch restatement in float64.  The host side is reported separately, by the wall
clock: ``write_animated_glb`` on arrays already on the host, and ``export_animated_glb`` as a whole (transform, normals, split, copies to
the host, file).

What the reference itself costs is not measured here: ``tools/mesh_animation/export_animated_mesh.py`` runs inside Blender, loops over
every vertex of every frame in Python, and is not part of this repository.  There is no pass/fail time: the export runs once per asset.

The mesh: tools/bench_mesh_ingest.py's, a triangulated grid of about ``--n`` vertices plus one hub of degree ``--hub``; ``--frames``
frames of a smooth deformation of it.

    python tools/bench_mesh_export.py [--n 100000] [--hub 64] [--frames 16] [--texture 1024] [--iters 20] [--rounds 5]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import mesh_export
from tools._timing import peak_mib, timed
from tools.bench_mesh_arap import grid_faces


def torch_normals(pos, faces):
    """``vertex_normals`` with torch ops in ``pos``'s dtype: the three corners of a face add the same ``u x w`` up to rounding."""
    a, b, d = pos[:, faces[:, 0]], pos[:, faces[:, 1]], pos[:, faces[:, 2]]
    area = torch.cross(b - a, d - a, dim=-1)
    s = torch.zeros_like(pos)
    for k in range(3):
        s.index_add_(1, faces[:, k], area)
    return s / s.norm(dim=-1, keepdim=True)


def wall_ms(fn, repeats=3):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--hub", type=int, default=64)
    ap.add_argument("--frames", type=int, default=16)
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
    others = [int(u) for u in torch.randperm(Nv, generator=g).tolist() if int(u) not in near][:a.hub - 6]
    rim = torch.tensor(others, device="cuda")
    faces = torch.cat([grid_faces(nx, ny, "cuda"), torch.stack([torch.full_like(rim, hub), rim, rim.roll(-1)], 1)])
    y, x = torch.meshgrid(torch.linspace(0, 1, ny), torch.linspace(0, 1, nx), indexing="ij")
    uvs = torch.stack([x, y], -1).reshape(Nv, 2).cuda()
    verts = torch.cat([uvs - 0.5, 0.1 * torch.sin(6.0 * uvs[:, :1])], 1) + 0.002 * torch.randn(Nv, 3, generator=g).cuda()
    phase = torch.linspace(0, math.pi, a.frames, device="cuda")[:, None, None]
    pos = (verts[None] + torch.cat([torch.zeros(a.frames, Nv, 2, device="cuda"), 0.05 * torch.sin(4.0 * uvs[None, :, 1:] + phase)], 2)).contiguous()
    texture = torch.rand(a.texture, a.texture, 3, generator=g).cuda()
    plan = mesh_export.NormalPlan(faces, Nv)

    def kernel():
        return mesh_export.vertex_normals(pos, plan)

    def restatement():
        return torch_normals(pos, faces)

    def plan_alone():
        return mesh_export.NormalPlan(faces, Nv)

    ours, theirs, exact = kernel(), restatement(), torch_normals(pos.double(), faces)
    worst = lambda t: float((t.double() - exact).abs().max())
    res = {"Nv": Nv, "faces": int(faces.shape[0]), "frames": a.frames, "max_corners": int(torch.bincount(faces.reshape(-1)).max()),
           "device": torch.cuda.get_device_name(0), "vertex_normals_error_vs_float64": worst(ours),
           "torch_restatement_error_vs_float64": worst(theirs), "two_calls_bitwise_equal": bool(torch.equal(ours, kernel())),
           "torch_restatement_two_calls_bitwise_equal": bool(torch.equal(theirs, restatement()))}
    del exact
    ours_ms, torch_ms, plan_ms = [], [], []
    for _ in range(a.rounds):                                                     # alternating rounds in one process
        ours_ms.append(timed(kernel, a.iters))
        torch_ms.append(timed(restatement, a.iters))
        plan_ms.append(timed(plan_alone, a.iters))
    med = lambda ts: round(sorted(ts)[len(ts) // 2], 3)
    res.update({"vertex_normals_ms": med(ours_ms), "vertex_normals_ms_rounds": [round(t, 3) for t in ours_ms],
                "torch_restatement_ms": med(torch_ms), "torch_restatement_ms_rounds": [round(t, 3) for t in torch_ms],
                "normal_plan_alone_ms": med(plan_ms), "normal_plan_alone_ms_rounds": [round(t, 3) for t in plan_ms],
                "vertex_normals_peak_mib": round(peak_mib(kernel), 2), "torch_restatement_peak_mib": round(peak_mib(restatement), 2)})
    # the host side, by the wall clock
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.glb")
        arrays = mesh_export.export_animated_glb(path, pos, faces, texture=texture, uvs=uvs, faces_uvs=faces)
        res["glb_mib"] = round(os.path.getsize(path) / 2 ** 20, 1)
        res["write_animated_glb_host_ms"] = wall_ms(lambda: mesh_export.write_animated_glb(
            path, arrays["positions"], arrays["normals"], arrays["indices"], uvs=arrays["uvs"], texture=arrays["texture"]))
        res["export_animated_glb_wall_ms"] = wall_ms(lambda: mesh_export.export_animated_glb(path, pos, faces, texture=texture, uvs=uvs, faces_uvs=faces))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
