"""Generate tests/golden/gs_camera.npz by running the REFERENCE's own Gaussian camera helpers.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_gs_camera_goldens.py

``convert_pose``, ``get_projection_matrix_gaussian`` and ``get_cam_info_gaussian`` (threestudio/utils/ops.py:305-359) are compiled
from the reference file as it lies (the module imports more than this box has, so only these function definitions are executed),
with ``.cuda()`` redirected to the CPU.  Only data (seeded inputs and the reference's outputs) is written.
"""
import ast
import math
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NAMES = ("convert_pose", "get_projection_matrix_gaussian", "get_cam_info_gaussian")


def main():
    tree = ast.parse(open(os.path.join(REF, "threestudio/utils/ops.py")).read())
    fns = [nd for nd in tree.body if isinstance(nd, ast.FunctionDef) and nd.name in NAMES]
    assert len(fns) == len(NAMES)
    ns = {"torch": torch, "math": math}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "gs_camera", "exec"), ns)
    ns["get_projection_matrix_gaussian"].__defaults__ = ("cpu",)
    torch.Tensor.cuda = lambda self, *a, **k: self                     # device redirect: the CPU stands in for cuda
    g = torch.Generator().manual_seed(0)
    B = 6
    c2w = torch.eye(4).repeat(B, 1, 1)
    q = torch.randn(B, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    c2w[:, :3, :3] = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(B, 3, 3)
    c2w[:, :3, 3] = torch.randn(B, 3, generator=g) * 3
    fovy = torch.deg2rad(15 + torch.rand(B, generator=g) * 45)
    out = {"c2w": c2w.numpy(), "fovy": fovy.numpy(), "znear": np.float32(0.1), "zfar": np.float32(100.0)}
    w2c, full, center, proj, conv = [], [], [], [], []
    for i in range(B):
        a, b, c = ns["get_cam_info_gaussian"](c2w=c2w[i], fovx=float(fovy[i]), fovy=float(fovy[i]), znear=0.1, zfar=100)
        w2c.append(a); full.append(b); center.append(c)
        proj.append(ns["get_projection_matrix_gaussian"](0.1, 100, float(fovy[i]), float(fovy[i])))
        conv.append(ns["convert_pose"](c2w[i]))
    for k, v in (("world_view_transform", w2c), ("full_proj_transform", full), ("camera_center", center), ("projection", proj),
                 ("converted_pose", conv)):
        out[k] = torch.stack(v).float().numpy()
    np.savez(os.path.join(HERE, "gs_camera.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
