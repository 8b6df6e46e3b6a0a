"""Generate tests/golden/stage4d_reg.npz by running the REFERENCE's own ``Animate3DSystem.training_step`` and ``tv_loss`` on the CPU with the
six regulariser weights of animate3d.py:256-296 switched on.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_stage4d_reg_goldens.py <path to the reference tree>

As tests/golden/make_stage4d_goldens.py does, ``training_step`` is taken out of custom/threestudio-animate3d/systems/animate3d.py through
the syntax tree, and ``tv_loss`` with its helper out of threestudio/utils/loss.py; both are executed as they lie, against stubs.  The
render stub returns seeded leaves (tests/stage4d_ref.py, tests/stage4d_reg_ref.py): besides ``comp_rgb`` / ``comp_mask`` / ``means3D`` also
``comp_depth`` and per-image ``scales``; ``geometry`` has ``get_scaling`` (the exponential of a seeded log-scale leaf) and ``get_opacity``.
Cases (tests/stage4d_reg_ref.cases): each weight non-zero alone and all six together, with and without guidance and ARAP.  Only data is
written: per case what the reference logs for each term and returns, and the gradients of the returned total with respect to the raw
render, depth and alpha of each render call, the means, the scales and the opacity."""
import ast
import os
import random
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import stage4d_ref as R  # noqa: E402
from tests import stage4d_reg_ref as G  # noqa: E402
from tests.golden.make_stage4d_goldens import AttrDict, cal_arap_error, cal_connectivity_from_points, extract  # noqa: E402

TERMS = tuple(G.LAMBDAS)                                          # the column order of `logged`


def extract_functions(path, names):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names)
    return ast.fix_missing_locations(ast.Module(body=body, type_ignores=[]))


class System:
    """What ``training_step`` touches of ``self``."""

    def __init__(self, case):
        self.cfg = AttrDict(load_guidance=case["guidance"], n_view=case["n_view"], n_frame=case["n_frame"],
                            progressive_iter_per_frame=R.PROGRESSIVE, sample_strategy=case["strategy"], loss=AttrDict(G.case_loss(case)),
                            connected_vertices_info_path="", guidance_eval_feq=0)
        self.global_step = case["step"]
        self.renderer = types.SimpleNamespace(cfg=types.SimpleNamespace(back_ground_color=list(R.BG)))
        self.scaling, self.opacity = (t.requires_grad_(True) for t in G.make_static())
        self.geometry = types.SimpleNamespace(_xyz=R.make_means("xyz", 1)[0], get_scaling=torch.exp(self.scaling), get_opacity=self.opacity)
        self.prompt_utils = None
        self.key = G.case_key(case)
        self.calls, self.logged = [], {}

    def C(self, value):
        return value

    def log(self, name, value, **kwargs):
        self.logged[name] = float(value.detach()) if isinstance(value, torch.Tensor) else float(value)

    def guidance(self, rgb, prompt_utils, **kwargs):
        return {"loss_sds": R.guidance_stub(rgb)}

    def __call__(self, batch):
        B = batch["c2w"].shape[0]
        key = f"{self.key}/r{len(self.calls)}"
        image, alpha = R.make_render(key, B)
        leaves = dict(image=image, alpha=alpha, depth=G.make_depth(key, B), means=R.make_means(key, B), scales=G.make_scales(key, B))
        for t in leaves.values():
            t.requires_grad_(True)
        self.calls.append(leaves)
        return {"comp_rgb": image.clamp(0, 1).permute(0, 2, 3, 1), "comp_mask": alpha.permute(0, 2, 3, 1),
                "comp_depth": leaves["depth"].permute(0, 2, 3, 1), "means3D": list(leaves["means"]), "scales": list(leaves["scales"]),
                "viewspace_points": []}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    ns = {"torch": torch, "F": F, "random": random, "cal_connectivity_from_points": cal_connectivity_from_points,
          "cal_arap_error": cal_arap_error}
    exec(compile(extract_functions(os.path.join(ref, "threestudio", "utils", "loss.py"), ("_tensor_size", "tv_loss")), "loss.py", "exec"), ns)
    exec(compile(extract(os.path.join(ref, "custom", "threestudio-animate3d", "systems", "animate3d.py")), "animate3d.py", "exec"), ns)
    cases = G.cases()
    n, h, w, pts = len(cases), R.H, R.W, R.N_POINTS
    logged = np.full((n, len(TERMS)), np.nan, np.float32)          # what the reference logs per term (NaN: not part of the step)
    returned = np.zeros(n, np.float32)
    render_b = np.zeros((n, 2), np.int32)                         # images of each render call (0: no such call)
    grads = dict(image=np.zeros((n, 2, G.MAX_B, 3, h, w), np.float32), depth=np.zeros((n, 2, G.MAX_B, 1, h, w), np.float32),
                 alpha=np.zeros((n, 2, G.MAX_B, 1, h, w), np.float32), means=np.zeros((n, 2, G.MAX_B, pts, 3), np.float32),
                 scales=np.zeros((n, 2, G.MAX_B, pts, 3), np.float32))
    d_opacity, d_scaling = np.zeros((n, pts, 1), np.float32), np.zeros((n, pts, 3), np.float32)
    for i, c in enumerate(cases):
        batch = R.make_batch(c["n_view"], c["n_frame"])
        if c["guidance"]:
            batch["random_camera"] = R.make_random_camera()
        random.seed(c["seed"])
        system = System(c)
        total = ns["training_step"](system, batch, 0)["loss"]
        total.backward()
        returned[i] = float(total.detach())
        for j, name in enumerate(TERMS):
            logged[i, j] = system.logged.get(G.LOGGED[name][0], np.nan)
            assert np.isnan(logged[i, j]) == (name not in c["on"]), (c, name)
        assert len(system.calls) == 1 + c["guidance"]
        for r, call in enumerate(system.calls):
            nb = call["image"].shape[0]
            render_b[i, r] = nb
            for name, leaf in call.items():
                if leaf.grad is not None:
                    grads[name][i, r, :nb] = leaf.grad.numpy()
        if system.opacity.grad is not None:
            d_opacity[i] = system.opacity.grad.numpy()
        if system.scaling.grad is not None:
            d_scaling[i] = system.scaling.grad.numpy()
    assert not d_scaling.any()                                    # the opacity term detaches the scales
    path = os.path.join(HERE, "stage4d_reg.npz")
    np.savez_compressed(path, logged=logged, returned=returned, render_b=render_b, d_opacity=d_opacity, n_cases=np.array(n),
                        **{f"d_{k}": v for k, v in grads.items()})
    print(n, "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
