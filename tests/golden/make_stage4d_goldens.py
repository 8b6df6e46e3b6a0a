"""Generate tests/golden/stage4d.npz by running the REFERENCE's own ``Animate3DSystem.training_step`` on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_stage4d_goldens.py <path to the reference tree>

``training_step`` (custom/threestudio-animate3d/systems/animate3d.py:120-370) is taken out of the reference file through the syntax tree
and executed as it lies; the module imports threestudio, pytorch3d and more at its top, so only this one definition is executed, against
stubs: ``cfg`` is an attribute-and-item dictionary, ``C`` the identity, ``log`` keeps the reference's own loss names; the system is callable (the renderer), records
``do_guidance`` and the gathered ``c2w`` / ``fovy`` / ``timestamps`` of each call and returns seeded tensors (tests/stage4d_ref.py:
``comp_rgb`` is the clamp and permute of a leaf with values below 0, above 1 and at the bounds, as advanced_4d.py:180 and
batch_renderer:73 make it); ``guidance`` is a fixed quadratic; ``cal_connectivity_from_points`` / ``cal_arap_error`` return a weighted sum
of ``nodes_t`` whose weights tell the node's position, so the gradient shows which ``means3D`` entries the reference hands to ARAP.
``random`` is seeded per case.  Only data is written: per case the sampled index, what each render call saw, the losses it logs
and returns; for the numeric cases also the gradients with respect to the raw render and alpha."""
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

MAX_B = 4 * 7
LOGGED = ("loss", "loss_rgb", "loss_mask", "loss_sds", "loss_arap")      # the reference's log names; the terms times their lambdas


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def extract(path):
    tree = ast.parse(open(path).read())
    (cls,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Animate3DSystem"]
    (fn,) = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "training_step"]
    return ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))


class System:
    """What ``training_step`` touches of ``self``."""

    def __init__(self, case):
        loss = AttrDict(R.LOSS, lambda_arap=R.LOSS["lambda_arap"] if case["arap"] else 0.0)
        self.cfg = AttrDict(load_guidance=case["guidance"], n_view=case["n_view"], n_frame=case["n_frame"],
                            progressive_iter_per_frame=R.PROGRESSIVE, sample_strategy=case["strategy"], loss=loss,
                            connected_vertices_info_path="", guidance_eval_feq=0)
        self.global_step = case["step"]
        self.renderer = types.SimpleNamespace(cfg=types.SimpleNamespace(back_ground_color=list(R.BG)))
        self.geometry = types.SimpleNamespace(_xyz=R.make_means("xyz", 1)[0])
        self.prompt_utils = None
        self.key = R.case_key(case)
        self.calls, self.logged = [], {}

    def C(self, value):
        return value

    def log(self, name, value, **kwargs):
        if name in LOGGED:
            self.logged[name] = float(value.detach()) if isinstance(value, torch.Tensor) else float(value)

    def guidance(self, rgb, prompt_utils, **kwargs):
        assert kwargs["rgb_as_latents"] is False and kwargs["guidance_eval"] is False
        return {"loss_sds": R.guidance_stub(rgb)}

    def __call__(self, batch):
        B = batch["c2w"].shape[0]
        image, alpha = R.make_render(f"{self.key}/r{len(self.calls)}", B)
        means = R.make_means(f"{self.key}/r{len(self.calls)}", B)
        for t in (image, alpha, means):
            t.requires_grad_(True)
        self.calls.append(dict(do_guidance=batch["do_guidance"], do_reconstruction=batch["do_reconstruction"], ids=batch["c2w"][:, 0, 3].clone(),
                               fovy=batch["fovy"].clone(), timestamps=batch["timestamps"].clone(), image=image, alpha=alpha, means=means))
        return {"comp_rgb": torch.stack([im.clamp(0, 1) for im in image], dim=0).permute(0, 2, 3, 1),
                "comp_mask": torch.stack(list(alpha), dim=0).permute(0, 2, 3, 1), "means3D": list(means), "viewspace_points": []}


def cal_connectivity_from_points(points, radius, K):
    return None, None, None, None


def cal_arap_error(nodes_t, ii, jj, nn, K, sample_num):
    return (nodes_t * R.arap_stub_weight(nodes_t.shape)).sum()


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    ns = {"torch": torch, "F": F, "random": random, "cal_connectivity_from_points": cal_connectivity_from_points,
          "cal_arap_error": cal_arap_error}
    exec(compile(extract(os.path.join(ref, "custom", "threestudio-animate3d", "systems", "animate3d.py")), "animate3d.py", "exec"), ns)
    cases = R.cases()
    n = len(cases)
    sampled_idx = np.full((n, MAX_B), -1, np.int32)
    render_ids = np.full((n, 2, MAX_B), -1, np.int32)             # what each render call was handed, in order: c2w[:, 0, 3]
    render_flags = np.full((n, 2), -1, np.int32)                  # do_guidance of each call
    arap_pos = np.full((n, 2, MAX_B), -1, np.int32)               # position among ARAP's targets of each image's means, per render
    losses = np.full((n, len(LOGGED)), np.nan, np.float32)        # what the reference logs under LOGGED (NaN: not part of the step)
    returned = np.zeros(n, np.float32)                            # the returned total
    d_image, d_alpha, numeric_at = [], [], np.full((n, 2, 2), -1, np.int64)      # [case, render] -> (first row, rows) in d_image / d_alpha
    rows = 0
    for i, c in enumerate(cases):
        batch = R.make_batch(c["n_view"], c["n_frame"])
        if c["guidance"]:
            batch["random_camera"] = R.make_random_camera()
        random.seed(c["seed"])
        system = System(c)
        total = ns["training_step"](system, batch, 0)["loss"]
        leaves = [t for call in system.calls for t in (call["image"], call["alpha"], call["means"])]
        grads = torch.autograd.grad(total, leaves, allow_unused=True)
        first = system.calls[0]
        B = first["ids"].shape[0]
        sampled_idx[i, :B] = first["ids"].int().numpy()
        assert torch.equal(first["fovy"], batch["fovy"]) and torch.equal(first["timestamps"], batch["timestamps"])   # gathered in place
        assert torch.equal(first["fovy"], (0.5 + 0.01 * first["ids"]))
        returned[i] = float(total.detach())
        for j, name in enumerate(LOGGED):
            losses[i, j] = system.logged.get(name, np.nan)
        for r, call in enumerate(system.calls):
            nb = call["ids"].shape[0]
            render_ids[i, r, :nb] = call["ids"].int().numpy()
            render_flags[i, r] = int(call["do_guidance"])
            assert call["do_reconstruction"] is True
            g_img, g_alpha, g_means = grads[3 * r:3 * r + 3]
            if g_means is not None:
                lam = R.LOSS["lambda_arap"]
                pos = torch.floor(g_means[:, 0, 0] / lam + 0.5).int() - 1          # weight (f, 0, 0) = f; node 0 is xyz
                arap_pos[i, r, :nb] = torch.where(g_means.abs().sum((1, 2)) > 0, pos, torch.full_like(pos, -1)).numpy()
            if c["numeric"]:
                numeric_at[i, r] = (rows, nb)
                d_image.append((torch.zeros_like(call["image"]) if g_img is None else g_img).numpy())
                d_alpha.append((torch.zeros_like(call["alpha"]) if g_alpha is None else g_alpha).numpy())
                rows += nb
    out = dict(sampled_idx=sampled_idx, render_ids=render_ids, render_flags=render_flags, arap_pos=arap_pos, losses=losses, returned=returned,
               numeric_at=numeric_at, d_image=np.concatenate(d_image), d_alpha=np.concatenate(d_alpha), n_cases=np.array(n))
    path = os.path.join(HERE, "stage4d.npz")
    np.savez_compressed(path, **out)
    print(n, "cases,", int((numeric_at[:, 0, 0] >= 0).sum()), "numeric,", rows, "gradient images,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
