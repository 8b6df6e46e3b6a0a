#!/usr/bin/env python
"""Time the regularisers of the 4-D stage's step (csrc/stage_reg.hip) with HIP events against the torch chains they replace, alternating in
one process:

* ``stage4d.image_regularizers`` forward + backward from a fixed render, against animate3d.py:270-296 as written: ``comp_rgb`` materialised
  (the clamp and permute of advanced_4d.py:180 / batch_renderer:73), ``tv_loss`` of it and of ``comp_depth`` permuted back, the sparsity of
  ``comp_mask``;
* ``stage4d.gaussian_regularizers`` forward + backward, against :256-279 as written (the norm of the concatenated means, the detached scale
  norm times the opacity, the sum of the concatenated scales);
* one ``stage4d.training_step`` with all six weights set against the same step with them at 0.

Per shape the rounds are printed one by one: their spread is what a difference has to be read against.  Peak device memory of one call of
each variant, and the bytes the two kernels have to move computed from the shapes, are in the same output.

    python tools/bench_stage4d_reg.py [--n 100000] [--rounds 5] [--iters 5] [--sides 256 1024]

Shapes: those of tools/bench_stage4d.py (60 images at 256^2 and 1024^2, 100 000 Gaussians).  A shape that does not fit in memory is
reported as such.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import arap, stage4d
from tests.stage4d_reg_ref import tv_ref as tv_loss       # threestudio/utils/loss.py:8-16: shifted slices, differences, squares
from tools._timing import peak_mib, timed
from tools.bench_stage4d import BG, LOSS, N_FRAME, N_VIEW, PROGRESSIVE, STEP, make_scene

REG = dict(lambda_tv_loss=1.0, lambda_depth_tv_loss=1.0, lambda_sparsity=1.0, lambda_position=1.0, lambda_opacity=1.0, lambda_scales=1.0)


def torch_image_terms(image, depth, alpha):
    comp_rgb = image.clamp(0, 1).permute(0, 2, 3, 1)                                              # what RenderOutput builds on access
    comp_depth, comp_mask = depth.permute(0, 2, 3, 1), alpha.permute(0, 2, 3, 1)
    loss = (comp_mask ** 2 + 0.01).sqrt().mean() * REG["lambda_sparsity"]
    loss = loss + REG["lambda_tv_loss"] * tv_loss(comp_rgb.permute(0, 3, 1, 2))
    return loss + REG["lambda_depth_tv_loss"] * tv_loss(comp_depth.permute(0, 3, 1, 2))


def torch_gaussian_terms(means, scales, scaling, opacity):
    loss = REG["lambda_position"] * torch.cat(list(means)).norm(dim=-1).mean()
    loss = loss + REG["lambda_opacity"] * (torch.exp(scaling).norm(dim=-1).detach().unsqueeze(-1) * opacity).sum()
    return loss + REG["lambda_scales"] * torch.sum(torch.cat(list(scales), dim=0))


def bench_side(n, side, rounds, iters):
    gaussians, field, batch = make_scene(n, side)
    graph = arap.ArapGraph(gaussians.xyz, K=3, radius=0.01)
    bg = torch.tensor(BG, device="cuda")
    frames = stage4d.sampled_frames(STEP, N_FRAME, PROGRESSIVE, do_guidance=False)
    sel = stage4d.sampled_image_index(frames, N_VIEW, N_FRAME, "cuda").long()
    B = len(sel)
    gen = torch.Generator(device="cuda")

    def step(loss_cfg):
        def run():
            for p in field.parameters():
                p.grad = None
            out = stage4d.training_step(field, gaussians, batch, loss=loss_cfg, global_step=STEP, n_view=N_VIEW, n_frame=N_FRAME,
                                        progressive_iter_per_frame=PROGRESSIVE, bg=BG, graph=graph, generator=gen.manual_seed(1))
            out["loss"].backward()
            return out
        return run
    step_reg, step_zero = step(dict(LOSS, **REG)), step(LOSS)
    res = {"side": side, "images": B, "gaussians": n, "device": torch.cuda.get_device_name(0)}
    res["step_terms"] = {k: round(float(v.detach()), 6) for k, v in step_reg().items()}
    # the two calls alone, from a fixed render
    with torch.no_grad():
        out = stage4d.render_batch(field, gaussians, batch["c2w"][sel], batch["fovy"][sel], batch["timestamps"][sel], side, side, bg,
                                   do_guidance=False)
    image, alpha = out["image"].detach().requires_grad_(True), out["alpha"].detach().requires_grad_(True)
    depth = out["comp_depth"].permute(0, 3, 1, 2).detach().contiguous().requires_grad_(True)
    means, scales = out["means3D"].detach().requires_grad_(True), out["scales"].detach().requires_grad_(True)
    opacity = gaussians.opacity.detach().clone().requires_grad_(True)
    del out
    leaves = (image, depth, alpha, means, scales, opacity)

    def clear():
        for t in leaves:
            t.grad = None

    def image_new():
        clear()
        stage4d.image_regularizers(image, depth, alpha, lambda_tv=REG["lambda_tv_loss"], lambda_depth_tv=REG["lambda_depth_tv_loss"],
                                   lambda_sparsity=REG["lambda_sparsity"])[0].backward()

    def image_torch():
        clear()
        torch_image_terms(image, depth, alpha).backward()

    def gauss_new():
        clear()
        stage4d.gaussian_regularizers(means, scales, gaussians.scaling, opacity, lambda_position=REG["lambda_position"],
                                      lambda_scales=REG["lambda_scales"], lambda_opacity=REG["lambda_opacity"])[0].backward()

    def gauss_torch():
        clear()
        torch_gaussian_terms(means, scales, gaussians.scaling, opacity).backward()
    grads = {}
    for tag, image_fn, gauss_fn in (("new", image_new, gauss_new), ("torch", image_torch, gauss_torch)):      # each call clears every leaf
        image_fn()
        grads[tag] = [t.grad.clone() for t in leaves[:3]]
        gauss_fn()
        grads[tag] += [t.grad.clone() for t in leaves[3:]]
    res["max_abs_grad_difference"] = {k: float((a - b).abs().max()) for k, a, b in
                                      zip(("image", "depth", "alpha", "means", "scales", "opacity"), grads["new"], grads["torch"])}
    del grads
    pixels = B * side * side
    # both directions read the five planes once (the neighbours come from the caches); the backward writes them
    res["image_kernel_bytes"] = pixels * 5 * 4 * 3
    res["gaussian_kernel_bytes"] = B * n * (2 * 12 + 12 + 2 * 12) + n * (2 * 12 + 4 + 4)
    series = {k: [] for k in ("image_new", "image_torch", "gauss_new", "gauss_torch", "step_reg", "step_zero")}
    fns = dict(image_new=image_new, image_torch=image_torch, gauss_new=gauss_new, gauss_torch=gauss_torch, step_reg=step_reg,
               step_zero=step_zero)
    for r in range(rounds):                                         # alternating: every round times all six, in this order
        for name in series:
            series[name].append(round(timed(fns[name], iters), 3))
        print(f"[side {side} round {r}] " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in series.items()), flush=True)
    for name, ts in series.items():
        s = sorted(ts)
        res[name + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": ts}
    res["image_new_GBps"] = round(res["image_kernel_bytes"] / (res["image_new_ms"]["median"] * 1e-3) / 1e9, 1)
    res["gauss_new_GBps"] = round(res["gaussian_kernel_bytes"] / (res["gauss_new_ms"]["median"] * 1e-3) / 1e9, 1)
    clear()
    for p in field.parameters():
        p.grad = None
    for name in series:
        res["peak_mib_" + name] = round(peak_mib(fns[name]), 1)
        clear()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage4d_reg.py needs the GPU: there is no CPU fallback and a CPU time would say nothing")
    for side in a.sides:
        try:
            res = bench_side(a.n, side, a.rounds, a.iters)
        except torch.cuda.OutOfMemoryError as e:
            res = {"side": side, "not_measured": f"out of memory: {str(e).splitlines()[0]}"}
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
