#!/usr/bin/env python
"""Time one optimisation step of the 4-D stage (forward and ``backward()``) with HIP events, in two variants that alternate in the same
process on the same kernels: ``stage4d.training_step`` (the loss kernel reading the resident ground truth through the index, the
keep-mask as one autograd function) and the torch glue it replaces, written out as the reference has it (the ``val[sampled_idx]`` copies,
the ``t * keep + t.detach() * (1 - keep)`` blend, clamp / permute, the compositing with the float mask and two ``F.mse_loss``).  Both run
the same deformation field, rasterizer and ARAP kernels.  Each variant's loss alone (forward + backward from a fixed render) is timed too,
with the bytes the kernel has to move computed from the shapes.  Per shape the rounds are printed one by one: their spread is what a
difference between the variants has to be read against.  Peak device memory of one step of each variant is in the same output.

    python tools/bench_stage4d.py [--n 100000] [--rounds 5] [--iters 5] [--sides 256 1024]

Shapes: 4 views x 16 frames of ground truth, the 15 frames after the first sampled (60 images: the stage-1 step at its last schedule
position, and the batch of the refine config) at 256^2 and 1024^2.  A shape that does not fit in memory is reported as such.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from animate3d_amd import arap, deform4d, splat, stage4d
from tests import gs_ref
from tools._timing import peak_mib, timed

N_VIEW, N_FRAME, PROGRESSIVE = 4, 16, 50
LOSS = dict(lambda_rgb=100.0, lambda_mask=100.0, lambda_arap=12.0, arap_sample_num=512)         # configs/motion_recon_frame_16.yaml
BG = (0.5, 0.5, 0.5)
STEP = PROGRESSIVE * (N_FRAME - 1)                                                                # every frame after the first


def make_scene(n, side):
    g = torch.Generator().manual_seed(0)
    xyz = (torch.randn(n, 3, generator=g) * 0.6).cuda()
    gaussians = stage4d.Gaussians(xyz, (torch.rand(n, 3, generator=g) * 2.0 - 5.2).cuda(), torch.randn(n, 4, generator=g).cuda(),
                                  torch.sigmoid(torch.randn(n, 1, generator=g) * 1.5).cuda(), (torch.randn(n, 16, 3, generator=g) * 0.3).cuda(), 3)
    field = deform4d.HexPlaneDeformation(use_global_trans=True)
    with torch.no_grad():
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    field = field.cuda()
    views = torch.stack([gs_ref.look_at((3.5 * math.cos(a), 3.5 * math.sin(a), 0.3)) for a in (0.0, math.pi / 2, math.pi, 1.5 * math.pi)])
    S = N_VIEW * N_FRAME
    batch = dict(c2w=views[:, None].expand(N_VIEW, N_FRAME, 4, 4).reshape(S, 4, 4).cuda().contiguous(),
                 fovy=torch.full((S,), math.radians(40.0), device="cuda"), timestamps=torch.linspace(-1, 1, N_FRAME).repeat(N_VIEW).cuda(),
                 rgb=torch.rand(S, side, side, 3, device="cuda"), mask=torch.rand(S, side, side, 1, device="cuda") > 0.5)
    return gaussians, field, batch


def glue_loss(image, alpha, batch, sampled_idx):
    """animate3d.py:160-184 on the renderer's outputs, as written."""
    sub = {k: v[sampled_idx] for k, v in batch.items() if k in ("rgb", "mask")}                  # batch[key] = val[sampled_idx]
    pred_rgb = image.clamp(0, 1).permute(0, 2, 3, 1)                                              # advanced_4d.py:180, batch_renderer:73
    comp_mask = alpha.permute(0, 2, 3, 1)
    gt_mask, gt_rgb = sub["mask"], sub["rgb"]
    gt_rgb = gt_rgb * gt_mask.float() + BG[0] * (1 - gt_mask.float())
    return LOSS["lambda_rgb"] * F.mse_loss(gt_rgb, pred_rgb) + LOSS["lambda_mask"] * F.mse_loss(gt_mask.float(), comp_mask)


def bench_side(n, side, rounds, iters):
    gaussians, field, batch = make_scene(n, side)
    graph = arap.ArapGraph(gaussians.xyz, K=3, radius=0.01)
    bg = torch.tensor(BG, device="cuda")
    frames = stage4d.sampled_frames(STEP, N_FRAME, PROGRESSIVE, do_guidance=False)
    index = stage4d.sampled_image_index(frames, N_VIEW, N_FRAME, "cuda")
    sampled_idx = index.long()
    B = len(sampled_idx)
    gen = torch.Generator(device="cuda")

    def zero():
        for p in field.parameters():
            p.grad = None

    def new_step():
        zero()
        out = stage4d.training_step(field, gaussians, batch, loss=LOSS, global_step=STEP, n_view=N_VIEW, n_frame=N_FRAME,
                                    progressive_iter_per_frame=PROGRESSIVE, bg=BG, graph=graph, generator=gen.manual_seed(1))
        out["loss"].backward()
        return out["loss"]

    def glue_step():
        zero()
        gen.manual_seed(1)
        sub = {k: batch[k][sampled_idx] for k in ("c2w", "fovy", "timestamps")}
        ts, i2t = stage4d.frames_of_images(sub["timestamps"])
        means, scales, rots = field(gaussians.xyz, gaussians.scaling, gaussians.rotation, ts, i2t, deform_scales=False)
        keep = (torch.rand(B, n, 1, generator=gen, device="cuda") < 0.1).float()                 # advanced_4d.py:147-154
        m_in = means * keep + means.detach().clone() * (1 - keep)
        s_in = scales * keep + scales.detach().clone() * (1 - keep)
        r_in = rots * keep + rots.detach().clone() * (1 - keep)
        w2c, proj, cam_p = splat.get_cam_info_gaussian(sub["c2w"], sub["fovy"], sub["fovy"], znear=0.1, zfar=100)
        tan = torch.tan(sub["fovy"] / 2)
        image, _, _, alpha = splat.rasterize_gaussians(m_in, s_in, r_in, gaussians.opacity, shs=gaussians.shs, viewmatrix=w2c, projmatrix=proj,
                                                       campos=cam_p, tanfovx=tan, tanfovy=tan, image_height=side, image_width=side, bg=bg,
                                                       sh_degree=3)
        loss = glue_loss(image, alpha, batch, sampled_idx)
        loss = loss + LOSS["lambda_arap"] * arap.arap_energy(gaussians.xyz, means[:len(frames)], graph.refresh(gaussians.xyz).nn_idx,
                                                             sample_num=LOSS["arap_sample_num"], generator=gen)
        loss.backward()
        return loss

    res = {"side": side, "images": B, "gaussians": n, "device": torch.cuda.get_device_name(0)}
    l_new, l_glue = float(new_step().detach()), float(glue_step().detach())
    res.update(loss_new=l_new, loss_glue=l_glue, instances=splat.last_instance_count())
    # the loss alone, from a fixed render
    with torch.no_grad():
        out = stage4d.render_batch(field, gaussians, batch["c2w"][sampled_idx], batch["fovy"][sampled_idx], batch["timestamps"][sampled_idx],
                                   side, side, bg, do_guidance=False)
    image, alpha = out["image"].detach().requires_grad_(True), out["alpha"].detach().requires_grad_(True)
    del out

    def new_loss():
        image.grad = alpha.grad = None
        stage4d.masked_recon_loss(image, alpha, batch["rgb"], batch["mask"], index, bg=BG[0], lambda_rgb=LOSS["lambda_rgb"],
                                  lambda_mask=LOSS["lambda_mask"])[0].backward()

    def glue_loss_alone():
        image.grad = alpha.grad = None
        glue_loss(image, alpha, batch, sampled_idx).backward()
    pixels = B * side * side
    moved = pixels * (2 * (12 + 4 + 12 + 1) + 16)                  # both directions read image, alpha, gt_rgb, mask; the backward writes 16 B
    series = {"step_new": [], "step_glue": [], "loss_new": [], "loss_glue": []}
    for r in range(rounds):                                         # alternating: every round times all four, in this order
        for name, fn in (("step_new", new_step), ("step_glue", glue_step), ("loss_new", new_loss), ("loss_glue", glue_loss_alone)):
            series[name].append(round(timed(fn, iters), 3))
        print(f"[side {side} round {r}] " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in series.items()), flush=True)
    for name, ts in series.items():
        s = sorted(ts)
        res[name + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": ts}
    res["loss_kernel_bytes"] = moved
    res["loss_new_GBps"] = round(moved / (res["loss_new_ms"]["median"] * 1e-3) / 1e9, 1)
    image.grad = alpha.grad = None
    zero()
    res["peak_mib_step_new"], res["peak_mib_step_glue"] = round(peak_mib(new_step), 1), round(peak_mib(glue_step), 1)
    zero()
    res["peak_mib_loss_new"], res["peak_mib_loss_glue"] = round(peak_mib(new_loss), 1), round(peak_mib(glue_loss_alone), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage4d.py needs the GPU: there is no CPU fallback and a CPU time would say nothing")
    for side in a.sides:
        try:
            res = bench_side(a.n, side, a.rounds, a.iters)
        except torch.cuda.OutOfMemoryError as e:
            res = {"side": side, "not_measured": f"out of memory: {str(e).splitlines()[0]}"}
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
