#!/usr/bin/env python
"""Time the frames layer of the 4-D stage (``animate3d_amd/frames.py``, ``stage4d.masked_recon_loss_rgba8``) against the fp32 ground truth it
stands in for, with HIP events, in one process, the variants alternating:

* the reconstruction loss alone, forward + backward from a fixed render: ``masked_recon_loss_rgba8`` on ``rgba8 [S, H, W, 4]`` uint8 against
  ``masked_recon_loss`` on ``rgb [S, H, W, 3]`` fp32 + ``mask`` bool holding the same values, with the bytes each has to move;
* one whole ``training_step`` with ``backward()`` on each;
* the resident bytes of the ground truth and the peak device memory of one step of each;
* ``load_frames`` of ``n_view * n_frame`` PNGs by the wall clock, decode (host) and upload + unpack (device, synchronised) apart;
* ``test_renders`` of the 192 test-set cameras (3 elevations x 4 azimuths x 16 frames), by the wall clock, synchronised.

    python tools/bench_stage_frames.py [--n 100000] [--rounds 5] [--iters 5] [--sides 256 1024] [--io-side 1024]

Shapes: 4 views x 16 frames of ground truth, the 15 frames after the first sampled (60 images), as tools/bench_stage4d.py.  Per shape the
rounds are printed one by one: their spread is what a difference between the variants has to be read against.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import cameras, frames, stage4d
from tools._timing import peak_mib, timed
from tools.bench_stage4d import BG, LOSS, N_FRAME, N_VIEW, PROGRESSIVE, STEP, make_scene

STEP_LOSS = dict(LOSS, lambda_arap=0.0)                          # the step without ARAP: rendering and the reconstruction loss


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ts):
    s = sorted(ts)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": ts}


def bench_side(n, side, rounds, iters):
    gaussians, field, batch = make_scene(n, side)
    S = N_VIEW * N_FRAME
    del batch["rgb"], batch["mask"]
    rgba8 = torch.randint(0, 256, (S, side, side, 4), dtype=torch.uint8, device="cuda")
    fs = frames.FrameSet(rgba8, N_VIEW, N_FRAME)
    batch_u8 = dict(batch, rgba8=fs)
    batch_f32 = dict(batch, rgb=fs.rgb(), mask=fs.mask())
    bg = torch.tensor(BG, device="cuda")
    frames_ = stage4d.sampled_frames(STEP, N_FRAME, PROGRESSIVE, do_guidance=False)
    index = stage4d.sampled_image_index(frames_, N_VIEW, N_FRAME, "cuda")
    B = index.numel()
    gen = torch.Generator(device="cuda")

    def step(b):
        def run():
            for p in field.parameters():
                p.grad = None
            out = stage4d.training_step(field, gaussians, b, loss=STEP_LOSS, global_step=STEP, n_view=N_VIEW, n_frame=N_FRAME,
                                        progressive_iter_per_frame=PROGRESSIVE, bg=BG, generator=gen.manual_seed(1))
            out["loss"].backward()
            return out["loss"]
        return run
    step_u8, step_f32 = step(batch_u8), step(batch_f32)
    res = {"side": side, "images": B, "frames_resident": S, "gaussians": n, "device": torch.cuda.get_device_name(0)}
    l_u8, l_f32 = step_u8().detach(), step_f32().detach()
    res.update(loss_u8=float(l_u8), loss_f32=float(l_f32), step_losses_bitwise_equal=bool(torch.equal(l_u8, l_f32)))
    with torch.no_grad():
        gather = index.long()
        out = stage4d.render_batch(field, gaussians, batch["c2w"][gather], batch["fovy"][gather], batch["timestamps"][gather], side, side, bg,
                                   do_guidance=False)
    image, alpha = out["image"].detach().requires_grad_(True), out["alpha"].detach().requires_grad_(True)
    del out
    kw = dict(bg=BG[0], lambda_rgb=LOSS["lambda_rgb"], lambda_mask=LOSS["lambda_mask"])

    def loss_u8():
        image.grad = alpha.grad = None
        stage4d.masked_recon_loss_rgba8(image, alpha, rgba8, index, **kw)[0].backward()

    def loss_f32():
        image.grad = alpha.grad = None
        stage4d.masked_recon_loss(image, alpha, batch_f32["rgb"], batch_f32["mask"], index, **kw)[0].backward()
    pixels = B * side * side
    moved = {"loss_u8": pixels * (2 * (12 + 4 + 4) + 16), "loss_f32": pixels * (2 * (12 + 4 + 12 + 1) + 16)}      # both directions read, the backward writes 16 B
    series = {"step_u8": [], "step_f32": [], "loss_u8": [], "loss_f32": []}
    for r in range(rounds):                                         # alternating: every round times all four, in this order
        for name, fn in (("step_u8", step_u8), ("step_f32", step_f32), ("loss_u8", loss_u8), ("loss_f32", loss_f32)):
            series[name].append(round(timed(fn, iters), 3))
        print(f"[side {side} round {r}] " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in series.items()), flush=True)
    for name, ts in series.items():
        res[name + "_ms"] = summary(ts)
    for name, nbytes in moved.items():
        res[name + "_bytes"] = nbytes
        res[name + "_GBps"] = round(nbytes / (res[name + "_ms"]["median"] * 1e-3) / 1e9, 1)
    res["resident_mib_u8"] = round(rgba8.numel() / 2 ** 20, 1)
    res["resident_mib_f32"] = round((batch_f32["rgb"].numel() * 4 + batch_f32["mask"].numel()) / 2 ** 20, 1)
    image.grad = alpha.grad = None
    for p in field.parameters():
        p.grad = None
    res["peak_mib_step_u8"], res["peak_mib_step_f32"] = round(peak_mib(step_u8), 1), round(peak_mib(step_f32), 1)
    return res


def bench_io(n, side, rounds):
    """The two ends on files: the 64 data views rendered, written, and loaded back; the 192 test-set cameras rendered."""
    gaussians, field, _ = make_scene(n, 8)
    bg = torch.tensor(BG, device="cuda")
    data = cameras.data_view_cameras(default_elevation_deg=5.0, default_azimuth_deg=[0.0, 90.0, 180.0, 270.0], default_camera_distance=3.5,
                                     default_fovy_deg=40.0, n_view=N_VIEW, total_frame=N_FRAME, height=side, width=side, device="cuda")
    test = cameras.testset_cameras(dict(total_frame=N_FRAME, eval_height=side, eval_width=side, eval_camera_distance=3.5, eval_fovy_deg=40.0),
                                   device="cuda")
    res = {"io_side": side, "files": N_VIEW * N_FRAME, "test_cameras": test.c2w.shape[0], "gaussians": n}
    rendered = frames.test_renders(field, gaussians, data, bg, do_guidance=False)
    series = {"decode": [], "upload_unpack": [], "load_frames": [], "test_renders_192": [], "write_64": []}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            ms, _ = wall_ms(lambda: frames.write_test_renders(tmp, rendered, n_frame=N_FRAME, test_option="four_view"))
            series["write_64"].append(round(ms, 1))
            root = os.path.join(tmp, "images")
            ms, host = wall_ms(lambda: frames.decode_frames(root, count=N_VIEW * N_FRAME))
            series["decode"].append(round(ms, 1))
            ms, _ = wall_ms(lambda: frames.unpack_rgba8(torch.from_numpy(host).cuda(), out8=True))
            series["upload_unpack"].append(round(ms, 1))
            ms, fs = wall_ms(lambda: frames.load_frames(root, side, side, n_view=N_VIEW, n_frame=N_FRAME))
            series["load_frames"].append(round(ms, 1))
            ms, out = wall_ms(lambda: frames.test_renders(field, gaussians, test, bg, do_guidance=False))
            series["test_renders_192"].append(round(ms, 1))
            print(f"[io side {side} round {r}] " + "  ".join(f"{k} {v[-1]:.1f} ms" for k, v in series.items()), flush=True)
        res["png_bytes"] = sum(os.path.getsize(os.path.join(root, f)) for f in os.listdir(root))
        res["round_trip_bitwise_equal"] = bool(torch.equal(fs.rgba8, rendered))
    for name, ts in series.items():
        res[name + "_wall_ms"] = summary(ts)
    res["test_renders_result_mib"] = round(out.numel() / 2 ** 20, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--io-side", type=int, default=1024)
    ap.add_argument("--io-rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage_frames.py needs the GPU: there is no CPU fallback and a CPU time would say nothing")
    for side in a.sides:
        try:
            res = bench_side(a.n, side, a.rounds, a.iters)
        except torch.cuda.OutOfMemoryError as e:
            res = {"side": side, "not_measured": f"out of memory: {str(e).splitlines()[0]}"}
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(bench_io(a.n, a.io_side, a.io_rounds)), flush=True)


if __name__ == "__main__":
    main()
