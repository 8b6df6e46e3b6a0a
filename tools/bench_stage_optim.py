#!/usr/bin/env python
"""Time the optimiser step of the 4-D stage: ``stage_optim.StageAdam.step()`` (csrc/stage_optim.hip: at most four launches for the 22
tensors of the released field) against ``torch.optim.Adam`` on the same parameters, for-each and, where this torch build offers it on
ROCm, ``fused=True``.  One process, the variants alternating, every call between two HIP events after a warm-up; per variant the median,
the range and the host's time to enqueue a call (a clock around the call, without a synchronise).  Then one stage-1 ``stage4d.fit`` step
with each optimiser, alternating again: 100 k Gaussians at 256^2 on the scene of tools/bench_stage4d.py.

    python tools/bench_stage_optim.py [--calls 250] [--block 10] [--n 100000] [--side 256] [--rounds 7] [--iters 3]

The field is the released one (``use_global_trans=True``, grids [[50, 50, 50, 8], [100, 100, 100, 16]] x 16 channels: 22 tensors); its
gradients are seeded and stay in place, so every call of every variant reads the same numbers.  The bytes a step has to move (p, m, v
read and written, g read: 28 per parameter) are computed from the shapes."""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from animate3d_amd import arap, deform4d, stage4d
from animate3d_amd.stage_optim import StageAdam
from tools._timing import timed
from tools.bench_stage4d import BG, LOSS, N_FRAME, N_VIEW, PROGRESSIVE, STEP, make_scene

RATES = dict(delta_xyz_network_lr=1e-4, delta_rot_network_lr=1e-4, delta_scaling_network_lr=1e-4, grid_lr=1e-2, global_trans_lr=1e-3)


def optimisers(field):
    """{variant: (field copy, optimiser)}; a variant this build cannot construct or step is left out, with the reason."""
    made, left_out = {}, {}
    for name, kw in (("stage_adam", None), ("torch_foreach", dict(foreach=True)), ("torch_fused", dict(fused=True))):
        f = copy.deepcopy(field)
        g = torch.Generator(device="cuda").manual_seed(5)
        for p in f.parameters():
            p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3
        try:
            opt = StageAdam.for_field(f, **RATES) if kw is None else torch.optim.Adam(stage4d.field_param_groups(f, **RATES), lr=0.0, eps=1e-15, **kw)
            opt.step()
            torch.cuda.synchronize()
        except Exception as e:                                   # fused=True on a build without it
            left_out[name] = f"{type(e).__name__}: {str(e).splitlines()[0]}"
            continue
        made[name] = (f, opt)
    return made, left_out


def summary(ts):
    s = sorted(ts)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "calls": len(s)}


def bench_step(calls, block):
    field = deform4d.HexPlaneDeformation(use_global_trans=True).cuda()
    n_params = sum(p.numel() for p in field.parameters())
    made, left_out = optimisers(field)
    for _, opt in made.values():                                 # warm-up: code objects, torch's for-each plans
        for _ in range(10):
            opt.step()
    torch.cuda.synchronize()
    device_ms, host_us = {k: [] for k in made}, {k: [] for k in made}
    for r in range(-(-calls // block)):
        for name, (_, opt) in made.items():                      # alternating: a block of calls of each variant per round
            for _ in range(block):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                t0 = time.perf_counter()
                opt.step()
                host_us[name].append((time.perf_counter() - t0) * 1e6)
                e.record()
                torch.cuda.synchronize()
                device_ms[name].append(s.elapsed_time(e))
        if r % 5 == 0:
            print(f"[step round {r}] " + "  ".join(f"{k} {sorted(v[-block:])[block // 2] * 1e3:.1f} us" for k, v in device_ms.items()), flush=True)
    res = {"what": "optimiser step alone", "device": torch.cuda.get_device_name(0), "tensors": len(list(field.parameters())),
           "parameters": n_params, "bytes_moved": 28 * n_params, "left_out": left_out}
    for name in made:
        res[name + "_ms"] = summary(device_ms[name])
        res[name + "_host_enqueue_us"] = summary(host_us[name])
    return res


def bench_fit(n, side, rounds, iters):
    gaussians, field, batch = make_scene(n, side)
    graph = arap.ArapGraph(gaussians.xyz, K=3, radius=0.01)
    made, left_out = {}, {}
    for name, kw in (("stage_adam", None), ("torch_foreach", dict(foreach=True)), ("torch_fused", dict(fused=True))):
        f = copy.deepcopy(field)
        try:
            opt = StageAdam.for_field(f, **RATES) if kw is None else torch.optim.Adam(stage4d.field_param_groups(f, **RATES), lr=0.0, eps=1e-15, **kw)
        except Exception as e:
            left_out[name] = f"{type(e).__name__}: {str(e).splitlines()[0]}"
            continue
        made[name] = (f, opt, torch.Generator(device="cuda").manual_seed(1))
    kwargs = dict(loss=LOSS, n_view=N_VIEW, n_frame=N_FRAME, progressive_iter_per_frame=PROGRESSIVE, bg=BG, graph=graph)

    def one(name):
        f, opt, gen = made[name]
        return lambda: stage4d.fit(f, gaussians, batch, opt, steps=1, start_step=STEP, generator=gen, **kwargs)
    for name in list(made):
        try:
            one(name)()
            torch.cuda.synchronize()
        except Exception as e:
            left_out[name] = f"{type(e).__name__}: {str(e).splitlines()[0]}"
            del made[name]
    series = {k: [] for k in made}
    for r in range(rounds):
        for name in made:
            series[name].append(round(timed(one(name), iters), 3))
        print(f"[fit round {r}] " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in series.items()), flush=True)
    res = {"what": "one stage-1 fit step", "side": side, "gaussians": n, "images": N_VIEW * (N_FRAME - 1), "left_out": left_out}
    for name, ts in series.items():
        s = sorted(ts)
        res[name + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "rounds": ts}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=250)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage_optim.py needs the GPU: there is no CPU fallback and a CPU time would say nothing")
    print(json.dumps(bench_step(max(a.calls, 200), a.block)), flush=True)
    torch.cuda.empty_cache()
    print(json.dumps(bench_fit(a.n, a.side, a.rounds, a.iters)), flush=True)


if __name__ == "__main__":
    main()
