"""animate3d_amd.stage_optim and ``stage4d.fit`` on the GPU: the Adam kernel (csrc/stage_optim.hip) against the float64 restatement of
tests/stage_optim_ref.py (the bars are derived there), its per-tensor rules, the dropped step, its bitwise and host-independence
guarantees, the reference's own optimiser run (tests/golden/make_stage_optim_goldens.py), and the loop against the same steps written
out by hand.  Where two runs of this package are compared the bar is equality: no kernel of the stage has an order of its own."""
import copy
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from animate3d_amd import arap, cameras, deform4d, hip_ops, stage4d
from animate3d_amd.stage_optim import StageAdam
from tests import gs_ref
from tests import stage4d_ref
from tests import stage_optim_ref as R
from tests.golden.seeded import fill_named, seeded_tensor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_optim.npz")
CAPACITY = hip_ops.STAGE_ADAM_MAX_TENSORS
SEAM_SIZES = (1, 3, 255, 256, 257, 1023, 1025, 65537)            # around the 256-thread block and the 1 024-element chunk, and many chunks
RATES = (1e-3, 2e-2)


def _np(t):
    return t.detach().cpu().numpy()


def _offset_view(values: np.ndarray) -> torch.Tensor:
    """A contiguous device tensor that starts 4 bytes into its storage."""
    base = torch.zeros(values.size + 1, device="cuda")
    base[1:] = torch.from_numpy(values).cuda()
    view = base[1:]
    assert view.storage_offset() == 1 and view.data_ptr() % 8 == 4
    return view


def _make_params(key, sizes, offset_at=None):
    params = []
    for i, n in enumerate(sizes):
        values = R.make_params(f"{key}/{i}", n)
        t = _offset_view(values) if i == offset_at else torch.from_numpy(values).cuda()
        params.append(t.detach().requires_grad_(True))
    return params


def _set_grads(key, params, offset_at=None):
    for i, p in enumerate(params):
        values = R.make_grads(f"{key}/{i}", p.numel())
        p.grad = _offset_view(values) if i == offset_at else torch.from_numpy(values).cuda()


def _two_groups(params):
    return [dict(params=params[0::2], lr=RATES[0], name="even"), dict(params=params[1::2], lr=RATES[1], name="odd")]


def _state(opt, params):
    """(p, m, v, step) of every parameter, cloned."""
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["step"].clone()) for p in params]


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for s, t in zip(a, b) for x, y in zip(s, t))


# ---- parity against float64

@pytest.mark.parametrize("case", ["seams", "single", "over_capacity"])
def test_three_steps_against_float64(case):
    """Every step is compared from the kernel's own fp32 state before it.  ``seams``: the eight sizes in one call, the 257-element tensor
    and its gradient both starting 4 bytes into their storage; ``single``: one tensor; ``over_capacity``: capacity + 1 tensors of 5
    elements, which takes a second call."""
    sizes, offset_at = {"seams": (SEAM_SIZES, 4), "single": ((1025,), None), "over_capacity": ((5,) * (CAPACITY + 1), None)}[case]
    params = _make_params(case, sizes, offset_at)
    opt = StageAdam(_two_groups(params))
    lr_of = {id(p): g["lr"] for g in opt.param_groups for p in g["params"]}
    failures = []
    for k in range(3):
        _set_grads(f"{case}/{k}", params, offset_at)
        before = _state(opt, params)
        opt.step()
        assert int(opt.skipped) == 0
        for i, (p, (p0, m0, v0, s0)) in enumerate(zip(params, before)):
            assert float(s0) == k and float(opt.state[p]["step"]) == k + 1
            st = opt.state[p]
            R.check_step(f"{case} tensor {i} [{p.numel()}]", (_np(p0), _np(p.grad), _np(m0), _np(v0)),
                         (_np(p), _np(st["exp_avg"]), _np(st["exp_avg_sq"])), k, lr_of[id(p)], failures, verbose=len(sizes) <= 8)
    assert not failures, failures


def test_per_tensor_rules():
    """One call: a parameter without a gradient keeps its bits and its step; a group at rate 0 keeps p while m, v and step move; a zero
    gradient on zero moments leaves p as it is; two groups get a rate each."""
    idle, frozen, still, slow, fast = params = _make_params("rules", (300, 1025, 77, 513, 513))
    with torch.no_grad():
        fast.copy_(slow)
    opt = StageAdam([dict(params=[idle, slow], lr=1e-3), dict(params=[frozen], lr=0.0), dict(params=[still, fast], lr=5e-2)])
    _set_grads("rules", params)
    idle.grad = None
    still.grad = torch.zeros_like(still)
    fast.grad = slow.grad.clone()
    before = _state(opt, params)
    opt.step()
    after = _state(opt, params)
    assert int(opt.skipped) == 0
    assert _same_bits(before[:1], after[:1]) and float(opt.state[idle]["step"]) == 0.0
    assert _same_bits([before[1][:1]], [after[1][:1]]) and float(after[1][3]) == 1.0            # rate 0: p bit for bit
    assert not torch.equal(before[1][1], after[1][1]) and not torch.equal(before[1][2], after[1][2])
    assert _same_bits([before[2][:3]], [after[2][:3]]) and float(after[2][3]) == 1.0 and not after[2][1].any()
    failures = []
    for name, i, lr in (("slow", 3, 1e-3), ("fast", 4, 5e-2), ("frozen", 1, 0.0)):
        R.check_step(name, tuple(_np(t) for t in (before[i][0], params[i].grad, before[i][1], before[i][2])),
                     tuple(_np(t) for t in after[i][:3]), 0, lr, failures)
    assert not failures, failures
    assert torch.equal(after[3][1], after[4][1]) and torch.equal(after[3][2], after[4][2])     # the same gradient: the same moments
    moved_slow, moved_fast = (before[3][0] - after[3][0]).abs(), (before[4][0] - after[4][0]).abs()
    nonzero = slow.grad != 0
    assert bool((moved_fast[nonzero] > 10 * moved_slow[nonzero]).all()) and bool((moved_slow[nonzero] > 0).all())


# ---- the dropped step

def _skip_setup(key, sizes):
    params = _make_params(key, sizes)
    opt = StageAdam(_two_groups(params))
    _set_grads(f"{key}/warm", params)
    opt.step()                                                   # moments and steps that are not zero
    assert int(opt.skipped) == 0
    return params, opt


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf], ids=["nan", "inf", "-inf"])
def test_a_non_finite_gradient_drops_the_step(bad, where):
    """Non-finite numbers go through arithmetic; nothing here can fault."""
    params, opt = _skip_setup("skip", (1025, 3, 65537, 257))
    before = _state(opt, params)
    _set_grads("skip/bad", params)
    target = params[0].grad if where == "first" else params[-1].grad
    target[0 if where == "first" else -1] = bad
    opt.step()
    assert int(opt.skipped) == 1
    assert _same_bits(before, _state(opt, params))
    assert all(float(opt.state[p]["step"]) == 1.0 for p in params)
    # the clean step that follows is the step a copy of that state takes
    twins = [p.detach().clone().requires_grad_(True) for p in params]
    twin = StageAdam(_two_groups(twins))
    twin.load_state_dict(opt.state_dict())
    _set_grads("skip/clean", params)
    for p, t in zip(params, twins):
        t.grad = p.grad.clone()
    opt.step()
    twin.step()
    assert int(opt.skipped) == 0 and int(twin.skipped) == 0       # the flag needs no reset
    assert _same_bits(_state(opt, params), _state(twin, twins))
    assert all(float(opt.state[p]["step"]) == 2.0 for p in params) and not _same_bits(before, _state(opt, params))


def test_a_non_finite_gradient_in_the_second_call_keeps_the_first_call_too():
    params, opt = _skip_setup("skip_over", (5,) * (CAPACITY + 1))
    before = _state(opt, params)
    _set_grads("skip_over/bad", params)
    params[-1].grad[-1] = math.nan
    opt.step()
    assert int(opt.skipped) == 1 and _same_bits(before, _state(opt, params))
    _set_grads("skip_over/clean", params)
    opt.step()
    after = _state(opt, params)
    assert int(opt.skipped) == 0 and all(float(s[3]) == 2.0 for s in after)
    assert all(not torch.equal(b[0], a[0]) for b, a in zip(before, after))


# ---- reproducibility and synchronisation

def test_bitwise_reproducible_order_free_and_no_host_sync():
    sizes = (1025, 3, 65537, 257, 256)
    runs = []
    for order in (list(range(len(sizes))), list(range(len(sizes))), [3, 0, 4, 2, 1]):
        params = _make_params("repro", sizes)
        lr = {i: RATES[i % 2] for i in range(len(sizes))}
        groups = [dict(params=[params[i] for i in order if lr[i] == rate], lr=rate) for rate in RATES]
        if order[0] != 0:
            groups.reverse()
        opt = StageAdam(groups)
        for k in range(2):
            _set_grads(f"repro/{k}", params)
            opt.step()
        runs.append(_state(opt, params))
    assert _same_bits(runs[0], runs[1])                          # two optimisers from one state
    assert _same_bits(runs[0], runs[2])                          # another order of the parameters and the groups
    params = _make_params("sync", sizes)
    opt = StageAdam([dict(params=params[:2], lr=1e-3, schedule=[0, 1e-3, 1e-5, 10], name="a"), dict(params=params[2:], lr=1e-2, name="b")])
    _set_grads("sync/0", params)
    opt.step()                                                   # loads the library and the kernels outside the guarded region
    _set_grads("sync/1", params)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        opt.update_learning_rate(5)
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert int(opt.skipped) == 0 and all(float(opt.state[p]["step"]) == 2.0 for p in params)
    assert opt.param_groups[0]["lr"] == math.exp(math.log(1e-3) * 0.5 + math.log(1e-5) * 0.5)


# ---- the reference's optimiser

@pytest.fixture(scope="module")
def golden():
    data = dict(np.load(GOLDEN))
    return data, json.loads(str(data["meta"]))


def test_the_references_four_steps(golden):
    data, meta = golden
    field = fill_named(deform4d.HexPlaneDeformation(tuple(tuple(r) for r in meta["grid"]), use_global_trans=True), meta["tag"], 0.2).cuda()
    named = dict(field.named_parameters())
    opt = StageAdam.for_field(field, **meta["cfg"])
    in_order = [n for g in meta["groups"] for n in g["params"]]
    group_of = {n: gi for gi, g in enumerate(meta["groups"]) for n in g["params"]}
    initial = {n: p.detach().clone() for n, p in named.items()}
    failures, torch_worst = [], dict(p=0.0, m=0.0, v=0.0)
    for k in range(1, meta["steps"] + 1):
        # the reference's state after step k - 1, through load_state_dict
        state = {}
        with torch.no_grad():
            for i, n in enumerate(in_order):
                if k == 1:
                    named[n].copy_(initial[n])
                    continue
                named[n].copy_(torch.from_numpy(data[f"s{k - 2}/p/{n}"]))
                state[i] = dict(step=torch.tensor(float(k - 1)), exp_avg=torch.from_numpy(data[f"s{k - 2}/m/{n}"]),
                                exp_avg_sq=torch.from_numpy(data[f"s{k - 2}/v/{n}"]))
        opt.load_state_dict(dict(state=state, param_groups=opt.state_dict()["param_groups"]))
        for n, p in named.items():
            p.grad = seeded_tensor(f"{meta['tag']}/grad/{k - 1}/{n}", p.shape).cuda()
        before = {n: (_np(p), _np(p.grad), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"])) for n, p in named.items()}
        opt.update_learning_rate(k - 1)
        assert [g["lr"] for g in opt.param_groups] == meta["lr"][k - 1]
        opt.step()
        assert int(opt.skipped) == 0
        for n, p in named.items():
            st = opt.state[p]
            assert float(st["step"]) == k
            after = (_np(p), _np(st["exp_avg"]), _np(st["exp_avg_sq"]))
            lr = meta["lr"][k - 1][group_of[n]]
            R.check_step(f"golden step {k} {n}", before[n], after, k - 1, lr, failures, verbose=False)          # the float64 restatement
            p1, m1, v1, u = R.adam_step(*before[n], k - 1, lr)
            for q, got, bar in zip("pmv", after, R.bars(*before[n], p1, m1, v1, u)):                          # the reference's record
                dev = R.deviation(got, data[f"s{k - 1}/{q}/{n}"].astype(np.float64))
                allow = bar + data[f"s{k - 1}/ref_err_{q}/{n}"].astype(np.float64)
                if not (dev <= allow).all():
                    failures.append((f"golden step {k} {n} against the reference", q, float((dev / np.maximum(allow, 1e-300)).max())))
        # one more step from our state, ours and torch's own Adam on the device
        twin = copy.deepcopy(field)
        twin_named = dict(twin.named_parameters())
        theirs = torch.optim.Adam([dict(params=[twin_named[n] for n in g["params"]], lr=0.0, name=g["name"]) for g in meta["groups"]],
                                  lr=0.0, eps=1e-15)
        theirs.load_state_dict(copy.deepcopy(opt.state_dict()))      # torch's load keeps the tensors it is handed: a copy, not ours
        assert [g["lr"] for g in theirs.param_groups] == meta["lr"][k - 1]
        for n, p in named.items():
            p.grad = seeded_tensor(f"{meta['tag']}/extra/{k}/{n}", p.shape).cuda()
            twin_named[n].grad = p.grad.clone()
        before = {n: (_np(p), _np(p.grad), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"])) for n, p in named.items()}
        opt.step()
        theirs.step()
        for n, p in named.items():
            lr = meta["lr"][k - 1][group_of[n]]
            p1, m1, v1, u = R.adam_step(*before[n], k, lr)
            tp = twin_named[n]
            pairs = ((p, tp, p1), (opt.state[p]["exp_avg"], theirs.state[tp]["exp_avg"], m1), (opt.state[p]["exp_avg_sq"], theirs.state[tp]["exp_avg_sq"], v1))
            for q, (mine, torchs, exact), bar in zip("pmv", pairs, R.bars(*before[n], p1, m1, v1, u)):
                torch_dev = R.deviation(_np(torchs), exact)        # torch's own deviation from float64 on this step, measured
                torch_worst[q] = max(torch_worst[q], float((torch_dev / np.maximum(bar, 1e-300)).max()))
                dev = R.deviation(_np(mine), _np(torchs).astype(np.float64))
                if not (dev <= bar + torch_dev).all():
                    failures.append((f"golden step {k} {n} against torch.optim.Adam", q, float((dev / np.maximum(bar + torch_dev, 1e-300)).max())))
            assert float(opt.state[p]["step"]) == float(theirs.state[tp]["step"]) == k + 1
    print("[stage_optim golden] torch.optim.Adam on the device, worst deviation from float64 / the kernel's bar: "
          + "  ".join(f"{q} {v:.3g}" for q, v in torch_worst.items()))
    assert not failures, failures[:10]


# ---- the loop

N_VIEW, N_FRAME, SIDE, N_GAUSS, PROGRESSIVE = 2, 4, 16, 64, 1
GRID = ((6, 5, 7, 3), (12, 10, 14, 6))
FIELD_RATES = dict(delta_xyz_network_lr=1e-4, delta_rot_network_lr=1e-4, delta_scaling_network_lr=1e-4, grid_lr=[0, 0.01, 0.0001, 6],
                   global_trans_lr=1e-3)


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(21)
    xyz = (torch.randn(N_GAUSS, 3, generator=g) * 0.5).cuda()
    gaussians = stage4d.Gaussians(xyz=xyz, scaling=(torch.rand(N_GAUSS, 3, generator=g) * 1.0 - 2.5).cuda(),
                                  rotation=torch.randn(N_GAUSS, 4, generator=g).cuda(),
                                  opacity=torch.sigmoid(torch.randn(N_GAUSS, 1, generator=g) * 1.5).cuda(),
                                  shs=(torch.randn(N_GAUSS, 16, 3, generator=g) * 0.3).cuda(), sh_degree=3)
    field = deform4d.HexPlaneDeformation(GRID, use_global_trans=True)
    with torch.no_grad():                                        # the reference's zero last layers give zero gradient to everything before them
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    views = torch.stack([gs_ref.look_at((3.5 * math.cos(a), 3.5 * math.sin(a), 0.3)) for a in (0.0, math.pi / 2)])
    S = N_VIEW * N_FRAME
    batch = dict(c2w=views[:, None].expand(N_VIEW, N_FRAME, 4, 4).reshape(S, 4, 4).cuda().contiguous(),
                 fovy=torch.full((S,), math.radians(40.0), device="cuda"), timestamps=torch.linspace(-1, 1, N_FRAME).repeat(N_VIEW).cuda(),
                 rgb=torch.rand(S, SIDE, SIDE, 3, generator=g).cuda(), mask=(torch.rand(S, SIDE, SIDE, 1, generator=g) > 0.5).cuda())
    loss = dict(stage4d_ref.LOSS, arap_sample_num=32)            # fewer samples than Gaussians: ARAP draws from the generator
    kwargs = dict(loss=loss, n_view=N_VIEW, n_frame=N_FRAME, progressive_iter_per_frame=PROGRESSIVE, bg=stage4d_ref.BG,
                  graph=arap.ArapGraph(xyz, K=3))
    return dict(gaussians=gaussians, field=field.cuda(), batch=batch, kwargs=kwargs)


def _guidance(rgb):                                              # a stand-in: a sum of the render
    return (rgb * rgb).sum()


def _run(scene, steps, by_hand=False, guided=False, segments=None, torch_adam=False, guidance=None):
    """A fresh copy of the field, a fresh optimiser and fresh generators; the loop through ``fit`` (in ``segments``) or written out."""
    field = copy.deepcopy(scene["field"])
    if torch_adam:
        opt = torch.optim.Adam(stage4d.field_param_groups(field, **dict(FIELD_RATES, grid_lr=0.01)), lr=0.0, eps=1e-15)
    else:
        opt = StageAdam.for_field(field, **FIELD_RATES)
    gen, rng = torch.Generator(device="cuda").manual_seed(33), random.Random(4)
    kwargs = dict(scene["kwargs"])
    sampler = None
    if guided:
        kwargs["guidance"] = guidance or _guidance
        sampler = cameras.RandomCameraSampler(batch_size=N_VIEW * N_FRAME, n_view=N_VIEW, total_frame=N_FRAME, height=SIDE, width=SIDE,
                                              progressive_until=4, device="cuda")
    logs = []
    if by_hand:
        for s in range(steps):
            batch = dict(scene["batch"])
            if sampler is not None:
                sampler.update_step(s)
                batch["random_camera"] = sampler.sample(gen, rng=rng)
            opt.update_learning_rate(s)
            opt.zero_grad(set_to_none=True)
            out = stage4d.training_step(field, scene["gaussians"], batch, global_step=s, generator=gen, rng=rng, **kwargs)
            out["loss"].backward()
            opt.step()
            logs.append({**{k: v.detach().clone() for k, v in out.items()}, "skipped": opt.skipped.clone()})
        log = {k: torch.stack([entry[k].reshape(()).float() for entry in logs]) for k in logs[0]}
    else:
        parts, start = [], 0
        for n in segments or [steps]:
            parts.append(stage4d.fit(field, scene["gaussians"], scene["batch"], opt, steps=n, start_step=start, sampler=sampler, generator=gen,
                                     rng=rng, **kwargs))
            assert all(v.shape == (n,) and v.dtype == torch.float32 and v.is_cuda for v in parts[-1].values())
            start += n
        log = {k: torch.cat([part[k] for part in parts]) for k in parts[0]}
    state = [(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"]) for p in field.parameters()]
    return field, state, log


@pytest.mark.parametrize("guided", [False, True], ids=["stage1", "guided"])
def test_fit_is_the_loop_written_out(scene, guided):
    """Three steps of stage 1 with ARAP (and once more with a guidance stand-in and a ``RandomCameraSampler``): parameters, optimiser state
    and every logged term, bit for bit."""
    field_a, state_a, log_a = _run(scene, 3, guided=guided)
    field_b, state_b, log_b = _run(scene, 3, guided=guided, by_hand=True)
    assert _same_bits(state_a, state_b)
    want = {"loss", "loss_rgb", "loss_mask", "loss_arap", "skipped"} | ({"loss_sds"} if guided else set())
    assert set(log_a) == set(log_b) == want
    for key in want:
        assert torch.equal(log_a[key].view(torch.int32), log_b[key].view(torch.int32)), key
        assert bool(torch.isfinite(log_a[key]).all()), key
    assert not log_a["skipped"].any() and all(float(s[3]) == 3.0 for s in state_a)
    moved = {n: not torch.equal(p, q) for (n, p), q in zip(field_a.named_parameters(), scene["field"].parameters())}
    assert all(moved[n] for n in moved if guided or not n.startswith("delta_scaling_network")), moved      # stage 1 does not deform the scales


def test_fit_in_segments_is_fit_in_one_piece(scene):
    _, whole, log_whole = _run(scene, 5)
    _, parts, log_parts = _run(scene, 5, segments=[3, 2])
    assert _same_bits(whole, parts) and all(float(s[3]) == 5.0 for s in whole)
    assert set(log_whole) == set(log_parts) and all(torch.equal(log_whole[k], log_parts[k]) for k in log_whole)
    assert len({float(v) for v in log_whole["loss"]}) == 5


def test_fit_with_torch_adam_and_with_a_non_finite_guidance(scene):
    _, _, log = _run(scene, 2, torch_adam=True)
    assert set(log) == {"loss", "loss_rgb", "loss_mask", "loss_arap"} and bool(torch.isfinite(log["loss"]).all())
    # a guidance whose gradient is not finite: every step is dropped, on the device, and the field stays as it was
    field, state, log = _run(scene, 2, guided=True, guidance=lambda rgb: _guidance(rgb) * math.inf)
    assert log["skipped"].tolist() == [1.0, 1.0] and all(float(s[3]) == 0.0 and not s[1].any() for s in state)
    assert all(torch.equal(p, q) for p, q in zip(field.parameters(), scene["field"].parameters()))
    with pytest.raises(ValueError):
        stage4d.fit(field, scene["gaussians"], scene["batch"], None, steps=0, **scene["kwargs"])
    with pytest.raises(TypeError):
        stage4d.fit(field, scene["gaussians"], scene["batch"], None, steps=1, global_step=3, **scene["kwargs"])
