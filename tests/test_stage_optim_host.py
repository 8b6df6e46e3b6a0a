"""animate3d_amd.stage_optim without a GPU: ``scheduled`` against the values the reference's ``C`` returned, ``StageAdam.for_field``'s groups
and rates against the reference's ``training_setup`` / ``update_learning_rate`` (tests/golden/make_stage_optim_goldens.py), the state
dict's interchange with ``torch.optim.Adam``, what the constructor refuses, and what ``a3d_stage_adam_f32`` refuses before any launch.
The device addresses handed to the C-ABI are made up and never dereferenced: every call differs from a valid one in exactly one
argument (no call here may be valid: that would launch a kernel on made-up addresses)."""
import copy
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from animate3d_amd import deform4d, hip_ops, stage4d
from animate3d_amd.stage_optim import StageAdam, scheduled
from tests.golden.seeded import fill_named, seeded_tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_optim.npz")
A3D_EINVAL = -1
BASE = 0x7F00_0010_0000


@pytest.fixture(scope="module")
def golden():
    data = dict(np.load(GOLDEN))
    return data, json.loads(str(data["meta"]))


def _field(meta):
    field = deform4d.HexPlaneDeformation(tuple(tuple(r) for r in meta["grid"]), use_global_trans=True)
    return fill_named(field, meta["tag"], 0.2)


def test_scheduled_is_the_references_C(golden):
    _, meta = golden
    assert len(meta["c_cases"]) > 200
    kinds = set()
    for case in meta["c_cases"]:
        got = scheduled(case["value"], case["step"], case["interpolation"], epoch=case["epoch"])
        assert repr(float(got)) == case["want"], case
        kinds.add((len(case["value"]) if isinstance(case["value"], list) else 0, case["interpolation"]))
    assert kinds == {(n, i) for n in (0, 3, 4, 6, 8) for i in ("linear", "exp")}
    assert scheduled(3, 10) == 3 and isinstance(scheduled(3, 10), int) and scheduled(0.5, 10, "exp") == 0.5      # scalars pass through
    assert scheduled((0.01, 0.0001, 6), 3, "exp") == scheduled([0.01, 0.0001, 6], 3, "exp")                      # a tuple is a list
    assert scheduled([0, 1.0, 0.1, 3.5], 99, epoch=0) == 1.0 and scheduled([0, 1.0, 0.1, 3.5], 0, epoch=7) == 1.0 + (0.1 - 1.0) * 1.0  # a float end: the epoch


def test_scheduled_raises_what_C_raises():
    for bad in ("0.01", {"a": 1}, None):
        with pytest.raises(TypeError):
            scheduled(bad, 0)
    for bad in ([], [1.0], [1.0, 2.0], [0, 1.0, 2.0, 10, 3.0]):
        with pytest.raises(AssertionError):
            scheduled(bad, 0)
    with pytest.raises(ValueError, match="Unknown interpolation"):
        scheduled([0, 1.0, 2.0, 10], 5, "cosine")
    with pytest.raises(ValueError):                              # log of a zero rate, as in C
        scheduled([0, 0.0, 1.0, 10], 5, "exp")


def test_for_field_builds_the_references_groups_and_rates(golden):
    _, meta = golden
    field = _field(meta)
    opt = StageAdam.for_field(field, **meta["cfg"])
    names = {id(p): n for n, p in field.named_parameters()}
    assert [dict(name=g["name"], params=[names[id(p)] for p in g["params"]]) for g in opt.param_groups] == meta["groups"]
    assert [g["lr"] for g in opt.param_groups] == meta["lr0"]
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-15 for g in opt.param_groups)
    for k, want in enumerate(meta["lr"]):
        opt.update_learning_rate(k)
        assert [g["lr"] for g in opt.param_groups] == want, k
    assert len({tuple(w) for w in meta["lr"]}) == len(meta["lr"])                    # the list-valued rate moves every step
    plain = deform4d.HexPlaneDeformation(tuple(tuple(r) for r in meta["grid"]), use_global_trans=False)
    assert [g["name"] for g in StageAdam.for_field(plain, **meta["cfg"]).param_groups] == [g["name"] for g in meta["groups"][:4]]
    with pytest.raises(NotImplementedError, match="no schedule is built"):           # field_param_groups is as it was
        stage4d.field_param_groups(field, **meta["cfg"])


def test_state_exists_from_construction_on_and_never_moves(golden):
    _, meta = golden
    field = _field(meta)
    opt = StageAdam.for_field(field, **meta["cfg"])
    addresses = {}
    for p in field.parameters():
        st = opt.state[p]
        assert st["step"].shape == () and st["step"].dtype == torch.float32 and float(st["step"]) == 0.0
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
        addresses[id(p)] = tuple(st[k].data_ptr() for k in ("step", "exp_avg", "exp_avg_sq"))
    assert opt.skipped.shape == (1,) and opt.skipped.dtype == torch.int32
    opt.load_state_dict(opt.state_dict())
    assert all(addresses[id(p)] == tuple(opt.state[p][k].data_ptr() for k in ("step", "exp_avg", "exp_avg_sq")) for p in field.parameters())
    assert opt.step() is None                                    # no parameter has a gradient: nothing is launched, no device is needed


def _torch_adam(opt):
    return torch.optim.Adam([{k: g[k] for k in ("params", "lr", "name")} for g in opt.param_groups], lr=0.0, eps=1e-15)


def test_state_dict_interchange_with_torch_adam(golden):
    """Both directions on CPU tensors: torch's Adam takes two steps, ours loads its state; torch's Adam loads ours and goes on exactly
    as the one that never left."""
    _, meta = golden
    field = _field(meta)
    params = list(field.parameters())
    ours = StageAdam.for_field(field, **meta["cfg"])
    theirs = _torch_adam(ours)

    def take_step(optimizer, k):
        for n, p in field.named_parameters():
            p.grad = seeded_tensor(f"interchange/{k}/{n}", p.shape)
        optimizer.step()
    for k in range(2):
        take_step(theirs, k)
    ours.update_learning_rate(3)
    sd = theirs.state_dict()
    assert sd["param_groups"][3]["lr"] == meta["lr0"][3] != ours.param_groups[3]["lr"]
    ours.load_state_dict(sd)
    for p in params:
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(ours.state[p][key], theirs.state[p][key]) and ours.state[p][key] is not theirs.state[p][key]
        assert float(ours.state[p]["step"]) == 2.0 and ours.state[p]["step"].shape == ()
    assert [g["lr"] for g in ours.param_groups] == meta["lr0"] and [g["name"] for g in ours.param_groups] == [g["name"] for g in meta["groups"]]
    assert ours.param_groups[3]["schedule"] == meta["cfg"]["grid_lr"]                  # torch's groups carry none: ours is kept
    # our layout is torch's
    mine = ours.state_dict()
    assert set(mine) == {"state", "param_groups"} and sorted(mine["state"]) == list(range(len(params)))
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in mine["state"].values())
    assert all({"lr", "betas", "eps", "name", "params"} <= set(g) for g in mine["param_groups"])
    assert [i for g in mine["param_groups"] for i in g["params"]] == list(range(len(params)))
    # torch's Adam loads ours and continues as the original does
    keep = [p.detach().clone() for p in params]
    other = _torch_adam(ours)
    other.load_state_dict(copy.deepcopy(mine))                                        # torch's load keeps the tensors it is handed
    take_step(theirs, 2)
    want = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, k in zip(params, keep):
            p.copy_(k)
    take_step(other, 2)
    assert all(torch.equal(p, w) for p, w in zip(params, want))
    assert all(float(other.state[p]["step"]) == 3.0 for p in params)
    # a state that does not know a parameter (torch creates state lazily): ours starts that one from zero
    partial = theirs.state_dict()
    del partial["state"][0]
    ours.load_state_dict(partial)
    in_order = [p for g in ours.param_groups for p in g["params"]]                     # a state dict numbers them group by group
    assert float(ours.state[in_order[0]]["step"]) == 0.0 and not ours.state[in_order[0]]["exp_avg"].any()
    assert float(ours.state[in_order[1]]["step"]) == 3.0 and bool(ours.state[in_order[1]]["exp_avg"].any())
    with pytest.raises(ValueError):
        ours.load_state_dict(dict(sd, param_groups=sd["param_groups"][:4]))
    with pytest.raises(NotImplementedError):
        ours.load_state_dict(dict(sd, param_groups=[dict(g, weight_decay=0.1) for g in sd["param_groups"]]))


def test_constructor_refusals():
    """Every one without a device."""
    p, q = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(5))
    for option in ("weight_decay", "amsgrad", "maximize"):
        with pytest.raises(NotImplementedError, match=option):
            StageAdam([dict(params=[p], lr=0.1)], **{option: 0.1 if option == "weight_decay" else True})
        with pytest.raises(NotImplementedError, match=option):
            StageAdam([dict(params=[p], lr=0.1, **{option: 0.1 if option == "weight_decay" else True})])
    StageAdam([dict(params=[p], lr=0.1, weight_decay=0, amsgrad=False)], maximize=False)       # the values that mean "off" pass
    with pytest.raises(ValueError, match="more than one group"):
        StageAdam([dict(params=[p, q], lr=0.1), dict(params=[p], lr=0.2)])
    with pytest.raises(ValueError, match="more than one group"):
        StageAdam([dict(params=[p, p], lr=0.1)])
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float32"):
            StageAdam([dict(params=[torch.nn.Parameter(torch.zeros(3, dtype=dtype))], lr=0.1)])
    with pytest.raises(ValueError, match="non-contiguous"):
        StageAdam([dict(params=[torch.nn.Parameter(torch.zeros(4, 6).t())], lr=0.1)])
    with pytest.raises(ValueError, match="non-contiguous"):
        StageAdam([dict(params=[torch.zeros(4, 6)[:, ::2].requires_grad_(True)], lr=0.1)])
    for lr in (-0.1, math.nan, math.inf, [0, 0.01, 0.0001, 6]):
        with pytest.raises(ValueError, match="lr"):
            StageAdam([dict(params=[p], lr=lr)])
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999)):
        with pytest.raises(ValueError, match="betas"):
            StageAdam([dict(params=[p], lr=0.1)], betas=betas)
    with pytest.raises(ValueError, match="eps"):
        StageAdam([dict(params=[p], lr=0.1)], eps=-1e-8)
    with pytest.raises(ValueError):
        StageAdam([dict(params=[p])])
    with pytest.raises(TypeError, match="unknown options"):
        StageAdam([dict(params=[p], lr=0.1)], fused=True)
    opt = StageAdam([dict(params=[p], lr=0.1)])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    p.grad = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # a CPU parameter reaches no kernel and no torch arithmetic
        opt.step()
    assert float(opt.state[p]["step"]) == 0.0


# ---- the C-ABI: a3d_stage_adam_f32 refuses before any launch

FIELDS = ("p", "g", "m", "v", "step")
ALL_PHASES = hip_ops.STAGE_ADAM_BEGIN | hip_ops.STAGE_ADAM_CHECK | hip_ops.STAGE_ADAM_UPDATE


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build
    build.build(verbose=False)
    return hip_ops.load_library()


def _call(lib, count=3, entry=None, table="valid", beta1=0.9, beta2=0.999, eps=1e-15, phases=ALL_PHASES, flag=BASE + 0x800_0000, at=1):
    """The valid call of three tensors with entry ``at``'s fields, or one scalar argument, replaced.  Callers replace exactly one."""
    assert entry or table != "valid" or (count, beta1, beta2, eps, phases, flag) != (3, 0.9, 0.999, 1e-15, ALL_PHASES, BASE + 0x800_0000)
    arr = (hip_ops.StageAdamEntry * max(count, 1))()
    for t, e in enumerate(arr):
        for j, name in enumerate(FIELDS):
            setattr(e, name, BASE + 0x10_0000 * (len(FIELDS) * t + j))
        e.n, e.lr = 1000 + t, 0.01
    for name, value in (entry or {}).items():
        setattr(arr[at], name, value)
    return lib.a3d_stage_adam_f32(None, arr if table == "valid" else table, count, beta1, beta2, eps, phases, flag)


def test_cabi_capacity_is_stated_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "animate3d_hip.h")).read()
    assert f"#define A3D_STAGE_ADAM_MAX_TENSORS {hip_ops.STAGE_ADAM_MAX_TENSORS}\n" in header and hip_ops.STAGE_ADAM_MAX_TENSORS >= 32
    for name in ("BEGIN", "CHECK", "UPDATE"):
        assert f"#define A3D_STAGE_ADAM_{name} {getattr(hip_ops, 'STAGE_ADAM_' + name)}\n" in header
    assert ctypes.sizeof(hip_ops.StageAdamEntry) == 56 and "a3d_stage_adam_f32" in hip_ops.EXPORTED_SYMBOLS


def test_cabi_refuses_bad_counts_and_scalars(lib):
    cap = hip_ops.STAGE_ADAM_MAX_TENSORS
    for count in (0, -1, cap + 1, 2 * cap):
        assert _call(lib, count=count) == A3D_EINVAL, count
    assert _call(lib, table=None) == A3D_EINVAL
    for flag in (None, BASE + 2):
        assert _call(lib, flag=flag) == A3D_EINVAL, flag
    for phases in (0, -1, 8, ALL_PHASES + 1, 16 | ALL_PHASES):
        assert _call(lib, phases=phases) == A3D_EINVAL, phases
    for beta in (1.0, 1.5, -0.1, math.nan, math.inf, -math.inf):
        assert _call(lib, beta1=beta) == A3D_EINVAL, beta
        assert _call(lib, beta2=beta) == A3D_EINVAL, beta
    for eps in (-1e-15, -1.0, math.nan, math.inf):
        assert _call(lib, eps=eps) == A3D_EINVAL, eps


def test_cabi_refuses_bad_entries(lib):
    for at in (0, 1, 2):                                         # the first, a middle and the last entry
        for name in FIELDS:
            assert _call(lib, entry={name: None}, at=at) == A3D_EINVAL, (at, name, "NULL")
            for off in (1, 2, 3):
                ptr = BASE + 0x10_0000 * (len(FIELDS) * at + FIELDS.index(name)) + off
                assert _call(lib, entry={name: ptr}, at=at) == A3D_EINVAL, (at, name, off)
        for n in (0, -1, -2 ** 40):
            assert _call(lib, entry=dict(n=n), at=at) == A3D_EINVAL, (at, n)
        for lr in (-1e-9, -1.0, math.nan, math.inf, -math.inf):
            assert _call(lib, entry=dict(lr=lr), at=at) == A3D_EINVAL, (at, lr)
    assert _call(lib, entry=dict(n=2 ** 42), at=1) == A3D_EINVAL         # more blocks than a grid has
    assert _call(lib, count=1, entry=dict(g=None), at=0) == A3D_EINVAL   # a single tensor
    assert _call(lib, count=hip_ops.STAGE_ADAM_MAX_TENSORS, entry=dict(v=None), at=hip_ops.STAGE_ADAM_MAX_TENSORS - 1) == A3D_EINVAL
