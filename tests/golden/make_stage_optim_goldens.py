"""Generate tests/golden/stage_optim.npz by running the REFERENCE's own schedule and optimiser set-up on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_stage_optim_goldens.py <path to the reference tree>

``C`` of threestudio/utils/misc.py and ``training_setup``, ``update_learning_rate`` and the five ``get_*_parameters`` of
``Gaussian4DModel`` (custom/threestudio-animate3d/geometry/gaussian_4d.py) are taken out of the reference files through the syntax tree
and executed as they lie; the modules import threestudio, tinycudann and the rasterizer at their top, so only these definitions are
executed, against stubs.  ``config_to_primitive`` hands a list back as it is.  The model is a class that holds those seven methods over
``animate3d_amd.deform4d.HexPlaneDeformation(((2, 2, 2, 2), (3, 3, 3, 2)), use_global_trans=True)``, which carries the reference's
parameter names; its ``cfg`` holds the released rates with a list-valued ``grid_lr``.  Only data is written:

(a) ``c_cases`` (json): every case of ``c_cases()`` below with the value the reference's ``C`` returned (``repr`` of the float: exact);
(b) the group names and their parameter names, every group's ``lr`` at every step, and after each of 4 steps of the reference's
    ``torch.optim.Adam`` (gradients ``seeded_tensor(f"stage_optim/grad/{step}/{name}")``, stored as seeds, not values) every parameter,
    ``exp_avg`` and ``exp_avg_sq``, and ``ref_err``: the reference's element-wise deviation from tests/stage_optim_ref.py's float64
    restatement advanced from the reference's own previous state (fp32, rounded up)."""
import ast
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from animate3d_amd.deform4d import HexPlaneDeformation  # noqa: E402
from tests import stage_optim_ref as R  # noqa: E402
from tests.golden.seeded import fill_named, seeded_tensor  # noqa: E402

GRID = ((2, 2, 2, 2), (3, 3, 3, 2))
STEPS = 4
TAG = "stage_optim"
CFG = dict(delta_xyz_network_lr=0.0001, delta_rot_network_lr=0.0001, delta_scaling_network_lr=0.0001, grid_lr=[0, 0.01, 0.0001, 6],
           global_trans_lr=0.001, use_global_trans=True, pred_normal=False, color_clip=2.0)
METHODS = ("get_xyz_mlp_parameters", "get_rot_mlp_parameters", "get_scaling_mlp_parameters", "get_global_trans_parameters",
           "get_grid_parameters", "training_setup", "update_learning_rate")

# every rate of the released configs (scalars, and the one list: position_lr of visualize_four_view_static.yaml); 3-, 4- and 6-element
# lists (8 as well); steps before, inside, at and after the interval; a float end_step, which reads the epoch
RELEASED = [0.0001, 0.01, 0.001, 0.05, 0.005, [0, 0.001, 0.00002, 1000]]
LISTS = [[0.01, 0.0001, 6], [10, 0.01, 0.0001, 30], [0, 0.001, 0.00002, 1000], [5, 1.0, 0.5, 20, 0.25, 40], [0, 0.1, 0.01, 100, 0.001, 200, 0.0001, 300],
         [0, 1.0, 0.1, 3.5]]
STEPS_AT = [0, 1, 5, 6, 10, 19, 20, 21, 30, 40, 41, 100, 150, 200, 250, 300, 999, 1000, 1001]
EPOCHS_AT = [0, 1, 3, 4]


def c_cases():
    cases = []
    for value in RELEASED[:5]:
        cases += [dict(value=value, step=s, epoch=0, interpolation=i) for s in (0, 500) for i in ("linear", "exp")]
    for value in LISTS:
        for interpolation in ("linear", "exp"):
            if isinstance(value[-1], float):
                cases += [dict(value=value, step=7, epoch=e, interpolation=interpolation) for e in EPOCHS_AT]
            else:
                cases += [dict(value=value, step=s, epoch=0, interpolation=interpolation) for s in STEPS_AT]
    return cases


def function_def(path, name):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(body) == 1, name
    return ast.fix_missing_locations(ast.Module(body=body, type_ignores=[]))


def methods_of(path, cls, names):
    tree = ast.parse(open(path).read())
    (node,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls]
    body = [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    holder = ast.ClassDef(name=cls, bases=[ast.Name(id="Base", ctx=ast.Load())], keywords=[], body=body, decorator_list=[])
    return ast.fix_missing_locations(ast.Module(body=[holder], type_ignores=[]))


def f32(t):
    return t.detach().numpy().astype(np.float32)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    ns = dict(math=__import__("math"), Any=object, config_to_primitive=lambda value: value, torch=torch, Base=HexPlaneDeformation)
    exec(compile(function_def(os.path.join(ref, "threestudio", "utils", "misc.py"), "C"), "misc.py", "exec"), ns)
    exec(compile(methods_of(os.path.join(ref, "custom", "threestudio-animate3d", "geometry", "gaussian_4d.py"), "Gaussian4DModel", METHODS),
                 "gaussian_4d.py", "exec"), ns)
    C = ns["C"]
    out, meta = {}, {}

    cases = c_cases()
    for case in cases:
        case["want"] = repr(float(C(case["value"], case["epoch"], case["step"], interpolation=case["interpolation"])))
    meta["c_cases"] = cases

    model = ns["Gaussian4DModel"](GRID, use_global_trans=True)
    fill_named(model, TAG, 0.2)
    model.cfg = types.SimpleNamespace(**CFG)
    model.training_setup()
    names = {id(p): n for n, p in model.named_parameters()}
    meta["groups"] = [dict(name=g["name"], params=[names[id(p)] for p in g["params"]]) for g in model.optimizer.param_groups]
    meta["cfg"] = {k: v for k, v in CFG.items() if k.endswith("_lr")}
    meta["lr0"] = [g["lr"] for g in model.optimizer.param_groups]
    meta["lr"], meta["steps"], meta["grid"], meta["tag"] = [], STEPS, GRID, TAG
    worst = dict(p=0.0, m=0.0, v=0.0)
    for k in range(STEPS):
        model.update_learning_rate(k)
        meta["lr"].append([g["lr"] for g in model.optimizer.param_groups])
        before = {}
        for group in model.optimizer.param_groups:
            for p in group["params"]:
                p.grad = seeded_tensor(f"{TAG}/grad/{k}/{names[id(p)]}", p.shape)
                st = model.optimizer.state.get(p, {})
                zeros = np.zeros(tuple(p.shape), np.float32)
                before[id(p)] = (f32(p), f32(p.grad), f32(st["exp_avg"]) if st else zeros, f32(st["exp_avg_sq"]) if st else zeros,
                                 float(st["step"]) if st else 0.0, group["lr"])
        model.optimizer.step()
        for p in model.parameters():
            name, st = names[id(p)], model.optimizer.state[p]
            assert float(st["step"]) == k + 1
            pb, gb, mb, vb, step, lr = before[id(p)]
            after = dict(p=f32(p), m=f32(st["exp_avg"]), v=f32(st["exp_avg_sq"]))
            exact = dict(zip("pmv", R.adam_step(pb, gb, mb, vb, step, lr)[:3]))
            for q in "pmv":
                out[f"s{k}/{q}/{name}"] = after[q]
                err = R.deviation(after[q], exact[q])
                err32 = err.astype(np.float32)                   # stored as fp32, rounded up: still the reference's deviation at least
                out[f"s{k}/ref_err_{q}/{name}"] = np.where(err32.astype(np.float64) < err, np.nextafter(err32, np.float32(np.inf)), err32)
                bar = dict(zip("pmv", R.bars(pb, gb, mb, vb, *R.adam_step(pb, gb, mb, vb, step, lr))))[q]
                worst[q] = max(worst[q], float((out[f"s{k}/ref_err_{q}/{name}"] / np.maximum(bar, 1e-300)).max()))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "stage_optim.npz")
    np.savez_compressed(path, **out)
    print(len(cases), "cases of C;", STEPS, "steps;", os.path.getsize(path), "bytes")
    print("groups", [(g["name"], len(g["params"])) for g in meta["groups"]], "lr per step", meta["lr"])
    print("the reference's own deviation / the kernel's bar, worst element:", {k: f"{v:.3g}" for k, v in worst.items()})


if __name__ == "__main__":
    main()
