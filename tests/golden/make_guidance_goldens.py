"""Generate tests/golden/guidance.json by running the REFERENCE's own timestep-range methods on the CPU.

Run in the build container only (needs the reference tree):

    python -B tests/golden/make_guidance_goldens.py <path to the reference tree>

``set_min_max_steps`` and ``update_step`` of ``AnimateMVDiffusionGuidance`` (custom/threestudio-animate3d/guidance/animatemv_guidance.py)
and ``C`` of threestudio/utils/misc.py are taken out of the reference files through the syntax tree and executed as they lie (without
their decorators: ``autocast(enabled=False)`` does nothing to integer arithmetic); the modules import diffusers and threestudio at their
top, so only these definitions are executed, over a holder that has ``cfg`` and ``num_train_timesteps``.  Only numbers are written: every
case of ``cases()`` with the ``min_step`` / ``max_step`` the reference left behind."""
import ast
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

ANNEAL_LIST = [0, 0.98, 0.02, 10000]                      # the schedule the released configs carry in their comment
# (min_step_percent, max_step_percent) of every released config with a guidance block, and the class defaults
RELEASED = [(0.02, 0.2), (0.02, [1000, 0.98, 0.5, 1001]), (0.02, 0.98)]
# percents that are not exact in binary (100 p falls below 29, 57, 58).  1000 p rounds back to 290, 570, 580 exactly, so int() does not
# bite here (no three-decimal percent makes it bite at 1000 timesteps); it does on the interpolated values of the list schedules
INEXACT = [0.29, 0.57, 0.58]


def cases():
    out = []
    for lo, hi in RELEASED:
        out += [dict(min_step_percent=lo, max_step_percent=hi, step=s) for s in (0, 1, 199, 999, 1000, 1001, 5000)]
    out += [dict(min_step_percent=ANNEAL_LIST, max_step_percent=0.98, step=s) for s in (0, 1, 5000, 9999, 10000, 20000)]
    out += [dict(min_step_percent=0.02, max_step_percent=ANNEAL_LIST, step=s) for s in (0, 1, 5000, 9999, 10000, 20000)]
    for hi in (0.98, [0, 0.98, 0.5, 5000]):
        for lo in (0.02, ANNEAL_LIST):
            out += [dict(min_step_percent=lo, max_step_percent=hi, sqrt_anneal=True, trainer_max_steps=25000, step=s)
                    for s in (0, 1, 100, 6250, 12345, 25000)]
    for p in INEXACT:
        out += [dict(min_step_percent=p, max_step_percent=0.98, step=0), dict(min_step_percent=0.02, max_step_percent=p, step=0)]
    for case in out:
        case.setdefault("sqrt_anneal", False)
        case.setdefault("trainer_max_steps", 25000)
        case.setdefault("epoch", 0)
    return out


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
    for n in body:
        n.decorator_list = []
    holder = ast.ClassDef(name=cls, bases=[], keywords=[], body=body, decorator_list=[])
    return ast.fix_missing_locations(ast.Module(body=[holder], type_ignores=[]))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["ANIMATE3D_REFERENCE"]
    ns = dict(math=__import__("math"), Any=object, config_to_primitive=lambda value: value)
    exec(compile(function_def(os.path.join(ref, "threestudio", "utils", "misc.py"), "C"), "misc.py", "exec"), ns)
    exec(compile(methods_of(os.path.join(ref, "custom", "threestudio-animate3d", "guidance", "animatemv_guidance.py"),
                            "AnimateMVDiffusionGuidance", ("set_min_max_steps", "update_step")), "animatemv_guidance.py", "exec"), ns)
    done = []
    for case in cases():
        g = ns["AnimateMVDiffusionGuidance"]()
        g.num_train_timesteps = 1000
        g.cfg = types.SimpleNamespace(grad_clip=None, sqrt_anneal=case["sqrt_anneal"], trainer_max_steps=case["trainer_max_steps"],
                                      min_step_percent=case["min_step_percent"], max_step_percent=case["max_step_percent"])
        g.update_step(case["epoch"], case["step"])
        assert isinstance(g.min_step, int) and isinstance(g.max_step, int)
        done.append(dict(case, min_step=g.min_step, max_step=g.max_step))
    direct = []
    for lo, hi in [(0.02, 0.98), (0.02, 0.2)] + [(p, p) for p in INEXACT]:
        g = ns["AnimateMVDiffusionGuidance"]()
        g.num_train_timesteps = 1000
        g.set_min_max_steps(lo, hi)
        direct.append(dict(min_step_percent=lo, max_step_percent=hi, min_step=g.min_step, max_step=g.max_step))
    g.set_min_max_steps()
    defaults = dict(min_step=g.min_step, max_step=g.max_step)
    path = os.path.join(HERE, "guidance.json")
    with open(path, "w") as f:
        json.dump(dict(num_train_timesteps=1000, update_step=done, set_min_max_steps=direct, defaults=defaults), f, indent=0)
    print(len(done), "update_step cases,", len(direct), "set_min_max_steps cases;", os.path.getsize(path), "bytes")
    print("inexact percents:", [(d["min_step_percent"], d["min_step"]) for d in direct[2:]])


if __name__ == "__main__":
    main()
