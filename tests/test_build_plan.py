"""CPU checks of the compile plan of animate3d_amd/build.py: which source is compiled for which storage types, that both builds take their
jobs from it, and that the fp32 kernels that used to ride along in twin sources are in the library once."""
import os
import types

import pytest

from animate3d_amd import build
from tests.test_cabi import _device_kernels

TWIN_DEF = "-DA3D_STORAGE_F16"


def _plan_by_source():
    by_src = {}
    for src, obj, defs in build.compile_plan(build.OBJDIR):
        by_src.setdefault(os.path.basename(src), []).append((os.path.basename(obj), defs))
    return by_src


def test_every_source_is_planned_once_or_twice():
    by_src = _plan_by_source()
    assert sorted(by_src) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    objs = [o for jobs in by_src.values() for o, _ in jobs]
    assert len(objs) == len(set(objs))
    for name, jobs in by_src.items():
        stem = name[:-4]
        if name in build.SINGLE_STORAGE:
            assert jobs == [(stem + ".o", [])], name
        else:
            assert jobs == [(stem + ".o", []), (stem + "_f16.o", [TWIN_DEF])], name


def test_single_storage_sources_exist_and_carry_no_twin_macros():
    assert len(set(build.SINGLE_STORAGE)) == len(build.SINGLE_STORAGE)
    for name in build.SINGLE_STORAGE:
        path = os.path.join(build.CSRC, name)
        assert os.path.isfile(path), name
        text = open(path).read()
        assert "A3D_FN(" not in text and "A3D_FN_BARE(" not in text and "A3D_STORAGE_F16" not in text, name


def test_build_and_experiment_build_run_the_plan(monkeypatch, tmp_path):
    """Both builds issue exactly the plan's compile jobs and link exactly the plan's objects (so a stale <stem>_f16.o in the object directory
    is never linked).  No compiler runs: the commands are recorded."""
    cmds = []
    monkeypatch.setattr(build, "_hipcc", lambda: "hipcc")
    monkeypatch.setattr(build, "subprocess", types.SimpleNamespace(run=lambda cmd, **kw: cmds.append(cmd)))
    monkeypatch.setattr(build, "LIBDIR", str(tmp_path))
    monkeypatch.setattr(build, "OBJDIR", str(tmp_path / "obj"))
    monkeypatch.setattr(build, "LIB", str(tmp_path / "lib.so"))
    os.makedirs(tmp_path / "obj")
    open(tmp_path / "obj" / "arap_f16.o", "w").close()                # left behind by a build from before the plan

    def jobs_and_link(extra):
        compiles = sorted((c[c.index("-c") + 1], os.path.basename(c[-1]), TWIN_DEF in c) for c in cmds if "-c" in c)
        links = [[os.path.basename(a) for a in c if a.endswith(".o")] for c in cmds if "-shared" in c]
        assert all(set(extra) <= set(c) for c in cmds if "-c" in c)
        return compiles, links

    want = build.compile_plan(str(tmp_path))
    want_jobs = sorted((s, os.path.basename(o), TWIN_DEF in d) for s, o, d in want)
    want_link = [os.path.basename(o) for _, o, _ in want]
    assert "arap_f16.o" not in want_link

    build.build(force=True, verbose=False)
    assert jobs_and_link([]) == (want_jobs, [want_link])
    cmds.clear()
    build.build_experiment("A3D_SOME_MACRO", verbose=False)
    assert jobs_and_link(["-DA3D_SOME_MACRO"]) == (want_jobs, [want_link])


@pytest.fixture(scope="module")
def lib_path():
    return build.build(verbose=False)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_moved_fp32_kernels_are_in_one_object(lib_path, tmp_path):
    """channel_mix / cfg_ddim used to be compiled into both elementwise objects (only their entry points were guarded); the optimiser kernels
    sat behind a guard inside train_ops.hip.  Each must now be device code of exactly one object: looked for in the objects of the sources
    that name the kernel and of the two twin sources they left."""
    moved = ["channel_mix_kernel", "cfg_ddim_kernel", "sqnorm_kernel", "clip_ctrl_kernel", "adamw_kernel"]
    by_src = _plan_by_source()
    look_in = {"elementwise.hip", "train_ops.hip"}
    for name in by_src:
        text = open(os.path.join(build.CSRC, name)).read()
        if any(k + "(" in text for k in moved):
            look_in.add(name)
    found = {k: [] for k in moved}
    for name in sorted(look_in):
        for obj, _ in by_src[name]:
            work = tmp_path / obj
            work.mkdir()
            for sym in _device_kernels(os.path.join(build.OBJDIR, obj), str(work)):
                for k in moved:
                    if k in sym and not sym.endswith(".kd"):
                        found[k].append(obj)
    assert found == {"channel_mix_kernel": ["pipeline_f32.o"], "cfg_ddim_kernel": ["pipeline_f32.o"], "sqnorm_kernel": ["train_optim.o"],
                     "clip_ctrl_kernel": ["train_optim.o"], "adamw_kernel": ["train_optim.o"]}, found
