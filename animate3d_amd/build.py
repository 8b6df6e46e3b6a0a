"""Build libanimate3d_hip.so (gfx950) in-tree with hipcc.  No torch, no cmake.

    python -m animate3d_amd.build            # incremental
    python -m animate3d_amd.build --force
    python -m animate3d_amd.build --experiment MACRO    # side build lib/exp/libanimate3d_hip_MACRO.so with -DMACRO on every compile job, for
                                                         # tools/microbench.py and the pmc_* tools (A3D_LIB=...); never loaded by the package
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "libanimate3d_hip.so")
ARCH = "gfx950"
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
EXTRA_FLAGS = {}      # per-file additions, e.g. {"flash_attn.hip": ["-fno-honor-nans"]} (measured: no effect, not used)


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _digest(path: str) -> str:
    h = hashlib.sha256()
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))
    for dep in [path, *headers, os.path.join(os.path.dirname(PKG), "include", "animate3d_hip.h")]:
        with open(dep, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS + EXTRA_FLAGS.get(os.path.basename(path), [])).encode())
    return h.hexdigest()


# Storage types of the 16-bit activations / weights.  A twin source is compiled once per entry: as is for bf16 storage and with
# -DA3D_STORAGE_F16 for IEEE fp16 storage (its a3d_*_f16 entry points; objects <stem>.o and <stem>_f16.o).
STORAGE_VARIANTS = (("", []), ("_f16", ["-DA3D_STORAGE_F16"]))
# Sources compiled once: fp32 / integer code, or 16-bit outputs chosen by a run-time dtype code.  Every other .hip of csrc/ is a twin source.
# A single-storage file missing from this tuple fails at the link (every symbol defined twice); a twin source listed here loses its _f16
# entry points, which hip_ops.load_library() and tests/test_cabi.py refuse.
SINGLE_STORAGE = (
    "arap.hip", "camera_batch.hip", "clip_preprocess.hip", "deform4d.hip", "mesh_export.hip", "mesh_ingest.hip", "pipeline_f32.hip",
    "recon_loss.hip", "splat.hip", "stage_frames.hip", "stage_optim.hip", "stage_reg.hip", "train_optim.hip", "video_io.hip",
)


def compile_plan(objdir: str):
    """Every compile job of the library as (source path, object path, extra defines); the link line is the plan's objects, in this order."""
    plan = []
    for src in sources():
        name = os.path.basename(src)
        for suffix, defs in STORAGE_VARIANTS[:1] if name in SINGLE_STORAGE else STORAGE_VARIANTS:
            plan.append((src, os.path.join(objdir, name[:-4] + suffix + ".o"), list(defs)))
    return plan


def _link(hipcc: str, objs, lib: str, verbose: bool) -> None:
    cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", *objs, "-o", lib]
    if verbose:
        print("[a3d build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJDIR, exist_ok=True)
    hipcc = _hipcc()
    plan = compile_plan(OBJDIR)
    jobs = []
    for src, obj, defs in plan:
        stamp = obj + ".sha"
        dig = _digest(src) + " ".join(defs)
        fresh = (not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == dig)
        if not fresh:
            jobs.append((src, obj, stamp, dig, defs))

    def compile_one(job):
        src, obj, stamp, dig, defs = job
        cmd = [hipcc, *FLAGS, *defs, *EXTRA_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
        if verbose:
            print("[a3d build]", " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        with open(stamp, "w") as f:
            f.write(dig)

    with ThreadPoolExecutor(max_workers=min(10, max(1, len(jobs)))) as ex:
        list(ex.map(compile_one, jobs))
    if jobs or force or not os.path.exists(LIB):
        _link(hipcc, [obj for _, obj, _ in plan], LIB, verbose)
    return LIB


def build_experiment(macro: str, verbose: bool = True) -> str:
    """Compile every job of the plan with -D<macro> into lib/exp/ (measurement builds of code that is compiled out of the product)."""
    expdir = os.path.join(LIBDIR, "exp", macro)
    os.makedirs(expdir, exist_ok=True)
    hipcc = _hipcc()
    plan = compile_plan(expdir)

    def compile_one(job):
        src, obj, defs = job
        cmd = [hipcc, *FLAGS, *defs, "-D" + macro, "-c", src, "-o", obj]
        if verbose:
            print("[a3d build]", " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=10) as ex:
        list(ex.map(compile_one, plan))
    lib = os.path.join(LIBDIR, "exp", f"libanimate3d_hip_{macro}.so")
    _link(hipcc, [obj for _, obj, _ in plan], lib, verbose)
    return lib


if __name__ == "__main__":
    if "--experiment" in sys.argv:
        print(build_experiment(sys.argv[sys.argv.index("--experiment") + 1]))
    else:
        print(build(force="--force" in sys.argv))
