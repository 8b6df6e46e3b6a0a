#!/usr/bin/env python
"""Bit equality of one kernel family between two builds of the library.

    python tools/attn_bit_equality.py dump FAMILY LIB OUT.json     # FAMILY: attn | gemm; one fresh process per library
    python tools/attn_bit_equality.py compare A.json B.json

`dump` runs the family's cases of the GPU tests (both storage types) in this process with LIB loaded instead of the in-tree library
(hip_ops._LIB_PATH set before the first load, as tools/microbench.py does) and records a sha256 of every tensor that the family's HipOps
methods return.  `compare` wants the same calls in the same order with the same hashes; exit status 1 otherwise.
  attn: HipOps.flash_attn, flash_attn2, flash_attn_bwd under the attention cases of tests/test_hip_kernels_gpu.py,
        tests/test_attention_bench_shapes_gpu.py and tests/test_train_kernels_gpu.py
  gemm: HipOps.gemm, gemm2, gemm_geglu, conv3x3, gemm_f32out under the GEMM / conv / split-K / GEGLU cases of tests/test_hip_kernels_gpu.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# family -> (wrapped HipOps methods, test files, pytest -k selection in those files)
FAMILIES = {
    "attn": (("flash_attn", "flash_attn2", "flash_attn_bwd"),
             ["tests/test_hip_kernels_gpu.py", "tests/test_attention_bench_shapes_gpu.py", "tests/test_train_kernels_gpu.py"],
             "attn or attention or level or fp16_mixed or fp16_window or head_dim"),
    "gemm": (("gemm", "gemm2", "gemm_geglu", "conv3x3", "gemm_f32out"), ["tests/test_hip_kernels_gpu.py"],
             "gemm or conv or split_k or geglu"),
}


def dump(family, lib, out):
    import pytest
    import torch
    import animate3d_amd.hip_ops as H
    H._LIB_PATH = os.path.abspath(lib)
    records = []

    def digest(t):
        if not isinstance(t, torch.Tensor):          # None, or the Ho / Wo of conv3x3
            return None
        return [list(t.shape), str(t.dtype), hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()]

    def wrap(name):
        orig = getattr(H.HipOps, name)

        def call(self, *a, **kw):
            r = orig(self, *a, **kw)
            if torch.cuda.is_current_stream_capturing():          # nothing has run yet: the replayed results are compared by the test itself
                return r
            torch.cuda.synchronize()
            records.append([name, str(self.act_dtype)] + [digest(t) for t in (r if isinstance(r, tuple) else (r,))])
            return r
        setattr(H.HipOps, name, call)

    names, tests, select = FAMILIES[family]
    for name in names:
        wrap(name)
    rc = int(pytest.main([os.path.join(ROOT, t) for t in tests] + ["-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select]))
    with open(out, "w") as f:
        json.dump({"family": family, "lib": lib, "pytest_rc": rc, "records": records}, f)
    print(f"[attn_bit_equality] {family} {lib}: pytest rc {rc}, {len(records)} calls, {sum(t is not None for r in records for t in r[2:])} tensors")
    return rc


def compare(a, b):
    ra, rb = json.load(open(a))["records"], json.load(open(b))["records"]
    n = bad = 0
    for i, (x, y) in enumerate(zip(ra, rb)):
        if x[:2] != y[:2]:
            print(f"call {i}: {x[:2]} against {y[:2]}")
            return 1
        for tx, ty in zip(x[2:], y[2:]):
            n += tx is not None or ty is not None
            if tx != ty:
                bad += 1
                print(f"call {i} {x[0]} {x[1]}: {tx} against {ty}")
    print(f"[attn_bit_equality] calls {len(ra)} / {len(rb)}, tensors compared {n}, differing {bad}")
    return 1 if bad or len(ra) != len(rb) else 0


if __name__ == "__main__":
    sys.exit(dump(*sys.argv[2:5]) if sys.argv[1] == "dump" else compare(*sys.argv[2:4]))
