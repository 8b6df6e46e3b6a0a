"""The binding is typed from include/animate3d_hip.h (animate3d_amd/hip_ops.py, ``parse_header``).  A wrong type shifts every argument behind
it and the call may still return 0, so: signatures written out by hand here for entry points that together use every type kind of the header
must equal what the loader derived; the two hand-written structs must equal the header's; what the parser does not know must raise; and the
constants the module exposes are the header's.  tests/test_cabi_contract.py drives about 60 entry points through the typed library and is
the broad net.  One GPU test: a refused call names the symbol that ran."""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_void_p as vp

import pytest

from animate3d_amd import hip_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "animate3d_hip.h")

# every kind: const char* result and no parameters; int64_t result; stream, pointers to void / float / int / int64_t / unsigned / uint8_t /
# the two structs; int, int64_t, float and double by value
PINNED = {
    "a3d_version": (c_char_p, []),
    "a3d_group_norm_ws_floats": (c_int64, [c_int, c_int64, c_int]),
    "a3d_flash_attn_bf16": (c_int, [vp] * 8 + [c_int, c_int, c_int, c_int64, c_int64, c_float, c_float, c_int]),
    "a3d_flash_attn_counted_f16": (c_int, [vp] * 8 + [c_int, c_int, c_int, c_int64, c_int64, c_float, c_float, c_int, vp]),
    "a3d_gemm_ws_bf16": (c_int, [vp, vp, c_int64, vp, c_int64, vp, vp, c_int64, vp, c_int64, vp, c_int64, c_int64, c_int64, c_int64,
                                 c_float, c_float, c_int, vp, c_int64, vp]),
    "a3d_adamw_f32": (c_int, [vp] * 5 + [c_int64] + [c_float] * 7 + [vp]),
    "a3d_stage_adam_f32": (c_int, [vp, vp, c_int, c_double, c_double, c_double, c_int, vp]),
    "a3d_clip_preprocess": (c_int, [vp, vp, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, vp, c_int, c_int, vp, vp, c_int, c_int,
                                    vp, vp, c_int, c_int, c_int, c_int, vp, c_int, vp, vp, c_int, c_int, vp]),
}


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build
    build.build(verbose=False)
    return hip_ops.load_library()


@pytest.fixture(scope="module")
def header():
    return hip_ops.read_header(HEADER)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(lib, header, name):
    fn = getattr(lib, name)
    assert (fn.restype, list(fn.argtypes)) == PINNED[name]
    assert header.functions[name] == PINNED[name]


def test_every_entry_point_is_typed(lib, header):
    assert tuple(header.functions) == hip_ops.EXPORTED_SYMBOLS and len(hip_ops.EXPORTED_SYMBOLS) == len(set(hip_ops.EXPORTED_SYMBOLS))
    for name, (res, args) in header.functions.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (res, args), name


@pytest.mark.parametrize("struct,cls", [("a3d_rowmap", hip_ops._RowMapC), ("a3d_stage_adam_entry", hip_ops.StageAdamEntry)])
def test_structs_equal_the_headers(header, struct, cls):
    assert [tuple(f) for f in cls._fields_] == header.structs[struct]
    assert ctypes.sizeof(cls) == 8 * len(cls._fields_)                  # every field is 8 bytes wide: no padding to get wrong


def test_entry_resolves_twins_once(lib):
    bf16, f16 = hip_ops._Entry(lib, False), hip_ops._Entry(lib, True)
    for name in hip_ops.EXPORTED_SYMBOLS:
        assert vars(bf16)[name] is getattr(lib, name)                   # plain attributes, no lookup hook
    twins = {n for n in hip_ops.EXPORTED_SYMBOLS if vars(f16)[n] is not getattr(lib, n)}
    assert twins == {n for n in hip_ops.EXPORTED_SYMBOLS if n.endswith("_bf16")} | {"a3d_im2col_in", "a3d_unpack_out", "a3d_im2col_in_bwd"}
    assert f16.a3d_gemm_bf16 is lib.a3d_gemm_f16 and f16.a3d_im2col_in is lib.a3d_im2col_in_f16 and f16.a3d_adamw_f32 is lib.a3d_adamw_f32
    assert f16.a3d_gemm_bf16.__name__ == "a3d_gemm_f16"                 # what ``call`` puts into its error text


@pytest.mark.parametrize("decl", [
    "int a3d_x(a3d_stream_t stream, long double v);",           # a scalar type outside the vocabulary
    "int a3d_x(a3d_stream_t stream, size_t n);",
    "int a3d_x(a3d_stream_t stream, const a3d_unknown* m);",      # a struct the header does not define
    "int a3d_x(a3d_stream_t stream, float** rows);",             # pointer to pointer
    "short a3d_x(a3d_stream_t stream);",                         # result type
    "int a3d_x(a3d_stream_t stream, int);",                      # a parameter without a name: no way to tell type from name
    "int a3d_x(a3d_stream_t stream, int n[4]);",
    "static inline int helper(int n) { return n; }",             # not a declaration of an entry point
    "typedef struct a3d_s { long double v; } a3d_s;",
])
def test_parser_refuses_what_it_does_not_know(decl):
    with pytest.raises(RuntimeError, match="animate3d_hip.h"):
        hip_ops.parse_header("typedef void* a3d_stream_t;\n" + decl + "\n")


def test_parser_reads_a_small_header():
    h = hip_ops.parse_header('#ifdef __cplusplus\nextern "C" {\n#endif\ntypedef void* a3d_stream_t; /* s */\nenum { A3D_A = 0, A3D_B = -3 };\n'
                             "#define A3D_C 0x30\ntypedef struct a3d_s { int64_t a, b; const float* p; } a3d_s;\n"
                             "/* int a3d_commented(int n); */\nint a3d_f(a3d_stream_t stream, const a3d_s* s,\n  double x);\n"
                             "const char* a3d_g(void);\n#ifdef __cplusplus\n}\n#endif\n")
    assert h.functions == {"a3d_f": (c_int, [vp, vp, c_double]), "a3d_g": (c_char_p, [])}
    assert h.constants == {"A3D_A": 0, "A3D_B": -3, "A3D_C": 0x30}
    assert h.structs == {"a3d_s": [("a", c_int64), ("b", c_int64), ("p", vp)]}


def test_missing_header_is_named(monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "animate3d_hip.h")
    monkeypatch.setattr(hip_ops, "_HEADER_PATH", missing)
    monkeypatch.setattr(hip_ops, "_lib", None)
    with pytest.raises(RuntimeError, match=re.escape(missing)):
        hip_ops.load_library()
    assert hip_ops._lib is None


def test_constants_are_the_headers(header):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    spelled = dict(re.findall(r"\b(A3D_[A-Z0-9_]+)\s*=?\s+(-?(?:0x[0-9a-fA-F]+|\d+))\b", text))      # "#define NAME v" and "NAME = v"
    assert {k: int(v, 0) for k, v in spelled.items()} == header.constants and len(spelled) == 18
    for name, value in header.constants.items():
        assert getattr(hip_ops, name) == value, name
    assert (hip_ops.A3D_ATTN_PLAIN, hip_ops.A3D_GEMM_RING, hip_ops.A3D_EINVAL, hip_ops.A3D_EUNSUPPORTED) == (8, 0x200, -1, -2)
    assert (hip_ops.STAGE_ADAM_MAX_TENSORS, hip_ops.STAGE_ADAM_BEGIN, hip_ops.STAGE_ADAM_CHECK, hip_ops.STAGE_ADAM_UPDATE) == tuple(
        header.constants["A3D_STAGE_ADAM_" + n] for n in ("MAX_TENSORS", "BEGIN", "CHECK", "UPDATE"))
    import torch
    assert hip_ops._DTYPE_CODE == {torch.float32: header.constants["A3D_F32"], torch.bfloat16: header.constants["A3D_BF16"],
                                   torch.float16: header.constants["A3D_F16"]}


def test_call_names_the_symbol_and_the_code(lib):
    """``call`` on an entry point that refuses before it touches the GPU: made-up addresses, X 8 bytes off the 16 that a3d_axpby reads at a
    time (tests/test_cabi_contract.py, whose rule holds here too: no call may pass with every pointer aligned)."""
    args = (0x7F00_0010_0008, 0x7F00_0020_0000, 1024, 0.5, 2.0)          # after the stream, which is None
    with pytest.raises(RuntimeError, match=r"^a3d_axpby_f16 n=1024 failed: A3D_EINVAL"):
        hip_ops.call(hip_ops._Entry(lib, True), "a3d_axpby_bf16", None, args, what="n=1024")
    with pytest.raises(RuntimeError, match=r"^a3d_axpby_bf16 failed: A3D_EINVAL"):
        hip_ops.call(lib, "a3d_axpby_bf16", None, args)
    assert hip_ops.call(lib, "a3d_axpby_bf16", None, args, tolerate=(hip_ops.A3D_EINVAL,)) == hip_ops.A3D_EINVAL
    with pytest.raises(RuntimeError, match="hipError 700"):
        hip_ops._check(700, "a3d_x")


@pytest.mark.gpu
@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_refused_launch_names_the_storage_twin(suffix):
    """A contiguous [rows, C] tensor 8 bytes into its storage passes every Python-side guard; a3d_axpby reads 16 bytes at a time and
    refuses the pointer before it launches anything (tests/test_cabi_contract.py shows that for both twins on the CPU)."""
    import torch
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[suffix]
    ops = hip_ops.HipOps(act_dtype=dtype)
    rows, C = 24, 64
    x = torch.zeros(rows * C + 8, dtype=dtype, device="cuda")[4:4 + rows * C].view(rows, C)
    y = torch.zeros(rows, C, dtype=dtype, device="cuda")
    with pytest.raises(RuntimeError, match=rf"\ba3d_axpby_{suffix} failed: A3D_EINVAL"):
        ops.axpby_(x, y)
    torch.cuda.synchronize()
