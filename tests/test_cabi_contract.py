"""CPU checks of the training entry points' preconditions (include/animate3d_hip.h, "Training path"): a pointer that is not aligned to
the widest access the kernels make through it, or an attention-backward do_scale without a usable reciprocal, is refused with
A3D_EINVAL before anything reaches the GPU.  The device addresses below are made up and never dereferenced: every call differs from a
valid launch in exactly one operand, and the argument checks run before the first HIP call, so this runs on a machine without a GPU.
(No call here may pass with every pointer aligned: that would launch a kernel on made-up addresses.)  The forward attention entry
points, the deformation field's (a3d_dg_*), the ARAP loss's (a3d_knn_f32, a3d_arap_*), the splat rasterizer's (a3d_gs_*) and the forward
normalisations (a3d_group_norm*, a3d_layer_norm) are held to the same discipline further down."""
import ctypes
import math

import pytest

from animate3d_amd.hip_ops import RowMap

A3D_EINVAL = -1
A3D_EUNSUPPORTED = -2
BASE = 0x7F00_0010_0000          # fake device addresses: BASE + 0x10_0000 * i, 256-byte aligned


@pytest.fixture(scope="module")
def lib():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.load_library()


def _ptrs(names):
    return {n: BASE + 0x10_0000 * i for i, n in enumerate(names)}


def _map(ld):
    return ctypes.byref(RowMap(1, 64, 0, 64, 0).c(ld))


# entry point (bf16 name) -> (operand -> widest access in bytes, argument list of a valid geometry given the operand addresses)
def _flash_attn_bwd(p, do_scale=1.0, accumulate=0):
    return [None, p["Q"], p["K"], p["V"], p["dO"], p["dQ"], p["dK"], p["dV"], p["lse2"], p["delta"],
            _map(960), _map(960), _map(320), _map(960), _map(960), 4, 8, 40, 64, 64, 1, 40 ** -0.5, do_scale, accumulate]


CASES = {
    "a3d_flash_attn_bwd_bf16": (dict(Q=16, K=16, V=16, dO=16, dQ=16, dK=16, dV=16, lse2=4, delta=4), _flash_attn_bwd),
    "a3d_attn_delta_bf16": (dict(dO=16, O=16, delta=4),
                            lambda p: [None, p["dO"], p["O"], _map(320), _map(320), p["delta"], 4, 8, 40, 64]),
    "a3d_temporal_attn_bwd_bf16": (dict(Q=16, K=16, V=16, dO=16, dQ=16, dK=16, dV=16),
                                   lambda p: [None, p["Q"], p["K"], p["V"], 960, p["dO"], 320, p["dQ"], p["dK"], p["dV"], 960,
                                              2, 16, 9, 8, 40, 40 ** -0.5]),
    "a3d_group_norm_bwd_bf16": (dict(X=16, dY=16, gamma=4, beta=4, stats=4, dX=16, ws=4, dgamma=4, dbeta=4),
                                lambda p: [None, p["X"], p["dY"], p["gamma"], p["beta"], p["stats"], p["dX"], p["ws"], p["dgamma"], p["dbeta"],
                                           2, 64, 320, 32, 1]),
    "a3d_geglu_bwd_bf16": (dict(P=16, dY=16, dP=16), lambda p: [None, p["P"], 2560, p["dY"], 1280, p["dP"], 2560, 70, 1280]),
    "a3d_axpby_bf16": (dict(X=16, Y=16), lambda p: [None, p["X"], p["Y"], 1024, 0.5, 2.0]),
    "a3d_zero_insert2x_bf16": (dict(dY=16, Z=16), lambda p: [None, p["dY"], p["Z"], 2, 6, 6, 64]),
    "a3d_upsample2x_bwd_bf16": (dict(dU=16, dX=16), lambda p: [None, p["dU"], p["dX"], 2, 3, 5, 6, 10, 64]),
    "a3d_im2col_in_bwd": (dict(dCol=2, dX=4), lambda p: [None, p["dCol"], p["dX"], 2, 3, 2, 8, 8, 1.0]),
    "a3d_wgrad_bf16": (dict(dY=16, X=16, ws=16),
                       lambda p: [None, p["dY"], 320, p["X"], 320, p["dW"], 320, p["ws"], 64, 320, 320, 1.0, 0]),
    "a3d_softmax_rows_bwd_bf16": (dict(P=8, dP=16, dS=8), lambda p: [None, p["P"], 512, p["dP"], 512, p["dS"], 512, 16, 512, 1.0]),
}


def _twin(name, f16):
    if not f16:
        return name
    return name[:-5] + "_f16" if name.endswith("_bf16") else name + "_f16"


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("entry", sorted(CASES))
def test_misaligned_operand_is_refused(lib, entry, f16):
    """One call per operand, that operand moved off its alignment by the largest offset that still keeps the element size (8 bytes for
    a 16-byte access, 2 for a 4-byte one, 1 for a 2-byte one): a column view at a 4-element offset is the case this guards."""
    align, args_of = CASES[entry]
    fn = getattr(lib, _twin(entry, f16))
    names = list(align) + [n for n in ("dW",) if entry == "a3d_wgrad_bf16"]
    for operand, a in align.items():
        p = _ptrs(names)
        p[operand] += a // 2
        rc = fn(*args_of(p))
        assert rc == A3D_EINVAL, f"{entry}: {operand} at +{a // 2} bytes returned {rc}"


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("do_scale", [1e-40, -1e-45, 1.0e-38 / 2, math.inf, -math.inf, math.nan])
def test_flash_attn_bwd_refuses_do_scale_without_reciprocal(lib, do_scale, f16):
    """dP starts at -delta / do_scale: a subnormal do_scale (whose reciprocal overflows or loses range) or a non-finite one is refused
    rather than turned into NaN gradients.  (0 and every normal value are accepted: GPU tier, tests/test_train_kernels_gpu.py.)"""
    fn = getattr(lib, _twin("a3d_flash_attn_bwd_bf16", f16))
    for accumulate in (0, 1, 3):
        assert fn(*_flash_attn_bwd(_ptrs(CASES["a3d_flash_attn_bwd_bf16"][0]), do_scale, accumulate)) == A3D_EINVAL


# ---- forward attention (a3d_flash_attn, _lse, _counted, a3d_flash_attn2): one argument check serves the four entry points
ACCUMULATE, CAUSAL, EXACT, PLAIN = 1, 2, 4, 8          # A3D_ATTN_* of include/animate3d_hip.h
FWD_OPERANDS = {"a3d_flash_attn_bf16": ("Q", "K", "V", "O"), "a3d_flash_attn_lse_bf16": ("Q", "K", "V", "O", "lse2"),
                "a3d_flash_attn_counted_bf16": ("Q", "K", "V", "O", "counters"), "a3d_flash_attn2_bf16": ("Q", "K", "V", "K2", "V2", "O")}
FWD_VALID = dict(groups=4, heads=8, head_dim=40, q_len=64, kv_len=64, kv_len2=64, flags=0, ld=dict(q=320, k=320, k2=320, o=320))


def _fwd_call(lib, entry, f16, ptr=None, ld=None, **geometry):
    """The valid launch of `entry` (head_dim 40, 64 queries, 64 keys, 4 groups of 8 heads) with the named pointers / row pitches /
    geometry words replaced.  Callers replace exactly one, and never none."""
    assert ptr or ld or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _ptrs(FWD_OPERANDS[entry])
    p.update(ptr or {})
    g = dict(FWD_VALID, **geometry)
    lds = dict(FWD_VALID["ld"], **(ld or {}))
    shape = [g["groups"], g["heads"], g["head_dim"], g["q_len"], g["kv_len"]]
    if entry == "a3d_flash_attn2_bf16":
        args = [None, p["Q"], p["K"], p["V"], p["K2"], p["V2"], p["O"], _map(lds["q"]), _map(lds["k"]), _map(lds["k2"]), _map(lds["o"]),
                *shape, g["kv_len2"], 40 ** -0.5, 1.0, 0.5, g["flags"]]
    else:
        args = [None, p["Q"], p["K"], p["V"], p["O"], _map(lds["q"]), _map(lds["k"]), _map(lds["o"]), *shape, 40 ** -0.5, 1.0, g["flags"]]
        args += [p[n] for n in ("lse2", "counters") if n in p]
    return getattr(lib, _twin(entry, f16))(*args)


FWD = pytest.mark.parametrize("entry", sorted(FWD_OPERANDS))
F16 = pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])


@F16
@FWD
def test_flash_attn_refuses_misaligned_or_missing_operand(lib, entry, f16):
    """Q, K, V (K2, V2) are read 16 bytes at a time, O is written 8 bytes at a time, the counters are 4-byte words; lse2 and the counters
    are what their entry points exist for, so NULL is refused there."""
    base = _ptrs(FWD_OPERANDS[entry])
    for operand in FWD_OPERANDS[entry]:
        off = {"O": 4, "counters": 2, "lse2": None}.get(operand, 8)
        if off is not None:
            rc = _fwd_call(lib, entry, f16, ptr={operand: base[operand] + off})
            assert rc == A3D_EINVAL, f"{entry}: {operand} at +{off} bytes returned {rc}"
        if operand in ("lse2", "counters"):
            rc = _fwd_call(lib, entry, f16, ptr={operand: None})
            assert rc == A3D_EINVAL, f"{entry}: NULL {operand} returned {rc}"


@F16
@FWD
def test_flash_attn_refuses_bad_geometry(lib, entry, f16):
    """Flag bits outside the entry point's set, more groups than a grid's y extent, sequence positions beyond the 32-bit row maps'
    range and row pitches that break the 16-byte rows are A3D_EINVAL; shapes without a kernel are A3D_EUNSUPPORTED."""
    two = entry == "a3d_flash_attn2_bf16"
    for flags in ([CAUSAL, EXACT, 16, ACCUMULATE | 32] if two else [16, ACCUMULATE | 32]):
        assert _fwd_call(lib, entry, f16, flags=flags) == A3D_EINVAL, f"{entry}: flags {flags}"
    assert _fwd_call(lib, entry, f16, groups=65536) == A3D_EINVAL
    for length in ("q_len", "kv_len") + (("kv_len2",) if two else ()):
        assert _fwd_call(lib, entry, f16, **{length: 2 ** 30}) == A3D_EINVAL, f"{entry}: {length} = 2^30"
    for which in ("q", "k", "o") + (("k2",) if two else ()):
        assert _fwd_call(lib, entry, f16, ld={which: 324}) == A3D_EINVAL, f"{entry}: ld of the {which} map = 324"
    assert _fwd_call(lib, entry, f16, head_dim=48) == A3D_EUNSUPPORTED
    if two:
        assert _fwd_call(lib, entry, f16, head_dim=160) == A3D_EUNSUPPORTED
    else:
        assert _fwd_call(lib, entry, f16, flags=CAUSAL) == A3D_EUNSUPPORTED          # head_dim 40: causal is offered at 64 / 160 only


# ---- deformation field (a3d_dg_*, csrc/deform4d.hip): fp32 only, one build
DG_T, DG_N, DG_B, DG_FLAGS = 3, 300, 5, 3          # flags: use_global_trans | deform_scales, so mpart / gmean / glob are required
DG_ALIGN16 = ("grid", "rotation", "sp", "rots", "ws", "d_grid", "d_rots", "d_rotation")       # read or written 16 bytes at a time
DG_OPERANDS = {
    "a3d_dg_cells_f32": ("xyz", "cells"),
    "a3d_dg_forward_f32": ("xyz", "scaling", "rotation", "ts", "grid", "w", "img_start", "img_list", "sp", "mpart", "gmean", "glob", "means",
                           "scales", "rots"),
    "a3d_dg_backward_f32": ("xyz", "scaling", "rotation", "ts", "grid", "w", "img_start", "img_list", "sp", "gmean", "glob", "order", "starts",
                            "d_means", "d_scales", "d_rots", "ws", "d_grid", "d_weights", "d_scaling", "d_rotation"),
}
DG_OPTIONAL = ("mpart", "gmean", "glob")             # may be NULL without use_global_trans only


def _dg_desc(off=None, W=None, H=None):
    """Host plane descriptor off[12] | W[12] | H[12] of the grid ((6, 5, 7, 3), (12, 10, 14, 6)), entries replaced per {plane: value}."""
    from animate3d_amd import deform4d
    desc, _, _ = deform4d._plane_desc(((6, 5, 7, 3), (12, 10, 14, 6)))
    for base, repl in ((0, off), (12, W), (24, H)):
        for k, v in (repl or {}).items():
            desc[base + k] = v
    return desc


def _dg_call(lib, entry, ptr=None, desc="valid", **geometry):
    """The valid launch of `entry` (T = 3, N = 300, B = 5, flags 3) with the named pointers / the descriptor / geometry words replaced.
    Callers replace exactly one, and never none."""
    assert ptr or not isinstance(desc, str) or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _ptrs(DG_OPERANDS[entry])
    p.update(ptr or {})
    g = dict(dict(T=DG_T, N=DG_N, B=DG_B, flags=DG_FLAGS), **geometry)
    d = _dg_desc() if isinstance(desc, str) else desc
    if entry == "a3d_dg_cells_f32":
        return lib.a3d_dg_cells_f32(None, g["N"], p["xyz"], d, p["cells"])
    head = [None, g["T"], g["N"], g["B"], p["xyz"], p["scaling"], p["rotation"], p["ts"], p["grid"], d, p["w"], g["flags"], p["img_start"],
            p["img_list"]]
    return getattr(lib, entry)(*head, *[p[n] for n in DG_OPERANDS[entry][8:]])


DG = pytest.mark.parametrize("entry", sorted(DG_OPERANDS))


@DG
def test_deform_field_refuses_misaligned_or_missing_operand(lib, entry):
    """Every operand moved off the alignment the kernels need (8 bytes off for a 16-byte access, 2 for a 4-byte one), every operand
    NULL; mpart / gmean / glob are required because use_global_trans is set."""
    base = _ptrs(DG_OPERANDS[entry])
    for operand in DG_OPERANDS[entry]:
        off = 8 if operand in DG_ALIGN16 else 2
        rc = _dg_call(lib, entry, ptr={operand: base[operand] + off})
        assert rc == A3D_EINVAL, f"{entry}: {operand} at +{off} bytes returned {rc}"
        rc = _dg_call(lib, entry, ptr={operand: None})
        assert rc == A3D_EINVAL, f"{entry}: NULL {operand} returned {rc}"
    if entry != "a3d_dg_cells_f32":
        for operand in ("rotation", "rots" if "rots" in base else "d_rots"):       # a float-aligned view: what a flat parameter buffer gives
            assert _dg_call(lib, entry, ptr={operand: base[operand] + 4}) == A3D_EINVAL, operand


@DG
def test_deform_field_refuses_bad_geometry(lib, entry):
    """Empty or oversized extents (T is a grid's y extent; T N and B N index 4-wide rows in 32 bits) and plane descriptors that are
    absent, below the minimum resolution 2, above 32768, or whose offset is negative or breaks the 64-byte texel lines."""
    cells = entry == "a3d_dg_cells_f32"
    limit = (2 ** 31 - 1) // 4
    bad = [dict(N=0), dict(N=-1)]
    if not cells:
        bad += [dict(T=0), dict(T=-1), dict(B=0), dict(B=-1), dict(T=65536), dict(T=1, N=limit + 1), dict(T=2, N=limit // 2 + 1),
                dict(B=1, N=limit // DG_T + 1), dict(T=1, N=limit // DG_B + 1)]       # the last two: T N alone, B N alone
    for g in bad:
        assert _dg_call(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"
    assert _dg_call(lib, entry, desc=None) == A3D_EINVAL, f"{entry}: NULL plane descriptor"
    for k in (0, 5, 11):
        for field, values in (("W", (1, 0, 32769)), ("H", (1, 32769)), ("off", (-16, 8, 17))):
            for v in values:
                assert _dg_call(lib, entry, desc=_dg_desc(**{field: {k: v}})) == A3D_EINVAL, f"{entry}: plane {k} {field} = {v}"


def test_deform_field_size_queries(lib):
    """a3d_dg_mean_partials: blocks of 256 Gaussians; a3d_dg_backward_ws_floats: 0 for whatever a3d_dg_backward_f32 would refuse."""
    assert [lib.a3d_dg_mean_partials(n) for n in (-1, 0, 1, 256, 257)] == [0, 0, 1, 1, 2]
    ws = lib.a3d_dg_backward_ws_floats
    assert ws(DG_T, DG_N, _dg_desc()) > 0 and ws(1, 1, _dg_desc()) > 0
    assert ws(2 * DG_T, DG_N, _dg_desc()) > ws(DG_T, DG_N, _dg_desc()) < ws(DG_T, 2 * DG_N, _dg_desc())
    for args in ((0, DG_N, _dg_desc()), (-1, DG_N, _dg_desc()), (DG_T, 0, _dg_desc()), (DG_T, -1, _dg_desc()), (DG_T, DG_N, None),
                 (DG_T, DG_N, _dg_desc(W={3: 1})), (DG_T, DG_N, _dg_desc(H={8: 32769})), (DG_T, DG_N, _dg_desc(off={1: 8})),
                 (DG_T, DG_N, _dg_desc(off={1: -16}))):
        assert ws(*args) == 0, args[:2]


# ---- GEMM / implicit-GEMM convolution family (csrc/gemm_conv.hip): one argument check serves the dense entry points, one the convolutions
GEMM_VALID = dict(ldx=320, ldx2=320, ldw=320, ldr=320, ldy=320, M=256, N=320, K=320, K1=128, rb_div=256, flags=0,
                  B=2, H=8, W=8, Cin=64, Cout=320, stride=1, up2x=0)
# entry point -> operand -> bytes of the widest access made through it
GEMM_OPERANDS = {
    "a3d_gemm_bf16": dict(X=16, W=16, bias=16, rowbias=8, R=8, Y=8),
    "a3d_gemm_ws_bf16": dict(X=16, W=16, bias=16, rowbias=8, R=8, Y=8),
    "a3d_gemm2_bf16": dict(X=16, X2=16, W=16, bias=16, Y=16),
    "a3d_gemm_f32out_bf16": dict(X=16, W=16, bias=16, Y=16),
    "a3d_gemm_geglu_bf16": dict(X=16, W=16, bias=16, Y=16),
    "a3d_conv3x3_bf16": dict(X=16, W=16, bias=16, Y=8),
    "a3d_conv3x3_ws_bf16": dict(X=16, W=16, bias=16, Y=8),
}
GEMM_HAS_FLAGS = sorted(set(GEMM_OPERANDS) - {"a3d_gemm_f32out_bf16"})
GEMM_WS = ("a3d_gemm_ws_bf16", "a3d_conv3x3_ws_bf16")


def _gemm_call(lib, entry, f16, ptr=None, ws_needed=None, **geometry):
    """The valid launch of `entry` (dense: 256 x 320 x 320, GEGLU: N2 = 640; conv: 2 x 8 x 8 x 64 -> 320) with the named pointers /
    geometry words replaced.  Callers replace exactly one, and never none (a workspace query launches nothing)."""
    assert ptr or geometry or ws_needed is not None, "a fully valid call would launch a kernel on made-up addresses"
    conv = "conv3x3" in entry
    p = _ptrs(["X", "X2", "W", "bias", "rowbias", "R", "Y", "ws"])
    p.update(ptr or {})
    g = dict(GEMM_VALID, **geometry)
    if conv:
        args = [None, p["X"], p["W"], p["bias"], p["rowbias"], g["rb_div"], p["R"], p["Y"], g["B"], g["H"], g["W"], g["Cin"], g["Cout"],
                g["stride"], g["up2x"], g["flags"]]
    elif entry == "a3d_gemm2_bf16":
        args = [None, p["X"], g["ldx"], p["X2"], g["ldx2"], g["K1"], p["W"], g["ldw"], p["bias"], p["Y"], g["ldy"], g["M"], g["N"], g["K"], g["flags"]]
    elif entry == "a3d_gemm_f32out_bf16":
        args = [None, p["X"], g["ldx"], p["W"], g["ldw"], p["bias"], p["Y"], g["ldy"], g["M"], g["N"], g["K"], 1.0]
    elif entry == "a3d_gemm_geglu_bf16":
        args = [None, p["X"], g["ldx"], p["W"], g["ldw"], p["bias"], p["Y"], g["ldy"], g["M"], 2 * g["N"], g["K"], g["flags"]]
    else:
        args = [None, p["X"], g["ldx"], p["W"], g["ldw"], p["bias"], p["rowbias"], g["rb_div"], p["R"], g["ldr"], p["Y"], g["ldy"],
                g["M"], g["N"], g["K"], 1.0, 1.0, g["flags"]]
    if entry in GEMM_WS:
        args += [None, 0, ctypes.byref(ws_needed)] if ws_needed is not None else [p["ws"], 1 << 20, None]
    return getattr(lib, _twin(entry, f16))(*args)


GEMM = pytest.mark.parametrize("entry", sorted(GEMM_OPERANDS))


@F16
@GEMM
def test_gemm_family_refuses_misaligned_operand(lib, entry, f16):
    """X, W (X2) and the fp32 bias are fetched 16 bytes at a time (the persistent kernel's bias by LDS-DMA: a3d_gemm_geglu included);
    Y, R and rowbias of a3d_gemm are accessed 8 bytes at a time at least; the outputs of a3d_gemm2, _f32out and _geglu 16."""
    base = _ptrs(["X", "X2", "W", "bias", "rowbias", "R", "Y", "ws"])
    for operand, a in GEMM_OPERANDS[entry].items():
        rc = _gemm_call(lib, entry, f16, ptr={operand: base[operand] + a // 2})
        assert rc == A3D_EINVAL, f"{entry}: {operand} at +{a // 2} bytes returned {rc}"


@F16
@GEMM
def test_gemm_family_refuses_bad_geometry(lib, entry, f16):
    """Every divisibility rule of include/animate3d_hip.h, the stride and up2x codes, a rowbias without a positive rb_div, and a flags
    word with a bit outside the two masks."""
    if "conv3x3" in entry:
        bad = [dict(Cin=96), dict(Cin=32), dict(Cout=322), dict(stride=0), dict(stride=3), dict(up2x=-1), dict(up2x=8), dict(up2x=2),
               dict(up2x=4), dict(up2x=6), dict(up2x=1, stride=2), dict(rb_div=0), dict(rb_div=-256), dict(B=0), dict(H=0), dict(W=0)]
    else:
        bad = [dict(K=352), dict(K=32), dict(ldx=324), dict(ldw=324), dict(M=0), dict(N=0), dict(K=0)]
        bad += {"a3d_gemm_bf16": [dict(N=322), dict(ldy=322), dict(ldr=322), dict(rb_div=0), dict(rb_div=-256)],
                "a3d_gemm_ws_bf16": [dict(N=322), dict(ldy=322), dict(ldr=322), dict(rb_div=0), dict(rb_div=-256)],
                "a3d_gemm2_bf16": [dict(N=324), dict(ldy=324), dict(ldx2=324), dict(K1=100), dict(K1=0), dict(K1=320), dict(K1=384)],
                "a3d_gemm_f32out_bf16": [dict(N=324), dict(ldy=322)],
                "a3d_gemm_geglu_bf16": [dict(N=336), dict(N=304), dict(ldy=324)]}[entry]        # N2 = 2 N: 672 and 608 are no multiples of 64
    if entry in GEMM_HAS_FLAGS:
        bad += [dict(flags=0x400), dict(flags=0x1000 | 8), dict(flags=1 << 30)]
    for g in bad:
        assert _gemm_call(lib, entry, f16, **g) == A3D_EINVAL, f"{entry}: {g}"


@F16
@pytest.mark.parametrize("entry", GEMM_HAS_FLAGS)
def test_gemm_family_refuses_unassigned_kernel_choice(lib, entry, f16):
    """Kernel choice 0x300 (both bits of A3D_GEMM_KERNEL_MASK) names no kernel."""
    for flags in (0x300, 0x300 | 16):
        assert _gemm_call(lib, entry, f16, flags=flags) == A3D_EINVAL, f"{entry}: flags {flags:#x}"


@F16
@pytest.mark.parametrize("entry", GEMM_WS)
def test_gemm_family_ws_query_with_invalid_flags(lib, entry, f16):
    """The workspace query of a call whose flags word would be refused answers 0 bytes ("does not split") and no error."""
    for flags in (0x400, 0x1000 | 8, 1 << 30, 0x300):
        need = ctypes.c_int64(-1)
        assert _gemm_call(lib, entry, f16, ws_needed=need, flags=flags) == 0, f"{entry}: flags {flags:#x}"
        assert need.value == 0, f"{entry}: flags {flags:#x} -> {need.value} bytes"


# ---- ARAP loss and its k-NN graph (a3d_knn_f32, a3d_arap_*_f32, csrc/arap.hip): fp32 only, one build
KNN_OPERANDS = ("points", "nn_idx", "nn_dist")
KNN_VALID = dict(N=300, K=3, least=3)
ARAP_VALID = dict(F=4, Nv=300, K=3, S=64, bs=900)
ARAP_HEAD = ("source", "targets", "nn_idx", "weight", "sample_idx")
ARAP_OPERANDS = {
    "a3d_arap_energy_f32": ARAP_HEAD + ("rot", "rot_f32", "energy", "loss"),
    "a3d_arap_backward_f32": ARAP_HEAD + ("rot", "order", "starts", "grad_out", "d_targets", "d_source"),
}
ARAP_ALIGN8 = ("rot", "energy")                                  # fp64: the rotations and the per-sample energies
# weight, rot_f32, grad_out and d_source may be NULL (unit weights, no fp32 copy of R, zero gradients, no source gradient): with every
# other operand valid such a call would launch, so none is made here.
ARAP_OPTIONAL = ("weight", "rot_f32", "grad_out", "d_source")


def _knn_call(lib, ptr=None, **geometry):
    """The valid search (300 points, K = 3) with the named pointers / geometry words replaced.  Callers replace exactly one, and never none."""
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _ptrs(KNN_OPERANDS)
    p.update(ptr or {})
    g = dict(KNN_VALID, **geometry)
    return lib.a3d_knn_f32(None, g["N"], p["points"], g["K"], g["least"], 0.01, p["nn_idx"], p["nn_dist"])


def _arap_call(lib, entry, ptr=None, **geometry):
    """The valid launch of `entry` (F = 4, Nv = 300, K = 3, S = 64, dense frames) with the named pointers / geometry words replaced."""
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _ptrs(ARAP_OPERANDS[entry])
    p.update(ptr or {})
    g = dict(ARAP_VALID, **geometry)
    head = [None, g["F"], g["Nv"], g["K"], g["S"], p["source"], p["targets"], g["bs"], p["nn_idx"], p["weight"], p["sample_idx"]]
    return getattr(lib, entry)(*head, *[p[n] for n in ARAP_OPERANDS[entry][5:]])


def test_knn_refusals(lib):
    """No points, a missing or misaligned operand and a negative least_edge_num are A3D_EINVAL; a K without a kernel (the list lengths are
    1 ... 16) is A3D_EUNSUPPORTED; fewer than K other points is A3D_EINVAL."""
    base = _ptrs(KNN_OPERANDS)
    for operand in KNN_OPERANDS:
        assert _knn_call(lib, ptr={operand: None}) == A3D_EINVAL, f"NULL {operand}"
        assert _knn_call(lib, ptr={operand: base[operand] + 2}) == A3D_EINVAL, f"{operand} at +2 bytes"
    for g in (dict(N=0), dict(N=-1), dict(least=-1), dict(N=3), dict(N=2), dict(N=16, K=16)):
        assert _knn_call(lib, **g) == A3D_EINVAL, g
    for K in (0, 17, -1):
        assert _knn_call(lib, K=K) == A3D_EUNSUPPORTED, K


ARAP = pytest.mark.parametrize("entry", sorted(ARAP_OPERANDS))


@ARAP
def test_arap_refuses_misaligned_or_missing_operand(lib, entry):
    """Every required operand NULL; rot / energy 4 bytes off their 8-byte alignment; every 4-byte operand 2 bytes off."""
    base = _ptrs(ARAP_OPERANDS[entry])
    for operand in ARAP_OPERANDS[entry]:
        off = 4 if operand in ARAP_ALIGN8 else 2
        rc = _arap_call(lib, entry, ptr={operand: base[operand] + off})
        assert rc == A3D_EINVAL, f"{entry}: {operand} at +{off} bytes returned {rc}"
        if operand not in ARAP_OPTIONAL:
            rc = _arap_call(lib, entry, ptr={operand: None})
            assert rc == A3D_EINVAL, f"{entry}: NULL {operand} returned {rc}"


@ARAP
def test_arap_refuses_bad_geometry(lib, entry):
    """Empty extents, a negative batch stride, F beyond a grid's y extent (the backward launches F + 1 rows), and the 32-bit limits:
    F S <= 2^28 (frame, sample) pairs, S (K + 1) <= 2^30 inverse-list entries."""
    bad = [{k: v} for k in ("F", "Nv", "K", "S") for v in (0, -1)]
    bad += [dict(bs=-1), dict(F=65535), dict(F=16385, S=16384), dict(F=1, S=2 ** 28, K=4)]
    for g in bad:
        assert _arap_call(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"


# ---- splat rasterizer (a3d_gs_*_f32, csrc/splat.hip): fp32 only, one build
GS_VALID = dict(B=2, N=300, H=40, W=56, M=16, deg=3, L=1000, n_tiles=24, sumB=2, sumM=900)
GS_INPUTS = ("means", "scales", "rots", "opac", "shs", "colors", "view", "proj", "campos", "tanfovx", "tanfovy")
GS_OPERANDS = {
    "a3d_gs_preprocess_f32": GS_INPUTS + ("radii", "xy", "depth", "conic_o", "rgb", "clamped", "tiles_touched"),
    "a3d_gs_duplicate_f32": ("xy", "depth", "radii", "offsets", "keys", "vals"),
    "a3d_gs_tile_ranges_f32": ("keys", "ranges"),
    "a3d_gs_render_f32": ("ranges", "perm", "vals", "xy", "conic_o", "rgb", "depth", "bg", "out_img", "out_depth", "out_alpha", "T_final",
                          "n_contrib"),
    "a3d_gs_render_bwd_f32": ("ranges", "perm", "vals", "xy", "conic_o", "rgb", "depth", "bg", "T_final", "n_contrib", "d_img", "d_depth",
                              "d_alpha", "rows"),
    "a3d_gs_preprocess_bwd_f32": GS_INPUTS + ("radii", "clamped", "offsets", "tiles_touched", "rows", "d_means2d", "d_means", "d_scales",
                                              "d_rots", "d_opac", "d_shs", "d_colors"),
    "a3d_gs_sum_batch_f32": ("src", "dst"),
}
GS_ALIGN = dict(conic_o=16, rows=16, xy=8, ranges=8, keys=8, offsets=8, perm=8)          # every other operand: 4 bytes
GS_ABSENT = ("colors", "d_colors")                      # the valid call renders from shs: the other colour source and its gradient are NULL
GS_OPTIONAL = ("d_depth", "d_alpha")                    # NULL reads as a zero cotangent: with every other operand valid such a call would launch


def _gs_call(lib, entry, ptr=None, **geometry):
    """The valid launch of `entry` (B = 2, N = 300, 40 x 56, degree-3 SH with M = 16, L = 1000 instances) with the named pointers /
    geometry words replaced.  Callers replace exactly one, and never none."""
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _ptrs(GS_OPERANDS[entry])
    p.update({n: None for n in GS_ABSENT if n in p})
    p.update(ptr or {})
    g = dict(GS_VALID, **geometry)
    inputs = [g["B"], g["N"], p.get("means"), 0, p.get("scales"), 0, p.get("rots"), 0, p.get("opac"), 0, p.get("shs"), 0, g["M"],
              g["deg"], p.get("colors"), 0, p.get("view"), p.get("proj"), p.get("campos"), p.get("tanfovx"), p.get("tanfovy"), g["H"],
              g["W"], 1.0]
    dims = [g["B"], g["N"], g["H"], g["W"]]
    tail = lambda names: [p[n] for n in names]
    if entry in ("a3d_gs_preprocess_f32", "a3d_gs_preprocess_bwd_f32"):
        args = [None, *inputs, *tail(GS_OPERANDS[entry][len(GS_INPUTS):])]
    elif entry == "a3d_gs_tile_ranges_f32":
        args = [None, p["keys"], g["L"], p["ranges"], g["n_tiles"]]
    elif entry == "a3d_gs_sum_batch_f32":
        args = [None, p["src"], p["dst"], g["sumB"], g["sumM"]]
    else:
        args = [None, *dims, *tail(GS_OPERANDS[entry])]
    return getattr(lib, entry)(*args)


GS = pytest.mark.parametrize("entry", sorted(GS_OPERANDS))
GS_WITH_EXTENTS = sorted(set(GS_OPERANDS) - {"a3d_gs_tile_ranges_f32", "a3d_gs_sum_batch_f32"})
GS_WITH_INPUTS = ("a3d_gs_preprocess_f32", "a3d_gs_preprocess_bwd_f32")


@GS
def test_splat_refuses_misaligned_or_missing_operand(lib, entry):
    """Every required operand NULL (perm, vals and rows included: they are one element long when nothing is visible, never absent);
    conic_o and rows 8 bytes off their 16, xy / ranges / keys / offsets / perm 4 bytes off their 8, every other operand 2 bytes off.
    d_depth / d_alpha may be NULL, so only their misalignment is refused here."""
    base = _ptrs(GS_OPERANDS[entry])
    for operand in GS_OPERANDS[entry]:
        if operand in GS_ABSENT:
            continue
        off = GS_ALIGN.get(operand, 4) // 2
        rc = _gs_call(lib, entry, ptr={operand: base[operand] + off})
        assert rc == A3D_EINVAL, f"{entry}: {operand} at +{off} bytes returned {rc}"
        if operand not in GS_OPTIONAL:
            rc = _gs_call(lib, entry, ptr={operand: None})
            assert rc == A3D_EINVAL, f"{entry}: NULL {operand} returned {rc}"
    if entry == "a3d_gs_render_bwd_f32":                 # absent cotangents do not rescue a call that is refused for another reason
        assert _gs_call(lib, entry, ptr=dict(d_depth=None, d_alpha=None, rows=None)) == A3D_EINVAL
        assert _gs_call(lib, entry, ptr=dict(d_depth=None, d_alpha=None, perm=base["perm"] + 4)) == A3D_EINVAL


@pytest.mark.parametrize("entry", GS_WITH_INPUTS)
def test_splat_refuses_bad_colour_source_and_sh_arguments(lib, entry):
    """shs and colors both set or both NULL; a colour source without its gradient buffer; deg outside 0 .. 3; M < (deg + 1)^2; a colour
    source (and its gradient) moved off its 4-byte alignment in the colors form too."""
    base = _ptrs(GS_OPERANDS[entry])
    assert _gs_call(lib, entry, ptr=dict(colors=base["colors"])) == A3D_EINVAL, "shs and colors"
    assert _gs_call(lib, entry, ptr=dict(shs=None)) == A3D_EINVAL, "neither shs nor colors"
    assert _gs_call(lib, entry, ptr=dict(shs=None, colors=base["colors"] + 2, **({"d_colors": base["d_colors"]} if "d_colors" in base else {}))) \
        == A3D_EINVAL, "colors at +2 bytes"
    if "d_colors" in base:
        assert _gs_call(lib, entry, ptr=dict(shs=None, colors=base["colors"])) == A3D_EINVAL, "colors without d_colors"
        assert _gs_call(lib, entry, ptr=dict(shs=None, colors=base["colors"], d_colors=base["d_colors"] + 2)) == A3D_EINVAL
    for g in (dict(deg=-1), dict(deg=4), dict(deg=3, M=15), dict(deg=2, M=8), dict(deg=1, M=3), dict(deg=0, M=0)):
        assert _gs_call(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"


@pytest.mark.parametrize("entry", GS_WITH_EXTENTS)
def test_splat_refuses_bad_extents(lib, entry):
    """B, N, H, W <= 0; more than 2^31 - 1 (image, Gaussian) pairs; more than 2^31 - 1 (image, tile) ranges."""
    bad = [{k: v} for k in ("B", "N", "H", "W") for v in (0, -1)]
    bad += [dict(B=2, N=2 ** 30), dict(B=3, N=2 ** 30), dict(B=2, H=2 ** 19, W=2 ** 19), dict(B=1, H=2 ** 31 - 1, W=2 ** 31 - 1)]
    for g in bad:
        assert _gs_call(lib, entry, **g) == A3D_EINVAL, f"{entry}: {g}"


def test_splat_tile_ranges_and_sum_batch_refusals(lib):
    """a3d_gs_tile_ranges_f32: L < 0, L > 2^31 - 1, keys NULL with L > 0, n_tiles <= 0.  a3d_gs_sum_batch_f32: non-positive sizes (its
    NULL and misaligned pointers are with the other entry points')."""
    for g in (dict(L=-1), dict(L=2 ** 31), dict(n_tiles=0), dict(n_tiles=-1)):
        assert _gs_call(lib, "a3d_gs_tile_ranges_f32", **g) == A3D_EINVAL, g
    assert _gs_call(lib, "a3d_gs_tile_ranges_f32", ptr=dict(keys=None), L=1) == A3D_EINVAL
    assert _gs_call(lib, "a3d_gs_tile_ranges_f32", ptr=dict(ranges=None), L=0) == A3D_EINVAL
    for g in (dict(sumB=0), dict(sumB=-1), dict(sumM=0), dict(sumM=-1)):
        assert _gs_call(lib, "a3d_gs_sum_batch_f32", **g) == A3D_EINVAL, g


# ---- forward normalisation (a3d_group_norm, _group_norm2, _group_norm_sums, _group_norm_apply, a3d_layer_norm: csrc/norms.hip)
NORM_VALID = dict(B=2, rows=64, C=320, Ca=192, Cb=128, groups=32, M=64, pe1_div=4, pe1_mod=3, pe2_div=1, pe2_mod=5)
# entry point -> operands in argument order; every one of them is accessed 16 bytes at a time except the fp32 / fp64 arrays of GroupNorm
NORM_OPERANDS = {
    "a3d_group_norm_bf16": ("X", "Y", "gamma", "beta", "ws"),
    "a3d_group_norm2_bf16": ("X", "Xb", "Y", "gamma", "beta", "ws"),
    "a3d_group_norm_sums_bf16": ("X", "ws", "sums"),
    "a3d_group_norm_apply_bf16": ("X", "Y", "gamma", "beta", "stats"),
    "a3d_layer_norm_bf16": ("X", "Y1", "Y2", "gamma", "beta", "pe1", "pe2"),
}
NORM_ALIGN16 = {"a3d_group_norm_bf16": ("X", "Y"), "a3d_group_norm2_bf16": ("X", "Xb", "Y"), "a3d_group_norm_sums_bf16": ("X",),
                "a3d_group_norm_apply_bf16": ("X", "Y"), "a3d_layer_norm_bf16": ("X", "Y1", "Y2", "gamma", "beta", "pe1", "pe2")}
NORM_REQUIRED = {"a3d_group_norm_bf16": ("X", "Y", "gamma", "beta", "ws"), "a3d_group_norm2_bf16": ("X", "Xb", "Y", "gamma", "beta", "ws"),
                 "a3d_group_norm_sums_bf16": ("X", "ws", "sums"), "a3d_group_norm_apply_bf16": ("X", "Y", "gamma", "beta", "stats"),
                 "a3d_layer_norm_bf16": ("X", "Y1", "gamma", "beta")}          # Y2, pe1, pe2 may be NULL: such a call would launch


def _norm_call(lib, entry, f16, ptr=None, **geometry):
    """The valid launch of `entry` (GroupNorm: 2 x 64 rows x 320 channels in 32 groups, two-source 192 + 128; LayerNorm: 64 x 320 with
    both embedding maps) with the named pointers / geometry words replaced.  Callers replace exactly one, and never none."""
    assert ptr or geometry, "a fully valid call would launch a kernel on made-up addresses"
    p = _ptrs(NORM_OPERANDS[entry])
    p.update(ptr or {})
    g = dict(NORM_VALID, **geometry)
    if entry == "a3d_group_norm_bf16":
        args = [None, p["X"], p["Y"], p["gamma"], p["beta"], p["ws"], g["B"], g["rows"], g["C"], g["groups"], 1e-5, 1]
    elif entry == "a3d_group_norm2_bf16":
        args = [None, p["X"], g["Ca"], p["Xb"], g["Cb"], p["Y"], p["gamma"], p["beta"], p["ws"], g["B"], g["rows"], g["groups"], 1e-5, 1]
    elif entry == "a3d_group_norm_sums_bf16":
        args = [None, p["X"], p["ws"], p["sums"], g["B"], g["rows"], g["C"], g["groups"]]
    elif entry == "a3d_group_norm_apply_bf16":
        args = [None, p["X"], p["Y"], p["gamma"], p["beta"], p["stats"], g["B"], g["rows"], g["C"], g["groups"], 1]
    else:
        args = [None, p["X"], p["Y1"], p["Y2"], p["gamma"], p["beta"], g["M"], g["C"], 1e-5, p["pe1"], g["pe1_div"], g["pe1_mod"],
                p["pe2"], g["pe2_div"], g["pe2_mod"]]
    return getattr(lib, _twin(entry, f16))(*args)


NORM = pytest.mark.parametrize("entry", sorted(NORM_OPERANDS))


@F16
@NORM
def test_forward_norms_refuse_misaligned_or_missing_operand(lib, entry, f16):
    """X, Y, Xb of the GroupNorm entry points and every operand of a3d_layer_norm (pe1 / pe2 included: the embedding rows are read 16 bytes
    at a time) 8 bytes off; every required operand NULL (the workspace, the sums and the statistics among them)."""
    base = _ptrs(NORM_OPERANDS[entry])
    for operand in NORM_ALIGN16[entry]:
        rc = _norm_call(lib, entry, f16, ptr={operand: base[operand] + 8})
        assert rc == A3D_EINVAL, f"{entry}: {operand} at +8 bytes returned {rc}"
    for operand in NORM_REQUIRED[entry]:
        rc = _norm_call(lib, entry, f16, ptr={operand: None})
        assert rc == A3D_EINVAL, f"{entry}: NULL {operand} returned {rc}"


@F16
@NORM
def test_forward_norms_refuse_bad_geometry(lib, entry, f16):
    """GroupNorm: channels-per-group 5 and 6 (a 16-byte chunk could touch three groups), C % 8, more than 1024 groups, B > 65535, empty
    extents; two-source: C1 % 8 and C1 outside (0, C).  LayerNorm: C % 8, C > 1536, pe_div / pe_mod <= 0, M <= 0."""
    if entry == "a3d_layer_norm_bf16":
        bad = [dict(C=324), dict(C=1544), dict(C=2048), dict(C=0), dict(M=0), dict(M=-1),
               dict(pe1_div=0), dict(pe1_div=-4), dict(pe1_mod=0), dict(pe1_mod=-3), dict(pe2_div=0), dict(pe2_div=-1), dict(pe2_mod=0), dict(pe2_mod=-5)]
    elif entry == "a3d_group_norm2_bf16":
        bad = [dict(Ca=196, Cb=124), dict(Ca=0, Cb=320), dict(Ca=320, Cb=0), dict(Ca=-8, Cb=328), dict(Ca=328, Cb=-8),
               dict(Ca=96, Cb=64), dict(Ca=128, Cb=64), dict(Ca=192, Cb=132), dict(Ca=8 * 1100, Cb=8 * 1100, groups=1100),
               dict(B=65536), dict(B=0), dict(rows=0), dict(groups=0), dict(groups=33)]          # 160 / 32 = 5, 192 / 32 = 6
    else:
        bad = [dict(C=160), dict(C=192), dict(C=324), dict(C=8 * 1100, groups=1100), dict(C=96, groups=32), dict(B=65536), dict(B=0), dict(rows=0),
               dict(C=0), dict(groups=0), dict(groups=33), dict(C=8 * 1032, groups=8)]          # cg = 5, 6, 3; C / 8 > 1024
    for g in bad:
        assert _norm_call(lib, entry, f16, **g) == A3D_EINVAL, f"{entry}: {g}"
