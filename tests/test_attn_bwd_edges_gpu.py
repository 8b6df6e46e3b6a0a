"""Attention backward at the kernels' seams: csrc/attn_bwd.hip (statistics, dQ and dK|dV passes; LDS-DMA, aligned and unaligned launches;
full and ragged tile bodies; the in-kernel dK|dV sharing loop), a3d_attn_delta and the temporal backward of csrc/train_ops.hip, against the
float64 oracle of tests/attn_bwd_ref.py, for both storage types, through the existing entry points.

Bars (tests/attn_bwd_ref.py, ``row_report``): the whole-tensor relative L2 of tests/test_train_kernels_gpu.py (2e-2 bf16 / 3e-3 fp16; temporal
2 x 6e-3 / 2 x 1e-3) AND, per row i of dQ, dK and dV, ||kernel_i - exact_i|| <= 2 max(||model_i - exact_i||, median_j ||model_j - exact_j||),
where ``model`` is the float64 evaluation with only the roundings the kernel's header admits (``rounded``).  Rows the maps never reach must
be exactly zero.  The margin of 2 is not tuned on the kernel; tests/test_attn_bwd_ref_host.py shows on the CPU that five classic mistakes
fail these bars.  Which (pass, variant, body) cell a case reaches is in the case table's ``claims`` and checked there against a mirror of
the dispatch.  Every comparison prints a ``[parity]`` line before it asserts.

Measured on an MI355X (worst row ratio over every case, regime, statistics path and route of this file; bar 2; bf16 / fp16):

    head_dim   dQ pass (dq)    dK|dV pass (dk)   dK|dV pass (dv)
      40       1.08 / 1.15     1.27 / 1.31       1.33 / 1.43       (dv, dk bf16 and dq fp16: the flat 32 768-key case; dk fp16: planted)
      64       1.10 / 1.08     1.06 / 1.12       1.14 / 1.10
      80       1.04 / 1.12     1.04 / 1.15       1.02 / 1.05
     160       1.00 / 1.23     1.01 / 1.06       1.01 / 1.04
    temporal backward, head_dim 40 / 80 / 160, dq, dk, dv: 1.000 in bf16, <= 1.003 in fp16 (it IS the exact gradient rounded once)

Whole tensor against float64, kernel within 1.2 % of the model in every line: at most 3.8e-3 in bf16 and 5.7e-4 in fp16, except the flat
32 768-key case in fp16, where P and dS are subnormal: dv 6.1e-4, dk 2.0e-3 (the model's figures to four digits); bars 2e-2 / 3e-3.
dO x 2^-20 and 2^+20 in bf16 gave the k = 0 gradients times 2^k bit for bit at all four head dims, on both statistics paths, ragged and
DMA.  a3d_attn_delta: at most 0.083 of its derived bar.  No rounding had to be added to the model for the kernel; the per-group-partials
route's extra 16-bit store was in the model from the start, read from HipOps.flash_attn_bwd.
"""
import ctypes
import functools

import pytest
import torch

from tests import attn_bwd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
TAG = {torch.bfloat16: "bf16", torch.float16: "fp16"}
STATS = ["recompute", "given"]


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp16"])
def ops(request):
    from animate3d_amd.hip_ops import HipOps
    return HipOps(act_dtype=request.param)


# ------------------------------------------------------------------ references: computed once per (case, regime, dtype, ...), never changed
@functools.lru_cache(maxsize=None)
def _case(D, name):
    return R.cases(D)[name]


@functools.lru_cache(maxsize=None)
def _inputs(c, dtype, regime, do_exp=0):
    q, k, v, do = R.make_inputs(c, dtype, device=DEV, regime=regime)
    if do_exp:
        do = (do.float() * 2.0 ** do_exp).to(dtype)           # an exact scaling of every 16-bit value that stays normal
        wide = torch.empty(do.shape[0], do.shape[1] + 8, dtype=dtype, device=DEV)
        wide[:, :do.shape[1]] = do
        do = wide[:, :do.shape[1]]
    return q, k, v, do


@functools.lru_cache(maxsize=None)
def _exact(c, dtype, regime, do_exp=0):
    return R.exact(*R.case_args(c, _inputs(c, dtype, regime, do_exp)), q_per_kv=c.q_per_kv, do_scale=c.do_scale)


@functools.lru_cache(maxsize=None)
def _model(c, dtype, regime, stats, route, do_exp=0):
    return R.rounded(*R.case_args(c, _inputs(c, dtype, regime, do_exp)), storage=dtype, stats=stats, route=route, q_per_kv=c.q_per_kv,
                     do_scale=c.do_scale)


def _given(ex, dtype):
    """o= / lse= of the given-statistics path, from the oracle (the composition with the forward kernel has its own test)."""
    return dict(o=ex.o.to(dtype), lse=ex.lse2.to(torch.float32).reshape(-1).contiguous())


def _p(t):
    return None if t is None else t.data_ptr()


def _direct(ops, c, tensors, *, given=None, dq=None, dk=None, dv=None, accumulate=False):
    """a3d_flash_attn_bwd with the case's own q_per_kv, the way HipOps.flash_attn_bwd's ``run`` calls it: the in-kernel dK|dV sharing loop,
    which HipOps itself only takes from 512 workgroups on."""
    q, k, v, do = tensors
    C, n = c.C, c.groups * c.heads * c.q_len
    dq = torch.zeros(c.q_rows, C, dtype=ops.act_dtype, device=DEV) if dq is None else dq
    dk = torch.zeros(c.k_rows, C, dtype=ops.act_dtype, device=DEV) if dk is None else dk
    dv = torch.zeros(c.k_rows, C, dtype=ops.act_dtype, device=DEV) if dv is None else dv
    qm, km, dom = c.qmap.c(q.stride(0)), c.kmap.c(k.stride(0)), c.qmap.c(do.stride(0))
    dqm, dkm = c.qmap.c(dq.stride(0)), c.kmap.c(dk.stride(0))
    assert dk.stride(0) == dv.stride(0) and k.stride(0) == v.stride(0)
    flags = 1 if accumulate else 0
    if given is not None:
        o, lse2 = given["o"], given["lse"]
        delta = torch.empty(n, dtype=torch.float32, device=DEV)
        om = c.qmap.c(o.stride(0))
        rc = ops.lib.a3d_attn_delta_bf16(ops._stream(), _p(do), _p(o), ctypes.byref(dom), ctypes.byref(om), _p(delta), c.groups, c.heads, c.D, c.q_len)
        assert rc == 0, rc
        flags |= 2
    else:
        st = torch.empty(2, n, dtype=torch.float32, device=DEV)
        lse2, delta = st[0], st[1]
    rc = ops.lib.a3d_flash_attn_bwd_bf16(ops._stream(), _p(q), _p(k), _p(v), _p(do), _p(dq), _p(dk), _p(dv), _p(lse2), _p(delta),
                                         ctypes.byref(qm), ctypes.byref(km), ctypes.byref(dom), ctypes.byref(dqm), ctypes.byref(dkm),
                                         c.groups, c.heads, c.D, c.q_len, c.kv_len, c.q_per_kv, float(c.D) ** -0.5, c.do_scale, flags)
    assert rc == 0, rc
    return dq, dk, dv


def _run(ops, c, tensors, *, stats, route, ex, need_dkv=True, **outs):
    """The gradients by the route named: "kernel" with shared keys is the direct call above, everything else goes through HipOps (whose own
    choice must then BE the route named)."""
    given = _given(ex, ops.act_dtype) if stats == "given" else None
    if c.q_per_kv > 1 and route == "kernel" and need_dkv:
        return _direct(ops, c, tensors, given=given, **outs)
    assert not need_dkv or R.dkv_route(c.groups, c.heads, c.kv_len, c.q_per_kv) == route
    q, k, v, do = tensors
    return ops.flash_attn_bwd(q, k, v, do, c.qmap, c.kmap, c.groups, c.heads, c.q_len, c.kv_len, q_per_kv=c.q_per_kv, do_scale=c.do_scale,
                              need_dkv=need_dkv, **(given or {}), **outs)


def _compare(label, dtype, got, ex, model, need_dkv=True):
    reports = []
    for t, g, rows in (("dq", got[0], ex.q_index), ("dk", got[1], ex.k_index), ("dv", got[2], ex.k_index)):
        if g is None:
            assert not need_dkv and t != "dq"
            continue
        rep = R.row_report(g, getattr(ex, t), getattr(model, t), rows=rows, tol=R.ATTN_TOL[dtype], name=f"{TAG[dtype]} {t} {label}")
        print(rep.line())
        reports.append(rep)
    torch.cuda.synchronize()
    bad = [r.line() for r in reports if not r.ok]
    assert not bad, "\n".join(bad)


def _routes(c):
    return ["partials", "kernel"] if c.q_per_kv > 1 and c.name.startswith("first_frame") else [R.dkv_route(c.groups, c.heads, c.kv_len, c.q_per_kv)]


def _check_case(ops, c, regime, stats, do_exp=0):
    dt = ops.act_dtype
    tensors, ex = _inputs(c, dt, regime, do_exp), _exact(c, dt, regime, do_exp)
    for route in _routes(c):
        label = f"D={c.D} {c.name} {regime} stats={stats} route={route}" + (f" dO*2^{do_exp}" if do_exp else "")
        got = _run(ops, c, tensors, stats=stats, route=route, ex=ex)
        _compare(label, dt, got, ex, _model(c, dt, regime, stats, route, do_exp))
    if c.name == "cross77":                # text tokens are frozen inputs in training: the query-only call
        got = _run(ops, c, tensors, stats=stats, route="partials", ex=ex, need_dkv=False)
        assert got[1] is None and got[2] is None
        _compare(f"D={c.D} {c.name} {regime} stats={stats} dq only", dt, got, ex, _model(c, dt, regime, stats, "partials", do_exp), need_dkv=False)


# ------------------------------------------------------------------ the launch matrix
MATRIX = [(D, name) for D in R.HEAD_DIMS for name in R.cases(D)]


@pytest.mark.parametrize("stats", STATS)
@pytest.mark.parametrize("D,name", MATRIX, ids=[f"D{D}-{n}" for D, n in MATRIX])
def test_launch_matrix(ops, D, name, stats):
    """Every (pass, variant, body) cell of the dispatch at every head dim, randn inputs; the cells per case are the table's ``claims``."""
    _check_case(ops, _case(D, name), "randn", stats)


# ------------------------------------------------------------------ value regimes
@pytest.mark.parametrize("stats", STATS)
@pytest.mark.parametrize("regime", ["planted", "ramp_up", "ramp_down"])
@pytest.mark.parametrize("name", ["ragged_self", "dma_self"])
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_value_regimes(ops, D, name, regime, stats):
    """planted: keys 0, B - 1, B, the first of the last tile and the LAST VALID one are 1.5 x a query of the group, so a failed ragged mask or
    a counted clamped row is an O(1) error; ramps: the statistics pass's running maximum moves in every tile (up) or is set in tile 0 (down)."""
    _check_case(ops, _case(D, name), regime, stats)


@pytest.mark.parametrize("stats", STATS)
def test_flat_scores_over_32768_keys(ops, stats):
    """32 queries scaled by 0.05 against 32 768 keys at head_dim 40, one head: every P is about 3e-5 — subnormal in fp16 going into the
    MFMA of dV.  The model rounds P the same way, so the bar is the model's own (three times its usual dV row error in fp16)."""
    dt, D, S, T = ops.act_dtype, 40, 32, 32768
    c = R.Case("flat32768", D, 1, 1, S, T, 1, R.RowMap(1, S, 0, S, 0), R.RowMap(1, T, 0, T, 0), S, T, False,
               {"stats": ("aligned", "full"), "dq": ("dma", "full"), "dkv": ("unaligned", "ragged")})
    for p in R.PASSES:
        assert R.launch_variant(D, p, c.qmap, c.kmap, S, T) == c.claims[p]
    q, k, v, do = R.make_inputs(c, dt, device=DEV)
    wide = torch.zeros(S, 2 * D, dtype=dt, device=DEV)
    wide[:, D:] = (q.float() * 0.05).to(dt)
    tensors = (wide[:, D:], k, v, do)
    ex = R.exact(*R.case_args(c, tensors))
    assert float(torch.exp2((tensors[0].double() @ k.double().t()) * D ** -0.5 * 1.4426950408889634 - ex.lse2[0, 0][:, None]).max()) < 6.1e-5
    model = R.rounded(*R.case_args(c, tensors), storage=dt, stats=stats)
    got = _run(ops, c, tensors, stats=stats, route="kernel", ex=ex)
    _compare(f"D=40 flat32768 randn stats={stats} route=kernel", dt, got, ex, model)


@pytest.mark.parametrize("stats", STATS)
@pytest.mark.parametrize("name", ["ragged_self", "dma_self"])
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_linear_in_do_over_a_loss_scale_range(ops, D, name, stats):
    """dO x 2^k.  bf16, k = -20 / +20: every operation on dO's path is linear and a power of two commutes with every rounding while nothing
    leaves the normal range, so the gradients are those of k = 0 times 2^k BIT FOR BIT.  fp16, k = -4 / +4: held to the bars."""
    dt, c = ops.act_dtype, _case(D, name)
    if dt == torch.float16:
        for k in (-4, 4):
            _check_case(ops, c, "randn", stats, do_exp=k)
        return
    ex = _exact(c, dt, "randn")
    base = _run(ops, c, _inputs(c, dt, "randn"), stats=stats, route="kernel", ex=ex)
    for k in (-20, 20):
        # (the given-statistics path takes o= and lse= of the UNscaled problem: O does not depend on dO)
        got = _run(ops, c, _inputs(c, dt, "randn", k), stats=stats, route="kernel", ex=ex)
        for t, a, b in zip(("dq", "dk", "dv"), got, base):
            same = torch.equal(a.float(), b.float() * 2.0 ** k)
            nbad = int((a.float() != b.float() * 2.0 ** k).sum())
            print(f"[parity] bf16 {t} D={D} {name} stats={stats} dO*2^{k}: {'bit-identical to 2^k x the k=0 gradients' if same else f'{nbad} values differ'}")
            assert same, (t, k, nbad)


# ------------------------------------------------------------------ write discipline and determinism
SENTINEL = 0x5A3C          # a finite 16-bit pattern in both storage types


def _walled(rows, C, dt):
    """A [rows, C] middle column block of a [rows, 3 C] buffer filled with the sentinel."""
    wide = torch.full((rows, 3 * C), SENTINEL, dtype=torch.int16, device=DEV).view(dt)
    return wide, wide[:, C:2 * C]


def _walls_intact(wide, C):
    w = wide.view(torch.int16)
    return bool((w[:, :C] == SENTINEL).all()) and bool((w[:, 2 * C:] == SENTINEL).all())


@pytest.mark.parametrize("stats", STATS)
@pytest.mark.parametrize("name,route", [("ragged_self", "kernel"), ("dma_self", "kernel"), ("first_frame_ragged", "partials"),
                                        ("first_frame_ragged", "kernel"), ("cross77", "partials")])
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_writes_stay_inside_their_column_block_and_runs_repeat(ops, D, name, route, stats):
    dt, c = ops.act_dtype, _case(D, name)
    tensors, ex = _inputs(c, dt, "randn"), _exact(c, dt, "randn")
    plain = _run(ops, c, tensors, stats=stats, route=route, ex=ex)
    wq, dq = _walled(c.q_rows, c.C, dt)
    wk, dk = _walled(c.k_rows, c.C, dt)
    wv, dv = _walled(c.k_rows, c.C, dt)
    got = _run(ops, c, tensors, stats=stats, route=route, ex=ex, dq=dq, dk=dk, dv=dv) if (c.q_per_kv > 1 and route == "kernel") else \
        _run(ops, c, tensors, stats=stats, route=route, ex=ex, dq_out=dq, dk_out=dk, dv_out=dv)
    torch.cuda.synchronize()
    assert _walls_intact(wq, c.C) and _walls_intact(wk, c.C) and _walls_intact(wv, c.C), "a plain run wrote outside its column block"
    if c.q_per_kv > 1 and route == "kernel":
        # the direct call writes only the rows the maps reach: the rest of the block keeps the sentinel
        for blk, rows in ((dk, ex.k_index), (dv, ex.k_index)):
            off = torch.ones(c.k_rows, dtype=torch.bool, device=DEV)
            off[rows] = False
            assert bool((blk.view(torch.int16)[off] == SENTINEL).all())
            blk[off] = 0
    for t, a, b in zip(("dq", "dk", "dv"), got, plain):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{t}: two runs differ bit for bit"
    # accumulate on top of what is there: still nothing outside the block, and about twice the gradient inside
    if c.q_per_kv > 1 and route == "kernel":
        _run(ops, c, tensors, stats=stats, route=route, ex=ex, dq=dq, dk=dk, dv=dv, accumulate=True)
    else:
        _run(ops, c, tensors, stats=stats, route=route, ex=ex, dq_out=dq, dk_out=dk, dv_out=dv, accumulate=True)
    torch.cuda.synchronize()
    assert _walls_intact(wq, c.C) and _walls_intact(wk, c.C) and _walls_intact(wv, c.C), "an accumulating run wrote outside its column block"
    for t, a, b in zip(("dq", "dk", "dv"), (dq, dk, dv), plain):
        want = 2.0 * b.double()
        err = float((a.double() - want).norm() / (want.norm() + 1e-300))
        print(f"[parity] {TAG[dt]} {t} D={D} {name} stats={stats} route={route} accumulated twice: rel L2 to 2 x the plain run {err:.3e}")
        assert err <= R.ELEM_TOL[dt]              # one more rounding of the sum to the storage type


def _video_case(D, L, F, share):
    """b = 2 videos of the multi-view layout, one group per (video, frame); ``share``: first-frame keys for the F frames of a video."""
    qm, k0, rows = R.views(2, F, L, b=2)
    return R.Case(f"videos_L{L}_F{F}", D, 2, 2 * F, 2 * L, 2 * L, F if share else 1, qm, k0 if share else qm, rows, rows, True)


@pytest.mark.parametrize("share", [False, True], ids=["self", "sharing-loop"])
@pytest.mark.parametrize("tail", [0, 8], ids=["dma", "ragged"])
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_a_video_alone_equals_its_rows_in_the_batch(ops, D, tail, share):
    """A group's gradients do not depend on what else the launch holds: a call on one video's rows alone (one group for self attention, the
    F = 3 groups of one key set for the in-kernel sharing loop) is bit-identical to that video's rows of the batched call."""
    dt, F = ops.act_dtype, (3 if share else 1)
    c = _video_case(D, R.BR[D] - tail, F, share)
    tensors = R.make_inputs(c, dt, device=DEV)
    both = _direct(ops, c, tensors)
    per = c.q_rows // 2
    one = R.Case(c.name + "_alone", D, 2, F, c.q_len, c.kv_len, c.q_per_kv, c.qmap, c.kmap, per, per, True)
    for vid in range(2):
        alone = _direct(ops, one, tuple(t[vid * per:(vid + 1) * per] for t in tensors))
        for t, a, b in zip(("dq", "dk", "dv"), alone, both):
            assert torch.equal(a.view(torch.int16), b[vid * per:(vid + 1) * per].view(torch.int16)), (t, vid)
    ex = R.exact(*R.case_args(c, tensors), q_per_kv=c.q_per_kv)
    model = R.rounded(*R.case_args(c, tensors), storage=dt, q_per_kv=c.q_per_kv)
    _compare(f"D={D} {c.name} randn stats=recompute route=kernel x2 videos", dt, both, ex, model)


# ------------------------------------------------------------------ temporal attention backward
def _temporal_inputs(F, D, C, L, dt, regime):
    videos = 2
    rows = videos * F * L
    g = torch.Generator().manual_seed(100 * F + D + C + L)
    buf = torch.randn(rows, 3 * C, generator=g)
    if regime == "last_key_dominates":
        # a common component in every query and in the LAST frame's keys: score gap c^2 sqrt(D) = 6 in every head
        cst = (6.0 / D ** 0.5) ** 0.5
        buf[:, :C] += cst
        last = (torch.arange(rows) // L) % F == F - 1
        buf[last, C:2 * C] += cst
    buf = buf.to(dt).to(DEV)
    do = torch.randn(rows, C + 8, generator=g).to(dt).to(DEV)[:, 8:]
    return buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:], do


@pytest.mark.parametrize("D", [40, 80, 160])
@pytest.mark.parametrize("F", [1, 2, 16, 17, 32])
def test_temporal_attn_bwd_frame_counts_and_partial_dot_widths(ops, F, D):
    """F = 16 | 17: the 16- and the 32-frame instantiation; F = 32: its last frame; F = 1, 2: nearly every thread idle; head_dim 80 / 160:
    the 2- and 4-way partial-dot shuffles, on both instantiations.  Q, K, V are column blocks of one [rows, 3C] buffer, dO has its own
    stride.  P and dS stay in fp32 in this kernel: the model is the exact gradient rounded once."""
    dt = ops.act_dtype
    bad = []
    for C in (320, 640):
        for L in (1, 3):
            for regime in ("randn", "last_key_dominates"):
                q, k, v, do = _temporal_inputs(F, D, C, L, dt, regime)
                heads = C // D
                got = ops.temporal_attn_bwd(q, k, v, do, 2, F, L, heads)
                ex = R.exact_temporal(q, k, v, do, 2, F, L, heads)
                for i, t in enumerate(("dq", "dk", "dv")):
                    rep = R.row_report(got[:, i * C:(i + 1) * C], ex[i], R.round_to(ex[i], dt), tol=2 * R.ELEM_TOL[dt],
                                       name=f"{TAG[dt]} {t} temporal D={D} F={F} C={C} L={L} {regime}")
                    print(rep.line())
                    if not rep.ok:
                        bad.append(rep.line())
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ a3d_attn_delta
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_attn_delta_on_a_column_view(ops, D):
    """delta = rowsum(dO * O) per (group, head, query) with O a column view of a wider buffer (its own leading dimension) and the
    two-view row map; bar DERIVED for an fp32 fused-multiply-add chain of D terms: |err| <= D 2^-24 sum_d |dO_d O_d|."""
    dt, c = ops.act_dtype, _case(D, "ragged_self")
    _, _, _, do = _inputs(c, dt, "randn")
    g = torch.Generator().manual_seed(D)
    o = torch.randn(c.q_rows, 2 * c.C + 16, generator=g).to(dt).to(DEV)[:, c.C + 16:]
    assert o.stride(0) != do.stride(0)
    n = c.groups * c.heads * c.q_len
    delta = torch.full((n + 64,), 12345.0, dtype=torch.float32, device=DEV)
    dom, om = c.qmap.c(do.stride(0)), c.qmap.c(o.stride(0))
    rc = ops.lib.a3d_attn_delta_bf16(ops._stream(), _p(do), _p(o), ctypes.byref(dom), ctypes.byref(om), _p(delta), c.groups, c.heads, D, c.q_len)
    assert rc == 0, rc
    torch.cuda.synchronize()
    want, bound = R.exact_delta(do, o, c.qmap, c.qmap, c.groups, c.heads, c.q_len)
    err = (delta[:n].double().reshape(want.shape) - want).abs()
    worst = float((err / bound).max())
    print(f"[parity] {TAG[dt]} attn_delta D={D}: worst |err| / (D 2^-24 sum|dO O|) = {worst:.3f} (bar 1)")
    assert bool((err <= bound).all()), worst
    assert bool((delta[n:] == 12345.0).all()), "a3d_attn_delta wrote past groups * heads * q_len"
