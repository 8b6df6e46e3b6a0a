"""GPU parity tests of the normalisation kernels at the seams of their launch plans, on inputs that can fail (tests/norm_ref.py): GroupNorm
forward (one-launch and three-launch, one and two sources, sums / apply halves), GroupNorm backward, LayerNorm forward (one wave per row
and sub-wave rows, every embedding map) and LayerNorm backward, in both storage types, against float64 references computed from the same
16-bit inputs.  Row counts come from the launch plan itself (a3d_group_norm_plan) and from the kernels' constants, and every case asserts
that it still sits on the intended side of its seam.  The bounds are derived in tests/norm_ref.py; tests/test_norm_ref_host.py shows on
the CPU that a reference with a row, a channel or a lane misplaced exceeds each of them at least four times on these very inputs.
Every check prints its figure before it asserts ([norm-edges] lines: profiles/pytest_gpu_norm_edges.log).
"""
import pytest
import torch

from tests import norm_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5
G = R.GROUPS


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp16"])
def ops(request):
    from animate3d_amd.hip_ops import HipOps
    return HipOps(act_dtype=request.param)


@pytest.fixture(scope="module")
def plan():
    from animate3d_amd.hip_ops import group_norm_plan
    return group_norm_plan


def cuda(*ts):
    return tuple(t.cuda() for t in ts)


def check_fwd(name, got, ref, terms, dt):
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    excess, at = R.fwd_excess(got, ref, R.fwd_bound(terms, dt))
    print(f"[norm-edges] {name}: worst |err| / bound = {excess:.3f} at element {at}")
    assert excess <= 1.0, f"{name}: error is {excess:.3f} x the per-element bound at flat element {at}"


def check_blocks(name, got, ref, tol):
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    e = R.block_rel_l2(got, ref)
    print(f"[norm-edges] {name}: worst block rel_l2 = {e:.3e} (bar {tol:.1e})")
    assert e <= tol, f"{name}: relative L2 {e:.3e} of the worst block > {tol:.1e}"


def check_vec(name, got, ref, tol=R.PARAM_TOL):
    e = R.rel_l2(got, ref)
    print(f"[norm-edges] {name}: rel_l2 = {e:.3e} (bar {tol:.1e})")
    assert torch.isfinite(got).all() and e <= tol, f"{name}: relative L2 {e:.3e} > {tol:.1e}"


# ------------------------------------------------------------------ GroupNorm forward
def _gn_case(plan, C, rows, dt, **kw):
    p = plan(rows, C, G)
    probes = R.batch_probes(R.probe_rows(p, rows))
    x, gamma, beta = cuda(*R.structured(len(probes), rows, C, G, probes, dt, seed=rows + C, **kw))
    return p, len(probes), x, gamma, beta


def _gn_forward_both(ops, name, B, rows, x, gamma, beta, run):
    for act in (False, True):          # the one-launch kernel's SiLU multiplies by v_rcp_f32, the three-launch kernel's divides
        ref, terms = R.gn_forward(x, B, rows, gamma, beta, G, EPS, act)
        check_fwd(f"{name} silu{int(act)}", run(act), ref, terms, ops.act_dtype)


SEAM_OF = {}
for _C, _lo, _hi, _field in R.GN_SEAMS:
    SEAM_OF[_C, _lo] = SEAM_OF[_C, _hi] = (_lo, _hi, _field)


@pytest.mark.parametrize("C,rows", R.gn_forward_rows())
def test_group_norm_at_the_plan_seams(ops, plan, C, rows):
    """Both sides of every switch of gn_fused_plan (slab width, 256 / 512 threads, 11 / 21 chunks per thread, streaming, one launch / three)
    and row counts below, at and above the row lanes (threads that own no row); probe rows where the threads' row ownership changes
    hands.  A slice of the batch reproduces the full launch bit for bit."""
    dt = ops.act_dtype
    if (C, rows) in SEAM_OF:
        lo, hi, field = SEAM_OF[C, rows]
        assert plan(lo, C, G)[field] != plan(hi, C, G)[field], f"C={C}: rows {lo} | {hi} no longer differ in {field}"
    p, B, x, gamma, beta = _gn_case(plan, C, rows, dt)
    out = {}
    _gn_forward_both(ops, f"group_norm C{C} rows{rows} fused{p['fused']} sg{p['sg']} threads{p['threads']} rmax{p['rmax']}", B, rows, x, gamma, beta,
                     lambda act: out.setdefault(act, ops.group_norm(x, B, rows, gamma, beta, G, EPS, act)))
    one = ops.group_norm(x[:rows].contiguous(), 1, rows, gamma, beta, G, EPS, True)
    two = ops.group_norm(x[rows:3 * rows].contiguous(), 2, rows, gamma, beta, G, EPS, True)
    assert torch.equal(one, out[True][:rows]) and torch.equal(two, out[True][rows:3 * rows]), "a batch slice differs from the full launch"


def test_group_norm_three_launch_tails(ops, plan):
    """Last 128-row chunk of 1, ny, 4 ny - 1, 4 ny and 4 ny + 1 rows: the four-rows-in-flight loops of gn_partial_kernel / gn_apply_kernel
    and their remainders."""
    ny = plan(1 << 20, 320, G)["ny"]
    for rows in R.gn_tail_rows(ny):
        p, B, x, gamma, beta = _gn_case(plan, 320, rows, ops.act_dtype)
        assert p["fused"] == 0 and p["ny"] == ny
        _gn_forward_both(ops, f"group_norm C320 rows{rows} (tail {rows % R.GN_CHUNK_ROWS})", B, rows, x, gamma, beta,
                         lambda act: ops.group_norm(x, B, rows, gamma, beta, G, EPS, act))


@pytest.mark.parametrize("C,rows", [(1280, 133), (320, 2143)])
def test_group_norm_mean_64_times_the_deviation(ops, plan, C, rows):
    """Every group's mean is 64 x its standard deviation (no probe rows: they would raise the deviation): the single-pass variance
    E[x^2] - mean^2 of both paths loses 12 bits there, and the output is held to the same bound."""
    p = plan(rows, C, G)
    B = 4
    x, gamma, beta = cuda(*R.structured(B, rows, C, G, [None] * B, ops.act_dtype, seed=rows, mean_over_std=64.0))
    _gn_forward_both(ops, f"group_norm mean/std=64 C{C} rows{rows} fused{p['fused']}", B, rows, x, gamma, beta,
                     lambda act: ops.group_norm(x, B, rows, gamma, beta, G, EPS, act))


@pytest.mark.parametrize("rows,Ca,Cb", R.GN2_CASES)
def test_group_norm_two_source_at_the_kernel_level(ops, plan, rows, Ca, Cb):
    """a3d_group_norm2 against float64 and bit-equal to the one-source kernel on the concatenation.  1280 + 640 at 256 rows (an up-block
    shape): one launch, 240-channel slabs, the sixth straddles C1; 1280 + 1280 at 64 rows: one launch, C1 on a slab boundary (the
    one-source launch streams, the two-source one does not); 640 + 320 at 2143 rows: three launches."""
    dt, C = ops.act_dtype, Ca + Cb
    p, B, x, gamma, beta = _gn_case(plan, C, rows, dt)
    if (rows, Ca, Cb) == (256, 1280, 640):
        slab = p["sg"] * (C // G)
        assert p["fused"] == 1 and Ca % slab != 0, "no slab straddles the two sources any more"
    elif rows == 2143:
        assert p["fused"] == 0
    else:
        assert p["fused"] == 1
    xa, xb = x[:, :Ca].contiguous(), x[:, Ca:].contiguous()
    for act in (False, True):
        got = ops.group_norm2(xa, xb, B, rows, gamma, beta, G, EPS, act)
        ref, terms = R.gn_forward2(xa, xb, B, rows, gamma, beta, G, EPS, act)
        check_fwd(f"group_norm2 {Ca}+{Cb} rows{rows} silu{int(act)}", got, ref, terms, dt)
        assert torch.equal(got, ops.group_norm(x, B, rows, gamma, beta, G, EPS, act)), f"two-source differs from one-source (silu {act})"


@pytest.mark.parametrize("C", R.GN_SUMS_WIDTHS)
def test_group_norm_sums_and_apply_shards(ops, plan, C):
    """The two halves on shards of 1, 127, 128 and 129 rows (one chunk short, exact, one row into the next) at channels-per-group 4, 7
    and 9.  Sums: |d sum| <= n 2^-24 sum|x|, |d sumsq| <= n 2^-24 sum x^2 with n = sums_chain: a thread's ceil(128 / ny) rows x 8 channels
    plus the ny row lanes x chunk columns of the one-thread-per-group LDS stage (n = 80, 138, 166 for C = 128, 224, 288; the chunks are
    combined in fp64).  Apply: the forward bound, statistics from the float64 reference rounded to fp32."""
    dt = ops.act_dtype
    ny = plan(1 << 20, C, G)["ny"]
    n = R.sums_chain(ny, C, G)
    assert n == {128: 80, 224: 138, 288: 166}[C]
    for rows in R.GN_SHARD_ROWS:
        probes = R.batch_probes(R.probe_rows(dict(fused=0, ny=ny), rows))
        B = len(probes)
        x, gamma, beta = cuda(*R.structured(B, rows, C, G, probes, dt, seed=C + rows))
        got = ops.group_norm_sums(x, B, rows, G)
        ref = R.gn_sums(x, B, rows, G)
        excess = float(((got - ref).abs() / (n * 2.0 ** -24 * R.gn_sums(x.abs(), B, rows, G))).max())
        print(f"[norm-edges] group_norm_sums C{C} rows{rows}: worst |err| / (n 2^-24 sum) = {excess:.3f} (n = {n})")
        assert excess <= 1.0
        mean, rstd, _ = R.gn_stats(x, B, rows, G, EPS)
        stats = torch.stack([mean, rstd], dim=-1).float().contiguous()
        for act in (False, True):
            ref_y, terms = R.gn_forward(x, B, rows, gamma, beta, G, EPS, act, stats=(mean, rstd))
            check_fwd(f"group_norm_apply C{C} rows{rows} silu{int(act)}", ops.group_norm_apply(x, B, rows, gamma, beta, G, stats, act), ref_y, terms, dt)


# ------------------------------------------------------------------ GroupNorm backward
@pytest.mark.parametrize("B,rows,C,groups", R.gn_bwd_cases())
def test_group_norm_bwd_at_the_row_step_seams(ops, B, rows, C, groups):
    """rows around the workgroup's row step rpb and its 8-step minimum, B = 700 (three workgroups per instance where the rows would fill
    four), 64 groups and 4 channels per group; SiLU and parameter gradients both ways.  dx: relative L2 per (instance, group) block."""
    dt = ops.act_dtype
    probes = R.gn_bwd_probes(B, rows, C)
    x, gamma, beta = R.structured(B, rows, C, groups, probes, dt, seed=B + rows + C)
    dy = R.structured_dy(x, B, rows, C, groups, probes, dt, seed=B + rows + C)
    x, dy, gamma, beta = cuda(x, dy, gamma, beta)
    mean, rstd, _ = R.gn_stats(x, B, rows, groups, EPS)
    stats = torch.stack([mean, rstd], dim=-1).float().contiguous()
    for act in (False, True):
        rx, rg, rb = R.gn_backward(x, dy, B, rows, gamma, beta, groups, EPS, act)
        for need in (True, False):
            dx, dg, db = ops.group_norm_bwd(x, dy, B, rows, gamma, beta, groups, stats, act, need_param=need)
            name = f"group_norm_bwd B{B} rows{rows} C{C} g{groups} silu{int(act)} param{int(need)}"
            check_blocks(f"{name} dx", R.gn_blocks(dx, B, rows, groups), R.gn_blocks(rx, B, rows, groups), R.DX_TOL[dt])
            if need:
                check_vec(f"{name} dgamma", dg, rg)
                check_vec(f"{name} dbeta", db, rb)
            else:
                assert dg is None and db is None


# ------------------------------------------------------------------ LayerNorm forward
def _pe(n, C, dt, seed):
    return cuda((0.5 * torch.randn(n, C, generator=torch.Generator().manual_seed(seed))).to(dt))[0]


LN_FWD_CASES = R.LN_FWD_GENERIC + [(M, C) for C in R.LN_ROWS_WIDTHS for M in R.ln_rows_seams(C)]


@pytest.mark.parametrize("M,C", LN_FWD_CASES)
def test_layer_norm_at_the_row_seams(ops, M, C):
    """One wave per row at 1 chunk, 64 / 65, 128 / 129 and 192 chunks per row; the sub-wave rows kernel at M around the rows per wave step
    and per workgroup (masked tail rows).  Both outputs, each with its own embedding map."""
    dt = ops.act_dtype
    x, gamma, beta = cuda(*R.structured_rows(M, C, R.ln_probes(M, C), dt, seed=M + C))
    pe1, pe2 = _pe(3, C, dt, 3), _pe(5, C, dt, 4)
    y1, y2 = ops.layer_norm(x, gamma, beta, EPS, pe1=pe1, pe1_div=2, pe2=pe2, pe2_div=1, two=True)
    (r1, t1), (r2, t2) = R.ln_forward(x, gamma, beta, EPS, pe1=pe1, pe1_div=2, pe2=pe2, pe2_div=1)
    check_fwd(f"layer_norm {M}x{C} y1", y1, r1, t1, dt)
    check_fwd(f"layer_norm {M}x{C} y2", y2, r2, t2, dt)


@pytest.mark.parametrize("M,C", [(33, 1280), (9, 320), (7, 768)])
def test_layer_norm_embedding_maps(ops, M, C):
    """pe1 only; pe2 only; two outputs without pe2; a one-row embedding; a pe_div that does not divide M."""
    dt = ops.act_dtype
    x, gamma, beta = cuda(*R.structured_rows(M, C, R.ln_probes(M, C), dt, seed=M + C + 1))
    pe, one = _pe(4, C, dt, 5), _pe(1, C, dt, 6)
    plain = R.ln_forward(x, gamma, beta, EPS)[0]
    cases = {
        "pe1 only": (dict(pe1=pe, pe1_div=1), R.ln_forward(x, gamma, beta, EPS, pe1=pe)[0], None),
        "pe2 only": (dict(pe2=pe, pe2_div=1, two=True), plain, R.ln_forward(x, gamma, beta, EPS, pe2=pe)[1]),
        "two without pe2": (dict(pe1=pe, pe1_div=1, two=True), R.ln_forward(x, gamma, beta, EPS, pe1=pe)[0], plain),
        "one-row pe": (dict(pe1=one, pe1_div=1, pe2=one, pe2_div=3, two=True), *R.ln_forward(x, gamma, beta, EPS, pe1=one, pe2=one, pe2_div=3)),
        "pe_div 5": (dict(pe1=pe, pe1_div=5, pe2=pe, pe2_div=M + 1, two=True), *R.ln_forward(x, gamma, beta, EPS, pe1=pe, pe1_div=5, pe2=pe, pe2_div=M + 1)),
    }
    assert M % 5 != 0
    for name, (kw, want1, want2) in cases.items():
        got = ops.layer_norm(x, gamma, beta, EPS, **kw)
        got1, got2 = got if kw.get("two") else (got, None)
        check_fwd(f"layer_norm {M}x{C} {name} y1", got1, *want1, dt)
        if want2 is not None:
            check_fwd(f"layer_norm {M}x{C} {name} y2", got2, *want2, dt)


# ------------------------------------------------------------------ LayerNorm backward
def _ln_bwd_check(ops, name, x, dy, gamma, params=(True, False)):
    dt = ops.act_dtype
    rx, rg, rb = R.ln_backward(x, dy, gamma, EPS)
    for need in params:
        dx, dg, db = ops.layer_norm_bwd(x, dy, gamma, EPS, need_param=need)
        check_blocks(f"{name} param{int(need)} dx", dx, rx, R.DX_TOL[dt])
        if need:
            check_vec(f"{name} dgamma", dg, rg)
            check_vec(f"{name} dbeta", db, rb)
        else:
            assert dg is None and db is None
    return dx


def _ln_bwd_inputs(M, C, dt):
    probes = R.ln_probes(M, C)
    x, gamma, _ = R.structured_rows(M, C, probes, dt, seed=M + C)
    dy = R.structured_rows_dy(x, gamma, probes, dt, seed=M + C)
    return cuda(x, dy, gamma)


@pytest.mark.parametrize("M,C", R.LN_BWD_GENERIC + [(M, C) for C in R.LN_ROWS_WIDTHS for M in R.ln_rows_seams(C)])
def test_layer_norm_bwd_at_the_row_seams(ops, M, C):
    """One wave per row at every instantiation (5, 10, 20, 32 channels per lane) with ragged last lanes, and its grid-stride loop
    (8195 rows: 2048 workgroups x 4 rows, then three more); the sub-wave rows kernel at M around the rows per wave step and per 16 steps.
    dx: relative L2 per row."""
    x, dy, gamma = _ln_bwd_inputs(M, C, ops.act_dtype)
    _ln_bwd_check(ops, f"layer_norm_bwd {M}x{C}", x, dy, gamma)


@pytest.mark.parametrize("M,C,param", R.LN_BWD_LOOPS)
def test_layer_norm_bwd_rows_kernel_grid_stride_loop(ops, M, C, param):
    """More row batches than the launch has waves: 513 workgroups' worth against the 512 launched with parameter gradients, 4097 against
    4096 without; the row count is odd, so the last batch is ragged too."""
    rpw = R.ln_rpw(C)
    assert -(-(-(-M // rpw)) // 4) > (512 if param else 4096)
    x, dy, gamma = _ln_bwd_inputs(M, C, ops.act_dtype)
    _ln_bwd_check(ops, f"layer_norm_bwd loop {M}x{C}", x, dy, gamma, params=(param,))


def test_layer_norm_bwd_8_byte_offset_view(ops):
    """C = 320 through a flat view that starts 8 bytes into its buffer: not 16-byte aligned, so the one-wave kernel serves it, and the result
    agrees with the aligned launch (sub-wave rows kernel) within the bar."""
    dt, M, C = ops.act_dtype, 37, 320
    x, dy, gamma = _ln_bwd_inputs(M, C, dt)

    def shifted(t):
        buf = torch.empty(M * C + 8, dtype=dt, device=t.device)
        v = buf[4:4 + M * C].view(M, C)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    aligned = _ln_bwd_check(ops, f"layer_norm_bwd {M}x{C} aligned", x, dy, gamma)
    off = _ln_bwd_check(ops, f"layer_norm_bwd {M}x{C} at +8 bytes", shifted(x), shifted(dy), gamma)
    check_blocks("layer_norm_bwd +8 bytes against aligned dx", off, aligned.double(), R.DX_TOL[dt])
