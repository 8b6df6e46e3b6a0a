"""CPU checks of what tests/test_norm_edges_gpu.py relies on (no GPU):

  * the plan table: every seam of gn_fused_plan / group_norm_launch, the thread count on each side and the last one-launch row count, read
    from a3d_group_norm_plan, equal the table in tests/norm_ref.py (so the GPU cases sit where the kernels change);
  * mutation checks on the float64 references alone: for every layout the GPU tests use, a reference with one classic kernel mistake built
    in (a row left out of the statistics / group sums, a boundary channel counted next door, a lane's chunks left out of a LayerNorm row, a
    row past the range counted into dgamma / dbeta) must exceed the GPU test's bound by >= 4 x under the GPU test's measure.  The bounds
    are those of bf16, the wider of the two storage types (fp16's are 4 x tighter on the same values).
"""
import pytest
import torch

from tests import norm_ref as R

BF = torch.bfloat16
MARGIN = 4.0
EPS = 1e-5


@pytest.fixture(scope="module")
def plan():
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    return hip_ops.group_norm_plan


# ------------------------------------------------------------------ plan table
@pytest.mark.parametrize("C", sorted(R.GN_PLAN_TABLE))
def test_plan_table(plan, C):
    want, last_fused = R.GN_PLAN_TABLE[C]
    got, prev = [], None
    for rows in range(1, last_fused + 1):
        p = plan(rows, C, R.GROUPS)
        assert p["fused"] == 1, (C, rows)
        assert p["nx"] * p["ny"] <= p["threads"] and p["nx"] == p["sg"] * (C // R.GROUPS) // 8 and p["iters"] <= p["rmax"], (C, rows, p)
        key = (p["threads"], p["rmax"], p["sg"])
        if key != prev:
            got.append((rows, *key))
            prev = key
    assert got == want
    three = plan(last_fused + 1, C, R.GROUPS)
    assert three["fused"] == 0 and three["nx"] == C // 8 and three["ny"] == min(32, max(1, 256 // (C // 8))), three


def test_seams_change_the_named_field(plan):
    for C, lo, hi, field in R.GN_SEAMS:
        a, b = plan(lo, C, R.GROUPS), plan(hi, C, R.GROUPS)
        assert hi == lo + 1 and a[field] != b[field], (C, lo, hi, field, a, b)
    p = plan(12, 1280, R.GROUPS)
    assert p["ny"] == 12 and p["fused"] == 1          # rows 11 | 12 | 13 of GN_EXTRA_ROWS: below, at and above the row lanes


def test_plan_query_refuses_what_the_launch_refuses(plan):
    from animate3d_amd import hip_ops
    lib = hip_ops.load_library()
    out = (hip_ops.c_int * 7)()
    for rows, C, groups in ((0, 320, 32), (64, 324, 32), (64, 320, 64), (64, 192, 32), (64, 320, 0), (64, 8200 * 8, 8), (64, 4 * 1032, 1032)):
        assert lib.a3d_group_norm_plan(rows, C, groups, out) == -1, (rows, C, groups)
    assert lib.a3d_group_norm_plan(64, 320, 32, None) == -1
    for cg in (4, 7, 9):
        assert plan(100, cg * 32, 32)["fused"] == 1


# ------------------------------------------------------------------ mutation checks: GroupNorm forward
def _gn_forward_layouts(plan):
    out = [(C, rows) for C, rows in R.gn_forward_rows()]
    out += [(320, rows) for rows in R.gn_tail_rows(plan(1 << 20, 320, R.GROUPS)["ny"])]
    out += [(Ca + Cb, rows) for rows, Ca, Cb in R.GN2_CASES]
    return sorted(set(out))


def _boundary_channels(C, groups, sg):
    """Four group boundaries: the first channel of group 1 and of the last group counted one group down, the last channel in front of
    the first slab boundary and of group 2 counted one group up."""
    cg = C // groups
    slab = sg if 0 < sg < groups else groups // 2
    return [cg, (groups - 1) * cg, slab * cg - 1, 2 * cg - 1]


def gn_forward_mutants(plan, C, rows, iid):
    """Smallest excess (error / bound: the GPU test's measure) over the mutants of the layout, behind the SiLU (slope <= 1.1: an excess
    e there is at least e / 1.1 without it; the bound is the same).  A row mutant shows only in the instance whose probe row it drops;
    a channel mutant is wrong in every instance and the GPU test sees the worst element of the launch, so one instance has to show it:
    the one without a probe row where there is one (all of a small launch)."""
    p = plan(rows, C, R.GROUPS)
    probes = R.batch_probes(R.probe_rows(p, rows))
    B = len(probes)
    x, gamma, beta = R.structured(B, rows, C, R.GROUPS, probes, BF, seed=rows + C, iid=iid)
    ref, terms = R.gn_forward(x, B, rows, gamma, beta, R.GROUPS, EPS, True)
    bound = R.fwd_bound(terms, BF)
    worst = []
    bc = probes.index(None) if None in probes else 0
    one, nb = (slice(bc * rows, (bc + 1) * rows), 1) if B * rows * C > 1 << 20 else (slice(None), B)          # (small launches: all of it)
    for c in _boundary_channels(C, R.GROUPS, p["sg"]):
        mut, _ = R.gn_forward(x[one], nb, rows, gamma, beta, R.GROUPS, EPS, True, sums=R.gn_sums(x[one], nb, rows, R.GROUPS, shift_channel=c))
        worst.append(("channel", c, R.fwd_excess(mut, ref[one], bound[one])[0]))
    if rows > 1:
        w = torch.ones(B, rows, dtype=torch.float64)
        for b, r in enumerate(probes):
            if r is not None:
                w[b, r] = 0.0
        mut, _ = R.gn_forward(x, B, rows, gamma, beta, R.GROUPS, EPS, True, sums=R.gn_sums(x, B, rows, R.GROUPS, row_weight=w))
        per = ((mut - ref).abs() / bound).reshape(B, -1).max(dim=1).values
        worst += [("row", (b, r), float(per[b])) for b, r in enumerate(probes) if r is not None]
    return min(worst, key=lambda t: t[-1])


def test_group_norm_forward_mutants_exceed_the_bound(plan):
    for C, rows in _gn_forward_layouts(plan):
        kind, at, excess = gn_forward_mutants(plan, C, rows, iid=False)
        assert excess >= 1.1 * MARGIN, f"C={C} rows={rows}: mutant {kind} at {at} is only {excess:.2f} x the bound"


def test_group_norm_sums_mutants_exceed_the_bound(plan):
    """A row left out / a channel next door against |d sum| <= n 2^-24 sum|x| (and the sum of squares alike)."""
    for C in R.GN_SUMS_WIDTHS:
        n = R.sums_chain(plan(1 << 20, C, R.GROUPS)["ny"], C, R.GROUPS)
        for rows in R.GN_SHARD_ROWS:
            probes = R.batch_probes(R.probe_rows(dict(fused=0, ny=plan(1 << 20, C, R.GROUPS)["ny"]), rows))
            x, _, _ = R.structured(len(probes), rows, C, R.GROUPS, probes, BF, seed=C + rows)
            B = len(probes)
            ref = R.gn_sums(x, B, rows, R.GROUPS)
            bound = n * 2.0 ** -24 * R.gn_sums(x.abs(), B, rows, R.GROUPS)
            muts = [R.gn_sums(x, B, rows, R.GROUPS, shift_channel=c) for c in _boundary_channels(C, R.GROUPS, 0)]
            if rows > 1:
                w = torch.ones(B, rows, dtype=torch.float64)
                for b, r in enumerate(probes):
                    if r is not None:
                        w[b, r] = 0.0
                muts.append(R.gn_sums(x, B, rows, R.GROUPS, row_weight=w))
            for m in muts:
                assert float(((m - ref).abs() / bound).max()) >= MARGIN, (C, rows)


# ------------------------------------------------------------------ mutation checks: GroupNorm backward
def gn_backward_mutants(B, rows, C, groups, iid):
    probes = R.gn_bwd_probes(B, rows, C)
    nb = min(B, 6)                                    # instances beyond the distinct probe rows repeat them
    x, gamma, beta = R.structured(B, rows, C, groups, probes, BF, seed=B + rows + C, iid=iid)
    dy = R.structured_dy(x, B, rows, C, groups, probes, BF, seed=B + rows + C, iid=iid)
    out = {}
    for act in (False, True):
        _, rg, rb = R.gn_backward(x, dy, B, rows, gamma, beta, groups, EPS, act)
        b_last = probes.index(rows - 1)
        _, mg, mb = R.gn_backward(x, dy, B, rows, gamma, beta, groups, EPS, act, extra_row=(b_last, rows - 1))
        out["param", act] = min(R.rel_l2(mg, rg), R.rel_l2(mb, rb)) / R.PARAM_TOL
        if rows > 1:
            xs, ds = x[:nb * rows], dy[:nb * rows]
            rx, _, _ = R.gn_backward(xs, ds, nb, rows, gamma, beta, groups, EPS, act)
            w = torch.ones(nb, rows, dtype=torch.float64)
            for b in range(nb):
                w[b, probes[b]] = 0.0
            mx, _, _ = R.gn_backward(xs, ds, nb, rows, gamma, beta, groups, EPS, act, row_weight=w)
            per = ((R.gn_blocks(mx, nb, rows, groups) - R.gn_blocks(rx, nb, rows, groups)).norm(dim=-1)
                   / R.gn_blocks(rx, nb, rows, groups).norm(dim=-1)).reshape(nb, groups)
            # every instance must show its dropped row in its worst group (the GPU test takes the maximum over blocks; behind a SiLU the
            # probe row of a negative-mean group carries no gradient, so not every group can)
            out["row", act] = float(per.max(dim=1).values.min()) / R.DX_TOL[BF]
    return out


def test_group_norm_backward_mutants_exceed_the_bound():
    for B, rows, C, groups in R.gn_bwd_cases():
        for key, excess in gn_backward_mutants(B, rows, C, groups, iid=False).items():
            assert excess >= MARGIN, f"B={B} rows={rows} C={C} groups={groups}: mutant {key} is only {excess:.2f} x the bound"


# ------------------------------------------------------------------ mutation checks: LayerNorm
def _ln_layouts():
    fwd = [(M, C, "chunks") for M, C in R.LN_FWD_GENERIC] + [(M, C, "rows") for C in R.LN_ROWS_WIDTHS for M in R.ln_rows_seams(C)]
    bwd = [(M, C, "elems", True) for M, C in R.LN_BWD_GENERIC] + [(37, 320, "elems", True)]
    bwd += [(M, C, "rows", True) for C in R.LN_ROWS_WIDTHS for M in R.ln_rows_seams(C)] + [(M, C, "rows", p) for M, C, p in R.LN_BWD_LOOPS]
    return fwd, bwd


def _lanes(C, kind):
    n = C // 40 if kind == "rows" else min(64, C // 8 if kind == "chunks" else C)
    return sorted({0, n // 2, n - 1})


def ln_forward_mutants(M, C, kind, iid):
    probes = R.ln_probes(M, C)
    x, gamma, beta = R.structured_rows(M, C, probes, BF, seed=M + C, iid=iid)
    pe = (0.5 * torch.randn(3, C, generator=torch.Generator().manual_seed(5))).to(BF)
    (ref, terms), _ = R.ln_forward(x, gamma, beta, EPS, pe1=pe, pe1_div=2)
    bound = R.fwd_bound(terms, BF)
    worst = float("inf")
    for r in probes:
        for lane in _lanes(C, kind):
            (mut, _), _ = R.ln_forward(x[r:r + 1], gamma, beta, EPS, pe1=pe[((r // 2) % 3):((r // 2) % 3) + 1], skip=(0, R.ln_lane_mask(C, kind, lane)))
            worst = min(worst, R.fwd_excess(mut, ref[r:r + 1], bound[r:r + 1])[0])
    return worst


def ln_backward_mutants(M, C, kind, param, iid):
    probes = R.ln_probes(M, C)
    x, gamma, _ = R.structured_rows(M, C, probes, BF, seed=M + C, iid=iid)
    dy = R.structured_rows_dy(x, gamma, probes, BF, seed=M + C, iid=iid)
    out = {}
    worst = float("inf")
    for r in probes:
        rx, _, _ = R.ln_backward(x[r:r + 1], dy[r:r + 1], gamma, EPS)
        for lane in _lanes(C, kind):
            mx, _, _ = R.ln_backward(x[r:r + 1], dy[r:r + 1], gamma, EPS, skip=(0, R.ln_lane_mask(C, kind, lane)))
            worst = min(worst, R.block_rel_l2(mx, rx) / R.DX_TOL[BF])
    out["lane"] = worst
    if param:
        _, rg, rb = R.ln_backward(x, dy, gamma, EPS)
        _, mg, mb = R.ln_backward(x, dy, gamma, EPS, extra_row=M - 1)
        out["param"] = min(R.rel_l2(mg, rg), R.rel_l2(mb, rb)) / R.PARAM_TOL
    return out


def test_layer_norm_forward_mutants_exceed_the_bound():
    for M, C, kind in _ln_layouts()[0]:
        excess = ln_forward_mutants(M, C, kind, iid=False)
        assert excess >= MARGIN, f"M={M} C={C}: a lane left out is only {excess:.2f} x the bound"


def test_layer_norm_backward_mutants_exceed_the_bound():
    for M, C, kind, param in _ln_layouts()[1]:
        for key, excess in ln_backward_mutants(M, C, kind, param, iid=False).items():
            assert excess >= MARGIN, f"M={M} C={C}: mutant {key} is only {excess:.2f} x the bound"


# ------------------------------------------------------------------ the counter-example: `randn + 0.5` in every row, channel and group
def test_iid_inputs_hide_the_backward_and_one_wave_mutants():
    """The same mutation checks on iid inputs fall short of the margin: a row left out of the GroupNorm backward's group sums (every
    case), a lane left out of a LayerNorm row in the backward (one-wave kernel; rows kernel at C = 1280) and in the one-wave forward at
    C = 512 / 768 / 1024.  (Not everything hides: the per-element forward measure is sharp enough that a GroupNorm forward mutant or a
    lane of the forward rows kernel shows 4 - 100 x on iid inputs too — structured inputs raise that to 50 - 800 x — and a row counted
    twice in dgamma / dbeta always shows among few rows.)"""
    for B, rows, C, groups in R.gn_bwd_cases():
        if rows > 100:                                # (among a handful of rows a missing one shows on any input)
            got = gn_backward_mutants(B, rows, C, groups, iid=True)
            assert max(got["row", False], got["row", True]) < MARGIN, (B, rows, C, got)
    for M, C in [(7, 100), (7, 648), (7, 2048)]:
        assert ln_backward_mutants(M, C, "elems", False, iid=True)["lane"] < MARGIN, (M, C)
    for M in R.ln_rows_seams(1280):
        assert ln_backward_mutants(M, 1280, "rows", False, iid=True)["lane"] < MARGIN, M
    for C in (512, 768, 1024):
        assert ln_forward_mutants(7, C, "chunks", iid=True) < MARGIN, C


@pytest.mark.parametrize("C,rows", [(1280, 2142), (320, 2143)])
def test_iid_inputs_pass_the_global_bar_with_a_row_left_out(plan, C, rows):
    """What the suite could not see: under the whole-tensor measure of tests/test_hip_kernels_gpu.py (3 ulps of the output's maximum) a
    GroupNorm that leaves a row out of its statistics passes on iid inputs, and is far outside on structured ones."""
    p = plan(rows, C, R.GROUPS)
    probes = R.batch_probes(R.probe_rows(p, rows))
    B = len(probes)
    w = torch.ones(B, rows, dtype=torch.float64)
    for b, r in enumerate(probes):
        if r is not None:
            w[b, r] = 0.0
    ulps = {}
    for iid in (True, False):
        x, gamma, beta = R.structured(B, rows, C, R.GROUPS, probes, BF, seed=rows + C, iid=iid)
        ref, _ = R.gn_forward(x, B, rows, gamma, beta, R.GROUPS, EPS, False)
        mut, _ = R.gn_forward(x, B, rows, gamma, beta, R.GROUPS, EPS, False, sums=R.gn_sums(x, B, rows, R.GROUPS, row_weight=w))
        ulps[iid] = float((mut - ref).abs().max() / (ref.abs().max() * 2.0 ** -8))
    assert ulps[True] < 3.0 <= 3.0 * MARGIN < ulps[False], ulps
