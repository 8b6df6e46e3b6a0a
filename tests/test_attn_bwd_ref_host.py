"""CPU checks of what tests/test_attn_bwd_edges_gpu.py relies on (no GPU, no kernel):

  * ``exact`` of tests/attn_bwd_ref.py equals torch autograd in float64 through the forward reference, on every map of the case table
    (q_len != kv_len, shared key groups, do_scale), and its temporal twin equals autograd through the temporal forward reference;
  * every case of the table reaches the (variant, body) per pass it claims, according to the mirror of csrc/attn_bwd.hip's dispatch, and
    the table as a whole reaches every cell that exists, for each of the four head dims; the first-frame cases at the suite's sizes take
    the host's partials route, and the column count 136 leaves 8 valid columns in the second workgroup;
  * the bars bite: ``row_report`` rejects five deliberately wrong variants of the rounding model (``mutant=``), each on the case built
    for it, while the unmodified model passes (worst row ratios of 140 and more against a bar of 2).  At the small shapes of the table
    the whole-tensor bar sees whole-launch mistakes too; a mistake confined to ONE row of 512 (a neighbouring head's statistic on one
    query) passes the whole-tensor bar and fails the row bar, which is the reason for the row bar.
"""
import pytest
import torch

from tests import attn_bwd_ref as R

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def _autograd(c, tensors, q_per_kv, do_scale):
    q, k, v, do = tensors
    with torch.enable_grad():
        qf, kf, vf = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
        C = q.shape[1]
        D = C // c.heads
        qi = R.rowmap_indices(c.qmap, c.groups, c.q_len)
        ki = R.rowmap_indices(c.kmap, c.groups, c.kv_len)
        sh = lambda t, i, n: t[i].reshape(c.groups, n, c.heads, D).transpose(1, 2)
        p = torch.softmax(sh(qf, qi, c.q_len) @ sh(kf, ki, c.kv_len).transpose(-1, -2) * D ** -0.5, dim=-1)
        o = (p @ sh(vf, ki, c.kv_len)).transpose(1, 2).reshape(c.groups * c.q_len, C) * do_scale
        (o * do.double()[qi.reshape(-1)]).sum().backward()
    return qf.grad, kf.grad, vf.grad, o.detach(), qi


@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_exact_equals_float64_autograd(D):
    for c in R.cases(D).values():
        tensors = R.make_inputs(c, torch.bfloat16, regime="randn")
        ex = R.exact(*R.case_args(c, tensors), q_per_kv=c.q_per_kv, do_scale=c.do_scale)
        dq, dk, dv, o, qi = _autograd(c, tensors, c.q_per_kv, c.do_scale)
        for name, a, b in (("dq", ex.dq, dq), ("dk", ex.dk, dk), ("dv", ex.dv, dv), ("o", ex.o[qi.reshape(-1)], o)):
            err = float((a - b).abs().max())
            assert err <= 1e-12 * max(1.0, float(b.abs().max())), (c.name, name, err)
        # lse2 against a direct evaluation of the definition
        q, k = tensors[0].double(), tensors[1].double()
        g, h = c.groups - 1, c.heads - 1
        qr = R.rowmap_indices(c.qmap, c.groups, c.q_len)[g]
        kr = R.rowmap_indices(c.kmap, c.groups, c.kv_len)[g]
        s = q[qr][:, h * D:(h + 1) * D] @ k[kr][:, h * D:(h + 1) * D].t() * D ** -0.5
        assert float((ex.lse2[g, h] - torch.log2(torch.exp(s).sum(-1))).abs().max()) < 1e-12, c.name


@pytest.mark.parametrize("F,D,C,L", [(1, 40, 320, 3), (2, 80, 320, 1), (17, 160, 640, 3), (32, 40, 640, 1)])
def test_exact_temporal_equals_float64_autograd(F, D, C, L):
    videos, heads = 2, C // D
    g = torch.Generator().manual_seed(F)
    q, k, v, do = (torch.randn(videos * F * L, C, generator=g).to(torch.bfloat16) for _ in range(4))
    with torch.enable_grad():
        leaves = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
        seq = lambda t: t.reshape(videos, F, L, heads, D).permute(0, 2, 3, 1, 4)          # TorchRefOps.temporal_attn, without its .float()
        p = torch.softmax(seq(leaves[0]) @ seq(leaves[1]).transpose(-1, -2) * D ** -0.5, dim=-1)
        (p @ seq(leaves[2])).permute(0, 3, 1, 2, 4).reshape(videos * F * L, C).backward(do.double())
    for a, b in zip(R.exact_temporal(q, k, v, do, videos, F, L, heads), leaves):
        assert float((a - b.grad).abs().max()) <= 1e-12 * max(1.0, float(b.grad.abs().max()))


# ------------------------------------------------------------------ the launch matrix
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_every_case_reaches_the_variants_it_claims_and_the_table_covers_every_cell(D):
    reached = {p: set() for p in R.PASSES}
    table = R.cases(D)
    for c in table.values():
        for p in R.PASSES:
            got = R.launch_variant(D, p, c.qmap, c.kmap, c.q_len, c.kv_len, ld_max=3 * c.C)
            assert got == c.claims[p], (D, c.name, p, got, c.claims[p])
            reached[p].add(got)
    for p in R.PASSES:
        assert reached[p] == R.CELLS[p], (D, p, R.CELLS[p] - reached[p], reached[p] - R.CELLS[p])
    B = R.BR[D]
    # the geometry the cases are named for
    assert table["cross77"].kv_len == 77 and table["cross77"].q_len == 2 * B and table["cross77"].q_per_kv == 3
    wide = table["cols136" if "cols136" in table else "identity_ragged"]
    assert wide.q_len == wide.kv_len == 136
    for p in R.PASSES:
        assert R.column_tiles(D, p, wide.q_len, wide.kv_len) == (2, 8)
    # the suite's first-frame and cross sizes go by per-group partials through HipOps; the smallest shape the issue names clears the threshold
    for name in ("first_frame", "first_frame_ragged", "cross77"):
        c = table[name]
        assert R.dkv_route(c.groups, c.heads, c.kv_len, c.q_per_kv) == "partials"
    assert R.dkv_route(16 * 3, 8, 512, 3) == "kernel" and (16 * 8 * 4) == R.SHARED_WG_THRESHOLD
    assert R.dkv_route(15 * 3, 8, 512, 3) == "partials"


# ------------------------------------------------------------------ the bars bite
def _reports(c, dtype, regime, mutant, route="kernel", stats="recompute"):
    tensors = R.make_inputs(c, dtype, regime=regime)
    kw = dict(q_per_kv=c.q_per_kv, do_scale=c.do_scale)
    ex = R.exact(*R.case_args(c, tensors), **kw)
    model = R.rounded(*R.case_args(c, tensors), storage=dtype, stats=stats, route=route, **kw)
    wrong = R.rounded(*R.case_args(c, tensors), storage=dtype, stats=stats, route=route, mutant=mutant, **kw)
    out = {}
    for t, rows in (("dq", ex.q_index), ("dk", ex.k_index), ("dv", ex.k_index)):
        good = R.row_report(getattr(model, t), getattr(ex, t), getattr(model, t), rows=rows, tol=R.ATTN_TOL[dtype], name=f"model {t}")
        bad = R.row_report(getattr(wrong, t), getattr(ex, t), getattr(model, t), rows=rows, tol=R.ATTN_TOL[dtype],
                           name=f"{mutant} {c.name} D={c.D} {regime} {t}")
        print(bad.line())
        assert good.ok and good.ratio == 1.0 and good.stray == 0, good.line()
        out[t] = bad
    return out


# (mutant, case, value regime, gradients that must be rejected)
MUTANT_CASES = [("clamped_key_twice", "ragged_self", "randn", ("dq", "dk", "dv")),
                ("clamped_key_twice", "ragged_self", "planted", ("dq", "dk", "dv")),
                ("last_row_tile_dropped", "dma_self", "randn", ("dq", "dk", "dv")),
                ("first_group_stats", "first_frame", "randn", ("dk", "dv")),
                ("first_group_stats", "first_frame_ragged", "randn", ("dk", "dv")),
                ("neighbour_head_lse", "dma_self", "randn", ("dq", "dk", "dv")),
                ("neighbour_head_lse", "cross77", "randn", ("dq", "dk", "dv")),
                ("key_row_shifted", "dma_self", "randn", ("dk", "dv")),
                ("key_row_shifted", "ragged_self", "randn", ("dk", "dv"))]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", R.HEAD_DIMS)
@pytest.mark.parametrize("mutant,case,regime,must_fail", MUTANT_CASES)
def test_row_report_rejects_the_wrong_models(mutant, case, regime, must_fail, D, dtype):
    c = R.cases(D)[case]
    rep = _reports(c, dtype, regime, mutant)
    for t in must_fail:
        assert not rep[t].ok and rep[t].ratio > R.ROW_MARGIN, rep[t].line()


def test_one_wrong_row_passes_the_whole_tensor_bar_and_fails_the_row_bar():
    dtype = torch.bfloat16
    c = R.cases(40)["dma_self"]
    tensors = R.make_inputs(c, dtype)
    ex = R.exact(*R.case_args(c, tensors))
    model = R.rounded(*R.case_args(c, tensors), storage=dtype)
    wrong = R.rounded(*R.case_args(c, tensors), storage=dtype, mutant="neighbour_head_lse")
    got = model.dq.clone()
    got[ex.q_index[300]] = wrong.dq[ex.q_index[300]]
    rep = R.row_report(got, ex.dq, model.dq, rows=ex.q_index, tol=R.ATTN_TOL[dtype], name="one query row with the neighbouring head's lse")
    print(rep.line())
    assert rep.rel_kernel <= rep.tol                # the whole-tensor bar does not see it
    assert rep.row == int(ex.q_index[300]) and rep.ratio > 10 * R.ROW_MARGIN and not rep.ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_partials_route_is_its_own_model(dtype):
    """The host's partials route stores every group's dK | dV in 16 bits before summing: a rounding the in-kernel loop does not have.  Both
    models pass their own bars; neither is the other bit for bit (so the GPU test must name the route it ran)."""
    c = R.cases(80)["first_frame_ragged"]
    tensors = R.make_inputs(c, dtype)
    kw = dict(q_per_kv=c.q_per_kv, do_scale=c.do_scale, storage=dtype)
    a = R.rounded(*R.case_args(c, tensors), route="kernel", **kw)
    b = R.rounded(*R.case_args(c, tensors), route="partials", **kw)
    ex = R.exact(*R.case_args(c, tensors), q_per_kv=c.q_per_kv)
    assert torch.equal(a.dq, b.dq) and not torch.equal(a.dk, b.dk) and not torch.equal(a.dv, b.dv)
    for t in ("dk", "dv"):
        assert R.row_report(getattr(b, t), getattr(ex, t), getattr(b, t), rows=ex.k_index, tol=R.ATTN_TOL[dtype]).ok
        other = ex.k_index.new_tensor(sorted(set(range(c.k_rows)) - set(ex.k_index.tolist())))
        assert float(getattr(ex, t)[other].abs().max()) == 0.0          # frames > 0 hold no keys: their gradient rows are zero


def test_row_report_counts_stray_writes_and_non_finite_values():
    ex = torch.zeros(6, 8, dtype=torch.float64)
    ex[:3] = 1.0
    model = ex + 1e-3
    rows = torch.arange(3)
    model[3:] = 0.0
    got = model.clone()
    assert R.row_report(got, ex, model, rows=rows).ok
    got[4, 2] = 1e-30
    assert R.row_report(got, ex, model, rows=rows).stray == 1 and not R.row_report(got, ex, model, rows=rows).ok
    got = model.clone()
    got[1, 1] = float("nan")
    assert not R.row_report(got, ex, model, rows=rows).ok
    got = model.clone()
    got[2] += 2.1e-3                                                    # one row at 3.1 x the model's error
    rep = R.row_report(got, ex, model, rows=rows)
    assert rep.row == 2 and 3.0 < rep.ratio < 3.2 and not rep.ok
    assert not R.row_report(model, ex, model, rows=rows, tol=1e-6).ok     # the whole-tensor bar is part of ok
