"""Host (CPU) tests of tests/gemm_ref.py, the float64 oracle of the GEMM / implicit-GEMM convolution family: the oracles agree with
independent statements of the same operations, the exact inputs are exact in fp32 arithmetic in three summation orders (and the GEGLU
gates are pinned under an fp32 restatement of gelu_erf), every wrong kernel of MUTANTS is rejected by the exact comparison and by the
per-element bound, the case table reaches every dispatch cell, and the Python mirror of the dispatch reproduces every routing fact the
GPU tests of tests/test_hip_kernels_gpu.py assert.

The mutant test also records which wrong kernels the whole-tensor bar of tests/test_hip_kernels_gpu.py (relative L2 <= 4e-3 in bf16,
1e-3 in fp16) accepts and prints the list ([gemm-ref] lines): that list is the reason tests/test_gemm_edges_gpu.py exists.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R
from tests.torch_ops import TorchRefOps

BF, FP = R.BF, R.FP
IDS = {BF: "bf16", FP: "fp16"}
BIG = 2_500_000          # output elements above which a case joins the mutant test only if named below
MUTANT_BIG = ("pp4-8192x1280x64-res0-bias1-rb0", "pp4-8192x1280x64-res1-bias1-rb256", "two-k1-64", "two-k1-last")


def _mutant_cases():
    return [c for c in R.CASES if c.kind != "f32out" and (c.dims()[0] * c.dims()[1] <= BIG or c.name in MUTANT_BIG)]


# ------------------------------------------------------------------ oracles against independent statements
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up", [(2, 5, 7, 64, 8, 1, 0), (2, 5, 7, 64, 8, 2, 0), (3, 6, 8, 64, 8, 2, 0), (2, 1, 7, 64, 4, 1, 0), (2, 5, 1, 64, 4, 2, 0),
                                                       (2, 3, 5, 64, 8, 1, 1), (2, 3, 5, 64, 8, 1, 3), (2, 3, 5, 64, 8, 1, 5), (2, 3, 5, 64, 8, 1, 7), (1, 1, 1, 64, 4, 1, 7)])
def test_conv_oracle_against_conv2d(B, H, W, Cin, Cout, stride, up):
    """Zero pad + nine shifted slices + one matmul == F.conv2d in float64 on the CPU; the crops == F.interpolate(mode="nearest") to the forced size."""
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(B * H * W, Cin, generator=g).to(BF), torch.randn(Cout, 9 * Cin, generator=g).to(BF)
    bias, He, We = torch.randn(Cout, generator=g), *R.conv_extents(H, W, stride, up)[:2]
    got, Ho, Wo = R.conv3x3(x, B, H, W, w, bias, stride, up)
    img = x.double().reshape(B, H, W, Cin).permute(0, 3, 1, 2)
    if up:
        img = F.interpolate(img, size=(He, We), mode="nearest")
    want = F.conv2d(img, w.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2), bias.double(), stride=stride, padding=1)
    assert want.shape[2:] == (Ho, Wo)
    want = want.permute(0, 2, 3, 1).reshape(B * Ho * Wo, Cout)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()


def test_dense_oracles_against_torch_ops():
    """The epilogue and GEGLU oracles against tests/torch_ops.py (fp32 arithmetic from the same 16-bit inputs)."""
    ref = TorchRefOps(act_dtype=torch.float64)
    g = torch.Generator().manual_seed(5)
    M, N, K = 77, 128, 192
    x, w = torch.randn(M, K, generator=g).to(BF), (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
    bias, rb, res = torch.randn(N, generator=g), torch.randn(4, N, generator=g).to(BF), torch.randn(M, N, generator=g).to(BF)
    for kw in (dict(), dict(residual=res, alpha=0.37, beta=0.9), dict(rowbias=rb, rb_div=20), dict(rowbias=rb, rb_div=20, residual=res, alpha=1.7)):
        assert R.rel_l2(R.gemm(x, w, bias, **kw), ref.gemm(x, w, bias, **kw)) < 1e-6
    assert R.rel_l2(R.gemm2(x[:, :64], x[:, 64:], w, bias), ref.gemm2(x[:, :64], x[:, 64:], w, bias)) < 1e-6
    w_il, b_il = R.interleave(w), R.interleave(bias)
    assert torch.equal(R.deinterleave(w_il), w) and torch.equal(w_il, TorchRefOps.interleave_geglu(w))
    assert R.rel_l2(R.geglu(x, w, bias), ref.gemm_geglu(x, w_il, b_il)) < 1e-6
    kw = R.kwalk(9 * 128, True)
    assert sorted(kw.tolist()) == list(range(9 * 128)) and kw[64].item() == 128 and kw[9 * 64].item() == 64     # tap 1 of slice 0; tap 0 of slice 1


# ------------------------------------------------------------------ exact inputs are exact
def _gelu_erf_f32(g):
    """gelu_erf of csrc/gemm_common.h in fp32 numpy (an fma = the double-precision expression rounded once); returns (gelu, erfx)."""
    f = np.float32
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    c = lambda v: np.full_like(g, v, dtype=f)
    x = np.abs(g) * f(0.70710678118654752)
    t = f(1.0) / fma(c(0.3275911), x, c(1.0))
    poly = fma(c(1.061405429), t, c(-1.453152027))
    for a in (1.421413741, -0.284496736, 0.254829592):
        poly = fma(poly, t, c(a))
    poly = poly * t
    with np.errstate(under="ignore"):
        e = np.exp2(-x * x * f(1.4426950408889634)).astype(f)
    erfx = fma(-poly, e, c(1.0))
    hg = f(0.5) * g
    return fma(np.abs(hg), erfx, hg), erfx


def _fp32_orders(A, W, kw):
    """fp32 accumulation of A W^T over 64-wide K-tiles taken in the kernels' K walk: forward, reversed, and 16 slices summed in index order."""
    tiles = [kw[i:i + 64] for i in range(0, len(kw), 64)]
    part = lambda ks: A[:, ks] @ W[:, ks].t()

    def chain(seq):
        acc = torch.zeros(A.shape[0], W.shape[0])
        for ks in seq:
            acc = acc + part(ks)
        return acc

    yield "forward", chain(tiles)
    yield "reversed", chain(tiles[::-1])
    n = min(16, len(tiles))
    bounds = [len(tiles) * i // n for i in range(n + 1)]
    slices = [chain(tiles[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    acc = slices[0]
    for s in slices[1:]:
        acc = acc + s
    yield "16 slices", acc


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS.values())
@pytest.mark.parametrize("case", [c for c in R.CASES if c.exact], ids=lambda c: c.name)
def test_exact_inputs_are_exact(case, dtype):
    """exact_inputs() asserts its conditions in float64 (sums bound, fp16 range, >= 10 % inexact outputs, ties of both parities); here fp32
    arithmetic itself — the accumulators' type — reproduces the float64 result in three orders, through the kernels' epilogue expression."""
    inp = R.case_inputs(case, dtype, "exact")
    want = inp["exact64"].float()
    assert torch.equal(want.double(), inp["exact64"])
    M, N, K = case.dims()
    A = R.case_A(case, inp).float()
    W = inp["w"].float()
    for order, acc in _fp32_orders(A, W, R.kwalk(K, case.conv)):
        if case.kind == "geglu":
            hg = acc + inp["bias"]
            h, g = hg.chunk(2, dim=1)
            gel, erfx = _gelu_erf_f32(g.numpy())
            assert (erfx == 1.0).all(), "a gate is not pinned: erfx != 1.0f"
            v = h * torch.from_numpy(gel)
        else:
            v = acc
            if inp["bias"] is not None:
                v = v + inp["bias"]
            if inp["rowbias"] is not None:
                v = v + inp["rowbias"].float()[torch.arange(M) // case.rb_div]
            v = v * torch.tensor(inp["alpha"], dtype=torch.float32)
            if inp["residual"] is not None:
                v = v + torch.tensor(inp["beta"], dtype=torch.float32) * inp["residual"].float()       # beta r is exact: one rounding, as the fma
        bad = R.mismatches(v, want)
        assert not bad.any(), f"{case.name} {order}: fp32 arithmetic differs from float64 in {int(bad.sum())} elements"


# ------------------------------------------------------------------ every mutant is rejected
def test_every_mutant_is_rejected_and_the_old_bar_accepts_some(capsys):
    applied = {m: 0 for m in R.MUTANTS}
    old_bar_accepts = {m: [] for m in R.MUTANTS}
    weakest = {}
    for case in _mutant_cases():
        for dtype in R.DTYPES:
            tag = f"{case.name}/{IDS[dtype]}"
            rnd = R.case_inputs(case, dtype, "random")
            ref, bound = R.case_bound(case, rnd, dtype)
            good = R.store(ref, dtype)
            ratio, _ = R.worst_ratio(good, ref, bound)
            assert ratio <= 1.0, f"{tag}: the correctly rounded float64 result exceeds elem_bound ({ratio:.3f})"
            ref32 = ref.float()                                     # the old bar's reference is fp32
            if case.exact:
                ex = R.case_inputs(case, dtype, "exact")
                want = R.expected(ex["exact64"], dtype)
                assert torch.equal(R.store(R.oracle(case, ex), dtype).float(), want.float()), f"{tag}: oracle(case) != exact64"
            # a truncating store errs by less than one ulp: elem_bound can see it only where its accumulation term (which grows as K^1.5
            # relative to the output) leaves room, here: where it is typically below a quarter ulp.  The exact comparison sees it always.
            hu = R.half_ulp(ref, dtype)
            trunc_visible = float(((bound - hu) / hu).median()) < 0.5
            for m in R.MUTANTS:
                out = R.mutant_output(m, case, rnd, dtype, y64=ref)
                if out is None:
                    continue
                applied[m] += 1
                r, _ = R.worst_ratio(out, ref, bound)
                if m != "truncating_store" or trunc_visible:
                    weakest[m] = min(weakest.get(m, float("inf")), r)
                assert r > 1.0 or (m == "truncating_store" and not trunc_visible), f"{tag}: mutant {m} stays inside elem_bound (worst ratio {r:.3f})"
                if R.rel_l2(out, ref32) <= R.OLD_BAR[dtype]:
                    old_bar_accepts[m].append(tag)
                if case.exact:
                    wrong = R.mutant_output(m, case, ex, dtype, y64=ex["exact64"])
                    assert wrong is not None and R.mismatches(wrong, want).any(), f"{tag}: mutant {m} equals the exact expected output"
    with capsys.disabled():
        for m, (what, _) in R.MUTANTS.items():
            acc = old_bar_accepts[m]
            print(f"[gemm-ref] mutant {m} ({what}): {applied[m]} case(s), weakest |err| / bound = {weakest.get(m, float('nan')):.1f}; "
                  f"the whole-tensor bar accepts it in {len(acc)}: {', '.join(acc[:4])}{' ...' if len(acc) > 4 else ''}")
    assert all(n > 0 for n in applied.values()), f"mutants that applied to no case: {[m for m, n in applied.items() if not n]}"
    accepted = [m for m, a in old_bar_accepts.items() if a]
    assert "truncating_store" in accepted and "chunk_from_neighbour" in accepted, accepted


# ------------------------------------------------------------------ coverage of the dispatch cells
def _required_cells():
    req = {}
    both = lambda name, pred: req.update({(name, IDS[dt]): pred for dt in R.DTYPES})
    for kern in ("tile128-bk32", "ring", "persist"):
        for res in (False, True):
            for bias in (False, True):
                for rb in (False, True):
                    both(f"{kern} RES{int(res)} bias{int(bias)} rowbias{int(rb)}",
                         lambda c, i, kern=kern, res=res, bias=bias, rb=rb: i["cell"].kernel == kern and i["cell"].RES == res and c.bias == bias
                         and bool(c.rb_div) == rb and i["cell"].EPI == "linear" and not i["cell"].CONV and not i["cell"].TWO)
    # the ring kernel needs K >= 256 (plan_ring), i.e. nk >= 4: nk = depth is reachable for the ring of four (nb 2) only; the rings of three
    # and two (nb 4, 5) are covered from nk = 4 = depth + 1 and depth + 2 up to two full turns
    for nb, nks in ((2, (4, 5)), (4, (4, 5, 6)), (5, (4, 5, 6))):
        for nk in nks:
            both(f"ring nb{nb} nk{nk}", lambda c, i, nb=nb, nk=nk: i["cell"].kernel == "ring" and i["cell"].nb == nb and i["nk"] == nk)
        both(f"ring nb{nb} several tiles per workgroup", lambda c, i, nb=nb: i["cell"].kernel == "ring" and i["cell"].nb == nb and i["items"] > i["grid"])
    for nb in (4, 5):
        both(f"persist nb{nb}", lambda c, i, nb=nb: i["cell"].kernel == "persist" and i["cell"].nb == nb)
    both("persist one round", lambda c, i: i["cell"].kernel == "persist" and i["rounds"] == 1)
    both("persist partial last round", lambda c, i: i["cell"].kernel == "persist" and i["rounds"] > 1 and i["items"] % i["grid"] != 0)
    both("persist several tiles per workgroup", lambda c, i: i["cell"].kernel == "persist" and i["rounds"] >= 4)
    both("split-K dense", lambda c, i: i["cell"].S > 1 and not i["cell"].CONV)
    both("split-K conv", lambda c, i: i["cell"].S > 1 and i["cell"].CONV == 1)
    both("two-source A", lambda c, i: i["cell"].TWO)
    both("GEGLU tile128", lambda c, i: i["cell"].EPI == "geglu" and i["cell"].kernel.startswith("tile128"))
    both("GEGLU persist", lambda c, i: i["cell"].EPI == "geglu" and i["cell"].kernel == "persist")
    for stride in (1, 2):
        both(f"CONV 1 stride {stride}", lambda c, i, s=stride: i["cell"].CONV == 1 and c.shape[5] == s)
        both(f"persist CONV 1 stride {stride}", lambda c, i, s=stride: i["cell"].CONV == 1 and c.shape[5] == s and i["cell"].kernel == "persist")
    for up in (1, 3, 5, 7):
        both(f"CONV 2 crop code {up}", lambda c, i, up=up: i["cell"].CONV == 2 and c.shape[6] == up)
    both("persist CONV 2", lambda c, i: i["cell"].CONV == 2 and i["cell"].kernel == "persist")
    for v in (True, False):
        both(f"vec16 {v}", lambda c, i, v=v: i["cell"].vec16 == v and not i["cell"].CONV)
        both(f"conv vec16 {v}", lambda c, i, v=v: i["cell"].vec16 == v and i["cell"].CONV)
    both("tile128-bk32", lambda c, i: i["cell"].kernel == "tile128-bk32")
    both("tile128-bk64", lambda c, i: i["cell"].kernel == "tile128-bk64")
    return req


def test_case_table_reaches_every_cell():
    """From plan() with cus = 256: every case sits in the cell it claims, and every required cell is reached (both storage types run every case)."""
    infos = [(c, R.case_plan(c, cus=256)) for c in R.CASES]
    for c, i in infos:
        assert i["cell"] == c.cell, f"{c.name}: claims {c.cell}, plan() says {i['cell']}"
        assert c.seam
    unreached = [name for name, pred in _required_cells().items() if not any(pred(c, i) for c, i in infos)]
    assert not unreached, f"unreached cells: {unreached}"


# ------------------------------------------------------------------ plan() against the routing facts of tests/test_hip_kernels_gpu.py
def test_plan_reproduces_the_routing_the_gpu_tests_assert():
    from tests.test_hip_kernels_gpu import _persistent_eligible
    kern = lambda *a, **kw: getattr(R.plan(*a, **kw), "kernel", None)
    # test_gemm_persistent_path / test_gemm_geglu_persistent_path(_without_bias) / test_conv3x3_persistent_path: _persistent_eligible holds, and
    # the default dispatch is the persistent kernel (K < 256 or the cost model keeps the ring kernel out)
    for M, N, K in [(65536, 320, 64), (65536, 320, 320), (65536, 640, 192), (65536, 256, 128), (49152, 1280, 128), (24576, 2560, 64), (8192, 1280, 128)]:
        assert _persistent_eligible(M, N) and kern("gemm", M, N, K) == "persist", (M, N, K)
        assert kern("gemm", M, N, K, residual=True, rb_div=4096) == "persist" and kern("gemm", M, N, K, flags=R.TILE128).startswith("tile128")
        assert kern("gemm", M, N, K, ldx=3 * K, ldy=2 * N) == "persist"
    assert R.plan("gemm", 8192, 1280, 128).nb == 4                      # "one round only -> the 256 x 256 tile (160 tiles) instead of 256 x 320"
    for M, N2, K in [(65536, 512, 64), (49152, 2560, 320)]:
        assert _persistent_eligible(M, N2, geglu=True) and kern("geglu", M, N2, K) == "persist" and kern("geglu", M, N2, K, bias=False) == "persist"
    for B, H, W, Cin, Cout, stride, up in [(16, 64, 64, 64, 320, 1, 0), (64, 32, 32, 128, 320, 1, 0), (64, 64, 64, 64, 320, 2, 0), (64, 32, 32, 64, 256, 1, 0),
                                           (256, 16, 16, 192, 640, 1, 0), (16, 32, 32, 64, 320, 1, 1), (64, 16, 16, 128, 256, 1, 1), (4, 64, 128, 64, 320, 1, 1)]:
        _, _, Ho, Wo = R.conv_extents(H, W, stride, up)
        assert _persistent_eligible(B * Ho * Wo, Cout)
        assert kern("conv", B * Ho * Wo, Cout, 9 * Cin, conv_geom=(B, H, W, Cin, up)) == "persist", (B, H, W, Cin, Cout)
    # agreement with _persistent_eligible off its own shapes too (K = 64: the ring kernel cannot compete)
    for M in (256, 2048, 8192, 16384, 16640, 32768, 65536, 300):
        for N in (128, 256, 320, 640, 960, 1280, 2560):
            assert (kern("gemm", M, N, 64) == "persist") == _persistent_eligible(M, N), (M, N)
    # test_gemm_ring_path: the ring kernel, except the two toss-ups that stay persistent
    ring_shapes = [(1024, 1280, 1280), (2048, 1280, 2560), (4096, 1280, 1280), (5120, 960, 320), (1024, 1280, 5120), (2048, 3840, 1280), (128, 128, 256),
                   (384, 640, 256), (16384, 128, 640), (1152, 2560, 704), (40960, 128, 256), (2048, 1280, 256), (38528, 960, 256)]
    for M, N, K in ring_shapes:
        assert kern("gemm", M, N, K) == "ring" and kern("gemm", M, N, K, rb_div=128, residual=True) == "ring", (M, N, K)
    assert [R.plan("gemm", *s).nb for s in [(128, 128, 256), (4096, 1280, 1280), (2048, 3840, 1280), (5120, 960, 320), (38528, 960, 256)]] == [2, 4, 4, 5, 5]
    for M, N, K in [(8192, 1280, 640), (16384, 640, 320)]:
        assert kern("gemm", M, N, K) == "persist" and kern("gemm", M, N, K, flags=R.RING) == "ring"
    # test_split_k_gemm / test_split_k_conv3x3: "the shape was expected to split"
    for M, N, K in [(8192, 1280, 1280), (2048, 3840, 1280), (2048, 1280, 5120), (8192, 1280, 2560), (4096, 640, 2304)]:
        i = R.plan_info("gemm", M, N, K, ws="query")
        assert i["ws_needed"] > 0 and i["cell"].S > 1 and i["ws_needed"] == i["tiles"] * i["cell"].S * i["cell"].nb * 65536, (M, N, K)
    for B, H, W, Cin, Cout in [(128, 8, 8, 1280, 1280), (32, 8, 8, 2560, 1280), (128, 4, 4, 1280, 1280), (16, 16, 16, 640, 640)]:
        i = R.plan_info("conv", B * H * W, Cout, 9 * Cin, conv_geom=(B, H, W, Cin, 0), ws="query")
        assert i["ws_needed"] > 0 and i["cell"].S > 1 and (Cin // 64) % i["cell"].S == 0, (B, H, W, Cin)
    # test_gemm_two_source_a_operand: taken at full M, None for 300 rows, and for 16384 rows at N = 320
    for M, Ka, Kb, N in [(32768, 1280, 640, 640), (65536, 640, 320, 320), (8192, 1280, 1280, 1280), (65536, 320, 320, 320)]:
        assert R.plan("gemm2", M, N, Ka + Kb, ldx=Ka) == R.Cell("persist", R.plan("gemm2", M, N, Ka + Kb, ldx=Ka).nb, 1, False, 0, "linear", True, True)
        assert R.plan("gemm2", 300, N, Ka + Kb, ldx=Ka) is None
        if N == 320:
            assert R.plan("gemm2", 16384, N, Ka + Kb, ldx=Ka) is None
