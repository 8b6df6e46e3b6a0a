"""GPU parity tests of the GEMM / implicit-GEMM convolution family, element by element, against the float64 oracle of tests/gemm_ref.py:
the 128 x 128 register-staged kernel (K-steps 32 and 64), the LDS-DMA ring kernel (tiles of 128, 256 and 320 columns), the persistent
kernel (256 x 256 / 256 x 320, split-K, two-source A, fused GEGLU) and the 3x3 convolutions on both, in bf16 and fp16 storage.

Every case of gemm_ref.CASES names the dispatch cell it claims and the seam it probes; the test first asserts, from gemm_ref.plan() with
the device's own CU count, that the case still reaches that cell (it fails, never skips, if it does not), then makes three checks:

1. exact inputs (integers on a dyadic grid, gemm_ref.exact_inputs): the output equals round-to-nearest-even of the float64 result in
   EVERY element — no tolerance, ties included.  A mismatch reports the count, the first (row, column) and the tile / wave / lane
   that owns it;
2. structured random inputs of realistic scale: |err| <= gemm_ref.elem_bound in every element (half an ulp of the store plus the fp32
   accumulation bound); prints ``[parity] name: worst |err| / bound``;
3. bit equality of the default dispatch with the forced 128 x 128 kernel and with another CU reservation, where
   tests/test_hip_kernels_gpu.py already claims it (everything but split-K); a3d_gemm2 against a3d_gemm on the concatenation.

The premise of check 1 — MFMA accumulation of such inputs is exact, in any order — is measured on its own through a3d_gemm_f32out
(test_accumulation_premise): fp32 output == float64 result, at one K-tile and at eighty.

Measured on an MI355X (256 CUs; 140 cases in 7 s): a3d_gemm_f32out's fp32 output equals the float64 result in all 17 544 elements at
K = 64 and at K = 5 120, both storage types — accumulation is exact, so the exact tests are not restricted.  Every exact comparison
holds in every element on every kernel.  Worst |err| / bound on the random inputs, bf16 / fp16: tile128-bk32 dense 0.997 / 0.984, conv
0.973 / 0.854, GEGLU 0.993 / 0.951; tile128-bk64 0.981 / 0.875; ring 0.993 / 0.946; persist dense 0.998 / 0.988, conv 0.982 / 0.884,
GEGLU 0.995 / 0.963; split-K dense 0.853 / 0.432, conv 0.806 / 0.398 (profiles/pytest_gpu_gemm_edges.log).
tests/test_gemm_ref_host.py shows on the CPU that thirteen wrong kernels fail these checks, and which of them the whole-tensor bar
of tests/test_hip_kernels_gpu.py lets through.
"""
import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

IDS = {R.BF: "bf16", R.FP: "fp16"}
CANARY = 24576.0          # exactly representable in both storage types, far from every output


@pytest.fixture(scope="module", params=R.DTYPES, ids=IDS.values())
def ops(request):
    from animate3d_amd.hip_ops import HipOps
    return HipOps(act_dtype=request.param)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sync():
    """A GPU fault ends the session: nothing more is launched on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # pragma: no cover
        pytest.exit(f"GPU fault, session ended: {e}", returncode=3)


def run(ops, c, inp, *, tile128=None, reserved=None):
    """Launch case ``c`` on ``inp`` with its layout (strided A, row-sliced W, Y as a column block between canaries); returns the [M, N] output."""
    M, N, K = c.dims()
    dt = ops.act_dtype
    x, w, bias = inp["x"], inp["w"], inp["bias"]
    t128 = c.tile128 if tile128 is None else tile128
    saved = ops.reserved_cus, ops.split_k, ops.split_k_gemm
    ops.reserved_cus, ops.split_k, ops.split_k_gemm = (c.reserved if reserved is None else reserved), c.split, c.split
    try:
        if c.x3:
            big = torch.full((M, 3 * K), 3.0, dtype=dt, device="cuda")
            big[:, K:2 * K] = x
            x = big[:, K:2 * K]
        if c.wslice:
            w = torch.cat([torch.full_like(w, -2.0), w])[N:]
        if c.kind == "f32out":
            y = ops.gemm_f32out(x, w, bias, alpha=inp["alpha"])
        elif c.kind == "gemm2":
            if t128:
                y = ops.gemm(x, w, bias, tile128=True)
            else:
                y = ops.gemm2(x[:, :c.K1].contiguous(), x[:, c.K1:].contiguous(), w, bias)
                assert y is not None, "a3d_gemm2 answered A3D_EUNSUPPORTED"
        elif c.kind == "geglu":
            y = ops.gemm_geglu(x, R.interleave(w), None if bias is None else R.interleave(bias), tile128=t128)
        elif c.kind == "conv":
            B, H, W, _, _, stride, up = c.shape
            He, We, _, _ = R.conv_extents(H, W, stride, up)
            y, _, _ = ops.conv3x3(x, B, H, W, w, bias, stride=stride, up2x=bool(up), rowbias=inp["rowbias"], rb_div=c.rb_div or 1, residual=inp["residual"],
                                  up_size=(He, We) if up > 1 else None, tile128=t128)
        else:
            out = buf = None
            if c.y_off or c.y_pad:
                buf = torch.full((M, N + c.y_off + c.y_pad), CANARY, dtype=dt, device="cuda")
                out = buf[:, c.y_off:c.y_off + N]
            y = ops.gemm(x, w, bias, residual=inp["residual"], alpha=inp["alpha"], beta=inp["beta"], rowbias=inp["rowbias"], rb_div=c.rb_div or 1, out=out,
                         tile128=t128, ring=c.ring)
            if buf is not None:
                _sync()
                assert (buf[:, :c.y_off] == CANARY).all() and (buf[:, c.y_off + N:] == CANARY).all(), f"{c.name}: canary columns around Y were written"
        _sync()
        return y
    finally:
        ops.reserved_cus, ops.split_k, ops.split_k_gemm = saved


def check_exact(c, got, want, what=""):
    bad = R.mismatches(got, want)
    n = int(bad.sum())
    if n:
        m, col = divmod(int(bad.flatten().nonzero()[0]), got.shape[1])
        ncol = col * 2 if c.kind == "geglu" else col           # GEGLU: the owning tile is named in the interleaved N space
        raise AssertionError(f"{c.name}{what}: {n} of {bad.numel()} elements differ from round-to-nearest-even of the float64 result; first at (row {m}, "
                             f"column {col}): got {float(got[m, col])!r}, expected {float(want[m, col])!r}; owner: {R.owner(c, m, ncol)}")


def assert_cell(ops, c, cus):
    info = R.case_plan(c, cus=cus)
    assert info["cell"] == c.cell, f"{c.name}: on {cus} CUs plan() gives {info['cell']}, the case claims {c.cell}"
    return info


@pytest.mark.parametrize("case", [c for c in R.CASES if c.kind == "f32out"], ids=lambda c: c.name)
def test_accumulation_premise(ops, cus, case):
    """a3d_gemm_f32out on exact inputs: the fp32 output IS the float64 result (alpha a power of two, fp32 bias on the grid) — MFMA
    accumulation of integers below 2^24 quanta is exact.  Any mismatch elsewhere is then placement or the store, not accumulation."""
    assert_cell(ops, case, cus)
    inp = R.case_inputs(case, ops.act_dtype, "exact", device="cuda")
    got = run(ops, case, inp)
    assert got.dtype == torch.float32
    check_exact(case, got, inp["exact64"].float(), " (fp32 output)")
    print(f"[parity] {case.name} {IDS[ops.act_dtype]}: fp32 output == float64 result in all {got.numel()} elements (max |y| = {float(got.abs().max()):.0f} = "
          f"{float(got.abs().max()) / inp['q']:.0f} quanta)")


@pytest.mark.parametrize("case", [c for c in R.CASES if c.kind != "f32out"], ids=lambda c: c.name)
def test_gemm_family_per_element(ops, cus, case):
    dt = ops.act_dtype
    info = assert_cell(ops, case, cus)
    cell = case.cell
    alt = cell.kernel in ("ring", "persist") and cell.S == 1          # bit equality with the 128 x 128 kernel and another CU reservation
    other_reserved = 16 if case.reserved == 0 else 0
    # 1. exact inputs
    if case.exact:
        inp = R.case_inputs(case, dt, "exact", device="cuda")
        want = R.expected(inp["exact64"], dt)
        got = run(ops, case, inp)
        check_exact(case, got, want)
        if alt:
            check_exact(case, run(ops, case, inp, tile128=True), want, " (128 x 128 kernel)")
            check_exact(case, run(ops, case, inp, reserved=other_reserved), want, f" (reserved_cus = {other_reserved})")
        del inp, want
    if cell.S > 1:          # the workspace query the launch was planned from: S = ws_needed / (tiles nb 65536)
        needs = [v for k, v in ops._ws_plan.items() if k[0] == ("conv" if case.conv else "gemm") and v > 0 and
                 (k[1:8] == case.shape if case.conv else k[1:4] == case.shape)]
        assert needs and all(v == info["ws_needed"] for v in needs), f"{case.name}: workspace query says {needs}, plan() {info['ws_needed']}"
        assert info["ws_needed"] == info["tiles"] * cell.nb * 65536 * cell.S
    # 2. structured random inputs under the per-element bound
    inp = R.case_inputs(case, dt, "random", device="cuda")
    ref, bound = R.case_bound(case, inp, dt)
    got = run(ops, case, inp)
    ratio, at = R.worst_ratio(got, ref, bound)
    m, col = divmod(at, got.shape[1])
    print(f"[parity] {case.name} {IDS[dt]} [{cell.kernel} nb{cell.nb} S{cell.S}]: worst |err| / bound = {ratio:.3f} at ({m}, {col})")
    assert ratio <= 1.0, (f"{case.name}: |err| = {ratio:.3f} x elem_bound at (row {m}, column {col}): got {float(got[m, col])!r}, float64 {float(ref[m, col])!r}; "
                          f"owner: {R.owner(case, m, col * 2 if case.kind == 'geglu' else col)}")
    # 3. bit equality between the kernels
    if alt:
        assert torch.equal(got, run(ops, case, inp, tile128=True)), f"{case.name}: {cell.kernel} kernel and 128 x 128 kernel differ"
        assert torch.equal(got, run(ops, case, inp, reserved=other_reserved)), f"{case.name}: reserved_cus = {other_reserved} changes the result"
    assert torch.equal(got, run(ops, case, inp)), f"{case.name}: two launches differ"
