"""GPU tests of the up-sampling conv's 2x2 phase form (a3d_conv3x3_up2x_folded_{bf16,f16}: gemm_pp.hip CONV 3) at the smallest shapes
the persistent kernel takes.

1. exact inputs: x and w are small integers on a dyadic grid, so every tap sum (|sum| <= 60 quanta <= 256: exact in 8 significant bits)
   and every fp32 accumulation is exact.  The phase form must then equal the nine-tap kernel (``conv3x3(up2x=True)`` on the unfolded
   weights) BIT FOR BIT, and both must equal the float64 result rounded once; border rows 0 / 2H-1 and columns 0 / 2W-1 are asserted
   on their own.  Cases: one and two 64-channel slices, 320- and 256-column tiles, a non-square 4 x 8 map whose 256-row tile straddles
   eight images, and a grid smaller than the tile list (a workgroup walks tiles of different phases);
2. random inputs: against float64 over the ROUNDED folded weights with tests/gemm_ref.py's per-element bound, K = 4 Cin — the kernel
   is held to the family's standard; the fold's own rounding is judged in tests/test_conv_up_folded_host.py;
3. the A3D_EINVAL rules of include/animate3d_hip.h through the entry point;
4. HIP-graph capture of a UNet forward that takes the new path.
"""
import pytest
import torch

from animate3d_amd import hip_ops as HO
from tests import gemm_ref as R
from tests import up_fold_ref as U

pytestmark = pytest.mark.gpu

IDS = {R.BF: "bf16", R.FP: "fp16"}
# (B, H, W, Cin, Cout, reserved CUs)
CASES = {
    "1slice-320": (4, 8, 8, 64, 320, 0),
    "2slices-640": (4, 8, 8, 128, 640, 0),
    "1slice-640": (4, 8, 8, 64, 640, 0),
    "2slices-320": (4, 8, 8, 128, 320, 0),
    "4x8-straddles-images": (8, 4, 8, 64, 320, 0),
    "256-column-tiles": (4, 8, 8, 64, 256, 0),
    "two-tiles-per-workgroup": (32, 8, 8, 64, 640, 224),      # 64 tiles on 32 CUs: tile t and t + 32 are of different phases
}


@pytest.fixture(scope="module", params=R.DTYPES, ids=IDS.values())
def ops(request):
    return HO.HipOps(act_dtype=request.param)


def _sync():
    """A GPU fault ends the session: nothing more is launched on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # pragma: no cover
        pytest.exit(f"GPU fault, session ended: {e}", returncode=3)


def _both(ops, x, B, H, W, w, wf, bias, reserved=0):
    saved = ops.reserved_cus
    ops.reserved_cus = reserved
    try:
        assert HO.up2x_folded_applies(B, H, W, x.shape[1], w.shape[0], up2x=True, folded=wf)
        new, Ho, Wo = ops.conv3x3(x, B, H, W, w, bias, up2x=True, folded=wf)
        assert (Ho, Wo) == (2 * H, 2 * W)
        old, _, _ = ops.conv3x3(x, B, H, W, w, bias, up2x=True)
        _sync()
    finally:
        ops.reserved_cus = saved
    return new, old


def _exact(shape, dtype):
    B, H, W, Cin, Cout, _ = shape
    g = torch.Generator().manual_seed(B + 7 * H + 13 * Cin + Cout)
    xi = torch.randint(-3, 16, (B * H * W, Cin), generator=g).double() * (torch.randint(0, 2, (B * H * W, 1), generator=g) * 2 - 1)
    wi = torch.randint(-3, 16, (Cout, 9 * Cin), generator=g).double() * (torch.randint(0, 2, (Cout, 1), generator=g) * 2 - 1)
    bi = (torch.arange(Cout, dtype=torch.float64) * 37) % 2047 - 1023
    ex, ew = -2, -4                                   # quantum 2^-6: |y| <= 9 * 128 * 225 / 64 + 16 < 2^13, inside fp16's range
    x, w, bias = (xi * 2.0 ** ex).to(dtype), (wi * 2.0 ** ew).to(dtype), (bi * 2.0 ** (ex + ew)).float()
    assert torch.equal(x.double(), xi * 2.0 ** ex) and torch.equal(w.double(), wi * 2.0 ** ew)
    sums = U.tap_sums64(wi)
    assert sums.abs().max() <= 256, "a tap sum leaves the 8 significant bits of bf16"
    wf = HO.fold_up2x_weights(w)
    assert torch.equal(wf.double(), sums * 2.0 ** ew), "the folded weights of the exact inputs are not exact"
    assert 9 * Cin * 15 * 15 + 1023 < 2 ** 23                       # every partial sum of either kernel is an fp32 integer of quanta
    return x, w, wf, bias


@pytest.mark.parametrize("name", list(CASES))
def test_exact_inputs_equal_the_nine_tap_kernel_bit_for_bit(ops, name):
    shape = CASES[name]
    B, H, W, Cin, Cout, reserved = shape
    dt = ops.act_dtype
    x, w, wf, bias = _exact(shape, dt)
    xc, wc, wfc, bc = x.cuda(), w.cuda(), wf.cuda(), bias.cuda()
    new, old = _both(ops, xc, B, H, W, wc, wfc, bc, reserved)
    exact64 = U.up_conv64(x, B, H, W, w, bias)
    want = R.expected(exact64, dt)
    new4, old4, want4 = (t.cpu().view(B, 2 * H, 2 * W, Cout) for t in (new, old, want))
    bits = lambda t: t.contiguous().view(torch.int16)
    # the borders on their own: the phase form's zero reads must be the nine-tap kernel's zero padding
    for what, sl in (("row 0", (slice(None), 0)), (f"row {2 * H - 1}", (slice(None), 2 * H - 1)),
                     ("column 0", (slice(None), slice(None), 0)), (f"column {2 * W - 1}", (slice(None), slice(None), 2 * W - 1))):
        bad = R.mismatches(new4[sl], want4[sl])
        assert not bad.any(), f"{name} {IDS[dt]}: {int(bad.sum())} wrong elements in output {what}"
        assert torch.equal(bits(new4[sl]), bits(old4[sl])), f"{name} {IDS[dt]}: output {what} differs from the nine-tap kernel"
    bad = R.mismatches(new4, want4)
    if bad.any():
        b, yy, xx, co = (int(v) for v in bad.nonzero()[0])
        pytest.fail(f"{name} {IDS[dt]}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 result; first at image {b} pixel "
                    f"({yy}, {xx}) = phase {2 * (yy & 1) + (xx & 1)} channel {co}: got {float(new4[b, yy, xx, co])} want {float(want4[b, yy, xx, co])}")
    assert torch.equal(bits(new4), bits(old4)), f"{name} {IDS[dt]}: the phase form differs from conv3x3(up2x=True)"


@pytest.mark.parametrize("name", ["2slices-640", "4x8-straddles-images", "256-column-tiles", "two-tiles-per-workgroup"])
def test_random_inputs_within_the_family_bound(ops, name):
    B, H, W, Cin, Cout, reserved = CASES[name]
    dt = ops.act_dtype
    inp = R.random_inputs("conv", (B, H, W, Cin, Cout, 1, 1), dt, seed=11)
    x, w, bias = inp["x"], inp["w"], inp["bias"]
    wf = HO.fold_up2x_weights(w)
    new, _ = _both(ops, x.cuda(), B, H, W, w.cuda(), wf.cuda(), bias.cuda(), reserved)
    ref = U.phase_conv64(x, B, H, W, wf, bias)                       # over the ROUNDED folded weights
    scale = U.phase_conv64(x, B, H, W, wf, bias, absolute=True)
    bound = R.elem_bound(ref, scale, 4 * Cin, dt)
    ratio, i = R.worst_ratio(new.cpu(), ref, bound)
    print(f"[parity] up2x-folded {name} {IDS[dt]}: worst |err| / bound = {ratio:.3f} at row {i // Cout} column {i % Cout}; rel L2 = {R.rel_l2(new.cpu(), ref):.2e}")
    assert ratio <= 1.0


def test_einval_rules(ops):
    """Every rule of the header through the entry point itself; the valid call next to them returns 0."""
    dt = ops.act_dtype
    B, H, W, Cin, Cout = 4, 8, 8, 64, 320
    x = torch.zeros(B * H * W + 64, Cin, dtype=dt, device="cuda")
    wf = torch.zeros(4, Cout + 64, 4 * 128, dtype=dt, device="cuda")
    bias = torch.zeros(Cout + 64, dtype=torch.float32, device="cuda")
    y = torch.zeros(4 * (B * H * W + 64) * (Cout + 64) + 8, dtype=dt, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = ops.lib.a3d_conv3x3_up2x_folded_bf16

    def rc(**kw):
        a = dict(X=x.data_ptr(), Wf=wf.data_ptr(), bias=bias.data_ptr(), rowbias=None, R=None, Y=y.data_ptr(), B=B, H=H, W=W, Cin=Cin, Cout=Cout, flags=0)
        a.update(kw)
        return fn(stream, a["X"], a["Wf"], a["bias"], a["rowbias"], a["R"], a["Y"], a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["flags"])

    assert rc() == 0 and rc(bias=None) == 0 and rc(flags=16) == 0
    bad = [dict(B=3), dict(B=5), dict(H=7), dict(Cin=96), dict(Cin=32), dict(Cout=384), dict(Cout=128), dict(Cout=64),
           dict(rowbias=x.data_ptr()), dict(R=y.data_ptr()), dict(X=None), dict(Wf=None), dict(Y=None), dict(B=0), dict(H=0), dict(W=-1),
           dict(X=x.data_ptr() + 8), dict(Wf=wf.data_ptr() + 2), dict(Y=y.data_ptr() + 8), dict(bias=bias.data_ptr() + 4),
           dict(flags=HO.A3D_GEMM_TILE128), dict(flags=HO.A3D_GEMM_RING), dict(flags=0x300), dict(flags=0x400)]
    for kw in bad:
        assert rc(**kw) == HO.A3D_EINVAL, kw
    _sync()


def test_unet_forward_on_the_new_path_is_graph_capturable():
    """A two-level UNet (320 / 640 channels) at 2 views x 4 frames x 16 x 16: its one up-sampler (8 x 8 -> 16 x 16, B H W = 512, 640
    channels) qualifies for the phase form.  The eager forward takes it (counted at the C-ABI call), a captured graph replays it on new
    inputs bit for bit, and the output stays within the end-to-end rounding noise of the nine-tap forward."""
    from animate3d_amd.config import UNetConfig
    from animate3d_amd.unet import MVUNetMotionModel
    from bench import make_inputs
    cfg = UNetConfig(block_out_channels=(320, 640), down_has_attn=(True, False), layers_per_block=1)
    m = MVUNetMotionModel(cfg, num_views=2, device="cuda")
    m.init_synthetic(seed=1)
    m = m.to(torch.bfloat16).eval()
    ops = m.ops
    calls = []
    real = ops.lib.a3d_conv3x3_up2x_folded_bf16

    def counting(*a):
        calls.append(a)
        return real(*a)
    counting.__name__ = "a3d_conv3x3_up2x_folded_bf16"
    ops.lib.a3d_conv3x3_up2x_folded_bf16 = counting
    try:
        inp_a = make_inputs(cfg, 2, 2, 4, (16, 16), torch.device("cuda"), seed=1)
        inp_b = make_inputs(cfg, 2, 2, 4, (16, 16), torch.device("cuda"), seed=2)
        y_new = m(**inp_a).sample
        assert len(calls) == 1, "the up-sampler did not take the phase form"
        assert m._packed.up[0].up_folded is not None or m._packed.up[1].up_folded is not None
        step = m.capture_graph(**inp_a)
        for src in (inp_a, inp_b):
            y_static = step(**src).sample
            _sync()
            assert torch.equal(y_static, m(**src).sample), "graph replay differs from the eager forward"
        # the same forward on the nine-tap kernel (split_k off is the op set's switch for shape-independent kernels)
        ops.split_k = False
        n = len(calls)
        y_old = m(**inp_a).sample
        assert len(calls) == n
        rel = ((y_new.float() - y_old.float()).norm() / y_old.float().norm()).item()
        print(f"[parity] two-level UNet, phase form vs nine-tap up-sampler: rel L2 = {rel:.3e}")
        # two honest bf16 executions of one graph: each is held to 3e-2 against the fp32 oracle (tests/test_unet_gpu.py), and they
        # differ from one another by no more than that bar
        assert torch.isfinite(y_new).all() and rel <= 3e-2
    finally:
        ops.split_k = True
        ops.lib.a3d_conv3x3_up2x_folded_bf16 = real
