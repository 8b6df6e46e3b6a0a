"""CPU tests of the up-sampling conv's phase form (include/animate3d_hip.h: a3d_conv3x3_up2x_folded): the pack-time weight fold, the index
logic of the four 2x2 phase convolutions, and the dispatcher's choice between the phase form and the nine-tap kernel.  The kernel itself
is held to the family's standard in tests/test_conv_up_folded_gpu.py; what the FOLD's one rounding costs is judged here."""
import pytest
import torch

from animate3d_amd import hip_ops as HO
from tests import up_fold_ref as U

DTYPES = (torch.bfloat16, torch.float16)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
def test_fold_is_the_float64_tap_sum_rounded_once(dtype):
    """wf == round-to-nearest-even(float64 tap sums), bit for bit, against a fold and a rounding written independently in
    tests/up_fold_ref.py (the rounding is decided in float64 between neighbouring storage values, never through float32)."""
    g = torch.Generator().manual_seed(3)
    Cout, Cin = 24, 40
    w = (torch.randn(Cout, 9 * Cin, generator=g) * 2.0 ** torch.randint(-6, 3, (Cout, 1), generator=g)).to(dtype)
    sums = U.tap_sums64(w)
    assert torch.equal(HO.fold_up2x_sums(w), sums)
    got = HO.fold_up2x_weights(w)
    want = U.round_nearest_even(sums, dtype)
    assert got.dtype == dtype and got.shape == (4, Cout, 4 * Cin) and got.is_contiguous()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())
    # the one rounding: at most half an ulp, i.e. 2^-p relative (p = 8 / 11 significant bits)
    rel = ((got.double() - sums).abs() / sums.abs().clamp(min=1e-300)).max().item()
    assert rel <= 2.0 ** -(8 if dtype == torch.bfloat16 else 11)


def test_round_once_beats_two_roundings():
    """A value a hair above a bf16 tie that float32 rounds ONTO the tie: two nearest roundings go down to even, one goes up."""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 + 2.0 ** -40), 1.0 + 3 * 2.0 ** -8 - 2.0 ** -40], dtype=torch.float64)
    twice = x.float().to(torch.bfloat16).double()
    once = HO.round_once(x, torch.bfloat16).double()
    assert torch.equal(once, torch.tensor([1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 1.0 + 2.0 ** -7], dtype=torch.float64))
    assert not torch.equal(once, twice)
    assert torch.equal(U.round_nearest_even(x, torch.bfloat16).double(), once)
    # exactly representable values and exact ties are left to nearest-even
    y = torch.tensor([0.0, 1.5, -3.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(HO.round_once(y, torch.bfloat16).double(), torch.tensor([0.0, 1.5, -3.0, 1.0, 1.0 + 2.0 ** -6], dtype=torch.float64))


@pytest.mark.parametrize("B,H,W", [(2, 4, 4), (2, 3, 5), (1, 8, 8)])
def test_phase_form_is_the_upsampled_conv(B, H, W):
    """Pure index logic: the float64 phase conv over the UNROUNDED folded weights equals the float64 up-sample + 3x3 conv to 1e-12,
    borders included (every tap group that lands outside the source image holds only taps that were outside the up-sampled one)."""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    Cin, Cout = 2, 3
    x = torch.randn(B * H * W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 9 * Cin, generator=g, dtype=torch.float64)
    bias = torch.randn(Cout, generator=g, dtype=torch.float64)
    want = U.up_conv64(x, B, H, W, w, bias)
    got = U.phase_conv64(x, B, H, W, HO.fold_up2x_sums(w), bias)
    assert got.shape == want.shape == (B * 4 * H * W, Cout)
    assert (got - want).abs().max().item() <= 1e-12
    # and the layout is not a symmetric accident: a phase's weights in another phase's place are far off
    wrong = HO.fold_up2x_sums(w)[[1, 0, 3, 2]]
    assert (U.phase_conv64(x, B, H, W, wrong, bias) - want).abs().max().item() > 1e-3


def test_dispatcher_falls_back():
    f = object()      # any non-None stands for the folded weights
    ok = dict(up2x=True, folded=f)
    assert HO.up2x_folded_applies(4, 8, 8, 64, 320, **ok)
    assert HO.up2x_folded_applies(128, 32, 32, 640, 640, **ok, up_size=(64, 64))
    assert HO.up2x_folded_applies(4, 16, 16, 512, 512, **ok) and HO.up2x_folded_applies(8, 4, 8, 128, 1280, **ok)
    # no folded weights, no up-sampling
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, up2x=True, folded=None)
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, up2x=False, folded=f)
    # the cropped sizes keep the nine-tap kernel
    for size in ((15, 16), (16, 15), (15, 15)):
        assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, **ok, up_size=size)
    # shapes the persistent kernel does not take
    assert not HO.up2x_folded_applies(3, 8, 8, 64, 320, **ok)            # B H W % 256
    assert not HO.up2x_folded_applies(4, 8, 8, 96, 320, **ok)            # Cin % 64
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 384, **ok)            # Cout: neither 320 nor 256 columns per tile
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 128, **ok)
    assert not HO.up2x_folded_applies(1 << 14, 32, 32, 128, 320, **ok)   # a 4 GB input
    # operands the entry point does not take, the forced 128 x 128 kernel, and runs that are compared bit for bit across row counts
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, **ok, rowbias=f)
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, **ok, residual=f)
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, **ok, tile128=True)
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, **ok, shape_independent=True)
    assert not HO.up2x_folded_applies(4, 8, 8, 64, 320, **ok, stride=2)


def test_header_declares_both_storage_types():
    fns = HO.read_header(HO._HEADER_PATH).functions
    assert fns["a3d_conv3x3_up2x_folded_bf16"] == fns["a3d_conv3x3_up2x_folded_f16"]
    assert len(fns["a3d_conv3x3_up2x_folded_bf16"][1]) == 13
