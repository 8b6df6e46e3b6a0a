"""Float64 references for the up-sampling conv's 2x2 phase form (a3d_conv3x3_up2x_folded; animate3d_amd.hip_ops.fold_up2x_weights).
TEST INFRASTRUCTURE: plain torch on the device of its inputs, written from the definition in include/animate3d_hip.h and independent of
the product's fold (its own tap table, its own rounding); the product never imports this file.
"""
from __future__ import annotations

import torch

# taps ky of one axis that land on window position r of phase a: the up-sampled pixel 2i + a + ky - 1 is source pixel (2i + a + ky - 1) >> 1
# = i - 1 + a + r.  Derived here, not copied: r = (a + ky + 1) // 2 - a.
TAPS = tuple(tuple(tuple(ky for ky in range(3) if (a + ky + 1) // 2 - a == r) for r in range(2)) for a in range(2))


def tap_sums64(w):
    """float64 [4, Cout, 4 Cin] from w [Cout, 9 Cin] (ky, kx, ci): phase p = 2a + b, row = (r, c), ci."""
    Cout, K9 = w.shape
    Cin = K9 // 9
    w4 = w.double().reshape(Cout, 3, 3, Cin)
    out = torch.zeros(4, Cout, 2, 2, Cin, dtype=torch.float64, device=w.device)
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for c in range(2):
                    out[2 * a + b, :, r, c] = sum(w4[:, ky, kx] for ky in TAPS[a][r] for kx in TAPS[b][c])
    return out.reshape(4, Cout, 4 * Cin)


def round_nearest_even(x64, dtype):
    """float64 -> storage with one round-to-nearest-even, decided in float64 between the two neighbouring storage values (no float32 step).
    For normal-range values whose neighbours are finite."""
    near = x64.float().to(dtype)                                  # some storage value within an ulp
    i16 = near.view(torch.int16).to(torch.int32)
    best, best_err = near.clone(), (near.double() - x64).abs()
    for d in (-1, 1):
        # the neighbour one storage step further from / nearer to zero (sign-magnitude encoding: +-1 on the magnitude bits)
        mag = (i16 & 0x7FFF) + d
        ok = mag >= 0
        cand_bits = ((i16 & 0x8000) | mag.clamp(min=0)).to(torch.int16)
        cand = cand_bits.view(dtype)
        err = (cand.double() - x64).abs()
        even = (cand_bits.to(torch.int32) & 1) == 0
        better = ok & torch.isfinite(cand.double()) & ((err < best_err) | ((err == best_err) & even & ((best.view(torch.int16).to(torch.int32) & 1) == 1)))
        best = torch.where(better, cand, best)
        best_err = torch.where(better, err, best_err)
    return best


def up_conv64(x, B, H, W, w, bias=None):
    """Nearest-2x up-sample then 3x3 conv (pad 1) in float64, straight from the definition: y [B 2H 2W, Cout]."""
    Cin = x.shape[1]
    img = x.double().reshape(B, H, W, Cin)
    up = img[:, torch.arange(2 * H, device=x.device) // 2][:, :, torch.arange(2 * W, device=x.device) // 2]
    pad = torch.zeros(B, 2 * H + 2, 2 * W + 2, Cin, dtype=torch.float64, device=x.device)
    pad[:, 1:-1, 1:-1] = up
    w4 = w.double().reshape(w.shape[0], 3, 3, Cin)
    y = torch.zeros(B, 2 * H, 2 * W, w.shape[0], dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            y += pad[:, ky:ky + 2 * H, kx:kx + 2 * W] @ w4[:, ky, kx].t()
    if bias is not None:
        y = y + bias.double()
    return y.reshape(B * 4 * H * W, -1)


def phase_conv64(x, B, H, W, wf, bias=None, *, absolute=False):
    """The phase form in float64 over folded weights wf [4, Cout, 4 Cin] (any dtype): output pixel (2i + a, 2j + b) = bias + the 2x2
    window of SOURCE pixels from (i - 1 + a, j - 1 + b), zero outside the image.  ``absolute``: sum |x||wf| + |bias| instead (the scale
    of tests/gemm_ref.py's elem_bound).  y [B 2H 2W, Cout]."""
    Cin = x.shape[1]
    Cout = wf.shape[1]
    img = x.double().reshape(B, H, W, Cin)
    wf5 = wf.double().reshape(4, Cout, 2, 2, Cin)
    bb = None if bias is None else bias.double()
    if absolute:
        img, wf5, bb = img.abs(), wf5.abs(), None if bb is None else bb.abs()
    pad = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64, device=x.device)
    pad[:, 1:-1, 1:-1] = img
    y = torch.zeros(B, H, 2, W, 2, Cout, dtype=torch.float64, device=x.device)
    for a in range(2):
        for b in range(2):
            acc = torch.zeros(B, H, W, Cout, dtype=torch.float64, device=x.device)
            for r in range(2):
                for c in range(2):
                    # source pixel (i - 1 + a + r, j - 1 + b + c) = padded (i + a + r, j + b + c)
                    acc += pad[:, a + r:a + r + H, b + c:b + c + W] @ wf5[2 * a + b, :, r, c].t()
            y[:, :, a, :, b] = acc
    if bb is not None:
        y = y + bb
    return y.reshape(B * 4 * H * W, Cout)
