"""The summation order of the 4-D stage's scalar losses, pinned (csrc/loss_reduce.h): the forward entry points of csrc/recon_loss.hip and
csrc/stage_reg.hip, called through ``f32_stage.launch`` with the test's own ``partials`` buffer, against a NumPy emulation of that order:

* a thread's run in fp32, item after item in the order its kernel visits them (``_runs``);
* the halving tree over the block's 256 threads in fp32: one partial per block;
* thread t of the final block adds partials t, t + 256, ... in fp64;
* the same tree in fp64.

Every input is chosen so that what a thread adds is exactly representable in fp32 (sums of the inputs themselves, or squares of at most
24 bits): the emulation is then exact whether or not the compiler contracts ``acc += d * d`` into an fma, and each case checks this itself
(``_exact_squares``).  Each case also shows that it tells orders apart: the same values added one after another in fp32, in memory order,
give other bits than the emulated order in every block (for the one-Gaussian case, whose single thread adds three numbers, the
comparison is with the reverse order).  The seeds below were drawn until that held; it is asserted, not assumed."""
import numpy as np
import pytest
import torch

from animate3d_amd import f32_stage
from animate3d_amd.hip_ops import _p

pytestmark = pytest.mark.gpu

BLOCK = 256                      # LR_BLOCK
f32, f64 = np.float32, np.float64


# ---- the emulation

def _runs(vals, per_block, group):
    """vals [images, items, C] -> [images * blocks per image, 256, run * C]: what each thread adds, in its order.  Block j of an image
    covers items [j per_block, (j + 1) per_block); a thread visits ``group`` neighbours at a time, group i of thread t starting at item
    ``group * (i * 256 + t)`` of the block, and an item's C values one after another.  Items past the end add nothing (here: 0)."""
    images, items, C = vals.shape
    run, chunks = per_block // BLOCK, -(-items // per_block)
    s = np.arange(run)
    idx = (np.arange(chunks)[:, None, None] * per_block + group * ((s // group)[None, None, :] * BLOCK + np.arange(BLOCK)[None, :, None])
           + (s % group)[None, None, :])
    padded = np.zeros((images, chunks * per_block, C), f32)
    padded[:, :items] = vals
    return padded[:, idx].reshape(images * chunks, BLOCK, run * C)


def _tree(red):
    """The halving tree over axis 1 (256 wide), in red's own precision."""
    red = red.copy()
    h = BLOCK // 2
    while h > 0:
        red[:, :h] = red[:, :h] + red[:, h:2 * h]
        h >>= 1
    return red[:, 0]


def _partials(runs):
    """One fp32 partial per block of ``runs`` [blocks, 256, steps]."""
    assert runs.dtype == f32
    acc = np.zeros(runs.shape[:2], f32)
    for step in range(runs.shape[2]):
        acc = acc + runs[:, :, step]
    assert acc.dtype == f32
    return _tree(acc)


def _final(partials):
    """The final block's fp64 sum of fp32 ``partials`` [n]."""
    n = partials.shape[0]
    padded = np.zeros(-(-n // BLOCK) * BLOCK, f64)
    padded[:n] = partials.astype(f64)
    acc = np.zeros(BLOCK, f64)
    for row in padded.reshape(-1, BLOCK):
        acc = acc + row
    return _tree(acc[None])[0]


def _sequential(vals, per_block):
    """The fp32 sum of each block's values one after another in memory order: [images * blocks per image]."""
    images, items, C = vals.shape
    chunks = -(-items // per_block)
    padded = np.zeros((images, chunks * per_block, C), f32)
    padded[:, :items] = vals
    return np.cumsum(padded.reshape(images * chunks, per_block * C), axis=1, dtype=f32)[:, -1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _assert_discriminates(emulated, other_order):
    assert emulated.shape == other_order.shape and bool((_bits(emulated) != _bits(other_order)).all()), \
        "this draw does not tell the documented order from another one: choose another seed"


def _exact_squares(d):
    """d * d for fp32 ``d``, after checking that the fp32 product is the exact one."""
    sq = d * d
    assert d.dtype == f32 and sq.dtype == f32 and np.array_equal(sq.astype(f64), d.astype(f64) * d.astype(f64))
    return sq


def _check(name, got, want):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    print(f"[loss_reduce {name}] kernel {_bits(got)[:4]} emulation {_bits(want)[:4]} ({got.size} values)")
    assert np.array_equal(_bits(got), _bits(want)), name


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the Gaussian scale sum: additions only

GR_PAIRS = 1024                  # GR_ITEMS of csrc/stage_reg.hip: four (image, Gaussian) pairs per thread


@pytest.mark.parametrize("shared", [False, True], ids=["scales_bs=3N", "scales_bs=0"])
@pytest.mark.parametrize("B,N,seed", [(2, 1500, 11), (1, 1, 13)], ids=["three_blocks_last_partial", "one_gaussian"])
def test_gaussian_scale_sum_is_added_in_the_documented_order(B, N, seed, shared):
    rng = np.random.default_rng(seed)
    scales = rng.uniform(0.01, 2.0, size=(1 if shared else B, N, 3)).astype(f32)
    vals = np.broadcast_to(scales, (B, N, 3)).reshape(1, B * N, 3)              # the pairs are numbered across the images
    runs = _runs(vals, GR_PAIRS, 1)
    want_partials = _partials(runs)
    want = _final(want_partials)
    n_partials = -(-B * N // GR_PAIRS)
    assert want_partials.shape == (n_partials,) and n_partials == (3 if N > 1 else 1)
    if N > 1:
        _assert_discriminates(want_partials, _sequential(vals, GR_PAIRS))
    else:                                                                       # one thread, three numbers: against c + b + a
        _assert_discriminates(want_partials, _sequential(vals[:, :, ::-1], GR_PAIRS))
    sc = _cuda(scales)
    partials = torch.full((3, n_partials), float("nan"), device="cuda")
    out = torch.full((4,), float("nan"), device="cuda")
    f32_stage.launch("a3d_gaussian_reg_f32", sc.device, B, N, None, _p(sc), 0 if shared else 3 * N, None, None, 0.0, 1.0, 0.0, _p(partials),
                     n_partials, _p(out))
    partials, out = partials.cpu().numpy(), out.cpu().numpy()
    _check("gaussian partials[1]", partials[1], want_partials)
    _check("gaussian out[2]", out[2], f32(want))                               # scale 1.0: the fp64 epilogue is exact
    assert not partials[0].any() and not partials[2].any() and out[1] == 0.0 and out[3] == 0.0


# ---- the mask term of the reconstruction loss

RL_PIXELS = 2048                 # RL_PIXELS of csrc/recon_loss.hip: eight pixels per thread


@pytest.mark.parametrize("H,W,group,seed", [(33, 65, 1, 21), (36, 64, 4, 22)], ids=["scalar_path", "16_byte_path"])
def test_recon_mask_term_is_added_in_the_documented_order(H, W, group, seed):
    B, P = 2, H * W
    assert (P % 4 == 0) == (group == 4) and -(-P // RL_PIXELS) == 2
    rng = np.random.default_rng(seed)
    alpha = (rng.integers(0, 2049, size=(B, P)).astype(f32) * f32(2.0 ** -11))
    mask = rng.integers(0, 2, size=(B, P)).astype(np.uint8)
    vals = _exact_squares(alpha - mask.astype(f32))[:, :, None]
    want_partials = _partials(_runs(vals, RL_PIXELS, group))
    want = f32(_final(want_partials) / f64(B * P))                              # the epilogue: one fp64 division
    _assert_discriminates(want_partials, _sequential(vals, RL_PIXELS))
    image = _cuda(rng.uniform(-0.2, 1.2, size=(B, 3, P)).astype(f32))
    gt = _cuda(rng.uniform(0.0, 1.0, size=(B, P, 3)).astype(f32))
    alp, msk = _cuda(alpha), _cuda(mask)
    assert all(t.data_ptr() % 16 == 0 for t in (image, gt, alp, msk))
    n_partials = 2 * B
    partials = torch.full((2, n_partials), float("nan"), device="cuda")
    out = torch.full((3,), float("nan"), device="cuda")
    f32_stage.launch("a3d_recon_loss_f32", image.device, B, H, W, _p(image), _p(alp), _p(gt), _p(msk), None, 0.5, 1.0, 1.0, _p(partials),
                     n_partials, _p(out))
    partials, out = partials.cpu().numpy(), out.cpu().numpy()
    _check("recon partials[1]", partials[1], want_partials)
    _check("recon out[2]", out[2], want)
    assert np.isfinite(partials[0]).all() and np.isfinite(out).all()


# ---- the depth's total variation

IR_PIXELS = 8192                 # IR_PIXELS of csrc/stage_reg.hip: 32 pixels per thread


@pytest.mark.parametrize("H,W,group,seed", [(65, 129, 1, 32), (66, 128, 4, 35)], ids=["G=1", "G=4"])
def test_depth_tv_is_added_in_the_documented_order(H, W, group, seed):
    B, P = 2, H * W
    assert (W % 4 == 0) == (group == 4) and -(-P // IR_PIXELS) == 2
    rng = np.random.default_rng(seed)
    depth = (rng.integers(-2047, 2048, size=(B, H, W)).astype(f32) * f32(2.0 ** -12))
    # a pixel adds its difference to the pixel below to one sum and the one to its right neighbour to another, in pixel order both
    down, right = np.zeros((B, H, W), f32), np.zeros((B, H, W), f32)
    down[:, :-1] = _exact_squares(depth[:, 1:] - depth[:, :-1])
    right[:, :, :-1] = _exact_squares(depth[:, :, 1:] - depth[:, :, :-1])
    want_partials = []
    for vals in (down.reshape(B, P, 1), right.reshape(B, P, 1)):
        want_partials.append(_partials(_runs(vals, IR_PIXELS, group)))
        _assert_discriminates(want_partials[-1], _sequential(vals, IR_PIXELS))
    dep = _cuda(depth)
    assert dep.data_ptr() % 16 == 0
    n_partials = 2 * B
    partials = torch.full((5, n_partials), float("nan"), device="cuda")
    out = torch.full((4,), float("nan"), device="cuda")
    f32_stage.launch("a3d_image_reg_f32", dep.device, B, H, W, None, _p(dep), None, 0.0, 1.0, 0.0, _p(partials), n_partials, _p(out))
    partials, out = partials.cpu().numpy(), out.cpu().numpy()
    _check("depth_tv partials[2]", partials[2], want_partials[0])
    _check("depth_tv partials[3]", partials[3], want_partials[1])
    assert not partials[0].any() and not partials[1].any() and not partials[4].any()
    # out[2]: the epilogue's t += scale * sum may or may not be contracted: one fp32 ulp of the fp64 formula
    tv = 2.0 / B
    formula = tv / ((H - 1.0) * W) * _final(want_partials[0]) + tv / (H * (W - 1.0)) * _final(want_partials[1])
    print(f"[loss_reduce depth_tv out[2]] kernel {out[2]!r} formula {formula!r}")
    assert abs(f64(out[2]) - formula) <= f64(np.spacing(f32(formula)))
