"""Float64 oracles, exact-input builders, per-element bounds, a Python mirror of the dispatch and wrong-kernel models for the GEMM /
implicit-GEMM convolution family (csrc/gemm_conv.hip, gemm_pp.hip, gemm_ring.hip, gemm_common.h).  TEST INFRASTRUCTURE: plain torch,
runs on the device of its inputs; the product never imports this file.

Why a zero-tolerance comparison is possible.  (1) The operands are 16-bit, so a product of two of them is exact in fp32, and the
accumulators are fp32.  (2) `exact_inputs` takes every operand from one dyadic grid: integers of magnitude <= 15 (rowbias and residual
<= 128, bias <= 1023) times a power of two.  (3) It asserts, on the float64 side, that sum |x||w| + |bias| + |rowbias|, scaled by
max(alpha, 1), plus beta |r| stays below 2^23 quanta: with alpha, beta in {0.5, 1, 2} every partial result of every kernel is a multiple
of half a quantum below 2^24 half-quanta, i.e. an fp32 number, so (4) every add, the alpha product and the beta fma are exact in any
order, on any MFMA shape, through any split-K slicing, and (5) the only rounding left is the store: the output must equal
round_to_nearest_even(float64 result) element for element.  tests/test_gemm_ref_host.py re-proves (3)-(4) in fp32 arithmetic in three
summation orders and shows that thirteen wrong kernels (`MUTANTS`) are rejected; tests/test_gemm_edges_gpu.py runs the kernels.

The fused GEGLU epilogue is pinned the same way: for |g| >= 8 the `erfx` of gelu_erf (gemm_common.h) rounds to exactly 1.0f, so
gelu(g) = fma(|g / 2|, 1, g / 2) = g for g > 0 and +0 for g < 0 without rounding; the gate columns carry a bias of +/- 2^10 quanta,
alternating per column, and amplitudes small enough that (h + b_h)(g + b_g) < 2^24 quanta: the output is exactly that product, or 0.

`elem_bound` is the per-element bound for random, realistic inputs (derivation in its docstring).
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass
from functools import lru_cache

import torch

BF, FP = torch.bfloat16, torch.float16
DTYPES = (BF, FP)
PREC = {BF: 8, FP: 11}                          # significant bits of the storage types
OLD_BAR = {BF: 4e-3, FP: 1e-3}                  # whole-tensor relative L2 of tests/test_hip_kernels_gpu.py

# flags word (include/animate3d_hip.h)
RESERVED_MASK, KERNEL_MASK, TILE128, RING = 0xFF, 0x300, 0x100, 0x200

Cell = namedtuple("Cell", "kernel nb S RES CONV EPI TWO vec16")
RING_DEPTH = {2: 4, 4: 3, 5: 2}                 # gemm_ring.hip: RingCfg<NB>::RING


def f32(v: float) -> float:
    """The value a float argument has once it has crossed the C-ABI (alpha and beta are C floats)."""
    return float(torch.tensor(v, dtype=torch.float32))


# ===================================================================================================================== oracles
def _epilogue(core, bias, rowbias, rb_div, residual, alpha, beta):
    y = core
    if bias is not None:
        y = y + bias.double()
    if rowbias is not None:
        y = y + rowbias.double()[torch.arange(y.shape[0], device=y.device) // rb_div]
    y = f32(alpha) * y
    if residual is not None:
        y = y + f32(beta) * residual.double()
    return y


def gemm(x, w, bias=None, rowbias=None, rb_div=1, residual=None, alpha=1.0, beta=1.0):
    """alpha (x w^T + bias + rowbias[m // rb_div]) + beta r in float64 from the 16-bit operands."""
    return _epilogue(x.double() @ w.double().t(), bias, rowbias, rb_div, residual, alpha, beta)


def gemm2(xa, xb, w, bias=None):
    return gemm(torch.cat([xa, xb], dim=1), w, bias)


def deinterleave(t):
    """Inverse of HipOps.interleave_geglu: 32-row blocks [h | gate] -> [all h rows | all gate rows]."""
    n = t.shape[0] // 2
    blk = t.reshape(n // 32, 2, 32, *t.shape[1:])
    return torch.cat([blk[:, 0].reshape(n, *t.shape[1:]), blk[:, 1].reshape(n, *t.shape[1:])], 0)


def interleave(t):
    n = t.shape[0] // 2
    h, g = t[:n].reshape(n // 32, 32, *t.shape[1:]), t[n:].reshape(n // 32, 32, *t.shape[1:])
    return torch.stack([h, g], dim=1).reshape(t.shape).contiguous()


def geglu(x, w, bias=None):
    """(x Wh^T + bh) * gelu_erf(x Wg^T + bg) in float64; ``w`` / ``bias`` are the UN-interleaved [h rows | gate rows]."""
    hg = x.double() @ w.double().t()
    if bias is not None:
        hg = hg + bias.double()
    h, g = hg.chunk(2, dim=1)
    return h * (0.5 * g * (1.0 + torch.erf(g * math.sqrt(0.5))))


def conv_extents(H, W, stride, up_code):
    He = 2 * H - ((up_code >> 1) & 1) if up_code else H
    We = 2 * W - ((up_code >> 2) & 1) if up_code else W
    return He, We, (He - 1) // stride + 1, (We - 1) // stride + 1


def im2col(x, B, H, W, stride=1, up_code=0, *, leak=False, ignore_crop=False, off_centre=False):
    """The virtual A matrix [B Ho Wo, (ky, kx, ci)] of the 3x3 convolution (pad 1) in float64: the nearest-2x upsample is an index gather,
    cropped by its last row (up_code bit 1) / column (bit 2); then a zero pad and nine shifted slices.  No vendor convolution library.
    The keyword switches are the wrong models 7-9 of MUTANTS."""
    Cin = x.shape[1]
    img = x.double().reshape(B, H, W, Cin)
    He, We, Ho, Wo = conv_extents(H, W, stride, up_code)
    if up_code:
        Hs, Ws = (2 * H, 2 * W) if ignore_crop else (He, We)
        img = img[:, torch.arange(Hs, device=x.device) // 2][:, :, torch.arange(Ws, device=x.device) // 2]
    Hi, Wi = img.shape[1], img.shape[2]
    pad = torch.zeros(B, max(Hi, He) + 2, max(Wi, We) + 2, Cin, dtype=torch.float64, device=x.device)
    pad[:, 1:Hi + 1, 1:Wi + 1] = img
    if leak:                                   # the row above an image is the last row of the image before it (linear addressing, no mask)
        pad[1:, 0, 1:Wi + 1] = img[:-1, Hi - 1]
    o = 1 if off_centre else 0                 # taps centred one pixel off
    cols = []
    for ky in range(3):
        for kx in range(3):
            ys = torch.arange(Ho, device=x.device) * stride + ky + o
            xs = torch.arange(Wo, device=x.device) * stride + kx + o
            ys, xs = ys.clamp(max=pad.shape[1] - 1), xs.clamp(max=pad.shape[2] - 1)
            cols.append(pad[:, ys][:, :, xs])
    return torch.cat(cols, dim=3).reshape(B * Ho * Wo, 9 * Cin)


def conv3x3(x, B, H, W, w, bias=None, stride=1, up_code=0, rowbias=None, rb_div=1, residual=None):
    """x [B H W, Cin], w packed [Cout, (ky, kx, ci)] as in HipOps.conv3x3 -> (float64 y [B Ho Wo, Cout], Ho, Wo); up_code 0, 1, 3, 5, 7."""
    assert up_code in (0, 1, 3, 5, 7) and (stride == 1 or not up_code)
    _, _, Ho, Wo = conv_extents(H, W, stride, up_code)
    y = _epilogue(im2col(x, B, H, W, stride, up_code) @ w.double().t(), bias, rowbias, rb_div, residual, 1.0, 1.0)
    return y, Ho, Wo


def kwalk(K, conv):
    """The order in which the kernels visit the K columns: dense = index order; conv = nine taps of one 64-channel slice, then the next slice."""
    k = torch.arange(K)
    if not conv:
        return k
    Cin = K // 9
    kt, r = k // 64, k % 64
    return (kt % 9) * Cin + (kt // 9) * 64 + r


# ===================================================================================================================== storage rounding
def expected(exact64, dtype):
    """float64 -> float (exact on the exact inputs, asserted) -> storage, round to nearest even."""
    y32 = exact64.float()
    assert torch.equal(y32.double(), exact64), "the float64 result is not an fp32 number: the inputs are not exact inputs"
    return y32.to(dtype)


def truncate(y64, dtype):
    """Round toward zero to storage (normal range): the store of a kernel that drops the low mantissa bits."""
    bits = y64.float().contiguous().view(torch.int32)
    drop = 16 if dtype == BF else 13
    return (bits & ~((1 << drop) - 1)).view(torch.float32).to(dtype)


def mismatches(got, want):
    """Numeric inequality (-0 == +0; a NaN never equals): boolean mask, no element exempt."""
    return ~(got.float() == want.float())


def rounding_census(y64, dtype):
    """(share of elements the store has to round, ties rounded down, ties rounded up)."""
    y = y64.float()
    lo = truncate(y64, dtype).float()
    rn = y.to(dtype).float()
    inexact = rn != y
    ulp = torch.where(rn != lo, (rn - lo).abs(), torch.zeros_like(y))           # where rn == lo the upper neighbour is lo + ulp(lo)
    e = torch.frexp(lo.abs().clamp(min=1e-30))[1] - 1
    ulp_lo = torch.ldexp(torch.ones_like(y), e - (7 if dtype == BF else 10))
    ulp = torch.where(rn != lo, ulp, ulp_lo)
    tie = inexact & (((y - lo).abs() * 2) == ulp)
    return inexact.float().mean().item(), int((tie & (rn == lo)).sum()), int((tie & (rn != lo)).sum())


# ===================================================================================================================== cases
@dataclass(frozen=True)
class Case:
    name: str
    kind: str                 # gemm | gemm2 | geglu | conv | f32out
    shape: tuple              # dense: (M, N, K) (geglu: N = N2, the interleaved width); conv: (B, H, W, Cin, Cout, stride, up_code)
    cell: Cell                # the dispatch cell the case claims on a 256-CU device
    seam: str                 # what it probes
    bias: bool = True
    rb_div: int = 0           # 0: no rowbias
    residual: bool = False
    alpha: float = 1.0
    beta: float = 1.0
    K1: int = 0               # gemm2: columns of the first source
    tile128: bool = False     # A3D_GEMM_TILE128
    ring: bool = False        # A3D_GEMM_RING
    reserved: int = 0         # reserved compute units of the flags word
    split: bool = False       # through the workspace entry point (HipOps.split_k / split_k_gemm on)
    x3: bool = False          # A is the middle third of an [M, 3 K] buffer
    y_off: int = 0            # Y starts y_off elements into rows of N + y_off + y_pad elements; the rest are canaries
    y_pad: int = 0
    wslice: bool = False      # W is the second half of the rows of a fused weight
    exact: bool = True        # has an exact-input form (GEGLU without a bias cannot pin its gates)

    @property
    def conv(self):
        return self.kind == "conv"

    def dims(self):
        if self.conv:
            B, H, W, Cin, Cout, stride, up = self.shape
            _, _, Ho, Wo = conv_extents(H, W, stride, up)
            return B * Ho * Wo, Cout, 9 * Cin
        return self.shape

    @property
    def flags(self):
        return self.reserved | (TILE128 if self.tile128 else (RING if self.ring else 0))

    def rb_rows(self):
        M = self.dims()[0]
        return (M + self.rb_div - 1) // self.rb_div if self.rb_div else 0


# ===================================================================================================================== the dispatch, mirrored
def _plan_persist(conv, epi, M, N, K, flags, allow_split, cus_dev, *, vec16, ldx, ldw, rb_div, out_f32, ws_bytes, conv_geom=None):
    """plan_persist<CONV, EPI> of gemm_conv.hip.  ws_bytes: None = no workspace attached.  Returns (nb, S, grid cus, tiles_m, tiles_n) or None."""
    if (flags & KERNEL_MASK) == TILE128 or out_f32:
        return None
    reserved = flags & RESERVED_MASK
    cus = cus_dev - reserved if cus_dev - reserved > 32 else 32
    if not vec16 or K % 64 or M % 256 or (rb_div and rb_div % 256):
        return None
    if ldw % 64 or (conv == 0 and ldx % 64):
        return None
    if (conv == 0 and ldx * 16 >= 1 << 31) or ldw * 16 >= 1 << 31:
        return None
    if conv:
        B, H, W, Cin = conv_geom
        if (B * H * W + 2 * W + 2) * Cin * 2 >= 1 << 32:
            return None
    tm, nk, unit, OVH = (M + 255) // 256, K // 64, (9 if conv else 1), 12
    best = best1 = -1
    bnb = bnb1 = 0
    bS = 1
    for nb in (5, 4):
        if (epi == "geglu" and nb == 5) or N % (nb * 64):
            continue
        tiles = tm * (N // (nb * 64))
        for S in range(1, (16 if allow_split and epi == "linear" else 1) + 1):
            if (nk // unit) % S or (S > 1 and nk // S < 9):
                continue
            items = tiles * S
            rounds = (items + cus_dev - 1) // cus_dev
            if items * 100 < rounds * cus_dev * 50:
                continue
            if S > 1 and ws_bytes is not None and items * nb * 65536 > ws_bytes:
                continue
            cost = rounds * (nk // S + OVH) * nb * (108 if nb == 4 else 100) + (100 * nb if S > 1 else 0)
            if S == 1 and (best1 < 0 or cost < best1):
                best1, bnb1 = cost, nb
            if best < 0 or cost < best:
                best, bnb, bS = cost, nb, S
    if best < 0:
        return None
    if bS > 1 and best1 >= 0 and best * 100 > best1 * 85:
        bnb, bS = bnb1, 1
    return bnb, bS, cus, tm, N // (bnb * 64)


def _plan_ring(M, N, K, flags, cus_dev, *, vec16, ldx, ldw, rb_div, out_f32, two):
    """plan_ring of gemm_conv.hip: (nb, grid cus, cost) or None."""
    if (flags & KERNEL_MASK) == TILE128 or out_f32 or not vec16 or two:
        return None
    if M % 128 or K % 64 or K < 256 or ldx % 64 or ldw % 64:
        return None
    if ldx * 64 >= 1 << 32 or ldw * 256 >= 1 << 32 or (rb_div and rb_div % 128):
        return None
    reserved = flags & RESERVED_MASK
    cus = cus_dev - reserved if cus_dev - reserved > 32 else 32
    bnb, bcost = 0, 0
    for nb in (5, 4, 2):
        if N % (64 * nb):
            continue
        tiles = (M // 128) * (N // (64 * nb))
        cost = ((tiles + cus - 1) // cus) * (128 + 64 * nb)
        if bnb == 0 or cost < bcost:
            bnb, bcost = nb, cost
    return (bnb, cus, bcost) if bnb else None


def plan_info(kind, M, N, K, *, ldx=None, ldw=None, ldy=None, ldr=None, y_off=0, bias=True, rb_div=0, residual=False, conv_geom=None,
              flags=0, cus=256, ws=None):
    """Mirror of launch<> / plan_persist<> / plan_ring / splitk_ws_bytes<> (gemm_conv.hip) for one call.

    kind: gemm | gemm2 | geglu | conv (conv_geom = (B, H, W, Cin, up)) | f32out; rb_div 0 = no rowbias; y_off = elements between a 16-byte
    aligned address and Y; ws: None = the entry point without a workspace, "query" = what HipOps does (ask a3d_*_ws for the bytes, attach
    exactly those when > 0), an int = a workspace of that many bytes.  Returns a dict with the Cell (None where a3d_gemm2 answers
    A3D_EUNSUPPORTED) and the launch geometry: grid, items, rounds of the grid, nk, ws_needed."""
    assert flags & ~(RESERVED_MASK | KERNEL_MASK) == 0 and (flags & KERNEL_MASK) <= RING
    ldx = K if ldx is None else ldx
    ldw = K if ldw is None else ldw
    ldy = (N // 2 if kind == "geglu" else N) if ldy is None else ldy
    ldr = N if ldr is None else ldr
    out_f32 = kind == "f32out"
    conv = 0 if kind != "conv" else (2 if conv_geom[4] else 1)
    epi = "geglu" if kind == "geglu" else "linear"
    if conv:
        vec16 = N % 8 == 0
        ldx, ldw = conv_geom[3], K
    else:
        vec16 = (ldy * (4 if out_f32 else 2)) % 16 == 0 and (y_off * 2) % 16 == 0 and (not residual or ldr % 8 == 0) and (not rb_div or N % 8 == 0)
    common = dict(vec16=vec16, ldx=ldx, ldw=ldw, rb_div=rb_div, out_f32=out_f32)
    pp = lambda allow, wsb: _plan_persist(conv, epi, M, N, K, flags, allow, cus, ws_bytes=wsb, conv_geom=conv_geom[:4] if conv else None, **common)
    ws_needed = 0
    if ws is not None and epi == "linear" and kind in ("gemm", "conv"):
        q = pp(True, None)                                     # splitk_ws_bytes<>
        if q and q[1] > 1:
            ws_needed = q[3] * q[4] * q[1] * q[0] * 65536
    ws_bytes = None if ws is None else (ws_needed if ws == "query" else int(ws))
    if ws_bytes is not None and ws_bytes <= 0:
        ws_bytes = None
    two = kind == "gemm2"
    info = dict(ws_needed=ws_needed, nk=K // 64, vec16=vec16)

    def cell(kernel, nb, S=1):
        return Cell(kernel, nb, S, bool(residual) and epi == "linear", conv, epi, two, bool(vec16))

    if two:
        pl = pp(False, None) if ldx % 64 == 0 else None
        if pl is None:
            return dict(info, cell=None)
    else:
        pl = None
        if conv == 0 and epi == "linear":
            rp = _plan_ring(M, N, K, flags, cus, two=False, **common)
            if rp:
                ring = True
                if (flags & KERNEL_MASK) != RING:
                    pl = pp(ws_bytes is not None, ws_bytes)
                    if pl:
                        items = pl[3] * pl[4] * pl[1]
                        ring = pl[1] == 1 and rp[2] * 100 < ((items + cus - 1) // cus) * (256 + 64 * pl[0]) * 75
                if ring:
                    tiles = (M // 128) * (N // (64 * rp[0]))
                    grid = min(tiles, rp[1])
                    return dict(info, cell=cell("ring", rp[0]), items=tiles, grid=grid, rounds=-(-tiles // grid), depth=RING_DEPTH[rp[0]])
        pl = pp(ws_bytes is not None, ws_bytes)
    if pl:
        nb, S, gcus, tm, tn = pl
        items = tm * tn * S
        grid = min(items, gcus)
        return dict(info, cell=cell("persist", nb, S), items=items, tiles=tm * tn, grid=grid, rounds=-(-items // grid))
    nblk = -(-M // 128) * -(-N // 128)
    small = (conv == 0 and K <= 640) or nblk < 768
    return dict(info, cell=cell("tile128-bk32" if small else "tile128-bk64", 2), items=nblk, grid=nblk, rounds=1)


def plan(kind, M, N, K, **kw):
    """The cell (kernel, nb, S, RES, CONV, EPI, TWO, vec16) a call reaches; see plan_info.  Supersedes _persistent_eligible of
    tests/test_hip_kernels_gpu.py (kept there), which knows the persistent kernel's rule only."""
    return plan_info(kind, M, N, K, **kw)["cell"]


def case_plan(c: Case, cus=256):
    M, N, K = c.dims()
    kw = dict(bias=c.bias, rb_div=c.rb_div, residual=c.residual, flags=c.flags, cus=cus)
    if c.conv:
        B, H, W, Cin, _, _, up = c.shape
        kw["conv_geom"] = (B, H, W, Cin, up)
        if c.split and M <= 32768 and not c.tile128:            # HipOps.conv3x3's gate
            kw["ws"] = "query"
    else:
        kw.update(ldx=3 * K if c.x3 else (c.K1 if c.kind == "gemm2" else K), ldy=(N // 2 if c.kind == "geglu" else N) + c.y_off + c.y_pad, y_off=c.y_off)
        if c.kind == "gemm2" and (K - c.K1) % 64:
            return dict(cell=None)
        if c.split and c.kind == "gemm" and not c.tile128 and M <= 32768 and K >= 1152:      # HipOps.gemm's gate
            kw["ws"] = "query"
    return plan_info(c.kind, M, N, K, **kw)


# ===================================================================================================================== inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


@lru_cache(maxsize=2)
def _exact_operands(kind, shape, seed):
    """Integer operands (float64, CPU) of the exact inputs: x, w (geglu: un-interleaved) — shared by the epilogue variants of one shape."""
    g = _gen(seed)
    if kind == "conv":
        B, H, W, Cin, Cout, _, _ = shape
        xs, ws = (B * H * W, Cin), (Cout, 9 * Cin)
    else:
        M, N, K = shape
        xs, ws = (M, K), (N, K)
    if kind == "geglu":
        a = int(math.isqrt(576 // shape[2]))       # K a^2 <= 576: |h|, |g| <= 576 quanta, well inside the +/- 1024 gate bias
        assert a >= 1, "GEGLU exact inputs need K <= 576"
        x = torch.randint(-a, a + 1, xs, generator=g).double()
        w = torch.randint(-a, a + 1, ws, generator=g).double()
        return x, w
    # magnitudes <= 15 with a positive mean, so that sums grow with K and need rounding in both storage types even at K = 64; a sign per
    # output column (and per input row) gives outputs of both signs
    x = torch.randint(-3, 16, xs, generator=g).double() * (torch.randint(0, 2, (xs[0], 1), generator=g) * 2 - 1)
    w = torch.randint(-3, 16, ws, generator=g).double() * (torch.randint(0, 2, (ws[0], 1), generator=g) * 2 - 1)
    return x, w


def exact_inputs(kind, shape, dtype, seed=0, *, bias=True, rb_div=0, residual=False, alpha=1.0, beta=1.0, device="cpu"):
    """Dyadic-grid inputs on which every kernel of the family must reproduce the float64 result exactly (module docstring).

    Returns a dict: x, w (geglu: un-interleaved; interleave() gives the kernel's layout), bias (fp32), rowbias, residual (storage type),
    alpha, beta, q (the quantum) and exact64, the float64 result.  Rowbias rows all differ, the bias differs per column (also from the
    column 64 further on).  Asserted here: the sums bound, the fp16 output range, >= 10 % of the outputs inexact in ``dtype`` and at least
    one tie of each parity."""
    assert alpha in (0.5, 1.0, 2.0) and beta in (0.5, 1.0, 2.0)
    c = Case("", kind, tuple(shape), None, "", bias=bias, rb_div=rb_div, residual=residual, alpha=alpha, beta=beta)
    M, N, K = c.dims()
    xi, wi = (t.to(device) for t in _exact_operands(kind, tuple(shape), seed))      # integers from the CPU generator; the matmuls run on ``device``
    g = _gen(seed + 1)
    cols = torch.arange(N, dtype=torch.float64, device=device)
    if kind == "geglu":
        n = N // 2
        bi = None
        if bias:
            bh = (cols[:n] * 37) % 129 - 64
            bg = torch.where(cols[:n] % 2 == 0, 1024.0, -1024.0).double()      # gate on / off per column
            bi = torch.cat([bh, bg])
        A = xi
        core = A @ wi.t()
        absb = (A.abs() @ wi.abs().t()) + (bi.abs() if bias else 0)
        hh, gg = (core + (bi if bias else 0)).chunk(2, dim=1)
        assert bias, "the GEGLU pin needs the gate bias"
        assert gg.abs().min() >= 8 * 32, "a gate inside the range where erfx != 1"
        y_int = hh * torch.where(gg > 0, gg, torch.zeros_like(gg))
        assert absb[:, :n].max() * absb[:, n:].max() < 2 ** 24, "GEGLU product leaves the exact fp32 range"
        ex, ew, q = 0, -5, 2.0 ** -10
        ri = rbi = None
    else:
        A = im2col(xi, *shape[:3], shape[5], shape[6]) if kind == "conv" else xi
        core = A @ wi.t()
        bi = ((cols * 37) % 2047 - 1023) if bias else None
        rows = c.rb_rows()
        rbi = ((torch.arange(rows, dtype=torch.float64, device=device)[:, None] * 53 + cols[None, :] * 29) % 257 - 128) if rb_div else None
        ri = torch.randint(-128, 129, (M, N), generator=g).double().to(device) if residual else None
        y_int = _epilogue(core, bi, rbi, rb_div or 1, ri, alpha, beta)
        absb = A.abs() @ wi.abs().t()
        if bias:
            absb = absb + bi.abs()
        if rb_div:
            absb = absb + rbi.abs()[torch.arange(M, device=device) // rb_div]
        absb = max(alpha, 1.0) * absb + (beta * ri.abs() if residual else 0)
        assert absb.max() < 2 ** 23, f"sums bound: {absb.max():.0f} quanta >= 2^23"
        # one quantum for both storage types: the largest output lands in [2^13, 2^14), inside fp16's range
        e = 13 - int(math.floor(math.log2(max(float(y_int.abs().max()), 1.0))))
        ex, ew, q = e // 2, e - e // 2, 2.0 ** e
    exact64 = y_int * q
    nz = exact64[exact64 != 0].abs()
    assert exact64.abs().max() < 60000 and (nz.numel() == 0 or nz.min() >= 2.0 ** -14), "fp16 output range"
    if kind != "f32out":
        share, down, up = rounding_census(exact64, dtype)
        assert share >= 0.10, f"only {share:.1%} of the outputs need rounding in {dtype}"
        assert down > 0 and up > 0, f"ties rounded down / up: {down} / {up}"
    st = lambda t, e: None if t is None else (t * 2.0 ** e).to(dtype)
    out = dict(x=st(xi, ex), w=st(wi, ew), bias=None if bi is None else (bi * 2.0 ** (ex + ew)).float(), rowbias=st(rbi, ex + ew),
               residual=st(ri, ex + ew), alpha=alpha, beta=beta, q=q, exact64=exact64)
    for k, t, e in (("x", xi, ex), ("w", wi, ew), ("rowbias", rbi, ex + ew), ("residual", ri, ex + ew)):
        assert t is None or torch.equal(out[k].double(), t * 2.0 ** e), f"{k} is not representable in {dtype}"
    return out


@lru_cache(maxsize=2)
def _random_operands(kind, shape, seed):
    g = _gen(seed)
    if kind == "conv":
        B, H, W, Cin, Cout, _, _ = shape
        xs, ws = (B * H * W, Cin), (Cout, 9 * Cin)
    else:
        M, N, K = shape
        xs, ws = (M, K), (N, K)
    ramp = lambda n: 2.0 ** (2.0 * torch.arange(n, dtype=torch.float32) / max(n - 1, 1) - 1.0)        # two octaves
    x = torch.randn(xs, generator=g) * ramp(xs[0])[:, None]
    w = torch.randn(ws, generator=g) * ramp(ws[0])[:, None] * ws[1] ** -0.5
    return x, w


def random_inputs(kind, shape, dtype, seed=0, *, bias=True, rb_div=0, residual=False, alpha=1.0, beta=1.0, device="cpu"):
    """Structured random inputs of realistic scale: normal values under per-row (x) and per-column (w) scale ramps over two octaves, so a
    value from the wrong row or column is far outside elem_bound.  Same dict as exact_inputs, without exact64 / q."""
    c = Case("", kind, tuple(shape), None, "", rb_div=rb_div)
    M, N, K = c.dims()
    x, w = _random_operands(kind, tuple(shape), seed)
    g = _gen(seed + 1)
    st = lambda t: t.to(dtype).to(device)
    return dict(x=st(x), w=st(w), bias=torch.randn(N, generator=g).to(device) if bias else None,
                rowbias=st(torch.randn(c.rb_rows(), N, generator=g)) if rb_div else None,
                residual=st(torch.randn(M, N, generator=g)) if residual else None, alpha=alpha, beta=beta)


def case_inputs(c: Case, dtype, mode, device="cpu", seed=0):
    fn = exact_inputs if mode == "exact" else random_inputs
    alpha, beta = (c.alpha, c.beta) if mode == "exact" else ({0.5: 0.37, 2.0: 1.7}.get(c.alpha, c.alpha), {0.5: 0.9, 2.0: 1.3}.get(c.beta, c.beta))
    return fn(c.kind, c.shape, dtype, seed, bias=c.bias, rb_div=c.rb_div, residual=c.residual, alpha=alpha, beta=beta, device=device)


# ===================================================================================================================== oracle of a case, and its wrong models
def case_A(c: Case, inp, **kw):
    if c.conv:
        B, H, W, _, _, stride, up = c.shape
        return im2col(inp["x"], B, H, W, stride, up, **kw)
    return inp["x"].double()


def oracle(c: Case, inp, *, with_abs=False, mutant=None):
    """float64 result of the case on ``inp`` (and, with_abs, the same expression over absolute values: the scale of the fp32 accumulation
    bound).  ``mutant``: one of the K-side / operand-side wrong models (MUTANTS 3-13); None where it does not apply to the case."""
    M, N, K = c.dims()
    W = inp["w"].double()
    bias, rowbias, res, rb_div = inp["bias"], inp["rowbias"], inp["residual"], c.rb_div or 1
    alpha, beta = inp["alpha"], inp["beta"]
    if c.kind == "geglu":
        if mutant == "geglu_swap":
            n = N // 2
            W = W.clone()
            W[:32], W[n:n + 32] = inp["w"].double()[n:n + 32], inp["w"].double()[:32]
            if bias is not None:
                bias = bias.clone()
                bias[:32], bias[n:n + 32] = inp["bias"][n:n + 32], inp["bias"][:32]
        elif mutant is not None:
            return None
        y = geglu(inp["x"], W, bias)
        if not with_abs:
            return y
        xa = inp["x"].double().abs() @ W.abs().t() + (bias.double().abs() if bias is not None else 0)
        hg = inp["x"].double() @ W.t() + (bias.double() if bias is not None else 0)
        return y, (xa, hg)
    A = None
    if mutant == "conv_leak":
        A = case_A(c, inp, leak=True) if c.conv and c.shape[0] > 1 else None
    elif mutant == "crop_ignored":
        A = case_A(c, inp, ignore_crop=True) if c.conv and c.shape[6] in (3, 5, 7) else None
    elif mutant == "stride_off":
        A = case_A(c, inp, off_centre=True) if c.conv and c.shape[5] == 2 else None
    if mutant in ("conv_leak", "crop_ignored", "stride_off") and A is None:
        return None
    if A is None:
        A = case_A(c, inp)
    core = A @ W.t()
    cell = c.cell
    tm = 256 if cell.kernel == "persist" else 128
    tn = 64 * cell.nb
    kw_ = kwalk(K, c.conv).to(A.device)
    r, cs = slice(0, min(tm, M)), slice(0, min(tn, N))
    part = lambda rows, ks: A[rows][:, ks] @ W[cs][:, ks].t()
    if mutant == "rowbias_row":
        if rowbias is None or rowbias.shape[0] < 2:
            return None
        idx = ((torch.arange(M, device=A.device) + 1) // rb_div).clamp(max=rowbias.shape[0] - 1)
        return f32(alpha) * (core + (bias.double() if bias is not None else 0) + rowbias.double()[idx]) + (f32(beta) * res.double() if res is not None else 0)
    if mutant == "bias_parity":
        if bias is None or N < 128:
            return None
        y = _epilogue(core, bias, rowbias, rb_div, res, alpha, beta)
        y[r, 0:64] += f32(alpha) * (inp["bias"][64:128].double() - inp["bias"][0:64].double())
        return y
    if mutant == "drop_last_ktile":
        if not A[r][:, kw_[K - 64:]].any():            # (a conv whose last tap is padding for every row of the tile: nothing to drop)
            return None
        core = core.clone()
        core[r, cs] -= part(r, kw_[K - 64:])
    elif mutant == "ktile_from_next_tile":
        if M < 2 * tm:
            return None
        core = core.clone()
        nxt = slice(tm, 2 * tm)
        core[r, cs] += part(nxt, kw_[:64]) - part(r, kw_[:64])
    elif mutant == "split_slice_missing":
        if cell.S <= 1:
            return None
        per = K // cell.S
        core = core.clone()
        core[r, cs] -= part(r, kw_[per:2 * per])
    elif mutant == "two_source_seam":
        if c.kind != "gemm2":
            return None
        k1 = c.K1
        core = core.clone()
        lo = max(k1 - 64, 0)
        core[r, cs] += (A[r, lo:lo + 64] - A[r, k1:k1 + 64]) @ W[cs, k1:k1 + 64].t()
    elif mutant == "alpha_after_residual":
        if res is None or f32(alpha) == 1.0:
            return None
        return f32(alpha) * (core + (bias.double() if bias is not None else 0) + (rowbias.double()[torch.arange(M, device=A.device) // rb_div] if rowbias is not None else 0)
                             + f32(beta) * res.double())
    elif mutant is not None and mutant not in ("conv_leak", "crop_ignored", "stride_off"):
        return None
    y = _epilogue(core, bias, rowbias, rb_div, res, alpha, beta)
    if not with_abs:
        return y
    ab = A.abs() @ W.abs().t()
    if bias is not None:
        ab = ab + bias.double().abs()
    if rowbias is not None:
        ab = ab + rowbias.double().abs()[torch.arange(M, device=A.device) // rb_div]
    ab = abs(f32(alpha)) * ab
    if res is not None:
        ab = ab + abs(f32(beta)) * res.double().abs()
    return y, ab


def store(y64, dtype):
    return y64.float().to(dtype)


def _chunk_from_neighbour(c, y64, dtype):
    out = store(y64, dtype)
    M, N = out.shape
    if N < 16:
        return None
    m = min(M - 1, 37)
    out[m, 0:8] = out[m, 8:16].clone()
    return out


# name -> (what the wrong kernel does, where it is applied).  "store": a wrong store of the right float64 result; "oracle": a wrong model
# of the computation (oracle(..., mutant=name)), stored correctly.  A mutant that does not apply to a case yields None there.
MUTANTS = {
    "truncating_store": ("the store truncates instead of rounding to nearest even", "store"),
    "chunk_from_neighbour": ("one lane's 16-byte store (8 elements) holds its neighbour's values", "store"),
    "rowbias_row": ("rowbias row (m + 1) // rb_div", "oracle"),
    "bias_parity": ("one tile reads the bias of the adjacent 64-column block (bias-image parity)", "oracle"),
    "drop_last_ktile": ("one tile drops its last K-tile", "oracle"),
    "ktile_from_next_tile": ("one tile takes its first K-tile from the next tile (stream across the tile boundary)", "oracle"),
    "conv_leak": ("a border tap reads the neighbouring image's pixel instead of zero", "oracle"),
    "crop_ignored": ("the upsample crop is ignored", "oracle"),
    "stride_off": ("stride-2 taps centred one pixel off", "oracle"),
    "split_slice_missing": ("one split-K slice missing from one tile", "oracle"),
    "geglu_swap": ("h and gate swapped in one 32-row block of the GEGLU interleave", "oracle"),
    "two_source_seam": ("the two-source seam tile read from X instead of X2", "oracle"),
    "alpha_after_residual": ("alpha applied after the residual", "oracle"),
}


def mutant_output(name, c: Case, inp, dtype, y64=None):
    """The storage-type output of wrong kernel ``name`` on the case, or None where it does not apply."""
    if MUTANTS[name][1] == "store":
        y64 = oracle(c, inp) if y64 is None else y64
        return truncate(y64, dtype) if name == "truncating_store" else _chunk_from_neighbour(c, y64, dtype)
    y = oracle(c, inp, mutant=name)
    return None if y is None else store(y, dtype)


# ===================================================================================================================== per-element bound
# erf by Abramowitz-Stegun 7.1.26 as gelu_erf evaluates it: erfx = 1 - P(t) e, P(t) = sum_{k=1..5} a_k t^k, t = rcp(1 + p x), e = exp2(-x^2 log2 e).
#   approximation: |erf error| <= 1.5e-7 (A&S);
#   rcpf, 1 ulp (2^-23 relative) on t: |dP| <= sum k |a_k| t^k 2^-23 <= 16.2 * 2^-23 (t <= 1), times e <= 1;
#   exp2f, 1 ulp on e: |P e| = 1 - erf <= 1, so 2^-23;
#   fp32 roundings of the evaluation itself: five fma + one product on partial sums <= sum |a_k| = 4.5 (27 * 2^-24), three roundings in the
#   exponent's argument, relative error of e <= 3 * 2^-24 x^2 and x^2 e <= 1/e (1.2 * 2^-24), the final fma (2^-24).
E_ERF = 1.5e-7 + 2.0 ** -23 * (16.2 + 1.0) + 2.0 ** -24 * (27.0 + 1.2 + 1.0)


def half_ulp(ref, dtype):
    """Half a unit in the last place of the storage type at |ref|: 2^(floor(log2 |ref|) - p), p = 8 significant bits (bf16) / 11 (fp16; from
    2^-14 down the spacing stays 2^-24).  Never more than 2^-p |ref|, up to twice less."""
    e = torch.frexp(ref.abs().clamp(min=1e-300))[1] - 1
    if dtype == FP:
        e = e.clamp(min=-14)
    return torch.ldexp(torch.ones_like(ref), e - PREC[dtype])


def elem_bound(ref, scale, K, dtype, geglu_terms=None):
    """Per-element bound of |kernel - float64 reference| on realistic inputs:

        half_ulp(ref) + (K + 8) 2^-24 (|alpha| sum |x||w| + |alpha bias| + |alpha rowbias| + |beta r|)

    half_ulp: the one rounding of the store, <= u |ref| with u = 2^-8 (bf16, 8 significant bits) / 2^-11 (fp16).  (A relative 2^-9 for
    bf16 is not attainable: the correctly rounded float64 result itself errs by up to 1.97 x 2^-9 |ref|, which the host test shows; the
    binade's own half ulp used here is the tightest statement of "half an ulp".)  The second term is the standard bound of a
    length-K fp32 sum in any order, (K - 1) unit roundoffs of 2^-24 on the sum of absolute values, with 8 more for the bias, rowbias,
    alpha, beta-fma and split-K reduce steps and the error those leave in the value the store then rounds; ``scale`` is that sum of
    absolute values, a second float64 matmul (oracle(..., with_abs=True)).

    GEGLU (geglu_terms = (scale of [h | gate] incl. |bias|, float64 [h | gate])): out = hh * gelu(gg).  With eh, eg the accumulation
    bounds of hh and gg as above, |gelu'| <= 1.13, and gelu evaluated as gg/2 + |gg/2| erfx (gelu_erf: erf error E_ERF above, one more
    rounding each for gg/2's fma and the product), the error before the store is at most
        |gelu(gg)| eh + |hh| (1.13 eg + |gg| / 2 * E_ERF + 2^-24 |gelu(gg)|) + 2^-24 |ref|.
    No constant is fitted to what the kernels produce."""
    hu = half_ulp(ref, dtype)
    acc = (K + 8) * 2.0 ** -24
    if geglu_terms is None:
        return hu + acc * scale
    sc, hg = geglu_terms
    (sh, sg), (hh, gg) = sc.chunk(2, dim=1), hg.chunk(2, dim=1)
    gel = 0.5 * gg * (1.0 + torch.erf(gg * math.sqrt(0.5)))
    return hu + gel.abs() * acc * sh + hh.abs() * (1.13 * acc * sg + 0.5 * gg.abs() * E_ERF + 2.0 ** -24 * gel.abs()) + 2.0 ** -24 * ref.abs()


def case_bound(c: Case, inp, dtype):
    """(float64 reference, per-element bound) of a case on random inputs."""
    K = c.dims()[2]
    if c.kind == "geglu":
        ref, terms = oracle(c, inp, with_abs=True)
        return ref, elem_bound(ref, None, K, dtype, geglu_terms=terms)
    ref, scale = oracle(c, inp, with_abs=True)
    return ref, elem_bound(ref, scale, K, dtype)


def worst_ratio(got, ref, bound):
    """(max |err| / bound, flat index): a non-finite output counts as infinitely wrong."""
    r = (got.double() - ref).abs() / bound.clamp(min=1e-300)
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.flatten()[i]), i


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-300))


def owner(c: Case, m, n):
    """The tile, wave and lane that store element (m, n): what a mismatch report names."""
    cell = c.cell
    if cell.kernel == "persist":
        tm, tn = 256, 64 * cell.nb
        return f"tile ({m // tm}, {n // tn}) of 256 x {tn}, wave row {(m % tm) // 64}, 32-column block {(n % tn) // 32}, row {m % 32} of half {(m % 64) // 32}"
    tn = 64 * cell.nb if cell.kernel == "ring" else 128
    w = 64 if cell.EPI == "linear" else 32
    return (f"tile ({m // 128}, {n // tn}) of 128 x {tn}, wave ({(m % 128) // 64}, {(n % tn) // 64}), half {(m % 64) // 32}, "
            f"lane {8 * (m % 8) + (n % w) // 8} (row group {(m % 32) // 8}, columns {8 * ((n % w) // 8)}..)")


# ===================================================================================================================== the case table
def _c(kernel, nb=2, S=1, RES=False, CONV=0, EPI="linear", TWO=False, vec16=True):
    return Cell(kernel, nb, S, RES, CONV, EPI, TWO, vec16)


T32, T64 = "tile128-bk32", "tile128-bk64"
CASES = []


def _add(name, kind, shape, cell, seam, **kw):
    CASES.append(Case(name, kind, tuple(shape), cell, seam, **kw))


def _epilogue_grid(prefix, kind, shape, kernel, nb, rb_div, seam, **kw):
    """kernel x RES x {bias, none} x {rowbias, none}"""
    for res in (False, True):
        for bias in (True, False):
            for rb in (0, rb_div):
                _add(f"{prefix}-res{int(res)}-bias{int(bias)}-rb{rb}", kind, shape, _c(kernel, nb, RES=res), seam,
                     residual=res, bias=bias, rb_div=rb, alpha=2.0 if res else 0.5, beta=0.5 if res else 1.0, **kw)


# ---- the accumulation premise
_add("f32out-k64", "f32out", (129, 136, 64), _c(T32), "fp32 output: accumulation alone, one K-tile", alpha=0.5)
_add("f32out-k5120", "f32out", (129, 136, 5120), _c(T32), "fp32 output: accumulation alone, 80 K-tiles", alpha=2.0)
# ---- 128 x 128 kernel
_epilogue_grid("t128-129x320x128", "gemm", (129, 320, 128), T32, 2, 111, "every epilogue operand; residual rows clamped at M - 1 (one row in the last tile)")
_add("t128-m1-n132-k64", "gemm", (1, 132, 64), _c(T32, RES=True, vec16=False), "M = 1, N % 8 = 4: 8-byte halves, one K-tile", rb_div=1, residual=True, alpha=2.0,
     beta=0.5)
_add("t128-m127-n4-k128", "gemm", (127, 4, 128), _c(T32, vec16=False), "N = 4: one 8-byte half per row; rb_div = 1", rb_div=1)
_add("t128-m389-n320-k192", "gemm", (389, 320, 192), _c(T32, RES=True), "three K-tiles; rb_div = 111 crossing tiles; ragged M and N", rb_div=111, residual=True,
     alpha=0.5, beta=2.0)
_add("t128-m389-n132-k704", "gemm", (389, 132, 704), _c(T32, vec16=False), "eleven K-tiles (odd count: the loop ends on an even step)", rb_div=389)
_add("t128-m100-rbdiv111", "gemm", (100, 136, 64), _c(T32), "M < rb_div: every row reads rowbias row 0", rb_div=111)
_add("t128-bk64-4000x3072x704", "gemm", (4000, 3072, 704), _c(T64, RES=True), "K-step 64 (>= 768 tiles, K > 640), ragged M", residual=True, alpha=0.5)
_add("t128-strided", "gemm", (389, 320, 128), _c(T32, RES=True), "A = middle third of [M, 3K]; Y a column block with canaries, 16-byte aligned", x3=True, y_off=8,
     y_pad=8, residual=True, beta=2.0)
_add("t128-y-8-byte-offset", "gemm", (129, 320, 64), _c(T32, RES=True, vec16=False), "Y at an 8-byte offset, ldy % 8 != 0: 8-byte halves with rowbias and residual",
     y_off=4, y_pad=0, rb_div=129, residual=True, alpha=2.0)
# ---- ring kernel (reserved_cus = 224 leaves a 32-workgroup grid: small shapes walk several tiles per workgroup)
_epilogue_grid("ring2-384x640x256", "gemm", (384, 640, 256), "ring", 2, 128, "ring of four at nk = 4 = its depth; every epilogue operand; rb_div = 128")
_add("ring2-nk5-tiles40", "gemm", (5120, 128, 320), _c("ring", 2, RES=True), "nk = depth + 1; 40 tiles on 32 workgroups: bias parity and K-tile stream across tiles",
     reserved=224, rb_div=128, residual=True, alpha=0.5)
_add("ring4-nk4", "gemm", (512, 1280, 256), _c("ring", 4), "ring of three at nk = 4 = depth + 1 (K >= 256: nk = depth is not reachable), one tile per workgroup",
     reserved=224, rb_div=128)
_add("ring4-nk5-tiles64", "gemm", (4096, 512, 320), _c("ring", 4, RES=True), "nk = 5; two tiles per workgroup", reserved=224, residual=True, beta=2.0)
_add("ring4-nk6-wslice", "gemm", (512, 1280, 384), _c("ring", 4), "nk = 6 = two turns of the ring; W a row slice of a fused weight", reserved=224, wslice=True, bias=False)
_add("ring5-nk4", "gemm", (1280, 960, 256), _c("ring", 5), "ring of two at nk = 4; 128 x 320 tiles (WaveCols<5> split), one tile per workgroup", reserved=224, rb_div=128)
_add("ring5-nk5-tiles60", "gemm", (2560, 960, 320), _c("ring", 5, RES=True), "nk = 5 (odd); two tiles per workgroup, partial second round", reserved=224, rb_div=1280,
     residual=True, alpha=2.0, beta=0.5)
_add("ring5-nk6-x3", "gemm", (1280, 960, 384), _c("ring", 5), "nk = 6; A strided (ldx = 3K)", reserved=224, x3=True)
_add("ring-full-chip-4096x1280", "gemm", (4096, 1280, 256), _c("ring", 4), "default dispatch on the whole chip: 160 tiles of 128 x 256", rb_div=128)
# ---- persistent kernel
_epilogue_grid("pp4-8192x1280x64", "gemm", (8192, 1280, 64), "persist", 4, 256, "nb 4, one round of 160 tiles, one K-tile; every epilogue operand; rb_div = 256")
_add("pp4-k640-reserved224", "gemm", (8192, 1280, 640), _c("persist", 4, RES=True), "32-workgroup grid: five tiles per workgroup, ten K-tiles", reserved=224,
     residual=True, alpha=0.5, beta=2.0, rb_div=8192)
_add("pp4-partial-second-round", "gemm", (16640, 1280, 64), _c("persist", 4), "325 tiles on 256 workgroups: a partial second round")
_add("pp5-32768x320", "gemm", (32768, 320, 64), _c("persist", 5), "nb 5 (WaveCols<5>), N = 320: one column of tiles; no bias", bias=False)
_add("pp5-res-rbM-ldx3", "gemm", (32768, 320, 128), _c("persist", 5, RES=True), "nb 5 with residual; rb_div = M; ldx = 3K; 128 tiles on a 32-workgroup grid",
     residual=True, rb_div=32768, x3=True, alpha=2.0, reserved=224)
_add("pp4-strided-out", "gemm", (8192, 1280, 64), _c("persist", 4), "Y a column block of a wider buffer, canaries untouched", y_off=8, y_pad=56)
# ---- two-source A
_add("two-k1-64", "gemm2", (8192, 1280, 192), _c("persist", 4, TWO=True), "seam after the first K-tile", K1=64)
_add("two-k1-last", "gemm2", (8192, 1280, 192), _c("persist", 4, TWO=True), "seam before the last K-tile", K1=128, bias=False)
# ---- split-K
_add("splitk-dense", "gemm", (1024, 1280, 4608), _c("persist", 4, S=8, RES=True), "dense split-K: 8 slices of 9 K-tiles, reduce kernel applies every operand", split=True,
     residual=True, rb_div=256, alpha=0.5, beta=2.0)
_add("splitk-conv", "conv", (16, 8, 8, 512, 1280, 1, 0), _c("persist", 4, S=8, CONV=1), "conv split-K: 8 channel slices, S in {2, 4, 8} only", split=True, rb_div=256)
_add("splitk-conv-res", "conv", (16, 8, 8, 640, 1280, 1, 0), _c("persist", 4, S=10, RES=True, CONV=1), "ten channel slices: S in {2, 5, 10} only; residual in the reduce",
     split=True, residual=True)
# ---- conv on the 128 x 128 kernel (B >= 2: a tap leaking into the neighbouring image is visible)
_add("conv-h1", "conv", (2, 1, 7, 64, 64, 1, 0), _c(T32, CONV=1), "H = 1: every tap row but the centre is padding")
_add("conv-w1", "conv", (3, 5, 1, 64, 64, 1, 0), _c(T32, CONV=1, RES=True), "W = 1", residual=True, rb_div=5)
_add("conv-5x7", "conv", (4, 5, 7, 128, 136, 1, 0), _c(T32, CONV=1), "5 x 7, M = 140 (M % 128 != 0), two channel slices, N % 128 != 0", rb_div=35)
_add("conv-cout4", "conv", (3, 5, 7, 64, 4, 1, 0), _c(T32, CONV=1, vec16=False), "Cout = 4: 8-byte stores")
_add("conv-s2-odd", "conv", (2, 5, 7, 64, 64, 2, 0), _c(T32, CONV=1), "stride 2 on odd extents (3 x 4 outputs)")
_add("conv-s2-even", "conv", (2, 6, 8, 128, 64, 2, 0), _c(T32, CONV=1, RES=True), "stride 2 on even extents: the last tap column is the image's last", residual=True)
for _up in (1, 3, 5, 7):
    _add(f"conv-up{_up}", "conv", (2, 3, 5, 64, 64, 1, _up), _c(T32, CONV=2, RES=_up == 7), f"nearest-2x upsample, crop code {_up}, 3 x 5", residual=_up == 7,
         rb_div=0 if _up != 3 else (2 * 3 - 1) * 10)
# ---- persistent conv
_add("pconv-s1", "conv", (8, 32, 32, 64, 1280, 1, 0), _c("persist", 4, CONV=1), "stride 1, nine K-tiles of one slice", rb_div=1024)
_add("pconv-up", "conv", (8, 16, 16, 64, 1280, 1, 1), _c("persist", 4, CONV=2, RES=True), "upsample folded into the DMA addresses", residual=True)
_add("pconv-s2", "conv", (8, 64, 64, 64, 1280, 2, 0), _c("persist", 4, CONV=1), "stride 2 from 64 x 64")
# ---- GEGLU
_add("geglu-m5", "geglu", (5, 512, 64), _c(T32, EPI="geglu"), "M = 5: masked rows; gates pinned on / off per column (512 columns: enough outputs for ties of both parities)")
_add("geglu-m300", "geglu", (300, 192, 64), _c(T32, EPI="geglu"), "ragged M and a 64-column last tile")
_add("geglu-persist", "geglu", (8192, 1024, 64), _c("persist", 4, EPI="geglu"), "persistent GEGLU epilogue (rounded, swizzled staging)")
_add("geglu-nobias", "geglu", (300, 192, 128), _c(T32, EPI="geglu"), "bias None (random inputs only: no bias, no pin)", bias=False, exact=False)
_add("geglu-persist-nobias", "geglu", (8192, 1024, 128), _c("persist", 4, EPI="geglu"), "persistent GEGLU reading the zero-filled bias image", bias=False, exact=False)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
