"""float64 references, structured inputs and error measures for the normalisation kernels (csrc/norms.hip, the GroupNorm / LayerNorm
backward of csrc/train_ops.hip).  Shared by tests/test_norm_ref_host.py (CPU: the references' mutants must exceed the GPU tests' bounds)
and tests/test_norm_edges_gpu.py (the kernels against the references).  Everything here is plain torch in float64 computed from the
SAME 16-bit inputs the kernels read, and runs on whatever device its inputs live on.

Why structured inputs: with `randn + const` in every row, channel and group, a row dropped from the statistics or a channel counted in
the neighbouring group moves the output by less than the rounding of the storage type.  Here neighbouring groups differ in mean and scale,
and each instance carries one *probe row* of 16 x amplitude, placed where a kernel's row ownership changes hands.

Error measures (u = 2^-8 for bf16, 2^-10 for fp16: the suite's ulp; 3 is the suite's bar):
  forward, per element   |got - ref| <= 3 u (|x^ g| + |b| [+ |pe|]) + 2^-20 (|x rstd g| + |mean rstd g| + |b| [+ |pe|])
                         the second term is fp32 evaluation noise (16 roundings of 2^-24) of y = x (rstd g) + (b - mean rstd g), which
                         cancels where x^ is small; SiLU (slope <= 1.1, |silu z| <= |z|) does not amplify either term
  backward dx            relative L2 per (instance, group) block (GroupNorm) / per row (LayerNorm), the maximum over blocks
  dgamma / dbeta         relative L2 of the vector
  group_norm_sums        |d sum| <= n 2^-24 sum|x|, |d sumsq| <= n 2^-24 sum x^2, n = the longest fp32 addition chain (sums_chain)
"""
import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
FWD_ULPS = 3.0
F32_NOISE = 2.0 ** -20
DX_TOL = {torch.bfloat16: 6e-3, torch.float16: 1e-3}          # ELEM_TOL of tests/test_train_kernels_gpu.py
PARAM_TOL = 1e-4
PROBE_GAIN = 16.0

# ---- plan seams of gn_fused_plan / group_norm_launch at groups = 32: (C, last row count of one plan, first of the next, field that changes)
GN_SEAMS = [
    (1280, 132, 133, "rmax"), (1280, 252, 253, "sg"), (1280, 525, 526, "sg"), (1280, 2142, 2143, "fused"),
    (320, 252, 253, "sg"), (320, 2142, 2143, "fused"),
    (960, 88, 89, "rmax"), (960, 168, 169, "threads"), (960, 714, 715, "fused"),
    (1920, 714, 715, "fused"),
    (2560, 1071, 1072, "fused"),
    (128, 176, 177, "rmax"), (224, 99, 100, "rmax"), (288, 154, 155, "rmax"),
]
# rows below, at and above the row lanes of the C = 1280 plan (ny = 12: threads that own no row), one row, and a mid-plan count per narrow width
GN_EXTRA_ROWS = [(1280, 1), (1280, 11), (1280, 12), (1280, 13), (128, 100), (288, 100)]
# every plan segment per width at groups = 32: (first row count, threads, rmax, sg), then the last row count of the one-launch kernel
GN_PLAN_TABLE = {
    128: ([(1, 256, 11, 32), (177, 256, 21, 32), (337, 512, 11, 32), (353, 512, 21, 32), (673, 512, 11, 16), (705, 512, 21, 16),
           (1345, 512, 11, 8), (1409, 512, 21, 8), (2689, 512, 11, 4), (2817, 512, 21, 4), (5377, 512, 11, 2), (5633, 512, 21, 2)], 10752),
    224: ([(1, 256, 11, 32), (100, 256, 21, 32), (190, 512, 11, 32), (199, 512, 21, 32), (379, 512, 11, 16), (397, 512, 21, 16),
           (757, 512, 11, 8), (804, 512, 21, 8)], 1533),
    288: ([(1, 512, 11, 32), (155, 512, 21, 32), (295, 512, 11, 16), (309, 512, 21, 16), (589, 512, 11, 8), (617, 512, 21, 8)], 1176),
    320: ([(1, 512, 11, 32), (133, 512, 21, 32), (253, 512, 11, 16), (276, 512, 21, 16), (526, 512, 11, 8), (562, 512, 21, 8),
           (1072, 512, 11, 4), (1123, 512, 21, 4)], 2142),
    640: ([(1, 512, 11, 16), (133, 512, 21, 16), (253, 512, 11, 8), (276, 512, 21, 8), (526, 512, 11, 4), (562, 512, 21, 4),
           (1072, 512, 11, 2), (1123, 512, 21, 2)], 2142),
    960: ([(1, 256, 11, 8), (89, 256, 21, 8), (169, 512, 11, 8), (188, 512, 21, 8), (358, 512, 11, 4), (375, 512, 21, 4)], 714),
    1280: ([(1, 512, 11, 8), (133, 512, 21, 8), (253, 512, 11, 4), (276, 512, 21, 4), (526, 512, 11, 2), (562, 512, 21, 2),
            (1072, 512, 11, 1), (1123, 512, 21, 1)], 2142),
    1920: ([(1, 256, 11, 4), (89, 256, 21, 4), (169, 512, 11, 4), (188, 512, 21, 4), (358, 512, 11, 2), (375, 512, 21, 2)], 714),
    2560: ([(1, 512, 11, 4), (133, 512, 21, 4), (253, 512, 11, 2), (276, 512, 21, 2), (526, 512, 11, 1), (562, 512, 21, 1)], 1071),
}
GN_CHUNK_ROWS = 128          # GN_ROWS_PER_BLOCK of csrc/norms.hip: rows of one workgroup of the three-launch kernels


def gn_forward_rows():
    """(C, rows) of the GroupNorm forward cases: both sides of every seam, the extra rows, and the three-launch tails at C = 320."""
    out = []
    for C, lo, hi, _ in GN_SEAMS:
        out += [(C, lo), (C, hi)]
    out += GN_EXTRA_ROWS
    return sorted(set(out))


def gn_tail_rows(ny):
    """Row counts past 17 whole 128-row chunks whose last chunk holds 1, ny, 4 ny - 1, 4 ny and 4 ny + 1 rows: around the four-rows-in-flight
    loop of gn_partial_kernel / gn_apply_kernel."""
    return [17 * GN_CHUNK_ROWS + t for t in (1, ny, 4 * ny - 1, 4 * ny, 4 * ny + 1)]


def probe_rows(plan, rows):
    """Rows at which ownership changes hands under `plan` (hip_ops.group_norm_plan): first and last row, the last row lane and the first row
    of the second sweep, and both sides of the last sweep (one launch) or of the last 128-row chunk (three launches)."""
    ny = plan["ny"]
    if plan["fused"]:
        edge = (-(-rows // ny) - 1) * ny
    else:
        edge = (-(-rows // GN_CHUNK_ROWS) - 1) * GN_CHUNK_ROWS
    cand = [0, ny - 1, ny, edge - 1, edge, rows - 1]
    out = []
    for r in cand:
        r = min(max(r, 0), rows - 1)
        if r not in out:
            out.append(r)
    return out


def batch_probes(probes, least=4, most=6):
    """One probe row per instance: every probe once, then (while there is room) one instance WITHOUT a probe row (None) — at few rows a
    16 x row dominates its groups' variance and would hide a channel counted next door — then probes repeated up to `least` instances."""
    out = list(probes)
    if len(out) < most:
        out.append(None)
    while len(out) < least:
        out.append(probes[len(out) % len(probes)])
    return out


def sums_chain(ny, C, groups):
    """Longest fp32 addition chain of a3d_group_norm_sums (gn_partial_kernel; gn_finalize_kernel adds in fp64): a thread adds the 8
    channels of each of its ceil(128 / ny) rows, then one thread per group adds the ny row lanes of every chunk column its group touches
    (cfirst .. clast of the kernel; the widest group counts)."""
    cg = C // groups
    cols = max(((g + 1) * cg - 1) // 8 - (g * cg) // 8 + 1 for g in range(groups))
    return -(-GN_CHUNK_ROWS // ny) * 8 + ny * cols


# ------------------------------------------------------------------ input builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def group_profile(groups):
    """Per-group mean alternating +-2 and scale alternating 0.5 / 2 in pairs of groups."""
    g = torch.arange(groups)
    mean = torch.where(g % 2 == 0, 2.0, -2.0).double()
    scale = torch.where((g // 2) % 2 == 0, 0.5, 2.0).double()
    return mean, scale


def affine(C, seed):
    gen = _gen(seed + 7)
    gamma = (1.0 + 0.2 * torch.randn(C, generator=gen)).float()
    beta = (0.1 * torch.randn(C, generator=gen)).float()
    return gamma, beta


def structured(B, rows, C, groups, probes, dtype, seed=0, mean_over_std=None, iid=False):
    """x [B * rows, C] in `dtype` (CPU), gamma, beta (fp32).  probes[b] = None: no probe row in instance b.  mean_over_std = k: every
    group's mean is +-k times its scale instead of +-2.  iid=True: `randn + 0.5` everywhere, no probe rows (the counter-example)."""
    assert len(probes) == B
    cg = C // groups
    z = torch.randn(B, rows, C, generator=_gen(seed), dtype=torch.float64)
    if iid:
        x = z + 0.5
    else:
        mean, scale = group_profile(groups)
        if mean_over_std is not None:
            mean = mean.sign() * mean_over_std * scale
        x = z * scale.repeat_interleave(cg) + mean.repeat_interleave(cg)
        for b, r in enumerate(probes):
            if r is not None:
                x[b, r] *= PROBE_GAIN
    gamma, beta = affine(C, seed)
    return x.reshape(B * rows, C).to(dtype), gamma, beta


def structured_dy(x, B, rows, C, groups, probes, dtype, seed=0, iid=False):
    """dy = per-group constant (1 or -1.5) x (1 + 0.5 x^) + 0.5 randn, the probe row scaled like x's: both group sums of the backward
    (sum g gamma, sum g gamma x^) are then of the size of the main term."""
    z = torch.randn(B, rows, C, generator=_gen(seed + 1), dtype=torch.float64)
    if iid:
        return z.reshape(B * rows, C).to(dtype)
    cg = C // groups
    xh = gn_stats(x, B, rows, groups, 1e-5)[2]
    const = torch.where(torch.arange(groups) % 2 == 0, 1.0, -1.5).double().repeat_interleave(cg)
    dy = const * (1.0 + 0.5 * xh.reshape(B, rows, C).cpu()) + 0.5 * z
    for b, r in enumerate(probes):
        if r is not None:
            dy[b, r] *= PROBE_GAIN
    return dy.reshape(B * rows, C).to(dtype)


def structured_rows(M, C, probes, dtype, seed=0, iid=False):
    """LayerNorm analogue, per row: mean alternating +-8, scale 0.25 .. 4 cycling over five rows, a different offset per 16-byte chunk (a
    lane left out of a row's reduction then moves the mean), the rows of `probes` at 16 x amplitude.  Returns x, gamma, beta."""
    z = torch.randn(M, C, generator=_gen(seed), dtype=torch.float64)
    gamma, beta = affine(C, seed)
    if iid:
        return (z + 0.5).to(dtype), gamma, beta
    r = torch.arange(M)
    mean = torch.where(r % 2 == 0, 8.0, -8.0).double()[:, None]
    scale = (0.25 * 2.0 ** (r % 5).double())[:, None]
    chunk = (0.25 * ((torch.arange(C) // 8 * 7) % 5 - 2)).double()[None, :]          # |scale * chunk| <= 2: never cancels the row mean
    x = mean + scale * (z + chunk)
    for p in probes:
        x[p] *= PROBE_GAIN
    return x.to(dtype), gamma, beta


def structured_rows_dy(x, gamma, probes, dtype, seed=0, iid=False):
    z = torch.randn(x.shape, generator=_gen(seed + 1), dtype=torch.float64)
    if iid:
        return z.to(dtype)
    xh = ln_stats(x, 1e-5)[2].cpu()
    const = torch.where(torch.arange(x.shape[0]) % 2 == 0, 1.0, -1.5).double()[:, None]
    dy = const * (1.0 + 0.5 * xh) + 0.5 * z
    for p in probes:
        dy[p] *= PROBE_GAIN
    return dy.to(dtype)


# ------------------------------------------------------------------ GroupNorm references
def _group_of(C, groups, shift_channel=None):
    """Channel -> group map; shift_channel = c: the MUTANT that counts boundary channel c in the neighbouring group (c = first channel of
    a group: in the one before; last channel: in the one after)."""
    cg = C // groups
    grp = torch.arange(C) // cg
    if shift_channel is not None:
        grp[shift_channel] += -1 if shift_channel % cg == 0 else 1
    return grp


def gn_sums(x, B, rows, groups, row_weight=None, shift_channel=None):
    """float64 [B, groups, 2] = (sum, sum of squares) and the element counts [B, groups].  row_weight [B, rows] (0 / 1) and shift_channel
    build the mutants: a row left out, a boundary channel counted next door."""
    C = x.shape[1]
    t = x.double().reshape(B, rows, C)
    if row_weight is not None:
        t = t * row_weight.to(t)[:, :, None]
    grp = _group_of(C, groups, shift_channel).to(x.device)
    onehot = torch.zeros(C, groups, dtype=torch.float64, device=x.device)
    onehot[torch.arange(C, device=x.device), grp] = 1.0
    s = t.sum(dim=1) @ onehot
    q = (t * t).sum(dim=1) @ onehot
    return torch.stack([s, q], dim=-1)


def gn_stats(x, B, rows, groups, eps, sums=None):
    """(mean [B, groups], rstd [B, groups], x^ [B * rows, C]) in float64; `sums` replaces the tensor's own (mutants).  The element count is
    always rows * cg: a kernel that loses a row still divides by the full count."""
    C = x.shape[1]
    cg = C // groups
    if sums is None:
        sums = gn_sums(x, B, rows, groups)
    n = float(rows * cg)
    mean = sums[..., 0] / n
    var = (sums[..., 1] / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x.double().reshape(B, rows, C) - mean.repeat_interleave(cg, dim=1)[:, None, :]) * rstd.repeat_interleave(cg, dim=1)[:, None, :]
    return mean, rstd, xh.reshape(B * rows, C)


def silu(z):
    return z * torch.sigmoid(z)


def gn_forward(x, B, rows, gamma, beta, groups, eps, act, sums=None, stats=None):
    """(y, bound_terms): y float64 [B * rows, C]; bound_terms = (|x^ g| + |b|, |x rstd g| + |mean rstd g| + |b|) for fwd_bound.
    stats = (mean, rstd) float64 [B, groups] given: the apply half."""
    C = x.shape[1]
    cg = C // groups
    if stats is None:
        mean, rstd, xh = gn_stats(x, B, rows, groups, eps, sums)
    else:
        mean, rstd = stats
        xh = ((x.double().reshape(B, rows, C) - mean.repeat_interleave(cg, dim=1)[:, None, :])
              * rstd.repeat_interleave(cg, dim=1)[:, None, :]).reshape(B * rows, C)
    g, b = gamma.double().to(x.device), beta.double().to(x.device)
    pre = xh * g + b
    y = silu(pre) if act else pre
    sc = (rstd.repeat_interleave(cg, dim=1) * g)[:, None, :]                                   # [B, 1, C]
    big = ((x.double().reshape(B, rows, C) * sc).abs() + (mean.repeat_interleave(cg, dim=1)[:, None, :] * sc).abs()).reshape(B * rows, C)
    return y, ((xh * g).abs() + b.abs(), big + b.abs())


def gn_forward2(xa, xb, B, rows, gamma, beta, groups, eps, act):
    """Two-source GroupNorm: the reference is the one-source one over the concatenation."""
    return gn_forward(torch.cat([xa, xb], dim=1), B, rows, gamma, beta, groups, eps, act)


def fwd_bound(terms, dtype):
    small, big = terms
    return FWD_ULPS * U[dtype] * small + F32_NOISE * big


def gn_backward(x, dy, B, rows, gamma, beta, groups, eps, act, row_weight=None, extra_row=None):
    """float64 dx [B * rows, C], dgamma [C], dbeta [C].  Mutants: row_weight [B, rows] leaves rows out of the two group sums (dx only);
    extra_row = (b, r) counts that row once more in dgamma / dbeta (a row index past the range, clamped)."""
    C = x.shape[1]
    cg = C // groups
    mean, rstd, xh = gn_stats(x, B, rows, groups, eps)
    gm, bt = gamma.double().to(x.device), beta.double().to(x.device)
    g = dy.double()
    if act:
        z = xh * gm + bt
        sg = torch.sigmoid(z)
        g = g * sg * (1.0 + z * (1.0 - sg))
    gg = (g * gm).reshape(B, rows, groups, cg)
    xh4 = xh.reshape(B, rows, groups, cg)
    w = 1.0 if row_weight is None else row_weight.to(gg)[:, :, None, None]
    n = float(rows * cg)
    s1 = (gg * w).sum(dim=(1, 3), keepdim=True) / n
    s2 = (gg * xh4 * w).sum(dim=(1, 3), keepdim=True) / n
    dx = (rstd[:, None, :, None] * (gg - s1 - xh4 * s2)).reshape(B * rows, C)
    dgamma, dbeta = (g * xh).sum(dim=0), g.sum(dim=0)
    if extra_row is not None:
        i = extra_row[0] * rows + extra_row[1]
        dgamma, dbeta = dgamma + g[i] * xh[i], dbeta + g[i]
    return dx, dgamma, dbeta


# ------------------------------------------------------------------ LayerNorm references


def ln_stats(x, eps, skip=None):
    """(mean [M, 1], rstd [M, 1], x^) in float64.  skip = (row, channel mask): the MUTANT that leaves a lane's chunks out of that row's two
    reductions (the divisor stays C)."""
    t = x.double()
    C = t.shape[1]
    w = torch.ones_like(t)
    if skip is not None:
        w[skip[0], skip[1].to(x.device)] = 0.0
    mean = (t * w).sum(dim=1, keepdim=True) / C
    var = (((t - mean) ** 2) * w).sum(dim=1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(var + eps)
    return mean, rstd, (t - mean) * rstd


def pe_rows(pe, div, M):
    m = torch.arange(M, device=pe.device)
    return pe.double()[(m // div) % pe.shape[0]]


def ln_forward(x, gamma, beta, eps, pe1=None, pe1_div=1, pe2=None, pe2_div=1, skip=None):
    """((y1, terms1), (y2, terms2)) as gn_forward, the embedding's magnitude added to both bound terms."""
    mean, rstd, xh = ln_stats(x, eps, skip)
    g, b = gamma.double().to(x.device), beta.double().to(x.device)
    y = xh * g + b
    small = (xh * g).abs() + b.abs()
    big = (x.double() * rstd * g).abs() + (mean * rstd * g).abs() + b.abs()
    out = []
    for pe, div in ((pe1, pe1_div), (pe2, pe2_div)):
        e = 0.0 if pe is None else pe_rows(pe, div, x.shape[0])
        ea = 0.0 if pe is None else e.abs()
        out.append((y + e, (small + ea, big + ea)))
    return out


def ln_backward(x, dy, gamma, eps, skip=None, extra_row=None):
    """float64 dx, dgamma, dbeta.  Mutants: skip as ln_stats (and out of the row's two backward sums); extra_row counts a row twice in
    dgamma / dbeta."""
    mean, rstd, xh = ln_stats(x, eps, skip)
    C = x.shape[1]
    gm = gamma.double().to(x.device)
    d = dy.double()
    gy = d * gm
    w = torch.ones_like(gy)
    if skip is not None:
        w[skip[0], skip[1].to(x.device)] = 0.0
    a = (gy * w).sum(dim=1, keepdim=True) / C
    b = (gy * xh * w).sum(dim=1, keepdim=True) / C
    dx = rstd * (gy - a - xh * b)
    dgamma, dbeta = (d * xh).sum(dim=0), d.sum(dim=0)
    if extra_row is not None:
        dgamma, dbeta = dgamma + d[extra_row] * xh[extra_row], dbeta + d[extra_row]
    return dx, dgamma, dbeta


# ------------------------------------------------------------------ error measures
def fwd_excess(got, ref, bound):
    """max over elements of |got - ref| / bound (<= 1 passes), and where."""
    ratio = (got.double() - ref).abs() / bound
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i


def block_rel_l2(got, ref):
    """Relative L2 per block (row of the 2-D arguments), the maximum over blocks."""
    g, r = got.double(), ref.double()
    return float(((g - r).norm(dim=-1) / (r.norm(dim=-1) + 1e-300)).max())


def gn_blocks(t, B, rows, groups):
    """[B * rows, C] -> [B * groups, rows * cg]: one block per (instance, group)."""
    C = t.shape[1]
    return t.reshape(B, rows, groups, C // groups).permute(0, 2, 1, 3).reshape(B * groups, -1)


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / (ref.norm() + 1e-300))


# ------------------------------------------------------------------ the cases of tests/test_norm_edges_gpu.py (and of the mutation checks)
GROUPS = 32
GN2_CASES = [(256, 1280, 640), (64, 1280, 1280), (2143, 640, 320)]          # rows, Ca, Cb: two straddling one-launch slabs, one three-launch
GN_SUMS_WIDTHS = (128, 224, 288)
GN_SHARD_ROWS = (1, 127, 128, 129)


def gn_bwd_rpb(C):
    """Rows a workgroup of gn_bwd_sums_kernel / gn_bwd_apply_kernel steps over at once (a3d_group_norm_bwd)."""
    nch = C // 8
    return 1 if nch >= 256 else 256 // nch


def gn_bwd_cases():
    """(B, rows, C, groups): rows in {1, rpb - 1, 8 rpb, 8 rpb + 1} per width (a workgroup takes at least 8 row steps), B = 700 at few rows
    (ceil(2048 / 700) = 3 workgroups per instance where the rows would fill 4: the workgroup-count cap), 64 groups, and 4 channels per group."""
    out = []
    for C in (320, 960, 1280, 2560):
        rpb = gn_bwd_rpb(C)
        for rows in sorted({1, rpb - 1, 8 * rpb, 8 * rpb + 1} - {0}):
            out.append((3, rows, C, GROUPS))
    out += [(700, 24 * gn_bwd_rpb(320) + 1, 320, GROUPS), (3, 33, 512, 64), (3, 8 * gn_bwd_rpb(128) + 1, 128, GROUPS)]
    return out


def gn_bwd_probes(B, rows, C):
    rpb = gn_bwd_rpb(C)
    base = [r for r in dict.fromkeys([rows - 1, 0, rpb - 1, rpb, 8 * rpb - 1, 8 * rpb]) if 0 <= r < rows]
    return [base[b % len(base)] for b in range(B)]


LN_ROWS_WIDTHS = (320, 640, 1280)


def ln_rpw(C):
    """Rows a wave of the sub-wave rows kernels handles per step (64 / LPR, LPR = C / 40 lanes per row)."""
    return 64 // (C // 40)


def ln_rows_seams(C):
    """M around the rows per wave step (RPW) and the rows per workgroup of the forward (R = 4 waves x LN_BATCH 4 x RPW)."""
    rpw = ln_rpw(C)
    R = 16 * rpw
    return sorted({1, rpw - 1, rpw, rpw + 1, R - 1, R, R + 1} - {0})


LN_FWD_GENERIC = [(7, C) for C in (8, 512, 520, 768, 1024, 1032, 1536)]
LN_BWD_GENERIC = [(7, C) for C in (8, 100, 328, 648, 1288, 2048)] + [(8195, 72)]       # the last: 2048 workgroups x 4 rows, then a second sweep
LN_BWD_LOOPS = [(4099, 1280, True), (16391, 320, True), (32771, 1280, False)]          # M, C, parameter gradients: > 512 / > 4096 workgroups' worth


def ln_probes(M, C):
    """Probe rows of a LayerNorm case: first and last row, both sides of the first wave step (rows kernels) or workgroup (4 rows), and both
    sides of the first grid-stride sweep where there is one."""
    step = ln_rpw(C) if C in LN_ROWS_WIDTHS else 4
    sweep = 512 * 4 * step if C in LN_ROWS_WIDTHS else 2048 * 4
    cand = [0, step - 1, step, sweep - 1, sweep, M - 1]
    return [r for r in dict.fromkeys(cand) if 0 <= r < M]


def ln_lane_mask(C, kind, lane):
    """Channels one lane of a row reads.  kind "rows": 16-byte chunk = lane + LPR i (sub-wave rows kernels, forward and backward);
    "chunks": chunk = lane + 64 i (layer_norm_kernel); "elems": channel = lane + 64 k (layer_norm_bwd_kernel)."""
    ch = torch.arange(C)
    if kind == "rows":
        return (ch // 8) % (C // 40) == lane
    if kind == "chunks":
        return (ch // 8) % 64 == lane
    return ch % 64 == lane
