"""float64 oracle of the attention backward (TEST INFRASTRUCTURE; plain torch, no HIP; the product never imports this file).

Three things live here, shared by tests/test_attn_bwd_ref_host.py (CPU) and tests/test_attn_bwd_edges_gpu.py:

  * ``exact`` / ``exact_temporal`` / ``exact_delta``: the gradients of ``out_scale * softmax(Q K^T / sqrt(D)) V`` in float64 from the
    16-bit inputs, through arbitrary row maps (``tests.torch_ops.rowmap_indices``), with ``q_len != kv_len``, shared key groups
    (``q_per_kv``) and ``do_scale``.
  * ``rounded`` / ``rounded_temporal``: the same formulas in float64 with ONLY the roundings the kernels' headers admit
    (csrc/attn_bwd.hip): P is rounded to the storage type before ``P^T dO``; ``dS = P (dP_raw - delta / do_scale)`` is rounded to it
    before ``dS K`` and ``dS^T Q``; every result is multiplied by ``scale * do_scale`` (dV: ``do_scale``) afterwards and rounded to the
    storage type, round-to-nearest-even as ``pack16`` does.  ``delta`` is the exact ``sum_k P dP`` (``stats="recompute"``) or
    ``rowsum(dO * round(O))`` (``stats="given"``: a3d_attn_delta on the 16-bit forward output).  The host's per-group-partials route
    for shared keys (hip_ops.py, ``HipOps.flash_attn_bwd``: every query group's dK | dV partial is STORED in 16 bits, the partials are
    summed in fp32 and rounded again) is ``route="partials"``; the in-kernel sharing loop sums in the accumulators and rounds once
    (``route="kernel"``).  The temporal kernel (csrc/train_ops.hip) keeps P and dS in fp32: its model is ``exact`` rounded once on the
    way out.  This model is the yardstick of the bars — the arithmetic of the header, never a kernel's output.
  * ``row_report``: the comparison of the bars, in one place; the case table (shapes, maps, value regimes) with the launch variant per
    pass each case claims to reach, and a small Python mirror of the dispatch predicates of csrc/attn_bwd.hip (``launch``) and of the
    host's 512-workgroup threshold.

``mutant=`` of ``rounded`` builds one classic kernel mistake into the model (CPU only; no kernel is ever built broken): the host
test feeds them to ``row_report`` to prove that the bars bite.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch

from animate3d_amd.hip_ops import RowMap
from tests.torch_ops import rowmap_indices

F64 = torch.float64
HEAD_DIMS = (40, 64, 80, 160)
ATTN_TOL = {torch.bfloat16: 2e-2, torch.float16: 3e-3}        # whole tensor, relative L2 (tests/test_train_kernels_gpu.py)
ELEM_TOL = {torch.bfloat16: 6e-3, torch.float16: 1e-3}
ROW_MARGIN = 2.0                                              # per row: e_i(kernel) <= 2 max(e_i(model), median_j e_j(model))

# ------------------------------------------------------------------ mirror of the dispatch (csrc/attn_bwd.hip: dispatch / launch)
BR = {40: 128, 64: 64, 80: 64, 160: 32}                       # rows per LDS tile = 32 * NU
COLS_PER_WG = 128                                             # 4 waves x 32 columns (CT = 1)
SHARED_WG_THRESHOLD = 512                                     # HipOps.flash_attn_bwd: below it, shared keys go by per-group partials
PASSES = ("stats", "dq", "dkv")


def launch_variant(D: int, mode: str, qmap: RowMap, kmap: RowMap, q_len: int, kv_len: int, ld_max: int = 4096) -> Tuple[str, str]:
    """(variant, body) of one pass: variant in dma / aligned / unaligned, body in full / ragged.  The row side is (Q, dO) in the dK|dV
    pass (HipOps passes the query map for dO) and K|V otherwise."""
    br = BR[D]
    seg, rlen = (qmap.seg_len, q_len) if mode == "dkv" else (kmap.seg_len, kv_len)
    aligned = seg % br == 0
    ragged = rlen % br != 0
    dma = mode != "stats" and aligned and not ragged and br * ld_max * 2 < (1 << 31)
    return ("dma" if dma else "aligned" if aligned else "unaligned", "ragged" if ragged else "full")


def dkv_route(groups: int, heads: int, kv_len: int, q_per_kv: int, need_dkv: bool = True) -> str:
    """"partials" (one private dK | dV per query group, reduced on the host side) or "kernel" (summed inside the dK|dV pass)."""
    wgs_shared = (groups // q_per_kv) * heads * ((kv_len + COLS_PER_WG - 1) // COLS_PER_WG)
    return "partials" if need_dkv and q_per_kv > 1 and wgs_shared < SHARED_WG_THRESHOLD else "kernel"


def column_tiles(D: int, mode: str, q_len: int, kv_len: int) -> Tuple[int, int]:
    """(workgroups along the column side, valid columns of the last one)."""
    clen = kv_len if mode == "dkv" else q_len
    n = (clen + COLS_PER_WG - 1) // COLS_PER_WG
    return n, clen - (n - 1) * COLS_PER_WG


# every (pass, variant, body) cell that exists: the statistics pass has no DMA launch; an aligned launch of full tiles IS the DMA launch
CELLS = {"stats": {("aligned", "full"), ("aligned", "ragged"), ("unaligned", "full"), ("unaligned", "ragged")},
         "dq": {("dma", "full"), ("aligned", "ragged"), ("unaligned", "full"), ("unaligned", "ragged")},
         "dkv": {("dma", "full"), ("aligned", "ragged"), ("unaligned", "full"), ("unaligned", "ragged")}}


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    name: str
    D: int
    heads: int
    groups: int
    q_len: int
    kv_len: int
    q_per_kv: int
    qmap: RowMap
    kmap: RowMap
    q_rows: int
    k_rows: int
    fused: bool                      # Q, K, V are column blocks of one [rows, 3C] buffer (q_rows == k_rows)
    claims: Dict[str, Tuple[str, str]] = field(hash=False, compare=False, default_factory=dict)
    do_scale: float = 1.0

    @property
    def C(self):
        return self.heads * self.D


def views(n, F, L, b=1):
    """The multi-view layout of the model: rows (b n f) l, one group per (b, f), n segments of L rows F L apart; and the first-frame key
    map (frame 0's keys for all F frames of a video)."""
    qm = RowMap(gdiv=F, ga=n * F * L, gb=L, seg_len=L, seg_stride=F * L)
    k0 = RowMap(gdiv=F, ga=n * F * L, gb=0, seg_len=L, seg_stride=F * L)
    return qm, k0, b * n * F * L


_ALL = lambda v, body: {"stats": ("aligned" if v == "dma" else v, body), "dq": (v, body), "dkv": (v, body)}


def cases(D: int, heads: int = 2) -> Dict[str, Case]:
    """The launch matrix at head_dim D (tile rows B = BR[D]); ``claims`` = (variant, body) per pass, written down here and checked
    against ``launch_variant`` by the host test."""
    B = BR[D]
    out = {}

    def add(name, groups, q_len, kv_len, share, qmap, kmap, q_rows, k_rows, fused, claims, do_scale=1.0):
        out[name] = Case(name, D, heads, groups, q_len, kv_len, share, qmap, kmap, q_rows, k_rows, fused, claims, do_scale)

    qm, k0, rows = views(2, 2, B)
    add("dma_self", 2, 2 * B, 2 * B, 1, qm, qm, rows, rows, True, _ALL("dma", "full"))
    add("one_view_q", 2, B, 2 * B, 1, qm, qm, rows, rows, True, _ALL("dma", "full"))
    qs, _, rows_s = views(2, 2, B - 8)
    add("ragged_self", 2, 2 * B - 16, 2 * B - 16, 1, qs, qs, rows_s, rows_s, True, _ALL("unaligned", "ragged"))
    qh, _, rows_h = views(2, 2, B // 2)
    add("half_segments", 2, B, B, 1, qh, qh, rows_h, rows_h, True, _ALL("unaligned", "full"))
    ident = lambda n: RowMap(gdiv=1, ga=n, gb=0, seg_len=B, seg_stride=B)            # seg_len = seg_stride: consecutive rows
    add("identity_ragged", 2, B + 8, B + 8, 1, ident(B + 8), ident(B + 8), 2 * (B + 8), 2 * (B + 8), True, _ALL("aligned", "ragged"))
    if B + 8 != 136:
        add("cols136", 2, 136, 136, 1, ident(136), ident(136), 2 * 136, 2 * 136, True, _ALL("aligned", "ragged"))
    add("short_q", 2, B - 8, 2 * B, 1, RowMap(1, B - 8, 0, B - 8, 0), qm, 2 * (B - 8), rows, False,
        {"stats": ("aligned", "full"), "dq": ("dma", "full"), "dkv": ("unaligned", "ragged")})
    # the cross-attention training geometry: 3 frames of one video against its 77 text tokens, out_scale 0.6 (the IP branch's)
    add("cross77", 3, 2 * B, 77, 3, RowMap(1, 2 * B, 0, 2 * B, 0), RowMap(3, 77, 0, 77, 0), 3 * 2 * B, 77, False,
        {"stats": ("unaligned", "ragged"), "dq": ("unaligned", "ragged"), "dkv": ("dma", "full")}, 0.6)
    q3, k3, rows3 = views(2, 3, B)
    add("first_frame", 3, 2 * B, 2 * B, 3, q3, k3, rows3, rows3, True, _ALL("dma", "full"))
    q3r, k3r, rows3r = views(2, 3, B - 8)
    add("first_frame_ragged", 3, 2 * B - 16, 2 * B - 16, 3, q3r, k3r, rows3r, rows3r, True, _ALL("unaligned", "ragged"))
    return out


PLANT_SCALE = 1.5                    # value regimes of make_inputs: randn, planted, ramp_up, ramp_down


def planted_positions(c: Case):
    """Key positions that get a copy of a query (and that query's position): 0, B - 1, B, the first key of the last tile, the last valid
    key.  Key 0 and the last key copy the SAME query: its weight splits about in half, so its gradient does not vanish."""
    B = BR[c.D]
    pos = [0, B - 1, B, (c.kv_len - 1) // B * B, c.kv_len - 1]
    qs = [5, 17, 29, 41, 5]
    seen, res = set(), []
    for p, s in zip(pos, qs):
        if 0 <= p < c.kv_len and p not in seen:
            seen.add(p)
            res.append((p, s % c.q_len))
    return res


def make_inputs(c: Case, dtype, device="cpu", regime: str = "randn", seed: int = 0):
    """(q, k, v, do) as the entry points take them: 16-bit [rows, C] column views of wider buffers (K | V | Q of one fused buffer where the
    case says so, K | V of one otherwise); dO has its own buffer and stride."""
    g = torch.Generator().manual_seed(1000 * c.D + seed)
    C = c.C
    qf = torch.randn(c.q_rows, C, generator=g)
    kf = torch.randn(c.k_rows, C, generator=g)
    vf = torch.randn(c.k_rows, C, generator=g)
    dof = torch.randn(c.q_rows, C, generator=g)
    qf = qf.to(dtype).float()
    qi = rowmap_indices(c.qmap, c.groups, c.q_len)
    ki = rowmap_indices(c.kmap, c.groups, c.kv_len)
    if regime == "planted":
        for grp in range(0, c.groups, c.q_per_kv):
            for p, s in planted_positions(c):
                kf[ki[grp, p]] = PLANT_SCALE * qf[qi[grp, s]]
    elif regime in ("ramp_up", "ramp_down"):
        ramp = torch.linspace(0.25, 4.0, c.kv_len)
        if regime == "ramp_down":
            ramp = ramp.flip(0)
        for grp in range(0, c.groups, c.q_per_kv):
            kf[ki[grp]] = kf[ki[grp]] * ramp[:, None]
    elif regime != "randn":
        raise ValueError(regime)
    if c.fused:
        buf = torch.cat([kf, vf, qf], dim=1).to(dtype).to(device)
        k, v, q = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:]
    else:
        kv = torch.cat([kf, vf], dim=1).to(dtype).to(device)
        k, v = kv[:, :C], kv[:, C:]
        q = torch.cat([qf, qf], dim=1).to(dtype).to(device)[:, C:]
    do = torch.cat([dof, dof[:, :8]], dim=1).to(dtype).to(device)[:, :C]
    return q, k, v, do


# ------------------------------------------------------------------ the float64 formulas
def round_to(x, storage):
    """Round to the storage type, nearest-even, from the fp32 value the kernel holds (pack16)."""
    return x if storage is None else x.to(torch.float32).to(storage).to(F64)


_r = round_to


def _gather(t, idx, heads):                     # [rows, C] -> [G, heads, len, D] float64
    G, n = idx.shape
    return t.to(F64)[idx.reshape(-1)].reshape(G, n, heads, -1).transpose(1, 2)


def _rows(vals):                                # [G, heads, len, D] -> [G * len, C]
    G, H, n, D = vals.shape
    return vals.transpose(1, 2).reshape(G * n, H * D)


@dataclass
class Grads:
    dq: torch.Tensor          # [q rows, C] float64, zero on rows the query map never reaches
    dk: torch.Tensor          # [k rows, C]
    dv: torch.Tensor
    lse2: torch.Tensor        # [groups, heads, q_len], log2 units
    o: torch.Tensor           # [q rows, C] float64: out_scale * softmax(..) V, unrounded
    q_index: torch.Tensor     # rows the maps reach (sorted, unique)
    k_index: torch.Tensor


MUTANTS = ("clamped_key_twice", "last_row_tile_dropped", "first_group_stats", "neighbour_head_lse", "key_row_shifted")


def _gradients(q, k, v, do, qmap, kmap, groups, heads, q_len, kv_len, q_per_kv, do_scale, storage, stats, route, mutant) -> Grads:
    dev = q.device
    C = q.shape[1]
    D = C // heads
    scale = D ** -0.5
    assert groups % q_per_kv == 0 and stats in ("recompute", "given") and route in ("kernel", "partials")
    assert mutant is None or mutant in MUTANTS
    qi = rowmap_indices(qmap, groups, q_len).to(dev)
    ki = rowmap_indices(kmap, groups, kv_len).to(dev)
    sets = groups // q_per_kv
    assert torch.equal(ki.reshape(sets, q_per_kv, kv_len), ki[::q_per_kv, None, :].expand(sets, q_per_kv, kv_len)), \
        "the q_per_kv query groups of a set must read the same key rows"
    ki_read, T = ki, kv_len
    if mutant == "key_row_shifted":             # one key read one row further on, inside the second map segment
        ki_read = ki.clone()
        ki_read[:, kmap.seg_len + 3] += 1
    if mutant == "clamped_key_twice":           # the clamped row behind the last valid key is not masked: the key counts once more
        ki_read = torch.cat([ki, ki[:, -1:]], dim=1)
        T = kv_len + 1
    if mutant == "last_row_tile_dropped":       # the row loop ends one tile early (keys in the statistics / dQ passes)
        T = (kv_len - 1) // BR[D] * BR[D]
        ki_read = ki[:, :T]
    Q, dO = _gather(q, qi, heads), _gather(do, qi, heads)
    K, V = _gather(k, ki_read, heads), _gather(v, ki_read, heads)
    S = Q @ K.transpose(-1, -2) * scale
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    O = P @ V * do_scale
    dP = dO @ V.transpose(-1, -2)                                   # dP_raw: do_scale is applied once, to the finished gradients
    if stats == "given":
        assert do_scale != 0.0
        delta = (dO * _r(O, storage)).sum(-1) / do_scale            # a3d_attn_delta on the 16-bit O, then -delta / do_scale seeds dP
    else:
        delta = (P * dP).sum(-1)
    lse_q, lse_kv, delta_kv = lse, lse, delta
    if mutant == "neighbour_head_lse":
        lse_q = lse_kv = lse.roll(1, dims=1)
    if mutant == "first_group_stats":           # the dK|dV pass reads lse / delta of group grp_c for all q_per_kv groups of the set
        first = lambda t: t.reshape(sets, q_per_kv, *t.shape[1:])[:, :1].expand(sets, q_per_kv, *t.shape[1:]).reshape(t.shape)
        lse_kv, delta_kv = first(lse), first(delta)

    def p_ds(lse_, delta_):
        P_ = torch.exp(S - lse_[..., None])
        return _r(P_, storage), _r(P_ * (dP - delta_[..., None]), storage)

    _, dS_q = p_ds(lse_q, delta)
    P_kv, dS_kv = p_ds(lse_kv, delta_kv)
    dQ = _r(dS_q @ K * (scale * do_scale), storage)
    dK = dS_kv.transpose(-1, -2) @ Q * (scale * do_scale)           # per query group: [G, heads, T, D]
    dV = P_kv.transpose(-1, -2) @ dO * do_scale
    if mutant == "clamped_key_twice":           # both copies land on the last key's row
        fold = lambda t: torch.cat([t[:, :, :kv_len - 1], t[:, :, kv_len - 1:kv_len] + t[:, :, kv_len:]], dim=2)
        dK, dV = fold(dK), fold(dV)
    if mutant == "last_row_tile_dropped":
        pad = lambda t: torch.cat([t, t.new_zeros(groups, heads, kv_len - T, D)], dim=2)
        dK, dV = pad(dK), pad(dV)

    def share(t):                               # sum over the q_per_kv query groups of a set, with the route's roundings
        t = t.reshape(sets, q_per_kv, heads, kv_len, D)
        if route == "partials" and q_per_kv > 1:
            t = _r(t, storage)                  # every group's partial is stored in 16 bits; torch.sum then accumulates in fp32
        return _r(t.sum(dim=1), storage)

    dK, dV = share(dK), share(dV)
    q_index, k_index = torch.unique(qi), torch.unique(ki)
    assert q_index.numel() == qi.numel() and k_index.numel() == sets * kv_len, "the maps address every row at most once"
    dq = torch.zeros(q.shape[0], C, dtype=F64, device=dev).index_copy_(0, qi.reshape(-1), _rows(dQ))
    o = torch.zeros(q.shape[0], C, dtype=F64, device=dev).index_copy_(0, qi.reshape(-1), _rows(P @ V * do_scale))
    kset = ki[::q_per_kv].reshape(-1)
    dk = torch.zeros(k.shape[0], C, dtype=F64, device=dev).index_copy_(0, kset, _rows(dK))
    dv = torch.zeros(k.shape[0], C, dtype=F64, device=dev).index_copy_(0, kset, _rows(dV))
    return Grads(dq, dk, dv, lse / math.log(2.0), o, q_index, k_index)


def exact(q, k, v, do, qmap, kmap, groups, heads, q_len, kv_len, *, q_per_kv=1, do_scale=1.0) -> Grads:
    """float64 gradients from the 16-bit inputs: no rounding anywhere."""
    return _gradients(q, k, v, do, qmap, kmap, groups, heads, q_len, kv_len, q_per_kv, do_scale, None, "recompute", "kernel", None)


def rounded(q, k, v, do, qmap, kmap, groups, heads, q_len, kv_len, *, storage, stats="recompute", q_per_kv=1, do_scale=1.0,
            route="kernel", mutant=None) -> Grads:
    """The same formulas with the roundings of the kernel's header (module docstring)."""
    return _gradients(q, k, v, do, qmap, kmap, groups, heads, q_len, kv_len, q_per_kv, do_scale, storage, stats, route, mutant)


def case_args(c: Case, tensors):
    q, k, v, do = tensors
    return (q, k, v, do, c.qmap, c.kmap, c.groups, c.heads, c.q_len, c.kv_len)


# ------------------------------------------------------------------ temporal attention: rows (v f) l, attention over f per pixel and head
def exact_temporal(q, k, v, do, videos, frames, L, heads):
    """(dq, dk, dv), each [rows, C] float64."""
    C = q.shape[1]
    D = C // heads
    seq = lambda t: t.to(F64).reshape(videos, frames, L, heads, D).permute(0, 2, 3, 1, 4)       # [v, l, heads, f, D]
    back = lambda t: t.permute(0, 3, 1, 2, 4).reshape(videos * frames * L, C)
    Q, K, V, dO = seq(q), seq(k), seq(v), seq(do)
    P = torch.softmax(Q @ K.transpose(-1, -2) * D ** -0.5, dim=-1)
    dP = dO @ V.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True)) * D ** -0.5
    return back(dS @ K), back(dS.transpose(-1, -2) @ Q), back(P.transpose(-1, -2) @ dO)


def rounded_temporal(q, k, v, do, videos, frames, L, heads, *, storage):
    """P and dS stay in fp32 in csrc/train_ops.hip's temporal_attn_bwd_kernel: the only rounding is the store."""
    return tuple(_r(t, storage) for t in exact_temporal(q, k, v, do, videos, frames, L, heads))


def exact_delta(do, o, domap, omap, groups, heads, q_len):
    """(delta, bound): float64 rowsum(dO * O) per [group, head, query] and the derived bar D * 2^-24 * sum_d |dO_d O_d| of an fp32
    fused-multiply-add chain of D terms (each partial sum is at most sum |terms|, each step rounds once: (D - 1) half-ulps, below D ulps)."""
    di = rowmap_indices(domap, groups, q_len).to(do.device)
    oi = rowmap_indices(omap, groups, q_len).to(do.device)
    prod = _gather(do, di, heads) * _gather(o, oi, heads)
    D = do.shape[1] // heads
    return prod.sum(-1), D * 2.0 ** -24 * prod.abs().sum(-1)


# ------------------------------------------------------------------ the bars
@dataclass
class RowReport:
    name: str
    ratio: float              # worst e_i(kernel) / max(e_i(model), median e(model)) over the rows compared
    row: int                  # the row it is at
    rel_kernel: float         # whole tensor, relative L2 against exact
    rel_model: float
    stray: int                # values off the compared rows that are not exactly zero
    finite: bool
    tol: Optional[float]

    @property
    def ok(self) -> bool:
        return (self.finite and self.stray == 0 and self.ratio <= ROW_MARGIN and (self.tol is None or self.rel_kernel <= self.tol))

    def line(self) -> str:
        return (f"[parity] {self.name}: worst row ratio {self.ratio:.3f} (row {self.row}, bar {ROW_MARGIN:g}); rel L2 kernel {self.rel_kernel:.3e} "
                f"model {self.rel_model:.3e}" + (f" (bar {self.tol:.1e})" if self.tol is not None else "") + f"; stray {self.stray}")


def row_report(got, exact_, model, *, rows=None, tol=None, name="") -> RowReport:
    """Per row i of [rows, C] tensors, e_i(x) = ||x_i - exact_i||_2; the kernel passes when e_i(kernel) <= 2 max(e_i(model), median_j
    e_j(model)) on every row of ``rows`` (default: all), is exactly zero on all others, finite, and within ``tol`` as a whole."""
    got = got.to(F64)
    idx = torch.arange(got.shape[0], device=got.device) if rows is None else rows.to(got.device)
    ek = (got - exact_)[idx].norm(dim=1)
    em = (model - exact_)[idx].norm(dim=1)
    bound = torch.maximum(em, em.median())
    ratio = torch.where(ek <= 0, torch.zeros_like(ek), ek / bound)          # 0 / 0 -> 0, x / 0 -> inf
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = int(ratio.argmax())
    off = torch.ones(got.shape[0], dtype=torch.bool, device=got.device)
    off[idx] = False
    den = float(exact_.norm()) + 1e-300
    return RowReport(name, float(ratio[worst]), int(idx[worst]), float((got - exact_).norm()) / den, float((model - exact_).norm()) / den,
                     int((got[off] != 0).sum()), bool(torch.isfinite(got).all()), tol)
