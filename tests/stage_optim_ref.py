"""The float64 restatement of one ``StageAdam`` step (animate3d_amd/stage_optim.py, csrc/stage_optim.hip) in numpy, the bars the kernel
is held to, and the seeded inputs the tests share (TEST INFRASTRUCTURE).

The step, from the fp32 state before it, with k = step + 1 (``torch.optim.Adam`` without amsgrad, weight decay or maximize):

    m' = beta1 m + (1 - beta1) g
    v' = beta2 v + (1 - beta2) g^2
    u  = (lr / (1 - beta1^k)) m' / (sqrt(v') / sqrt(1 - beta2^k) + eps)
    p' = p - u

Bars, for every element, nothing excluded:

    m: |got - m'| <= 2^-24 |m'| + 2^-50 (|m| + |g|)
    v: |got - v'| <= 2^-24 |v'| + 2^-50 (v + g^2)
    p: |got - p'| <= 2^-24 |p'| + 2^-50 (|p| + |u|)

The first term is the one rounding to fp32 (half a unit in the last place is at most 2^-24 of the value).  The second allows eight fp64
roundings of 2^-53 on the operands: contraction and the device's ``pow`` may differ from numpy's.  Precondition, asserted here on the
restatement itself: no value to be stored is a non-zero fp32 subnormal (the first term does not cover a rounding there) and no g^2
overflows fp32.  Inputs that miss it are changed, never the bar."""
import zlib

import numpy as np

BETAS, EPS = (0.9, 0.999), 1e-15
TINY = float(np.finfo(np.float32).tiny)
F32_MAX = float(np.finfo(np.float32).max)


def adam_step(p, g, m, v, step, lr, betas=BETAS, eps=EPS):
    """(p', m', v', u) in float64 from the fp32 arrays ``p, g, m, v`` and the step count before the step."""
    p, g, m, v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    k = float(step) + 1.0
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * (g * g)
    u = (float(lr) / (1.0 - b1 ** k)) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** k) + float(eps))
    p1 = p - u
    for name, a in (("p'", p1), ("m'", m1), ("v'", v1)):
        mag = np.abs(a)
        assert not ((mag > 0) & (mag < TINY)).any(), f"{name}: a non-zero fp32 subnormal would be stored (change the inputs)"
        assert (mag <= F32_MAX).all(), f"{name}: overflows fp32 (change the inputs)"
    assert (g * g <= F32_MAX).all(), "g^2 overflows fp32 (change the inputs)"
    return p1, m1, v1, u


def bars(p, g, m, v, p1, m1, v1, u):
    """(bar_p, bar_m, bar_v), element-wise, from the fp32 state before the step and the restatement's result."""
    p, g, m, v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, g, m, v))
    r, s = 2.0 ** -24, 2.0 ** -50
    return (r * np.abs(p1) + s * (np.abs(p) + np.abs(u)), r * np.abs(m1) + s * (np.abs(m) + np.abs(g)), r * np.abs(v1) + s * (v + g * g))


def deviation(got, want):
    return np.abs(np.asarray(got).astype(np.float64) - want)


def check_step(tag, before, after, step, lr, failures, extra=None, betas=BETAS, eps=EPS, verbose=True):
    """``before`` = (p, g, m, v) fp32 arrays before the step, ``after`` = (p, m, v) as the code under test left them.  Appends to ``failures``
    what misses its bar (plus ``extra``, a per-quantity allowance such as a reference's own deviation); returns the worst ratios."""
    p, g, m, v = before
    p1, m1, v1, u = adam_step(p, g, m, v, step, lr, betas, eps)
    bp, bm, bv = bars(p, g, m, v, p1, m1, v1, u)
    worst = {}
    for name, got, want, bar in (("p", after[0], p1, bp), ("m", after[1], m1, bm), ("v", after[2], v1, bv)):
        allow = bar + (0.0 if extra is None else extra[name])
        dev = deviation(got, want)
        ratio = np.where(dev == 0, 0.0, dev / np.where(allow > 0, allow, 1e-300))
        worst[name] = float(ratio.max()) if ratio.size else 0.0
        if not (dev <= allow).all():
            failures.append((tag, name, worst[name], int((dev > allow).sum())))
    if verbose:
        print(f"[stage_optim {tag}] step {int(step)} lr {lr:g}: worst deviation / bar  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")
    return worst


def _rng(key: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(key.encode()))


def make_params(key: str, n: int) -> np.ndarray:
    """N(0, 0.3^2)"""
    return (_rng("p/" + key).standard_normal(n) * 0.3).astype(np.float32)


def make_grads(key: str, n: int) -> np.ndarray:
    """Log-uniform magnitudes in [1e-12, 1e3] with random signs, and exact zeros at every 7th element (checked on the CPU: against
    ``make_params`` these keep the precondition for three steps)."""
    r = _rng("g/" + key)
    g = (10.0 ** r.uniform(-12.0, 3.0, n)) * np.where(r.random(n) < 0.5, -1.0, 1.0)
    g[::7] = 0.0
    return g.astype(np.float32)
