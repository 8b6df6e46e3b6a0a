"""The splat rasterizer on the MI355X, one branch at a time: the constructed scenes of tests/splat_scenes.py through the public
``splat.rasterize_gaussians`` / ``GaussianRasterizer`` against the float64 oracle tests/gs_ref.py evaluated on the device.

Every scene keeps each decision of the contract (cull, clamp, skip, stop, depth order, radius and rectangle rounding) at least
gs_ref.MIN_MARGINS from its threshold, and the fp32 oracle takes them all the way float64 does (tests/test_splat_host.py proves both
on the CPU), so nothing is masked here: integers are compared exactly, every tensor by relative L2, and with at most 8 Gaussians a
wrong branch is an O(1) relative error.

Bars.  e32 is the relative L2 of the oracle evaluated in fp32 on the same inputs against float64: what plain fp32 arithmetic costs on
this scene and tensor.
* forward (image, depth, alpha): max(4 e32, 2^-20), the project's factor for another summation order and its floor (tests/test_arap_gpu.py,
  tests/test_stage4d_gpu.py);
* gradients of every input, means2D included: max(16 e32, 2^-18).  16 = 4 x 4: the same 4, times 4 for ``__expf``, whose argument
  power * log2(e) is rounded in fp32 with |power| <= ln 255, which bounds the relative error of G by about 9 * 2^-23 ~ 2^-20
  against 2^-23 for torch's exp.
A reference tensor that is exactly zero asks for exactly zero.  Each test prints e32, the kernel's error and the bar per tensor
(profiles/pytest_gpu_splat_edges.log)."""
import pytest
import torch

from animate3d_amd import splat
from tests import gs_ref, splat_scenes

pytestmark = pytest.mark.gpu

SCENES = splat_scenes.SCENES
FWD = ("image", "depth", "alpha")
COTANGENTS = {"all": (1.0, 1.0, 1.0), "image": (1.0, 0.0, 0.0), "alpha": (0.0, 0.0, 1.0), "depth": (0.0, 1.0, 0.0)}
_REF = {}


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    d, n = float((a - b).norm()), float(b.norm())
    return d / n if n > 0 else (0.0 if d == 0 else float("inf"))


def _cot(sc, B):
    g = torch.Generator().manual_seed(11)
    H, W = sc["H"], sc["W"]
    return [torch.randn(B, 3, H, W, generator=g).cuda(), (torch.randn(B, 1, H, W, generator=g) * 0.1).cuda(), torch.randn(B, 1, H, W, generator=g).cuda()]


def _run(fn, sc, dtype, means2D, cot="all", cots=None):
    """(image, radii, depth, alpha), {input: gradient} of ``fn`` on the scene under the loss that ``cot`` selects: only the selected
    outputs enter the loss, so the others reach the backward as absent cotangents."""
    kw, rest = splat_scenes.to(sc, "cuda", dtype, means2D=means2D)
    out = fn(**kw, **rest)
    terms = [(o * c.to(dtype)).sum() for o, c, on in zip((out[0], out[2], out[3]), cots or _cot(sc, out[0].shape[0]), COTANGENTS[cot]) if on]
    grads = torch.autograd.grad(sum(terms), list(kw.values()), allow_unused=True)
    return out, {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(kw.items(), grads)}


def _reference(name, means2D="per_image", cot="all"):
    """The oracle in float64 and in fp32 on the device, computed once per (scene, means2D form, loss) and never modified."""
    key = (name, means2D, cot)
    if key not in _REF:
        sc = SCENES[name]
        out64, g64 = _run(gs_ref.rasterize, sc, torch.float64, means2D, cot)
        out32, g32 = _run(gs_ref.rasterize, sc, torch.float32, means2D, cot)
        e32 = {n: _rel(a, b) for n, a, b in zip(FWD, (out32[0], out32[2], out32[3]), (out64[0], out64[2], out64[3]))}
        e32.update({k: _rel(g32[k], g64[k]) for k in g64})
        _REF[key] = dict(out=out64, grads=g64, e32=e32)
    return _REF[key]


def _compare(name, out, grads, ref, tag=""):
    """Radii exactly; every forward tensor and every gradient against the float64 oracle under the module's bars."""
    assert torch.equal(out[1].long(), ref["out"][1].long()), (name, "radii", out[1].tolist()[:1], ref["out"][1].tolist()[:1])
    lines, failed = [], []
    pairs = [(n, a, b, 4.0, 2.0 ** -20) for n, a, b in zip(FWD, (out[0], out[2], out[3]), (ref["out"][0], ref["out"][2], ref["out"][3]))]
    pairs += [(k, grads[k], ref["grads"][k], 16.0, 2.0 ** -18) for k in ref["grads"]]
    for n, a, b, factor, floor in pairs:
        assert a.shape == b.shape, (name, n, a.shape, b.shape)
        err, e32 = _rel(a, b), ref["e32"][n]
        bar = 0.0 if float(b.detach().double().norm()) == 0 else max(factor * e32, floor)
        lines.append(f"[splat-edges] {name}{tag} {n}: e32 {e32:.2e} error {err:.2e} bar {bar:.2e}")
        if not err <= bar:
            failed.append(lines[-1])
    print("\n".join(lines))
    assert not failed, failed


def _oracle_counts(name):
    return splat_scenes.oracle(SCENES[name], device="cuda")[1]["counts"]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_matches_oracle(name):
    """Exact radii, forward and every gradient (per-image means2D included) under the bars, exactly-zero gradient rows for every
    (image, Gaussian) that contributes to no pixel, exactly-zero trailing SH gradients and third means2D component."""
    sc = SCENES[name]
    ref = _reference(name)
    out, grads = _run(splat.rasterize_gaussians, sc, torch.float32, "per_image")
    instances = splat.last_instance_count()
    _compare(name, out, grads, ref)
    counts = _oracle_counts(name)
    B, N = counts.shape
    for k, g in grads.items():
        if B > 1 and tuple(g.shape[:2]) != (B, N):
            continue                                            # an input shared by B > 1 images: its rows are sums over the images
        rows = g.reshape(B, N, -1)
        assert float(rows[counts == 0].abs().sum()) == 0.0, (name, k, "a Gaussian that contributes to no pixel has a non-zero gradient")
        if k in ("means3D", "scales", "rotations", "opacities") and bool((counts > 0).any()):
            assert float(rows[counts > 0].abs().sum(-1).min()) > 0.0, (name, k)
    assert float(grads["means2D"][..., 2].abs().max()) == 0.0
    if "shs" in grads:
        K = (sc["sh_degree"] + 1) ** 2
        assert float(grads["shs"][..., K:, :].abs().sum()) == 0.0                      # beyond the degree in use: written as zeros
        assert float(grads["shs"][ref["grads"]["shs"] == 0].abs().sum()) == 0.0        # and the clamped channels' coefficients
    if name == "no_instances":
        bg = sc["bg"].cuda()
        assert instances == 0
        assert torch.equal(out[0], bg[None, :, None, None].expand_as(out[0])) and not bool(out[2].detach().any()) and not bool(out[3].detach().any())
        assert all(float(g.abs().max()) == 0.0 for g in grads.values())


@pytest.mark.parametrize("cot", ["image", "alpha", "depth", "all"])
@pytest.mark.parametrize("name", ["alpha_clamp", "depth_tie"])
def test_cotangent_subsets(name, cot):
    """The loss on the image only, on alpha only, on depth only and on all three, each against the oracle under the same loss."""
    out, grads = _run(splat.rasterize_gaussians, SCENES[name], torch.float32, "per_image", cot)
    _compare(name, out, grads, _reference(name, "per_image", cot), tag=f" (loss on {cot})")


@pytest.mark.parametrize("name", ["ewa_clamp_x", "ewa_clamp_y", "ewa_clamp_xy", "depth_tie", "shared_b3"])
def test_means2d_forms(name):
    """means2D as [N, 3], as [B, N, 3] and absent: the outputs and the other gradients do not depend on it (bitwise), the [N, 3]
    gradient is the in-order sum over the images of the [B, N, 3] gradient (bitwise) and matches the oracle's."""
    sc = SCENES[name]
    out_b, g_b = _run(splat.rasterize_gaussians, sc, torch.float32, "per_image")
    out_s, g_s = _run(splat.rasterize_gaussians, sc, torch.float32, "shared")
    out_n, g_n = _run(splat.rasterize_gaussians, sc, torch.float32, None)
    for a, b, c in zip(out_b, out_s, out_n):
        assert torch.equal(a, b) and torch.equal(a, c)
    for k in g_n:
        assert torch.equal(g_n[k], g_b[k]) and torch.equal(g_n[k], g_s[k]), k
    acc = torch.zeros_like(g_s["means2D"])
    for b in range(g_b["means2D"].shape[0]):
        acc = acc + g_b["means2D"][b]
    assert g_s["means2D"].shape == acc.shape == (sc["inputs"]["means3D"].shape[-2], 3)
    assert torch.equal(g_s["means2D"], acc)
    assert float(g_s["means2D"][:, :2].abs().min()) > 0.0 and float(g_s["means2D"][:, 2].abs().max()) == 0.0
    _compare(name, out_s, g_s, _reference(name, "shared"), tag=" (means2D [N, 3])")


def test_drop_in_rasterizer_means2d_matches_oracle():
    """The single-image drop-in: ``means2D.grad`` after ``backward()`` is the oracle's dL / d p_proj.xy."""
    name = "ewa_clamp_xy"
    sc = SCENES[name]
    kw, rest = splat_scenes.to(sc, "cuda", torch.float32, means2D="shared")
    settings = splat.GaussianRasterizationSettings(
        image_height=sc["H"], image_width=sc["W"], tanfovx=float(rest["tanfovx"][0]), tanfovy=float(rest["tanfovy"][0]), bg=rest["bg"],
        scale_modifier=1.0, viewmatrix=rest["viewmatrix"][0], projmatrix=rest["projmatrix"][0], sh_degree=0, campos=rest["campos"][0],
        prefiltered=False)
    img, radii, dep, alp = splat.GaussianRasterizer(settings)(
        means3D=kw["means3D"], means2D=kw["means2D"], opacities=kw["opacities"], colors_precomp=kw["colors_precomp"], scales=kw["scales"],
        rotations=kw["rotations"])
    cot = _cot(sc, 1)
    ((img * cot[0][0]).sum() + (dep * cot[1][0]).sum() + (alp * cot[2][0]).sum()).backward()
    ref = _reference(name, "shared")
    _compare(name, (img[None], radii[None], dep[None], alp[None]), {k: v.grad for k, v in kw.items()}, ref, tag=" (GaussianRasterizer)")


@pytest.mark.parametrize("name", sorted(splat_scenes.SEAMS))
def test_batch_seam(name):
    """One tile holding 256, 257, 512, 513 or 700 Gaussians: alpha at every pixel is 1 - T of the oracle's blend mask, the backward is
    bit-identical between two runs, the batch nobody reaches (seam_dead_batch) writes exact zero rows, and the scene rendered twice
    in one call (the 20 x 20 render: four tiles, three of them partial) is bit-identical to the single-image call."""
    sc = SCENES[name]
    ref = _reference(name)
    out, grads = _run(splat.rasterize_gaussians, sc, torch.float32, "per_image")
    out2, grads2 = _run(splat.rasterize_gaussians, sc, torch.float32, "per_image")
    for a, b in zip(out, out2):
        assert torch.equal(a, b)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    pre, ex = splat_scenes.oracle(sc, device="cuda")
    pr = ex["pairs"][0]
    T = torch.where(pr["use"], 1 - pr["alpha"], torch.ones_like(pr["alpha"])).prod(1)
    err, bar = _rel(out[3].reshape(-1), 1 - T), max(4 * ref["e32"]["alpha"], 2.0 ** -20)
    print(f"[splat-edges] {name} alpha against 1 - T: error {err:.2e} bar {bar:.2e}")
    assert err <= bar
    dead = ex["counts"][0] == 0
    if name == "seam_dead_batch":
        assert int(dead.sum()) >= 700 - 512
    for k, g in grads.items():
        assert float(g.reshape(dead.shape[0], -1)[dead].abs().sum()) == 0.0, k
    twice = dict(sc, inputs={k: torch.stack([v, v]) for k, v in sc["inputs"].items()}, cam={k: torch.cat([v, v]) for k, v in sc["cam"].items()})
    out_t, grads_t = _run(splat.rasterize_gaussians, twice, torch.float32, "per_image", cots=[c.repeat(2, 1, 1, 1) for c in _cot(sc, 1)])
    for a, b in zip(out_t, out):
        assert torch.equal(a[0:1], b) and torch.equal(a[1:2], b)
    for k in grads:
        assert torch.equal(grads_t[k][0], grads[k].reshape(grads_t[k][0].shape)) and torch.equal(grads_t[k][1], grads_t[k][0]), k
