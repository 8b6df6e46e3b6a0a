"""The ARAP kernels (csrc/arap.hip) against the float64 restatement tests/arap_ref.py, their bitwise guarantees, the reference's golden
through the drop-ins, and the chain deformation field -> ARAP -> backward, alone and inside the config-5 SDS step.

k-NN: ``nn_idx`` must EQUAL the float64 oracle's for every point; arap_ref.make_points draws again every point with a near-tie or a
distance at the radius cut, duplicates stay in (they tie exactly on both sides and the index decides).
Energy tolerance, the project's existing bar: per compared tensor, e32 = relative L2 of the float32 restatement against the float64 one on
the same inputs; the kernels' relative L2 against float64 must be at most max(4 e32, 16 * 2^-24).  Golden bars: tests/test_arap_host.py."""
import math
import os

import numpy as np
import pytest
import torch

from animate3d_amd import arap, deform4d, splat
from tests import arap_ref, deform_ref, gs_ref
from tests.test_arap_host import GOLDEN, ROT_BAR, SUM_BAR

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _check_graph(pts64, idx64, dist64, radius, tag, Ks=(1, 3, 10, 16), least_edge_num=3, exact=False):
    """``knn_graph`` for every K of ``Ks``, without a radius and with ``radius``: ``nn_idx`` equal to the float64 oracle's, the distances
    within 8 * 2^-24 of it (``exact``: equal to it)."""
    x = pts64.float().cuda()
    for K in Ks:
        for r in dict.fromkeys((None, radius)):
            got_i, got_d = arap.knn_graph(x, K, radius=r, least_edge_num=least_edge_num)
            want_i, want_d = arap_ref.mask_radius(idx64[:, :K], dist64[:, :K], r, least_edge_num)
            torch.cuda.synchronize()
            wrong = int((got_i.long().cpu() != want_i.cpu()).any(1).sum())
            fin = torch.isfinite(want_d.cpu())
            assert torch.equal(torch.isfinite(got_d.cpu()), fin)
            err = float(((got_d.double().cpu() - want_d.cpu())[fin].abs() / want_d.cpu()[fin].clamp_min(1e-300)).max()) if fin.any() else 0.0
            print(f"[arap knn {tag} K {K} radius {r} least {least_edge_num}] points with a wrong neighbour {wrong} / {len(x)}; "
                  f"cut {int((want_i < 0).sum())}; distance max rel err {err:.3e}")
            assert wrong == 0 and got_i.dtype == torch.int32 and err <= 8 * 2.0 ** -24
            assert got_i.shape == got_d.shape == (len(x), K) and got_d.dtype == torch.float32
            assert not exact or torch.equal(got_d.double().cpu(), want_d.cpu())
            assert bool((got_i.cpu() != torch.arange(len(x))[:, None]).all())            # never its own neighbour


def test_knn_equals_float64_oracle_20k_cpu():
    pts, rounds, idx, dist = arap_ref.make_points(20000, 16, 5, radius=0.03)
    assert int((dist[:, 0] == 0).sum()) == 11                                           # the duplicates
    _check_graph(pts, idx, dist, 0.03, f"20k cpu oracle, {rounds} rounds")


def test_knn_equals_float64_oracle_100k_gpu():
    pts, rounds, idx, dist = arap_ref.make_points(100000, 16, 6, radius=0.018, device="cuda")
    assert int((dist[:, 0] == 0).sum()) == 11
    _check_graph(pts.cpu(), idx.cpu(), dist.cpu(), 0.018, f"100k gpu oracle, {rounds} rounds")


def test_knn_limits():
    x = torch.rand(50, 3, device="cuda")
    for K in (0, 17):
        with pytest.raises(NotImplementedError):
            arap.knn_graph(x, K)
    with pytest.raises(ValueError):
        arap.knn_graph(x[:16], 16)
    i, d = arap.knn_graph(x[:17], 16)                                                   # Nv = K + 1: everybody else
    assert torch.equal(i.long().sort(1).values.cpu(), torch.stack([torch.tensor([j for j in range(17) if j != v]) for v in range(17)]))


def _run_hip(scene, weighted, need_source_grad=True, strided=False):
    src = scene["source"].float().cuda().requires_grad_(need_source_grad)
    tgt = scene["targets"].float().cuda()
    if strided:                                                                         # every second image of a [2 F, Nv, 3] batch
        big = torch.randn(2 * tgt.shape[0], *tgt.shape[1:], device="cuda")
        big[::2] = tgt
        big.requires_grad_(True)
        view = big[::2]
        assert not view.is_contiguous()
    else:
        big = view = tgt.requires_grad_(True)
    w = scene["weight"].float().cuda() if weighted else None
    loss, R = arap.arap_energy(src, view, scene["nn_idx"].cuda(), weight=w, sample_idx=scene["sample_idx"].cuda(), return_rotations=True)
    grads = torch.autograd.grad(loss, [big] + ([src] if need_source_grad else []))
    d_t = grads[0][::2] if strided else grads[0]
    return dict(loss=loss.detach(), R=R, d_targets=d_t, d_source=grads[1] if need_source_grad else None), grads[0]


def check_against_float64(tag, got, r64, r32, keys=("loss", "R", "d_targets", "d_source"), floor_only=False):
    """The acceptance rule of the energy tests.  The float32 and the float64 restatement take every unchanged flag alike, so that e32, the
    relative L2 of the float32 one against the float64 one, measures rounding only; per tensor of ``keys`` the kernels' relative L2 against
    float64 is at most max(4 e32, FLOOR), with ``floor_only`` at most FLOOR: an fp64 result rounded once to fp32.  A tensor the run did
    not ask for (``d_source`` without ``source.requires_grad``) is None on both sides.  Returns the worst error as a fraction of its bar."""
    assert torch.equal(r64["unchanged"], r32["unchanged"])                              # e32 below measures rounding only
    failures, worst = [], 0.0
    for k in keys:
        if r64[k] is None:
            assert got[k] is None, k
            continue
        e32, err = _rel(r32[k], r64[k]), _rel(got[k], r64[k])
        bar = FLOOR if floor_only else max(4 * e32, FLOOR)
        worst = max(worst, err / bar)
        print(f"[arap {tag}] {k}: e32 {e32:.3e} kernel {err:.3e} bar {bar:.3e}")
        if not err <= bar:
            failures.append((k, e32, err, bar))
    assert not failures, failures
    return worst


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(arap_ref.SCENES))
def test_energy_and_gradients_against_float64(name, weighted):
    scene = arap_ref.named_scene(name)                                                  # tests/test_arap_host.py checks the same scenes on the CPU
    r64, r32 = arap_ref.run(scene, torch.float64, weighted=weighted), arap_ref.run(scene, torch.float32, weighted=weighted)
    got, _ = _run_hip(scene, weighted)
    torch.cuda.synchronize()
    assert got["loss"].dim() == 0 and got["loss"].dtype == torch.float32 and got["R"].shape == r64["R"].shape
    check_against_float64(f"{name} w{int(weighted)}", got, r64, r32)
    eye = torch.eye(3, device="cuda")
    assert torch.equal(got["R"][:2], eye.expand_as(got["R"][:2]))                       # the unchanged rule: exactly the identity


def test_backward_is_bitwise_reproducible_zero_where_untouched_and_stride_blind():
    scene = arap_ref.named_scene("gpu_parity_k3")
    a, _ = _run_hip(scene, True)
    b, _ = _run_hip(scene, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    touched = torch.zeros(scene["source"].shape[0], dtype=torch.bool)
    s = scene["sample_idx"]
    touched[s] = True
    nb = scene["nn_idx"][s]
    touched[nb[nb >= 0]] = True
    assert 0 < int(touched.sum()) < len(touched)
    assert float(a["d_targets"][:, ~touched.cuda()].abs().max()) == 0.0 and float(a["d_source"][~touched.cuda()].abs().max()) == 0.0
    assert float(a["d_targets"][2:, touched.cuda()].abs().max()) > 0.0
    c, full = _run_hip(scene, True, strided=True)
    for k in a:
        assert torch.equal(a[k], c[k]), k
    assert float(full[1::2].abs().max()) == 0.0                                          # the images the view skips get no gradient
    d, _ = _run_hip(scene, True, need_source_grad=False)
    assert d["d_source"] is None and torch.equal(d["d_targets"], a["d_targets"])
    src, tgt = scene["source"].float().cuda(), scene["targets"].float().cuda().requires_grad_(True)
    loss = arap.arap_energy(src, tgt, scene["nn_idx"].cuda(), sample_idx=scene["sample_idx"].cuda())
    (g2,) = torch.autograd.grad(loss * 12.0, [tgt])
    (g1,) = torch.autograd.grad(arap.arap_energy(src, tgt, scene["nn_idx"].cuda(), sample_idx=scene["sample_idx"].cuda()), [tgt])
    assert _rel(g2, g1 * 12.0) <= 2.0 ** -23
    with pytest.raises(ValueError):
        arap.arap_energy(src, tgt.detach().transpose(1, 2).contiguous().transpose(1, 2), scene["nn_idx"].cuda())


def test_default_sample_is_every_vertex_or_a_device_draw():
    scene = arap_ref.named_scene("gpu_parity_k8")
    src, tgt, nn = scene["source"].float().cuda()[:400], scene["targets"].float().cuda()[:, :400], scene["nn_idx"].cuda()[:400]
    nn = torch.where(nn < 400, nn, torch.full_like(nn, -1))
    tgt = tgt.contiguous()
    every = arap.arap_energy(src, tgt, nn, sample_idx=torch.arange(400, device="cuda"))
    assert torch.equal(arap.arap_energy(src, tgt, nn), every)                           # Nv <= sample_num
    gen = torch.Generator(device="cuda").manual_seed(3)
    l1, R1 = arap.arap_energy(src, tgt, nn, sample_num=64, generator=gen, return_rotations=True)
    gen.manual_seed(3)
    idx = torch.randint(400, (64,), generator=gen, device="cuda")
    l2, R2 = arap.arap_energy(src, tgt, nn, sample_idx=idx, return_rotations=True)
    assert R1.shape == (tgt.shape[0], 64, 3, 3) and torch.equal(l1, l2) and torch.equal(R1, R2)
    assert float(arap.arap_energy(src, tgt[:0], nn)) == 0.0


@pytest.mark.parametrize("tag,variant", [("k3", "unit"), ("k3", "weighted"), ("k8", "unit")])
def test_golden_through_the_drop_ins(tag, variant):
    g = np.load(GOLDEN)
    K, radius = int(g[f"{tag}_K"]), float(g[f"{tag}_radius"])
    ii, jj, nn, weight = arap.cal_connectivity_from_points(torch.from_numpy(g[f"{tag}_points"]).cuda(), radius=radius, K=K)
    for got, key in ((ii, "ii"), (jj, "jj"), (nn, "nn")):
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(g[f"{tag}_{key}"]).long()), key
    want_w = torch.from_numpy(g[f"{tag}_weight"])
    assert torch.equal(torch.isnan(weight).cpu(), torch.isnan(want_w))                  # the reference's NaN rows, as written
    fin = ~torch.isnan(want_w)
    assert fin.any() and float((weight.cpu()[fin] - want_w[fin]).abs().max()) <= 1e-6
    nodes = torch.from_numpy(g["nodes"]).cuda().requires_grad_(True)
    err, R = arap.cal_arap_error(nodes, ii, jj, nn, K=K, weight=weight if variant == "weighted" else None, sample_num=int(g["sample_num"]),
                                 sample_idx=torch.from_numpy(g["sample_idx"]).cuda(), return_rotations=True)
    (grad,) = torch.autograd.grad(err, [nodes])
    errs = {"R": _rel(R, torch.from_numpy(g[f"{tag}_{variant}_rotations"])), "loss": _rel(err, torch.from_numpy(g[f"{tag}_{variant}_error"])),
            "grad": _rel(grad, torch.from_numpy(g[f"{tag}_{variant}_grad"]))}
    print(f"[arap golden on the GPU {tag} {variant}] " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["R"] <= ROT_BAR and errs["loss"] <= SUM_BAR and errs["grad"] <= SUM_BAR, errs
    drawn = arap.cal_arap_error(nodes.detach(), ii, jj, nn, K=K, sample_num=int(g["sample_num"]))      # the draw on the device
    assert torch.isfinite(drawn) and float(drawn) > 0.0


def test_graph_is_cached_and_follows_in_place_changes():
    p1, p2 = arap_ref.make_points(5000, 3, 8)[0], arap_ref.make_points(5000, 3, 9)[0]
    xyz = p1.float().cuda()
    graph = arap.ArapGraph(xyz, K=3, radius=0.01)
    first = graph.nn_idx
    assert graph.refresh(xyz) is graph and graph.nn_idx is first and graph.builds == 1
    assert torch.equal(first.long().cpu(), arap_ref.knn_bruteforce(p1, 3)[0])
    xyz.copy_(p2)                                                                       # in place: same tensor, same storage, a new version
    assert not graph.matches(xyz)
    graph.refresh(xyz)
    assert graph.builds == 2 and graph.nn_idx is not first and graph.matches(xyz)
    assert torch.equal(graph.nn_idx.long().cpu(), arap_ref.knn_bruteforce(p2, 3)[0]) and not torch.equal(graph.nn_idx, first)


def _field_leaves(s, names):
    out = {}
    for si, g in enumerate(s["grids"]):
        for pi, p in enumerate(g):
            out[f"grids.{si}.{pi}"] = p
    for n in names:
        out[f"{n}.layers.0.weight"], out[f"{n}.layers.2.weight"] = s["nets"][n]
    return out


def test_chain_from_the_deformation_field_against_float64():
    """deform_gaussians -> arap_energy -> backward: the plane and MLP gradients against deform_ref.deform + arap_ref in float64.

    The energy does not change when a frame is translated, so the gradient of ``global_trans_network`` is zero in exact arithmetic: every
    format returns only its own cancellation residue there, and a relative error between two residues says nothing (float32 against
    float64: 4e8).  Such a tensor is recognised from float64 alone: ``scale`` is the same backward pass with ``|d loss / d means|`` as
    the cotangent of the means, the size of the sums without the cancellation between vertices, and a gradient below 1e-9 of it (2^-24
    is 6e-8: no fp32 term could carry it; float64 residues are near 1e-13) is zero by cancellation.  There the kernels' residue must be at
    most the floor of the bar, 16 * 2^-24, times ``scale``; everywhere else the bar is the usual one."""
    scene = deform_ref.named_scene("gpu_parity", True)
    names = deform_ref.LOCAL + deform_ref.GLOBAL
    N = scene["xyz"].shape[0]
    nn_idx, _ = arap_ref.knn_bruteforce(scene["xyz"].double(), 3)
    sample_idx = torch.randint(N, (512,), generator=torch.Generator().manual_seed(4))
    F_ = 4

    def ref(dtype):
        s = deform_ref.cast(scene, dtype)
        leaves = _field_leaves(s, names)
        for t in leaves.values():
            t.requires_grad_(True)
        means, _, _ = deform_ref.deform(s["xyz"], s["scaling"], s["rotation"], s["timestamps"], s["grids"], {n: s["nets"][n] for n in names},
                                        use_global_trans=True)
        loss, R, un = arap_ref.energy(s["xyz"], means[:F_], nn_idx, None, sample_idx)
        (d_means,) = torch.autograd.grad(loss, [means], retain_graph=True)
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True, retain_graph=True)
        scale = torch.autograd.grad((means * d_means.abs()).sum(), list(leaves.values()), allow_unused=True)
        fill = lambda gs: {k: (torch.zeros_like(t) if g is None else g) for (k, t), g in zip(leaves.items(), gs)}
        return loss.detach(), fill(grads), un, fill(scale)
    l64, g64, un64, scale64 = ref(torch.float64)
    l32, g32, un32, _ = ref(torch.float32)
    assert torch.equal(un64, un32) and bool(un64[1].all()) and not bool(un64[0].any())    # timestamp -1 is the second frame: means = xyz
    s = deform_ref.cast(scene, torch.float32, "cuda")
    leaves = _field_leaves(s, names)
    for t in leaves.values():
        t.requires_grad_(True)
    means, _, _ = deform4d.deform_gaussians(s["xyz"], s["scaling"], s["rotation"], s["timestamps"], s["grids"], {n: s["nets"][n] for n in names},
                                            use_global_trans=True)
    loss = arap.arap_energy(s["xyz"], means[:F_], nn_idx.cuda(), sample_idx=sample_idx.cuda())
    grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)))
    torch.cuda.synchronize()
    failures = []
    for k, r64, r32, got in [("loss", l64, l32, loss)] + [(k, g64[k], g32[k], grads[k]) for k in g64]:
        if float(r64.abs().max()) == 0.0:
            print(f"[arap chain] {k}: reference is zero")
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        if k in scale64 and float(r64.norm()) <= 1e-9 * float(scale64[k].norm()):
            sc, res = float(scale64[k].norm()), float(got.double().norm())
            print(f"[arap chain] {k}: zero by cancellation (float64 {float(r64.norm()):.3e}, float32 {float(r32.norm()):.3e}, scale {sc:.3e}); "
                  f"kernel {res:.3e} bar {FLOOR * sc:.3e}")
            if not res <= FLOOR * sc:
                failures.append((k, res, FLOOR * sc))
            continue
        e32, err = _rel(r32, r64), _rel(got, r64)
        bar = max(4 * e32, FLOOR)
        print(f"[arap chain] {k}: e32 {e32:.3e} kernel {err:.3e} bar {bar:.3e}")
        if not err <= bar:
            failures.append((k, e32, err, bar))
    assert not failures, failures


def test_sds_config5_step_with_the_arap_term_gpu():
    """The config-5 SDS step from the deformation field (test_sds_config5_step_from_deformation_field_gpu) plus 12 * arap: finite gradients
    that differ from the run without the term.  The SDS step is not bit-reproducible from run to run, so the printed difference of the two
    runs against 12 x the term's own gradient carries that too; what is asserted about the term's reach is taken from its own backward."""
    from animate3d_amd.config import UNetConfig
    from animate3d_amd.sds import sds_guidance_loss
    from animate3d_amd.unet import MVUNetMotionModel
    from animate3d_amd.vae import AutoencoderKLEncoder
    from oracle import vae_ref as R
    n, f, H, W, N, dt = 4, 16, 256, 256, 20000, torch.float16
    enc = AutoencoderKLEncoder(device="cuda")
    enc.load_state_dict(R.init_synthetic_weights(R.VAEEncoderRef(), seed=1).state_dict(), strict=True)
    enc = enc.to(dt).eval()
    unet = MVUNetMotionModel(UNetConfig(), num_views=n, device="cuda")
    unet.init_synthetic(seed=0)
    unet = unet.to(dt).eval()
    g = torch.Generator().manual_seed(12)
    xyz = (torch.randn(N, 3, generator=g) * 0.6).cuda()
    scaling = (torch.rand(N, 3, generator=g) * 2.0 - 4.2).cuda()
    rotation = torch.randn(N, 4, generator=g).cuda()
    opac = (torch.sigmoid(torch.randn(N, 1, generator=g) * 1.5) * 0.1).cuda()
    shs = (torch.randn(N, 16, 3, generator=g) * 0.3).cuda()
    field = deform4d.HexPlaneDeformation(use_global_trans=True).cuda()
    with torch.no_grad():                                       # the reference's zero last layers give zero gradient to everything before them
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.normal_(0.0, 0.02, generator=None)
    c2w_v = torch.stack([gs_ref.look_at((3.5 * math.cos(a), 3.5 * math.sin(a), 0.0)) for a in (0.0, math.pi / 2, math.pi, 1.5 * math.pi)])
    c2w = c2w_v[:, None].expand(n, f, 4, 4).reshape(n * f, 4, 4).cuda()
    fovy = torch.full((n * f,), math.radians(40.0), device="cuda")
    w2c, full, center = splat.get_cam_info_gaussian(c2w, fovy, fovy, 0.1, 100.0)
    ts = torch.linspace(-1, 1, f).cuda()
    i2t = (torch.arange(n * f) % f).cuda()
    text = torch.randn(2 * n, 77, 768, generator=g).cuda()
    emb = torch.randn(n, 1024, generator=g).cuda()
    vae_noise = torch.randn(n * f, 4, 32, 32, generator=g).cuda()
    graph = arap.ArapGraph(xyz, K=3, radius=0.01)
    sample_idx = torch.randint(N, (512,), generator=torch.Generator(device="cuda").manual_seed(6), device="cuda")

    def step(lambda_arap):
        for p in field.parameters():
            p.grad = None
        means, scales, rots = field(xyz, scaling, rotation, ts, i2t)
        img, _, _, _ = splat.rasterize_gaussians(means, scales, rots, opac, shs=shs, viewmatrix=w2c, projmatrix=full, campos=center,
                                                 tanfovx=torch.tan(fovy / 2), tanfovy=torch.tan(fovy / 2), image_height=H, image_width=W,
                                                 bg=torch.ones(3, device="cuda"), sh_degree=3)
        loss, _ = sds_guidance_loss(enc, unet, img.permute(0, 2, 3, 1), torch.tensor([500], device="cuda"), text, emb, c2w, n_view=n, n_frame=f,
                                    weights_dtype=dt, vae_noise=vae_noise, generator=torch.Generator(device="cuda").manual_seed(2))
        term = None
        if lambda_arap:
            term = arap.arap_energy(xyz, means[:f], graph.refresh(xyz).nn_idx, sample_idx=sample_idx)      # the first view's f frames
            loss = loss + lambda_arap * term
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        return {k: p.grad.clone() for k, p in field.named_parameters()}, term
    plain, _ = step(0.0)
    with_term, term = step(12.0)
    assert graph.builds == 1 and torch.isfinite(term) and float(term.detach()) > 0.0
    for p in field.parameters():                                                        # the term alone, through the field only
        p.grad = None
    means, _, _ = field(xyz, scaling, rotation, ts, i2t)
    arap.arap_energy(xyz, means[:f], graph.refresh(xyz).nn_idx, sample_idx=sample_idx).backward()
    alone = {k: p.grad for k, p in field.named_parameters()}
    differs = 0
    for k in plain:
        assert torch.isfinite(with_term[k]).all() and float(with_term[k].abs().max()) > 0.0, k
        if k.startswith(("delta_rot_network", "delta_scaling_network")):                # those two feed rotations and scales only
            assert alone[k] is None or float(alone[k].abs().max()) == 0.0, k
            print(f"[sds config 5 + 12 arap] {k}: the term does not reach it; |grad| max {with_term[k].abs().max().item():.3e}")
            continue
        assert float(alone[k].abs().max()) > 0.0 and not torch.equal(plain[k], with_term[k]), k
        differs += 1
        print(f"[sds config 5 + 12 arap] {k}: |grad| max {with_term[k].abs().max().item():.3e} (without the term {plain[k].abs().max().item():.3e}); "
              f"difference against 12 x the term's own gradient: rel {_rel(with_term[k] - plain[k], 12.0 * alone[k]):.3e}")
    print(f"[sds config 5 + 12 arap] arap {float(term.detach()):.4e}; {differs} of {len(plain)} parameter gradients differ")
    assert differs == len(plain) - 4
