"""Constructed scenes for the splat rasterizer's parity tests (tests/test_splat_host.py, tests/test_splat_edges_gpu.py): each puts one
branch of csrc/splat.hip to work on at most 8 Gaussians (the seam scenes: up to 700), so a whole-tensor relative L2 is effectively per
Gaussian.  A scene is a dict: ``inputs`` (fp32 CPU tensors of rasterize_gaussians' per-Gaussian arguments), ``cam`` (viewmatrix,
projmatrix, campos, tanfovx, tanfovy), ``H``, ``W``, ``sh_degree``, ``bg``, ``branch`` (what it is for) and ``active(pre, ex)``, a
predicate on the float64 oracle's ``preprocess`` result and ``extras`` below that proves the branch is taken.  ``ordinary_counterparts``
rebuilds some of them with the branch idle (the predicate must then fail).  Everything is seeded; the seeds of the seam scenes were
searched on the CPU until ``gs_ref.decision_margins`` met ``gs_ref.MIN_MARGINS`` (tests/test_splat_host.py asserts it for every scene).

Anisotropic scales and non-axis rotations everywhere (no gradient tensor is analytically zero), centres off the pixel grid, and
non-square tanfov in more than half of the scenes."""
import math

import torch

from animate3d_amd import splat
from tests import gs_ref

QUATS = torch.tensor([[0.9, 0.2, -0.3, 0.25], [0.7, -0.4, 0.35, 0.45], [0.5, 0.6, 0.3, -0.55], [0.8, -0.15, -0.5, 0.3],
                      [0.6, 0.45, -0.25, -0.6], [0.95, 0.1, 0.2, -0.2], [0.4, -0.7, 0.5, 0.3], [0.75, 0.35, 0.4, 0.4]])
ANISO = torch.tensor([1.0, 0.75, 1.3])
COLORS = torch.tensor([[0.9, 0.3, 0.1], [0.2, 0.8, 0.4], [0.1, 0.4, 0.95], [0.7, 0.7, 0.2], [0.5, 0.1, 0.6], [0.3, 0.9, 0.8],
                       [0.85, 0.5, 0.5], [0.15, 0.25, 0.35]])
BG = torch.tensor([0.9, 0.2, 0.5])


def camera(eye=(3.5, 0.0, 0.0), fovx=40.0, fovy=40.0):
    """One camera at ``eye`` looking at the origin: dict of viewmatrix / projmatrix [1, 4, 4], campos [1, 3], tanfovx / tanfovy [1]."""
    c2w = gs_ref.look_at(eye)[None]
    fx, fy = torch.tensor([math.radians(fovx)]), torch.tensor([math.radians(fovy)])
    w2c, full, center = splat.get_cam_info_gaussian(c2w, fx, fy, 0.1, 100.0)
    return dict(viewmatrix=w2c, projmatrix=full, campos=center, tanfovx=torch.tan(fx / 2), tanfovy=torch.tan(fy / 2))


def cameras(*cams):
    return {k: torch.cat([c[k] for c in cams]) for k in cams[0]}


def place(cam, px, py, z, H, W, b=0):
    """World position whose pixel centre is (px, py) at view depth z for image b of ``cam`` (up to fp32 rounding)."""
    V = cam["viewmatrix"][b]
    vx = z * float(cam["tanfovx"][b]) * ((2 * px + 1) / W - 1)
    vy = z * float(cam["tanfovy"][b]) * ((2 * py + 1) / H - 1)
    return cam["campos"][b] + vx * V[:3, 0] + vy * V[:3, 1] + z * V[:3, 2]


def world_scale(cam, sigma_px, z, W, b=0):
    """Scale whose projection has about ``sigma_px`` pixels of standard deviation at depth z."""
    return sigma_px * z * 2 * float(cam["tanfovx"][b]) / W


def gaussians(cam, H, W, spec, b=0):
    """spec: rows of (px, py, depth, sigma_px, opacity) -> means, anisotropic scales, non-axis rotations, opacities, colours."""
    n = len(spec)
    means = torch.stack([place(cam, px, py, z, H, W, b) for px, py, z, _, _ in spec])
    scales = torch.stack([world_scale(cam, s, z, W, b) * ANISO.roll(i) for i, (_, _, z, s, _) in enumerate(spec)])
    opac = torch.tensor([[o] for *_, o in spec], dtype=torch.float32)
    return dict(means3D=means.float(), scales=scales.float(), rotations=QUATS[:n].clone(), opacities=opac, colors_precomp=COLORS[:n].clone())


def scene(name, branch, inputs, cam, H, W, active, sh_degree=0):
    return dict(name=name, branch=branch, inputs=inputs, cam=cam, H=H, W=W, sh_degree=sh_degree, bg=BG.clone(), active=active)


def to(sc, device, dtype, grad=True, means2D=None):
    """(per-Gaussian kwargs as leaves, remaining kwargs) of ``rasterize`` / ``rasterize_gaussians`` on ``device`` in ``dtype``;
    ``means2D``: None, "shared" ([N, 3] zeros) or "per_image" ([B, N, 3] zeros)."""
    kw = {k: v.to(device, dtype).detach().requires_grad_(grad) for k, v in sc["inputs"].items()}
    B, N = sc["cam"]["viewmatrix"].shape[0], sc["inputs"]["means3D"].shape[-2]
    if means2D is not None:
        kw["means2D"] = torch.zeros(*((B,) if means2D == "per_image" else ()), N, 3, device=device, dtype=dtype, requires_grad=grad)
    rest = {k: v.to(device, dtype) for k, v in sc["cam"].items()}
    rest.update(image_height=sc["H"], image_width=sc["W"], bg=sc["bg"].to(device, dtype), sh_degree=sc["sh_degree"])
    return kw, rest


def oracle(sc, device="cpu", dtype=torch.float64, counts=True):
    """(pre, extras) of the oracle on a scene: extras = dict(counts [B, N], use [B, H W, N], pairs (per image, gs_ref._pairs))."""
    kw, rest = to(sc, device, dtype, grad=False)
    with torch.no_grad():
        pre = gs_ref.preprocess(kw["means3D"], kw["scales"], kw["rotations"], kw["opacities"], kw.get("shs"), kw.get("colors_precomp"),
                                rest["viewmatrix"], rest["projmatrix"], rest["campos"], rest["tanfovx"], rest["tanfovy"], sc["H"], sc["W"],
                                1.0, sc["sh_degree"])
        if not counts:
            return pre, None
        B = rest["viewmatrix"].shape[0]
        pairs = [gs_ref._pairs(pre, b, sc["H"], sc["W"]) for b in range(B)]
        counts = gs_ref.composite(pre, sc["H"], sc["W"], rest["bg"], return_counts=True)[3]
        use = gs_ref.use_mask(pre, sc["H"], sc["W"])
    return pre, dict(counts=counts, use=use, pairs=pairs)


# ---- 1. EWA clamp: the centre at 1.5x the half-width (beyond 1.3 tanfov), sigma ~ 8 px so it still covers the 32 x 32 screen
def _ewa(axes, ordinary=False):
    H = W = 32
    cam = camera(fovx=50.0, fovy=36.0)
    px = (8.7 if ordinary else 40.2) if "x" in axes else 12.3          # ndc +1.5 is pixel 15.5 + 1.5 * 16
    py = (22.4 if ordinary else -8.8) if "y" in axes else 18.6         # ndc -1.5
    inputs = gaussians(cam, H, W, [(px, py, 3.4, 8.0, 0.8), (14.4, 15.7, 3.1, 5.0, 0.35)])

    def active(pre, ex):
        raw = pre["raw"]
        cx, cy = bool(raw["txtz"][0, 0].abs() > raw["limx"][0, 0]), bool(raw["tytz"][0, 0].abs() > raw["limy"][0, 0])
        return cx == ("x" in axes) and cy == ("y" in axes) and int(ex["counts"][0, 0]) > 0 and int(ex["counts"][0, 1]) > 0
    return scene(f"ewa_clamp_{axes}" + ("_ordinary" if ordinary else ""), "EWA clamp of t." + axes, inputs, cam, H, W, active)


# ---- 2. alpha clamp: o G > 0.99 on a block of pixels around two centres, below it on the rest of the tile; a translucent one behind
def _alpha_clamp(ordinary=False):
    H = W = 32
    cam = camera(fovx=40.0, fovy=40.0)
    o = (0.5, 0.5) if ordinary else (1.0, 0.995)
    inputs = gaussians(cam, H, W, [(8.31, 9.62, 3.2, 11.0, o[0]), (22.43, 21.27, 3.3, 12.0, o[1]), (15.6, 14.8, 3.6, 9.0, 0.3)])

    def active(pre, ex):
        pr = ex["pairs"][0]
        ok = True
        for k in (0, 1):                                        # blending order = Gaussian order here
            over, used = pr["oG"][:, k] > 0.99, pr["use"][:, k]
            ok = ok and int((over & used).sum()) >= 4 and int((~over & used).sum()) >= 100
        return ok and int(ex["counts"][0, 2]) > 0
    return scene("alpha_clamp" + ("_ordinary" if ordinary else ""), "0.99 alpha clamp", inputs, cam, H, W, active)


# ---- 3. / 4. spherical harmonics
def _sh_inputs(cam, H, W, spec, M, seed):
    inputs = gaussians(cam, H, W, spec)
    del inputs["colors_precomp"]
    g = torch.Generator().manual_seed(seed)
    inputs["shs"] = torch.randn(len(spec), M, 3, generator=g) * 0.25
    return inputs


SH_SPEC = [(7.3, 8.6, 3.2, 3.5, 0.7), (22.4, 9.7, 3.3, 4.0, 0.6), (9.6, 23.3, 3.4, 3.0, 0.8), (21.7, 22.4, 3.5, 4.5, 0.5)]


def _sh_clamp(ordinary=False):
    H = W = 32
    cam = camera(eye=(3.0, 1.2, 0.8), fovx=44.0, fovy=34.0)
    inputs = _sh_inputs(cam, H, W, SH_SPEC, 16, 5)
    want = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=torch.bool)
    inputs["shs"][:, 0] = torch.where(want & (not ordinary), torch.tensor(-4.0), torch.tensor(2.0))          # v ~ 0.5 -+ C0 * dc

    def active(pre, ex):
        return bool(torch.equal(pre["raw"]["sh_pre"][0] < 0, want)) and bool((ex["counts"][0] > 0).all())
    return scene("sh_clamp" + ("_ordinary" if ordinary else ""), "SH colour clamp, per channel", inputs, cam, H, W, active, sh_degree=3)


def _sh_deg(deg, M):
    H = W = 32
    cam = camera(eye=(2.8, -1.5, 1.1), fovx=38.0, fovy=46.0)
    inputs = _sh_inputs(cam, H, W, [(x + 0.13, y - 0.21, z, s, o) for x, y, z, s, o in SH_SPEC], M, 10 * deg + M)
    inputs["shs"][:, 0] += 1.0                                   # no colour clamp here: that is sh_clamp's
    K = (deg + 1) ** 2

    def active(pre, ex):
        return inputs["shs"].shape[1] == M >= K and bool((pre["raw"]["sh_pre"] > 0).all()) and bool((ex["counts"][0] > 0).all()) and \
            (M == K or float(inputs["shs"][:, K:].abs().min()) > 0)
    return scene(f"sh_deg{deg}_M{M}", f"SH degree {deg} with M = {M}", inputs, cam, H, W, active, sh_degree=deg)


# ---- 5. depth ties: two pairs with bit-identical means; image 1 holds the same Gaussians in another order
def _depth_tie(ordinary=False):
    H = W = 32
    cam1 = camera(fovx=48.0, fovy=38.0)
    cam = cameras(cam1, cam1)
    inp = gaussians(cam1, H, W, [(11.3, 12.6, 3.2, 5.0, 0.6), (11.3, 12.6, 3.2, 7.0, 0.6), (21.4, 19.7, 3.4, 6.0, 0.6),
                                 (21.4, 19.7, 3.4, 4.0, 0.6), (16.2, 15.1, 3.7, 9.0, 0.4)])
    if ordinary:
        inp["means3D"][1] += 0.05 * cam1["viewmatrix"][0, :3, 2]
        inp["means3D"][3] += 0.05 * cam1["viewmatrix"][0, :3, 2]
    order = torch.tensor([1, 0, 3, 2, 4])
    inputs = {k: torch.stack([v, v[order]]) for k, v in inp.items()}

    def active(pre, ex):
        z = pre["depth"]
        tied = all(float(z[b, i]) == float(z[b, i + 1]) for b in (0, 1) for i in (0, 2))
        return tied and bool((ex["counts"] > 0).all())
    return scene("depth_tie" + ("_ordinary" if ordinary else ""), "equal depths: the lower index blends first", inputs, cam, H, W, active)


# ---- 6. near plane
def _near_plane():
    H = W = 32
    cam = camera(eye=(1.0, 0.4, 0.3), fovx=40.0, fovy=52.0)
    zs = (0.2 * (1 + 2.0 ** -12), 0.2 * (1 - 2.0 ** -12), -1.0, 0.9)
    inputs = gaussians(cam, H, W, [(12.3, 13.6, zs[0], 3.0, 0.7), (18.4, 17.7, zs[1], 3.0, 0.7), (15.5, 15.5, 1.0, 3.0, 0.7),
                                   (20.6, 11.3, zs[3], 4.0, 0.5)])
    inputs["means3D"][2] = cam["campos"][0] - 1.0 * cam["viewmatrix"][0, :3, 2]
    inputs["scales"][1] = inputs["scales"][0].roll(1)
    inputs["scales"][2] = inputs["scales"][3]

    def active(pre, ex):
        z = pre["raw"]["z"][0]
        return bool(0.2 < z[0] < 0.2 * (1 + 2.0 ** -11)) and bool(0.2 * (1 - 2.0 ** -11) < z[1] < 0.2) and bool(z[2] < -0.9) and \
            pre["radii"][0].gt(0).tolist() == [True, False, False, True] and int(ex["counts"][0, 0]) > 0
    return scene("near_plane", "z cull at 0.2", inputs, cam, H, W, active)


# ---- 7. images smaller than a tile (and one just above): the same three Gaussians, placed in NDC
def _tiny(H, W):
    cam = camera(eye=(3.2, 0.6, -0.5), fovx=42.0, fovy=33.0)
    ndc = [(0.12, -0.23, 3.1, 0.7), (-0.31, 0.34, 3.3, 0.6), (0.41, 0.13, 3.5, 0.8)]
    spec = [(((x + 1) * 33 - 1) / 2, ((y + 1) * 33 - 1) / 2, z, 5.5, o) for x, y, z, o in ndc]
    inputs = gaussians(cam, 33, 33, spec)                       # world positions do not depend on the image size

    def active(pre, ex):
        return bool((ex["counts"][0] > 0).all())
    return scene(f"tiny_{H}x{W}", f"{H} x {W} image: most lanes of a tile are outside", inputs, cam, H, W, active)


# ---- 8. tile rectangle edges on 40 x 56 (4 x 3 tiles)
def _rect_edges():
    H, W = 40, 56
    cam = camera(eye=(3.3, -0.4, 0.7), fovx=47.0, fovy=35.0)
    inputs = gaussians(cam, H, W, [(24.3, 24.6, 3.1, 1.0, 0.7), (3.4, 5.7, 3.2, 2.5, 0.6), (54.2, 38.3, 3.3, 2.5, 0.8),
                                   (-30.4, 20.3, 3.4, 1.0, 0.7), (30.7, 14.2, 3.6, 3.0, 0.5)])

    def active(pre, ex):
        r, raw = pre["rect"][0].tolist(), pre["raw"]["rect_raw"][0]
        return r[0] == [1, 2, 1, 2] and r[1][0] == 0 and r[1][2] == 0 and float(raw[1, 0]) < 0 and float(raw[1, 2]) < 0 and \
            r[2][1] == 4 and r[2][3] == 3 and float(raw[2, 1]) > 4 and float(raw[2, 3]) > 3 and r[3][0] == r[3][1] == 0 and \
            pre["radii"][0].gt(0).tolist() == [True, True, True, False, True] and bool((ex["counts"][0, [0, 1, 2, 4]] > 0).all())
    return scene("rect_edges", "tile rectangles: one tile, c - r < 0, clipped right / bottom, empty", inputs, cam, H, W, active)


# ---- 9. / 10. nothing to draw
def _culled_means(cam, b=0):
    """Behind the camera, off to the left with an empty rectangle, and just behind the near plane."""
    V, c = cam["viewmatrix"][b], cam["campos"][b]
    return torch.stack([c - 1.3 * V[:3, 2], place(cam, -40.3, 10.2, 3.0, 32, 32, b), c + 0.15 * V[:3, 2] + 0.01 * V[:3, 0]])


def _no_instances():
    H = W = 32
    cam = camera(fovx=40.0, fovy=30.0)
    inputs = gaussians(cam, H, W, [(10.3, 11.6, 3.0, 1.0, 0.7), (12.4, 9.7, 3.0, 1.0, 0.6), (15.2, 18.3, 3.0, 1.0, 0.5)])
    inputs["means3D"] = _culled_means(cam)

    def active(pre, ex):
        return not bool(pre["visible"].any()) and int(ex["counts"].sum()) == 0
    return scene("no_instances", "L == 0: nothing visible", inputs, cam, H, W, active)


def _empty_middle_image():
    H, W = 40, 56
    cam = cameras(camera(fovx=47.0, fovy=35.0), camera(eye=(0.0, 3.5, 0.5), fovx=40.0, fovy=30.0), camera(eye=(-2.0, -2.5, 1.0), fovx=50.0, fovy=38.0))
    spec = [(24.3, 22.6, 3.1, 1.6, 0.7), (30.4, 18.7, 3.3, 1.9, 0.6), (27.2, 25.3, 3.5, 1.4, 0.8)]        # middle tiles only
    per = [gaussians(cam, H, W, spec, b) for b in range(3)]
    inputs = {k: torch.stack([p[k] for p in per]) for k in per[0]}
    inputs["means3D"][1] = _culled_means(cam, 1)
    inputs["means3D"][1, 1] = cam["campos"][1] - 2.0 * cam["viewmatrix"][1, :3, 2]
    inputs["means3D"][1, 2] = cam["campos"][1] - 0.7 * cam["viewmatrix"][1, :3, 2]

    def active(pre, ex):
        rect = pre["rect"]
        edge = all((int(rect[b, i, 0]) >= 1 or int(rect[b, i, 2]) >= 1) and (int(rect[b, i, 1]) <= 3 or int(rect[b, i, 3]) <= 2)
                   for b in (0, 2) for i in range(3))                # tile (0, 0) and tile (3, 2) stay empty
        behind = bool((pre["raw"]["z"][1] < 0).all()) and not bool(pre["visible"][1].any())
        return edge and behind and bool((ex["counts"][[0, 2]] > 0).all())
    return scene("empty_middle_image", "image 1 of 3 has no instance; first and last tile of the others are empty", inputs, cam, H, W, active)


# ---- 12. one shared [N, ...] scene seen by three cameras (means2D [N, 3] summed over the images)
def _shared_b3():
    H, W = 24, 40
    cam = cameras(camera(fovx=47.0, fovy=35.0), camera(eye=(0.3, 3.4, 0.6), fovx=40.0, fovy=30.0), camera(eye=(-2.1, -2.4, 1.2), fovx=50.0, fovy=38.0))
    g = torch.Generator().manual_seed(3)
    n = 5
    inputs = dict(means3D=torch.randn(n, 3, generator=g) * 0.25, scales=(0.08 + 0.1 * torch.rand(n, 1, generator=g)) * ANISO,
                  rotations=QUATS[:n].clone(), opacities=0.4 + 0.4 * torch.rand(n, 1, generator=g), colors_precomp=COLORS[:n].clone())

    def active(pre, ex):
        return bool((ex["counts"] > 0).all())
    return scene("shared_b3", "inputs shared by three images", inputs, cam, H, W, active)


# ---- 13. the 256-Gaussian batch seam of the render kernels: one 16 x 16 tile holding N Gaussians on a depth grid
SEAM_SEEDS = {"seam_256": 0, "seam_257": 0, "seam_512": 4, "seam_513": 1, "seam_dead_batch": 0, "seam_513_20x20": 12}


def _seam(name, N, opacity, H=16, W=16, check=None):
    cam = camera(eye=(3.5, 0.0, 0.0), fovx=40.0, fovy=40.0)
    g = torch.Generator().manual_seed(SEAM_SEEDS[name])
    perm = torch.randperm(N, generator=g)
    means = torch.stack([0.3 - 0.002 * perm.float(), 0.08 * torch.randn(N, generator=g), 0.08 * torch.randn(N, generator=g)], 1)
    scales = 2.0 + torch.rand(N, 3, generator=g)
    rots = torch.randn(N, 4, generator=g)
    opac = opacity[0] + (opacity[1] - opacity[0]) * torch.rand(N, 1, generator=g)
    inputs = dict(means3D=means, scales=scales, rotations=rots, opacities=opac, colors_precomp=torch.rand(N, 3, generator=g))
    sc = scene(name, f"{N} Gaussians in one tile: the 256-Gaussian batches of the render kernels", inputs, cam, H, W, None)
    for _ in range(16):            # among hundreds of radii some 3 sqrt(lambda_max) sits next to an integer: grow those Gaussians by 0.3 %
        r3 = oracle(sc, counts=False)[0]["raw"]["r3"][0]
        close = (r3 - torch.round(r3)).abs() < 2.0 ** -7
        if not bool(close.any()):
            break
        inputs["scales"][close] *= 1.003

    def active(pre, ex):
        pr = ex["pairs"][0]
        if not bool(pre["visible"].all()) or not bool(pr["valid"].all()):        # every pixel sees every Gaussian above 1/255
            return False
        n_contrib = (pr["use"] * torch.arange(1, N + 1)).amax(1)                 # the forward's last contributor, per pixel
        return check(n_contrib, ex["counts"][0][pr["g"]])
    sc["active"] = active
    return sc


# Opacity ranges.  DENSE: every pixel stops between contributors 340 and 460.  TRANSLUCENT never stops (T stays above 0.04 after 257
# Gaussians) and keeps alpha >= 0.0056 at the tile's corners (G >= 0.7 there), clear of 1/255 = 0.0039: at opacities of 0.004 - 0.006
# the 65 000 pairs of the tile straddle 1/255 so densely that no seed keeps the alpha_skip margin, and the corner pixels would skip
# the last Gaussian, so their n_contrib would not be N.
TRANSLUCENT, DENSE = (0.008, 0.012), (0.020, 0.032)


def _seams():
    full = lambda N: (lambda n_contrib, counts: bool((n_contrib == N).all()) and int(counts.min()) == 256)
    # the stop falls inside the second batch at every pixel of seam_512 / 513, and some pixel's last contributor is past position 256
    stops = lambda N: (lambda n_contrib, counts: 256 < int(n_contrib.min()) and int(n_contrib.max()) < N and int(counts[N - 1]) == 0)
    dead = lambda n_contrib, counts: int(n_contrib.max()) <= 512 and int(counts[512:].max()) == 0 and int(counts[:256].min()) > 0
    return [_seam("seam_256", 256, TRANSLUCENT, check=full(256)), _seam("seam_257", 257, TRANSLUCENT, check=full(257)),
            _seam("seam_512", 512, DENSE, check=stops(512)), _seam("seam_513", 513, DENSE, check=stops(513)),
            _seam("seam_dead_batch", 700, DENSE, check=dead),
            _seam("seam_513_20x20", 513, DENSE, H=20, W=20, check=lambda n_contrib, counts: 256 < int(n_contrib.min()))]


def build():
    scenes = [_ewa("x"), _ewa("y"), _ewa("xy"), _alpha_clamp(), _sh_clamp(), _sh_deg(1, 4), _sh_deg(1, 16), _sh_deg(2, 9), _sh_deg(2, 16),
              _depth_tie(), _near_plane(), _tiny(1, 1), _tiny(5, 7), _tiny(16, 16), _tiny(17, 33), _rect_edges(), _no_instances(),
              _empty_middle_image(), _shared_b3()] + _seams()
    return {s["name"]: s for s in scenes}


def ordinary_counterparts():
    """scene name -> the same scene with its branch idle: centre on-screen, opacity 0.5, SH coefficients positive, depths apart."""
    return {"ewa_clamp_x": _ewa("x", True), "ewa_clamp_y": _ewa("y", True), "ewa_clamp_xy": _ewa("xy", True),
            "alpha_clamp": _alpha_clamp(True), "sh_clamp": _sh_clamp(True), "depth_tie": _depth_tie(True)}


SCENES = build()
SMALL = [n for n in SCENES if not n.startswith("seam_")]
SEAMS = [n for n in SCENES if n.startswith("seam_")]
