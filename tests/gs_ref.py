"""Dense plain-torch restatement of the splat rasterizer's contract (animate3d_amd/splat.py docstring): every pixel against every
Gaussian, stably sorted by depth, with the same cull, tile-rectangle, skip, clamp and stop rules.  Its autograd is the gradient
reference of the GPU tests.  Runs in the dtype of its inputs (the tests use float64) on any device."""
import math

import torch

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)


def sh_basis(deg, d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = [torch.full_like(x, SH_C0)]
    if deg >= 1:
        out += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if deg >= 2:
        xx, yy, zz = x * x, y * y, z * z
        out += [SH_C2[0] * x * y, SH_C2[1] * y * z, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * x * z, SH_C2[4] * (xx - yy)]
    if deg >= 3:
        out += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * x * y * z, SH_C3[2] * y * (4 * zz - xx - yy), SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3 * yy)]
    return torch.stack(out, -1)


def quat_to_rot(q):
    q = q / q.norm(dim=-1, keepdim=True)
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(*q.shape[:-1], 3, 3)


def preprocess(means3D, scales, rotations, opacities, shs, colors_precomp, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W,
               scale_modifier=1.0, sh_degree=0, means2D=None):
    """Per (image, Gaussian): dict of xy [B, N, 2] (pixels), depth, conic [B, N, 3], opacity, rgb [B, N, 3], radii (long), rect
    [B, N, 4] (x0, x1, y0, y1 tiles), visible (bool) -- differentiable where the contract is.  ``means2D`` ([N, 3] or [B, N, 3], zeros
    that require grad) is added to p_proj.xy, so its gradient is the contract's dL / d p_proj.xy; its third component is unused (zero
    gradient).  The entries under "raw" are the undecided quantities ``decision_margins`` measures, detached."""
    B = viewmatrix.shape[0]
    N = means3D.shape[-2]
    dt, dev = viewmatrix.dtype, viewmatrix.device
    ex = lambda t, k: (t if t.dim() == k + 1 else t.unsqueeze(0)).expand(B, *t.shape[-k:]) if t is not None else None
    m, s, q, o = ex(means3D, 2), ex(scales, 2), ex(rotations, 2), ex(opacities, 2)[..., 0]
    hom = torch.cat([m, torch.ones_like(m[..., :1])], -1)
    p_view = hom @ viewmatrix                                          # [B, N, 4]
    tz_raw = p_view[..., 2]
    vis_z = tz_raw > 0.2
    tz = torch.where(vis_z, tz_raw, torch.ones_like(tz_raw))          # culled: keep the arithmetic finite, gradient masked below
    ph = hom @ projmatrix
    pproj = ph[..., :2] / (ph[..., 3:] + 1e-7)
    if means2D is not None:
        m2 = ex(means2D, 2)
        pproj = pproj + m2[..., :2] + 0.0 * m2[..., 2:]
    R = quat_to_rot(q)
    sm = s * scale_modifier
    Sig = R @ torch.diag_embed(sm * sm) @ R.transpose(-1, -2)
    tfx = torch.as_tensor(tanfovx, dtype=dt, device=dev).reshape(-1).expand(B)[:, None]
    tfy = torch.as_tensor(tanfovy, dtype=dt, device=dev).reshape(-1).expand(B)[:, None]
    fx, fy = W / (2 * tfx), H / (2 * tfy)
    txtz, tytz = p_view[..., 0] / tz, p_view[..., 1] / tz
    txc = torch.clamp(txtz, -1.3 * tfx, 1.3 * tfx) * tz
    tyc = torch.clamp(tytz, -1.3 * tfy, 1.3 * tfy) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], -1).reshape(B, N, 2, 3)
    Wc = viewmatrix[:, :3, :3].transpose(-1, -2)[:, None]              # column-vector rotation
    T = J @ Wc
    cov = T @ Sig @ T.transpose(-1, -2)
    a, b, c = cov[..., 0, 0] + 0.3, cov[..., 0, 1], cov[..., 1, 1] + 0.3
    det = a * c - b * b
    vis = vis_z & (det != 0)
    det_s = torch.where(vis, det, torch.ones_like(det))
    conic = torch.stack([c / det_s, -b / det_s, a / det_s], -1)
    xy = torch.stack([((pproj[..., 0] + 1) * W - 1) * 0.5, ((pproj[..., 1] + 1) * H - 1) * 0.5], -1)
    with torch.no_grad():
        mid = 0.5 * (a + c)
        l1 = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
        radii = torch.ceil(3 * torch.sqrt(l1)).long()
        gx, gy = (W + 15) // 16, (H + 15) // 16
        trunc = lambda v: torch.trunc(v).long()
        rect_raw = torch.stack([(xy[..., 0] - radii) / 16, (xy[..., 0] + radii + 15) / 16,
                                (xy[..., 1] - radii) / 16, (xy[..., 1] + radii + 15) / 16], -1)
        x0, x1 = trunc(rect_raw[..., 0]).clamp(0, gx), trunc(rect_raw[..., 1]).clamp(0, gx)
        y0, y1 = trunc(rect_raw[..., 2]).clamp(0, gy), trunc(rect_raw[..., 3]).clamp(0, gy)
        pre_cull = vis
        vis = vis & ((x1 - x0) * (y1 - y0) > 0)
        radii = torch.where(vis, radii, torch.zeros_like(radii))
    sh_pre = None
    if colors_precomp is not None:
        rgb = ex(colors_precomp, 2)
    else:
        sh = ex(shs, 3)
        v = m - campos[:, None, :]
        d = v / v.norm(dim=-1, keepdim=True)
        Y = sh_basis(sh_degree, d)                                    # [B, N, K]
        sh_pre = (Y[..., None] * sh[:, :, :Y.shape[-1]]).sum(-2) + 0.5
        rgb = torch.clamp(sh_pre, min=0.0)
    raw = dict(z=tz_raw.detach(), vis_z=vis_z, pre_cull=pre_cull, txtz=txtz.detach(), tytz=tytz.detach(), limx=(1.3 * tfx).expand(B, N),
               limy=(1.3 * tfy).expand(B, N), r3=(3 * torch.sqrt(l1)).detach(), rect_raw=rect_raw.detach(), grid=(gx, gy),
               sh_pre=None if sh_pre is None else sh_pre.detach(), cov=torch.stack([a, b, c], -1).detach())
    return dict(xy=xy, depth=tz, conic=conic, opacity=o, rgb=rgb, radii=radii, rect=torch.stack([x0, x1, y0, y1], -1), visible=vis, raw=raw)


def _pairs(pre, b, H, W):
    """Every pixel of image b against its visible Gaussians in blending order: g (their indices, front to back), power, oG (opacity
    times the Gaussian), alpha = min(0.99, oG), and the contract's decisions: inrect, valid (in the rectangle, power <= 0, alpha >=
    1/255), cum (the running product of 1 - alpha over the valid pairs, i.e. every T (1 - alpha) the stop rule looks at), use."""
    dev, dt = pre["xy"].device, pre["xy"].dtype
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    px, py = xs.reshape(-1).to(dt), ys.reshape(-1).to(dt)
    tx, ty = (xs.reshape(-1) // 16), (ys.reshape(-1) // 16)
    idx = torch.nonzero(pre["visible"][b]).reshape(-1)
    z = pre["depth"][b, idx]
    order = torch.sort(z.detach(), stable=True).indices             # ascending depth, ties by lower Gaussian index
    g = idx[order]
    xy, co, o, rect = pre["xy"][b, g], pre["conic"][b, g], pre["opacity"][b, g], pre["rect"][b, g]
    dx = xy[None, :, 0] - px[:, None]
    dy = xy[None, :, 1] - py[:, None]
    power = -0.5 * (co[None, :, 0] * dx * dx + co[None, :, 2] * dy * dy) - co[None, :, 1] * dx * dy
    oG = o[None] * torch.exp(power)
    alpha = torch.clamp(oG, max=0.99)
    with torch.no_grad():
        inrect = ((tx[:, None] >= rect[None, :, 0]) & (tx[:, None] < rect[None, :, 1]) &
                  (ty[:, None] >= rect[None, :, 2]) & (ty[:, None] < rect[None, :, 3]))
        valid = inrect & (power <= 0) & (alpha >= 1.0 / 255.0)
        a0 = torch.where(valid, alpha, torch.zeros_like(alpha))
        cum = torch.cumprod(1 - a0, dim=1)
        keep = cum >= 1e-4                                            # stop before the Gaussian that takes T below 1e-4
        use = valid & keep
    return dict(g=g, power=power, oG=oG, alpha=alpha, inrect=inrect, valid=valid, cum=cum, keep=keep, use=use)


def composite(pre, H, W, bg, return_counts=False):
    """Front-to-back blending of the visible Gaussians: image [B, 3, H, W], depth [B, 1, H, W], alpha [B, 1, H, W]; with
    ``return_counts`` also, per (image, Gaussian), the number of pixels it contributes to [B, N] (0: every gradient row is zero)."""
    B, N = pre["xy"].shape[:2]
    dt = pre["xy"].dtype
    imgs, deps, alps = [], [], []
    counts = torch.zeros(B, N, dtype=torch.long, device=pre["xy"].device)
    for b in range(B):
        pr = _pairs(pre, b, H, W)
        g, alpha, use = pr["g"], pr["alpha"], pr["use"]
        counts[b, g] = use.sum(0)
        rgb, zz = pre["rgb"][b, g], pre["depth"][b, g]
        a = torch.where(use, alpha, torch.zeros_like(alpha))
        one_minus = 1 - a
        T_incl = torch.cumprod(one_minus, dim=1)
        T_excl = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], 1)
        w = a * T_excl
        T_final = T_incl[:, -1] if T_incl.shape[1] else torch.ones(H * W, dtype=dt, device=counts.device)
        C = w @ rgb + T_final[:, None] * bg.to(dt)[None]
        imgs.append(C.t().reshape(3, H, W))
        deps.append((w @ zz).reshape(1, H, W))
        alps.append((1 - T_final).reshape(1, H, W))
    out = (torch.stack(imgs), torch.stack(deps), torch.stack(alps))
    return out + (counts,) if return_counts else out


def use_mask(pre, H, W):
    """[B, H W, N] bool: pixel p of image b blends Gaussian i (every decision of the blending stage at once)."""
    B, N = pre["xy"].shape[:2]
    out = torch.zeros(B, H * W, N, dtype=torch.bool, device=pre["xy"].device)
    for b in range(B):
        pr = _pairs(pre, b, H, W)
        out[b][:, pr["g"]] = pr["use"]
    return out


def rasterize(means3D, scales, rotations, opacities, *, shs=None, colors_precomp=None, viewmatrix, projmatrix, campos, tanfovx, tanfovy,
              image_height, image_width, bg, scale_modifier=1.0, sh_degree=0, means2D=None):
    """Same call surface as animate3d_amd.splat.rasterize_gaussians: (image, radii, depth, alpha)."""
    pre = preprocess(means3D, scales, rotations, opacities, shs, colors_precomp, viewmatrix, projmatrix, campos, tanfovx, tanfovy,
                     image_height, image_width, scale_modifier, sh_degree, means2D)
    img, dep, alp = composite(pre, image_height, image_width, bg)
    return img, pre["radii"].int(), dep, alp


# Smallest margin a scene compared per Gaussian must keep from every decision (conic_condition: the largest it may have).
MIN_MARGINS = dict(stop=2.0 ** -14, alpha_skip=2.0 ** -12, alpha_clamp=2.0 ** -12, cull_z=2.0 ** -16, ewa_clamp=2.0 ** -16,
                   depth_order=2.0 ** -16, sh_clamp=2.0 ** -12, radius=2.0 ** -8, rect=2.0 ** -8)
MAX_CONIC_CONDITION = 2.0 ** 12


def decision_margins(pre, H, W):
    """The smallest distance from its threshold of every decision the contract makes on ``pre`` (the result of ``preprocess``, float64),
    as a dict of floats (inf where the scene makes no such decision).  Relative means divided by the threshold.  An fp32 evaluation
    takes every decision the way float64 does when its error on the decided quantity stays below the margin; MIN_MARGINS holds the
    margins demanded of a scene, each derived here from that error (u = 2^-24, the unit roundoff of fp32; inputs of size O(1)).

    * cull_z, relative: |p_view.z - 0.2|.  p_view.z is a 4-term dot product of O(1) terms, error <= 4 u |terms| ~ 2^-20 relative to 0.2
      for terms up to 3.  2^-16 leaves 16x.
    * ewa_clamp, relative: ||t.x / t.z| - 1.3 tanfov|, Gaussians that pass the z cull.  Two dot products and a division, ~ 6 u of
      cancellation-free terms up to 4x the result: 2^-19.  2^-16 leaves 8x.
    * radius, absolute: distance of 3 sqrt(lambda_max) to the nearest integer (the ceil), Gaussians that pass the z and det culls.
      lambda_max comes out of ~40 operations on cancellation-free sums (the covariance is a sum of squares, mid + sqrt(.) adds
      positives): relative error ~ 40 u = 2^-18.7, halved by the square root; in pixels, for radii up to 2^7: 2^-12.  2^-8 leaves 16x.
    * rect, absolute: distance of (c - r) / 16 and (c + r + 15) / 16 to the nearest integer in [1, tiles]; truncation toward zero makes
      0 harmless and the clip every integer above ``tiles``.  c is accurate to ~ 8 u 2^10 px = 2^-11 px (off-screen centres up to
      2^10 px), /16: 2^-15.  2^-8 leaves 128x.
    * sh_clamp, absolute: |v| of each colour channel before the clamp at 0, visible Gaussians.  v is a 16-term sum of products of O(1)
      coefficients and basis values <= 3: error <= 16 * 3 u ~ 2^-18.  2^-12 leaves 64x.
    * alpha_skip, relative: |alpha - 1/255| over the pairs (pixel, Gaussian whose rectangle holds the pixel's tile).  alpha = o exp(power):
      power (|power| <= ln 255 = 5.5 where it matters) is rounded to ~ 8 u relative from the conic and the centre, and its absolute
      error 5.5 * 8 u is the relative error of exp, plus the fast exponential's own argument rounding (5.5 log2(e) u): ~ 2^-18.
      2^-12 leaves 64x, enough for the conic's own error (condition <= 2^12 is what bounds it) on top.
    * alpha_clamp, relative: |o G - 0.99| over the same pairs; the same error.  2^-12.
    * stop, relative: |T (1 - alpha) - 1e-4| over every test the blending makes: the valid pairs of a pixel up to and including the one
      that stops it.  T is a product of at most 600 factors (the scenes hold at most 700 Gaussians and stop long before), each with
      the relative error of alpha scaled by alpha / (1 - alpha) <= 1 for the translucent seam scenes, plus one rounding per product:
      600 * u = 3.6e-5 worst case.  2^-14 = 6.1e-5 leaves 1.7x over that worst case.
    * depth_order, relative: the gap between depth-adjacent visible Gaussians of an image whose depths differ.  Depths are p_view.z,
      error ~ 4 u 2 = 2^-21 relative; 2^-16 leaves 32x.  Exactly equal depths come from bit-identical means and stay equal in fp32.
    * conic_condition (a maximum): lambda_max / lambda_min of the 2-D covariance.  power > 0 is reachable only through rounding of an
      ill-conditioned form; at condition <= 2^12 the form's relative error stays ~ 2^12 * 4 u = 2^-10 of its own size, never changing
      its sign except within 2^-10 of the centre, where alpha ~ o is far from 1/255."""
    raw = pre["raw"]
    inf = float("inf")
    least = lambda t: float(t.min()) if t.numel() else inf
    m = dict(cull_z=least((raw["z"] - 0.2).abs() / 0.2))
    vz = raw["vis_z"]
    m["ewa_clamp"] = min(least(((raw["txtz"].abs() - raw["limx"]).abs() / raw["limx"])[vz]),
                         least(((raw["tytz"].abs() - raw["limy"]).abs() / raw["limy"])[vz]))
    pc = raw["pre_cull"]
    r3 = raw["r3"][pc]
    m["radius"] = least((r3 - torch.round(r3)).abs())
    gx, gy = raw["grid"]
    rect = inf
    for comp, tiles in ((0, gx), (1, gx), (2, gy), (3, gy)):
        v = raw["rect_raw"][..., comp][pc]
        ks = torch.arange(1, tiles + 1, dtype=v.dtype, device=v.device)
        rect = min(rect, least((v[:, None] - ks[None]).abs()))
    m["rect"] = rect
    vis = pre["visible"]
    m["sh_clamp"] = inf if raw["sh_pre"] is None else least(raw["sh_pre"][vis].abs())
    cov = raw["cov"][vis]
    mid = 0.5 * (cov[:, 0] + cov[:, 2])
    rad = torch.sqrt(torch.clamp(mid * mid - (cov[:, 0] * cov[:, 2] - cov[:, 1] ** 2), min=0.0))
    m["conic_condition"] = float(((mid + rad) / (mid - rad)).max()) if cov.numel() else 1.0
    m["alpha_skip"] = m["alpha_clamp"] = m["stop"] = m["depth_order"] = inf
    with torch.no_grad():
        for b in range(pre["xy"].shape[0]):
            pr = _pairs(pre, b, H, W)
            z = pre["depth"][b, pr["g"]]
            gap = (z[1:] - z[:-1]) / z[:-1]
            m["depth_order"] = min(m["depth_order"], least(gap[gap != 0]))
            inr = pr["inrect"]
            m["alpha_skip"] = min(m["alpha_skip"], least((pr["alpha"][inr] - 1.0 / 255.0).abs() * 255.0))
            m["alpha_clamp"] = min(m["alpha_clamp"], least((pr["oG"][inr] - 0.99).abs() / 0.99))
            stopped = (~pr["keep"]).long().cumsum(1) > 1                  # strictly after the pair that stops the pixel
            tested = pr["valid"] & ~stopped
            m["stop"] = min(m["stop"], least((pr["cum"][tested] - 1e-4).abs() / 1e-4))
    return m


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """OpenGL-style camera-to-world [4, 4] looking from ``eye`` at ``target`` (the threestudio convention: the camera looks down -z)."""
    eye, target, up = (torch.tensor(v, dtype=torch.float32) for v in (eye, target, up))
    f = target - eye
    f = f / f.norm()
    r = torch.linalg.cross(f, up)
    r = r / r.norm()
    u = torch.linalg.cross(r, f)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, u, -f, eye
    return c2w


def fov_to_tan(fov_deg):
    return math.tan(math.radians(fov_deg) / 2)
