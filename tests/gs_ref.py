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
               scale_modifier=1.0, sh_degree=0):
    """Per (image, Gaussian): dict of xy [B, N, 2] (pixels), depth, conic [B, N, 3], opacity, rgb [B, N, 3], radii (long), rect
    [B, N, 4] (x0, x1, y0, y1 tiles), visible (bool) -- differentiable where the contract is."""
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
    R = quat_to_rot(q)
    sm = s * scale_modifier
    Sig = R @ torch.diag_embed(sm * sm) @ R.transpose(-1, -2)
    tfx = torch.as_tensor(tanfovx, dtype=dt, device=dev).reshape(-1).expand(B)[:, None]
    tfy = torch.as_tensor(tanfovy, dtype=dt, device=dev).reshape(-1).expand(B)[:, None]
    fx, fy = W / (2 * tfx), H / (2 * tfy)
    txc = torch.clamp(p_view[..., 0] / tz, -1.3 * tfx, 1.3 * tfx) * tz
    tyc = torch.clamp(p_view[..., 1] / tz, -1.3 * tfy, 1.3 * tfy) * tz
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
        x0 = trunc((xy[..., 0] - radii) / 16).clamp(0, gx)
        x1 = trunc((xy[..., 0] + radii + 15) / 16).clamp(0, gx)
        y0 = trunc((xy[..., 1] - radii) / 16).clamp(0, gy)
        y1 = trunc((xy[..., 1] + radii + 15) / 16).clamp(0, gy)
        vis = vis & ((x1 - x0) * (y1 - y0) > 0)
        radii = torch.where(vis, radii, torch.zeros_like(radii))
    if colors_precomp is not None:
        rgb = ex(colors_precomp, 2)
    else:
        sh = ex(shs, 3)
        v = m - campos[:, None, :]
        d = v / v.norm(dim=-1, keepdim=True)
        Y = sh_basis(sh_degree, d)                                    # [B, N, K]
        rgb = torch.clamp((Y[..., None] * sh[:, :, :Y.shape[-1]]).sum(-2) + 0.5, min=0.0)
    return dict(xy=xy, depth=tz, conic=conic, opacity=o, rgb=rgb, radii=radii, rect=torch.stack([x0, x1, y0, y1], -1), visible=vis)


def composite(pre, H, W, bg):
    """Front-to-back blending of the visible Gaussians: image [B, 3, H, W], depth [B, 1, H, W], alpha [B, 1, H, W]."""
    B = pre["xy"].shape[0]
    dev, dt = pre["xy"].device, pre["xy"].dtype
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    px, py = xs.reshape(-1).to(dt), ys.reshape(-1).to(dt)
    tx, ty = (xs.reshape(-1) // 16), (ys.reshape(-1) // 16)
    imgs, deps, alps = [], [], []
    for b in range(B):
        idx = torch.nonzero(pre["visible"][b]).reshape(-1)
        z = pre["depth"][b, idx]
        order = torch.sort(z.detach(), stable=True).indices             # ascending depth, ties by lower Gaussian index
        g = idx[order]
        xy, co, o = pre["xy"][b, g], pre["conic"][b, g], pre["opacity"][b, g]
        rgb, zz, rect = pre["rgb"][b, g], pre["depth"][b, g], pre["rect"][b, g]
        dx = xy[None, :, 0] - px[:, None]
        dy = xy[None, :, 1] - py[:, None]
        power = -0.5 * (co[None, :, 0] * dx * dx + co[None, :, 2] * dy * dy) - co[None, :, 1] * dx * dy
        alpha = torch.clamp(o[None] * torch.exp(power), max=0.99)
        with torch.no_grad():
            inrect = ((tx[:, None] >= rect[None, :, 0]) & (tx[:, None] < rect[None, :, 1]) &
                      (ty[:, None] >= rect[None, :, 2]) & (ty[:, None] < rect[None, :, 3]))
            valid = inrect & (power <= 0) & (alpha >= 1.0 / 255.0)
            a0 = torch.where(valid, alpha, torch.zeros_like(alpha))
            keep = torch.cumprod(1 - a0, dim=1) >= 1e-4                  # stop before the Gaussian that takes T below 1e-4
            use = valid & keep
        a = torch.where(use, alpha, torch.zeros_like(alpha))
        one_minus = 1 - a
        T_incl = torch.cumprod(one_minus, dim=1)
        T_excl = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], 1)
        w = a * T_excl
        T_final = T_incl[:, -1] if T_incl.shape[1] else torch.ones_like(px)
        C = w @ rgb + T_final[:, None] * bg.to(dt)[None]
        imgs.append(C.t().reshape(3, H, W))
        deps.append((w @ zz).reshape(1, H, W))
        alps.append((1 - T_final).reshape(1, H, W))
    return torch.stack(imgs), torch.stack(deps), torch.stack(alps)


def rasterize(means3D, scales, rotations, opacities, *, shs=None, colors_precomp=None, viewmatrix, projmatrix, campos, tanfovx, tanfovy,
              image_height, image_width, bg, scale_modifier=1.0, sh_degree=0):
    """Same call surface as animate3d_amd.splat.rasterize_gaussians: (image, radii, depth, alpha)."""
    pre = preprocess(means3D, scales, rotations, opacities, shs, colors_precomp, viewmatrix, projmatrix, campos, tanfovx, tanfovy,
                     image_height, image_width, scale_modifier, sh_degree)
    img, dep, alp = composite(pre, image_height, image_width, bg)
    return img, pre["radii"].int(), dep, alp


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
