"""Differentiable 3-D Gaussian splat rasterizer on the gfx950 kernels of csrc/splat.hip, batched over B cameras per call.

The reference renders its 4-D Gaussians with ``diff_gaussian_rasterization`` (custom/threestudio-animate3d/renderer/
diff_gaussian_rasterizer_advanced_4d.py:8-11, 98-163), a CUDA-only extension, once per image in a Python loop over the 64 images
of a step (gaussian_batch_renderer_4d.py:27-60).  This module is that rasterizer: ``GaussianRasterizationSettings`` /
``GaussianRasterizer`` are drop-ins for the single-image call, ``rasterize_gaussians`` takes all cameras of a step in one call.

Contract (the published 3DGS rasterizer, Kerbl et al. 2023, as the ashawkey fork exposes it; all arithmetic fp32).  Per image b
and Gaussian i, with W = viewmatrix[b] and P = projmatrix[b] in the row-vector convention (threestudio/utils/ops.py:344-359):

* p_view = [x, 1] W.  Culled (radius 0, no tiles) when p_view.z <= 0.2.
* p_hom = [x, 1] P, p_proj = p_hom.xyz / (p_hom.w + 1e-7); pixel centre ((p_proj.xy + 1) (W_img, H_img) - 1) / 2.
* Sigma = M^T M, M = diag(s * scale_modifier) R(q / |q|), q ordered (r, x, y, z); i.e. Sigma = R_q diag(s^2) R_q^T with R_q the
  usual rotation matrix of the unit quaternion.
* EWA: t = p_view with t.x / t.z, t.y / t.z clamped to +-1.3 tanfov (times t.z again); J = [[f_x/t_z, 0, -f_x t_x/t_z^2],
  [0, f_y/t_z, -f_y t_y/t_z^2]], f = size / (2 tanfov); Sigma' = J W_r Sigma W_r^T J^T (W_r the rotation part of the view
  transform) plus 0.3 on the diagonal.  det(Sigma') == 0 culls; conic = Sigma'^-1; radius = ceil(3 sqrt(lambda_max)),
  lambda_max = mid + sqrt(max(0.1, mid^2 - det)).  The Gaussian covers the 16 x 16 tiles of the rectangle
  [(c - r) / 16, (c + r + 15) / 16) (truncated, clipped to the grid); none touched culls.
* Colour: ``colors_precomp``, or SH of degree 0-3 at direction normalize(x - campos) plus 0.5, clamped at 0 (the clamp's
  gradient is zero).  Standard real-SH constants.
* Blending per pixel (pixel coordinates are the integer indices), front to back in ascending p_view.z (ties: lower Gaussian index),
  over the Gaussians whose tiles include the pixel's: d = centre - pixel, power = -(c0 dx^2 + c2 dy^2) / 2 - c1 dx dy, skipped
  when power > 0; alpha = min(0.99, o exp(power)), skipped when alpha < 1/255; stop before a Gaussian that would take
  T (1 - alpha) below 1e-4; C += c alpha T, T *= 1 - alpha.
* Outputs: image = C + T bg, depth = sum z_i alpha_i T_i (not normalised), alpha = 1 - T_final, radii int32.  The three image
  outputs are differentiable; the gradient that reaches ``means2D`` is dL / d p_proj.xy (NDC), its third component zero.

Gradients follow the exact derivative of that forward: no gradient through alpha's 0.99 clamp nor the SH colour clamp, and a
clamped EWA coordinate t.x = +-1.3 tanfov t.z passes its gradient to t.z.  (The CUDA package passes gradient through the 0.99
clamp and drops the t.z term: a difference only where those clamps are active.)  The backward uses no atomics: two backward
passes on the same inputs are bit-identical, and B images in one call are bit-identical to B single-image calls.

``cov3D_precomp`` and ``prefiltered=True`` raise ``NotImplementedError``: the reference passes neither.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Union

import torch

from .f32_stage import launch, require_f32_cuda
from .hip_ops import _p

TILE = 16
ROW_FLOATS = 12          # per-instance gradient row of a3d_gs_render_bwd_f32
_stats = {"instances": 0}


def tile_grid(height: int, width: int):
    """(tiles_x, tiles_y) of an image."""
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def tile_rect(px: float, py: float, radius: int, height: int, width: int):
    """The [x0, x1) x [y0, y1) tile rectangle a Gaussian at pixel (px, py) with ``radius`` touches (host restatement of the kernels')."""
    gx, gy = tile_grid(height, width)
    x0 = min(gx, max(0, int((px - radius) / TILE)))
    x1 = min(gx, max(0, int((px + radius + TILE - 1) / TILE)))
    y0 = min(gy, max(0, int((py - radius) / TILE)))
    y1 = min(gy, max(0, int((py + radius + TILE - 1) / TILE)))
    return x0, x1, y0, y1


def sort_key(image: int, tile: int, tiles_per_image: int, depth: float) -> int:
    """The duplicate stage's 64-bit key: (image * tiles + tile) << 32 | float bits of depth (depth > 0 sorts as unsigned)."""
    bits = int(torch.tensor([depth], dtype=torch.float32).view(torch.int32).item()) & 0xFFFFFFFF
    return ((image * tiles_per_image + tile) << 32) | bits


def last_instance_count() -> int:
    """Duplicated (image, Gaussian, tile) instances of the last forward: the backward's gradient rows are 48 B each."""
    return _stats["instances"]


def _per_gaussian(t: torch.Tensor, name: str, B: int, N: int, tail: Sequence[int]):
    require_f32_cuda(name, t)
    tail = tuple(tail)
    if tuple(t.shape) == (N, *tail):
        return t.contiguous(), 0
    if tuple(t.shape) == (B, N, *tail):
        return t.contiguous(), N * math.prod(tail)
    raise ValueError(f"{name}: shape {tuple(t.shape)} is neither {(N, *tail)} nor {(B, N, *tail)}")


def _per_image(v, B: int, device, name: str) -> torch.Tensor:
    t = torch.as_tensor(v, dtype=torch.float32, device=device).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"{name}: {t.numel()} values for {B} images")
    return t.contiguous()


def _reduce_to(g: torch.Tensor, shape: torch.Size, B: int) -> torch.Tensor:
    """Per-(image, Gaussian) gradient [B, N, ...] -> the input's shape: summed over images, in order, for an input shared by all."""
    if len(shape) == g.dim():
        return g
    if B == 1:
        return g.reshape(shape)
    out = torch.empty(shape, dtype=torch.float32, device=g.device)
    launch("a3d_gs_sum_batch_f32", g.device, _p(g), _p(out), B, out.numel())
    return out


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, opacities, shs, colors_precomp, means2D, viewmatrix, projmatrix, campos, tanfovx, tanfovy,
                bg, image_height, image_width, scale_modifier, sh_degree):
        B, N, H, W = viewmatrix.shape[0], means3D.shape[-2], int(image_height), int(image_width)
        dev = means3D.device
        m, m_bs = _per_gaussian(means3D.detach(), "means3D", B, N, (3,))
        s, s_bs = _per_gaussian(scales.detach(), "scales", B, N, (3,))
        r, r_bs = _per_gaussian(rotations.detach(), "rotations", B, N, (4,))
        o, o_bs = _per_gaussian(opacities.detach(), "opacities", B, N, (1,))
        M = 0
        if shs is not None:
            M = shs.shape[-2]
            sh, sh_bs = _per_gaussian(shs.detach(), "shs", B, N, (M, 3))
            if M < (sh_degree + 1) ** 2:
                raise ValueError(f"sh_degree {sh_degree} needs {(sh_degree + 1) ** 2} coefficients, shs has {M}")
            col, col_bs = None, 0
        else:
            col, col_bs = _per_gaussian(colors_precomp.detach(), "colors_precomp", B, N, (3,))
            sh, sh_bs = None, 0
        view = viewmatrix.detach().float().contiguous()
        proj = projmatrix.detach().float().contiguous()
        cam = campos.detach().float().reshape(B, 3).contiguous()
        bgc = bg.detach().float().reshape(3).contiguous()
        inputs = (B, N, _p(m), m_bs, _p(s), s_bs, _p(r), r_bs, _p(o), o_bs, _p(sh), sh_bs, M, int(sh_degree), _p(col), col_bs,
                  _p(view), _p(proj), _p(cam), _p(tanfovx), _p(tanfovy), H, W, float(scale_modifier))
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        radii, clamped, tiles = torch.empty(B, N, **i32), torch.empty(B, N, **i32), torch.empty(B, N, **i32)
        xy, depth, conic, rgb = torch.empty(B, N, 2, **f32), torch.empty(B, N, **f32), torch.empty(B, N, 4, **f32), torch.empty(B, N, 3, **f32)
        launch("a3d_gs_preprocess_f32", dev, *inputs, _p(radii), _p(xy), _p(depth), _p(conic), _p(rgb), _p(clamped), _p(tiles))
        offsets = torch.cumsum(tiles.view(-1), 0)
        L = int(offsets[-1])
        if L >= 2 ** 31:
            raise RuntimeError(f"{L} tile instances exceed the int32 range of the tile ranges")
        _stats["instances"] = L
        keys = torch.empty(max(L, 1), dtype=torch.int64, device=dev)
        vals = torch.empty(max(L, 1), **i32)
        launch("a3d_gs_duplicate_f32", dev, B, N, H, W, _p(xy), _p(depth), _p(radii), _p(offsets), _p(keys), _p(vals))
        keys_sorted, perm = torch.sort(keys[:L], stable=True)
        if L == 0:
            perm = torch.zeros(1, dtype=torch.int64, device=dev)
        gx, gy = tile_grid(H, W)
        ranges = torch.empty(B * gx * gy, 2, **i32)
        launch("a3d_gs_tile_ranges_f32", dev, _p(keys_sorted), L, _p(ranges), B * gx * gy)
        img, dep, alpha, T_final = (torch.empty(B, 3, H, W, **f32), torch.empty(B, 1, H, W, **f32), torch.empty(B, 1, H, W, **f32),
                                    torch.empty(B, H, W, **f32))
        n_contrib = torch.empty(B, H, W, **i32)
        launch("a3d_gs_render_f32", dev, B, N, H, W, _p(ranges), _p(perm), _p(vals), _p(xy), _p(conic), _p(rgb), _p(depth), _p(bgc), _p(img),
               _p(dep), _p(alpha), _p(T_final), _p(n_contrib))
        ctx.save_for_backward(m, s, r, o, sh, col, view, proj, cam, tanfovx, tanfovy, bgc, radii, clamped, tiles, offsets, ranges, perm,
                              vals, xy, conic, rgb, depth, T_final, n_contrib)
        ctx.meta = (B, N, H, W, M, int(sh_degree), float(scale_modifier), m_bs, s_bs, r_bs, o_bs, sh_bs, col_bs, L)
        ctx.shapes = (means3D.shape, scales.shape, rotations.shape, opacities.shape, None if shs is None else shs.shape,
                      None if colors_precomp is None else colors_precomp.shape, None if means2D is None else means2D.shape)
        ctx.mark_non_differentiable(radii)
        return img, radii, dep, alpha

    @staticmethod
    def backward(ctx, d_img, _d_radii, d_depth, d_alpha):
        (m, s, r, o, sh, col, view, proj, cam, tanfovx, tanfovy, bgc, radii, clamped, tiles, offsets, ranges, perm, vals, xy, conic, rgb,
         depth, T_final, n_contrib) = ctx.saved_tensors
        B, N, H, W, M, deg, smod, m_bs, s_bs, r_bs, o_bs, sh_bs, col_bs, L = ctx.meta
        dev = m.device
        f32 = dict(dtype=torch.float32, device=dev)
        d_img = torch.zeros(B, 3, H, W, **f32) if d_img is None else d_img.float().contiguous()
        d_depth = None if d_depth is None else d_depth.float().contiguous()
        d_alpha = None if d_alpha is None else d_alpha.float().contiguous()
        rows = torch.empty(max(L, 1), ROW_FLOATS, **f32)
        launch("a3d_gs_render_bwd_f32", dev, B, N, H, W, _p(ranges), _p(perm), _p(vals), _p(xy), _p(conic), _p(rgb), _p(depth), _p(bgc),
               _p(T_final), _p(n_contrib), _p(d_img), _p(d_depth), _p(d_alpha), _p(rows))
        g2d, gm, gs, gr, go = (torch.empty(B, N, 3, **f32), torch.empty(B, N, 3, **f32), torch.empty(B, N, 3, **f32), torch.empty(B, N, 4, **f32),
                               torch.empty(B, N, 1, **f32))
        gsh = torch.empty(B, N, M, 3, **f32) if sh is not None else None
        gcol = torch.empty(B, N, 3, **f32) if col is not None else None
        inputs = (B, N, _p(m), m_bs, _p(s), s_bs, _p(r), r_bs, _p(o), o_bs, _p(sh), sh_bs, M, deg, _p(col), col_bs,
                  _p(view), _p(proj), _p(cam), _p(tanfovx), _p(tanfovy), H, W, smod)
        launch("a3d_gs_preprocess_bwd_f32", dev, *inputs, _p(radii), _p(clamped), _p(offsets), _p(tiles), _p(rows), _p(g2d), _p(gm), _p(gs),
               _p(gr), _p(go), _p(gsh), _p(gcol))
        m_shape, s_shape, r_shape, o_shape, sh_shape, col_shape, m2_shape = ctx.shapes
        need = ctx.needs_input_grad
        out_m = _reduce_to(gm, m_shape, B) if need[0] else None
        out_s = _reduce_to(gs, s_shape, B) if need[1] else None
        out_r = _reduce_to(gr, r_shape, B) if need[2] else None
        out_o = _reduce_to(go, o_shape, B) if need[3] else None
        out_sh = _reduce_to(gsh, sh_shape, B) if (need[4] and gsh is not None) else None
        out_col = _reduce_to(gcol, col_shape, B) if (need[5] and gcol is not None) else None
        out_m2 = None
        if need[6] and m2_shape is not None:
            out_m2 = _reduce_to(g2d[..., :m2_shape[-1]].contiguous(), m2_shape, B)
        return out_m, out_s, out_r, out_o, out_sh, out_col, out_m2, None, None, None, None, None, None, None, None, None, None


def rasterize_gaussians(means3D: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor, *,
                        shs: Optional[torch.Tensor] = None, colors_precomp: Optional[torch.Tensor] = None, viewmatrix: torch.Tensor,
                        projmatrix: torch.Tensor, campos: torch.Tensor, tanfovx: Union[float, torch.Tensor],
                        tanfovy: Union[float, torch.Tensor], image_height: int, image_width: int, bg: torch.Tensor,
                        scale_modifier: float = 1.0, sh_degree: int = 0, means2D: Optional[torch.Tensor] = None,
                        cov3D_precomp: Optional[torch.Tensor] = None, prefiltered: bool = False):
    """Render B images.  Per-Gaussian inputs are [N, ...] (shared by every image) or [B, N, ...] (per image: the deformed means,
    scales and rotations of each frame): means3D / scales [., 3], rotations [., 4] (r, x, y, z; normalised here), opacities [., 1],
    shs [., M, 3] or colors_precomp [., 3].  viewmatrix / projmatrix [B, 4, 4] (row-vector convention), campos [B, 3], tanfov a
    scalar or [B].  ``means2D`` (optional, [N, 3] or [B, N, 3]) only receives the NDC centre gradient.
    Returns image [B, 3, H, W], radii [B, N] int32, depth [B, 1, H, W], alpha [B, 1, H, W]."""
    if cov3D_precomp is not None:
        raise NotImplementedError("cov3D_precomp: the reference never passes it; give scales and rotations")
    if prefiltered:
        raise NotImplementedError("prefiltered=True: the reference never passes it")
    if (shs is None) == (colors_precomp is None):
        raise ValueError("give exactly one of shs / colors_precomp")
    if not 0 <= int(sh_degree) <= 3:
        raise ValueError(f"sh_degree {sh_degree}: 0 .. 3")
    if viewmatrix.dim() != 3 or viewmatrix.shape[1:] != (4, 4) or projmatrix.shape != viewmatrix.shape:
        raise ValueError("viewmatrix / projmatrix must be [B, 4, 4]")
    B, dev = viewmatrix.shape[0], means3D.device
    tx, ty = _per_image(tanfovx, B, dev, "tanfovx"), _per_image(tanfovy, B, dev, "tanfovy")
    bg = torch.as_tensor(bg, dtype=torch.float32, device=dev)
    return _RasterizeGaussians.apply(means3D, scales, rotations, opacities, shs, colors_precomp, means2D, viewmatrix.to(dev),
                                     projmatrix.to(dev), campos.to(dev), tx, ty, bg, image_height, image_width, scale_modifier, sh_degree)


class GaussianRasterizationSettings(NamedTuple):
    """Same fields as diff_gaussian_rasterization.GaussianRasterizationSettings (one image)."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool = False


class GaussianRasterizer(torch.nn.Module):
    """Drop-in for diff_gaussian_rasterization.GaussianRasterizer: one image, returns (image [3, H, W], radii [N], depth [1, H, W],
    alpha [1, H, W]); ``means2D.grad`` receives the NDC centre gradient."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        rs = self.raster_settings
        if scales is None or rotations is None:
            raise NotImplementedError("scales and rotations are required (cov3D_precomp is not supported)")
        img, radii, depth, alpha = rasterize_gaussians(
            means3D, scales, rotations, opacities, shs=shs, colors_precomp=colors_precomp, viewmatrix=rs.viewmatrix.reshape(1, 4, 4),
            projmatrix=rs.projmatrix.reshape(1, 4, 4), campos=rs.campos.reshape(1, 3), tanfovx=rs.tanfovx, tanfovy=rs.tanfovy,
            image_height=rs.image_height, image_width=rs.image_width, bg=rs.bg, scale_modifier=rs.scale_modifier, sh_degree=rs.sh_degree,
            means2D=means2D, cov3D_precomp=cov3D_precomp, prefiltered=rs.prefiltered)
        return img[0], radii[0], depth[0], alpha[0]


# ---- camera helpers (threestudio/utils/ops.py:305-359), batched, on the caller's device

def convert_pose(c2w: torch.Tensor) -> torch.Tensor:
    """OpenGL -> COLMAP camera axes: c2w [..., 4, 4] times diag(1, -1, -1, 1)."""
    flip = torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=c2w.dtype, device=c2w.device)
    return c2w * flip


def get_projection_matrix_gaussian(znear: float, zfar: float, fovX, fovY, device=None) -> torch.Tensor:
    """Perspective matrix (column-vector form) for fov in radians: [4, 4] for scalar fovs, [B, 4, 4] for [B] tensors."""
    fx = torch.as_tensor(fovX, dtype=torch.float32, device=device)
    fy = torch.as_tensor(fovY, dtype=torch.float32, device=device)
    fx, fy = torch.broadcast_tensors(fx, fy)
    tan_y, tan_x = torch.tan(fy / 2), torch.tan(fx / 2)
    P = torch.zeros(*fx.shape, 4, 4, dtype=torch.float32, device=fx.device)
    top, right = tan_y * znear, tan_x * znear
    P[..., 0, 0] = 2.0 * znear / (2 * right)
    P[..., 1, 1] = 2.0 * znear / (2 * top)
    P[..., 3, 2] = 1.0
    P[..., 2, 2] = zfar / (zfar - znear)
    P[..., 2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def get_cam_info_gaussian(c2w: torch.Tensor, fovx, fovy, znear: float, zfar: float):
    """c2w [B, 4, 4] (or [4, 4]), fov [B] or scalar -> (world_view_transform, full_proj_transform, camera_center), row-vector
    convention, on c2w's device: [B, 4, 4], [B, 4, 4], [B, 3] (unbatched shapes for an unbatched c2w)."""
    single = c2w.dim() == 2
    c = convert_pose(c2w.reshape(-1, 4, 4).float())
    w2c = torch.linalg.inv(c).transpose(-1, -2)
    fx = torch.as_tensor(fovx, dtype=torch.float32, device=c.device).expand(c.shape[0])
    fy = torch.as_tensor(fovy, dtype=torch.float32, device=c.device).expand(c.shape[0])
    proj = get_projection_matrix_gaussian(znear, zfar, fx, fy, device=c.device).transpose(-1, -2)
    full = torch.bmm(w2c, proj)
    center = torch.linalg.inv(w2c)[:, 3, :3]
    if single:
        return w2c[0], full[0], center[0]
    return w2c, full, center
