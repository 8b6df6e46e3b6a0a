"""Reference side of the stage4d tests (TEST INFRASTRUCTURE): the reference's reconstruction loss as it is written, in any dtype, and the
seeded inputs that tests/golden/make_stage4d_goldens.py and the tests that replay its vectors both build (a tensor is a function of its key
and shape only, tests/golden/seeded.py, so the fixture holds expected outputs but no inputs)."""
import itertools

import torch
import torch.nn.functional as F

from tests.golden.seeded import seeded_tensor

BG = (0.3, 0.6, 0.9)             # back_ground_color: three different values, so that using any but [0] shows
LOSS = dict(lambda_rgb=100.0, lambda_mask=100.0, lambda_sds=0.01, lambda_arap=12.0, arap_K=3, arap_radius=0.01, arap_sample_num=512,
            lambda_position=0.0, lambda_opacity=0.0, lambda_scales=0.0, lambda_sparsity=0.0, lambda_tv_loss=0.0, lambda_depth_tv_loss=0.0,
            lambda_normal_tv=0.0)          # configs/motion_recon_frame_16.yaml:168-188
H = W = 8
N_POINTS, N_RANDOM_CAMERA, PROGRESSIVE = 5, 4, 10


def recon_loss_ref(image, alpha, gt_rgb, gt_mask, index, bg, lambda_rgb, lambda_mask, dtype=torch.float64):
    """animate3d.py:160-184 on the renderer's outputs (advanced_4d.py:180, batch_renderer:73, 107), literally: the indexed copies, the clamp
    and permute, the compositing with the float mask, two F.mse_loss.  ``image [B, 3, H, W]`` raw, ``alpha [B, 1, H, W]``; returns
    (loss, loss_rgb, loss_mask) in ``dtype``."""
    pred_rgb = image.to(dtype).clamp(0, 1).permute(0, 2, 3, 1)
    comp_mask = alpha.to(dtype).reshape(alpha.shape[0], 1, *alpha.shape[-2:]).permute(0, 2, 3, 1)
    if index is not None:
        gt_rgb, gt_mask = gt_rgb[index], gt_mask[index]
    gt_mask = gt_mask.reshape(*gt_mask.shape[:3], 1)
    gt_rgb = gt_rgb.to(dtype)
    m = gt_mask.to(dtype)                                       # gt_mask.float()
    gt = gt_rgb * m + bg * (1 - m)
    loss_rgb = F.mse_loss(gt, pred_rgb)
    loss_mask = F.mse_loss(m, comp_mask)
    return lambda_rgb * loss_rgb + lambda_mask * loss_mask, loss_rgb, loss_mask


def special_values():
    """Render values at and around the clamp's bounds: the bounds themselves (gradient passes) and their fp32 neighbours on both sides."""
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    return torch.stack([zero, one, torch.nextafter(zero, one), torch.nextafter(zero, -one), torch.nextafter(one, zero),
                        torch.nextafter(one, one + one), -zero, torch.tensor(-0.5), torch.tensor(1.5)])


def make_render(key, B, h=H, w=W):
    """(image [B, 3, h, w], alpha [B, 1, h, w]) fp32: values below 0, above 1, and ``special_values`` at fixed places."""
    image = seeded_tensor(f"stage4d/{key}/image", (B, 3, h, w), 0.6) + 0.5
    alpha = (seeded_tensor(f"stage4d/{key}/alpha", (B, 1, h, w), 0.35) + 0.5)
    sv = special_values()
    flat = image.view(-1)
    n = min(sv.numel(), flat.numel())
    flat[torch.arange(n) * (flat.numel() // n)] = sv[:n]
    return image.contiguous(), alpha.contiguous()


def make_means(key, B, n=N_POINTS):
    return seeded_tensor(f"stage4d/{key}/means", (B, n, 3), 0.3)


def make_batch(n_view, n_frame, h=H, w=W):
    """The data batch: image i = view * n_frame + frame carries its own number in ``c2w[i, 0, 3]`` and ``fovy[i]``."""
    S = n_view * n_frame
    ids = torch.arange(S, dtype=torch.float32)
    c2w = torch.eye(4).repeat(S, 1, 1)
    c2w[:, 0, 3] = ids
    return dict(rgb=seeded_tensor(f"stage4d/{n_view}x{n_frame}/rgb", (S, h, w, 3), 0.3) + 0.5,
                mask=seeded_tensor(f"stage4d/{n_view}x{n_frame}/mask", (S, h, w, 1)) > 0.2,
                c2w=c2w, fovy=0.5 + 0.01 * ids, timestamps=torch.linspace(-1, 1, n_frame).repeat(n_view), height=h, width=w)


def make_random_camera(h=H, w=W):
    B = N_RANDOM_CAMERA
    c2w = torch.eye(4).repeat(B, 1, 1)
    c2w[:, 0, 3] = 1000.0 + torch.arange(B)
    return dict(c2w=c2w, fovy=torch.full((B,), 0.7), timestamps=torch.linspace(-1, 1, B), height=h, width=w)


def guidance_stub(rgb):
    """A fixed quadratic of the guidance input ``comp_rgb``."""
    return 0.5 * ((rgb - 0.25) ** 2).sum()


def arap_stub_weight(shape):
    """nodes_t [F + 1, N, 3] -> weights whose integer part is the node's position in the stack."""
    f, n, c = torch.meshgrid(*(torch.arange(s, dtype=torch.float32) for s in shape), indexing="ij")
    return f + 0.1 * n / shape[1] + 0.01 * c


def cases():
    """Every golden case, in file order: dicts of n_view, n_frame, step, strategy, seed, guidance, arap, numeric."""
    out = []
    for n_view, n_frame in itertools.product((2, 4), (4, 8)):
        steps = (0, PROGRESSIVE - 1, 2 * PROGRESSIVE, PROGRESSIVE * (n_frame + 2))
        for step, (strategy, seed), guidance, arap in itertools.product(steps, (("normal", 0), ("light", 0), ("light", 1), ("light", 2)),
                                                                        (False, True), (False, True)):
            numeric = (not arap and seed == 0 and (n_view, n_frame) == (2, 4)) or \
                      ((n_view, n_frame, strategy, guidance, arap) == (4, 8, "normal", False, False) and step == steps[-1])
            out.append(dict(n_view=n_view, n_frame=n_frame, step=step, strategy=strategy, seed=seed, guidance=guidance, arap=arap,
                            numeric=numeric))
    return out


def case_key(c):
    return f"{c['n_view']}x{c['n_frame']}/s{c['step']}/{c['strategy']}{c['seed']}/g{int(c['guidance'])}"
