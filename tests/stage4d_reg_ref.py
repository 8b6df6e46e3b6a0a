"""Reference side of the stage4d regulariser tests (TEST INFRASTRUCTURE): the six terms of animate3d.py:256-296 restated in any dtype, and the
seeded inputs that tests/golden/make_stage4d_reg_goldens.py and the tests that replay its vectors both build (a tensor is a function of its
key and shape only, tests/golden/seeded.py, so the fixture holds expected outputs but no inputs)."""
import itertools

import torch

from tests import stage4d_ref as R
from tests.golden.seeded import seeded_tensor

# the weights of the golden cases: six different values, so that a swapped pair shows
LAMBDAS = dict(lambda_tv_loss=2.0, lambda_depth_tv_loss=0.5, lambda_sparsity=3.0, lambda_position=0.7, lambda_opacity=0.05, lambda_scales=0.3)
# the reference's log name of each term, and whether it logs the term times its lambda (animate3d.py:259-295)
LOGGED = dict(lambda_position=("train/loss_position", False), lambda_opacity=("train/loss_opacity", False),
              lambda_sparsity=("train/loss_sparsity", False), lambda_scales=("train/scales", False), lambda_tv_loss=("train/loss_tv", True),
              lambda_depth_tv_loss=("train/loss_depth_tv", True))
RETURNED = dict(lambda_position="loss_position", lambda_opacity="loss_opacity", lambda_sparsity="loss_sparsity", lambda_scales="loss_scales",
                lambda_tv_loss="loss_tv", lambda_depth_tv_loss="loss_depth_tv")      # the key of animate3d_amd.stage4d.training_step's dict
N_VIEW, N_FRAME, STEP = 2, 4, 2 * R.PROGRESSIVE               # frames 1, 2, 3 of both views: six images
MAX_B = 6


def tv_ref(x):
    """2 (sum of squared row differences / (C (H - 1) W) + sum of squared column differences / (C H (W - 1))) / B of ``x [B, C, H, W]``."""
    B, C, H, W = x.shape
    down = ((x[:, :, 1:] - x[:, :, :-1]) ** 2).sum() / (C * (H - 1) * W)
    right = ((x[..., 1:] - x[..., :-1]) ** 2).sum() / (C * H * (W - 1))
    return 2 * (down + right) / B


def image_reg_ref(image, depth, alpha, lambdas, dtype=torch.float64):
    """(loss, tv, depth_tv, sparsity) in ``dtype``; a term whose lambda is 0 is 0 and its operand is not touched."""
    l_tv, l_dtv, l_sp = lambdas
    zero = torch.zeros((), dtype=dtype, device=next(t for t in (image, depth, alpha) if t is not None).device)
    tv = tv_ref(image.to(dtype).clamp(0, 1)) if l_tv else zero
    dtv = tv_ref(depth.to(dtype)) if l_dtv else zero
    sp = (alpha.to(dtype) ** 2 + 0.01).sqrt().mean() if l_sp else zero
    return l_tv * tv + l_dtv * dtv + l_sp * sp, tv, dtv, sp


def gaussian_reg_ref(means, scales, scaling, opacity, lambdas, dtype=torch.float64):
    """(loss, position, scale_sum, opacity_term) in ``dtype``; ``scaling`` is the stored log-scale, ``opacity`` the activated one."""
    l_pos, l_sc, l_op = lambdas
    dev = next(t for t in (means, scales, scaling) if t is not None).device
    zero = torch.zeros((), dtype=dtype, device=dev)
    pos = means.to(dtype).norm(dim=-1).mean() if l_pos else zero
    sc = scales.to(dtype).sum() if l_sc else zero
    op = (scaling.to(dtype).exp().norm(dim=-1).detach().reshape(-1) * opacity.to(dtype).reshape(-1)).sum() if l_op else zero
    return l_pos * pos + l_sc * sc + l_op * op, pos, sc, op


def make_depth(key, B, h=R.H, w=R.W):
    """Unnormalised depth ``[B, 1, h, w]``: positive, a few units deep, with holes of exactly 0 as an empty pixel has."""
    d = seeded_tensor(f"stage4d_reg/{key}/depth", (B, 1, h, w), 1.5) + 3.0
    d.view(-1)[::7] = 0.0
    return d.contiguous()


def make_scales(key, B, n=R.N_POINTS):
    """Activated scales ``[B, n, 3]``, positive."""
    return (seeded_tensor(f"stage4d_reg/{key}/scales", (B, n, 3), 0.8) - 4.0).exp()


def make_static(n=R.N_POINTS):
    """(scaling [n, 3] log-scale, opacity [n, 1] activated) of the static Gaussians."""
    return seeded_tensor("stage4d_reg/scaling", (n, 3), 0.8) - 4.0, torch.sigmoid(seeded_tensor("stage4d_reg/opacity", (n, 1), 1.5))


def cases():
    """Every golden case, in file order: each weight alone and all together, with and without guidance and ARAP."""
    out = []
    for on, guidance, arap in itertools.product([(k,) for k in LAMBDAS] + [tuple(LAMBDAS)], (False, True), (False, True)):
        out.append(dict(on=on, guidance=guidance, arap=arap, n_view=N_VIEW, n_frame=N_FRAME, step=STEP, strategy="normal", seed=0))
    return out


def case_key(c):
    return f"reg/{'+'.join(k[7:] for k in c['on'])}/g{int(c['guidance'])}a{int(c['arap'])}"


def case_loss(c):
    """The ``cfg.loss`` of a case: the released config with the case's weights switched on."""
    return dict(R.LOSS, lambda_arap=R.LOSS["lambda_arap"] if c["arap"] else 0.0, **{k: LAMBDAS[k] for k in c["on"]})
