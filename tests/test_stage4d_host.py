"""CPU tier of animate3d_amd.stage4d: the frame schedule against the golden the reference's own ``training_step`` produced
(tests/golden/make_stage4d_goldens.py), the optimiser groups, and the refusals that need no device."""
import os
import random

import numpy as np
import pytest
import torch

from animate3d_amd import stage4d
from animate3d_amd.deform4d import HexPlaneDeformation
from tests import stage4d_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage4d.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_schedule_and_index_equal_the_reference_on_every_case(golden):
    cases = R.cases()
    assert len(cases) == int(golden["n_cases"]) == golden["sampled_idx"].shape[0]
    lengths = set()
    for i, c in enumerate(cases):
        frames = stage4d.sampled_frames(c["step"], c["n_frame"], R.PROGRESSIVE, do_guidance=c["guidance"], strategy=c["strategy"],
                                        rng=random.Random(c["seed"]))
        index = stage4d.sampled_image_index(frames, c["n_view"], c["n_frame"])
        want = golden["sampled_idx"][i]
        want = want[want >= 0]
        assert index.dtype == torch.int32 and index.tolist() == want.tolist(), (c, frames, want)
        lengths.add(len(frames))
    assert {1, 2, 3, 7} <= lengths                               # one frame, the light pair, every frame of both lengths


def test_schedule_draws_from_the_global_random_by_default():
    random.seed(5)
    a = stage4d.sampled_frames(45, 8, 10, do_guidance=False, strategy="light")
    assert a == stage4d.sampled_frames(45, 8, 10, do_guidance=False, strategy="light", rng=random.Random(5)) and a[1] == 5


def test_unknown_strategy_raises_as_the_reference_does():
    with pytest.raises(NotImplementedError):
        stage4d.sampled_frames(0, 8, 10, do_guidance=False, strategy="dense")


RATES = dict(delta_xyz_network_lr=6e-4, delta_rot_network_lr=6e-4, delta_scaling_network_lr=6e-4, grid_lr=6e-3, global_trans_lr=6e-4)


@pytest.mark.parametrize("use_global_trans", [False, True])
def test_param_groups_cover_every_parameter_once(use_global_trans):
    field = HexPlaneDeformation(((4, 4, 4, 2), (6, 6, 6, 3)), use_global_trans=use_global_trans)
    groups = stage4d.field_param_groups(field, **RATES)
    names = ["delta_xyz_network", "delta_rot_network", "delta_scaling_network", "grid"] + (["global_trans"] if use_global_trans else [])
    assert [g["name"] for g in groups] == names
    assert [g["lr"] for g in groups] == [6e-4, 6e-4, 6e-4, 6e-3] + ([6e-4] if use_global_trans else [])
    seen = [id(p) for g in groups for p in g["params"]]
    assert sorted(seen) == sorted(id(p) for p in field.parameters()) and len(set(seen)) == len(seen)
    by_name = {g["name"]: g["params"] for g in groups}
    assert len(by_name["grid"]) == 12 and all(len(by_name[n]) == 2 for n in names[:3])
    if use_global_trans:
        assert len(by_name["global_trans"]) == 4
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    assert [g["lr"] for g in opt.param_groups][:4] == [6e-4, 6e-4, 6e-4, 6e-3]


def test_list_valued_rate_is_refused():
    field = HexPlaneDeformation(((4, 4, 4, 2), (6, 6, 6, 3)))
    with pytest.raises(NotImplementedError):
        stage4d.field_param_groups(field, **dict(RATES, grid_lr=[0, 6e-3, 6e-5, 1000]))


def _inputs(B=2, S=2, h=4, w=4):
    return torch.zeros(B, 3, h, w), torch.zeros(B, 1, h, w), torch.zeros(S, h, w, 3), torch.zeros(S, h, w, 1, dtype=torch.bool)


def test_refusals_without_a_device():
    kw = dict(bg=0.5, lambda_rgb=1.0, lambda_mask=1.0)
    image, alpha, gt, mask = _inputs()
    with pytest.raises(TypeError):
        stage4d.masked_recon_loss(image, alpha, gt, mask.float(), **kw)                   # a float mask
    with pytest.raises(ValueError):
        stage4d.masked_recon_loss(image, alpha, *_inputs(S=3)[2:], **kw)                  # S != B without an index
    with pytest.raises(ValueError):
        stage4d.masked_recon_loss(image, alpha[:, :, :2], gt, mask, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.masked_recon_loss(image, alpha, gt, mask, **kw)                           # CPU tensors


@pytest.mark.parametrize("name", stage4d.UNSUPPORTED_LAMBDAS)
def test_unsupported_lambda_raises(name):
    with pytest.raises(NotImplementedError, match=name):
        stage4d.training_step(None, None, {}, loss=dict(R.LOSS, **{name: 0.1}), global_step=0, n_view=2, n_frame=4,
                              progressive_iter_per_frame=10, bg=R.BG)


def test_golden_gradients_are_the_float64_restatement(golden):
    """The reference's own fp32 gradients with respect to the raw render and alpha against tests/stage4d_ref.recon_loss_ref in float64 on the
    same inputs: what the GPU tier holds the kernel to is the reference's formula.  Four fp32 roundings on either side (the difference, the
    2 / n factor, two products): 4 * 2^-24 relative per element, and exactly 0 outside the clamp."""
    cases, checked = R.cases(), 0
    for i, c in enumerate(cases):
        first, rows = golden["numeric_at"][i, 0]
        if first < 0:
            continue
        batch = R.make_batch(c["n_view"], c["n_frame"])
        index = torch.from_numpy(golden["sampled_idx"][i, :rows]).long()
        image, alpha = R.make_render(f"{R.case_key(c)}/r0", int(rows))
        i64, a64 = image.double().requires_grad_(True), alpha.double().requires_grad_(True)
        bg = float(torch.tensor(R.BG[0], dtype=torch.float32))
        loss = R.recon_loss_ref(i64, a64, batch["rgb"], batch["mask"], index, bg, R.LOSS["lambda_rgb"], R.LOSS["lambda_mask"])[0]
        loss.backward()
        for got, want in ((golden["d_image"][first:first + rows], i64.grad), (golden["d_alpha"][first:first + rows], a64.grad)):
            got = torch.from_numpy(got).double()
            assert bool(((got - want).abs() <= 4 * 2.0 ** -24 * want.abs()).all()), c
        outside = (image < 0) | (image > 1)
        assert bool(outside.any()) and bool((torch.from_numpy(golden["d_image"][first:first + rows])[outside] == 0).all())
        checked += 1
    assert checked == 17
