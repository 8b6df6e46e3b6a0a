"""CPU tier of the 4-D stage's regularisers: the refusals that need no device, how ``training_step`` calls the two functions and adds their
terms (with counting stand-ins in place of the kernels), and the golden of the reference's own ``training_step`` and ``tv_loss``
(tests/golden/make_stage4d_reg_goldens.py) against the float64 restatement the GPU tier holds the kernels to."""
import os
import random

import numpy as np
import pytest
import torch

from animate3d_amd import stage4d
from tests import stage4d_ref as R
from tests import stage4d_reg_ref as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage4d_reg.npz")
IMG = dict(lambda_tv=1.0, lambda_depth_tv=1.0, lambda_sparsity=1.0)
GS = dict(lambda_position=1.0, lambda_scales=1.0, lambda_opacity=1.0)


def test_only_the_normal_tv_weight_is_still_refused():
    assert stage4d.UNSUPPORTED_LAMBDAS == ("lambda_normal_tv",)
    assert set(stage4d.IMAGE_REG_LAMBDAS + stage4d.GAUSSIAN_REG_LAMBDAS) == set(G.LAMBDAS) == {name for name, _ in stage4d.REG_ORDER}


def _image_ops(B=2, h=4, w=4):
    return torch.zeros(B, 3, h, w), torch.zeros(B, 1, h, w), torch.zeros(B, 1, h, w)


def test_image_regularizers_refusals_without_a_device():
    image, depth, alpha = _image_ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.image_regularizers(image, depth, alpha, **IMG)                           # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.image_regularizers(image, depth, alpha[:, 0], **IMG)                     # [B, H, W] alpha is a legal shape
    for h, w in ((1, 4), (4, 1), (1, 1)):                                               # the reference divides by zero
        ops = _image_ops(h=h, w=w)
        with pytest.raises(ValueError, match="H >= 2 and W >= 2"):
            stage4d.image_regularizers(*ops, **IMG)
        with pytest.raises(ValueError, match="H >= 2 and W >= 2"):
            stage4d.image_regularizers(*ops, lambda_tv=0.0, lambda_depth_tv=0.5, lambda_sparsity=0.0)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                      # sparsity alone has no such limit
            stage4d.image_regularizers(*ops, lambda_tv=0.0, lambda_depth_tv=0.0, lambda_sparsity=1.0)
    for bad in (dict(image=image[:, :2]), dict(depth=depth[:, 0]), dict(depth=depth[:1]), dict(alpha=alpha[..., :2]), dict(image=image[0])):
        ops = dict(dict(image=image, depth=depth, alpha=alpha), **bad)
        with pytest.raises(ValueError):
            stage4d.image_regularizers(ops["image"], ops["depth"], ops["alpha"], **IMG)
    with pytest.raises(TypeError):
        stage4d.image_regularizers(image, None, alpha, **IMG)                            # None only where the weight is 0
    with pytest.raises(ValueError, match="every weight is 0"):
        stage4d.image_regularizers(image, depth, alpha, lambda_tv=0.0, lambda_depth_tv=0.0, lambda_sparsity=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.image_regularizers(image.double(), None, None, lambda_tv=1.0, lambda_depth_tv=0.0, lambda_sparsity=0.0)


def test_gaussian_regularizers_refusals_without_a_device():
    means, scales, scaling, opacity = torch.zeros(2, 5, 3), torch.zeros(2, 5, 3), torch.zeros(5, 3), torch.zeros(5, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.gaussian_regularizers(means, scales, scaling, opacity, **GS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.gaussian_regularizers(means, scales[:1].expand(2, 5, 3), scaling, opacity[:, 0], **GS)
    for bad in (dict(means=means[0]), dict(scales=scales[:1]), dict(scaling=scaling[:4]), dict(opacity=opacity[:4]), dict(means=means[..., :2]),
                dict(opacity=torch.zeros(5, 2))):
        ops = dict(dict(means=means, scales=scales, scaling=scaling, opacity=opacity), **bad)
        with pytest.raises(ValueError):
            stage4d.gaussian_regularizers(ops["means"], ops["scales"], ops["scaling"], ops["opacity"], **GS)
    with pytest.raises(TypeError):
        stage4d.gaussian_regularizers(means, scales, scaling, None, **GS)
    with pytest.raises(ValueError, match="every weight is 0"):
        stage4d.gaussian_regularizers(means, scales, scaling, opacity, lambda_position=0.0, lambda_scales=0.0, lambda_opacity=0.0)


# ---- training_step with stand-ins for the three kernels

class _StandIns:
    """Counts the calls of the two regulariser functions and hands out fixed terms; the reconstruction loss is a fixed number too."""
    RECON = 0.1
    # times their weights about 2^25, 1, -2^25, 1, 1, 1: next to 2^25 a 1 is below half an ulp, so the fp32 total tells the order
    UNWEIGHTED = {k: v / G.LAMBDAS[k] for k, v in dict(lambda_position=2.0 ** 25, lambda_opacity=1.0, lambda_sparsity=-2.0 ** 25,
                                                       lambda_scales=1.0, lambda_tv_loss=1.0, lambda_depth_tv_loss=1.0).items()}

    def __init__(self, monkeypatch):
        self.image_calls, self.gaussian_calls = [], []
        self.carriers = []
        monkeypatch.setattr(stage4d, "masked_recon_loss", self.recon)
        monkeypatch.setattr(stage4d, "image_regularizers", self.image)
        monkeypatch.setattr(stage4d, "gaussian_regularizers", self.gaussian)

    def _leaf(self, value):
        self.carriers.append(torch.tensor(float(value), requires_grad=True))
        return self.carriers[-1] * 1.0

    def recon(self, image, alpha, rgb, mask, index, **kw):
        return self._leaf(self.RECON), torch.tensor(0.01), torch.tensor(0.02)

    def image(self, image, depth, alpha, **kw):
        self.image_calls.append(dict(kw, operands=(image, depth, alpha)))
        return (self._leaf(-1.0), *(torch.tensor(self.UNWEIGHTED[k] if kw[a] else 0.0) for k, a in
                                    zip(stage4d.IMAGE_REG_LAMBDAS, ("lambda_tv", "lambda_depth_tv", "lambda_sparsity"))))

    def gaussian(self, means, scales, scaling, opacity, **kw):
        self.gaussian_calls.append(dict(kw, operands=(means, scales, scaling, opacity)))
        return (self._leaf(-2.0), *(torch.tensor(self.UNWEIGHTED[k] if kw[k] else 0.0) for k in stage4d.GAUSSIAN_REG_LAMBDAS))


def _step(loss_cfg, calls=None):
    gaussians = stage4d.Gaussians(R.make_means("xyz", 1)[0], *G.make_static()[:1], None, G.make_static()[1], None, 0)

    def render(field, gs, c2w, fovy, timestamps, height, width, bg, **kwargs):
        nb = c2w.shape[0]
        image, alpha = R.make_render("host", nb)
        out = stage4d.RenderOutput(image=image, alpha=alpha, comp_depth=G.make_depth("host", nb).permute(0, 2, 3, 1),
                                   means3D=R.make_means("host", nb), scales=G.make_scales("host", nb))
        if calls is not None:
            calls.append(out)
        return out
    return stage4d.training_step(None, gaussians, R.make_batch(2, 4), loss=loss_cfg, global_step=G.STEP, n_view=2, n_frame=4,
                                 progressive_iter_per_frame=R.PROGRESSIVE, bg=R.BG, rng=random.Random(0), render=render), gaussians


def test_all_zero_step_calls_neither_function(monkeypatch):
    s = _StandIns(monkeypatch)
    out, _ = _step(dict(R.LOSS, lambda_arap=0.0))
    assert not s.image_calls and not s.gaussian_calls and set(out) == {"loss", "loss_rgb", "loss_mask"}
    assert float(out["loss"].detach()) == float(torch.tensor(_StandIns.RECON))
    out, _ = _step(dict(lambda_rgb=100.0, lambda_mask=100.0))                           # a config without the keys at all
    assert not s.image_calls and not s.gaussian_calls and set(out) == {"loss", "loss_rgb", "loss_mask"}


@pytest.mark.parametrize("name", list(G.LAMBDAS))
def test_one_weight_calls_one_function_with_that_weight_only(monkeypatch, name):
    """The refusal is lifted: on the parent commit this raises NotImplementedError."""
    s = _StandIns(monkeypatch)
    renders = []
    out, gaussians = _step(dict(R.LOSS, lambda_arap=0.0, **{name: G.LAMBDAS[name]}), renders)
    is_image = name in stage4d.IMAGE_REG_LAMBDAS
    assert (len(s.image_calls), len(s.gaussian_calls)) == ((1, 0) if is_image else (0, 1))
    call = (s.image_calls if is_image else s.gaussian_calls)[0]
    weights = {k: v for k, v in call.items() if k != "operands"}
    assert sorted(weights.values()) == [0.0, 0.0, G.LAMBDAS[name]]
    assert set(out) == {"loss", "loss_rgb", "loss_mask", G.RETURNED[name]}
    assert not out[G.RETURNED[name]].requires_grad
    assert float(out[G.RETURNED[name]]) == float(torch.tensor(_StandIns.UNWEIGHTED[name]) * G.LAMBDAS[name])
    r = renders[-1]
    given = [t for t in call["operands"] if t is not None]                              # the operand of a zero weight is not handed over
    want = {"lambda_tv_loss": [r["image"]], "lambda_depth_tv_loss": [r["image"], r["comp_depth"].permute(0, 3, 1, 2)],
            "lambda_sparsity": [r["image"], r["alpha"]], "lambda_position": [r["means3D"]], "lambda_scales": [r["scales"]],
            "lambda_opacity": [gaussians.scaling, gaussians.opacity]}[name]
    assert len(given) == len(want) and all(torch.equal(a, b) for a, b in zip(given, want))
    if name == "lambda_depth_tv_loss":
        assert given[1].shape == (6, 1, R.H, R.W) and given[1].is_contiguous()


def test_terms_are_added_in_the_reference_order_and_the_gradient_reaches_every_call(monkeypatch):
    s = _StandIns(monkeypatch)
    out, _ = _step(dict(R.LOSS, lambda_arap=0.0, **G.LAMBDAS))
    assert len(s.image_calls) == len(s.gaussian_calls) == 1
    weighted = {k: torch.tensor(v) * G.LAMBDAS[k] for k, v in _StandIns.UNWEIGHTED.items()}

    def total(order):
        value = torch.tensor(_StandIns.RECON)
        for k in order:
            value = value + weighted[k]
        return float(value)
    reference_order = ("lambda_position", "lambda_opacity", "lambda_sparsity", "lambda_scales", "lambda_tv_loss", "lambda_depth_tv_loss")
    grouped = stage4d.GAUSSIAN_REG_LAMBDAS + stage4d.IMAGE_REG_LAMBDAS                  # what adding the two calls' sums would give
    assert total(reference_order) != total(grouped) and total(reference_order) != total(tuple(reversed(reference_order)))
    assert float(out["loss"].detach()) == total(reference_order)
    assert list(out)[3:] == [G.RETURNED[k] for k in reference_order]
    out["loss"].backward()
    assert len(s.carriers) == 3 and all(float(c.grad) == 1.0 for c in s.carriers)       # the reconstruction loss and both calls' `loss`


def test_tv_weight_on_a_one_row_image_raises_before_anything_is_rendered():
    gaussians = stage4d.Gaussians(R.make_means("xyz", 1)[0], None, None, None, None, 0)

    def render(*args, **kwargs):
        raise AssertionError("rendered")
    for name, (h, w) in (("lambda_tv_loss", (1, 4)), ("lambda_depth_tv_loss", (4, 1))):
        with pytest.raises(ValueError, match="H >= 2 and W >= 2"):
            stage4d.training_step(None, gaussians, R.make_batch(2, 4, h, w), loss=dict(R.LOSS, lambda_arap=0.0, **{name: 0.5}), global_step=0,
                                  n_view=2, n_frame=4, progressive_iter_per_frame=10, bg=R.BG, render=render)


def test_negative_weight_raises():
    with pytest.raises(ValueError, match="lambda_sparsity"):
        stage4d.training_step(None, None, {}, loss=dict(R.LOSS, lambda_sparsity=-0.1), global_step=0, n_view=2, n_frame=4,
                              progressive_iter_per_frame=10, bg=R.BG)


# ---- the golden

def test_golden_is_the_float64_restatement():
    """What the reference logs per term, and its own fp32 gradients with respect to the last render's leaves and the opacity, against
    tests/stage4d_reg_ref in float64 on the same inputs: what the GPU tier holds the kernels to is the reference's formula.  Relative
    norms against 2^-18: the reference works in fp32 (2^-24 per rounding), and a total-variation gradient is a difference of differences
    of values up to 8 with typical results near 0.5, which costs up to four more bits; a wrong formula misses by whole percents."""
    golden = dict(np.load(GOLDEN))
    cases = G.cases()
    assert len(cases) == int(golden["n_cases"]) == 28
    bound = 2.0 ** -18

    def rel(a, b):
        return float((a.double() - b).norm() / b.norm())
    for i, c in enumerate(cases):
        loss_cfg = G.case_loss(c)
        r = int(c["guidance"])
        nb = int(golden["render_b"][i, r])
        assert nb == (R.N_RANDOM_CAMERA if c["guidance"] else 6) and int(golden["render_b"][i, 1 - r] > 0) == r
        key = f"{G.case_key(c)}/r{r}"
        image, alpha = R.make_render(key, nb)
        leaves = [t.double().requires_grad_(True) for t in (image, G.make_depth(key, nb), alpha, R.make_means(key, nb), G.make_scales(key, nb))]
        scaling, opacity = G.make_static()
        o64 = opacity.double().requires_grad_(True)
        lam_i = tuple(loss_cfg[k] for k in stage4d.IMAGE_REG_LAMBDAS)
        lam_g = tuple(loss_cfg[k] for k in stage4d.GAUSSIAN_REG_LAMBDAS)
        img = G.image_reg_ref(*leaves[:3], lam_i)
        gs = G.gaussian_reg_ref(*leaves[3:], scaling, o64, lam_g)
        term = dict(zip(stage4d.IMAGE_REG_LAMBDAS + stage4d.GAUSSIAN_REG_LAMBDAS, (*img[1:], *gs[1:])))
        for j, name in enumerate(G.LAMBDAS):
            if name in c["on"]:
                want = term[name].detach() * (loss_cfg[name] if G.LOGGED[name][1] else 1.0)
                assert rel(torch.tensor(golden["logged"][i, j]), want) <= bound, (c, name)
        (img[0] + gs[0]).backward()
        # the depth, the scales and the opacity get their gradient from these terms alone; the image and alpha also from the
        # reconstruction or guidance loss, the means from the ARAP stub: tests/test_stage4d_host.py's ground
        for name, leaf in (("depth", leaves[1]), ("scales", leaves[4])):
            gold = torch.from_numpy(golden[f"d_{name}"][i, r, :nb])
            if leaf.grad is None or not bool(leaf.grad.any()):
                assert not gold.any(), (c, name)
            else:
                assert rel(gold, leaf.grad) <= bound, (c, name)
        gold = torch.from_numpy(golden["d_opacity"][i])
        assert (rel(gold, o64.grad) <= bound) if "lambda_opacity" in c["on"] else not gold.any(), c
        if not c["arap"] and "lambda_position" in c["on"]:
            assert rel(torch.from_numpy(golden["d_means"][i, r, :nb]), leaves[3].grad) <= bound, c
