"""CLIP image pre-processing of rendered frames, host side (animate3d_amd/clip.py: ``resize_plan``, ``preprocess_frames``' argument checks)
and the oracle the GPU tier uses: tests/clip_pre_ref.py is held bit-equal to Pillow's resampler and within float32 rounding of
``transformers.CLIPImageProcessor()``, ``resize_plan``'s integers equal the restatement's, and the reference's own processor path agrees
through tests/golden/clip_preprocess.npz (made by tests/golden/make_clip_preprocess_goldens.py)."""
import os
import zlib

import numpy as np
import pytest
import torch

from animate3d_amd import clip
from tests import clip_pre_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_preprocess.npz")

# (in_h, in_w) -> (out_h, out_w): shortest edge to 224 (45 for the last).  224^2 and 224x300 skip both passes.
RESIZES = [((256, 256), (224, 224)), ((512, 512), (224, 224)), ((64, 64), (224, 224)), ((96, 160), (224, 373)), ((300, 256), (262, 224)),
           ((37, 29), (57, 45)), ((224, 224), (224, 224)), ((160, 96), (373, 224)), ((224, 300), (224, 300))]
KINDS = {"noise": R.noise_image, "smooth": R.smooth_image, "block": R.block_image}
# one float32 ulp at |x| <= 2.3 is 2.4e-7 and the processor takes a few float32 roundings (rescale, subtract, divide) where the table takes one
PROCESSOR_BAR = 1e-6


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("hw,out", RESIZES, ids=[f"{h}x{w}" for (h, w), _ in RESIZES])
def test_restatement_is_bit_equal_to_pillow(hw, out, kind):
    Image = pytest.importorskip("PIL.Image")
    (h, w), (oh, ow) = hw, out
    assert R.output_size(h, w, 45 if hw == (37, 29) else 224) == out
    img = KINDS[kind](h, w, seed=h + w)
    stats = []
    got = R.resize_u8(img, oh, ow, stats)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert len(stats) == (w != ow) + (h != oh)
    if kind == "block":                      # the clips are exercised: before them, every pass leaves [0, 255] in both directions
        for lo, hi in stats:
            assert lo < 0 and hi > 255, stats


@pytest.mark.parametrize("shape", [(256, 256, 224, 224), (512, 512, 224, 224), (64, 64, 224, 224), (96, 160, 224, 224), (160, 96, 224, 224),
                                   (300, 256, 224, 224), (224, 224, 224, 224), (224, 300, 224, 224), (37, 29, 28, 28), (1024, 768, 224, 224)],
                         ids=lambda s: "{}x{}-{}-{}".format(*s))
def test_resize_plan_equals_restatement(shape):
    h, w, size, crop = shape
    p = clip.resize_plan(h, w, size, crop, "cpu")
    oh, ow = R.output_size(h, w, size)
    assert (p.out_h, p.out_w) == (oh, ow) and (p.off_y, p.off_x) == R.crop_offsets(oh, ow, crop)
    spans = []
    for axis, n_in, n_out, off in (("x", w, ow, p.off_x), ("y", h, oh, p.off_y)):
        ksize, bounds, coef = getattr(p, "ksize_" + axis), getattr(p.host, "bounds_" + axis), getattr(p.host, "coef_" + axis)
        if n_in == n_out:                     # Pillow skips the pass
            assert ksize == 0 and bounds is None and coef is None and getattr(p, "coef_" + axis) is None
            continue
        want_k, want_b, want_c = R.coefficients(n_in, n_out)
        assert ksize == want_k and bounds.dtype == torch.int32 and coef.dtype == torch.int32
        assert np.array_equal(bounds.numpy(), want_b[off:off + crop]) and np.array_equal(coef.numpy(), want_c[off:off + crop])
        assert torch.equal(getattr(p, "coef_" + axis), coef) and torch.equal(getattr(p, "bounds_" + axis), bounds)
        spans.append(want_b[off:off + crop])
    # the tile's intermediate: the input rows from the first tap of the tile's first row to the last tap of its last row
    for tile_rows in (14, 7, crop):
        if p.ksize_y == 0:
            want = min(tile_rows, crop)
        else:
            b = spans[-1]
            want = max(int(b[min(t + tile_rows, crop) - 1].sum() - b[t, 0]) for t in range(0, crop, tile_rows))
        assert p.max_rows(tile_rows) == want
    assert p.table.dtype == torch.float32 and np.array_equal(p.host.table.numpy(), R.norm_table())
    assert clip.resize_plan(h, w, size, crop, "cpu") is p                         # cached: nothing is rebuilt or uploaded again


def test_normalisation_table_is_the_float64_formula_rounded_once():
    t = clip.resize_plan(256, 256, device="cpu").host.table.numpy()
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)       # CLIPImageProcessor()'s defaults
    for c in range(3):
        want = np.array([((v / 255.0) - mean[c]) / std[c] for v in range(256)], dtype=np.float64).astype(np.float32)
        assert np.array_equal(t[c], want)
    assert clip.OPENAI_CLIP_MEAN == mean == R.CLIP_MEAN and clip.OPENAI_CLIP_STD == std == R.CLIP_STD


def test_restatement_matches_clip_image_processor():
    Image = pytest.importorskip("PIL.Image")
    transformers = pytest.importorskip("transformers")
    proc = transformers.CLIPImageProcessor()
    assert tuple(proc.image_mean) == R.CLIP_MEAN and tuple(proc.image_std) == R.CLIP_STD
    worst = 0.0
    for (h, w), kind in (((256, 256), "noise"), ((300, 256), "block"), ((96, 160), "smooth"), ((224, 300), "noise"), ((512, 512), "block")):
        img = KINDS[kind](h, w, seed=3)
        want = proc([Image.fromarray(img)], return_tensors="np")["pixel_values"][0]
        got = R.pixel_values(R.preprocess_u8(img))
        assert got.shape == want.shape == (3, 224, 224)
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"[parity] restatement + table vs CLIPImageProcessor: max abs {worst:.3e}")
    assert worst <= PROCESSOR_BAR


@pytest.mark.parametrize("tag", ["small", "big"])
def test_restatement_matches_reference_golden(tag):
    """The reference's ``IPAdapterImageProcessor.encode_image`` pre-processing on seeded frames, recorded: needs neither Pillow nor transformers."""
    g = np.load(GOLDEN)
    (h, w), seed, size = g[f"{tag}_hw"], int(g[f"{tag}_seed"]), int(g[f"{tag}_size"])
    frame = R.golden_frame(int(h), int(w), seed)
    assert zlib.crc32(frame.tobytes()) == int(g[f"{tag}_crc"])                    # the seeded frame is the recorded one
    if tag == "small":
        assert np.array_equal(frame, g["small_rgb"])
    got = R.preprocess(frame[None], size, size)[1][0]
    err = float(np.abs(got.astype(np.float64) - g[f"{tag}_pixel_values"]).max())
    print(f"[parity] restatement vs the reference's processor path ({tag}): max abs {err:.3e}")
    assert got.shape == g[f"{tag}_pixel_values"].shape and err <= PROCESSOR_BAR


def test_quantisation_truncates_a_float32_product():
    x = R.ulp_image(16, 16, 0)
    want = (x * 255).astype(np.uint8)                                               # what the reference writes; defined for [0, 1]
    assert np.array_equal(R.quantise(x), want)
    assert (want == 0).any() and (want == 255).any()
    odd = np.array([np.nan, -0.5, -np.inf, 1.5, np.inf, 1.0, 0.0], np.float32)
    assert R.quantise(odd).tolist() == [0, 0, 0, 255, 255, 255, 0]


def test_argument_checks():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clip.preprocess_frames(torch.zeros(1, 64, 64, 3))                           # a CPU tensor
    with pytest.raises(RuntimeError):
        clip.preprocess_frames(torch.zeros(1, 64, 64, 3, dtype=torch.float16))      # not float32
    with pytest.raises(RuntimeError):
        clip.preprocess_frames(np.zeros((1, 64, 64, 3), np.float32))
    # a side too short for the crop: the resized frame is size x size and the crop larger
    with pytest.raises(ValueError, match="smaller than"):
        clip.resize_plan(64, 64, 28, 42, "cpu")
    with pytest.raises(ValueError):
        clip.resize_plan(0, 64, device="cpu")
    from animate3d_amd.sds import sds_guidance_loss
    with pytest.raises(ValueError, match="image_embeds or image_encoder"):
        sds_guidance_loss(None, None, torch.zeros(8, 16, 16, 3), torch.tensor([1]), torch.zeros(2, 1, 1), None, None, n_view=1, n_frame=8)
    enc = clip.CLIPVisionEncoderWithProjection(clip.CLIPTowerConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                                    num_attention_heads=4, image_size=28, patch_size=14, projection_dim=32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clip.encode_image_from_frames(enc, torch.zeros(1, 37, 29, 3))               # the tower and the frames live on the CPU


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """The C-ABI argument checks run before the first HIP call; the addresses are made up and never dereferenced, and no call here may pass."""
    from animate3d_amd import build, hip_ops
    build.build(verbose=False)
    lib = hip_ops.load_library()
    limit = lib.a3d_clip_preprocess_lds_limit()
    assert 0 < limit <= 160 * 1024
    P = 0x7F00_0010_0000

    def call(**kw):
        a = dict(rgb=P, n_src=1, in_h=64, in_w=64, s_img=64 * 64 * 3, s_y=64 * 3, s_x=3, s_c=1, index=None, n_img=1, crop=28, coef_x=P + 0x1000,
                 bounds_x=P + 0x2000, ksize_x=7, off_x=0, coef_y=P + 0x3000, bounds_y=P + 0x4000, ksize_y=7, off_y=0, tile_rows=14, max_rows=20,
                 table=P + 0x5000, dtype=0, pv=P + 0x6000, patch=None, ps=0, kp=0, u8=None)
        a.update(kw)
        return lib.a3d_clip_preprocess(None, *a.values())

    assert call(max_rows=limit // (3 * 28) + 1) == hip_ops.A3D_EUNSUPPORTED        # the tile's intermediate would not fit LDS
    for bad in (dict(pv=None), dict(dtype=3), dict(coef_x=None), dict(ksize_y=0, off_y=40), dict(ksize_x=0, off_x=-1), dict(rgb=P + 2),
                dict(pv=None, patch=P + 0x6000, ps=14, kp=587), dict(pv=None, patch=P + 0x6000, ps=14, kp=640, tile_rows=7),
                dict(pv=None, patch=P + 0x6000, ps=9, kp=640, tile_rows=9), dict(n_img=0), dict(max_rows=0)):
        assert call(**bad) == -1, bad
