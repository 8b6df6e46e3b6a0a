"""What ``MVVideoPipeline`` and ``VideoFrames`` decide on the host, without a GPU: every refusal is raised before any device work (the
pipeline here is built over no modules at all, so touching one would fail with another exception), the accepted image forms, the
``output_type`` table, and the files."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from animate3d_amd import pipeline as P
from animate3d_amd.video import VideoFrames
from tests import pipeline_ref as R

IDS = torch.ones(1, 77, dtype=torch.int64)


def _pipe(**kw):
    return P.MVVideoPipeline(None, None, None, None, None, **kw)


def _images(n=4, h=16, w=16, c=3):
    return np.random.default_rng(0).integers(0, 256, (n, h, w, c), dtype=np.uint8)


def _call(pipe=None, **kw):
    args = dict(prompt_ids=IDS, negative_prompt_ids=IDS, ip_adapter_image=_images())
    args.update(kw)
    return (pipe or _pipe())(**args)


@pytest.mark.parametrize("name,value", [
    ("guidance_scale", 1.0), ("guidance_scale", 0.0), ("i2v_similarity_init", {"strength": 0.5, "origin_prob": 0.1}), ("eta", 0.5),
    ("callback", print), ("callback_steps", 1), ("callback_on_step_end", print), ("callback_on_step_end_tensor_inputs", ["latents"]),
    ("clip_skip", 1), ("cross_attention_kwargs", {"scale": 1.0, "other": 2}), ("cross_attention_kwargs", {"gligen": {}}),
    ("ip_adapter_image_embeds", [torch.zeros(1, 1, 4)]),
])
def test_refused_arguments_name_themselves(name, value):
    with pytest.raises(NotImplementedError, match=name + r" = .*no released config uses it, not built"):
        _call(**{name: value})


def test_accepted_spellings_of_the_refusable_arguments_pass_the_checks():
    """eta = 0, null callbacks and ``{"scale": s}`` get past the argument checks: the call then fails on the absent UNet, not before."""
    with pytest.raises(AttributeError):
        _call(eta=0.0, callback=None, clip_skip=None, cross_attention_kwargs={"scale": 0.8}, ip_adapter_image_embeds=None)
    with pytest.raises(TypeError, match="unexpected keyword argument 'strength'"):
        _call(strength=0.5)


def test_free_init_switches():
    pipe = _pipe()
    assert not pipe.free_init_enabled
    pipe.enable_free_init(method="butterworth", num_iters=3, use_fast_sampling=False, order=4, spatial_stop_frequency=0.25,
                          temporal_stop_frequency=0.25)
    assert pipe.free_init_enabled
    pipe.disable_free_init()
    assert not pipe.free_init_enabled
    with pytest.raises(NotImplementedError, match="use_fast_sampling"):
        pipe.enable_free_init(use_fast_sampling=True)
    with pytest.raises(NotImplementedError, match="box"):
        pipe.enable_free_init(method="box")
    with pytest.raises(ValueError):
        pipe.enable_free_init(num_iters=0)


def test_prompt_needs_a_tokenizer_and_ids_bypass_it():
    with pytest.raises(ValueError, match="tokenizer"):
        _pipe()("a rotating teapot", ip_adapter_image=_images())
    with pytest.raises(ValueError, match="negative_prompt_ids"):
        _pipe()(prompt_ids=IDS, ip_adapter_image=_images())
    with pytest.raises(ValueError, match="one of"):
        _call(prompt="both")
    with pytest.raises(ValueError, match="one of"):
        _pipe()(ip_adapter_image=_images())
    with pytest.raises(ValueError, match="prompt_ids"):
        _call(prompt_ids=torch.ones(77, dtype=torch.int64))
    seen = []

    class Tok:
        model_max_length = 77

        def __call__(self, text, **kw):
            seen.append((text, kw))
            return type("Enc", (), {"input_ids": IDS})()

    with pytest.raises(AttributeError):                     # tokenised (on the host), then the absent modules
        _pipe(tokenizer=Tok())("a rotating teapot", negative_prompt="blurry", ip_adapter_image=_images())
    assert [s[0] for s in seen] == ["a rotating teapot", "blurry"]
    assert seen[0][1] == dict(padding="max_length", max_length=77, truncation=True, return_tensors="pt")


def test_image_forms_and_sizes():
    img = _images(4, 16, 24)
    pil = [Image.fromarray(i) for i in img]
    assert np.array_equal(P.condition_images(pil), img)
    assert np.array_equal(P.condition_images(pil, 16, 24), img)
    rgba = [Image.fromarray(np.concatenate([i, np.full((16, 24, 1), 77, np.uint8)], axis=-1)) for i in img]
    assert np.array_equal(P.condition_images(rgba), img)                        # converted to RGB as load_image does
    grey = [Image.fromarray(i[..., 0]) for i in img]
    assert P.condition_images(grey).shape == (4, 16, 24, 3)
    assert P.condition_images(img) is img and P.condition_images(_images(c=4)).shape[3] == 4
    t = torch.from_numpy(img)
    assert P.condition_images(t) is t
    with pytest.raises(ValueError, match="resize the images first"):
        P.condition_images(img, 32, 24)
    with pytest.raises(ValueError, match="resize the images first"):
        _call(ip_adapter_image=img, height=16, width=16)
    with pytest.raises(ValueError, match="different sizes"):
        _call(ip_adapter_image=pil[:3] + [Image.fromarray(_images(1, 16, 16)[0])])
    with pytest.raises(ValueError, match="uint8"):
        P.condition_images(img.astype(np.float32) / 255)
    with pytest.raises(ValueError, match="uint8"):
        P.condition_images(img[0])
    with pytest.raises(ValueError, match="one condition image per view"):
        _call(ip_adapter_image=_images(3))
    with pytest.raises(TypeError):
        P.condition_images("teapot.png")
    with pytest.raises(ValueError, match="num_frames"):
        _call(num_frames=1)


def test_output_type_table():
    assert P.OUTPUT_TYPES == ("latent", "u8", "pil", "np", "pt")
    for kind in P.OUTPUT_TYPES:
        P.check_output_type(kind)
    for kind in ("gif", "PIL", None):
        with pytest.raises(ValueError, match="does not exist. Please choose one of"):
            _call(output_type=kind)
    vid = torch.rand(2, 3, 3, 4, 5, generator=torch.Generator().manual_seed(1)) * 2.4 - 1.2
    as_np, as_pt = P.float_frames(vid, "np"), P.float_frames(vid, "pt")
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float32 and as_np.shape == (2, 3, 4, 5, 3)
    assert np.array_equal(as_np, R.video_to_np_ref(vid))
    assert as_pt.dtype == torch.float32 and tuple(as_pt.shape) == (2, 3, 3, 4, 5)
    assert np.array_equal(as_pt.permute(0, 1, 3, 4, 2).numpy(), as_np)
    with pytest.raises(ValueError):
        P.float_frames(vid, "pil")
    out = P.MVVideoPipelineOutput(frames=as_np)
    assert out.frames is as_np


def _frames(n=2, F=3, H=4, W=6):
    return VideoFrames(torch.from_numpy(np.random.default_rng(4).integers(0, 256, (n, F, H, W, 3), dtype=np.uint8)))


def test_view_frame_numbering_is_split_gifs(tmp_path):
    vf = _frames()
    paths = vf.write_view_frames(str(tmp_path / "views"))
    assert sorted(os.listdir(tmp_path / "views"), key=lambda s: int(s[:-4])) == [f"{i}.png" for i in range(6)]
    host = vf.numpy()
    for view in range(2):
        for frame in range(3):
            path = str(tmp_path / "views" / R.split_gif_name(view, frame, 3))
            assert path == paths[view * 3 + frame]
            with Image.open(path) as im:
                assert im.mode == "RGB" and np.array_equal(np.asarray(im), host[view, frame])      # lossless
    assert np.array_equal(vf.strip().numpy(), R.strip_ref(host))
    assert [[np.array_equal(np.asarray(im), host[v, f]) for f, im in enumerate(view)] for v, view in enumerate(vf.pil())] == [[True] * 3] * 2


def test_gif_holds_the_strip(tmp_path):
    vf = _frames()
    path = vf.write_gif(str(tmp_path / "out" / "sample.gif"), fps=10)
    with Image.open(path) as im:
        assert im.format == "GIF" and im.n_frames == 3 and im.size == (2 * 6, 4)
        assert im.info["duration"] == 100 and im.info.get("loop") == 0


def test_video_frames_refuses_other_layouts():
    with pytest.raises(ValueError):
        VideoFrames(torch.zeros(2, 3, 4, 6, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        VideoFrames(torch.zeros(2, 3, 4, 6, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _frames().with_alpha(torch.zeros(2, 3, 4, 6, dtype=torch.uint8))
