"""``MVVideoPipeline`` on the MI355X: one object against the same public functions called by hand, and its byte outputs against
tests/pipeline_ref.py.  Small models with synthetic weights: the two-level UNet of tests/test_denoise_loop.py's FreeInit test at its 16 x 16
latent (128 x 128 images), the small CLIP towers of tests/test_clip.py / tests/test_clip_preprocess_gpu.py at the widths the UNet reads (768,
1024), the SD VAE; n = 2 views, F = 3 frames, 2 inference steps, a seeded CPU generator.  The pipeline adds no arithmetic of its own to the
latents, so they are compared for equality; the bytes are the reference chain's, for equality as well."""
import numpy as np
import pytest
import torch

from animate3d_amd import clip, denoise, embeddings, frames, video
from animate3d_amd.config import UNetConfig
from animate3d_amd.pipeline import MVVideoPipeline, MVVideoPipelineOutput
from animate3d_amd.unet import MVUNetMotionModel
from animate3d_amd.vae import AutoencoderKLDecoder, AutoencoderKLEncoder
from tests import pipeline_ref as R

pytestmark = pytest.mark.gpu

N, F, SIDE, STEPS, SCALE = 2, 3, 128, 2, 7.5
ARCH = dict(block_out_channels=(320, 640), down_has_attn=(True, False), layers_per_block=1)
TEXT = dict(hidden_size=768, intermediate_size=1536, num_hidden_layers=1, num_attention_heads=12, vocab_size=100, max_position_embeddings=77)
VISION = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=14,
              projection_dim=1024, hidden_act="gelu")


@pytest.fixture(scope="module")
def pipe():
    torch.manual_seed(0)
    unet = MVUNetMotionModel(UNetConfig(**ARCH), num_views=N, device="cuda").init_synthetic(seed=1).to(torch.bfloat16).eval()
    enc = AutoencoderKLEncoder(device="cuda").init_synthetic(seed=2).eval()
    dec = AutoencoderKLDecoder(device="cuda").init_synthetic(seed=3).eval()
    text = clip.CLIPTextEncoder(clip.CLIPTowerConfig(**TEXT), device="cuda").eval()
    vision = clip.CLIPVisionEncoderWithProjection(clip.CLIPTowerConfig(**VISION), device="cuda").eval()
    return MVVideoPipeline(unet, enc, dec, text, vision)


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(21)
    images = torch.randint(0, 256, (N, SIDE, SIDE, 3), generator=g, dtype=torch.uint8)
    ids = torch.randint(1, 100, (1, 77), generator=g)
    neg = torch.randint(1, 100, (1, 77), generator=g)
    return dict(ip_adapter_image=images, prompt_ids=ids, negative_prompt_ids=neg, num_frames=F, num_videos_per_prompt=N,
                num_inference_steps=STEPS, guidance_scale=SCALE)


def _by_hand(pipe, inputs, seed, free_init_iters=None):
    """The documented order, written out with the public functions."""
    gen = torch.Generator().manual_seed(seed)
    pe, ne = clip.encode_prompt(pipe.text_encoder, inputs["prompt_ids"].cuda(), inputs["negative_prompt_ids"].cuda())
    prompt_embeds = torch.cat([ne.repeat(N, 1, 1), pe.repeat(N, 1, 1)])
    planar, unit = video.images_in_u8(inputs["ip_adapter_image"].cuda(), unit=True)
    e, zero = clip.encode_image_from_frames(pipe.image_encoder, unit)
    image_embeds = torch.cat([zero, e])
    first = pipe.vae_encoder.encode_latents(planar, gen)                                  # draw 1: the posterior sample
    latents, first = denoise.prepare_latents(first, F, gen, "cuda", torch.float32)        # draw 2: frames 1..
    camera = embeddings.get_camera(N).to(device="cuda", dtype=prompt_embeds.dtype)
    kw = dict(num_inference_steps=STEPS, guidance_scale=SCALE)
    if free_init_iters is None:
        return denoise.denoise_loop(pipe.unet, latents, first, prompt_embeds, image_embeds, camera, **kw)
    return denoise.denoise_free_init(pipe.unet, latents, first, prompt_embeds, image_embeds, camera, num_iters=free_init_iters,
                                     generator=gen, **kw)                                 # draw 3: FreeInit's fresh noise


@pytest.fixture(scope="module")
def latents(pipe, inputs):
    """The latents of seed 5 without FreeInit, and the fp32 video decoded from them: computed once, left unchanged."""
    pipe.disable_free_init()
    out = pipe(**inputs, generator=torch.Generator().manual_seed(5), output_type="latent")
    assert isinstance(out, MVVideoPipelineOutput)
    return out.frames, pipe.vae_decoder.decode_latents(out.frames).cpu()


def test_latents_equal_the_functions_called_by_hand(pipe, inputs, latents):
    got = latents[0]
    want = _by_hand(pipe, inputs, seed=5)
    assert got.dtype == torch.float32 and got.shape == (N, 4, F, SIDE // 8, SIDE // 8) and torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert not torch.equal(got, _by_hand(pipe, inputs, seed=6))                           # the generator reaches the result


def test_latents_equal_by_hand_with_free_init(pipe, inputs):
    pipe.enable_free_init(num_iters=2)
    try:
        got, = pipe(**inputs, generator=torch.Generator().manual_seed(8), output_type="latent", return_dict=False)
    finally:
        pipe.disable_free_init()
    assert torch.equal(got, _by_hand(pipe, inputs, seed=8, free_init_iters=2))


def test_byte_outputs(pipe, inputs, latents):
    lat, vid = latents
    want = R.video_to_u8_ref(vid)
    run = lambda kind: pipe(**inputs, generator=torch.Generator().manual_seed(5), output_type=kind).frames
    u8 = run("u8")
    assert isinstance(u8, video.VideoFrames) and u8.u8.is_cuda and tuple(u8.u8.shape) == (N, F, SIDE, SIDE, 3)
    diff = int((u8.numpy() != want).sum())
    print(f"[parity] pipeline output_type='u8' vs the reference chain on decode_latents: {diff} of {want.size} bytes differ "
          f"({np.unique(want).size} distinct byte values, {float(((want == 0) | (want == 255)).mean()):.3f} of them clamped)")
    assert diff == 0
    assert torch.equal(run("u8").u8, u8.u8)                                               # equal seeds: equal bytes
    assert np.array_equal(u8.strip().cpu().numpy(), R.strip_ref(want))
    assert np.array_equal(pipe.vae_decoder.decode_frames_u8(lat, strip=True).cpu().numpy(), R.strip_ref(want))
    pil = run("pil")
    assert len(pil) == N and all(len(v) == F for v in pil) and pil[0][0].mode == "RGB" and pil[0][0].size == (SIDE, SIDE)
    assert np.array_equal(np.stack([np.stack([np.asarray(im) for im in v]) for v in pil]), want)
    as_np = run("np")
    assert as_np.dtype == np.float32 and as_np.shape == (N, F, SIDE, SIDE, 3) and as_np.min() >= 0 and as_np.max() <= 1
    assert np.array_equal(as_np, R.video_to_np_ref(vid)) and np.array_equal(R.numpy_to_u8_ref(as_np), want)
    as_pt = run("pt")
    assert as_pt.is_cuda and as_pt.dtype == torch.float32 and tuple(as_pt.shape) == (N, F, 3, SIDE, SIDE)
    assert np.array_equal(as_pt.cpu().permute(0, 1, 3, 4, 2).numpy(), as_np)


def test_frames_reach_the_4d_stage_unchanged(pipe, latents, tmp_path):
    from PIL import Image
    vf = video.VideoFrames(pipe.vae_decoder.decode_frames_u8(latents[0]))
    mask = (torch.rand(N, F, SIDE, SIDE, generator=torch.Generator().manual_seed(2)) > 0.5).to(torch.uint8).cuda() * 255
    fs = vf.with_alpha(mask)
    assert isinstance(fs, frames.FrameSet) and (fs.n_view, fs.n_frame) == (N, F)
    assert torch.equal(fs.rgba8[..., :3].reshape(N, F, SIDE, SIDE, 3), vf.u8) and torch.equal(fs.rgba8[..., 3].reshape(N, F, SIDE, SIDE), mask)
    paths = vf.write_view_frames(str(tmp_path))
    assert [p.split("/")[-1] for p in paths] == [f"{i}.png" for i in range(N * F)]
    host_mask = mask.cpu().numpy().reshape(N * F, SIDE, SIDE)
    for i, path in enumerate(paths):                                                      # the segmentation step's part: the alpha
        im = Image.open(path).convert("RGB")
        im.putalpha(Image.fromarray(host_mask[i]))
        im.save(path)
    back = frames.load_frames(str(tmp_path), SIDE, SIDE, n_view=N, n_frame=F)
    assert torch.equal(back.rgba8, fs.rgba8)
