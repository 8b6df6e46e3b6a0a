"""``MVVideoPipeline.__call__`` and tests/pipeline_ref.py against vectors produced by the REFERENCE's own statements
(tests/golden/pipeline_call.npz, made by tests/golden/make_pipeline_call_goldens.py): ``encode_image``, ``encode_latents``,
``prepare_latents``, ``get_camera``, the loop statement, ``decode_latents`` and ``tensor2vid`` of animatediff/pipelines/pipeline.py, run in
``__call__``'s order with the stand-ins of tests/pipeline_ref.py and tests/sds_stub.py.  Here the pipeline object runs over the same
stand-ins, on the CPU; of the package only ``video.images_in_u8`` (a kernel) is replaced, by its restatement.  What the vectors pin is the
host-side ordering: which half is unconditional, the per-view repeat, what the VAE and the CLIP tower are fed, and the order in which one
generator serves the posterior sample, the noise of frames 1.. and FreeInit's fresh noise.

Bars.  Everything in front of the loop is the same float32 operations in the same order: equality (the camera: 1e-6, ``embeddings.get_camera``
computes it by other formulas than the reference's).  The loop's result: rtol 1e-4 / atol 1e-5, the bar of tests/test_denoise_loop.py for the
same comparison (the fused step's restatement sums in another order than the scheduler).  The bytes of the pipeline's own latents can then
differ from the recorded ones only where a value lies that close to a rounding tie: by one at most; from the RECORDED latents they are equal."""
import os

import numpy as np
import pytest
import torch

from animate3d_amd import pipeline as P
from animate3d_amd.video import VideoFrames
from tests import pipeline_ref as R
from tests.sds_stub import stub_unet
from tests.torch_ops import TorchRefOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_call.npz")


@pytest.fixture(scope="module")
def gold():
    data = np.load(GOLDEN)
    return {k: data[k] for k in data.files}


def test_restatements_reproduce_the_reference_chain(gold):
    images, video = gold["images"], torch.from_numpy(gold["video"])
    assert np.array_equal(R.video_to_u8_ref(video), gold["frames_u8"]) and np.array_equal(R.video_to_np_ref(video), gold["frames_np"])
    dec = R.StubDecoderHalf()
    assert torch.equal(dec.decode_latents(torch.from_numpy(gold["final"])), video)
    assert np.array_equal(dec.decode_frames_u8(torch.from_numpy(gold["final"])).numpy(), gold["frames_u8"])
    assert 0 in gold["frames_u8"] and 255 in gold["frames_u8"] and np.unique(gold["frames_u8"]).size > 200       # both clamps and the range between
    n = images.shape[0]
    first = R.StubEncoderHalf().encode_latents(R.images_in_ref(images), torch.Generator().manual_seed(int(gold["cfg"][6])))
    assert torch.equal(first, torch.from_numpy(gold["first"])[:, :, 0])
    assert torch.equal(R.stub_image_embeds(R.unit_ref(images)), torch.from_numpy(gold["image_embeds"])[n:])


class _UNet:
    device = torch.device("cpu")
    ops = TorchRefOps(torch.float32)

    def __init__(self):
        self.samples, self.cameras = [], []

    def __call__(self, sample, t, **kw):
        self.samples.append(sample.clone())
        self.cameras.append(kw["camera"].clone())
        return stub_unet(sample, t, **kw)


class _ImageEncoder:
    def encode_frames(self, rgb, image_index=None):
        assert image_index is None
        self.rgb = rgb
        return type("Out", (), {"image_embeds": R.stub_image_embeds(rgb)})()


def _pipeline(monkeypatch):
    monkeypatch.setattr(P, "images_in_u8", lambda u8, unit=False: (R.images_in_ref(u8.numpy()), R.unit_ref(u8.numpy())))
    unet, enc = _UNet(), _ImageEncoder()
    return P.MVVideoPipeline(unet, R.StubEncoderHalf(), R.StubDecoderHalf(), R.stub_text_encoder, enc), unet, enc


@pytest.mark.parametrize("form", ["numpy", "pil", "tensor"])
def test_call_reproduces_the_reference_order(gold, monkeypatch, form):
    n, F, side, steps, scale, iters, seed, ncalls = gold["cfg"].tolist()
    n, F, side, steps, iters, seed = int(n), int(F), int(side), int(steps), int(iters), int(seed)
    pipe, unet, enc = _pipeline(monkeypatch)
    pipe.enable_free_init(num_iters=iters)
    images = gold["images"]
    if form == "pil":
        from PIL import Image
        images = [Image.fromarray(i) for i in images]
    elif form == "tensor":
        images = torch.from_numpy(images)
    G = {k: torch.from_numpy(v) for k, v in gold.items()}
    call = dict(prompt_ids=G["ids"], negative_prompt_ids=G["neg_ids"], ip_adapter_image=images, num_frames=F, height=side, width=side,
                num_videos_per_prompt=n, num_inference_steps=steps, guidance_scale=scale)
    got = pipe(**call, generator=torch.Generator().manual_seed(seed), output_type="latent").frames
    assert len(unet.samples) == int(ncalls) == iters * steps
    assert torch.equal(enc.rgb, R.unit_ref(gold["images"]))                              # what the CLIP route is handed
    assert torch.equal(unet.samples[0], G["first_unet_sample"])                          # draws 1 and 2, the first-frame concat, the doubling
    assert torch.equal(unet.samples[0][:n], G["latents"]) and torch.equal(got[:, :, :1], G["first"])
    torch.testing.assert_close(unet.cameras[0], torch.cat([G["camera"]] * 2), rtol=0, atol=1e-6)
    torch.testing.assert_close(unet.samples[steps], G["second_pass_unet_sample"], rtol=1e-4, atol=1e-5)      # draw 3
    torch.testing.assert_close(got, G["final"], rtol=1e-4, atol=1e-5)
    # a generator consumed in another order does not get there: the same seed, the noise of frames 1.. drawn first
    other = torch.Generator().manual_seed(seed)
    noise = torch.randn(n, 4, F - 1, side // 8, side // 8, generator=other)
    swapped = pipe(**call, generator=other, latents=noise, output_type="latent").frames
    assert not torch.allclose(swapped[:, :, 1:], got[:, :, 1:], rtol=1e-2, atol=1e-3)
    frames = pipe(**call, generator=torch.Generator().manual_seed(seed), output_type="u8", return_dict=False)[0]
    assert isinstance(frames, VideoFrames)
    off = np.abs(frames.numpy().astype(np.int16) - gold["frames_u8"].astype(np.int16))
    print(f"[parity] pipeline bytes vs the reference chain's: {int((off != 0).sum())} of {off.size} differ, by {int(off.max())} at most")
    assert off.max() <= 1 and (off != 0).mean() < 1e-2
    as_np = pipe(**call, generator=torch.Generator().manual_seed(seed), output_type="np").frames
    assert as_np.shape == gold["frames_np"].shape and np.abs(as_np - gold["frames_np"]).max() < 1e-3


def test_prompt_halves_and_repeat(gold, monkeypatch):
    """(uncond, text), each repeated per view: the rows the UNet's text cross-attention reads, against the reference's cat statement."""
    pipe, unet, _ = _pipeline(monkeypatch)
    seen = {}
    real = P.denoise.denoise_loop

    def loop(unet_, latents, first, prompt_embeds, image_embeds, camera, **kw):
        seen.update(prompt_embeds=prompt_embeds, image_embeds=image_embeds, kw=kw)
        return real(unet_, latents, first, prompt_embeds, image_embeds, camera, **kw)

    monkeypatch.setattr(P.denoise, "denoise_loop", loop)
    n, F, side, steps, scale = (gold["cfg"][:5]).tolist()
    pipe(prompt_ids=torch.from_numpy(gold["ids"]), negative_prompt_ids=torch.from_numpy(gold["neg_ids"]), ip_adapter_image=gold["images"],
         num_frames=int(F), num_videos_per_prompt=int(n), num_inference_steps=1, guidance_scale=scale, output_type="latent",
         generator=torch.Generator().manual_seed(1), i2v_cond_time_zero=True)
    assert torch.equal(seen["prompt_embeds"], torch.from_numpy(gold["prompt_embeds"]))
    assert torch.equal(seen["image_embeds"], torch.from_numpy(gold["image_embeds"]))
    assert seen["kw"] == dict(num_inference_steps=1, guidance_scale=scale, i2v_cond_time_zero=True, scheduler_kwargs=None)
