"""CLIP image pre-processing of rendered frames on the MI355X (animate3d_amd/clip.py ``preprocess_frames`` / ``encode_frames`` /
``encode_image_from_frames``, csrc/clip_preprocess.hip, and ``sds.sds_guidance_loss(image_encoder=...)``).  The oracle is
tests/clip_pre_ref.py, which tests/test_clip_preprocess_host.py holds bit-equal to Pillow: the kernel's arithmetic is integer after an
exactly rounded float32 multiply, so bytes, table values and their 16-bit roundings are compared for equality, never within a tolerance.
Only the comparison with the recorded output of the reference's own processor (float32 arithmetic in another order) has a bar."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from animate3d_amd import clip
from tests import clip_pre_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_preprocess.npz")
PROCESSOR_BAR = 1e-6          # a few float32 roundings at |x| <= 2.3 (one ulp: 2.4e-7) in the processor against one in the table

# name -> (frames, in_h, in_w, size = crop, image_index or None)
CASES = {
    "256-indexed": (8, 256, 256, 224, (5, 0, 7, 2)),      # 4 of 8 frames, not in order
    "512": (1, 512, 512, 224, None),
    "64-upscale": (2, 64, 64, 224, None),
    "96x160": (2, 96, 160, 224, None),                    # crops along x at an odd offset (74)
    "160x96": (2, 160, 96, 224, None),                    # crops along y
    "300x256": (2, 300, 256, 224, None),                  # 262 x 224: offset 19
    "224-skipped": (2, 224, 224, 224, None),              # both passes skipped
    "224x300-skipped": (2, 224, 300, 224, None),          # both skipped, cropped at x = 38
    "37x29-to-28": (3, 37, 29, 28, None),                 # 2 x 2 patches of 14
}
KINDS = ("noise", "block", "ulp")
PATCH = 14
SMALL_V = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=PATCH,
               projection_dim=64, hidden_act="gelu")          # tests/test_clip.py's small tower at widths the HIP kernels take (head dim 64)


def _frames(kind, n, h, w, seed):
    if kind == "noise":
        return np.stack([R.golden_frame(h, w, seed + i) for i in range(n)])
    if kind == "block":                                   # exact 0.0 / 1.0 blocks: every pass overshoots [0, 255] both ways (host tier)
        return np.stack([(R.block_image(h, w, seed + i) == 255).astype(np.float32) for i in range(n)])
    return np.stack([R.ulp_image(h, w, seed + i) for i in range(n)])


@functools.lru_cache(maxsize=None)
def _reference(case, kind):
    """(frames float32 [N, H, W, 3], bytes [n, crop, crop, 3], pixel_values [n, 3, crop, crop]) of the restatement; computed once."""
    n, h, w, size, index = CASES[case]
    rgb = _frames(kind, n, h, w, seed=len(case) + 17 * KINDS.index(kind))
    picked = rgb if index is None else rgb[list(index)]
    u8, pv = R.preprocess(picked, size, size)
    for a in (rgb, u8, pv):
        a.setflags(write=False)
    return rgb, u8, pv


def _cuda(a):
    return torch.tensor(a, device="cuda")


def _index(case):
    index = CASES[case][4]
    return None if index is None else torch.tensor(index, device="cuda")


def _relayout(pv, patch, kp, dtype):
    """What ``CLIPVisionEncoderWithProjection.forward`` builds from pixel values: zero-padded patch rows in (c, ky, kx) order."""
    B, C, H, W = pv.shape
    gh, gw = H // patch, W // patch
    px = pv.float().reshape(B, C, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * patch * patch)
    pad = torch.zeros(B * gh * gw, kp, device=pv.device, dtype=dtype)
    pad[:, : px.shape[1]] = px.to(dtype)
    return pad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_bytes_and_pixel_values_equal_the_restatement(case, kind):
    rgb, want_u8, want_pv = _reference(case, kind)
    size = CASES[case][3]
    x = _cuda(rgb)
    pv, u8 = clip.preprocess_frames(x, _index(case), size=size, crop=size, return_u8=True)
    assert u8.dtype == torch.uint8 and u8.shape == want_u8.shape and pv.dtype == torch.float32 and pv.shape == want_pv.shape
    diff = int((u8.cpu().numpy() != want_u8).sum())
    print(f"[parity] clip_preprocess {case} {kind}: {diff} of {want_u8.size} bytes differ")
    assert diff == 0
    want = _cuda(want_pv)
    assert torch.equal(pv.view(torch.int32), want.view(torch.int32))               # bitwise: the table value of the byte
    for dtype in (torch.float16, torch.bfloat16):
        got = clip.preprocess_frames(x, _index(case), size=size, crop=size, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got.view(torch.int16), want.to(dtype).view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("case", sorted(CASES))
def test_patch_rows_equal_forwards_relayout(case, dtype):
    rgb, _, want_pv = _reference(case, "noise")
    size = CASES[case][3]
    k = 3 * PATCH * PATCH
    kp = (k + 63) // 64 * 64
    x = _cuda(rgb)
    want = _relayout(_cuda(want_pv), PATCH, kp, dtype)
    got = clip.preprocess_frames(x, _index(case), size=size, crop=size, dtype=dtype, patch_rows=(PATCH, kp))
    assert got.shape == want.shape and got.dtype == dtype and torch.equal(got, want)
    # into a buffer full of NaN, with guard rows around it: the padding columns come back zero, nothing outside is written
    buf = torch.full((want.shape[0] + 2, kp), float("nan"), device="cuda", dtype=dtype)
    ret = clip.preprocess_frames(x, _index(case), size=size, crop=size, dtype=dtype, patch_rows=(PATCH, kp), out=buf[1:-1])
    assert ret.data_ptr() == buf[1:-1].data_ptr() and torch.equal(buf[1:-1], want)
    assert float(buf[1:-1, k:].abs().max()) == 0.0 and bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


def test_strides_and_index():
    """The permuted view of a [B, 3, H, W] render is read in place and gives the bytes of its contiguous [B, H, W, 3] copy; no index is
    ``arange(B)``; int64 and int32 indices agree."""
    rgb, _, _ = _reference("300x256", "noise")
    nchw = _cuda(rgb).permute(0, 3, 1, 2).contiguous()           # what the rasterizer returns
    view = nchw.permute(0, 2, 3, 1)
    assert not view.is_contiguous() and view.data_ptr() == nchw.data_ptr()
    pv_v, u8_v = clip.preprocess_frames(view, return_u8=True)
    pv_c, u8_c = clip.preprocess_frames(view.contiguous(), return_u8=True)
    assert torch.equal(u8_v, u8_c) and torch.equal(pv_v, pv_c)
    every = torch.arange(view.shape[0], device="cuda")
    assert torch.equal(clip.preprocess_frames(view, every, return_u8=True)[1], u8_v)
    assert torch.equal(clip.preprocess_frames(view, every.to(torch.int32).flip(0), return_u8=True)[1], u8_v.flip(0))
    sliced = _cuda(rgb)[:, 3:-5, 2:-7]                            # a window of a larger render: strided rows
    assert torch.equal(clip.preprocess_frames(sliced, return_u8=True)[1], clip.preprocess_frames(sliced.contiguous(), return_u8=True)[1])


def test_documented_clamps():
    """NaN and values below 0 become byte 0, values above 1 byte 255; an index outside the batch gives a frame of zero bytes."""
    rgb = _reference("37x29-to-28", "noise")[0].copy()
    rng = np.random.default_rng(0)
    odd = np.array([np.nan, -np.inf, -0.25, -1e-30, 1.0 + 1e-6, 1.5, 300.0, np.inf], np.float32)
    where = rng.random(rgb.shape) < 0.2
    rgb[where] = odd[rng.integers(0, len(odd), int(where.sum()))]
    want_u8, want_pv = R.preprocess(rgb, 28, 28)
    x = _cuda(rgb)
    pv, u8 = clip.preprocess_frames(x, size=28, crop=28, return_u8=True)
    assert np.array_equal(u8.cpu().numpy(), want_u8) and np.array_equal(pv.cpu().numpy(), want_pv)
    outside = torch.tensor([-1, x.shape[0], 1], device="cuda")
    u8 = clip.preprocess_frames(x, outside, size=28, crop=28, return_u8=True)[1]
    assert int(u8[:2].max()) == 0 and np.array_equal(u8[2].cpu().numpy(), want_u8[1])


@pytest.mark.parametrize("tag", ["small", "big"])
def test_kernel_matches_reference_golden(tag):
    g = np.load(GOLDEN)
    (h, w), seed, size = g[f"{tag}_hw"], int(g[f"{tag}_seed"]), int(g[f"{tag}_size"])
    frame = torch.from_numpy(R.golden_frame(int(h), int(w), seed)[None]).cuda()
    got = clip.preprocess_frames(frame, size=size, crop=size)[0].cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - g[f"{tag}_pixel_values"]).max())
    print(f"[parity] clip_preprocess vs the reference's processor path ({tag}): max abs {err:.3e}")
    assert err <= PROCESSOR_BAR


def _small_tower(seed=0):
    torch.manual_seed(seed)
    return clip.CLIPVisionEncoderWithProjection(clip.CLIPTowerConfig(**SMALL_V), device="cuda").eval()


def test_small_tower_encode_frames_is_forward_of_preprocess():
    enc = _small_tower()
    rgb = _cuda(_reference("37x29-to-28", "noise")[0])
    index = torch.tensor([2, 0], device="cuda")
    for idx in (None, index):
        got = enc.encode_frames(rgb, idx)
        want = enc(clip.preprocess_frames(rgb, idx, size=28, crop=28))
        assert got.image_embeds.shape == ((3 if idx is None else 2), 64) and bool(torch.isfinite(got.image_embeds).all())
        assert torch.equal(got.image_embeds, want.image_embeds) and torch.equal(got.last_hidden_state, want.last_hidden_state)
    e, z = clip.encode_image_from_frames(enc, rgb, index)
    assert torch.equal(e, enc.encode_frames(rgb, index).image_embeds) and z.shape == e.shape and z.dtype == e.dtype
    assert float(z.abs().max()) == 0.0 and float(e.abs().max()) > 0.0


def test_vit_h_encode_frames_is_forward_of_own_pixel_values():
    torch.manual_seed(1)
    enc = clip.CLIPVisionEncoderWithProjection(device="cuda").to(torch.bfloat16).eval()
    rgb = _cuda(_reference("256-indexed", "noise")[0][:2])
    got = enc.encode_frames(rgb)
    want = enc(clip.preprocess_frames(rgb))
    assert got.image_embeds.shape == (2, 1024) and got.image_embeds.dtype == torch.bfloat16 and bool(torch.isfinite(got.image_embeds).all())
    assert torch.equal(got.image_embeds, want.image_embeds) and torch.equal(got.last_hidden_state, want.last_hidden_state)


def _stub_unet_cuda(sample, timestep, **kw):
    """tests/sds_stub.py's UNet, which computes on the CPU, around device tensors."""
    from tests.sds_stub import stub_unet
    cpu = lambda v: v.cpu() if isinstance(v, torch.Tensor) else v
    kw = {k: ({kk: cpu(vv) for kk, vv in v.items()} if isinstance(v, dict) else cpu(v)) for k, v in kw.items()}
    return SimpleNamespace(sample=stub_unet(sample.cpu(), cpu(timestep), **kw).sample.to(sample.device))


class _PoolVae:
    """A stand-in for the VAE encoder whose backward is bit-reproducible: 8 x 8 average pooling, a fixed 3 -> 4 channel mix, the noise."""

    def encode_images(self, imgs, generator=None, noise=None):
        mix = torch.tensor([[0.9, -0.4, 0.2], [0.1, 0.7, -0.6], [-0.5, 0.3, 0.8], [0.4, 0.4, 0.4]], device=imgs.device)
        pooled = torch.nn.functional.avg_pool2d(imgs, 8)
        return (pooled[:, None] * mix[None, :, :, None, None]).sum(2) + 0.1 * noise


def test_sds_guidance_loss_takes_the_encoder():
    """``image_encoder=`` gives the loss and ``rgb.grad`` of a call with the embeddings of the first frames, bit for bit, at 256^2 frames
    (the size of the existing SDS step tests) with tests/sds_stub.py's UNet.  Bit equality of ``rgb.grad`` needs a backward that two equal
    calls reproduce: at 256^2 the bilinear resize is the identity, and the VAE is a pooling stand-in, because the HIP encoder's GroupNorm
    backward sums its statistics with float atomics.  With the HIP encoder (fp16) the loss, which only runs its forward, is bit-equal too."""
    from animate3d_amd.sds import first_frame_index, sds_guidance_loss
    from animate3d_amd.vae import AutoencoderKLEncoder
    from oracle import vae_ref
    b, n, f = 1, 2, 2
    assert torch.equal(first_frame_index(3, 4, 8, "cuda").long(), torch.arange(3 * 4, device="cuda") * 8)
    first = first_frame_index(b, n, f, "cuda")
    assert first.dtype == torch.int32 and first.tolist() == [0, 2]
    enc = _small_tower(3)
    g = torch.Generator().manual_seed(5)
    rgb0 = torch.rand(b * n * f, 256, 256, 3, generator=g).cuda()
    vae_noise = torch.randn(b * n * f, 4, 32, 32, generator=g).cuda()
    noise = torch.randn(b, n, f - 1, 4, 32, 32, generator=g).cuda()
    text = torch.randn(2 * b * n, 7, 16, generator=g).cuda()
    c2w = torch.eye(4).repeat(b * n * f, 1, 1).cuda()
    t = torch.tensor([500], device="cuda")
    kw = dict(n_view=n, n_frame=f, vae_noise=vae_noise, noise=noise)

    def run(vae, image_embeds, **extra):
        rgb = rgb0.clone().requires_grad_(True)
        loss, _ = sds_guidance_loss(vae, _stub_unet_cuda, rgb, t, text, image_embeds, c2w, **kw, **extra)
        loss.backward()
        return loss.detach(), rgb.grad

    embeds = clip.encode_image_from_frames(enc, rgb0, first)[0]
    assert embeds.shape == (b * n, 64)
    pool = _PoolVae()
    loss_a, grad_a = run(pool, None, image_encoder=enc)
    loss_b, grad_b = run(pool, embeds)
    assert bool(torch.isfinite(loss_a)) and float(grad_a.abs().max()) > 0.0
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b)
    with pytest.raises(ValueError):
        run(pool, None)
    other = clip.encode_image_from_frames(enc, rgb0, first + 1)[0]                  # the embeddings matter: other frames, another loss
    assert not torch.equal(run(pool, other)[0], loss_a)
    vae = AutoencoderKLEncoder(device="cuda")
    vae.load_state_dict(vae_ref.init_synthetic_weights(vae_ref.VAEEncoderRef(), seed=1).state_dict(), strict=True)
    vae = vae.to(torch.float16).eval()
    (loss_c, grad_c), (loss_d, grad_d) = run(vae, None, image_encoder=enc), run(vae, embeds)
    rel = float((grad_c - grad_d).norm() / grad_d.norm())
    print(f"[sds] HIP VAE encoder: loss {float(loss_c):.4f} both ways; rgb.grad of the two calls differ by rel_l2 {rel:.2e} (float atomics)")
    assert torch.equal(loss_c, loss_d) and bool(torch.isfinite(grad_c).all()) and float(grad_c.abs().max()) > 0.0


def test_no_host_synchronisation_after_warm_up():
    """After one call per shape, ``preprocess_frames`` and ``encode_image_from_frames`` neither rebuild a plan nor synchronise: they run under
    torch's sync debug mode "error" (where this torch build does not raise for a ``.item()`` in that mode, the plan-cache identity alone
    is what this checks)."""
    enc = _small_tower()
    rgb = _cuda(_reference("37x29-to-28", "noise")[0])
    big = _cuda(_reference("96x160", "noise")[0])
    index = torch.tensor([1, 0], device="cuda")
    probe = torch.ones(1, device="cuda")
    clip.preprocess_frames(big, index, return_u8=True)
    clip.preprocess_frames(big, dtype=torch.bfloat16, patch_rows=(PATCH, 640))
    clip.encode_image_from_frames(enc, rgb, index)
    plans = dict(clip._PLANS)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    honoured = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        clip.preprocess_frames(big, index, return_u8=True)
        clip.preprocess_frames(big, dtype=torch.bfloat16, patch_rows=(PATCH, 640))
        clip.encode_image_from_frames(enc, rgb, index)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    print(f"[sync] torch's sync debug mode 'error' raises for .item() on this build: {honoured}")
    assert set(clip._PLANS) == set(plans) and all(clip._PLANS[k] is v for k, v in plans.items())
    assert clip.resize_plan(96, 160, 224, 224, big.device) is plans[(96, 160, 224, 224, str(big.device))]


def test_too_large_a_tile_is_refused():
    """A frame whose tile needs more intermediate rows than LDS holds gets an error from the entry point, never another computation; 1024 on
    a side is within the bound."""
    limit = clip.preprocess_lds_limit()
    assert clip.resize_plan(1024, 1024, 224, 224, "cuda").max_rows(PATCH) * 3 * 224 <= limit
    side = 1400
    assert clip.resize_plan(side, side, 224, 224, "cuda").max_rows(PATCH) * 3 * 224 > limit
    x = torch.zeros(1, side, side, 3, device="cuda")
    out = torch.full((1, 3, 224, 224), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="A3D_EUNSUPPORTED"):
        clip.preprocess_frames(x, out=out)
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0                      # nothing was launched
    large = torch.rand(1, 1024, 1024, 3, generator=torch.Generator().manual_seed(0))    # 21 taps per axis, 78-row tiles
    want = R.preprocess(large.numpy())[0]
    assert np.array_equal(clip.preprocess_frames(large.cuda(), return_u8=True)[1].cpu().numpy(), want)
