"""Input gradient of the VAE encoder and the 4D-SDS step from rendered pixels (animate3d_amd/vae_grad.py, ``encode_images``,
``sds_guidance_loss``) on the plain-torch op set: every backward formula against torch autograd of the oracle, without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from animate3d_amd.autograd_ops import AutogradOps
from animate3d_amd.sds import sds_guidance_loss, sds_recon_loss
from animate3d_amd.vae import AutoencoderKLEncoder, VAEConfig
from oracle import vae_ref as R
from tests.sds_stub import StubDDIM, stub_unet
from tests.vae_grad_ops import VaeGradRefOps

SMALL = dict(block_out_channels=(32, 64, 64, 64), attention_head_dim=64)


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _pair(wrap=False, seed=1):
    ref = R.init_synthetic_weights(R.VAEEncoderRef(R.VAEConfig(**SMALL)), seed=seed).eval()
    ops = VaeGradRefOps()
    enc = AutoencoderKLEncoder(VAEConfig(**SMALL), ops=AutogradOps(ops) if wrap else ops)
    enc.load_state_dict(ref.state_dict(), strict=True)
    return ref, enc


def _oracle_latents(ref, imgs, noise):
    """The guidance's encode_images through the oracle with autograd (its ``encode`` is no_grad): chunk, clamp and sample here."""
    with torch.enable_grad():
        moments = ref.quant_conv(ref.encoder(imgs * 2 - 1))
        mean, logvar = torch.chunk(moments, 2, dim=1)
        return (mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * noise) * ref.cfg.scaling_factor


@pytest.mark.parametrize("wrap", [False, True])
def test_encode_images_vjp_matches_oracle_autograd(wrap):
    ref, enc = _pair(wrap)
    g = torch.Generator().manual_seed(3)
    imgs = torch.rand(2, 3, 32, 48, generator=g)
    noise = torch.randn(2, 4, 4, 6, generator=g)
    cot = torch.randn(2, 4, 4, 6, generator=g)
    x = imgs.clone().requires_grad_(True)
    lat = enc.encode_images(x, noise=noise)
    assert lat.shape == (2, 4, 4, 6) and lat.dtype == torch.float32 and lat.grad_fn is not None
    lat.backward(cot)
    xr = imgs.clone().requires_grad_(True)
    want = _oracle_latents(ref, xr, noise)
    want.backward(cot)
    assert _rel(lat.detach(), want.detach()) <= 1e-5
    err = _rel(x.grad, xr.grad)
    print(f"[parity] encode_images VJP on the torch op set: rel_l2 {err:.3e}")
    assert err <= 1e-4
    assert all(p.grad is None for p in enc.parameters())          # frozen: only the input gradient is computed


def test_mid_attention_backward_with_padded_token_count():
    """8 x 12 latent = 96 mid-block tokens: the backward's zero-padded contractions over L (64 -> 128 columns), against autograd."""
    ref, enc = _pair()
    g = torch.Generator().manual_seed(5)
    imgs = torch.rand(1, 3, 64, 96, generator=g)
    noise = torch.randn(1, 4, 8, 12, generator=g)
    cot = torch.randn(1, 4, 8, 12, generator=g)
    x = imgs.clone().requires_grad_(True)
    enc.encode_images(x, noise=noise).backward(cot)
    xr = imgs.clone().requires_grad_(True)
    _oracle_latents(ref, xr, noise).backward(cot)
    assert _rel(x.grad, xr.grad) <= 1e-4


def test_encode_images_forward_is_encode_latents():
    """Same kernels as ``encode``: the latents equal ``encode_latents(imgs * 2 - 1)`` with the same generator, with and without autograd;
    ``imgs.dtype`` comes back."""
    _, enc = _pair()
    imgs = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    want = enc.encode_latents(imgs * 2 - 1, generator=torch.Generator().manual_seed(7))
    got = enc.encode_images(imgs.clone().requires_grad_(True), generator=torch.Generator().manual_seed(7))
    assert torch.equal(got.detach(), want)
    assert torch.equal(enc.encode_images(imgs, generator=torch.Generator().manual_seed(7)), want)
    assert enc.encode_images(imgs.double(), generator=torch.Generator().manual_seed(7)).dtype == torch.float64


def test_no_graph_without_grad():
    _, enc = _pair()
    imgs = torch.rand(1, 3, 32, 32, requires_grad=True)
    with torch.no_grad():
        z = enc.encode_images(imgs)
    assert z.grad_fn is None and not z.requires_grad
    z = enc.encode_images(imgs.detach())
    assert z.grad_fn is None and not z.requires_grad
    assert enc._gops is None                                          # the differentiable op set was never built


def _sds_inputs(n, f, hw, channels=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(n * f, *hw, channels, generator=g)
    t = torch.tensor([600])
    text = torch.randn(2 * n, 5, 16, generator=g)
    emb = torch.randn(n, 12, generator=g)
    c2w = torch.eye(4).repeat(n * f, 1, 1) + 0.2 * torch.randn(n * f, 4, 4, generator=g)
    noise = torch.randn(1, n, 4, f - 1, 32, 32, generator=g)        # the reference's "b n c f h w" draw
    vae_noise = torch.randn(n * f, 4, 32, 32, generator=g)
    return rgb, t, text, emb, c2w, noise, vae_noise


@pytest.mark.parametrize("rgb_as_latents", [False, True])
def test_sds_guidance_loss_gradient_reaches_rgb(rgb_as_latents):
    """The guidance call from rendered frames [(b n f), H, W, 3]: resize (bilinear, align_corners=False) to 256^2 -> encode_images ->
    sds_recon_loss with the stub UNet, or resize to 32^2 taken as latents.  ``rgb.grad`` against the same chain written out with the
    oracle encoder and torch autograd.  (With ``rgb_as_latents`` the renderer's output has the 4 latent channels.)"""
    n, f, hw = 2, 2, (24, 40)
    ref, enc = _pair()
    rgb0, t, text, emb, c2w, noise, vae_noise = _sds_inputs(n, f, hw, channels=4 if rgb_as_latents else 3)
    kw = dict(n_view=n, n_frame=f, guidance_scale=7.5, recon_std_rescale=0.5, alphas_cumprod=StubDDIM().alphas_cumprod, noise=noise)
    rgb = rgb0.clone().requires_grad_(True)
    loss, aux = sds_guidance_loss(enc, stub_unet, rgb, t, text, emb, c2w, rgb_as_latents=rgb_as_latents, vae_noise=vae_noise, **kw)
    loss.backward()

    rgb_r = rgb0.clone().requires_grad_(True)
    x = rgb_r.permute(0, 3, 1, 2)
    if rgb_as_latents:
        lat = F.interpolate(x, (32, 32), mode="bilinear", align_corners=False)
    else:
        lat = _oracle_latents(ref, F.interpolate(x, (256, 256), mode="bilinear", align_corners=False), vae_noise)
    loss_r, aux_r = sds_recon_loss(stub_unet, lat, t, text, emb, c2w, **kw)
    loss_r.backward()
    assert aux["latents"].shape == (n * f, 4, 32, 32)
    torch.testing.assert_close(loss.detach(), loss_r.detach(), rtol=1e-5, atol=0)
    err = _rel(rgb.grad, rgb_r.grad)
    print(f"[parity] sds_guidance_loss rgb.grad (rgb_as_latents={rgb_as_latents}): rel_l2 {err:.3e}")
    assert err <= 1e-4 and float(rgb.grad.abs().max()) > 0
