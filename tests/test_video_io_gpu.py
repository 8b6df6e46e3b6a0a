"""The byte ends of generation on the MI355X (csrc/video_io.hip through animate3d_amd/video.py) against tests/pipeline_ref.py, the float32 CPU
restatement of the reference's chain.  The kernels' arithmetic is a handful of correctly rounded float32 operations per value, so everything
is compared for equality, never within a tolerance."""
import numpy as np
import pytest
import torch

from animate3d_amd import clip, hip_ops, video
from tests import pipeline_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _all_patterns(dtype):
    """Rows [2 * 16384, 4] holding every 16-bit pattern in a channel that reaches the output: the 65 536 patterns as 16 384 pixels of 4
    channels, and once more shifted by one so that the patterns which sat in the padding channel 3 sit in channel 0."""
    bits = torch.arange(65536, dtype=torch.int32)
    both = torch.cat([bits.view(16384, 4), bits.roll(1).view(16384, 4)])
    return (both - 65536 * (both >= 32768)).to(torch.int16).view(dtype)           # the low 16 bits as a signed word


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_rows_path_every_16_bit_pattern(dtype):
    """Every rounding tie, both clamps, +-inf, -0 and the denormals of the storage type, exhaustively, in one launch."""
    rows = _all_patterns(dtype)
    wide = rows.float()[:, :3]                                                  # the widening is exact
    assert torch.unique(rows.view(torch.int16)[:, :3]).numel() == 65536
    got = video.video_to_u8(rows.cuda(), (1, 2, 128, 128)).cpu().numpy().reshape(-1, 3)
    nan = torch.isnan(wide).numpy()
    want = R.values_to_u8_ref(wide)
    assert nan.sum() > 0 and not got[nan].any()                                # a NaN gives 0: the kernel's definition
    diff = int((got[~nan] != want[~nan]).sum())
    print(f"[parity] video_to_u8 rows {dtype}: {diff} of {int((~nan).sum())} bytes differ, {int(nan.sum())} NaN patterns give 0")
    assert diff == 0


def _tie_inputs():
    """For each byte k the float32 inputs in a window of +-8 ulps around 2 (k + 0.5) / 255 - 1: those that land exactly on k + 0.5 after
    ``(x / 2 + 0.5) * 255`` in float32, and their neighbours on both sides."""
    xs = []
    for k in range(255):
        lo = hi = np.float32(2 * ((k + 0.5) / 255) - 1)
        xs.append(lo)
        for _ in range(8):
            lo, hi = np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(2))
            xs += [lo, hi]
    return np.array(xs, dtype=np.float32)


def test_planar_path_ties_edges_and_random_values():
    ties = _tie_inputs()
    t = R.denormalize_ref(torch.from_numpy(ties)).numpy() * np.float32(255)
    on_tie = int((t - np.floor(t) == 0.5).sum())
    one, big = np.float32(1), np.float32(np.inf)
    edges = np.array([-1, 1, np.nextafter(-one, -big), np.nextafter(-one, big), np.nextafter(one, big), np.nextafter(one, -big), -1.5, 1.5, 3e38,
                      -3e38, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45], dtype=np.float32)
    rand = (torch.rand(100000, generator=torch.Generator().manual_seed(11)) * 2.4 - 1.2).numpy()
    x = np.concatenate([ties, edges, rand])
    x = np.concatenate([x, np.zeros(-len(x) % 24, np.float32)])                 # [1, 3, 1, H, 8]
    vid = torch.from_numpy(x).view(1, 3, 1, -1, 8)
    got = video.video_to_u8(vid.cuda()).cpu().numpy()
    want = R.video_to_u8_ref(vid)
    diff = int((got != want).sum())
    print(f"[parity] video_to_u8 planar: {diff} of {want.size} bytes differ; {on_tie} of {len(ties)} tie-window inputs land exactly on k + 0.5")
    assert on_tie > 0 and diff == 0
    nan = torch.full((1, 3, 1, 2, 4), float("nan"))
    assert not video.video_to_u8(nan.cuda()).any()


def _canary_out(n, F, H, W, pixel, strip, pad_w):
    """(the whole padded buffer, the [n, F, H, W, pixel] view the kernel is to fill): rows are ``pad_w`` pixels longer than the frames and
    every image has one more row than H."""
    if strip:
        whole = torch.full((F, H + 1, n * W + pad_w, pixel), CANARY, dtype=torch.uint8, device="cuda")
        return whole, video.strip_as_views(whole[:, :H, :n * W], n)
    whole = torch.full((n, F, H + 1, W + pad_w, pixel), CANARY, dtype=torch.uint8, device="cuda")
    return whole, whole[:, :, :H, :W]


def _expected(whole_shape, n, F, H, W, pixel, strip, want):
    exp = np.full(whole_shape, CANARY, np.uint8)
    px = want if pixel == 3 else np.concatenate([want, np.full(want.shape[:-1] + (1,), 255, np.uint8)], axis=-1)
    if strip:
        exp[:, :H, :n * W] = R.strip_ref(px)
    else:
        exp[:, :, :H, :W] = px
    return exp


@pytest.mark.parametrize("pixel", [3, 4])
@pytest.mark.parametrize("strip", [False, True], ids=["views", "strip"])
@pytest.mark.parametrize("source", ["rows-bf16", "rows-fp16", "planar", "planar-w7"])
def test_layouts_write_the_addressed_pixels_and_nothing_else(source, strip, pixel):
    """n = 2, F = 3, H = 8, W = 12 (a row that is a multiple of 4 but not of 8 or 16; W = 7: the one-pixel-per-thread kernel) into a buffer
    pre-filled with a canary: per-view and strip strides, pixel sizes 3 and 4; alpha is 255, every byte outside the pixels is untouched."""
    n, F, H = 2, 3, 8
    W = 7 if source == "planar-w7" else 12
    g = torch.Generator().manual_seed(len(source) + 2 * pixel + strip)
    vid = torch.rand(n, 3, F, H, W, generator=g) * 2.4 - 1.2
    if source.startswith("rows"):
        dtype = torch.bfloat16 if source.endswith("bf16") else torch.float16
        rows = torch.cat([vid.permute(0, 2, 3, 4, 1), torch.full((n, F, H, W, 1), 7.0)], dim=-1).reshape(-1, 4).to(dtype)   # padding: not zero
        vid = rows[:, :3].float().reshape(n, F, H, W, 3).permute(0, 4, 1, 2, 3).contiguous()
        src, shape = rows.cuda(), (n, F, H, W)
    else:
        src, shape = vid.cuda(), None
    want = R.video_to_u8_ref(vid)
    whole, out = _canary_out(n, F, H, W, pixel, strip, pad_w=4 if W == 12 else 1)
    assert video.video_to_u8(src, shape, out=out, pixel=pixel) is out
    assert np.array_equal(whole.cpu().numpy(), _expected(tuple(whole.shape), n, F, H, W, pixel, strip, want))
    fresh = video.video_to_u8(src, shape, strip=strip, pixel=pixel).cpu().numpy()                 # and the buffers it allocates itself
    assert np.array_equal(fresh[..., :3], R.strip_ref(want) if strip else want) and (pixel == 3 or (fresh[..., 3] == 255).all())


def _byte_images(n, cin):
    """[n, 8, 8, cin]: with n = 4 the 256 pixels run through all 256 values in each channel (each channel in another order); with n = 2
    (128 pixels) red runs through 0 .. 127, green through 128 .. 255 and blue through the odd multiples.  Alpha holds values that would show."""
    p = np.arange(n * 64)
    chans = [p % 256, (p + 128) % 256, (p * 37 + 11) % 256]
    if cin == 4:
        chans.append((p * 91 + 3) % 256)
    return np.stack(chans, axis=-1).astype(np.uint8).reshape(n, 8, 8, cin)


@pytest.mark.parametrize("cin", [3, 4])
@pytest.mark.parametrize("n", [2, 4])
def test_images_in_bit_equal_and_clip_sees_the_bytes(n, cin):
    """``images_in_u8`` against the reference's host chain, bit for bit; and the float route to CLIP: at size = crop = 8 on an 8 x 8 image the
    resampler is the identity, so ``preprocess_frames``' bytes are its re-quantisation of the float image: they must be the input bytes.
    (A [2, 8, 8] image has 128 pixels, which cannot hold 256 values per channel: n = 4 is the case that does, in all three.)"""
    img = _byte_images(n, cin)
    if n == 4:
        assert all(np.unique(img[..., c]).size == 256 for c in range(3))
    planar, unit = video.images_in_u8(torch.from_numpy(img).cuda(), unit=True)
    assert torch.equal(planar.cpu(), R.images_in_ref(img)) and torch.equal(unit.cpu(), R.unit_ref(img))
    assert torch.equal(video.images_in_u8(torch.from_numpy(img).cuda()), planar)
    _, seen = clip.preprocess_frames(unit, size=8, crop=8, return_u8=True)
    assert np.array_equal(seen.cpu().numpy(), img[..., :3])


def test_images_in_one_pixel_per_thread_kernel():
    """H W = 15 is no multiple of 4: the scalar kernel."""
    img = np.random.default_rng(3).integers(0, 256, (3, 5, 3, 4), dtype=np.uint8)
    planar, unit = video.images_in_u8(torch.from_numpy(img).cuda(), unit=True)
    assert torch.equal(planar.cpu(), R.images_in_ref(img)) and torch.equal(unit.cpu(), R.unit_ref(img))


def test_argument_checks_return_einval_before_any_launch():
    lib = hip_ops.load_library()
    E = hip_ops.A3D_EINVAL
    src8 = torch.zeros(2, 8, 8, 4, dtype=torch.uint8, device="cuda")
    planar = torch.zeros(2, 3, 8, 8, device="cuda")
    p = lambda t: t.data_ptr()
    assert lib.a3d_images_in_u8(None, None, 2, 8, 8, 4, p(planar), None) == E                       # NULL
    assert lib.a3d_images_in_u8(None, p(src8), 2, 8, 8, 4, None, None) == E
    assert lib.a3d_images_in_u8(None, p(src8), 0, 8, 8, 4, p(planar), None) == E                    # zero extent
    assert lib.a3d_images_in_u8(None, p(src8), 2, 8, 8, 5, p(planar), None) == E                    # channels
    assert lib.a3d_images_in_u8(None, p(src8), 2, 8, 8, 4, p(planar) + 4, None) == E                # misaligned destination
    assert lib.a3d_images_in_u8(None, p(src8), 1 << 16, 1 << 16, 8, 4, p(planar), None) == E        # beyond the index range
    rows = torch.zeros(2 * 3 * 8 * 12, 4, dtype=torch.bfloat16, device="cuda")
    dst = torch.full((2 * 3 * 8 * 12 * 4 + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ok = (2, 3, 8, 12, p(dst), 3 * 8 * 36, 8 * 36, 36, 3)
    call = lambda src, dtype, *a: lib.a3d_video_to_u8(None, src, dtype, *a)
    assert call(None, hip_ops.A3D_BF16, *ok) == E                                                   # NULL
    assert call(p(rows), hip_ops.A3D_BF16, 2, 3, 8, 12, None, *ok[5:]) == E
    assert call(p(rows), hip_ops.A3D_BF16, 2, 0, 8, 12, *ok[4:]) == E                               # zero extent
    assert call(p(rows), hip_ops.A3D_BF16, 2, 3, 8, 12, p(dst) + 1, *ok[5:]) == E                   # misaligned destination
    assert call(p(rows), hip_ops.A3D_BF16, 2, 3, 8, 12, p(dst), 3 * 8 * 36 + 2, 8 * 36, 36, 3) == E  # misaligned stride
    assert call(p(rows), hip_ops.A3D_BF16, 2, 3, 8, 10, p(dst), 3 * 8 * 30, 8 * 30, 30, 3) == E     # W % 4 != 0 on the rows path
    assert call(p(rows), 7, *ok) == E                                                               # dtype code
    assert call(p(rows), hip_ops.A3D_BF16, 2, 3, 8, 12, p(dst), 3 * 8 * 36, 8 * 36, 35, 3) == E     # a row stride shorter than the row
    assert call(p(rows), hip_ops.A3D_BF16, 2, 3, 8, 12, p(dst), 3 * 8 * 36, 8 * 36, 36, 2) == E     # pixel size
    torch.cuda.synchronize()
    assert (dst == CANARY).all() and not planar.any()                                               # nothing ran
    with pytest.raises(RuntimeError, match="a3d_video_to_u8"):                                      # and through the launch path: raised, named
        hip_ops.call(lib, "a3d_video_to_u8", None, (p(rows), hip_ops.A3D_BF16, 2, 3, 8, 10, p(dst), 720, 240, 30, 3))
