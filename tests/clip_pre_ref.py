"""An independent numpy restatement of what ``CLIPImageProcessor`` does to an 8-bit RGB image, the oracle of animate3d_amd.clip's
``preprocess_frames`` where Pillow is absent:

* Pillow's 8-bit resampler (``src/libImaging/Resample.c``): ``precompute_coeffs`` with the bicubic filter (a = -0.5, support 2) in double
  precision, ``normalize_coeffs_8bpc`` to fixed point at 22 precision bits, a horizontal pass and then a vertical pass, each
  ``clip8((1 << 21) + sum(pixel * k))`` = the sum shifted right by 22 and clipped to [0, 255]; a pass whose sizes are equal is skipped;
* the shortest-edge output size and the centre crop of ``transformers.image_transforms``;
* ``/255`` and the mean / std normalisation with the OpenAI CLIP constants, here as a float64 table rounded once to float32.

It computes its own coefficients and imports nothing of the package.  tests/test_clip_preprocess_host.py holds it bit-equal to Pillow."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
BICUBIC_SUPPORT = 2.0


def bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(in_size: int, out_size: int):
    """``precompute_coeffs(in_size, 0, in_size, out_size)`` + ``normalize_coeffs_8bpc``: (ksize, bounds [out, 2] int32 = (first, count),
    kk [out, ksize] int32)."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = BICUBIC_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _pass(img: np.ndarray, out_size: int, stats=None) -> np.ndarray:
    """One resampling pass along axis 1 of ``img [rows, in, C]`` uint8 -> [rows, out, C] uint8.  ``stats`` (a list) receives the smallest and
    the largest value of the accumulator shifted by the precision, before the clip."""
    _, bounds, kk = coefficients(img.shape[1], out_size)
    src = img.astype(np.int64)
    out = np.empty((img.shape[0], out_size, img.shape[2]), np.int64)
    for xx in range(out_size):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, x0:x0 + n], kk[xx, :n].astype(np.int64), axes=([1], [0]))
        out[:, xx] = acc >> PRECISION_BITS
    if stats is not None:
        stats.append((int(out.min()), int(out.max())))
    return np.clip(out, 0, 255).astype(np.uint8)


def resize_u8(img: np.ndarray, out_h: int, out_w: int, stats=None) -> np.ndarray:
    """``PIL.Image.fromarray(img).resize((out_w, out_h), BICUBIC)`` for ``img [H, W, C]`` uint8: the horizontal pass, then the vertical one,
    each skipped when it would not change the size.  ``stats``: as ``_pass``, one entry per pass that ran (horizontal first)."""
    if img.shape[1] != out_w:
        img = _pass(img, out_w, stats)
    if img.shape[0] != out_h:
        img = _pass(img.transpose(1, 0, 2), out_h, stats).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


def output_size(h: int, w: int, size: int):
    """Shortest edge -> ``size``, the other edge ``int(size * long / short)`` (``get_resize_output_image_size``, default_to_square=False)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def crop_offsets(h: int, w: int, crop: int):
    return (h - crop) // 2, (w - crop) // 2


def quantise(rgb: np.ndarray) -> np.ndarray:
    """``(rgb * 255).astype(np.uint8)`` for float32 ``rgb`` in [0, 1]: a float32 multiply, then truncation.  Outside that range numpy leaves
    the cast undefined; the documented behaviour of the kernel is: NaN -> 0, below 0 -> 0, above 255 -> 255."""
    v = rgb.astype(np.float32) * np.float32(255.0)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.trunc(np.clip(v, 0, 255)).astype(np.uint8)


def norm_table() -> np.ndarray:
    """[3, 256] float32: ``((v / 255) - mean) / std`` in float64, rounded once."""
    v = np.arange(256, dtype=np.float64)[None] / 255.0
    return ((v - np.array(CLIP_MEAN, np.float64)[:, None]) / np.array(CLIP_STD, np.float64)[:, None]).astype(np.float32)


def preprocess_u8(img: np.ndarray, size: int = 224, crop: int = 224, stats=None) -> np.ndarray:
    """uint8 [H, W, 3] -> the resized and centre-cropped bytes [crop, crop, 3]."""
    oh, ow = output_size(img.shape[0], img.shape[1], size)
    if oh < crop or ow < crop:
        raise ValueError(f"{img.shape[0]}x{img.shape[1]} resized to {oh}x{ow} is smaller than the crop {crop}")
    out = resize_u8(img, oh, ow, stats)
    y0, x0 = crop_offsets(oh, ow, crop)
    return np.ascontiguousarray(out[y0:y0 + crop, x0:x0 + crop])


def pixel_values(u8: np.ndarray) -> np.ndarray:
    """Bytes [..., crop, crop, 3] -> normalised float32 [..., 3, crop, crop]."""
    t = norm_table()
    out = np.stack([t[c][u8[..., c]] for c in range(3)], axis=-3)
    return np.ascontiguousarray(out)


def preprocess(rgb: np.ndarray, size: int = 224, crop: int = 224):
    """float32 frames [B, H, W, 3] -> (bytes [B, crop, crop, 3] uint8, pixel_values [B, 3, crop, crop] float32)."""
    u8 = np.stack([preprocess_u8(quantise(f), size, crop) for f in rgb])
    return u8, pixel_values(u8)


# ---- the inputs the tests share
def noise_image(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_image(h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [127.5 + 127.5 * np.sin(x * rng.uniform(0.02, 0.2) + y * rng.uniform(0.02, 0.2) + rng.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def block_image(h: int, w: int, seed: int, cell: int = 5) -> np.ndarray:
    """0 / 255 blocks of ``cell`` pixels: the bicubic lobes overshoot on every edge, so the accumulators leave [0, 255] both ways."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 2, ((h + cell - 1) // cell, (w + cell - 1) // cell, 3), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(cells, np.ones((cell, cell, 1), np.uint8))[:h, :w])


def ulp_image(h: int, w: int, seed: int) -> np.ndarray:
    """float32 [h, w, 3]: exact 0.0, exact 1.0 and k / 255 moved one float32 ulp down, not at all, or up: the values at which the truncating
    quantisation decides between two bytes."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, (h, w, 3))
    v = (k.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    step = rng.integers(-1, 2, (h, w, 3))
    v = np.where(step < 0, np.nextafter(v, np.float32(-1)), np.where(step > 0, np.nextafter(v, np.float32(2)), v)).astype(np.float32)
    pick = rng.integers(0, 8, (h, w, 3))
    v = np.where(pick == 0, np.float32(0.0), np.where(pick == 1, np.float32(1.0), v)).astype(np.float32)
    return np.clip(v, 0, 1).astype(np.float32)


def golden_frame(h: int, w: int, seed: int) -> np.ndarray:
    """float32 [h, w, 3] in [0, 1): the seeded frames of tests/golden/clip_preprocess.npz (the file keeps a CRC of their bytes)."""
    return np.random.default_rng(seed).random((h, w, 3), dtype=np.float32)
