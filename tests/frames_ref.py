"""Reference side of the frames tests (TEST INFRASTRUCTURE): a numpy restatement of the arithmetic lines of the reference's
``SimpleMultiImageDataBase.load_images`` (custom/threestudio-animate3d/data/simple_multi_image.py:198, 205-215) and of
``Animate3DSystem.test_step`` (systems/animate3d.py:441-471), the integer box rule of csrc/stage_frames.hip, and the seeded renders that
tests/golden/make_stage_frames_goldens.py and the tests that replay its vectors both build (a tensor is a function of its key and shape
only, so the fixture holds the files the reference wrote but no inputs)."""
import os

import numpy as np
import torch

from tests.golden.seeded import seeded_tensor

H, W, N_FRAME, N_POINTS = 6, 8, 3, 5
COUNTS = {"testset": 3 * 4 * N_FRAME, "four_view": 4 * N_FRAME}          # 36 and 12 test cameras


# ---- load_images

def numeric_order(names):
    """simple_multi_image.py:198."""
    return sorted(names, key=lambda x: int(x[:-4]))


def unpack_ref(rgba8):
    """simple_multi_image.py:205-215 without the resize: (rgb float32 [..., 3], mask bool [..., 1]) of uint8 [..., 4]."""
    rgba = rgba8.astype(np.float32) / 255.0
    return rgba[..., :3], rgba[..., 3:] > 0.5


def box_reduce_ref(rgba8, k):
    """uint8 [S, k H, k W, 4] -> [S, H, W, 4]: per channel (2 sum + k^2) // (2 k^2) over each k x k block, the exact mean rounded half up."""
    S, h, w, C = rgba8.shape
    blocks = rgba8.reshape(S, h // k, k, w // k, k, C).astype(np.int64)
    total = blocks.sum(axis=(2, 4))
    return ((2 * total + k * k) // (2 * k * k)).astype(np.uint8)


# ---- test_step

def quantise_ref(comp_rgb, comp_mask):
    """animate3d.py:441-445 on numpy arrays [H, W, 3] and [H, W, 1]."""
    rgba_img = np.concatenate([comp_rgb, comp_mask], axis=-1)
    return (rgba_img * 255).astype(np.uint8)


def render_path_ref(batch_index, n_frame, test_option):
    """animate3d.py:448-462, relative to the save directory."""
    if test_option == "testset":
        elv_index = batch_index // (n_frame * 4)
        azi_index = (batch_index // n_frame) % 4
        frame_index = batch_index % n_frame
        output_folder = os.path.join("images", f"elv_{elv_index}_azi_{azi_index}")
    elif test_option == "four_view":
        frame_index = batch_index
        output_folder = "images"
    else:
        raise NotImplementedError(f"test_option {test_option} not supported")
    return os.path.join(output_folder, f"{frame_index}.png")


# ---- seeded renders

def special_values():
    """Values where the quantisation can go either way: below 0 and above 1 (the clamp), the bounds, and j / 255 in fp32 with its
    neighbours on both sides for a spread of j."""
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    vals = [torch.tensor(-0.25), torch.nextafter(zero, -one), -zero, zero, torch.nextafter(zero, one), torch.nextafter(one, zero), one,
            torch.nextafter(one, one + one), torch.tensor(1.25)]
    for j in (1, 2, 3, 64, 127, 128, 129, 200, 253, 254):
        v = torch.tensor(float(j)) / torch.tensor(255.0)
        vals += [torch.nextafter(v, zero), v, torch.nextafter(v, one)]
    return torch.stack(vals)


def make_render(key, h=H, w=W):
    """(image [3, h, w] raw, alpha [1, h, w] in [0, 1]) fp32 of one test camera: ``special_values`` at fixed places of both."""
    image = seeded_tensor(f"frames/{key}/image", (3, h, w), 0.6) + 0.5
    alpha = torch.sigmoid(seeded_tensor(f"frames/{key}/alpha", (1, h, w), 2.0))
    sv = special_values()
    for t, vals in ((image, sv), (alpha, sv[(sv >= 0) & (sv <= 1)])):
        flat = t.view(-1)
        n = min(vals.numel(), flat.numel())
        flat[torch.arange(n) * (flat.numel() // n)] = vals[:n]
    return image.contiguous(), alpha.contiguous()


def make_means(key, n=N_POINTS):
    return seeded_tensor(f"frames/{key}/means", (n, 3), 0.3)


def render_key(test_option, batch_index):
    return f"{test_option}/{batch_index}"
