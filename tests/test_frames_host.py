"""The frames of the 4-D stage on the host (animate3d_amd/frames.py): tests/frames_ref.py's restatement of the reference's ``test_step``
against the files the reference itself wrote (tests/golden/stage_frames.npz), the writers against the same files, the numeric file order,
every refusal of the loader, and the PNG round trip the recon -> refine chain rests on.  No GPU: everything here ends before the first
launch."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from animate3d_amd import frames, stage4d
from tests import frames_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_frames.npz")
OPTIONS = ("testset", "four_view")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _restated(option):
    out = []
    for i in range(R.COUNTS[option]):
        image, alpha = R.make_render(R.render_key(option, i))
        out.append(R.quantise_ref(image.clamp(0, 1).permute(1, 2, 0).numpy(), alpha.permute(1, 2, 0).numpy()))
    return np.stack(out)


@pytest.mark.parametrize("option", OPTIONS)
def test_restatement_is_what_the_reference_wrote(golden, option):
    count = R.COUNTS[option]
    assert list(golden[f"{option}_png_paths"]) == [R.render_path_ref(i, R.N_FRAME, option).replace(os.sep, "/") for i in range(count)]
    assert list(golden[f"{option}_npy_paths"]) == [f"mesh_trajectory/{i}.npy" for i in range(R.N_FRAME)]
    want = golden[f"{option}_rgba"]
    assert want.shape == (count, R.H, R.W, 4) and want.dtype == np.uint8
    assert np.array_equal(_restated(option), want)
    means = np.stack([R.make_means(R.render_key(option, i)).numpy() for i in range(R.N_FRAME)])
    assert np.array_equal(means, golden[f"{option}_npy"])
    # the inputs reach both sides of every decision: clamped values, the bounds, and bytes that a rounding cast would get wrong
    assert want.min() == 0 and want.max() == 255
    image, alpha = R.make_render(R.render_key(option, 0))
    assert float(image.min()) < 0 < 1 < float(image.max())
    rounded = np.rint(np.concatenate([image.clamp(0, 1).permute(1, 2, 0).numpy(), alpha.permute(1, 2, 0).numpy()], -1) * np.float32(255))
    assert (rounded.astype(np.uint8) != want[0]).any(), "no value of the render tells truncation from rounding"


@pytest.mark.parametrize("option", OPTIONS)
def test_writers_write_the_reference_files(golden, option, tmp_path):
    want = golden[f"{option}_rgba"]
    paths = frames.write_test_renders(str(tmp_path), want, n_frame=R.N_FRAME, test_option=option)
    assert [p.replace(os.sep, "/") for p in paths] == list(golden[f"{option}_png_paths"])
    assert paths == frames.render_paths(len(want), n_frame=R.N_FRAME, test_option=option)
    traj = frames.write_trajectory(str(tmp_path), torch.from_numpy(golden[f"{option}_npy"]))
    assert [p.replace(os.sep, "/") for p in traj] == list(golden[f"{option}_npy_paths"])
    written = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs)
    assert written == sorted(paths + traj)                                                     # these files and no others
    for rel, img in zip(paths, want):
        with Image.open(tmp_path / rel) as im:
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), img)
    for rel, arr in zip(traj, golden[f"{option}_npy"]):
        got = np.load(tmp_path / rel)
        assert got.dtype == np.float32 and np.array_equal(got, arr)


def test_write_refusals(tmp_path):
    good = np.zeros((2, 4, 4, 4), np.uint8)
    with pytest.raises(ValueError, match="test_option"):
        frames.write_test_renders(str(tmp_path), good, n_frame=1, test_option="test_set")       # the reference's own misspelling
    for bad in (good.astype(np.float32), good[..., :3], good[0]):
        with pytest.raises(ValueError, match="rgba8"):
            frames.write_test_renders(str(tmp_path), bad, n_frame=1, test_option="four_view")
    with pytest.raises(ValueError, match="trajectory"):
        frames.write_trajectory(str(tmp_path), np.zeros((3, 5, 2), np.float32))
    assert not os.listdir(tmp_path)


def _write(folder, name, arr):
    Image.fromarray(arr).save(os.path.join(folder, name))


def _rgba(seed, h=4, w=6):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def test_files_come_in_numeric_order(tmp_path):
    numbers = [10, 9, 0, 11, 2, 1, 100, 20, 3]
    for n in numbers:
        _write(tmp_path, f"{n}.png", _rgba(n))
    names = frames.frame_files(str(tmp_path))
    assert names == [f"{n}.png" for n in sorted(numbers)] == R.numeric_order(os.listdir(tmp_path))
    assert names != sorted(names)                                                              # the order a plain sort would give differs
    host = frames.decode_frames(str(tmp_path), count=len(numbers))
    assert host.dtype == np.uint8 and host.shape == (len(numbers), 4, 6, 4)
    for got, n in zip(host, sorted(numbers)):
        assert np.array_equal(got, _rgba(n))


def test_loader_refusals(tmp_path):
    """Each folder differs from a loadable one in one thing; all of it raises on the host, before a device is asked for."""
    def folder(name, files):
        d = tmp_path / name
        d.mkdir()
        for fname, arr in files.items():
            _write(d, fname, arr)
        return str(d)
    load = dict(n_view=1, n_frame=2, device="cuda")
    ok = {"0.png": _rgba(0), "1.png": _rgba(1)}
    with pytest.raises(ValueError, match="<int>"):
        frames.load_frames(folder("name", dict(ok, **{"frame2.png": _rgba(2)})), 4, 6, **dict(load, n_frame=3))
    with pytest.raises(ValueError, match="<int>"):
        frames.load_frames(folder("sign", dict(ok, **{"-1.png": _rgba(2)})), 4, 6, **dict(load, n_frame=3))
    with pytest.raises(ValueError, match="RGBA"):
        frames.load_frames(folder("rgb", {"0.png": _rgba(0), "1.png": _rgba(1)[..., :3].copy()}), 4, 6, **load)
    with pytest.raises(ValueError, match="RGBA"):
        frames.load_frames(folder("grey", {"0.png": _rgba(0), "1.png": _rgba(1)[..., 0].copy()}), 4, 6, **load)
    with pytest.raises(ValueError, match="frames before it"):
        frames.load_frames(folder("size", {"0.png": _rgba(0), "1.png": _rgba(1, 6, 4)}), 4, 6, **load)
    with pytest.raises(ValueError, match="n_view \\* n_frame"):
        frames.load_frames(folder("count", ok), 4, 6, **dict(load, n_frame=3))
    with pytest.raises(ValueError, match="no frames"):
        frames.load_frames(folder("empty", {}), 4, 6, **dict(load, n_frame=0))
    d = folder("resize", {"0.png": _rgba(0, 8, 12), "1.png": _rgba(1, 8, 12)})
    for height, width in ((3, 5), (16, 24), (4, 4), (8, 6), (2, 6), (5, 12)):                # no factor, enlarging, two factors, ...
        with pytest.raises(NotImplementedError, match="INTER_AREA"):
            frames.load_frames(d, height, width, **load)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.load_frames(d, 8, 12, **dict(load, device="cpu"))


def test_reduction_factor():
    assert frames.reduction_factor(1024, 1024, 1024, 1024) == 1
    assert frames.reduction_factor(12, 8, 6, 4) == 2 and frames.reduction_factor(64, 32, 4, 2) == 16
    for args in ((68, 34, 4, 2), (12, 8, 6, 2), (12, 8, 5, 4), (6, 4, 12, 8), (12, 8, 0, 0)):
        with pytest.raises(NotImplementedError):
            frames.reduction_factor(*args)


def test_box_rule_restatement():
    """The restatement of the rule against its definition in exact arithmetic, ties included: floor(mean + 1/2)."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    for k in (1, 2, 3, 4, 16):
        src = rng.integers(0, 256, (2, 2 * k, 3 * k, 4), dtype=np.uint8)
        src[0, :k, :k] = 255
        src[1, :k, :k, 3] = np.resize([127, 128], k * k).reshape(k, k)                          # even k: a mean of exactly 127.5
        got = R.box_reduce_ref(src, k)
        assert got.shape == (2, 2, 3, 4) and (got[0, 0, 0] == 255).all()
        for s, y, x, c in ((0, 1, 2, 0), (1, 0, 0, 3), (1, 1, 1, 2)):
            mean = Fraction(int(src[s, y * k:(y + 1) * k, x * k:(x + 1) * k, c].astype(np.int64).sum()), k * k)
            assert got[s, y, x, c] == (mean + Fraction(1, 2)).__floor__()
    quad = np.zeros((1, 2, 2, 4), np.uint8)
    quad[0, :, :, 0], quad[0, :, :, 3] = [[1, 0], [1, 0]], [[127, 128], [127, 128]]
    assert R.box_reduce_ref(quad, 2).tolist() == [[[[1, 0, 0, 128]]]]                           # 2 / 4 -> 1 (the tie goes up), 127.5 -> 128


def test_byte_arithmetic_claims():
    """What the GPU tests rest on, checked in fp32 on the host: a reciprocal multiply is not the division, the quantisation undoes the
    division for every byte, and ``> 0.5`` is ``>= 128``."""
    b = np.arange(256, dtype=np.uint8)
    div = b.astype(np.float32) / np.float32(255.0)
    assert int((b.astype(np.float32) * (np.float32(1.0) / np.float32(255.0)) != div).sum()) == 126
    assert np.array_equal((div * np.float32(255)).astype(np.uint8), b)
    assert np.array_equal(div > np.float32(0.5), b >= 128)
    rgb, mask = R.unpack_ref(np.stack([b, b, b, b], -1))
    assert rgb.dtype == np.float32 and np.array_equal(rgb[:, 0], div) and np.array_equal(mask[:, 0], b >= 128)


def test_png_round_trip_keeps_colour_under_zero_alpha(tmp_path):
    img = _rgba(3, 16, 16)
    img[:8, :, 3] = 0                                                                          # transparent, with colour underneath
    img[8:, :, 3] = np.arange(128, dtype=np.uint8).reshape(8, 16) * 2 + 1
    assert img[:8, :, :3].any()
    frames.write_test_renders(str(tmp_path), img[None], n_frame=1, test_option="four_view")
    host = frames.decode_frames(str(tmp_path / "images"), count=1)
    assert np.array_equal(host[0], img)


def _step_kwargs():
    return dict(loss=dict(lambda_rgb=1.0, lambda_mask=1.0), global_step=0, n_view=1, n_frame=2, progressive_iter_per_frame=10, bg=(0.5, 0.5, 0.5))


def test_training_step_wants_one_ground_truth():
    """Both, or neither, raises before the field, the Gaussians or the renderer are touched (they are ``None`` here)."""
    rgba8 = torch.zeros(2, 4, 4, 4, dtype=torch.uint8)
    rgb, mask = torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 4, 1, dtype=torch.bool)
    for batch, word in ((dict(rgba8=rgba8, rgb=rgb, mask=mask), "both"), (dict(rgba8=rgba8, mask=mask), "both"), (dict(c2w=None), "neither")):
        with pytest.raises(ValueError, match=word):
            stage4d.training_step(None, None, batch, render=None, **_step_kwargs())
    with pytest.raises(ValueError, match="rgba8.*expected 2 images"):
        stage4d.training_step(None, None, dict(rgba8=rgba8[:1]), render=None, **_step_kwargs())


def test_frameset_refuses_host_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.FrameSet(torch.zeros(2, 4, 4, 4, dtype=torch.uint8), 1, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.unpack_rgba8(torch.zeros(2, 4, 4, 4, dtype=torch.uint8), rgb=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.pack_rgba8(torch.zeros(2, 3, 4, 4), torch.zeros(2, 1, 4, 4))
    with pytest.raises(TypeError, match="uint8"):
        stage4d.masked_recon_loss_rgba8(torch.zeros(2, 3, 4, 4), torch.zeros(2, 1, 4, 4), torch.zeros(2, 4, 4, 4), bg=0.5, lambda_rgb=1.0,
                                        lambda_mask=1.0)
