"""CPU checks of the camera layer's host logic (animate3d_amd/cameras.py) against tests/golden/cameras.npz, which
tests/golden/make_camera_goldens.py takes from the reference's own data modules: the sampler's schedule, the frame structure of a batch
and of ``take``, the index maps of the evaluation sets, the refusals of the Python layer and of the C-ABI.  Nothing here launches a kernel."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from animate3d_amd import cameras, stage4d
from tests import cameras_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cameras.npz")


@pytest.fixture(scope="module")
def golden():
    data = dict(np.load(GOLDEN))
    return data, json.loads(str(data["meta"]))


def _cpu_batch(B, frame_ids, total_frame, height=8, width=8):
    """A batch of recognisable CPU tensors: the host logic does not care where they live."""
    ids = torch.arange(B, dtype=torch.float32)
    mats = ids[:, None, None].expand(B, 4, 4).contiguous()
    return cameras.CameraBatch(mats, ids.clone(), mats + 100, mats + 200, ids[:, None].expand(B, 3).contiguous(), ids + 300, height, width,
                               tuple(frame_ids), cameras.frame_times(total_frame), elevation=ids + 400, azimuth=ids + 500,
                               camera_distances=ids + 600)


def test_update_step_against_the_golden(golden):
    _, meta = golden
    for case, want in zip(R.RANDOM_CASES, meta["random"]):
        s = cameras.RandomCameraSampler(**case["cfg"])
        s.update_step(case["step"])
        assert (s.height, s.width, s.batch_size) == (want["height"], want["width"], want["batch_size"]), case["name"]
        assert s.elevation_range == want["elevation_range"] and s.azimuth_range == want["azimuth_range"], case["name"]   # the same float64 arithmetic
        assert want["coin"] == (case["elev_mode"] == 0)
    s = cameras.RandomCameraSampler(**dict(R.RANDOM_CASES[5]["cfg"]))
    sizes = []
    for step in (0, 499, 500, 10 ** 6):
        s.update_step(step)
        sizes.append((s.height, s.width, s.batch_size))
    assert sizes == [(8, 8, 12), (8, 8, 12), (16, 24, 24), (16, 24, 24)]
    s = cameras.RandomCameraSampler(progressive_until=0, batch_size=32)                  # the reference's step 0: one point
    s.update_step(0)
    assert s.elevation_range == [15.0, 15.0] and s.azimuth_range == [0.0, 0.0]
    s.update_step(1)
    assert s.elevation_range == [-10.0, 90.0] and s.azimuth_range == [-180.0, 180.0]


def test_sampler_takes_the_reference_config_and_its_defaults():
    s = cameras.RandomCameraSampler(batch_size=32, eval_height=512, light_sample_strategy="dreamfusion", rays_d_normalize=True)
    assert (s.height, s.width, s.n_view, s.total_frame, s.relative_radius) == (64, 64, 4, 8, True)
    assert s.cfg_elevation_range == (-10.0, 90.0) and s.fovy_range == (40.0, 70.0) and s.zoom_range == (1.0, 1.0)
    assert (s.camera_perturb, s.center_perturb, s.up_perturb, s.eval_elevation_deg) == (0.1, 0.2, 0.02, 15.0)
    with pytest.raises(TypeError, match="no_such_name"):
        cameras.RandomCameraSampler(batch_size=32, no_such_name=1)


@pytest.mark.parametrize("strategy,step,want", [("normal", 25, [1, 2, 3]), ("light", 25, None), ("light", 10 ** 6, [1, 2, 3])])
def test_take_frame_structure_for_the_frame_schedules(strategy, step, want):
    """What the step gathers: the (view, frame) images of the sampled frames, with their own ``frames`` / ``image_to_time``."""
    import random
    n_view, n_frame = 2, 4
    frames = stage4d.sampled_frames(step, n_frame, 10, do_guidance=False, strategy=strategy, rng=random.Random(5))
    if want is not None:
        assert frames == want
    else:
        assert len(frames) == 2 and frames[1] == 3
    full = _cpu_batch(n_view * n_frame, [f for _ in range(n_view) for f in range(n_frame)], n_frame)
    index = [v * n_frame + f for v in range(n_view) for f in frames]
    assert index == stage4d.sampled_image_index(frames, n_view, n_frame).tolist()
    sub = full.take(index)
    assert sub.frame_ids == tuple(frames) * n_view and sub.frame_times == full.frame_times
    distinct, i2t = cameras.frame_structure(sub.frame_ids)
    assert (distinct, i2t) == R.frame_structure(sub.frame_ids) and distinct == sorted(set(frames))
    times = torch.linspace(-1, 1, n_frame)
    assert torch.equal(sub.frames, times[distinct]) and sub.image_to_time.tolist() == i2t and sub.image_to_time.dtype == torch.int64
    assert torch.equal(sub.timestamps, times[list(sub.frame_ids)][:, None])
    want_frames, want_i2t = stage4d.frames_of_images(sub.timestamps)                     # what the tensor path finds in the timestamps
    assert torch.equal(sub.frames, want_frames) and torch.equal(sub.image_to_time, want_i2t)
    for name in ("c2w", "fovy", "w2c", "full_proj", "campos", "tanfov", "elevation", "azimuth", "camera_distances"):
        assert torch.equal(getattr(sub, name), getattr(full, name)[index]), name
    assert (sub.height, sub.width) == (full.height, full.width)
    again = full.take([3, 3, 0])                                                         # repeats, any order
    assert again.frame_ids == (3, 3, 0) and again.image_to_time.tolist() == [1, 1, 0] and again.fovy.tolist() == [3.0, 3.0, 0.0]
    with pytest.raises(IndexError):
        full.take([n_view * n_frame])


def test_batch_stands_where_the_reference_dict_stands():
    b = _cpu_batch(6, [0, 1, 2] * 2, 3)
    assert set(b.keys()) == {"c2w", "fovy", "timestamps", "elevation", "azimuth", "camera_distances", "camera_positions", "height", "width"}
    seen = {}
    (lambda **kw: seen.update(kw))(**b)
    assert seen["c2w"] is b.c2w and seen["camera_positions"] is b.campos and seen["timestamps"].shape == (6, 1) and seen["height"] == 8
    assert b.get("cameras") is None and "c2w" in b and "rays_o" not in b
    for key in ("rays_o", "rays_d", "light_positions", "proj_mtx", "mvp_mtx"):
        with pytest.raises(KeyError, match="not built"):
            b[key]
    with pytest.raises(KeyError):
        b["w2c_typo"]
    with pytest.raises(ValueError):
        cameras.CameraBatch(b.c2w, b.fovy, b.w2c, b.full_proj, b.campos, b.tanfov, 8, 8, (0, 1, 2), b.frame_times)      # 3 ids, 6 cameras
    with pytest.raises(ValueError):
        cameras.CameraBatch(b.c2w, b.fovy, b.w2c, b.full_proj, b.campos, b.tanfov, 8, 8, (0, 1, 3) * 2, b.frame_times)  # frame 3 of 3


def test_eval_set_index_maps_against_the_golden(golden, monkeypatch):
    """Which camera and which frame every item of the orbit and the test set holds, without a device: the kernel call is recorded."""
    data, meta = golden
    calls = []

    def record(elev, azim, dist, fovy, frame_ids, total_frame, height, width, device):
        calls.append(dict(elev=list(elev), azim=list(azim), dist=list(dist), fovy=list(fovy), frame_ids=list(frame_ids), F=total_frame,
                          size=(height, width)))
    monkeypatch.setattr(cameras, "_spherical", record)
    f32 = lambda values: np.asarray(values, np.float32)                                   # noqa: E731
    for i, case in enumerate(R.ORBIT_CASES):
        cfg = dict(R.ORBIT_CFG, n_val_views=case["n_val_views"], n_test_views=case["n_test_views"])
        cameras.orbit_cameras(cfg, case["split"])
        got, F = calls[-1], cfg["total_frame"]
        n = meta["orbit"][i]["n_items"]
        assert n == (case["n_val_views"] if case["split"] == "val" else case["n_test_views"]) == len(got["azim"])
        assert np.array_equal(f32(got["azim"]), data[f"orbit{i}_azimuth"]) and np.array_equal(f32(got["elev"]), data[f"orbit{i}_elevation"])
        assert np.array_equal(f32(got["dist"]), data[f"orbit{i}_camera_distances"])
        times = np.asarray(cameras.frame_times(F), np.float32)
        assert np.array_equal(times[got["frame_ids"]][:, None], data[f"orbit{i}_timestamps"])
        held = [(k // F) * F for k in range(n)]
        assert np.array_equal(data[f"orbit{i}_c2w"], data[f"orbit{i}_cameras_c2w"][held])        # the golden's own hold, as a cross-check
        assert got["size"] == (meta["orbit"][i]["height"], meta["orbit"][i]["width"])
    cameras.testset_cameras(dict(R.TESTSET_CFG))
    got, F = calls[-1], R.TESTSET_CFG["total_frame"]
    assert len(got["azim"]) == meta["testset"]["n_items"] == 2 * 3 * 2
    assert np.array_equal(f32(got["azim"]), data["testset_azimuth"]) and np.array_equal(f32(got["elev"]), data["testset_elevation"])
    assert np.array_equal(np.asarray(cameras.frame_times(F), np.float32)[got["frame_ids"]][:, None], data["testset_timestamps"])
    assert np.array_equal(data["testset_c2w"], data["testset_cameras_c2w"][[k // F for k in range(12)]])
    for k in range(12):                                                                   # test_step's arithmetic, systems/animate3d.py:448-451
        elv_index, azi_index, frame_index = k // F // 3, k // F % 3, k % F
        assert got["elev"][k] == R.TESTSET_CFG["eval_elevation_deg"][elv_index] and got["frame_ids"][k] == frame_index
        assert got["azim"][k] == R.TESTSET_CFG["eval_azimuth_deg"][elv_index][azi_index]
    cameras.data_view_cameras(**R.DATA_VIEW_CASE)
    got = calls[-1]
    assert np.array_equal(f32(got["azim"]), data["data_azimuth"]) and np.array_equal(f32(got["elev"]), data["data_elevation"])
    assert np.array_equal(f32(got["dist"]), data["data_camera_distances"])
    assert np.array_equal(np.asarray(cameras.frame_times(3), np.float32)[got["frame_ids"]][:, None], data["data_timestamps"])
    assert np.abs(f32([f * cameras.DEG for f in got["fovy"]]).astype(np.float64) - data["data_fovy"]).max() <= np.spacing(np.float32(1.0))
    per_image = [float(a) for a in range(12)]
    cameras.data_view_cameras(**dict(R.DATA_VIEW_CASE, default_azimuth_deg=per_image, default_elevation_deg=[5.0] * 12))
    assert calls[-1]["azim"] == per_image and calls[-1]["elev"] == [5.0] * 12


def test_value_errors():
    with pytest.raises(ValueError, match="batch_size"):
        cameras.RandomCameraSampler(batch_size=20, n_view=4, total_frame=3)
    with pytest.raises(ValueError, match="batch_size"):
        cameras.RandomCameraSampler(batch_size=[12, 20], height=[8, 8], width=[8, 8], resolution_milestones=[5], n_view=4, total_frame=3)
    with pytest.raises(ValueError, match="resolution_milestones"):
        cameras.RandomCameraSampler(batch_size=[12, 24], height=[8, 8], width=[8, 8], n_view=4, total_frame=3)
    for elevation in (90.0, -90.0, [0.0] * 11 + [90.0]):
        with pytest.raises(ValueError, match="singular"):
            cameras.data_view_cameras(**dict(R.DATA_VIEW_CASE, default_elevation_deg=elevation))
    with pytest.raises(ValueError, match="default_azimuth_deg"):
        cameras.data_view_cameras(**dict(R.DATA_VIEW_CASE, default_azimuth_deg=(0.0, 90.0, 180.0)))
    with pytest.raises(ValueError, match="test"):
        cameras.testset_cameras(dict(R.TESTSET_CFG), "val")
    b = _cpu_batch(2, [0, 1], 2)
    some = torch.zeros(2, 4, 4)
    for given in (dict(c2w=some), dict(fovy=some), dict(timestamps=some)):                # before anything touches a device
        args = dict(c2w=None, fovy=None, timestamps=None, **{}) | given
        with pytest.raises(ValueError, match="cameras="):
            stage4d.render_batch(None, None, args["c2w"], args["fovy"], args["timestamps"], 8, 8, None, do_guidance=True, cameras=b)
    with pytest.raises(ValueError, match="height"):
        stage4d.render_batch(None, None, None, None, None, 16, 8, None, do_guidance=True, cameras=b)


def test_cabi_refusals():
    """NULL and misaligned pointers, B = 0, bad planes and modes: A3D_EINVAL before any HIP call (no device is needed to be refused)."""
    from animate3d_amd.hip_ops import load_library
    lib = load_library()
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = [base + 256 * i for i in range(14)]
    ranges = (ctypes.c_double * 10)(-10, 90, -180, 180, 40, 70, 1, 1.5, 1, 1)
    EINVAL = -1

    def spherical(B=1, ptrs=None, perturb=None, unit=1.0, znear=0.1, zfar=100.0):
        q = list(p[:9]) if ptrs is None else ptrs
        return lib.a3d_cameras_spherical_f32(None, B, q[0], q[1], q[2], q[3], perturb, unit, znear, zfar, q[4], q[5], q[6], q[7], q[8])

    def rand(R=1, n_view=1, F=1, ptrs=None, rng=ranges, mode=0, znear=0.1, zfar=100.0):
        q = list(p[:12]) if ptrs is None else ptrs
        return lib.a3d_cameras_random_f32(None, R, n_view, F, q[0], q[1], q[2], rng, mode, 1, 0.1, 0.2, 0.02, znear, zfar, *q[3:12])

    def from_c2w(B=1, ptrs=None, znear=0.1, zfar=100.0):
        q = list(p[:6]) if ptrs is None else ptrs
        return lib.a3d_cameras_from_c2w_f32(None, B, q[0], q[1], znear, zfar, q[2], q[3], q[4], q[5])

    for call, n in ((spherical, 9), (rand, 12), (from_c2w, 6)):
        for B in (0, -1):
            assert call(B) == EINVAL, (call.__name__, B)
        for k in range(n):
            null, odd = list(p[:n]), list(p[:n])
            null[k], odd[k] = None, p[k] + 2
            assert call(ptrs=null) == EINVAL, (call.__name__, "NULL", k)
            assert call(ptrs=odd) == EINVAL, (call.__name__, "misaligned", k)
        assert call(znear=0.0) == EINVAL and call(znear=1.0, zfar=1.0) == EINVAL and call(zfar=float("inf")) == EINVAL
    assert spherical(perturb=p[9] + 1) == EINVAL and spherical(unit=0.0) == EINVAL and spherical(unit=float("nan")) == EINVAL
    assert rand(n_view=0) == EINVAL and rand(F=0) == EINVAL and rand(mode=2) == EINVAL and rand(rng=None) == EINVAL
    assert rand(R=1 << 20, n_view=1 << 5) == EINVAL
    assert rand(rng=(ctypes.c_double * 10)(*([float("nan")] + [0.0] * 9))) == EINVAL
