"""GPU checks of the frames layer (animate3d_amd/frames.py on csrc/stage_frames.hip, stage4d.masked_recon_loss_rgba8 on the rgba8 pair
of csrc/recon_loss.hip).  Nothing here has a tolerance: the kernels compute what tests/frames_ref.py's numpy lines compute (integer sums,
one IEEE fp32 division, a truncating cast), and the 8-bit loss computes what the fp32 loss computes on the unpacked tensors, so every
comparison is ``torch.equal`` / ``np.array_equal``.  tests/test_frames_host.py holds the arithmetic claims this rests on (a reciprocal
multiply differs from the division for 126 of the 256 bytes; quantising ``b / 255`` gives ``b`` back for all 256)."""
import copy
import os

import numpy as np
import pytest
import torch

from animate3d_amd import cameras, deform4d, frames, stage4d
from tests import frames_ref as R
from tests import stage4d_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_frames.npz")


def _np(t):
    return t.detach().cpu().numpy()


def _check_unpack(src, k):
    """All three outputs of one launch, and each alone, against the restatement; returns the reduced bytes."""
    want8 = R.box_reduce_ref(src, k)
    want_rgb, want_mask = R.unpack_ref(want8)
    dev = torch.from_numpy(src).cuda()
    got = frames.unpack_rgba8(dev, k, out8=True, rgb=True, mask=True)
    assert got["out8"].dtype == torch.uint8 and got["rgb"].dtype == torch.float32 and got["mask"].dtype == torch.bool
    assert np.array_equal(_np(got["out8"]), want8)
    assert np.array_equal(_np(got["rgb"]).view(np.uint32), want_rgb.view(np.uint32))          # bit for bit
    assert got["mask"].shape == (*want8.shape[:3], 1) and np.array_equal(_np(got["mask"]), want_mask)
    for name in ("out8", "rgb", "mask"):
        alone = frames.unpack_rgba8(dev, k, **{name: True})
        assert set(alone) == {name} and torch.equal(alone[name], got[name])
    return want8


def test_unpack_every_byte_value():
    b = np.arange(256, dtype=np.int64).reshape(16, 16)
    src = np.stack([b, (b * 7 + 3) % 256, 255 - b, (b + 128) % 256], -1).astype(np.uint8)[None]
    assert all(len(np.unique(src[..., c])) == 256 for c in range(4))
    assert np.array_equal(_check_unpack(src, 1), src)                                          # k = 1 is a copy
    fs = frames.FrameSet(torch.from_numpy(src).cuda(), 1, 1)
    want_rgb, want_mask = R.unpack_ref(src)
    assert np.array_equal(_np(fs.rgb()).view(np.uint32), want_rgb.view(np.uint32)) and np.array_equal(_np(fs.mask()), want_mask)
    assert fs.batch()["rgba8"] is fs.rgba8 and (fs.height, fs.width) == (16, 16)


def _box_source(S, h, w, seed):
    """Random bytes with, in every image, 2 x 2 quads whose sum is 2 (mod 4) (the ties: mean x.5), alpha quads that average 127.5 exactly,
    and saturated quads."""
    src = np.random.default_rng(seed).integers(0, 256, (S, h, w, 4), dtype=np.uint8)
    src[:, 0:2, 0:2] = np.array([[10, 11], [11, 12]], np.uint8)[None, :, :, None]             # sum 44: mean 11 exactly
    src[:, 0:2, 2:4] = np.array([[10, 11], [11, 10]], np.uint8)[None, :, :, None]             # sum 42 = 2 (mod 4): 10.5 -> 11
    src[:, 2:4, 0:2, 3] = np.array([[127, 128], [128, 127]], np.uint8)                        # 127.5 -> 128: inside
    src[:, 2:4, 2:4, 3] = np.array([[127, 127], [128, 127]], np.uint8)                        # 127.25 -> 127: outside
    src[:, 0:4, 4:8, 3] = np.resize(np.array([127, 128], np.uint8), 16).reshape(4, 4)         # the 4 x 4 block averages 127.5 too
    src[:, 4:8, 0:4] = 255
    src[:, 4:8, 4:8] = 0
    return src


@pytest.mark.parametrize("S,h,w,k", [(1, 8, 8, 2), (1, 8, 8, 4), (3, 12, 8, 2), (2, 8, 8, 1), (2, 48, 32, 16), (5, 9, 15, 3)])
def test_box_rule(S, h, w, k):
    src = _box_source(S, max(h, 8), max(w, 8), 11 * k + S)[:, :h, :w].copy()
    got = _check_unpack(src, k)
    if k == 2:
        assert got[0, 0, 0].tolist()[:3] == [11, 11, 11] and got[0, 0, 1].tolist()[:3] == [11, 11, 11]
        assert got[0, 1, 0, 3] == 128 and got[0, 1, 1, 3] == 127
    if k == 4 and h == 8:
        assert got[0, 0, 1, 3] == 128 and got[0, 1, 0].tolist() == [255] * 4 and got[0, 1, 1].tolist() == [0] * 4
    if k == 1:
        assert np.array_equal(got, src)
    with pytest.raises(ValueError, match="divides"):
        frames.unpack_rgba8(torch.from_numpy(src).cuda(), 7, out8=True)


# ---- the 8-bit loss against the fp32 loss on the unpacked tensors

S_GT, B_IM = 6, 4
LOSS_KW = dict(bg=stage4d_ref.BG[0], lambda_rgb=stage4d_ref.LOSS["lambda_rgb"], lambda_mask=stage4d_ref.LOSS["lambda_mask"])


def _ground_truth(h, w, offset):
    """uint8 [S_GT, h, w, 4] on the device, every byte value in it; ``offset``: a view that starts one pixel into a 16-byte aligned buffer."""
    n = S_GT * h * w * 4
    host = torch.from_numpy(np.random.default_rng(h * w).integers(0, 256, n, dtype=np.uint8))
    m = min(n, 1024)
    host[:m] = (torch.arange(m) % 256).to(torch.uint8)
    host[3:m:4] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8).repeat(64)[:m // 4]     # alpha on both sides of the threshold
    buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[4:4 + n] if offset else buf[:n]
    view.copy_(host)
    view = view.view(S_GT, h, w, 4)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 if offset else 0)
    return view


@pytest.fixture(scope="module", params=[(48, 48, False), (5, 7, False), (48, 48, True)], ids=["48x48-vector", "5x7-scalar", "48x48-offset-scalar"])
def loss_case(request):
    """48 x 48: 2 304 pixels, two blocks an image, the 16-byte path; 5 x 7: the scalar path with a tail; 48 x 48 from a 4-byte base: the
    scalar path on a size the 16-byte path would take.  The fp32 reference is computed once per shape and shared."""
    h, w, offset = request.param
    gt8 = _ground_truth(h, w, offset)
    unpacked = frames.unpack_rgba8(gt8, rgb=True, mask=True)
    want_rgb, want_mask = R.unpack_ref(_np(gt8))
    assert np.array_equal(_np(unpacked["rgb"]).view(np.uint32), want_rgb.view(np.uint32)) and np.array_equal(_np(unpacked["mask"]), want_mask)
    renders = {B: tuple(t.cuda() for t in stage4d_ref.make_render(f"frames/{h}x{w}/{B}", B, h, w)) for B in (B_IM, S_GT)}
    rgb = unpacked["rgb"]
    if offset:
        # each loss picks its path from the alignment of its own operands, and the two paths add a thread's pixels in different orders:
        # the fp32 ground truth gets the same kind of base as the bytes (one element into a 16-byte aligned buffer), so both run the
        # 4-byte path
        buf = torch.zeros(rgb.numel() + 4, dtype=torch.float32, device="cuda")
        buf[1:1 + rgb.numel()].copy_(rgb.reshape(-1))
        rgb = buf[1:1 + rgb.numel()].view(rgb.shape)
        assert rgb.is_contiguous() and rgb.data_ptr() % 16 == 4 and torch.equal(rgb, unpacked["rgb"])
    return dict(gt8=gt8, rgb=rgb, mask=unpacked["mask"], renders=renders)


def _both(case, B, index, need=(True, True)):
    """(outputs, d_image, d_alpha) of the 8-bit loss and of the fp32 loss on the same render, upstream gradient 0.75."""
    results = []
    for which in ("u8", "f32"):
        image, alpha = (t.clone().requires_grad_(n) for t, n in zip(case["renders"][B], need))
        if which == "u8":
            out = stage4d.masked_recon_loss_rgba8(image, alpha, case["gt8"], index, **LOSS_KW)
        else:
            out = stage4d.masked_recon_loss(image, alpha, case["rgb"], case["mask"], index, **LOSS_KW)
        (out[0] * 0.75).backward()
        results.append((out, image.grad, alpha.grad))
    return results


@pytest.mark.parametrize("index", [[5, 0, 3, 3], [2, 2, 2, 1], None], ids=["permuted", "repeated", "identity"])
def test_rgba8_loss_is_the_f32_loss_bitwise(loss_case, index):
    B = S_GT if index is None else B_IM
    dev_index = None if index is None else torch.tensor(index, dtype=torch.int64, device="cuda")
    (out8, di8, da8), (out32, di32, da32) = _both(loss_case, B, dev_index)
    for a, b, name in zip(out8, out32, ("loss", "loss_rgb", "loss_mask")):
        assert torch.equal(a, b), f"{name}: {float(a)!r} against {float(b)!r}"
    assert torch.equal(di8, di32) and torch.equal(da8, da32)
    assert float(out8[1]) > 0 and float(out8[2]) > 0 and bool((di8 == 0).any()) and bool((di8 != 0).any())     # clamped and passing values
    if index is not None:                                                                      # a host list is the same index
        again = stage4d.masked_recon_loss_rgba8(*loss_case["renders"][B], loss_case["gt8"], index, **LOSS_KW)
        assert all(torch.equal(a, b) for a, b in zip(again, out8))


@pytest.mark.parametrize("need", [(True, False), (False, True)], ids=["d_image-only", "d_alpha-only"])
def test_rgba8_loss_single_gradient(loss_case, need):
    index = torch.tensor([1, 4, 4, 0], dtype=torch.int32, device="cuda")
    (out8, di8, da8), (out32, di32, da32) = _both(loss_case, B_IM, index, need)
    assert all(torch.equal(a, b) for a, b in zip(out8, out32))
    for got, want, needed in ((di8, di32, need[0]), (da8, da32, need[1])):
        assert (got is None and want is None) if not needed else torch.equal(got, want)


def test_rgba8_loss_twice_is_bitwise_equal(loss_case):
    index = torch.tensor([5, 0, 3, 3], dtype=torch.int32, device="cuda")
    first, second = (_both(loss_case, B_IM, index)[0] for _ in range(2))
    assert all(torch.equal(a, b) for a, b in zip(first[0], second[0])) and torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])


def test_rgba8_loss_refusals(loss_case):
    image, alpha = loss_case["renders"][B_IM]
    gt8 = loss_case["gt8"]
    with pytest.raises(ValueError, match="S == B"):
        stage4d.masked_recon_loss_rgba8(image, alpha, gt8, None, **LOSS_KW)
    with pytest.raises(IndexError):
        stage4d.masked_recon_loss_rgba8(image, alpha, gt8, [0, 1, 2, S_GT], **LOSS_KW)
    with pytest.raises(ValueError, match="gt_rgba8"):
        stage4d.masked_recon_loss_rgba8(image, alpha, gt8[..., :3], [0, 1, 2, 3], **LOSS_KW)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stage4d.masked_recon_loss_rgba8(image, alpha, gt8.cpu(), [0, 1, 2, 3], **LOSS_KW)
    flat = torch.zeros(gt8.numel() + 16, dtype=torch.uint8, device="cuda")
    off1 = flat[1:1 + gt8.numel()].view(gt8.shape)                                             # a base off 4 bytes: refused by the entry point
    with pytest.raises(RuntimeError, match="A3D_EINVAL"):
        stage4d.masked_recon_loss_rgba8(image, alpha, off1, [0, 1, 2, 3], **LOSS_KW)


def test_cabi_refusals_with_a_device_present():
    """tests/test_frames_contract.py's checks again, on the machine that has a GPU: every refusal returns before a launch here too (the
    addresses are made up; nothing may reach the device)."""
    from animate3d_amd import hip_ops
    from tests import test_frames_contract as C
    lib = hip_ops.load_library()
    for entry in ("a3d_recon_loss_rgba8_f32", "a3d_recon_loss_rgba8_bwd_f32"):
        C.test_rgba8_loss_refuses_misaligned_or_missing_operand(lib, entry)
        C.test_rgba8_loss_refuses_bad_sizes(lib, entry)
    C.test_unpack_refusals(lib)
    C.test_pack_refusals(lib)
    torch.cuda.synchronize()


# ---- pack

@pytest.mark.parametrize("option", ["testset", "four_view"])
def test_pack_gives_the_reference_bytes(option):
    want = np.load(GOLDEN)[f"{option}_rgba"]
    renders = [R.make_render(R.render_key(option, i)) for i in range(R.COUNTS[option])]
    image, alpha = torch.stack([r[0] for r in renders]).cuda(), torch.stack([r[1] for r in renders]).cuda()
    got = frames.pack_rgba8(image, alpha)
    assert got.shape == want.shape and got.dtype == torch.uint8 and np.array_equal(_np(got), want)
    assert torch.equal(frames.pack_rgba8(image, alpha[:, 0]), got)                             # alpha [B, H, W]


def test_pack_random_against_numpy():
    g = torch.Generator().manual_seed(3)
    image, alpha = torch.rand(3, 3, 17, 19, generator=g) * 2 - 0.5, torch.rand(3, 1, 17, 19, generator=g) * 2 - 0.5     # 969 pixels: 4 blocks
    image.view(-1)[:4] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    want = np.concatenate([image.permute(0, 2, 3, 1).numpy(), alpha.permute(0, 2, 3, 1).numpy()], -1)
    want = (np.clip(np.nan_to_num(want, nan=0.0), 0, 1) * 255).astype(np.uint8)
    out = torch.full((3, 17, 19, 4), 7, dtype=torch.uint8, device="cuda")
    got = frames.pack_rgba8(image.cuda(), alpha.cuda(), out=out)
    assert got is out and np.array_equal(_np(got), want)
    assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) == 256
    with pytest.raises(ValueError, match="out"):
        frames.pack_rgba8(image.cuda(), alpha.cuda(), out=out[:2])


# ---- the chain: render -> files -> load -> step

N_GAUSS, SIDE, N_VIEW, N_FRAME = 64, 16, 2, 3


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    g = torch.Generator().manual_seed(21)
    gaussians = stage4d.Gaussians(xyz=(torch.randn(N_GAUSS, 3, generator=g) * 0.25).cuda(),
                                  scaling=(torch.rand(N_GAUSS, 3, generator=g) * 1.0 - 2.6).cuda(),
                                  rotation=torch.randn(N_GAUSS, 4, generator=g).cuda(),
                                  opacity=torch.sigmoid(torch.randn(N_GAUSS, 1, generator=g) + 1.0).cuda(),
                                  shs=(torch.randn(N_GAUSS, 1, 3, generator=g) * 0.5).cuda(), sh_degree=0)
    field = deform4d.HexPlaneDeformation(((4, 4, 4, 2), (6, 6, 6, 3)), use_global_trans=True)
    with torch.no_grad():
        for name, p in field.named_parameters():
            if name.endswith("layers.2.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    cams = cameras.data_view_cameras(default_elevation_deg=12.0, default_azimuth_deg=[0.0, 95.0], default_camera_distance=2.2, default_fovy_deg=45.0,
                                     n_view=N_VIEW, total_frame=N_FRAME, height=SIDE, width=SIDE, device="cuda")
    field = field.cuda()
    bg = torch.tensor(stage4d_ref.BG, device="cuda")
    rendered = frames.test_renders(field, gaussians, cams, bg, do_guidance=False, chunk=4)     # 6 images: a chunk of 4 and a short one of 2
    save_dir = str(tmp_path_factory.mktemp("recon"))
    paths = frames.write_test_renders(save_dir, rendered, n_frame=N_FRAME, test_option="four_view")
    return dict(gaussians=gaussians, field=field, cams=cams, bg=bg, rendered=rendered, save_dir=save_dir, paths=paths)


def test_chain_renders_come_back_from_the_files(chain):
    rendered = chain["rendered"]
    assert rendered.shape == (N_VIEW * N_FRAME, SIDE, SIDE, 4) and rendered.dtype == torch.uint8
    host = _np(rendered)
    assert host[..., 3].max() >= 128 and host[..., 3].min() < 128 and host[..., :3].std() > 1      # a picture: inside and outside
    assert not np.array_equal(host[0], host[N_FRAME])                                              # the two views differ
    with torch.no_grad():
        r = stage4d.render_batch(chain["field"], chain["gaussians"], None, None, None, None, None, chain["bg"], do_guidance=False,
                                 cameras=chain["cams"].take(range(4, 6)))
    assert torch.equal(frames.pack_rgba8(r["image"], r["alpha"]), rendered[4:6])                   # the short chunk is that render, packed
    assert chain["paths"] == [os.path.join("images", f"{i}.png") for i in range(N_VIEW * N_FRAME)]
    root = os.path.join(chain["save_dir"], "images")
    fs = frames.load_frames(root, SIDE, SIDE, n_view=N_VIEW, n_frame=N_FRAME, device="cuda")
    assert fs.rgba8.is_cuda and torch.equal(fs.rgba8, rendered) and (fs.n_view, fs.n_frame) == (N_VIEW, N_FRAME)
    half = frames.load_frames(root, SIDE // 2, SIDE // 2, n_view=N_VIEW, n_frame=N_FRAME)
    assert np.array_equal(_np(half.rgba8), R.box_reduce_ref(host, 2))
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        frames.load_frames(root, 12, 12, n_view=N_VIEW, n_frame=N_FRAME)
    traj = stage4d.vertex_trajectory(chain["field"], chain["gaussians"], chain["cams"].frames)
    written = frames.write_trajectory(chain["save_dir"], traj)
    assert written == [os.path.join("mesh_trajectory", f"{t}.npy") for t in range(N_FRAME)]
    for t, rel in enumerate(written):
        assert np.array_equal(np.load(os.path.join(chain["save_dir"], rel)), _np(traj[t]))


def _step_kwargs():
    return dict(loss=dict(stage4d_ref.LOSS, lambda_arap=0.0), global_step=25, n_view=N_VIEW, n_frame=N_FRAME, progressive_iter_per_frame=10,
                bg=stage4d_ref.BG)


def _field_grads(field):
    grads = {name: p.grad.clone() for name, p in field.named_parameters() if p.grad is not None}
    for p in field.parameters():
        p.grad = None
    return grads


def test_training_step_on_rgba8_is_the_step_on_rgb_and_mask(chain):
    field, g = chain["field"], chain["gaussians"]
    fs = frames.load_frames(os.path.join(chain["save_dir"], "images"), SIDE, SIDE, n_view=N_VIEW, n_frame=N_FRAME)
    batches = {"set": dict(rgba8=fs, cameras=chain["cams"]), "tensor": dict(fs.batch(), cameras=chain["cams"]),
               "f32": dict(rgb=fs.rgb(), mask=fs.mask(), cameras=chain["cams"])}
    assert batches["f32"]["rgb"].shape == (6, SIDE, SIDE, 3) and batches["f32"]["mask"].shape == (6, SIDE, SIDE, 1)
    outs, grads = {}, {}
    for name, batch in batches.items():
        outs[name] = stage4d.training_step(field, g, batch, generator=torch.Generator(device="cuda").manual_seed(17), **_step_kwargs())
        outs[name]["loss"].backward()
        grads[name] = _field_grads(field)
    assert len(grads["f32"]) > 0 and any(bool(v.abs().max() > 0) for v in grads["f32"].values())
    for name in ("set", "tensor"):
        assert set(outs[name]) == set(outs["f32"]) >= {"loss", "loss_rgb", "loss_mask"}
        for key in outs["f32"]:
            assert torch.equal(outs[name][key], outs["f32"][key]), (name, key)
        assert set(grads[name]) == set(grads["f32"])
        for key in grads["f32"]:
            assert torch.equal(grads[name][key], grads["f32"][key]), (name, key)
    with pytest.raises(ValueError, match="both"):
        stage4d.training_step(field, g, dict(batches["f32"], rgba8=fs), **_step_kwargs())
    with pytest.raises(ValueError, match="neither"):
        stage4d.training_step(field, g, dict(cameras=chain["cams"]), **_step_kwargs())


def test_fit_runs_on_a_frame_set(chain):
    field = copy.deepcopy(chain["field"])
    fs = frames.FrameSet(chain["rendered"], N_VIEW, N_FRAME)
    before = {name: p.detach().clone() for name, p in field.named_parameters()}
    opt = torch.optim.Adam(field.parameters(), lr=1e-3)
    kw = _step_kwargs()
    kw.pop("global_step")
    logs = stage4d.fit(field, chain["gaussians"], dict(rgba8=fs, cameras=chain["cams"]), opt, steps=3, start_step=24,
                       generator=torch.Generator(device="cuda").manual_seed(5), **kw)
    assert {"loss", "loss_rgb", "loss_mask"} <= set(logs)
    for key in ("loss", "loss_rgb", "loss_mask"):
        assert logs[key].shape == (3,) and bool(torch.isfinite(logs[key]).all()), key
    assert any(not torch.equal(p.detach(), before[name]) for name, p in field.named_parameters())
