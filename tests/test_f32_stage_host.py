"""CPU checks of animate3d_amd/f32_stage.py, the host layer the fp32 4-D stage shares: the gather plan, the tensor-keyed cache, the
workspace of a reduced loss and the shape refusal (the device / dtype check and the launch helper are exercised through splat, deform4d,
arap and stage4d: tests/test_*_host.py and tests/test_*_gpu.py)."""
import pytest
import torch

from animate3d_amd import f32_stage


def test_gather_plan_sorts_stably_and_brackets_every_bin():
    n_bins = 5
    ids = torch.tensor([4, 0, 2, 5, 0, 4, 4, 2, 5, 0, 1, 1, 2, 0, 4, 5, 2, 2, 1, 0, 4, 0, 5, 2, 1, 4, 0, 2, 5, 1, 0, 4, 2, 2, 5, 0, 1])
    assert ids.numel() == 37 and 3 not in ids and int((ids == n_bins).sum()) == 6       # bin 3 is empty; 5 is the "no vertex" bucket
    order, starts = f32_stage.gather_plan(ids, n_bins)
    assert order.dtype == starts.dtype == torch.int32 and order.shape == (37,) and starts.shape == (n_bins + 1,)
    assert torch.equal(order.long(), torch.argsort(ids, stable=True))
    assert bool((starts[1:] >= starts[:-1]).all()) and int(starts[0]) == 0
    assert int(starts[n_bins]) == int((ids < n_bins).sum()) == 31
    assert int(starts[3]) == int(starts[4])                                             # the empty bin
    for b in range(n_bins):
        assert order[starts[b]:starts[b + 1]].tolist() == [i for i in range(37) if int(ids[i]) == b]
    order32, starts32 = f32_stage.gather_plan(ids.to(torch.int32), n_bins)              # deform4d's cells are int32
    assert torch.equal(order32, order) and torch.equal(starts32, starts)


def test_tensor_keyed_follows_identity_version_and_parameters():
    x = torch.rand(12, 3)
    entry = f32_stage.TensorKeyed()
    entry.bind(x, 3, 0.01)
    assert entry.matches(x, 3, 0.01)
    assert entry.key == (x.data_ptr(), x._version, (12, 3), "cpu", 3, 0.01)
    assert not entry.matches(x, 4, 0.01) and not entry.matches(x, 3, None) and not entry.matches(x, 3)     # another parameter
    assert not entry.matches(x.clone(), 3, 0.01)                                        # equal contents, another tensor
    assert not entry.matches(x[:6], 3, 0.01) and not entry.matches(x.view(3, 12), 3, 0.01)
    x.add_(0)                                                                           # in place: same values, next version
    assert not entry.matches(x, 3, 0.01)
    entry.bind(x, 3, 0.01)
    assert entry.matches(x, 3, 0.01)
    other = f32_stage.TensorKeyed()
    other.bind(x, 3, 0.02)
    assert other.key != entry.key


def test_launch_reduced_sizes_the_workspace_by_the_grid_and_returns_out(monkeypatch):
    calls = []
    monkeypatch.setattr(f32_stage, "launch", lambda name, device, *args: calls.append((name, device, args)))
    dev = torch.device("cpu")                                                           # the allocations need no GPU; the launch is recorded
    for blocks, n_partials in (((2, 2145, 2048), 4), ((2, 2048, 2048), 2), ((1, 3000, 1024), 3), ((1, 1, 1024), 1), ((3, 8193, 8192), 6)):
        calls.clear()
        out = f32_stage.launch_reduced("a3d_some_loss_f32", dev, (2, 5, 7), (11, None, 0.5), 5, blocks, 4)
        (name, device, args), = calls
        assert name == "a3d_some_loss_f32" and device is dev
        assert args[:6] == (2, 5, 7, 11, None, 0.5) and args[7] == n_partials and len(args) == 9
        assert out.shape == (4,) and out.dtype == torch.float32 and args[8] == out.data_ptr()
        assert isinstance(args[6], int) and args[6] not in (0, out.data_ptr())          # the workspace [5, n_partials], dropped after the call


def test_require_shape_refuses_by_type_then_shape_and_names_what_it_expected():
    t = torch.zeros(2, 1, 5, 7)
    f32_stage.require_shape("alpha", t, (2, 1, 5, 7), (2, 5, 7))
    f32_stage.require_shape("alpha", t[:, 0], (2, 1, 5, 7), (2, 5, 7))
    f32_stage.require_shape("alpha", t)                                                 # no shape given: any tensor
    f32_stage.require_shape("image", t, ("B", 1, "H", "W"), non_empty=True)             # a name stands for any size
    f32_stage.require_shape("gt", torch.zeros(0, 5, 7, 3), ("S", 5, 7, 3))              # ... 0 too, unless non_empty
    f32_stage.require_shape("depth", None, (2, 1, 5, 7), optional=True)
    for bad in (None, [[1.0]], 3.0):
        with pytest.raises(TypeError, match="alpha: expected a tensor"):
            f32_stage.require_shape("alpha", bad, (2, 1, 5, 7))
    with pytest.raises(TypeError):
        f32_stage.require_shape("alpha", [1.0], optional=True)                          # optional admits None only
    with pytest.raises(ValueError, match=r"alpha: expected \[2, 1, 5, 7\] or \[2, 5, 7\], got \[2, 7, 5\]"):
        f32_stage.require_shape("alpha", torch.zeros(2, 7, 5), (2, 1, 5, 7), (2, 5, 7))
    with pytest.raises(ValueError, match=r"image: expected a non-empty \[B, 3, H, W\], got \[2, 1, 5, 7\]"):
        f32_stage.require_shape("image", t, ("B", 3, "H", "W"), non_empty=True)
    with pytest.raises(ValueError, match="non-empty"):
        f32_stage.require_shape("image", torch.zeros(2, 3, 0, 7), ("B", 3, "H", "W"), non_empty=True)
    with pytest.raises(ValueError):
        f32_stage.require_shape("image", torch.zeros(3, 5, 7), ("B", 3, "H", "W"))      # another rank
    with pytest.raises(ValueError):
        f32_stage.require_shape("scaling", torch.zeros(0, 3), (0, 3), non_empty=True)   # the sizes fit, and one of them is 0
