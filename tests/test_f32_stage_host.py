"""CPU checks of animate3d_amd/f32_stage.py, the host layer the fp32 4-D stage shares: the gather plan and the tensor-keyed cache (the
input check and the launch helper are exercised through splat, deform4d and arap: tests/test_*_host.py and tests/test_*_gpu.py)."""
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
