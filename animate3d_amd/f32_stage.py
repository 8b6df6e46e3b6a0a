"""The host layer shared by the fp32 4-D stage (``splat``, ``deform4d``, ``arap``, ``stage4d``): how its entry points are launched, what its inputs must
be, how work cached per tensor is keyed, the gather plan its atomic-free backward passes read, the workspace of its scalar losses.  No kernel of its own."""
from __future__ import annotations

import weakref
from typing import Tuple

import torch

from .hip_ops import _p, call, load_library


def launch(name: str, device: torch.device, *args):
    """Call the C-ABI entry point ``name(stream, *args)`` with ``device`` current and on ``device``'s current stream: the tensors behind
    ``args`` were allocated there, whichever device the caller has current.  A non-zero return code raises."""
    with torch.cuda.device(device):
        call(load_library(), name, torch.cuda.current_stream(device).cuda_stream, args)


def launch_reduced(name: str, device: torch.device, sizes, operands, n_sums: int, blocks, n_out: int) -> torch.Tensor:
    """``launch`` for a forward entry point that ends in csrc/loss_reduce.h's reduction, ``name(stream, *sizes, *operands, partials,
    n_partials, out)``.  ``blocks = (images, items, per_block)``: the entry point's grid is ``ceil(items / per_block)`` blocks per image.
    The fp32 workspace ``partials [n_sums, n_partials]`` (a column per block) and the returned ``out [n_out]`` are allocated here."""
    images, items, per_block = blocks
    n_partials = images * ((items + per_block - 1) // per_block)
    partials = torch.empty(n_sums, n_partials, dtype=torch.float32, device=device)
    out = torch.empty(n_out, dtype=torch.float32, device=device)
    launch(name, device, *sizes, *operands, _p(partials), n_partials, _p(out))
    return out


def require_shape(name: str, t, *shapes, non_empty: bool = False, optional: bool = False):
    """``t`` is a tensor (``TypeError``) of one of ``shapes`` (``ValueError``; none given: of any shape).  A size is an int, or a name that
    stands for any size; ``non_empty`` refuses a size of 0 as well, and ``optional`` lets ``None`` pass.  Device and dtype are
    ``require_f32_cuda``'s to check."""
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    have = tuple(t.shape)
    if not shapes or (have in shapes and not (non_empty and 0 in have)):        # the usual case, without a walk over the sizes
        return
    fits = any(len(s) == len(have) and all(isinstance(want, str) or want == h for want, h in zip(s, have)) for s in shapes)
    if not fits or (non_empty and 0 in have):
        spelled = " or ".join("[" + ", ".join(map(str, s)) + "]" for s in shapes)
        raise ValueError(f"{name}: expected {'a non-empty ' if non_empty else ''}{spelled}, got {list(have)}")


def _require_cuda(name: str, t, dtypes, label: str):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes):
        raise RuntimeError(f"{name}: expected {label} CUDA tensor, got {getattr(t, 'dtype', type(t))} on {getattr(t, 'device', '?')} "
                           "(no CPU fallback)")


def require_f32_cuda(name: str, t):
    _require_cuda(name, t, (torch.float32,), "a float32")


def require_index_cuda(name: str, t):
    _require_cuda(name, t, (torch.int32, torch.int64), "an int32 / int64")


class TensorKeyed:
    """Work cached for one tensor.  ``key`` is the tensor's data pointer, ``_version``, shape and device plus the parameters the work
    depends on; a weak reference pins the identity, since the address alone could be a later tensor on the same allocator block.  An
    in-place change, another tensor of equal contents and another parameter all stop ``matches``."""

    @staticmethod
    def _key(tensor: torch.Tensor, extra):
        return (tensor.data_ptr(), tensor._version, tuple(tensor.shape), str(tensor.device), *extra)

    def bind(self, tensor: torch.Tensor, *extra):
        self.key = self._key(tensor, extra)
        self._ref = weakref.ref(tensor)

    def matches(self, tensor: torch.Tensor, *extra) -> bool:
        return self._ref() is tensor and self.key == self._key(tensor, extra)


def gather_plan(ids: torch.Tensor, n_bins: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """ids [n] in [0, n_bins] -> (order [n] int32: the positions stable-sorted by id; starts [n_bins + 1] int32: the first sorted position
    of each bin).  Bin b's members are ``order[starts[b]:starts[b + 1]]`` in ascending position; id ``n_bins`` is the bucket of positions
    that belong to no bin, sorted last.  Fixed shapes, no host synchronisation."""
    srt, order = torch.sort(ids.long(), stable=True)
    starts = torch.searchsorted(srt, torch.arange(n_bins + 1, device=ids.device))
    return order.to(torch.int32).contiguous(), starts.to(torch.int32).contiguous()
