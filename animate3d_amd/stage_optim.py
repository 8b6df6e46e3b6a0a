"""The optimiser of the 4-D stage: the reference's rate schedule, its Adam on the gfx950 kernels of csrc/stage_optim.hip, and the step
that is dropped when a gradient is not finite.

The reference builds ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` over five named groups (``Gaussian4DModel.training_setup``,
custom/threestudio-animate3d/geometry/gaussian_4d.py:344-391), sets every group's rate before each step from
``C(value, 0, iteration, interpolation="exp")`` (``update_learning_rate``, :393-446) and trains under ``precision: 16-mixed``, where
Lightning's ``GradScaler`` drops a step whose gradients hold an inf or a NaN.  This stage is fp32 and needs no loss scale; a non-finite
SDS gradient still happens, and one of them in ``exp_avg`` / ``exp_avg_sq`` stays there for the rest of the run.

``scheduled(value, global_step, interpolation="linear", epoch=0) -> float``: threestudio's ``C`` (threestudio/utils/misc.py:66-101) in
Python floats, with the same expressions in the same order.  A number passes through; a list of 3 ``[start_value, end_value, end_step]``,
4 ``[start_step, start_value, end_value, end_step]`` or 6 and more elements (4 plus further ``end_value, end_step`` pairs) is
interpolated, ``"linear"`` or ``"exp"``; an int ``end_step`` reads ``global_step``, a float one ``epoch``.  What ``C`` refuses raises
what ``C`` raises (``TypeError`` for another type, ``AssertionError`` for another length, ``ValueError`` for another interpolation).

``StageAdam(groups, betas=(0.9, 0.999), eps=1e-15)``: a ``torch.optim.Optimizer`` with exactly the update of ``torch.optim.Adam`` without
``amsgrad``, ``weight_decay`` or ``maximize`` (each refused), computed in fp64 per element and rounded to fp32 once (the bars are in
tests/stage_optim_ref.py).  ``groups``: dicts of ``params``, ``lr`` and optionally ``name`` and ``schedule`` (the config value handed to
``scheduled``).  The parameters are fp32 and contiguous and each in one group (``ValueError`` / ``TypeError`` at construction, which
needs no device); they are updated where they are.  ``exp_avg``, ``exp_avg_sq`` and ``step`` (one fp32 per parameter, on the
parameter's device, as torch keeps it for capturable state) exist from construction on and never move.

* ``step()``: every parameter with a gradient goes through ``a3d_stage_adam_f32``, each with its own ``step`` and its group's ``lr``; one
  without (``.grad is None``) is left out, its step count included: torch's rule.  Nothing to update launches nothing.  If any element of
  any gradient is an inf or a NaN, no parameter, moment or step count changes and ``skipped`` (``[1]`` int32 on the device) reads 1;
  otherwise it reads 0.  The test is made on the device: ``step()`` synchronises with nothing and runs no torch arithmetic.  More than
  ``hip_ops.STAGE_ADAM_MAX_TENSORS`` parameters take several calls; the test still covers all of them before any is updated.  A sparse
  gradient, one of another dtype or device, or a non-contiguous one raises.
* ``update_learning_rate(global_step)``: ``lr = scheduled(schedule, global_step, "exp")`` for every group with a schedule
  (gaussian_4d.py:427-446).  Host arithmetic.
* ``state_dict()`` / ``load_state_dict()``: torch's layout, so that ``torch.optim.Adam(groups, lr=0.0, eps=1e-15)`` loads ours and ours
  loads its state.  Loading copies into the tensors that exist; a parameter the loaded state does not know starts from zero.
* ``StageAdam.for_field(field, *, delta_xyz_network_lr, ...)``: the reference's groups by ``stage4d.field_param_groups``' name matching;
  each rate a number or a schedule, the initial ``lr`` being ``scheduled(value, 0)`` as in ``training_setup``.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import torch

from .f32_stage import launch, require_f32_cuda
from .hip_ops import (STAGE_ADAM_BEGIN, STAGE_ADAM_CHECK, STAGE_ADAM_MAX_TENSORS, STAGE_ADAM_UPDATE, StageAdamEntry, _p)

REFUSED_OPTIONS = ("weight_decay", "amsgrad", "maximize")
FIELD_RATES = ("delta_xyz_network", "delta_rot_network", "delta_scaling_network", "grid", "global_trans")


def scheduled(value, global_step: int, interpolation: str = "linear", epoch: int = 0) -> float:
    """threestudio's ``C(value, epoch, global_step, interpolation)``; see the module docstring."""
    if isinstance(value, int) or isinstance(value, float):
        pass
    else:
        value = list(value) if isinstance(value, tuple) else value
        if not isinstance(value, list):
            raise TypeError("Scalar specification only supports list, got", type(value))
        if len(value) == 3:
            value = [0] + value
        if len(value) >= 6:
            select_i = 3
            for i in range(3, len(value) - 2, 2):
                if global_step >= value[i]:
                    select_i = i + 2
            if select_i != 3:
                start_value, start_step = value[select_i - 3], value[select_i - 2]
            else:
                start_step, start_value = value[:2]
            end_value, end_step = value[select_i - 1], value[select_i]
            value = [start_step, start_value, end_value, end_step]
        assert len(value) == 4
        start_step, start_value, end_value, end_step = value
        if isinstance(end_step, int):
            current_step = global_step
        elif isinstance(end_step, float):
            current_step = epoch
        t = max(min(1.0, (current_step - start_step) / (end_step - start_step)), 0.0)
        if interpolation == "linear":
            value = start_value + (end_value - start_value) * t
        elif interpolation == "exp":
            value = math.exp(math.log(start_value) * (1 - t) + math.log(end_value) * t)
        else:
            raise ValueError(f"Unknown interpolation method: {interpolation}, only support linear and exp")
    return value


class StageAdam(torch.optim.Optimizer):
    """Adam of the 4-D stage on csrc/stage_optim.hip; see the module docstring."""

    def __init__(self, groups: Sequence[Dict], betas=(0.9, 0.999), eps: float = 1e-15, **options):
        for name in REFUSED_OPTIONS:
            if options.pop(name, 0):
                raise NotImplementedError(f"{name}: not built (no released config of the 4-D stage sets it)")
        if options:
            raise TypeError(f"StageAdam: unknown options {sorted(options)}")
        groups = [dict(g) for g in groups]
        if not groups or not all(isinstance(g, dict) and "params" in g and "lr" in g for g in groups):
            raise ValueError("StageAdam: groups are dicts with 'params' and 'lr' (and optionally 'name' and 'schedule')")
        for g in groups:
            g["params"] = [g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])
            for p in g["params"]:
                if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
                    raise TypeError(f"StageAdam: parameters are float32 tensors, got {getattr(p, 'dtype', type(p))}")
                if not p.is_contiguous():
                    raise ValueError(f"StageAdam: a non-contiguous parameter of shape {tuple(p.shape)} (it is updated where it is)")
            g.setdefault("schedule", None)
        flat = [p for g in groups for p in g["params"]]
        if len({id(p) for p in flat}) != len(flat):
            raise ValueError("StageAdam: a parameter appears in more than one group")
        if len({p.device for p in flat}) > 1:
            raise ValueError(f"StageAdam: parameters on several devices {sorted({str(p.device) for p in flat})}")
        # torch.optim.Adam reads every one of these from a group it has loaded
        defaults = dict(lr=0.0, betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=0, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(groups, defaults)
        self._check_groups(self.param_groups)
        for p in flat:
            self.state[p] = dict(step=torch.zeros((), dtype=torch.float32, device=p.device),
                                 exp_avg=torch.zeros_like(p, memory_format=torch.contiguous_format),
                                 exp_avg_sq=torch.zeros_like(p, memory_format=torch.contiguous_format))
        self.skipped = torch.zeros(1, dtype=torch.int32, device=flat[0].device if flat else None)
        self._tables: Dict[tuple, List] = {}                    # (addresses of the parameters with a gradient) -> [ctypes table per call]

    @staticmethod
    def _check_groups(groups):
        for g in groups:
            for name in REFUSED_OPTIONS:
                if g.get(name, 0):
                    raise NotImplementedError(f"{name} = {g[name]!r}: not built (no released config of the 4-D stage sets it)")
            lr, (b1, b2), eps = g["lr"], g["betas"], g["eps"]
            if not (isinstance(lr, (int, float)) and math.isfinite(lr) and lr >= 0.0):
                raise ValueError(f"lr = {lr!r}: expected a finite number >= 0")
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise ValueError(f"betas = {(b1, b2)}: expected both in [0, 1)")
            if not (math.isfinite(eps) and eps >= 0.0):
                raise ValueError(f"eps = {eps!r}: expected a finite number >= 0")
        if len({(tuple(g["betas"]), g["eps"]) for g in groups}) > 1:
            raise NotImplementedError("betas / eps that differ between groups: one call takes one set")

    @classmethod
    def for_field(cls, field, *, delta_xyz_network_lr, delta_rot_network_lr, delta_scaling_network_lr, grid_lr, global_trans_lr=0.0,
                  betas=(0.9, 0.999), eps: float = 1e-15) -> "StageAdam":
        """The reference's groups (``training_setup``) for a ``deform4d.HexPlaneDeformation``; each rate a number or a schedule."""
        from .stage4d import field_param_groups                  # stage4d's fit takes any optimiser: it does not import this module
        rates = dict(delta_xyz_network=delta_xyz_network_lr, delta_rot_network=delta_rot_network_lr,
                     delta_scaling_network=delta_scaling_network_lr, grid=grid_lr, global_trans=global_trans_lr)
        groups = field_param_groups(field, **{f"{name}_lr": 0.0 for name in FIELD_RATES})
        for g in groups:
            value = rates[g["name"]]
            g["lr"] = scheduled(value, 0)
            g["schedule"] = value if isinstance(value, int) or isinstance(value, float) else list(value)
        return cls(groups, betas=betas, eps=eps)

    def update_learning_rate(self, global_step: int):
        for g in self.param_groups:
            if g.get("schedule") is not None:
                g["lr"] = scheduled(g["schedule"], global_step, "exp")

    def _table_for(self, key, entries):
        """The ctypes tables of this set of parameters: everything but ``g`` and ``lr`` is fixed, so they are filled once."""
        tables = []
        for at in range(0, len(entries), STAGE_ADAM_MAX_TENSORS):
            part = entries[at:at + STAGE_ADAM_MAX_TENSORS]
            table = (StageAdamEntry * len(part))()
            for e, (p, _) in zip(table, part):
                st = self.state[p]
                e.p, e.m, e.v, e.step, e.n = _p(p), _p(st["exp_avg"]), _p(st["exp_avg_sq"]), _p(st["step"]), p.numel()
            tables.append(table)
        self._tables = {key: tables}                            # one set is kept: the usual run has one
        return tables

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups(self.param_groups)
        entries, key = [], []
        for g in self.param_groups:
            for p in g["params"]:
                grad = p.grad
                if grad is not None:
                    if grad.is_sparse:
                        raise RuntimeError("StageAdam: a sparse gradient (the kernel reads dense fp32)")
                    require_f32_cuda("parameter", p)
                    if grad.dtype != torch.float32 or grad.device != p.device:
                        raise RuntimeError(f"StageAdam: a gradient of {grad.dtype} on {grad.device} for a float32 parameter on {p.device}")
                    if not grad.is_contiguous():
                        raise RuntimeError("StageAdam: a non-contiguous gradient")
                    entries.append((p, float(g["lr"])))
                    key.append(p.data_ptr())
        if not entries:
            return loss
        key = tuple(key)
        tables = self._tables.get(key) or self._table_for(key, entries)
        at = 0
        for table in tables:
            for e in table:
                p, lr = entries[at]
                e.g, e.lr = _p(p.grad), lr
                at += 1
        group = self.param_groups[0]
        consts = (group["betas"][0], group["betas"][1], group["eps"])
        device, flag = entries[0][0].device, _p(self.skipped)
        if len(tables) == 1:
            launch("a3d_stage_adam_f32", device, tables[0], len(tables[0]), *consts, STAGE_ADAM_BEGIN | STAGE_ADAM_CHECK | STAGE_ADAM_UPDATE, flag)
            return loss
        for i, table in enumerate(tables):                       # every gradient is tested before any parameter moves
            launch("a3d_stage_adam_f32", device, table, len(table), *consts, STAGE_ADAM_CHECK | (STAGE_ADAM_BEGIN if i == 0 else 0), flag)
        for table in tables:
            launch("a3d_stage_adam_f32", device, table, len(table), *consts, STAGE_ADAM_UPDATE, flag)
        return loss

    def load_state_dict(self, state_dict):
        """torch's layout, our own or ``torch.optim.Adam``'s: the values are copied into the tensors that exist (their addresses are in
        the kernel's tables), ``lr``, ``betas``, ``eps``, ``name`` and ``schedule`` are taken from the loaded groups."""
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups):
            raise ValueError(f"loaded state dict has {len(saved)} parameter groups, the optimiser has {len(self.param_groups)}")
        if any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        merged = [dict(g, **{k: s[k] for k in ("lr", "betas", "eps", "name", "schedule") + REFUSED_OPTIONS if k in s})
                  for s, g in zip(saved, self.param_groups)]
        for m in merged:
            m["betas"] = tuple(m["betas"])
        self._check_groups(merged)
        by_id = {i: p for s, g in zip(saved, self.param_groups) for i, p in zip(s["params"], g["params"])}
        loaded = state_dict["state"]
        for i, p in by_id.items():
            ours, theirs = self.state[p], loaded.get(i)
            for name in ("step", "exp_avg", "exp_avg_sq"):
                if theirs is None:
                    ours[name].zero_()
                else:
                    value = theirs[name]
                    ours[name].copy_(value if isinstance(value, torch.Tensor) else torch.tensor(float(value)))
        for g, m in zip(self.param_groups, merged):
            for k in ("lr", "betas", "eps", "name", "schedule"):
                if k in m:
                    g[k] = m[k]

