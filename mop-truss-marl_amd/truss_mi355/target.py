"""The target update of the MADDPG update as one native call (`truss_target_update`, csrc/truss_target.h): every target tensor
follows its online tensor, t <- t + tau (p - t), every `period`-th update -- the gate is read on the device from the optimiser's
step counter, so a captured update fires on some replays and not on others.  One launch per 160 pairs: two for the 222 parameter
tensors of three actors and three critics.  `target_hook(lib)` is the hook `truss2D_RL.set_target_update` installs
(BatchedMARL(target_path="hip")); the arithmetic is that of `truss2D_RL._target_update_torch`.
"""
from __future__ import annotations

import torch

from . import _lib, ops


def target_update(lib, targets, sources, tau, period=1, step=None):
    """One `truss_target_update`: `targets` (contiguous float32 tensors, updated in place) follow `sources` (as many elements each,
    not modified) with lerp weight `tau` in (0, 1] where `step` (0-dim float64 device tensor; None: always) is a multiple of
    `period`; nothing is written otherwise."""
    device = targets[0].device if len(targets) else torch.device("cpu")
    ops.call(ops.namespace().target_update, ops.bind(lib), ops.stream_of(device), list(targets), list(sources), float(tau), int(period), step)


_hooks: dict = {}


def target_hook(lib):
    """The hook of `truss2D_RL.set_target_update` for the library `lib` (which must have `truss_target_update`): one per library,
    made at the first request.  It keeps nothing: the pair descriptors travel in the kernel arguments, so no device-side table
    needs a fixed address for a captured update to hold."""
    if not lib.has_target_update:
        raise _lib.TrussError(f"{lib.path} has no truss_target_update")
    if lib.path in _hooks:
        return _hooks[lib.path]

    @torch.no_grad()
    def hook(targets, sources, tau, period, step):
        target_update(lib, targets, sources, tau, period, step)

    _hooks[lib.path] = hook
    return hook
