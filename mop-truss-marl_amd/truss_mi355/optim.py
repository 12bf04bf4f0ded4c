"""The optimiser steps of the MADDPG update as one native call each (`truss_optim_step`, csrc/truss_optim.h): the per-tensor
gradient clip and Adam -- the critics' shared Adam, or the first step of the fresh Adam of an actor update -- in two launches,
whatever the number of parameter tensors.  `optimizer_step(lib)` is the hook `truss2D_RL.set_optimizer_step` installs
(BatchedMARL(optimizer_path="hip")); the arithmetic is that of `truss2D_RL._clip_flat` + `SharedStepAdam.step` /
`_fresh_adam_step` with the sum of squares of the clip accumulated in float64.
"""
from __future__ import annotations

import torch

from . import _lib, ops


def n_chunks(sizes) -> int:
    """doubles of the scratch `truss_optim_step` needs for tensors of these sizes"""
    return sum((int(n) + _lib.OPTIM_CHUNK - 1) // _lib.OPTIM_CHUNK for n in sizes)


def optim_step(lib, params, grad, lr, eps, *, betas=(0.9, 0.999), step=None, exp_avg=None, exp_avg_sq=None, partials=None,
               clipped=None, norms=None):
    """One `truss_optim_step` over `params` (contiguous float32 tensors, updated in place) from the flat gradient `grad` (not
    modified): Adam at step number `step` (0-dim float64 tensor, already incremented) on the flat moments, or, with step None, the
    first step of a fresh Adam.  partials: float64 scratch of `n_chunks` elements (default: allocated here); clipped / norms: the
    optional outputs of the entry."""
    if partials is None:
        partials = torch.empty(max(1, n_chunks(p.numel() for p in params)), dtype=torch.float64, device=grad.device)
    mode = _lib.OPTIM_FIRST_STEP if step is None else _lib.OPTIM_ADAM
    ops.call(ops.namespace().optim_step, ops.bind(lib), ops.stream_of(grad.device), mode, list(params), grad, exp_avg, exp_avg_sq, step,
             float(lr), float(betas[0]), float(betas[1]), float(eps), partials, clipped, norms)


_hooks: dict = {}


def optimizer_step(lib):
    """The hook of `truss2D_RL.set_optimizer_step` for the library `lib` (which must have `truss_optim_step`): one per library, made
    at the first request.

    Per parameter list (the critics' 144 tensors, each actor's) it keeps what a call needs besides the caller's tensors: the list of
    the parameters' storages and the scratch for the partial sums, made at the list's first call -- an eager one: the engine warms
    the update up before it captures it -- and again only if a parameter's `data_ptr()` has changed.  The scratch therefore has a
    fixed address that a captured update may hold, and it is never freed (a few KB per list): the hook is installed process-wide,
    so the graph that holds the address need not belong to the engine that asked for the hook.  One scratch per list: the critics'
    step and the actors' steps follow each other on one stream, and so do the replays of a captured update."""
    if not lib.has_optim_step:
        raise _lib.TrussError(f"{lib.path} has no truss_optim_step")
    if lib.path in _hooks:
        return _hooks[lib.path]
    lists: dict = {}

    @torch.no_grad()
    def hook(params, flat_grad, lr, eps, betas=None, step=None, exp_avg=None, exp_avg_sq=None):
        key = tuple(p.data_ptr() for p in params)
        ent = lists.get(id(params[0]))         # a list is known by its first parameter
        if ent is None or ent[0] != key:
            data = [p.data for p in params]
            ent = (key, data, torch.empty(n_chunks(t.numel() for t in data), dtype=torch.float64, device=flat_grad.device), params[0])
            lists[id(params[0])] = ent
        _, data, partials, _ = ent
        optim_step(lib, data, flat_grad, lr, eps, betas=betas or (0.9, 0.999), step=step, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq,
                   partials=partials)

    _hooks[lib.path] = hook
    return hook
