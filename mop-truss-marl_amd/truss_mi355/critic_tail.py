"""The tail of a critic pass of the MADDPG update -- the 11 sum pools behind the second GCN level, their concatenation and the three
dense layers -- as native launches (`truss_critic_tail` / `truss_critic_tail_backward`, csrc/truss_critic_tail.h): one launch forward
for all the critics that reach their tail together, two backward (one where no parameter gradient is asked for).  `tail_hook(lib)`
is the hook `truss2D_RL.set_critic_tail` installs (BatchedMARL(critic_tail="hip")); `TorchTail` is the same contract in framework
operators (the arithmetic of `truss2D_RL._critic_steps`, and the reference of the tests).
"""
from __future__ import annotations

import torch

from . import _lib, ops


def critic_tail(lib, items, save):
    """One `truss_critic_tail` over `items` = [(outs, (w1, b1, w2, b2, w3, b3))] -> (qs, states): q [B, 1] per item and, where
    save[j], the (p, z1, z2) the backward reads (else None)."""
    dev = items[0][0][0].device
    o, counts, par, qs, states = [], [], [[] for _ in range(6)], [], []
    for (outs, params), keep in zip(items, save):
        outs = [t.contiguous() for t in outs]
        B, _, H = outs[0].shape
        Q = params[0].shape[0]
        o += outs
        counts.append(len(outs))
        for k in range(6):
            par[k].append(params[k].contiguous())
        qs.append(torch.empty((B, 1), dtype=torch.float32, device=dev))
        states.append((torch.empty((B, len(outs) * H), dtype=torch.float32, device=dev), torch.empty((B, Q), dtype=torch.float32, device=dev),
                       torch.empty((B, Q), dtype=torch.float32, device=dev)) if keep else None)
    pick = lambda k: [None if s is None else s[k] for s in states]
    ops.call(ops.namespace().critic_tail, ops.bind(lib), ops.stream_of(dev), o, counts, *par, qs, pick(0), pick(1), pick(2))
    return qs, states


def critic_tail_backward(lib, items, states, dqs, needs):
    """One `truss_critic_tail_backward`: needs[j] = (one bool per level output, one per parameter) -> [(d_outs, d_params)] with None
    where nothing was asked for.  An item that asks for parameter gradients gets its dz1 / dz2 scratch here."""
    dev = dqs[0].device
    new = lambda like: torch.empty(like.shape, dtype=torch.float32, device=dev)
    counts, nodes, d_o, res = [], [], [], []
    scratch, d_par = [[], []], [[] for _ in range(6)]
    for (outs, params), (need_o, need_p) in zip(items, needs):
        counts.append(len(outs))
        nodes.append(outs[0].shape[1])
        d_outs = [new(t) if n else None for t, n in zip(outs, need_o)]
        d_params = [new(t) if n else None for t, n in zip(params, need_p)]
        d_o += d_outs
        for k in range(6):
            d_par[k].append(d_params[k])
        B, Q = outs[0].shape[0], params[0].shape[0]
        for s in scratch:
            s.append(torch.empty((B, Q), dtype=torch.float32, device=dev) if any(need_p) else None)
        res.append((d_outs, d_params))
    par = lambda k: [params[k].contiguous() for _, params in items]
    ops.call(ops.namespace().critic_tail_backward, ops.bind(lib), ops.stream_of(dev), counts, nodes, list(dqs), [s[0] for s in states],
             [s[1] for s in states], [s[2] for s in states], par(0), par(2), par(4), [t if t.is_contiguous() else None for outs, _ in items for t in outs],
             d_o, scratch[0], scratch[1], *d_par)
    return res


class _HipTail:
    def __init__(self, lib):
        self.lib = lib

    @torch.no_grad()
    def forward(self, items, save):
        return critic_tail(self.lib, items, save)

    @torch.no_grad()
    def backward(self, items, states, dqs, needs):
        return critic_tail_backward(self.lib, items, states, dqs, needs)


class TorchTail:
    """the hook's contract in framework operators: the operations `truss2D_RL._critic_steps` runs without a hook, forward, and
    autograd's backward of the same graph"""

    @staticmethod
    def _q(outs, params):
        w1, b1, w2, b2, w3, b3 = params
        q = torch.stack(outs, dim=1).sum(dim=2).flatten(1)
        q = torch.relu(torch.nn.functional.linear(q, w1, b1))
        q = torch.relu(torch.nn.functional.linear(q, w2, b2))
        return torch.nn.functional.linear(q, w3, b3)

    @torch.no_grad()
    def forward(self, items, save):
        return [self._q(outs, params) for outs, params in items], [True if keep else None for keep in save]

    def backward(self, items, states, dqs, needs):
        res = []
        for (outs, params), dq, (need_o, need_p) in zip(items, dqs, needs):
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(n) for t, n in zip(list(outs) + list(params), list(need_o) + list(need_p))]
                q = self._q(leaves[:len(outs)], leaves[len(outs):])
                wanted = [t for t in leaves if t.requires_grad]
                got = iter(torch.autograd.grad(q, wanted, dq))
            grads = [next(got) if t.requires_grad else None for t in leaves]
            res.append((grads[:len(outs)], grads[len(outs):]))
        return res


_hooks: dict = {}


def tail_hook(lib):
    """The hook of `truss2D_RL.set_critic_tail` for the library `lib` (which must have `truss_critic_tail`): one per library, made at
    the first request.  It allocates its outputs through the framework's caching allocator, like the level kernels' glue, so a
    captured update holds them in the graph's pool."""
    if not lib.has_critic_tail:
        raise _lib.TrussError(f"{lib.path} has no truss_critic_tail")
    if lib.path not in _hooks:
        _hooks[lib.path] = _HipTail(lib)
    return _hooks[lib.path]
