"""The Pareto-graph inputs of the networks and the set-up of a chunk of (env, member) pairs of a game step: as framework
operators (`pareto_graph`, `design_coins`) and as one `truss_pair_setup` launch that writes the same bits (`pair_setup` with the
tables `pair_dtab` / `pair_frac_tab`).  `path_graph_table` is the sparsity pattern of the Pareto graph's adjacency."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops


def pareto_graph(pts, n, index, max_front):
    """Batched truss2D_ENV.pareto_state_data (:19-38) + zero padding to P nodes (master…:488-593).
    pts [B,P,4] (rows beyond n ignored), n [B], index [B] -> x_p [B,P,4], A_p [B,P,P] float32."""
    B, P, _ = pts.shape
    dev = pts.device
    ar = torch.arange(P, device=dev)
    vf = (ar[None, :] < n[:, None]).float()                                             # [B, P] 1 on the front's members
    x = torch.stack([pts[:, :, 0].float(), pts[:, :, 1].float(), (ar[None, :] == index[:, None]).float(),
                     (n.float() / max_front)[:, None].expand(B, P)], dim=2) * vf[:, :, None]
    # a path over the members with self loops, symmetrically normalised: deg_i = 1 + (left neighbour) + (right neighbour) on members
    z = torch.zeros((B, 1), dtype=torch.float32, device=dev)
    deg = vf * (1.0 + torch.cat([z, vf[:, :-1]], dim=1) + torch.cat([vf[:, 1:], z], dim=1))
    d = torch.where(deg > 0, deg.pow(-0.5), 0.0)
    return x, _tridiagonal(P, dev) * d[:, :, None] * d[:, None, :]


_TRI: dict = {}


def _tridiagonal(P, dev):
    """[P, P] ones on the three central diagonals (the path graph with self loops), cached per size and device"""
    key = (P, str(dev))
    if key not in _TRI:
        i = torch.arange(P, device=dev)
        _TRI[key] = ((i[:, None] - i[None, :]).abs() <= 1).float()
    return _TRI[key]


def path_graph_table(n_nodes):
    """int16 [P, 3] neighbour table of the Pareto graph: `pareto_graph` / truss2D_ENV.pareto_state_data build a PATH over the front's
    members (self loops + consecutive members), so row i of A_p is zero outside columns i - 1, i, i + 1"""
    t = np.full((n_nodes, 3), -1, np.int16)
    for i in range(n_nodes):
        t[i, 0] = i - 1 if i > 0 else -1
        t[i, 1] = i
        t[i, 2] = i + 1 if i + 1 < n_nodes else -1
    return t


_SM64 = (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)


def _splitmix64(z):
    """splitmix64 finaliser on int64 tensors (two's complement wrap-around == uint64 arithmetic; logical shifts by mask)"""
    s64 = lambda c: c - (1 << 64) if c >= 1 << 63 else c
    srl = lambda v, k: (v >> k) & ((1 << (64 - k)) - 1)
    z = z + s64(_SM64[0])
    z = (z ^ srl(z, 30)) * s64(_SM64[1])
    z = (z ^ srl(z, 27)) * s64(_SM64[2])
    return z ^ srl(z, 31)


def design_coins(seed, env_ids, game_step, members):
    """D6: the symmetry coin of every move of the design game, uint8 [K, 3] (agent a in column a) for the pairs (env_ids[k],
    members[k]) of game step `game_step`: the top bit of splitmix64(splitmix64(seed) ^ (env << 26 | step << 10 | member << 2 | agent))
    (env < 2^38, step < 2^16, member < 256).  A pure function of those fields: the same on any device, for any pair order."""
    dev = env_ids.device
    key = (env_ids.to(torch.int64)[:, None] << 26) | (int(game_step) << 10) | (members.to(torch.int64)[:, None] << 2) \
        | torch.arange(3, dtype=torch.int64, device=dev)[None, :]
    h0 = _splitmix64(torch.tensor(int(seed), dtype=torch.int64, device=dev))
    return (_splitmix64(key ^ h0) < 0).to(torch.uint8)


def pair_dtab(device):
    """[0, 1^-1/2, 2^-1/2, 3^-1/2] as float32 values the way the framework rounds them on `device` (what `pareto_graph` gets from
    `deg.pow(-0.5)` there): the table `pair_setup` takes, so that its A_p carries the bits of `pareto_graph`.  Synchronises once."""
    return [0.0] + torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device=device).pow(-0.5).tolist()


def pair_frac_tab(max_front, device):
    """float32 [P + 1]: column 3 of the Pareto-graph features for n = 0..P as `pareto_graph` computes it on `device` (`n.float() /
    max_front`: on a GPU the framework multiplies by the rounded reciprocal of a host scalar, which is not always the correctly
    rounded quotient -- 49 / 50 comes out one ulp lower): the table `pair_setup` takes so that its x_p carries those bits."""
    return torch.arange(max_front + 1, dtype=torch.int32, device=device).float() / max_front


_PAIR_ROWS = (("x", "c_x"), ("target", "c_target"), ("params", "c_params"), ("y", "arch_y"), ("sec", "arch_sec"))


def pair_setup(lib, idx, ms, pts, n, arch_y, arch_sec, c_x, c_target, c_params, ref_points, *, rep=3, dtab=None, frac_tab=None,
               coins=None, par=None, cand=None, out=None, stream=None):
    """The set-up of K (env, member) pairs of a game step as one `truss_pair_setup` launch (include/truss_mi355.h, csrc/truss_pairs.h).

    idx, ms [K] int64 (pair k = env idx[k], member ms[k]; envs may repeat)
    pts [B,P,4] float64, n [B] int32, arch_y [B,P,N] float32, arch_sec [B,P,E] int32          the step-start archive
    c_x, c_target [B,N] float32, c_params [B,NPARAM] float64, ref_points [B,2] float64        per-env constants
    rep     1 or 3: copies of the Pareto graph (3: the candidates' next states, agent-major)
    dtab    the four float32 values [0, 1, 2, 3]^-1/2 (default: `pair_dtab(device)`, which synchronises -- callers in a loop keep it)
    frac_tab  None: column 3 of x_p is float(n) / float(P), one float32 division; or float32 [P + 1] with the value for every n
              (`pair_frac_tab(P, device)`: what the framework computes there)
    coins   None, or (seed, env_ids [B] int64, game_step): also the design game's coins (`design_coins`, agent-major)
    par / cand   dicts x, target, params, y, sec of tensors with at least K / 3 K rows to write the design rows into (the env
                 objects' resident buffers; rows behind stay as they are); None: new tensors
    out     dict of preallocated p0, nn0, parent_obj, ref, x_p, A_p, coin to write into instead of new tensors
    Returns dict(par, cand (the dicts), p0 [K,P,4], nn0 [K] int32, parent_obj [K,2], ref [K,2], x_p [rep K,P,4], A_p [rep K,P,P],
    coin [3 K] uint8 or None).  No output may overlap an input."""
    lib = lib or _lib.load()
    if not lib.has_pair_setup:
        raise _lib.TrussError(f"{lib.path} has no truss_pair_setup (the fused set-up of a chunk of pairs)")
    if rep not in (1, 3):
        raise ValueError(f"rep must be 1 or 3, got {rep!r}")
    K, (B, P), dev = int(idx.shape[0]), pts.shape[:2], pts.device
    src = dict(c_x=c_x, c_target=c_target, c_params=c_params, arch_y=arch_y, arch_sec=arch_sec)
    rows = lambda given, mult: {k: (given[k] if given is not None else torch.empty((mult * K, src[s].shape[-1]), dtype=src[s].dtype, device=dev))
                                for k, s in _PAIR_ROWS}
    par, cand = rows(par, 1), rows(cand, 3)
    out = dict(out or {})
    new = lambda key, shape, dt: out[key] if key in out else torch.empty(shape, dtype=dt, device=dev)
    res = dict(par=par, cand=cand, p0=new("p0", (K, P, 4), torch.float64), nn0=new("nn0", (K,), torch.int32),
               parent_obj=new("parent_obj", (K, 2), torch.float64), ref=new("ref", (K, 2), torch.float64),
               x_p=new("x_p", (rep * K, P, 4), torch.float32), A_p=new("A_p", (rep * K, P, P), torch.float32),
               coin=new("coin", (3 * K,), torch.uint8) if coins is not None else None)
    seed, env_ids, game_step = coins if coins is not None else (0, None, 0)
    stream_i = ops.stream_of(dev) if stream is None else int(getattr(stream, "value", stream) or 0)
    ops.call(ops.namespace().pair_setup, ops.bind(lib), stream_i, int(rep), int(seed), int(game_step), list(dtab) if dtab is not None else pair_dtab(dev),
             idx, ms, pts, n, arch_y, arch_sec, c_x, c_target, c_params, ref_points, env_ids, frac_tab,
             par["x"], par["target"], par["params"], par["y"], par["sec"], cand["x"], cand["target"], cand["params"], cand["y"], cand["sec"],
             res["p0"], res["nn0"], res["parent_obj"], res["ref"], res["x_p"], res["A_p"], res["coin"])
    return res
