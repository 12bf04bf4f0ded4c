"""The replay of the batched MADDPG loop: a ring buffer of transitions in device memory (`DeviceReplay`)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops


class DeviceReplay:
    """Ring buffer of transitions in device memory (state / three next states as the eight observation
    tensors the networks take minus the topology-static A_n and mask, three agents' actions, rewards).

    storage="dense" (the default): every observation tensor is stored as it arrives; `add` / `sample` are indexing operations of the
    framework, one per tensor.
    storage="compact": the node-graph adjacencies A_s, A_n_ts, A_n_cs are stored as [capacity, N, Kn] through the truss's neighbour
    table `nbr` (int16 [N, Kn], TrussTopology.neighbor_table()) and the Pareto-graph adjacency A_p as [capacity, P, 3] through
    `nbr_p` (path_graph_table(P)); everything else as in dense storage.  `sample` still returns dense tensors, and the index draw is
    the same call on the same generator: a compact and a dense replay fed the same rows return the same batches.
    PRECONDITION (what makes compact storage lossless): every adjacency handed to `add` is exactly zero outside its table -- true of
    what the step / observation kernels and `pareto_graph` write (tests/test_replay_compact.py checks it on the emulator); entries
    outside the table would be dropped.
    On a cuda device with a native library that exports them, compact storage moves every field of a transition with ONE
    `replay_scatter` launch per `add` and ONE `replay_gather` launch per `sample` (csrc/truss_replay.h); on the cpu, or without the
    entries, the same semantics run as framework indexing (gather through the table on add, zeros + scatter on sample).
    fused=True does the same for dense storage (plain copies only); it needs the operators.
    `add(..., compact_in=True)` (compact storage only): the node-graph adjacencies of S / NS arrive in the compact observation layout
    already -- [.., N, Kn] rows of the same table, as the step / observation kernels write them with TRUSS_F_OBS_COMPACT -- and travel
    as plain fields, a row copy each; A_p is dense on the way in as ever.  The rings hold the same bits as after a dense-in add of
    the same transitions."""

    KEYS = ("x_n", "A_s", "A_n_ts", "A_n_cs", "x_p", "A_p")
    PATTERN_KEYS = ("A_s", "A_n_ts", "A_n_cs", "A_p")
    NODE_GRAPH_KEYS = ("A_s", "A_n_ts", "A_n_cs")             # what compact_in covers

    def __init__(self, capacity, N, P, device, storage="dense", nbr=None, nbr_p=None, lib=None, fused=False):
        if storage not in ("dense", "compact"):
            raise ValueError(f"storage must be 'dense' or 'compact', got {storage!r}")
        device = torch.device(device)
        f = lambda *s: torch.zeros((capacity,) + s, dtype=torch.float32, device=device)
        shapes = dict(x_n=(N, 13), A_s=(N, N), A_n_ts=(N, N), A_n_cs=(N, N), x_p=(P, 4), A_p=(P, P))
        self.storage, self.N, self.P = storage, N, P
        self._dense_shapes = dict(shapes)
        self._tab = {}                                        # key -> (table int16 [n, k], compact positions, dense positions)
        if storage == "compact":
            if nbr is None or nbr_p is None:
                raise ValueError("storage='compact' needs the neighbour tables nbr [N, Kn] and nbr_p [P, 3]")
            tn, tp = self._table(nbr, N, device), self._table(nbr_p, P, device)
            for k in self.PATTERN_KEYS:
                self._tab[k] = tp if k == "A_p" else tn
                shapes[k] = tuple(self._tab[k][0].shape)
        self.S = {k: f(*shapes[k]) for k in self.KEYS}
        self.NS = [{k: f(*shapes[k]) for k in self.KEYS} for _ in range(3)]
        self.a_geo, self.a_topo, self.R = f(3, N, 2), f(3, N, 3), f(3)
        self.capacity, self.size, self.head = capacity, 0, 0
        # the fused operators: compact storage takes them where they exist, fused dense storage demands them
        self._lib = None
        if device.type == "cuda" and (storage == "compact" or fused):
            lib = _lib.load() if lib is None else lib
            if lib.backend == "hip" and lib.has_replay_ops:
                self._lib = lib
        if fused and storage == "dense" and self._lib is None:
            raise _lib.TrussError("DeviceReplay(fused=True) needs a cuda device and a native library with truss_replay_scatter / truss_replay_gather")
        if self._lib is not None:
            # field lists in one fixed order: (ring tensor, key or None, table or None, row list of `rows`)
            self._fields = [(self.S[k], k, 0) for k in self.KEYS] + [(self.NS[a][k], k, 1 + a) for a in range(3) for k in self.KEYS]
            self._rings = [t for t, _, _ in self._fields] + [self.a_geo, self.a_topo, self.R]
            self._nbrs = [self._tab[k][0] if k in self._tab else None for _, k, _ in self._fields] + [None, None, None]
            # compact-in rows of the node-graph adjacencies are plain fields: no table for them
            self._nbrs_cin = [None if k in self.NODE_GRAPH_KEYS else n for (_, k, _), n in zip(self._fields, self._nbrs)] + [None, None, None]
            self._groups = [g for _, _, g in self._fields] + [0, 0, 0]

    @staticmethod
    def _table(t, n, device):
        t = torch.as_tensor(np.asarray(t.cpu() if torch.is_tensor(t) else t), dtype=torch.int16)
        if t.dim() != 2 or t.shape[0] != n:
            raise ValueError(f"a neighbour table must be [{n}, k], got {tuple(t.shape)}")
        k = t.shape[1]
        slot = torch.nonzero(t.flatten() >= 0).flatten()                       # positions in a compact row [n * k]
        cols = (slot // k) * n + t.flatten()[slot].long()                      # ... and where they sit in the dense row [n * n]
        return t.contiguous().to(device), slot.to(device), cols.to(device)

    @property
    def nbytes(self):
        """bytes held by the buffer's tensors"""
        ts = list(self.S.values()) + [t for ns in self.NS for t in ns.values()] + [self.a_geo, self.a_topo, self.R]
        return sum(t.numel() * t.element_size() for t in ts)

    def _put(self, ring, key, pos, rows, compact_in=False):
        """ring[pos] = rows (dense tensors [k, ...]); a pattern key of compact storage keeps the table's entries only -- unless the
        rows are compact already (compact_in, node-graph adjacencies): a plain row copy"""
        if key in self._tab and not (compact_in and key in self.NODE_GRAPH_KEYS):
            _, slot, cols = self._tab[key]
            ring.view(self.capacity, -1)[pos[:, None], slot[None, :]] = rows.reshape(rows.shape[0], -1)[:, cols]
        else:
            ring[pos] = rows

    def _get(self, ring, key, i):
        if key in self._tab:
            _, slot, cols = self._tab[key]
            out = torch.zeros((i.numel(),) + self._dense_shapes[key], dtype=ring.dtype, device=ring.device)
            out.view(i.numel(), -1)[:, cols] = ring.view(self.capacity, -1)[i[:, None], slot[None, :]]
            return out
        return ring[i]

    def add(self, sel, S, NS, a_geo, a_topo, R, src=None, compact_in=False):
        """append the transitions of the rows where sel[K] is True.  NS: three dicts (one per agent's next state), or -- with src
        [K, 3] -- ONE dict of tensors [3, K, ...] from which agent a's next state of row r is taken at [src[r, a], r].
        With the fused operators the sources are read in place, the accepted rows only, when they are float32 and strided over their
        first two dims at most (the [3, K, ...] tensors of the `src` form: contiguous); other layouts are copied whole first
        (`_rows_view`, and the `reshape` of a non-contiguous [3, K, ...] tensor).
        compact_in: A_s / A_n_ts / A_n_cs of S and NS are [.., N, Kn] rows of the table already (see the class)."""
        if compact_in:
            if self.storage != "compact":
                raise ValueError("compact_in needs storage='compact': a dense ring holds [N, N] adjacencies")
            for key in self.NODE_GRAPH_KEYS:
                want = tuple(self.S[key].shape[1:])
                for t in [S[key]] + ([NS[key]] if src is not None else [ns[key] for ns in NS]):
                    if tuple(t.shape[-2:]) != want:
                        raise ValueError(f"compact_in: {key} must end in {want}, got {tuple(t.shape)}")
        idx = torch.nonzero(sel, as_tuple=False).flatten()
        k = int(idx.numel())
        if k == 0:
            return 0
        if k > self.capacity:
            idx, k = idx[: self.capacity], self.capacity
        if self._lib is not None:
            self._add_fused(idx, k, S, NS, a_geo, a_topo, R, src, compact_in)
        else:
            pos = (self.head + torch.arange(k, device=idx.device)) % self.capacity
            pick = None if src is None else src[idx]                               # [k, 3]
            if self._tab:
                for key in self.KEYS:
                    self._put(self.S[key], key, pos, S[key][idx], compact_in)
                    for a in range(3):
                        self._put(self.NS[a][key], key, pos, NS[a][key][idx] if src is None else NS[key][pick[:, a], idx], compact_in)
            else:
                for key in self.KEYS:
                    self.S[key][pos] = S[key][idx]
                    for a in range(3):
                        self.NS[a][key][pos] = NS[a][key][idx] if src is None else NS[key][pick[:, a], idx]
            self.a_geo[pos], self.a_topo[pos], self.R[pos] = a_geo[idx], a_topo[idx], R[idx]
        self.head = (self.head + k) % self.capacity
        self.size = min(self.capacity, self.size + k)
        return k

    @staticmethod
    def _rows_view(t):
        """`t` [K, ...] as the operators read it in place, the accepted rows only: float32, strided over dims 0 and 1 at most (a
        permuted view of an agent-major tensor).  Anything else -- another dtype, a layout strided below dim 1 -- is first copied IN
        FULL, all K rows (`.float()` / `.contiguous()`): correct, but the caller then pays for the rows that are not accepted."""
        t = t if t.dtype == torch.float32 else t.float()
        inner = lambda d0: all(t.shape[d] == 1 or t.stride(d) == int(np.prod(t.shape[d + 1:])) for d in range(d0, t.dim()))
        return t if inner(1) or (t.dim() >= 2 and inner(2) and t.stride(1) >= 0 and t.stride(0) >= 0) else t.contiguous()

    def _add_fused(self, idx, k, S, NS, a_geo, a_topo, R, src, compact_in=False):
        K = S[self.KEYS[0]].shape[0]
        if src is None:
            rows = idx[None, :].expand(4, k).contiguous()
            nxt = lambda a, key: NS[a][key]
        else:
            # agent a's next state of row r = row src[r, a] * K + r of the candidate tensors [3, K, ...] seen as [3 K, ...]
            rows = torch.cat([idx[None, :], (src[idx].to(torch.int64) * K + idx[:, None]).t()], dim=0).contiguous()
            flat = {key: NS[key].reshape(3 * K, *NS[key].shape[2:]) for key in self.KEYS}
            nxt = lambda a, key: flat[key]
        srcs = [S[key] for key in self.KEYS] + [nxt(a, key) for a in range(3) for key in self.KEYS] + [a_geo, a_topo, R]
        srcs = [self._rows_view(t) for t in srcs]
        ops.call(ops.namespace().replay_scatter, ops.bind(self._lib), ops.stream_of(self.R.device), self._rings, srcs,
                 self._nbrs_cin if compact_in else self._nbrs, self._groups, rows, k, self.head, self.capacity)

    def sample(self, batch, generator=None):
        i = torch.randint(0, self.size, (batch,), device=self.R.device, generator=generator)
        if self._lib is not None:
            new = lambda *s: torch.empty((batch,) + s, dtype=torch.float32, device=self.R.device)
            outs = [new(*self._dense_shapes[k]) for _, k, _ in self._fields] + [new(*t.shape[1:]) for t in (self.a_geo, self.a_topo, self.R)]
            ops.call(ops.namespace().replay_gather, ops.bind(self._lib), ops.stream_of(self.R.device), self._rings, outs, self._nbrs, i, self.capacity)
            nk = len(self.KEYS)
            d = lambda j: dict(zip(self.KEYS, outs[j * nk:(j + 1) * nk]))
            return d(0), [d(1 + a) for a in range(3)], outs[-3], outs[-2], outs[-1]
        if self._tab:
            pick = lambda d: {k: self._get(v, k, i) for k, v in d.items()}
        else:
            pick = lambda d: {k: v[i] for k, v in d.items()}
        return pick(self.S), [pick(ns) for ns in self.NS], self.a_geo[i], self.a_topo[i], self.R[i]
