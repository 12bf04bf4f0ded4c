"""The MADDPG update above 64 nodes: neighbour sums through the node table.

  truss_gcn_level_aggregate      the kernel and its operator against float64, element by element:
                                   |y - y64| <= gamma_k (|A| |x|)_pattern + 2^-126,  gamma_k = k u / (1 - k u), u = 2^-24, k = k_nbr
                                 -- the bound of a k-term fmaf chain, nothing measured in it -- with host mutants that must leave it
  truss2D_RL.NodePattern         validation of the host table
  truss2D_RL.node_pattern        `gcn_level` with a pattern current against the same call without one (CPU, float64: 1e-10; GPU,
                                 float32 with the hook of `gcn.level_aggregate`: the caps of tests/test_update_float64.py)
  the update                     three updates with the pattern on against tests/update_reference.Update64, as
                                 tests/test_update_float64.py holds the library path
  BatchedMARL / MixedMARL        level_adjacency="table" against "dense"

Tables: TrussTopology.grid(33) (66 nodes, k = 6), grid(150) (300 nodes: beyond any tile), and a synthetic symmetric table of 130
nodes with k = 16 whose rows hold 1 to 16 entries in shuffled order with the -1 slots between them."""
import contextlib
import copy
import ctypes
import io
import types

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import gcn, marl, ops, pool, synthetic
import parity_common as pc
import gcn_reference as GR
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL
import update_reference as UR
import test_update_float64 as T

U = 2.0 ** -24


# ---- tables and adjacencies -----------------------------------------------------------------------------------------------------------

def grid_table(nx=33):
    return tm.TrussTopology.grid(nx).neighbor_table()


def synthetic_table(N=130, k=16, seed=3):
    """symmetric, rows of 1 (node 0: itself) to 16 (node 1) entries, every row's entries in random order on random slots"""
    rng = np.random.default_rng(seed)
    nb = [{i} for i in range(N)]

    def link(a, b):
        nb[a].add(b)
        nb[b].add(a)

    for j in range(2, k + 1):
        link(1, j)
    for _ in range(6 * N):
        a, b = (int(v) for v in rng.integers(2, N, 2))
        if a != b and b not in nb[a] and len(nb[a]) < k and len(nb[b]) < k:
            link(a, b)
    tab = np.full((N, k), -1, np.int16)
    for i, s in enumerate(nb):
        slots = np.sort(rng.choice(k, len(s), replace=False))
        tab[i, slots] = rng.permutation(sorted(s))
    counts = (tab >= 0).sum(1)
    assert counts.min() == 1 and counts.max() == k
    inner = [(row >= 0).nonzero()[0] for row in tab]
    assert any(len(p) < k and len(p) and p[-1] - p[0] + 1 > len(p) for p in inner)        # -1 slots BETWEEN entries of short rows
    return tab


def pattern_mask(table):
    N = table.shape[0]
    m = np.zeros((N, N), bool)
    r, c = np.nonzero(table >= 0)
    m[r, table[r, c]] = True
    return m


def pattern_adj(table, B, gen, dtype=torch.float32):
    """[B, N, N] (B None: [N, N]): random on the pattern -- negative values, and exact zeros inside it -- exactly zero outside"""
    N = table.shape[0]
    shape = (N, N) if B is None else (B, N, N)
    a = torch.randn(shape, generator=gen, dtype=torch.float64)
    a = torch.where(torch.rand(shape, generator=gen) < 0.1, torch.zeros((), dtype=torch.float64), a)
    return (a * torch.from_numpy(pattern_mask(table))).to(dtype)


def table_softmax_adj(table, B, gen):
    """a row-stochastic adjacency as the update's batches carry it (tests/test_update_float64._batch), zero outside the table"""
    N = table.shape[0]
    z = torch.randn(B, N, N, generator=gen)
    z = z.masked_fill(~torch.from_numpy(pattern_mask(table)), float("-inf"))
    return torch.softmax(z, -1)


# ---- NodePattern ----------------------------------------------------------------------------------------------------------------------

def test_node_pattern_refuses_bad_tables():
    good = grid_table()
    asym = good.copy()
    i = int(np.argmax((asym >= 0).sum(1) < asym.shape[1]))         # a row with a free slot: list a far node that does not list it back
    far = next(j for j in range(asym.shape[0]) if j not in asym[i] and i not in asym[j])
    asym[i, (asym[i] < 0).nonzero()[0][0]] = far
    dup = good.copy()
    dup[0, 1] = dup[0, 0]
    high = good.copy()
    high[0, 0] = good.shape[0]
    low = good.copy()
    low[0, -1] = -2
    wide = np.full((20, 17), -1, np.int16)
    wide[:, 0] = np.arange(20)
    for bad in (asym, dup, high, low, wide, good.astype(np.int32), good[:, :0]):
        with pytest.raises(ValueError):
            RL.NodePattern(bad)
    with pytest.raises(ValueError):
        RL.NodePattern(torch.from_numpy(asym))


def test_node_pattern_accepts_the_grid_and_the_synthetic_table():
    g = RL.NodePattern(grid_table())
    assert (g.n_nodes, g.k) == (66, 6) and g.table.dtype == torch.int16
    s = RL.NodePattern(torch.from_numpy(synthetic_table()))
    assert (s.n_nodes, s.k) == (130, 16)
    assert s.to("cpu") is s and torch.equal(s.on("cpu"), torch.from_numpy(synthetic_table())) and s.on("cpu") is s.on("cpu")


def _one_group(pattern, adj, B, K):
    return RL._Group([0], None, None, [adj], (B, pattern.n_nodes, K), None, pattern)


@pytest.mark.parametrize("which", ["grid", "synthetic"])
def test_torch_fallback_equals_the_dense_products(which):
    table = grid_table() if which == "grid" else synthetic_table()
    p, N, B, K = RL.NodePattern(table), table.shape[0], 3, 5
    gen = torch.Generator().manual_seed(7)
    for adj in (pattern_adj(table, B, gen, torch.float64), pattern_adj(table, None, gen, torch.float64)[None]):
        assert bool((adj == 0).logical_and(torch.from_numpy(pattern_mask(table))).any()) and bool((adj < 0).any())
        x = torch.randn(B, N, K, generator=gen, dtype=torch.float64)
        for transpose in (False, True):
            (y,) = RL._aggregate_library([_one_group(p, adj, B, K)], [[x]], transpose)
            want = torch.matmul(adj.transpose(1, 2) if transpose else adj, x)
            assert y.shape == (1, B * N, K)
            assert float((y.view(B, N, K) - want).abs().max()) <= 1e-12


# ---- gcn_level with a pattern ----------------------------------------------------------------------------------------------------------

def _layer(C, K, gen, dtype, device):
    w = (torch.randn(C, K, generator=gen, dtype=torch.float64) / K ** 0.5).to(dtype).to(device).requires_grad_()
    b = (0.1 * torch.randn(C, generator=gen, dtype=torch.float64)).to(dtype).to(device).requires_grad_()
    return types.SimpleNamespace(lin=types.SimpleNamespace(weight=w, out_features=C), bias=b)


def make_mix(table, seed, dtype=torch.float64, device="cpu", B=3, H=24):
    """one level: three node-graph layers (K = 13, 3, 24; relu, sigmoid, none; one shared and two per-sample adjacencies, zero outside
    the table) and a 6-node front layer.  Returns (reqs, coefficients of the scalar the gradients are taken of)."""
    N, gen = table.shape[0], torch.Generator().manual_seed(seed)
    leaf = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype).to(device).requires_grad_()
    shared = table_softmax_adj(table, 1, gen).to(dtype).to(device).expand(B, -1, -1)
    a1, a2 = (pattern_adj(table, B, gen, dtype).to(device) * 0.5 for _ in range(2))
    a_p = torch.softmax(torch.randn(B, 6, 6, generator=gen), -1).to(dtype).to(device)
    reqs = [(_layer(H, 13, gen, dtype, device), leaf(B, N, 13), shared, "relu"),
            (_layer(5, 3, gen, dtype, device), leaf(B, N, 3), a1, "sigmoid"),
            (_layer(H, 24, gen, dtype, device), leaf(B, N, 24), a2, None),
            (_layer(H, 4, gen, dtype, device), leaf(B, 6, 4), a_p, "relu")]
    coef = [torch.randn(B, r[1].shape[1], r[0].lin.out_features, generator=gen, dtype=torch.float64).to(dtype).to(device) for r in reqs]
    return reqs, coef


def level_and_grads(reqs, coef, pattern):
    wrt = [t for layer, x, _, _ in reqs for t in (x, layer.lin.weight, layer.bias)]
    with RL.node_pattern(pattern):
        outs = RL.gcn_level(reqs, {})
        grads = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, coef)), wrt)
    return [o.detach() for o in outs], list(grads)


def relu_margin(reqs):
    """the smallest |pre-activation| of the relu layers, in float64"""
    worst = float("inf")
    for layer, x, adj, act in reqs:
        if act == "relu":
            pre = GR.f64(adj) @ (GR.f64(x) @ GR.f64(layer.lin.weight).T) + GR.f64(layer.bias)
            worst = min(worst, float(np.abs(pre).min()))
    return worst


MIX_SEED = {66: 14, 130: 16}          # smallest |relu pre-activation| in float64: 1.0e-4, 1.1e-4 (seeds 11 .. 16 give 2e-6 .. 1.1e-4)


def test_gcn_level_with_a_pattern_matches_the_dense_level_in_float64():
    table = grid_table()
    reqs, coef = make_mix(table, MIX_SEED[66])
    assert relu_margin(reqs) > 1e-6
    o_d, g_d = level_and_grads(reqs, coef, None)
    o_t, g_t = level_and_grads(reqs, coef, RL.NodePattern(table))
    assert len(g_d) == 12
    for a, b in zip(o_d + g_d, o_t + g_t):
        assert a.shape == b.shape and float(a.abs().max()) > 0
        assert float((a - b).abs().max()) <= 1e-10


def test_a_pattern_group_never_stacks_its_adjacencies(monkeypatch):
    table = grid_table()
    reqs, coef = make_mix(table, MIX_SEED[66])
    calls, real = [], RL._adj_stack
    monkeypatch.setattr(RL, "_adj_stack", lambda adjs, B, N, cache=None: calls.append(N) or real(adjs, B, N, cache))
    level_and_grads(reqs, coef, RL.NodePattern(table))
    assert calls == [6]                                              # the front's group, once; none of the three 66-node groups
    del calls[:]
    level_and_grads(reqs, coef, None)
    assert sorted(calls) == [6, 66, 66, 66]                          # without a pattern: every group, once (forward; the backward re-uses it)


def test_without_a_pattern_nothing_changes(monkeypatch):
    """no context, node_pattern(None), and a current pattern that does not apply (a 66-node table over 12-node graphs; a 12-node
    table: N <= 64) make the same calls in the same order and return the same bits"""
    small = tm.TrussTopology.grid(6).neighbor_table()
    assert small.shape[0] == 12
    reqs, coef = make_mix(small, 5, dtype=torch.float32)
    wrt = [t for layer, x, _, _ in reqs for t in (x, layer.lin.weight, layer.bias)]
    log, real = [], RL._adj_stack
    monkeypatch.setattr(RL, "_adj_stack", lambda adjs, B, N, cache=None: log.append(("stack", B, N, len(adjs))) or real(adjs, B, N, cache))

    def fwd(groups, xs, ws, bs, want_grad):
        log.append(("forward", [tuple(g.idx) for g in groups], want_grad))

    def bwd(groups, douts, outs, xaggs, ws, need):
        log.append(("backward", [tuple(g.idx) for g in groups], [d is not None for d in douts], len(outs), len(xaggs)))

    def agg(groups, xs, transpose):
        log.append(("aggregate",))

    def run():
        del log[:]
        outs = RL.gcn_level(reqs, {})
        grads = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, coef)), wrt)
        return [o.detach() for o in outs] + list(grads), list(log)

    RL.set_level_forward(fwd, "cpu"), RL.set_level_backward(bwd, "cpu"), RL.set_level_aggregate(agg, "cpu")
    try:
        plain, calls = run()
        with RL.node_pattern(None):
            none, calls_none = run()
        with RL.node_pattern(RL.NodePattern(grid_table())):
            other, calls_other = run()
        with RL.node_pattern(RL.NodePattern(small)):
            below, calls_below = run()
    finally:
        RL.set_level_forward(None, "cpu"), RL.set_level_backward(None, "cpu"), RL.set_level_aggregate(None, "cpu")
    assert "cpu" not in RL._LEVEL_AGGREGATE
    assert [c[0] for c in calls] == ["forward"] + ["stack"] * 4 + ["backward"] and calls[0][1] == [(0,), (1,), (2,), (3,)]
    assert calls == calls_none == calls_other == calls_below
    for a, b, c, d in zip(plain, none, other, below):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


# ---- the operator, the engine switch (no GPU) -----------------------------------------------------------------------------------------

def test_operator_is_registered_and_the_emulator_declines_cleanly():
    ns = ops.namespace()
    schema = str(ns.gcn_level_aggregate.default._schema)
    assert schema == ("truss_mi355::gcn_level_aggregate(int lib, int stream, Tensor[] x, Tensor[] adj, Tensor[] nbr, Tensor(a!)[] y, "
                      "bool[] transpose) -> ()")
    for key in ("CPU", "CUDA", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("truss_mi355::gcn_level_aggregate", key)
    m = lambda *s, **kw: torch.empty(*s, device="meta", **kw)
    assert ns.gcn_level_aggregate(0, 0, [m(2, 4, 3)], [m(4, 4)], [m(4, 2, dtype=torch.int16)], [m(2, 4, 3)], [False]) is None
    assert "truss_gcn_level_aggregate" in ops.entries()
    emu = tm.load(pc.build_emu())
    assert emu.backend == "emu" and not emu.has_level_aggregate and not hasattr(emu.dll, "truss_gcn_level_aggregate")
    y = torch.full((2, 4, 3), float("nan"))
    nbr = torch.tensor([[0, 1], [1, 0], [2, 3], [3, 2]], dtype=torch.int16)
    with pytest.raises(tm.TrussError, match="no truss_gcn_level_aggregate"):
        ops.call(ns.gcn_level_aggregate, ops.bind(emu), 0, [torch.rand(2, 4, 3)], [torch.rand(4, 4)], [nbr], [y], [True])
    assert bool(torch.isnan(y).all())
    assert gcn.level_aggregate(emu) is not None and marl.level_aggregate is gcn.level_aggregate      # (building the hook binds nothing yet)


def test_engine_switch_and_environment(monkeypatch):
    """BatchedMARL(level_adjacency=...): "dense" by default, TRUSS_LEVEL_ADJACENCY=table selects "table" where the argument is not
    given, anything else is refused -- and so is "table" on a library without the entry; with it, the engine owns the pattern of its
    truss; on the CPU backend no hook is installed either way"""
    topo = tm.TrussTopology.grid(4)
    lib = pc.emu_lib()
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 8, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    mk = lambda **kw: marl.BatchedMARL(topo, 2, rl, max_front=6, lib=lib, device="cpu", replay_capacity=8, batch_size=2, **kw)
    monkeypatch.delenv("TRUSS_LEVEL_ADJACENCY", raising=False)
    assert mk().level_adjacency == "dense" and mk().pattern is None
    with pytest.raises(ValueError, match="truss_gcn_level_aggregate"):
        mk(level_adjacency="table")
    monkeypatch.setenv("TRUSS_LEVEL_ADJACENCY", "table")
    with pytest.raises(ValueError, match="truss_gcn_level_aggregate"):
        mk()
    assert mk(level_adjacency="dense").level_adjacency == "dense"
    monkeypatch.setattr(lib, "has_level_aggregate", True)           # a library with the entry
    eng = mk()
    assert eng.level_adjacency == "table" and isinstance(eng.pattern, RL.NodePattern) and eng.pattern.n_nodes == topo.N
    assert torch.equal(eng.pattern.on("cpu"), torch.from_numpy(topo.neighbor_table()))
    monkeypatch.setenv("TRUSS_LEVEL_ADJACENCY", "1")
    assert mk().level_adjacency == "dense" and mk(level_adjacency="table").level_adjacency == "table"
    with pytest.raises(ValueError):
        mk(level_adjacency="sparse")
    assert "cpu" not in RL._LEVEL_AGGREGATE


# ---- the kernel on the GPU -----------------------------------------------------------------------------------------------------------

def make_items(seed=1):
    """the items of the issue, (B, N, n_ch, table, shared adjacency), and one whose x is a view offset by one float; CPU tensors"""
    gen = torch.Generator().manual_seed(seed)
    tabs = {"grid": grid_table(), "synthetic": synthetic_table(), "grid150": grid_table(150)}
    assert tabs["grid150"].shape[0] == 300
    spec = [(3, 66, 200, "grid", False), (3, 66, 13, "grid", True), (2, 66, 2, "grid", False), (2, 66, 3, "grid", False),
            (3, 130, 16, "synthetic", False), (1, 130, 204, "synthetic", True), (2, 300, 8, "grid150", False), (0, 66, 8, "grid", False),
            (2, 66, 8, "grid", False)]
    items = []
    for n, (B, N, C, tab, shared) in enumerate(spec):
        table = tabs[tab]
        assert table.shape[0] == N
        adj = pattern_adj(table, None if shared else B, gen)
        if n == len(spec) - 1:
            x = torch.randn(B * N * C + 1, generator=gen)[1:].view(B, N, C)            # 4 bytes off a 16-byte boundary
        else:
            x = torch.randn(B, N, C, generator=gen)
        items.append(dict(x=x, adj=adj, table=table, offset=n == len(spec) - 1))
    return items


def to_gpu(items):
    out = []
    for it in items:
        x = it["x"]
        if it["offset"]:
            x = torch.cat([torch.zeros(1), x.reshape(-1)]).cuda()[1:].view(x.shape)
            assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        else:
            x = x.cuda()
        out.append(dict(x=x, adj=it["adj"].cuda(), nbr=torch.from_numpy(it["table"]).cuda()))
    return out


def run_op(lib, dev, transpose, sentinel=float("nan")):
    ys = [torch.full_like(d["x"], sentinel) for d in dev]
    ops.call(ops.namespace().gcn_level_aggregate, ops.bind(lib), ops.stream_of(dev[0]["x"].device), [d["x"] for d in dev],
             [d["adj"] for d in dev], [d["nbr"] for d in dev], ys, [transpose] * len(dev))
    return ys


def agg64(it, transpose, mutant=None):
    """float64 sum over the table's entries and its magnitude (|A| |x|)_pattern; mutants: see the test"""
    x, table = GR.f64(it["x"]), it["table"]
    B, N, C = x.shape
    A = GR.dense_adj(it["adj"], B, N)
    if mutant == "graph 0's adjacency for every graph":
        A = np.broadcast_to(A[:1], A.shape) if B else A
    if (transpose and mutant != "A instead of A^T") or (not transpose and mutant == "A instead of A^T"):
        A = A.transpose(0, 2, 1)
    t = table[:, :-1] if mutant == "last table column dropped" else table
    ref, mag = np.zeros((B, N, C)), np.zeros((B, N, C))
    rows = np.arange(N)
    for s in range(t.shape[1]):
        j = t[:, s].astype(np.int64)
        ok = j >= 0
        if mutant == "-1 read as node N - 1":
            j, ok = np.where(ok, j, N - 1), np.ones(N, bool)
        jc = np.where(ok, j, 0)
        coef = np.where(ok[None, :], A[:, rows, jc], 0.0)                               # [B, N]
        ref += coef[:, :, None] * x[:, jc]
        mag += np.abs(coef)[:, :, None] * np.abs(x[:, jc])
    return ref, mag


def bound(it, mag):
    k = it["table"].shape[1]
    return k * U / (1.0 - k * U) * mag + 2.0 ** -126


MUTANTS = ("A instead of A^T", "last table column dropped", "-1 read as node N - 1", "graph 0's adjacency for every graph")


@pytest.mark.gpu
def test_operator_matches_float64_and_the_bound_rejects_mutants():
    """all items in ONE call per direction; every element within the bound of a k-term fmaf chain; a second call gives the same
    bits; each mutant of the host reference falls outside the bound on at least one item.
    Measured on an MI355X: largest error / bound 0.46 (A x) and 0.455 (A^T x) over the nine items."""
    lib = tm.load()
    assert lib.has_level_aggregate
    items = make_items()
    dev = to_gpu(items)
    for transpose in (False, True):
        ys = run_op(lib, dev, transpose)
        again = run_op(lib, dev, transpose, sentinel=7.0)
        torch.cuda.synchronize()
        worst = 0.0
        for it, y, y2 in zip(items, ys, again):
            assert torch.equal(y, y2)
            ref, mag = agg64(it, transpose)
            err, lim = np.abs(GR.f64(y) - ref), bound(it, mag)
            assert y.shape == it["x"].shape and bool(np.all(err <= lim)), (tuple(y.shape), transpose, float((err / lim).max()))
            worst = max(worst, float((err / lim).max()) if err.size else 0.0)
        print(f"\n[level aggregate, transpose={transpose}] largest error / bound over {len(items)} items: {worst:.3g}")
        for mutant in MUTANTS:
            outside = 0
            for it, y in zip(items, ys):
                ref, _ = agg64(it, transpose, mutant)
                _, mag = agg64(it, transpose)
                outside += int(np.any(np.abs(GR.f64(y) - ref) > bound(it, mag)))
            assert outside >= 1, f"mutant '{mutant}' (transpose={transpose}) stays within the bound on every item"


@pytest.mark.gpu
def test_25_items_in_one_call_equal_one_by_one():
    lib = tm.load()
    table = grid_table()
    gen = torch.Generator().manual_seed(3)
    mk = lambda n: dict(x=torch.randn(2, 66, 4 + 4 * (n % 3), generator=gen).cuda(), adj=pattern_adj(table, 2, gen).cuda(),
                        nbr=torch.from_numpy(table).cuda())
    dev = [mk(n) for n in range(25)]
    for transpose in (False, True):
        together = run_op(lib, dev, transpose)
        singly = [run_op(lib, [d], transpose)[0] for d in dev]
        for a, b in zip(together, singly):
            assert torch.equal(a, b) and not bool(torch.isnan(a).any())


@pytest.mark.gpu
def test_captured_call_replays_like_eager():
    lib = tm.load()
    items = make_items(2)[:4]
    dev = to_gpu(items)
    ys = [torch.zeros_like(d["x"]) for d in dev]
    args = lambda: (ops.bind(lib), ops.stream_of(dev[0]["x"].device), [d["x"] for d in dev], [d["adj"] for d in dev], [d["nbr"] for d in dev],
                    ys, [True, False, True, False])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.call(ops.namespace().gcn_level_aggregate, *args())                          # (warm-up: the kernel is loaded before capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        ops.call(ops.namespace().gcn_level_aggregate, *args())
    gen = torch.Generator().manual_seed(9)
    for d in dev:                                                                       # fresh inputs, in place
        d["x"].copy_(torch.randn(d["x"].shape, generator=gen))
        d["adj"].mul_(-1.5)
    for y in ys:
        y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    replayed = [y.clone() for y in ys]
    ops.call(ops.namespace().gcn_level_aggregate, *args())
    torch.cuda.synchronize()
    for a, b in zip(replayed, ys):
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())


class _Agg(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("x", ctypes.c_void_p), ("adj", ctypes.c_void_p), ("a_batch_stride", ctypes.c_int64),
                ("nbr", ctypes.c_void_p), ("y", ctypes.c_void_p), ("n_batch", ctypes.c_int32), ("n_nodes", ctypes.c_int32),
                ("n_ch", ctypes.c_int32), ("k_nbr", ctypes.c_int32), ("transpose", ctypes.c_int32)]


@pytest.mark.gpu
def test_refusals_leave_the_outputs_alone():
    lib = tm.load()
    EINVAL = -1
    table = grid_table()
    B, N, C, K = 2, 66, 8, table.shape[1]
    gen = torch.Generator().manual_seed(4)
    x, adj, nbr = torch.randn(B, N, C, generator=gen).cuda(), pattern_adj(table, B, gen).cuda(), torch.from_numpy(table).cuda()
    buf = torch.full((2 * B * N * C,), -3.0).cuda()
    y = buf[:B * N * C]
    fn = lib.dll.truss_gcn_level_aggregate
    stream = ctypes.c_void_p(ops.stream_of(x.device))

    def item(**kw):
        a = _Agg(ctypes.sizeof(_Agg), x.data_ptr(), adj.data_ptr(), N * N, nbr.data_ptr(), y.data_ptr(), B, N, C, K, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert ctypes.sizeof(_Agg) == 72
    good = item()
    cases = {"x NULL": item(x=None), "adj NULL": item(adj=None), "nbr NULL": item(nbr=None), "y NULL": item(y=None),
             "k_nbr 0": item(k_nbr=0), "k_nbr 17": item(k_nbr=17), "n_ch 0": item(n_ch=0), "n_nodes 0": item(n_nodes=0),
             "n_batch -1": item(n_batch=-1), "y is x": item(y=x.data_ptr()), "y overlaps x": item(x=buf.data_ptr() + 16, y=buf.data_ptr()),
             "struct_size": item(struct_size=ctypes.sizeof(_Agg) - 4)}
    for name, bad in cases.items():
        before = x.clone()
        arr = (_Agg * 2)(good, bad)                                                  # the good item first: still nothing may be launched
        assert fn(ctypes.byref(arr), 2, stream) == EINVAL, name
        assert b"truss_gcn_level_aggregate" in lib.dll.truss_last_error()
        torch.cuda.synchronize()
        assert bool((buf == -3.0).all()) and torch.equal(x, before), name
    assert fn(None, 1, stream) == EINVAL and fn(None, -1, stream) == EINVAL
    assert fn(None, 0, stream) == 0                                                   # nothing to do
    empty = (_Agg * 1)(item(n_batch=0, x=None, y=None, adj=None, nbr=None, k_nbr=0))
    assert fn(ctypes.byref(empty), 1, stream) == 0                                    # an empty item passes unread
    torch.cuda.synchronize()
    assert bool((buf == -3.0).all())
    assert fn(ctypes.byref((_Agg * 1)(good)), 1, stream) == 0
    torch.cuda.synchronize()
    ref, mag = agg64(dict(x=x, adj=adj, table=table), False)
    assert bool(np.all(np.abs(GR.f64(y).reshape(B, N, C) - ref) <= bound(dict(table=table), mag))) and bool((buf[B * N * C:] == -3.0).all())


# ---- gcn_level through autograd on the GPU ---------------------------------------------------------------------------------------------

@contextlib.contextmanager
def hooks(lib, forward=True, backward=False, aggregate=True, log=None):
    prev = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda"), RL._LEVEL_AGGREGATE.get("cuda")
    agg = gcn.level_aggregate(lib)

    def logged(groups, xs, transpose):
        res = agg(groups, xs, transpose)
        log.append((len(groups), sum(len(x) for x in xs), bool(transpose), res is None))
        return res

    RL.set_level_forward(gcn.level_forward(lib) if forward else None, "cuda")
    RL.set_level_backward(gcn.level_backward(lib) if backward else None, "cuda")
    RL.set_level_aggregate((logged if log is not None else agg) if aggregate else None, "cuda")
    try:
        yield
    finally:
        RL.set_level_forward(prev[0], "cuda"), RL.set_level_backward(prev[1], "cuda"), RL.set_level_aggregate(prev[2], "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [66, 130])
def test_gcn_level_through_autograd_with_the_hook(N):
    """float32 on the GPU, the pattern groups through `truss_gcn_level_aggregate` (the front's group through the level kernels),
    against the float64 CPU result of the same call: outputs <= 1e-5, gradients <= 1e-4 of each tensor's norm (the caps of
    tests/test_update_float64.py), no tensor left out, no float64 gradient identically zero; the library path (no pattern, no hook)
    on the same inputs stays inside the same caps.
    Measured on an MI355X (outputs, gradients): 66 nodes 1.1e-07, 2.5e-07 (library 1.1e-07, 2.5e-07); 130 nodes 1.2e-07, 3.7e-07
    (library 1.2e-07, 3.8e-07)."""
    lib = tm.load()
    table = grid_table() if N == 66 else synthetic_table()
    reqs64, coef64 = make_mix(table, MIX_SEED[N])
    assert relu_margin(reqs64) > 5e-5                      # no relu changes side between float32 and float64 (pre-activations of size 1)
    o64, g64 = level_and_grads(reqs64, coef64, RL.NodePattern(table))
    reqs, coef = make_mix(table, MIX_SEED[N], dtype=torch.float32, device="cuda")
    log = []
    with hooks(lib, backward=True, log=log):
        o_t, g_t = level_and_grads(reqs, coef, RL.NodePattern(table))
    with hooks(lib, forward=False, aggregate=False):
        o_l, g_l = level_and_grads(reqs, coef, None)
    assert log == [(3, 3, False, False), (3, 3, True, False)]       # one call per direction for the three pattern groups
    assert len(o64) == 4 and len(g64) == 12 and all(float(g.abs().max()) > 0 for g in g64)
    rel = lambda got, want: float((got.detach().cpu().double() - want).norm() / want.norm())
    for name, got_o, got_g in (("table", o_t, g_t), ("library", o_l, g_l)):
        ro, rg = [rel(a, b) for a, b in zip(got_o, o64)], [rel(a, b) for a, b in zip(got_g, g64)]
        print(f"\n[gcn_level {N} nodes, {name}] outputs {max(ro):.3g}, gradients {max(rg):.3g}")
        assert max(ro) <= 1e-5 and max(rg) <= 1e-4, (name, ro, rg)


# ---- the update -----------------------------------------------------------------------------------------------------------------------

UPDATE_CASES = {"2x66": (2, 66, 6, 24, 8), "2x130": (2, 130, 6, 24, 8)}


def _table_batch(seed, B, table, P, device):
    """tests/test_update_float64._batch (shared A_n and mask), every node-graph adjacency zero outside the table"""
    N = table.shape[0]
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g).to(device)
    A = lambda: table_softmax_adj(table, B, g).to(device)
    A_p = lambda: torch.softmax(torch.randn(B, P, P, generator=g), -1).to(device)
    a_n, mask = A()[:1].expand(B, -1, -1), torch.ones(1, N, N).to(device).expand(B, -1, -1)
    state = lambda: [r(B, N, 13), a_n, A(), A(), A(), mask, r(B, P, 4), A_p()]
    return state(), [state() for _ in range(3)], [(r(B, N, 2), r(B, N, 3)) for _ in range(3)], r(B, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_update_with_the_pattern_against_float64(case, monkeypatch):
    """three updates at lr 1e-3 with `node_pattern` on and all three hooks installed, stage by stage against the float64 host model,
    teacher-forced, held the way tests/test_update_float64.py holds the library path (test_host_model_agrees_with_the_cpu_update):
    to the caps -- outputs and losses 1e-5, gradients 1e-4 -- the clip and the optimiser within their derived bounds, relu'(0) as
    that file treats it.  The library path (dense, no hook, no pattern) runs every stage from the same snapshots, is printed next to
    the path under test and must stay within the same caps.  (4 x the library's own ratio, which that file asks of the level kernels,
    is not asked here: the critics' gradients carry the factor Q - y, a difference of two sums over N x 2 200 features that cancels
    about fifty-fold, so that two valid float32 summation orders differ several-fold in that one ratio.)  The logs show that every
    level with node-graph layers went through the aggregation and that the level hooks saw the front's groups only.
    Largest ratios measured on an MI355X, under test / library path (output | loss | critic gradient | actor gradient):
      2x66    1.8e-07 / 1.8e-07 | 2.2e-06 / 2.2e-06 | 1.5e-06 / 1.5e-06 | 3.5e-07 / 3.5e-07
      2x130   2.0e-07 / 2.0e-07 | 3.6e-06 / 1.1e-06 | 8.3e-06 / 1.0e-06 | 3.5e-07 / 4.0e-07
    clip <= 0.20 and optimiser <= 0.99 of their bounds.  At 2x130 the critics' gradients are off by one factor per critic, the same
    for all of its tensors (5e-06 .. 6e-06 for every tensor of critic 1 in update 0): the loss's, not the layers'."""
    B, N, P, H, C = UPDATE_CASES[case]
    lib = tm.load()
    table = grid_table() if N == 66 else synthetic_table()
    torch.manual_seed(5)
    rl = RL.MADDPG(T.LR, M.ep, M.epd, M.gamma, H, C, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda")
    batches = [_table_batch(20 + k, B, table, P, "cuda") for k in range(3)]
    S, NS, A, R = batches[0]
    for t in (S[1], S[2], S[3], S[4]):
        assert not bool(t[0][~torch.from_numpy(pattern_mask(table)).cuda()].any())
    rl._ensure_ready(S, [t for a in A for t in a])
    rl_lib = copy.deepcopy(rl)
    spies = T._Spies(monkeypatch)
    entry = spies.watch(rl)
    flog, blog, alog = [], [], []
    prev = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda")
    with hooks(lib, log=alog):
        RL.set_level_forward(T._logged_forward(gcn.level_forward(lib), flog), "cuda")
        RL.set_level_backward(T._logged_backward(gcn.level_backward(lib), blog), "cuda")
        with RL.node_pattern(RL.NodePattern(table)):
            recs = T._run_updates(entry, batches)
        n = len(flog), len(blog), len(alog)
        RL.set_level_forward(None, "cuda"), RL.set_level_backward(None, "cuda"), RL.set_level_aggregate(None, "cuda")
        libs = T._library_records(spies, rl_lib, recs, batches)
    assert (RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda")) == prev
    assert min(n) > 0 and n == (len(flog), len(blog), len(alog))                     # the hooks ran, and not for the library's figures
    assert all(inside == groups and not back for groups, inside, _, _, back in flog), flog      # the level kernels: the front's groups only
    assert all(not back for *_, back in blog), blog
    assert not any(declined for *_, declined in alog) and any(tr for _, _, tr, _ in alog) and any(not tr for _, _, tr, _ in alog)
    names, title = UR.names_of(rl), f"gpu {case}, node pattern on"
    batches64 = [UR.batch64(b) for b in batches]
    ref = T._staged(UR.Update64(rl.gamma, T.LR), recs, batches64, names)
    fig, zeros = T._ratios(ref, recs, names)
    lib_ref = T._staged(UR.Update64(rl.gamma, T.LR), libs, batches64, names)
    lib_fig, _ = T._ratios(lib_ref, libs, names)
    fig["out"], fig["clip"], fig["opt"], lib_fig["out"] = ref["out"], ref["clip"], ref["opt"], lib_ref["out"]
    assert ref["signs"][1] == 0 and lib_ref["signs"][1] == 0
    T._report(f"{title}: library path against float64", lib_fig)
    T._report(f"{title}: update under test against float64", fig)
    assert not zeros, f"float64 gradient tensors that are exactly zero (nothing to compare): {zeros}"
    T._taus(lib_fig, title)                                # (printed: what 4 x the library path would have been)
    T._assert_within(lib_fig, dict(T.CAPS), title + ", library path")
    T._assert_within(fig, dict(T.CAPS), title)


# ---- the engines ----------------------------------------------------------------------------------------------------------------------

def _light_batch(topo, n_envs, seed):
    """synthetic.random_batch with a hundredth of the load and a hundred times the deflection limit: at 32 and 66 nodes (spans of about
    100 m) no candidate of the plain batch is feasible, nothing reaches the replay and nothing trains"""
    b = synthetic.random_batch(topo, n_envs, seed)
    b["load_y"], b["max_def"] = b["load_y"] * 1e-2, b["max_def"] * 1e2
    return b


def _agents(lr):
    """MADDPG (hidden width 24, critic width 8) with every lazy layer materialised now, from the global generator as it stands"""
    rl = RL.MADDPG(lr, M.ep, M.epd, M.gamma, 24, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda")
    S, _, A, _ = T._batch(1, 2, 12, 6, "cuda", True)
    rl._ensure_ready(S, [t for a in A for t in a])
    return rl


def _engine(lib, topo, adjacency, n_envs=8, lr=1e-4, **kw):
    torch.manual_seed(5)
    rl = _agents(lr)
    eng = marl.BatchedMARL(topo, n_envs, rl, max_front=6, lib=lib, device="cuda", replay_capacity=256, batch_size=4, seed=5,
                           level_adjacency=adjacency, tune_update_gemms=False, **kw)
    b = _light_batch(topo, n_envs, 5)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng, rl


def _weights(rl):
    return [p for ag in rl.agents for net in (ag.actor_model, ag.critic_model) for p in net.parameters()]


def _count_aggregate_calls(calls):
    agg = RL._LEVEL_AGGREGATE["cuda"]
    RL.set_level_aggregate(lambda *a: calls.append(a[2]) or agg(*a), "cuda")


@pytest.mark.gpu
def test_engine_table_against_dense():
    """BatchedMARL(grid(33), 8 envs, batch 4): "table" against "dense" from the same seed (one engine after the other: the lazy
    layers draw their initial weights from the global generator) -- after three game steps with training every weight agrees at
    rtol 1e-4, atol 2e-6 (learning rate 1e-4, as in the test those figures come from); the replayed graph of the "table" engine
    gives the eager update's weight deltas; every sampled node-graph adjacency is exactly zero outside the table"""
    lib = tm.load()
    topo = tm.TrussTopology.grid(33)
    prev = RL._LEVEL_AGGREGATE.get("cuda")
    calls = []
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            eng_d, rl_d = _engine(lib, topo, "dense")
            for _ in range(3):
                eng_d.game_step_all(train=True, explore=True, train_iters=1)
            eng_t, rl_t = _engine(lib, topo, "table")
            assert eng_t.pattern is not None and eng_d.pattern is None and "cuda" in RL._LEVEL_AGGREGATE
            _count_aggregate_calls(calls)
            start = [p.detach().clone() for p in _weights(rl_t)]
            for _ in range(3):
                eng_t.game_step_all(train=True, explore=True, train_iters=1)
        assert len(calls) > 0 and eng_t._tg is not None and eng_d._tg is not None
        assert eng_t.replay.size == eng_d.replay.size >= eng_t.batch_size
        assert max(float((p.detach() - s).abs().max()) for p, s in zip(_weights(rl_t), start)) > 1e-4
        for p, q in zip(_weights(rl_t), _weights(rl_d)):
            torch.testing.assert_close(p, q, rtol=1e-4, atol=2e-6)
        # the sampled adjacencies
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        outside = ~torch.from_numpy(pattern_mask(topo.neighbor_table())).cuda()
        S, NS, ag, at, R = eng_t.replay.sample(eng_t.batch_size, g)
        for state in [eng_t._net_state(S)] + [eng_t._net_state(ns) for ns in NS]:
            for a in state[1:5]:
                assert a.shape[-2:] == outside.shape and not bool(a[:, outside].any())
        # replay against eager, as tests/test_gcn_level_backward.test_train_graph_with_hip_backward_replays_like_eager
        rl, eng = rl_t, eng_t
        params = _weights(rl)
        state = params + [p for ag_ in rl.agents for n in (ag_.target_actor_model, ag_.target_critic_model) for p in n.parameters()]
        state += rl.critics_opt.state_tensors()
        snap = [t.detach().clone() for t in state]

        def batches(seed):
            g.manual_seed(seed)
            out = []
            for _ in range(3):
                S, NS, ag, at, R = eng.replay.sample(eng.batch_size, g)
                out.append((eng._net_state(S), [eng._net_state(ns) for ns in NS], [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)], R))
            return out

        def deltas(bs, graph):
            with torch.no_grad():
                for t, v in zip(state, snap):
                    t.copy_(v)
            eng.use_train_graph = graph
            for b_ in bs:
                eng._train(*b_)
            torch.cuda.synchronize()
            return torch.cat([(p.detach() - v).flatten().double() for p, v in zip(params, snap)])

        fixed = batches(1)
        n0 = len(calls)
        d_eager = deltas(fixed, False)
        n_eager = len(calls) - n0
        d_graph = deltas(fixed, True)
        assert eng.use_train_graph and n_eager > 0 and len(calls) == n0 + n_eager           # (a replay: no Python ran)
        d_other = deltas(batches(2), False)
        rel = lambda d: float((d - d_eager).norm() / d_eager.norm())
        print(f"\n[train graph, table adjacency] ||dW_graph - dW_eager|| / ||dW_eager|| = {rel(d_graph):.3g}; other batches: {rel(d_other):.3g}")
        assert float(d_eager.abs().max()) > 1e-4
        assert rel(d_graph) <= 0.05
        assert rel(d_other) > 0.05
    finally:
        RL.set_level_aggregate(prev, "cuda")


@pytest.mark.gpu
def test_option_changes_nothing_up_to_64_nodes_and_reaches_every_class():
    """MixedMARL over grid(16) (32 nodes) and grid(33) (66 nodes), level_adjacency="table": a game step with training runs; every class
    brings its own table; the 32-node class's update is bit for bit that of the option off (a step in which only that class
    updates: it is the first in turn)"""
    lib = tm.load()
    prev = RL._LEVEL_AGGREGATE.get("cuda")
    try:
        calls, after = [], {}
        with contextlib.redirect_stdout(io.StringIO()):
            for adjacency in ("dense", "table"):            # one after the other: the lazy layers draw from the global generator
                torch.manual_seed(4)
                rl = _agents(1e-3)
                classes = pool.grid_classes([16, 33], [16, 8])
                mix = marl.MixedMARL(classes, rl, bucket_envs=8, max_front=6, lib=lib, device="cuda", replay_capacity=128, batch_size=4, seed=2,
                                     tune_update_gemms=False, level_adjacency=adjacency)
                per_class = []
                for k, e in enumerate(mix.engines):
                    full = _light_batch(e.topo, classes[mix.class_ids[k]][1], 9 + k)
                    per_class.append({key: v[mix.global_ids(k)] for key, v in full.items()})
                mix.reset(per_class)
                assert [e.topo.N for e in mix.engines] == [32, 66] and all(e.level_adjacency == adjacency for e in mix.engines)
                if adjacency == "table":
                    assert [e.pattern.n_nodes for e in mix.engines] == [32, 66]              # every class brings its own table
                    _count_aggregate_calls(calls)
                else:
                    assert all(e.pattern is None for e in mix.engines)
                for _ in range(2):                                                           # fill both replays, no update yet
                    for e in mix.engines:
                        e.game_step_all(train=True, explore=True, update=False)
                assert all(e.replay.size >= e.batch_size for e in mix.engines)
                before = [p.detach().clone() for p in _weights(rl)]
                out = mix.game_step_all(train=True, explore=True, train_iters=1)
                assert out["updates"] == 1 and mix._turn == 1                                # the 32-node class updated, alone
                assert any(not torch.equal(p, b) for p, b in zip(_weights(rl), before))
                after[adjacency] = [p.detach().clone() for p in _weights(rl)]
                if adjacency == "table":
                    assert calls == []                                                       # ... on the dense paths
                    out = mix.game_step_all(train=True, explore=True, train_iters=1)         # the 66-node class's turn
                    assert out["updates"] == 1 and mix._turn == 2 and len(calls) > 0
                    assert all(bool(torch.isfinite(p).all()) for p in _weights(rl))
        for p, q in zip(after["table"], after["dense"]):
            assert torch.equal(p, q)
    finally:
        RL.set_level_aggregate(prev, "cuda")
