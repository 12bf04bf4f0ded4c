"""A GCN layer with a consumer of its output in the epilogue of the same launch (truss_gcn_layer_fused, csrc/truss_gcn.h): the
head and pool epilogues of both layer kernels against float64, their operator and wrappers (marl.gcn_layer_head / gcn_layer_pool),
actor_infer(fused=True) and the engine switch BatchedMARL(actor_path="fused").

Bounds are elementwise, |got - ref64| <= tau * Mag with the project's tau = 1e-6 (gcn_reference.TAU), and composite:

    Mag1 = |A1| (|X| |W1|^T) + |b1|                        the hidden layer's (gcn_reference.layer_ref)
    head: Mag = |A2| ((Mag1 + |V64|) |W2|^T) + |b2|         (relu is 1-Lipschitz, sigmoid 1/4-Lipschitz)
    pool: tau * sum_n Mag1 + N * 2^-24 * sum_n |V64|        (the second term: the worst case of any float32 summation order)

Every bound is shown to have teeth on the inputs of the GPU tests themselves, without a GPU: a host model of the fused arithmetic
(bf16x3 hidden product, float32 from there on) passes and every host mutant (A1 used for A2, b1 left out, the hidden relu left out,
hidden columns 192.. left out of the head product, b2 left out; pool: the last row of every graph left out) fails.

Measured max |got - ref64| / bound (the bound's tau * Mag, or the pool's two-term bound): see the docstrings of the GPU tests."""
import contextlib
import copy
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import gcn, marl, ops, synthetic
import parity_common as pc
import gcn_reference as G
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL

TAU = G.TAU["bf16x3"]
assert TAU == G.TAU["f32"] == 1e-6


def _pattern(tab):
    N = tab.shape[0]
    pat = np.zeros((N, N), bool)
    for i in range(N):
        pat[i, tab[i][tab[i] >= 0]] = True
    return pat


def _random_pattern(N, terms, seed):
    """a neighbour table of `terms` distinct columns per row (the node itself among them)"""
    rng = np.random.default_rng(seed)
    tab = np.empty((N, terms), np.int16)
    for i in range(N):
        others = rng.choice(np.delete(np.arange(N), i), terms - 1, replace=False)
        tab[i] = np.sort(np.concatenate([[i], others]))
    return tab


# ---- the cases: host tensors from a seeded generator, shared by the GPU tests and the CPU test of their teeth ---------------------

# name: (graph, B, k_in, c_out, c2, act2, A1 per env, A2 per env, hidden out requested)
HEAD_CASES = {
    "12 nodes": ("grid6", 21, 200, 200, 3, "sigmoid", True, False, False),      # 10 graphs per tile (120 live rows), the last holds one
    "16 nodes": ("grid8", 9, 200, 200, 2, None, True, True, True),
    "24 nodes, 9 + 6 terms": ("rand24", 6, 200, 200, 3, "sigmoid", True, True, False),
    "64 nodes": ("grid32", 3, 200, 200, 3, "sigmoid", True, False, False),
    "256 nodes": ("grid128", 2, 200, 200, 2, "sigmoid", False, True, False),     # NW = 8: one graph spans all eight waves
    "c_out 224, c2 8": ("grid8", 5, 200, 224, 8, None, True, True, False),
    "c_out 33": ("grid8", 5, 200, 33, 2, "sigmoid", True, True, False),
    "k_in 16": ("grid8", 5, 16, 200, 3, "sigmoid", True, True, False),
}
# name: (graph, B, k_in, c_out)
POOL_CASES = {
    "dense 7": ("dense7", 40, 4, 200),
    "path 20": ("path20", 13, 4, 200),                                          # 6 graphs per tile, the last tile holds one
    "path 50": ("path50", 5, 4, 200),                                           # 2 graphs per tile, 100 live rows
    "dense 64, float32 kernel": ("dense64", 3, 16, 33),
    "256 nodes": ("grid128", 2, 200, 200),
}


def _graph(kind):
    """(N, table of A1 or None, table of A2 or None, one shared adjacency or None)"""
    if kind.startswith("grid"):
        topo = tm.TrussTopology.grid(int(kind[4:]))
        tab = topo.neighbor_table()
        return topo.N, tab, tab, topo.normalized_adjacency()[0]
    if kind == "rand24":
        return 24, _random_pattern(24, 9, 1), _random_pattern(24, 6, 2), None
    if kind.startswith("path"):
        P = int(kind[4:])
        return P, marl.path_graph_table(P), None, None
    return int(kind[5:]), None, None, None                                      # dense


def _adjacency(g, B, N, tab, shared, per_env):
    if not per_env:
        return torch.tensor(shared) if shared is not None else torch.softmax(torch.randn(N, N, generator=g), -1)
    if tab is None:
        return torch.softmax(torch.randn(B, N, N, generator=g), dim=-1)
    return torch.rand(B, N, N, generator=g) * torch.tensor(_pattern(tab))


@functools.lru_cache(maxsize=None)
def head_case(name):
    """inputs (host, float32), float64 reference, bound magnitude and mutants of a head case; computed once per session"""
    kind, B, K, C, c2, act2, env1, env2, want_out = HEAD_CASES[name]
    g = torch.Generator(device="cpu").manual_seed(sorted(HEAD_CASES).index(name) + 100)
    N, tab1, tab2, shared = _graph(kind)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(x=rn(B, N, K), w=rn(C, K) / K ** 0.5, b=rn(C), w2=rn(c2, C) / C ** 0.5, b2=rn(c2), act2=act2, want_out=want_out,
             adj=_adjacency(g, B, N, tab1, shared, env1), adj2=_adjacency(g, B, N, tab2, shared, env2),
             nbr=torch.tensor(tab1), nbr2=torch.tensor(tab2))
    X, W, b1, W2, b2 = (G.f64(c[k]) for k in ("x", "w", "b", "w2", "b2"))
    A1, A2 = G.dense_adj(c["adj"], B, N), G.dense_adj(c["adj2"], B, N)
    pre = A1 @ (X @ W.T)
    V, mag1 = G.layer_ref(c["x"], c["adj"], c["w"], c["b"], "relu")
    head = lambda a2, v, w2, bias2: G.act64(a2 @ (v @ w2.T) + bias2, act2)
    c["V"], c["mag1"] = V, mag1
    c["ref"] = head(A2, V, W2, b2)
    c["mag"] = np.abs(A2) @ ((mag1 + np.abs(V)) @ np.abs(W2).T) + np.abs(b2)
    W2cut = W2.copy()
    W2cut[:, 192:] = 0.0
    c["mutants"] = {"A1 used for A2": head(A1, V, W2, b2), "b1 left out": head(A2, np.maximum(pre, 0.0), W2, b2),
                    "hidden relu left out": head(A2, pre + b1, W2, b2), "b2 left out": head(A2, V, W2, 0.0)}
    if C > 192:
        c["mutants"]["hidden columns 192.. left out"] = head(A2, V, W2cut, b2)
    return c


@functools.lru_cache(maxsize=None)
def pool_case(name):
    kind, B, K, C = POOL_CASES[name]
    g = torch.Generator(device="cpu").manual_seed(sorted(POOL_CASES).index(name) + 200)
    N, tab, _, _ = _graph(kind)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(x=rn(B, N, K), w=rn(C, K) / K ** 0.5, b=rn(C), adj=_adjacency(g, B, N, tab, None, True),
             nbr=torch.tensor(tab) if tab is not None else None)
    V, mag1 = G.layer_ref(c["x"], c["adj"], c["w"], c["b"], "relu")
    c["V"], c["ref"] = V, V.sum(axis=1)
    c["bound"] = TAU * mag1.sum(axis=1) + N * 2.0 ** -24 * np.abs(V).sum(axis=1)
    c["mutants"] = {"last row of every graph left out": V[:, :-1].sum(axis=1)}
    return c


def _ratio(got, ref, bound):
    """max |got - ref| / bound (a zero bound must be met exactly)"""
    return G.max_ratio(got, ref, bound)


def _on(c, device, *keys):
    return [c[k].to(device) if c[k] is not None else None for k in keys]


# ---- teeth, without a GPU -------------------------------------------------------------------------------------------------------

def _hidden_model32(c):
    """the hidden layer as the bf16x3 kernel computes it (gcn_reference.bf16x3_model), rounded to float32"""
    return G.bf16x3_model(c["x"], c["adj"], c["w"], c["b"], "relu").astype(np.float32)


@pytest.mark.parametrize("name", sorted(HEAD_CASES))
def test_head_bound_has_teeth(name):
    """on the GPU test's own inputs: the host model of the fused arithmetic (bf16x3 hidden product, then float32: h2 = V W2^T,
    A2 h2 + b2, activation) is within tau * Mag of float64, and every mutant is outside it"""
    c = head_case(name)
    B, N, _ = c["x"].shape
    V32 = _hidden_model32(c)
    A2 = G.dense_adj(c["adj2"], B, N).astype(np.float32)
    h2 = V32 @ c["w2"].numpy().T
    z = (A2 @ h2 + c["b2"].numpy()).astype(np.float32)
    model = G.act64(z, c["act2"]).astype(np.float32)
    r = _ratio(model, c["ref"], c["mag"])
    assert r <= TAU, f"{name}: host model at {r:.3g} * Mag"
    for mname, m in c["mutants"].items():
        assert not G.within(m, c["ref"], c["mag"], TAU), f"{name}: mutant '{mname}' passes the bound"
    if c["want_out"]:
        assert G.within(V32, c["V"], c["mag1"], TAU)


@pytest.mark.parametrize("name", sorted(POOL_CASES))
def test_pool_bound_has_teeth(name):
    """the same for the pool: the float32 sum of the modelled hidden rows, in row order, is inside the bound, the sum without the
    last row of every graph is outside"""
    c = pool_case(name)
    V32 = _hidden_model32(c)
    s = np.zeros((V32.shape[0], V32.shape[2]), np.float32)
    for n in range(V32.shape[1]):
        s = s + V32[:, n]
    r = _ratio(s, c["ref"], c["bound"])
    assert r <= 1.0, f"{name}: host model at {r:.3g} of the bound"
    for mname, m in c["mutants"].items():
        assert not bool(np.all(np.abs(m - c["ref"]) <= c["bound"])), f"{name}: mutant '{mname}' passes the bound"


# ---- the kernels against float64 ------------------------------------------------------------------------------------------------

def _bf16x3_taken(c):
    N = c["x"].shape[1]
    return c["w"].shape[0] > 32 and c["x"].shape[2] % 4 == 0 and (c["nbr"].shape[1] if c["nbr"] is not None else N) <= 9


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", sorted(HEAD_CASES))
def test_head_float64_hip(name, precision):
    """truss_gcn_layer_fused, head epilogue, on both products: |out2 - ref64| <= tau * Mag elementwise; the hidden output, where
    requested, within the layer's own bound and equal to truss_gcn_layer's; every mutant outside the bound.

    Measured on an MI355X, max |got - ref64| / Mag (tau = 1e-6): bf16x3 product 1.9e-9 (c_out 224, c2 8; 16 nodes 1.6e-9, the other
    cases 2.3e-10 ... 6.8e-10), float32 product 1.7e-9 (same case; 16 nodes 1.4e-9, the others 2.0e-10 ... 6.8e-10); the hidden
    output of the 16-node case 1.1e-7 / 9.5e-8 of the layer's own Mag1.  The weakest host mutant over the cases (hidden columns
    192.. left out, 24 nodes) lies 359 x outside the bound."""
    lib = tm.load()
    c = head_case(name)
    x, adj, w, b, w2, b2, adj2, nbr, nbr2 = _on(c, "cuda", "x", "adj", "w", "b", "w2", "b2", "adj2", "nbr", "nbr2")
    out = torch.full((x.shape[0], x.shape[1], w.shape[0]), float("nan"), device="cuda") if c["want_out"] else None
    got = marl.gcn_layer_head(lib, x, adj, w, b, "relu", w2, b2, adj2, c["act2"], nbr, nbr2, precision=precision, out=out)
    r = _ratio(got, c["ref"], c["mag"])
    path = "bf16x3" if precision == "bf16x3" and _bf16x3_taken(c) else "f32"
    print(f"\n[fused head] {name} {precision} ({path} product): max |got - ref64| / Mag = {r:.3g}")
    assert r <= TAU, f"{name} {precision}: max |got - ref64| / Mag = {r:.3g} > {TAU:g}"
    for mname, m in c["mutants"].items():
        assert not G.within(m, c["ref"], c["mag"], TAU), f"{name}: mutant '{mname}' passes the bound"
    if out is not None:
        ro = _ratio(out, c["V"], c["mag1"])
        print(f"[fused head] {name} {precision}: hidden out, max ratio {ro:.3g}")
        assert ro <= TAU
        assert torch.equal(out, marl.gcn_layer(lib, x, adj, w, b, "relu", nbr, precision=precision))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", sorted(POOL_CASES))
def test_pool_float64_hip(name, precision):
    """truss_gcn_layer_fused, pool epilogue, on both products: |pool - ref64| <= tau * sum_n Mag1 + N 2^-24 sum_n |V64|; the sum
    without the last row of every graph is outside that bound.

    Measured on an MI355X, max |got - ref64| / bound: dense 7 0.094, path 20 0.082, path 50 0.058 (bf16x3) / 0.053 (f32), dense 64
    (float32 kernel on both settings) 0.048, 256 nodes 0.019 / 0.021.  The mutant lies 383 x (256 nodes) to 1.4e5 x outside."""
    lib = tm.load()
    c = pool_case(name)
    x, adj, w, b, nbr = _on(c, "cuda", "x", "adj", "w", "b", "nbr")
    got = marl.gcn_layer_pool(lib, x, adj, w, b, "relu", nbr, precision=precision)
    r = _ratio(got, c["ref"], c["bound"])
    path = "bf16x3" if precision == "bf16x3" and _bf16x3_taken(c) else "f32"
    print(f"\n[fused pool] {name} {precision} ({path} product): max |got - ref64| / bound = {r:.3g}")
    assert r <= 1.0, f"{name} {precision}: {r:.3g} of the bound"
    for mname, m in c["mutants"].items():
        assert not bool(np.all(np.abs(m - c["ref"]) <= c["bound"])), f"{name}: mutant '{mname}' passes the bound"


# ---- reproducible and in bounds --------------------------------------------------------------------------------------------------

PAD = 64        # guard floats in front of and behind every output
POISON = -7.25e11


class Guarded:
    """an output tensor inside a larger buffer: NaN payload, poison around it"""

    def __init__(self, shape, device):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), POISON, dtype=torch.float32, device=device)
        self.t = self.buf[PAD:PAD + n].view(*shape)
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[:PAD] == POISON).all()) and bool((self.buf[-PAD:] == POISON).all())


@pytest.mark.gpu
def test_fused_is_reproducible_and_stays_in_bounds():
    """two calls on the same inputs give identical bits; out2 / pool pre-filled with NaN inside poisoned buffers come back fully
    written with the poison intact; with out == NULL no input changes; with out given, out2 / pool are the same bits"""
    lib = tm.load()
    for name, precision in (("12 nodes", "bf16x3"), ("12 nodes", "f32"), ("24 nodes, 9 + 6 terms", "bf16x3"), ("256 nodes", "bf16x3"), ("c_out 33", "f32")):
        c = head_case(name)
        ins = _on(c, "cuda", "x", "adj", "w", "b", "w2", "b2", "adj2", "nbr", "nbr2")
        x, adj, w, b, w2, b2, adj2, nbr, nbr2 = ins
        B, N, C, c2 = x.shape[0], x.shape[1], w.shape[0], w2.shape[0]
        keep = [t.clone() for t in ins]
        res = []
        for with_out in (False, False, True):
            o2 = Guarded((B, N, c2), "cuda")
            o = Guarded((B, N, C), "cuda") if with_out else None
            gcn._gcn_layer_fused(lib, x, adj, w, b, "relu", nbr, precision, None, o.t if o else None, 1, w2, b2, adj2, nbr2, c["act2"], out2=o2.t)
            assert o2.intact() and not bool(torch.isnan(o2.t).any()), f"{name} {precision}"
            assert o is None or (o.intact() and not bool(torch.isnan(o.t).any()))
            res.append(o2.t)
        assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]), f"{name} {precision}"
        assert all(torch.equal(a, k) for a, k in zip(ins, keep))
    for name, precision in (("path 20", "bf16x3"), ("dense 7", "f32"), ("dense 64, float32 kernel", "bf16x3"), ("256 nodes", "bf16x3")):
        c = pool_case(name)
        ins = _on(c, "cuda", "x", "adj", "w", "b", "nbr")
        x, adj, w, b, nbr = ins
        B, N, C = x.shape[0], x.shape[1], w.shape[0]
        keep = [t.clone() if t is not None else None for t in ins]
        res = []
        for with_out in (False, False, True):
            p = Guarded((B, C), "cuda")
            o = Guarded((B, N, C), "cuda") if with_out else None
            gcn._gcn_layer_fused(lib, x, adj, w, b, "relu", nbr, precision, None, o.t if o else None, 2, pool=p.t)
            assert p.intact() and not bool(torch.isnan(p.t).any()), f"{name} {precision}"
            assert o is None or (o.intact() and not bool(torch.isnan(o.t).any()))
            res.append(p.t)
        assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]), f"{name} {precision}"
        assert all(k is None or torch.equal(a, k) for a, k in zip(ins, keep))


# ---- refusals --------------------------------------------------------------------------------------------------------------------

class _LayerArgs(ctypes.Structure):          # truss_gcn_layer_args_t (include/truss_mi355.h)
    _fields_ = [("struct_size", ctypes.c_size_t)] + [(n, ctypes.c_int32) for n in ("n_batch", "n_nodes", "k_in", "c_out", "act", "accumulate", "k_nbr", "reserved")] + \
               [("x", ctypes.c_void_p), ("x_row_stride", ctypes.c_int64), ("adj", ctypes.c_void_p), ("a_batch_stride", ctypes.c_int64),
                ("nbr", ctypes.c_void_p), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("out_row_stride", ctypes.c_int64), ("w_bf16x3", ctypes.c_void_p)]


class _EpiArgs(ctypes.Structure):            # truss_gcn_epilogue_t
    _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_int32), ("w2", ctypes.c_void_p), ("bias2", ctypes.c_void_p),
                ("adj2", ctypes.c_void_p), ("a2_batch_stride", ctypes.c_int64), ("nbr2", ctypes.c_void_p), ("k_nbr2", ctypes.c_int32),
                ("c2", ctypes.c_int32), ("act2", ctypes.c_int32), ("out2", ctypes.c_void_p), ("out2_row_stride", ctypes.c_int64),
                ("pool", ctypes.c_void_p), ("pool_row_stride", ctypes.c_int64)]


@pytest.mark.gpu
def test_fused_refusals():
    """every TRUSS_EINVAL / TRUSS_EUNSUPPORTED case of the entry's contract raises with the library's code and writes nothing;
    n_batch == 0 is a no-op"""
    lib = tm.load()
    assert lib.has_gcn_fused
    dev = "cuda"
    B, N, K, C, c2 = 2, 8, 16, 40, 3
    tab = torch.tensor(marl.path_graph_table(N), device=dev)
    x, adj, w, b = torch.ones(B, N, K, device=dev), torch.ones(N, N, device=dev), torch.ones(C, K, device=dev), torch.ones(C, device=dev)
    w2, b2 = torch.ones(c2, C, device=dev), torch.ones(c2, device=dev)
    out, out2, pool = (torch.full(s, 7.0, device=dev) for s in ((B, N, C), (B, N, c2), (B, C)))
    big = torch.ones(B * 65 * K, device=dev)                   # x of a 65-node graph
    adj65, tab65 = torch.ones(65, 65, device=dev), torch.tensor(marl.path_graph_table(65), device=dev)
    st = ops.stream_of(x.device)

    def layer(**kw):
        a = dict(struct_size=ctypes.sizeof(_LayerArgs), n_batch=B, n_nodes=N, k_in=K, c_out=C, act=1, x=x.data_ptr(), adj=adj.data_ptr(),
                 w=w.data_ptr(), bias=b.data_ptr(), out=None)
        a.update(kw)
        return _LayerArgs(**a)

    def head(**kw):
        a = dict(struct_size=ctypes.sizeof(_EpiArgs), kind=1, w2=w2.data_ptr(), bias2=b2.data_ptr(), adj2=adj.data_ptr(), c2=c2, act2=2,
                 out2=out2.data_ptr())
        a.update(kw)
        return _EpiArgs(**a)

    def pooled(**kw):
        a = dict(struct_size=ctypes.sizeof(_EpiArgs), kind=2, pool=pool.data_ptr())
        a.update(kw)
        return _EpiArgs(**a)

    def call(la, ep):
        return lib.check(lib.dll.truss_gcn_layer_fused(ctypes.byref(la), ctypes.byref(ep), st), "truss_gcn_layer_fused")

    EINVAL, EUNSUP = r"failed \(-1\)", r"failed \(-2\)"
    l65 = dict(n_nodes=65, x=big.data_ptr(), adj=adj65.data_ptr(), nbr=tab65.data_ptr(), k_nbr=3)
    refused = [
        (layer(), head(struct_size=ctypes.sizeof(_EpiArgs) - 8), EINVAL), (layer(struct_size=8), head(), EINVAL),
        (layer(), head(kind=0), EINVAL), (layer(), head(kind=3), EINVAL),
        (layer(), head(c2=0), EINVAL), (layer(), head(c2=9), EINVAL), (layer(), head(act2=3), EINVAL), (layer(), head(act2=-1), EINVAL),
        (layer(), head(w2=None), EINVAL), (layer(), head(adj2=None), EINVAL), (layer(), head(out2=None), EINVAL),
        (layer(), pooled(pool=None), EINVAL),
        (layer(), head(nbr2=tab.data_ptr(), k_nbr2=0), EUNSUP), (layer(), head(nbr2=tab.data_ptr(), k_nbr2=17), EUNSUP),
        (layer(**l65), head(adj2=adj65.data_ptr()), EUNSUP),                                        # a dense adj2 above 64 nodes
        (layer(accumulate=1, out=out.data_ptr()), head(), EINVAL), (layer(accumulate=1, out=out.data_ptr()), pooled(), EINVAL),
        (layer(act=3), head(), EINVAL), (layer(x=None), pooled(), EINVAL), (layer(c_out=225), pooled(), EUNSUP),
        (layer(), head(out2=x.data_ptr()), EINVAL), (layer(), pooled(pool=x.data_ptr() + 64), EINVAL),
        (layer(out=out.data_ptr()), head(out2=out.data_ptr() + 4 * C), EINVAL), (layer(out=out.data_ptr()), pooled(pool=out.data_ptr()), EINVAL),
        (layer(), head(pool=out2.data_ptr() + 8), EINVAL),                                           # out2 and pool overlap each other
    ]
    for la, ep, code in refused:
        with pytest.raises(tm.TrussError, match=code):
            call(la, ep)
    assert call(layer(n_batch=0), head()) == 0 and call(layer(n_batch=0), pooled()) == 0
    ns, lid = ops.namespace(), ops.bind(lib)
    with pytest.raises(tm.TrussError, match="out2 must be"):                                             # the operator's own tensor checks
        ops.call(ns.gcn_layer_fused, lid, st, x, adj, None, w, b, None, 1, None, 1, w2, b2, adj, None, 2, pool, None)
    with pytest.raises(tm.TrussError, match=r"truss_gcn_layer_fused failed \(-1\)"):
        ops.call(ns.gcn_layer_fused, lid, st, x, adj, None, w, b, None, 1, None, 2, None, None, None, None, 0, None, None)
    torch.cuda.synchronize()
    for t, v in ((out, 7.0), (out2, 7.0), (pool, 7.0), (x, 1.0), (big, 1.0)):
        assert torch.equal(t, torch.full_like(t, v))


def test_emulator_lacks_the_entry_and_the_engine_refuses_it():
    """the CPU lane emulator does not export truss_gcn_layer_fused: its operator names the symbol, BatchedMARL(actor_path="fused")
    is refused at construction, and so is a value that is neither "layers" nor "fused" """
    lib = pc.emu_lib()
    assert not lib.has_gcn_fused
    t = lambda *s: torch.zeros(*s)
    with pytest.raises(tm.TrussError, match=r"has no truss_gcn_layer_fused$"):
        ops.call(ops.namespace().gcn_layer_fused, ops.bind(lib), 0, t(1, 2, 4), t(2, 2), None, t(4, 4), None, None, 1, None, 2,
                 None, None, None, None, 0, None, t(1, 4))
    topo = tm.TrussTopology.grid(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 16, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    kw = dict(max_front=6, lib=lib, device="cpu", replay_capacity=64, batch_size=8)
    with pytest.raises(ValueError, match="has no truss_gcn_layer_fused"):
        marl.BatchedMARL(topo, 2, rl, actor_path="fused", **kw)
    with pytest.raises(ValueError, match="actor_path must be"):
        marl.BatchedMARL(topo, 2, rl, actor_path="heads", **kw)
    assert marl.BatchedMARL(topo, 2, rl, **kw).actor_path == "layers"


def test_actor_path_follows_the_environment(monkeypatch):
    monkeypatch.setenv("TRUSS_ACTOR", "fused")
    topo = tm.TrussTopology.grid(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 16, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    with pytest.raises(ValueError, match="has no truss_gcn_layer_fused"):          # None -> "fused", which the emulator lacks
        marl.BatchedMARL(topo, 2, rl, max_front=6, lib=pc.emu_lib(), device="cpu", replay_capacity=64, batch_size=8)
    assert marl.BatchedMARL(topo, 2, rl, max_front=6, lib=pc.emu_lib(), device="cpu", replay_capacity=64, batch_size=8,
                            actor_path="layers").actor_path == "layers"


# ---- the actor end to end --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("P", [20, 50])
def test_actor_infer_fused_float64_hip(P, monkeypatch):
    """actor_infer(fused=True) on the inputs of test_gcn_float64._check_actor_infer_float64 (hidden 200, heads 2 and 3, 16 nodes,
    path table of P): max error against the float64 module no worse than 4x the float32 module's, outputs within 2e-5 of
    actor_infer(fused=False); 8 plain layer launches + 2 heads + 1 pool, no launch of the layers they replace.

    Measured on an MI355X (geometry / topology output): P 20 max error 1.5e-7 / 2.2e-7 against the float32 module's 1.1e-7 / 1.6e-7,
    P 50 2.1e-7 / 1.9e-7 against 1.8e-7 / 1.4e-7; at most 2.4e-7 from the layer path."""
    lib = tm.load()
    torch.manual_seed(9)
    B, device = 37, "cuda"
    topo = tm.TrussTopology.grid(8)
    N, tab = topo.N, topo.neighbor_table()
    patt = torch.tensor(_pattern(tab), device=device)
    actor = RL.multimodes_actor(200, 2, 3).to(device)
    r = lambda *s: torch.rand(*s, device=device)
    pts = torch.rand(B, P, 4, dtype=torch.float64, device=device)
    x_p, A_p = marl.pareto_graph(pts, torch.randint(1, P + 1, (B,), device=device), torch.zeros(B, dtype=torch.long, device=device), P)
    A_n = torch.tensor(topo.normalized_adjacency()[0], device=device)
    ins = [r(B, N, 13), A_n, r(B, N, N) * patt, r(B, N, N) * patt, r(B, N, N) * patt, x_p, A_p]
    mod_in = [ins[0], A_n[None].expand(B, -1, -1)] + ins[2:]
    nbr, nbr_p = torch.tensor(tab, device=device), torch.tensor(marl.path_graph_table(P), device=device)
    calls = {"layer": 0, "head": 0, "pool": 0}
    for key, fn in (("layer", "gcn_layer"), ("head", "gcn_layer_head"), ("pool", "gcn_layer_pool")):
        orig = getattr(marl, fn)
        monkeypatch.setattr(gcn, fn, lambda *a, _o=orig, _k=key, **k: (calls.__setitem__(_k, calls[_k] + 1), _o(*a, **k))[1])
    with torch.no_grad():
        f32 = actor(mod_in)
        ref = copy.deepcopy(actor).double()([t.double() for t in mod_in])
        plain = marl.actor_infer(lib, actor, ins, nbr=nbr, nbr_p=nbr_p)
        assert calls == {"layer": 13, "head": 0, "pool": 0}
        calls.update(layer=0)
        got = marl.actor_infer(lib, actor, ins, nbr=nbr, nbr_p=nbr_p, fused=True)
        assert calls == {"layer": 8, "head": 2, "pool": 1}
    for g, f, y, p in zip(got, f32, ref, plain):
        e_kernel, e_module = float((g.double() - y).abs().max()), float((f.double() - y).abs().max())
        print(f"\n[fused actor] P {P}: max error {e_kernel:.3g}, float32 module {e_module:.3g}, against the layer path {float((g - p).abs().max()):.3g}")
        assert e_kernel <= 4.0 * e_module, f"actor_infer(fused) max error {e_kernel:.3g} against the float32 module's {e_module:.3g}"
        assert float((g - p).abs().max()) <= 2e-5
        torch.testing.assert_close(g, p, rtol=2e-5, atol=2e-6)


def _engine(lib, device, B=6, num_x=4, seed=3, hidden=16, lr=M.lr, **engine_kw):
    topo = tm.TrussTopology.grid(num_x)
    torch.manual_seed(seed)
    rl = RL.MADDPG(lr, M.ep, M.epd, M.gamma, hidden, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)
    eng = marl.BatchedMARL(topo, B, rl, max_front=6, lib=lib, device=device, replay_capacity=256, batch_size=8, seed=seed, **engine_kw)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng


@pytest.mark.gpu
def test_fused_actor_infer_follows_replayed_updates():
    """after four hipGraph-replayed updates at lr 1e-3 (hidden width 40: bf16x3 hidden layers with cached split weights; the heads
    read lin.weight itself), actor_infer(fused=True) equals the module on its CURRENT weights to 2e-5, on replay states; the
    weights from before training give outputs far outside that tolerance"""
    lib = tm.load()
    with contextlib.redirect_stdout(io.StringIO()):
        eng = _engine(lib, "cuda", B=64, seed=5, hidden=40, lr=1e-3, actor_path="fused")
        eng.game_step_all(train=True, explore=True, train_iters=1)           # materialises every lazy layer, first update
        before = [copy.deepcopy(ag.actor_model) for ag in eng.rl.agents]
        for _ in range(4):
            eng.game_step_all(train=True, explore=True, train_iters=2)
    assert eng.use_train_graph and eng._tg is not None
    S = eng.replay.sample(16, eng.gen)[0]
    ins = [S["x_n"], eng.A_n[0], S["A_s"], S["A_n_ts"], S["A_n_cs"], S["x_p"], S["A_p"]]
    mod_in = [S["x_n"], eng.A_n.expand(16, -1, -1)] + ins[2:]
    for ag, old in zip(eng.rl.agents, before):
        with torch.no_grad():
            got = marl.actor_infer(lib, ag.actor_model, ins, nbr=eng.nbr, nbr_p=eng.nbr_p, fused=True)
            ref, stale = ag.actor_model(mod_in), old(mod_in)
        for g, r, st in zip(got, ref, stale):
            torch.testing.assert_close(g, r, rtol=2e-5, atol=2e-6)
            assert float((st - r).abs().max()) > 20 * (2e-6 + 2e-5 * float(r.abs().max())), "training did not move the outputs"


@pytest.mark.gpu
def test_engines_differ_only_in_actor_path():
    """two engines, 16-node class, 8 envs, exploration off, three game steps.  First step: every archive holds the reset design, the
    runs have not branched, and the action tensors of the two paths agree to 2e-5.  Later steps may part ways (decoding rounds
    heights to a 0.01 grid and sections to +-1): front sizes in range, rewards finite, status clean."""
    lib = tm.load()
    acts, engines = {}, {}
    for path in ("layers", "fused"):
        with contextlib.redirect_stdout(io.StringIO()):
            eng = _engine(lib, "cuda", B=8, num_x=8, seed=7, actor_path=path)
        assert eng.actor_path == path
        seen = []
        orig = eng._act
        eng._act = lambda S, explore, _o=orig, _s=seen: (_s.append(_o(S, explore)), _s[-1])[1]
        with contextlib.redirect_stdout(io.StringIO()):
            stats = [eng.game_step_all(train=False, explore=False) for _ in range(3)]
        acts[path], engines[path] = seen, eng
        for s in stats:
            assert bool(((s["n_front"] >= 1) & (s["n_front"] <= eng.P)).all())
            assert torch.isfinite(s["reward"]).all() and torch.isfinite(s["hv"]).all()
        assert int(eng.envP.status.sum()) == 0 and int(eng.envC.status.sum()) == 0
        assert 1 <= int(eng.n.min()) and int(eng.n.max()) <= eng.P
    (geo_l, topo_l), (geo_f, topo_f) = acts["layers"][0], acts["fused"][0]
    for a, b in zip(geo_l + topo_l, geo_f + topo_f):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 2e-5
