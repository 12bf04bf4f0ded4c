"""The split-weight GCN layer on one or two bf16 terms per operand (truss_gcn_layer_terms, csrc/truss_gcn.h; precisions "bf16x2" and
"bf16" of marl.gcn_layer / gcn_layer_head / gcn_layer_pool / actor_infer and BatchedMARL(actor_precision=...)).

Two bounds, both elementwise against float64 and both derived, not measured (T = bf16 terms per operand):

    loose   |got - ref64| <= (tau_T + 1e-6) * Mag        tau_2 = 2^-13, tau_1 = 2^-6, Mag = |A| (|X| |W|^T) + |b| (+ |out0|)
            truncation to T terms leaves |a - sum_{t<T} a_t| < 2^(1-8T) |a|; for T = 2 the dropped a1 w1 is below 2^-14 and the two
            remainders below 2^-15 each; 1e-6 is the project's bound for the float32 accumulation (gcn_reference.TAU["bf16x3"])
    tight   |got - act(bf16x3_pre(x, adj, w, products_T) + b)| <= 1e-6 * Mag      on inputs whose X' = A X is exact in float32
            products_1 = ("00",), products_2 = ("00", "01", "10"): the host model of the kernel's own arithmetic

The loose bound cannot tell T = 2 from T = 3; the tight one can: on the exact inputs of every GPU case the host models of the other
two T lie outside it (test_bounds_have_teeth, no GPU needed).

Measured on an MI355X: see the docstrings of the GPU tests (raw output: profiles/r10/terms_tests.txt)."""
import contextlib
import copy
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import gcn, marl, ops
import parity_common as pc
import gcn_reference as G
import test_actor_fused as F
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL

TAU32 = G.TAU["bf16x3"]                                      # float32 accumulation of the MFMAs
TAU_T = {1: 2.0 ** -6, 2: 2.0 ** -13, 3: 0.0}                # what truncation to T terms adds
PRODUCTS = {1: ("00",), 2: ("00", "01", "10"), 3: ("00", "01", "10", "02", "11", "20")}
PRECISION = {1: "bf16", 2: "bf16x2", 3: "bf16x3"}

# name: (graph, B, k_in, c_out, act, accumulate, random inputs: one adjacency per graph)
LAYER_CASES = {
    "16 nodes, 9 graphs": ("grid8", 9, 200, 200, "relu", True, False),        # two workgroups, the second ragged (one graph)
    "12 nodes, 21 graphs": ("grid6", 21, 200, 200, None, False, True),        # tiles of 120 live rows
    "24 nodes, 9 terms": ("rand24", 6, 200, 200, "relu", False, True),        # KT = 9
    "path 20": ("path20", 13, 48, 200, "relu", False, True),                  # three slabs
    "path 50": ("path50", 5, 32, 200, "sigmoid", False, True),                # two slabs
    "dense 7": ("dense7", 40, 4, 200, "relu", False, True),                   # no table
    "136 nodes": ("grid68", 2, 200, 200, "relu", True, True),                 # NW = 8: 2 / 1 LDS-DMA instructions per wave
    "256 nodes": ("grid128", 2, 200, 200, "sigmoid", False, False),
    "k_in 16": ("grid8", 5, 16, 200, "relu", False, True),                    # one slab: prologue only
    "k_in 32": ("grid8", 5, 32, 200, None, False, True),                      # two slabs
    "k_in 48": ("grid8", 5, 48, 200, "relu", False, False),                   # three: the first full turn of the double buffers
    "c_out 33": ("grid8", 5, 200, 33, "relu", False, True),
    "c_out 224": ("grid8", 5, 200, 224, None, True, True),
}


def _quarters(g, B, N, tab):
    """adjacency entries from {0, 1/4, 1/2, 1} on the pattern, one matrix per graph; the diagonal from {1/4, 1/2, 1}, so that no
    row's Mag shrinks to |b| alone"""
    vals = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, N, N), generator=g)]
    idx = torch.arange(N)
    vals[:, idx, idx] = torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (B, N), generator=g)]
    return vals * torch.tensor(F._pattern(tab)) if tab is not None else vals


@functools.lru_cache(maxsize=None)
def layer_case(name, kind):
    """host inputs (float32), float64 reference, Mag and the host models of T = 1, 2, 3 of a layer case; kind "exact": x multiples of
    2^-6 in [-4, 4) and adjacency entries from {0, 1/4, 1/2, 1}, so that X' = A X is exact in float32 in any order (asserted);
    "random": normal x, the truss's normalised adjacency or random entries on the pattern.  The exact inputs of a sigmoid case run
    without the activation: a sigmoid is 1/4-Lipschitz and saturates, so it would hide the 3e-6 Mag by which the pre-activations of
    neighbouring T differ below the 1e-6 Mag of the tight bound -- that check needs the pre-activation.  Computed once per session."""
    graph, B, K, C, act, acc, per_env = LAYER_CASES[name]
    if kind == "exact" and act == "sigmoid":
        act = None
    g = torch.Generator(device="cpu").manual_seed(sorted(LAYER_CASES).index(name) * 2 + 300 + (kind == "exact"))
    N, tab, _, shared = F._graph(graph)
    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == "exact":
        x = torch.randint(-256, 256, (B, N, K), generator=g).float() / 64.0
        adj = _quarters(g, B, N, tab)
    else:
        x = rn(B, N, K)
        adj = F._adjacency(g, B, N, tab, shared, per_env or shared is None)
    c = dict(x=x, adj=adj, w=rn(C, K) / K ** 0.5, b=rn(C), act=act, out0=rn(B, N, C) if acc else None,
             nbr=torch.tensor(tab) if tab is not None else None)
    if kind == "exact":
        A, X = G.dense_adj(adj, B, N), G.f64(x)
        assert np.array_equal(G._aggregate32(x, adj).astype(np.float64), A @ X), f"{name}: X' = A X is not exact in float32"
    c["ref"], c["mag"] = G.layer_ref(x, adj, c["w"], c["b"], act, c["out0"])
    o = G.f64(c["out0"]) if acc else 0.0
    c["model"] = {T: G.act64(G.bf16x3_pre(x, adj, c["w"], PRODUCTS[T]) + G.f64(c["b"]), act) + o for T in (1, 2, 3)}
    return c


def _run_layer(lib, c, precision, device="cuda", out=None):
    x, adj, w, b, nbr, out0 = F._on(c, device, "x", "adj", "w", "b", "nbr", "out0")
    if out is None and out0 is not None:
        out = out0.clone()
    return marl.gcn_layer(lib, x, adj, w, b, c["act"], nbr, out, out0 is not None, precision=precision)


# ---- teeth, without a GPU -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_bounds_have_teeth(name):
    """on the inputs of the GPU case: the host model of T (rounded to float32) satisfies the loose bound on both kinds of input and
    the tight bound on the exact ones; the models of the other two T violate the tight bound; the host mutants that apply (last K
    slab left out, diagonal term left out) violate the loose bound -- for T = 1 only where the mutant is further than
    (2^-6 + 1e-6) Mag from float64 somewhere at all, otherwise it is passed over by name (at most one per case)"""
    for kind in ("exact", "random"):
        c = layer_case(name, kind)
        ref, mag = c["ref"], c["mag"]
        muts = {k: v for k, v in G.mutants(c["x"], c["adj"], c["w"], c["b"], c["act"], c["out0"]).items()
                if k in ("last K slab left out", "diagonal term left out")}
        assert len(muts) == 2
        for T in (1, 2):
            model32 = c["model"][T].astype(np.float32)
            r = G.max_ratio(model32, ref, mag)
            assert r <= TAU_T[T] + TAU32, f"{name} {kind} T {T}: host model at {r:.3g} * Mag of float64"
            if kind == "exact":
                assert G.within(model32, c["model"][T], mag, TAU32)
                for other in (1, 2, 3):
                    if other != T:
                        ro = G.max_ratio(c["model"][other], c["model"][T], mag)
                        assert ro > TAU32, f"{name} T {T}: the model of T {other} passes the tight bound ({ro:.3g} * Mag)"
            passed_over = []
            for mname, m in muts.items():
                if T == 1 and G.within(m, ref, mag, TAU_T[1] + TAU32):
                    passed_over.append(mname)                  # closer than the one-term bound everywhere: nothing to tell apart
                    continue
                assert not G.within(m, ref, mag, TAU_T[T] + TAU32), f"{name} {kind} T {T}: mutant '{mname}' passes the loose bound"
            assert len(passed_over) <= 1, f"{name} {kind}: mutants passed over for T = 1: {passed_over}"
            if passed_over:
                print(f"\n[terms teeth] {name} {kind}: T = 1 cannot see mutant '{passed_over[0]}'")


# ---- refusals without the entry --------------------------------------------------------------------------------------------------

def _emu_engine(**kw):
    topo = tm.TrussTopology.grid(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 16, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    return marl.BatchedMARL(topo, 2, rl, max_front=6, lib=pc.emu_lib(), device="cpu", replay_capacity=64, batch_size=8, **kw)


def test_emulator_lacks_the_entry_and_the_engine_refuses_it(monkeypatch):
    """the CPU lane emulator does not export truss_gcn_layer_terms: the operator names the symbol, and so does
    BatchedMARL(actor_precision="bf16x2" / "bf16") at construction; an unknown precision is refused by the engine, by actor_infer
    and by the layer wrappers; TRUSS_ACTOR_PRECISION is honoured; the default engine reports "bf16x3" """
    lib = pc.emu_lib()
    assert not lib.has_gcn_terms and "truss_gcn_layer_terms" in ops.entries()
    t = lambda *s: torch.zeros(*s)
    with pytest.raises(tm.TrussError, match=r"has no truss_gcn_layer_terms$"):
        ops.call(ops.namespace().gcn_layer_terms, ops.bind(lib), 0, t(1, 2, 4), t(2, 2), None, t(40, 4), None, t(1, 2, 40), 1,
                 torch.zeros(3, 224, 16, dtype=torch.int16), 0, None, None, None, None, 0, None, None, False, 2)
    with pytest.raises(tm.TrussError, match=r"has no truss_gcn_layer_terms$"):
        marl.gcn_layer(lib, t(1, 2, 4), t(2, 2), t(40, 4), None, "relu", precision="bf16")
    for precision in ("bf16x2", "bf16"):
        with pytest.raises(ValueError, match="has no truss_gcn_layer_terms"):
            _emu_engine(actor_precision=precision)
    with pytest.raises(ValueError, match="actor_precision must be"):
        _emu_engine(actor_precision="fp8")
    with pytest.raises(ValueError, match="precision must be"):
        marl.gcn_layer(lib, t(1, 2, 4), t(2, 2), t(40, 4), None, "relu", precision="bf16x4")
    with pytest.raises(ValueError, match="precision must be"):
        marl.actor_infer(lib, None, [None] * 7, precision="half")
    assert _emu_engine().actor_precision == "bf16x3"
    assert _emu_engine(actor_precision="f32").actor_precision == "f32"
    monkeypatch.setenv("TRUSS_ACTOR_PRECISION", "f32")
    assert _emu_engine().actor_precision == "f32"
    assert _emu_engine(actor_precision="bf16x3").actor_precision == "bf16x3"
    monkeypatch.setenv("TRUSS_ACTOR_PRECISION", "bf16x2")
    with pytest.raises(ValueError, match="has no truss_gcn_layer_terms"):
        _emu_engine()
    monkeypatch.setenv("TRUSS_ACTOR_PRECISION", "bf15")
    with pytest.raises(ValueError, match="actor_precision must be"):
        _emu_engine()


def test_operator_meta_registration():
    ns = ops.namespace()
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    ns.gcn_layer_terms(0, 0, m(2, 16, 200), m(16, 16), None, m(200, 200), m(200), m(2, 16, 200), 1, m(3, 224, 208, dt=torch.int16), 0,
                       None, None, None, None, 0, None, None, True, 2)


# ---- the kernels against float64 and against the model of their own arithmetic ----------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layer_terms_float64_hip(name, T):
    """truss_gcn_layer_terms through marl.gcn_layer(precision="bf16x2" / "bf16"): the tight bound on the exact inputs, the loose
    bound on both kinds.

    Measured on an MI355X over the 13 cases, max |got - ref64| / Mag: two terms 3.3e-5 (exact inputs) / 4.8e-5 (random) against the
    bound 1.23e-4, one term 8.4e-3 / 8.2e-3 against 1.56e-2; exact inputs, max |got - model_T| / Mag: 8.6e-8 / 6.5e-8 against 1e-6
    (on the random inputs, where it is not asserted: 1.8e-5 / 2.2e-5).  Mean signed (got - ref64) / Mag of a case, the truncation
    bias: -1.4e-6 ... 2e-8 with two terms, -5.2e-4 ... 5e-6 with one."""
    lib = tm.load()
    assert lib.has_gcn_terms
    for kind in ("exact", "random"):
        c = layer_case(name, kind)
        got = _run_layer(lib, c, PRECISION[T])
        loose = G.max_ratio(got, c["ref"], c["mag"])
        tight = G.max_ratio(got, c["model"][T], c["mag"])
        bias = float(((G.f64(got) - c["ref"]) / np.where(c["mag"] > 0, c["mag"], 1.0)).mean())
        print(f"\n[terms layer] {name} T {T} {kind}: max |got - ref64| / Mag = {loose:.3g} (bound {TAU_T[T] + TAU32:.3g}), "
              f"max |got - model_T| / Mag = {tight:.3g}, mean (got - ref64) / Mag = {bias:.3g}")
        assert loose <= TAU_T[T] + TAU32, f"{name} T {T} {kind}: {loose:.3g} * Mag from float64"
        if kind == "exact":
            assert tight <= TAU32, f"{name} T {T}: {tight:.3g} * Mag from the host model of T terms"


class _LayerArgs(ctypes.Structure):          # truss_gcn_layer_args_t (include/truss_mi355.h)
    _fields_ = F._LayerArgs._fields_


class _EpiArgs(ctypes.Structure):            # truss_gcn_epilogue_t
    _fields_ = F._EpiArgs._fields_


def _terms_op(lib, x, adj, nbr, w, b, out, act, ws, terms, accumulate=False, kind=0, w2=None, b2=None, adj2=None, nbr2=None, act2=0,
              out2=None, pool=None):
    ops.call(ops.namespace().gcn_layer_terms, ops.bind(lib), ops.stream_of(x.device), x, adj, nbr, w, b, out, act, ws, kind, w2, b2,
             adj2, nbr2, act2, out2, pool, accumulate, terms)


@pytest.mark.gpu
def test_three_terms_are_the_existing_entries():
    """bf16_terms = 3 through the new entry: torch.equal to truss_gcn_layer with the same split weights (plain and accumulating), and
    to truss_gcn_layer_fused for a head and a pool case"""
    lib = tm.load()
    code = {None: 0, "relu": 1, "sigmoid": 2}
    for name in ("16 nodes, 9 graphs", "24 nodes, 9 terms", "256 nodes", "c_out 33"):
        c = layer_case(name, "random")
        x, adj, w, b, nbr, out0 = F._on(c, "cuda", "x", "adj", "w", "b", "nbr", "out0")
        ws = marl.split_weights(lib, w)
        want = marl.gcn_layer(lib, x, adj, w, b, c["act"], nbr, out0.clone() if out0 is not None else None, out0 is not None, w_split=ws)
        got = out0.clone() if out0 is not None else torch.full_like(want, float("nan"))
        _terms_op(lib, x, adj, nbr, w, b, got, code[c["act"]], ws, 3, accumulate=out0 is not None)
        assert torch.equal(got, want), name
    for name in ("16 nodes", "256 nodes"):
        c = F.head_case(name)
        x, adj, w, b, w2, b2, adj2, nbr, nbr2 = F._on(c, "cuda", "x", "adj", "w", "b", "w2", "b2", "adj2", "nbr", "nbr2")
        ws = marl.split_weights(lib, w)
        want = marl.gcn_layer_head(lib, x, adj, w, b, "relu", w2, b2, adj2, c["act2"], nbr, nbr2, w_split=ws)
        got = torch.full_like(want, float("nan"))
        _terms_op(lib, x, adj, nbr, w, b, None, 1, ws, 3, kind=1, w2=w2, b2=b2, adj2=adj2, nbr2=nbr2, act2=code[c["act2"]], out2=got)
        assert torch.equal(got, want), name
    c = F.pool_case("256 nodes")
    x, adj, w, b, nbr = F._on(c, "cuda", "x", "adj", "w", "b", "nbr")
    ws = marl.split_weights(lib, w)
    want = marl.gcn_layer_pool(lib, x, adj, w, b, "relu", nbr, w_split=ws)
    got = torch.full_like(want, float("nan"))
    _terms_op(lib, x, adj, nbr, w, b, None, 1, ws, 3, kind=2, pool=got)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_terms_are_reproducible_stay_in_bounds_and_refuse_cleanly():
    """two calls give equal bits; outputs pre-filled with NaN between poisoned guard bands come back fully written with the poison
    intact; after every refused call (terms 0 and 4, NULL split weights, c_out 32, k_in 18, a 10-term table) the poisoned outputs
    are unchanged and the library's code is the contract's; n_batch == 0 is a no-op"""
    lib = tm.load()
    for name in ("16 nodes, 9 graphs", "12 nodes, 21 graphs", "24 nodes, 9 terms", "136 nodes", "k_in 16", "c_out 33"):
        c = layer_case(name, "random")
        acc = c["out0"] is not None
        for T in (1, 2):
            res = []
            for _ in range(2):
                o = F.Guarded(tuple(c["ref"].shape), "cuda")
                if acc:
                    o.t.copy_(c["out0"])
                _run_layer(lib, c, PRECISION[T], out=o.t)
                assert o.intact() and not bool(torch.isnan(o.t).any()), f"{name} T {T}"
                res.append(o.t)
            assert torch.equal(res[0], res[1]), f"{name} T {T}"
    for name, T in (("16 nodes", 2), ("256 nodes", 1)):
        c = F.head_case(name)
        x, adj, w, b, w2, b2, adj2, nbr, nbr2 = F._on(c, "cuda", "x", "adj", "w", "b", "w2", "b2", "adj2", "nbr", "nbr2")
        res = []
        for _ in range(2):
            o2 = F.Guarded((x.shape[0], x.shape[1], w2.shape[0]), "cuda")
            gcn._gcn_layer_fused(lib, x, adj, w, b, "relu", nbr, PRECISION[T], None, None, 1, w2, b2, adj2, nbr2, c["act2"], out2=o2.t)
            assert o2.intact() and not bool(torch.isnan(o2.t).any()), f"head {name} T {T}"
            res.append(o2.t)
        assert torch.equal(res[0], res[1])
    c = F.pool_case("256 nodes")
    x, adj, w, b, nbr = F._on(c, "cuda", "x", "adj", "w", "b", "nbr")
    res = []
    for _ in range(2):
        p = F.Guarded((x.shape[0], w.shape[0]), "cuda")
        gcn._gcn_layer_fused(lib, x, adj, w, b, "relu", nbr, "bf16x2", None, None, 2, pool=p.t)
        assert p.intact() and not bool(torch.isnan(p.t).any())
        res.append(p.t)
    assert torch.equal(res[0], res[1])

    # refusals, through the C entry itself
    dev = "cuda"
    B, N, K, C = 2, 8, 16, 40
    tab = torch.tensor(marl.path_graph_table(N), device=dev)
    tab10 = torch.tensor(F._random_pattern(24, 10, 3), device=dev)
    x, adj, w, b = torch.ones(B * 24 * 20, device=dev), torch.ones(24 * 24, device=dev), torch.ones(C, 20, device=dev), torch.ones(C, device=dev)
    ws = torch.zeros(3, 224, 32, dtype=torch.int16, device=dev)
    out, pool = F.Guarded((B, 24, C), dev), F.Guarded((B, C), dev)
    out.t.fill_(7.0), pool.t.fill_(7.0)
    st = ops.stream_of(torch.device(dev))

    def layer(**kw):
        a = dict(struct_size=ctypes.sizeof(_LayerArgs), n_batch=B, n_nodes=N, k_in=K, c_out=C, act=1, x=x.data_ptr(), adj=adj.data_ptr(),
                 nbr=tab.data_ptr(), k_nbr=3, w=w.data_ptr(), bias=b.data_ptr(), out=out.t.data_ptr(), w_bf16x3=ws.data_ptr())
        a.update(kw)
        return _LayerArgs(**a)

    def call(la, terms, ep=None):
        return lib.check(lib.dll.truss_gcn_layer_terms(ctypes.byref(la), ctypes.byref(ep) if ep is not None else None, terms, st),
                         "truss_gcn_layer_terms")

    pooled = _EpiArgs(struct_size=ctypes.sizeof(_EpiArgs), kind=2, pool=pool.t.data_ptr())
    EINVAL, EUNSUP = r"failed \(-1\)", r"failed \(-2\)"
    refused = [(layer(), 0, None, EINVAL), (layer(), 4, None, EINVAL), (layer(), -1, pooled, EINVAL), (layer(w_bf16x3=None), 2, None, EINVAL),
               (layer(w_bf16x3=None, out=None), 1, pooled, EINVAL), (layer(c_out=32), 2, None, EUNSUP), (layer(k_in=18), 1, None, EUNSUP),
               (layer(n_nodes=24, nbr=tab10.data_ptr(), k_nbr=10), 2, None, EUNSUP), (layer(c_out=32, out=None), 2, pooled, EUNSUP),
               (layer(act=3), 2, None, EINVAL), (layer(accumulate=1), 2, pooled, EINVAL), (layer(struct_size=8), 2, None, EINVAL)]
    for la, terms, ep, code in refused:
        with pytest.raises(tm.TrussError, match=code):
            call(la, terms, ep)
    assert call(layer(n_batch=0), 2) == 0 and call(layer(n_batch=0, out=None), 1, pooled) == 0
    torch.cuda.synchronize()
    for gd in (out, pool):
        assert gd.intact() and torch.equal(gd.t, torch.full_like(gd.t, 7.0))
    assert call(layer(), 2) == 0                              # the same block, unrefused, does write
    torch.cuda.synchronize()
    flat = out.t.reshape(-1)                                  # relu(0 + bias) = 1 on the B * N rows of the block, nothing behind them
    assert out.intact() and bool((flat[:B * N * C] == 1.0).all()) and bool((flat[B * N * C:] == 7.0).all())


# ---- fused epilogues ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pool16():
    """a pool case at 16 nodes (test_actor_fused has none): 9 graphs, k_in 200, one adjacency per graph"""
    g = torch.Generator(device="cpu").manual_seed(416)
    N, tab, _, _ = F._graph("grid8")
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=rn(9, N, 200), w=rn(200, 200) / 200 ** 0.5, b=rn(200), adj=F._adjacency(g, 9, N, tab, None, True), nbr=torch.tensor(tab))


def _head_bound(x, adj, w, b, w2, b2, adj2, act2, tau):
    """(float64 reference, elementwise bound) of a head epilogue on these inputs: tau on the hidden layer's Mag1, 1e-6 on the head's
    own float32 product"""
    B, N, _ = x.shape
    V, mag1 = G.layer_ref(x, adj, w, b, "relu")
    A2, W2, bb2 = G.dense_adj(adj2, B, N), G.f64(w2), G.f64(b2)
    ref = G.act64(A2 @ (V @ W2.T) + bb2, act2)
    return ref, np.abs(A2) @ ((tau * mag1 + TAU32 * np.abs(V)) @ np.abs(W2).T) + TAU32 * np.abs(bb2)


def _pool_bound(x, adj, w, b, tau):
    V, mag1 = G.layer_ref(x, adj, w, b, "relu")
    return V.sum(axis=1), tau * mag1.sum(axis=1) + x.shape[1] * 2.0 ** -24 * np.abs(V).sum(axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2])
def test_fused_terms_float64_hip(T):
    """head and pool epilogues on T < 3 terms, at 16 and at 256 nodes: the composite bounds of test_actor_fused with tau_T + 1e-6 on the
    hidden layer's Mag1 and 1e-6 on the head's own float32 product; the host model of the fused arithmetic is inside them.

    Measured on an MI355X, max |got - ref64| / bound: head 16 / 256 nodes 2.2e-3 / 3.2e-4 (two terms), 4.4e-3 / 6.2e-4 (one term);
    pool 2.0e-2 / 6.6e-3 (two terms), 3.4e-2 / 1.4e-2 (one term)."""
    lib = tm.load()
    tau = TAU_T[T] + TAU32
    for name in ("16 nodes", "256 nodes"):
        c = F.head_case(name)
        ref, bound = _head_bound(c["x"], c["adj"], c["w"], c["b"], c["w2"], c["b2"], c["adj2"], c["act2"], tau)
        V32 = np.maximum(G.bf16x3_pre(c["x"], c["adj"], c["w"], PRODUCTS[T]) + G.f64(c["b"]), 0.0).astype(np.float32)
        A2 = G.dense_adj(c["adj2"], *c["x"].shape[:2]).astype(np.float32)
        model = G.act64((A2 @ (V32 @ c["w2"].numpy().T) + c["b2"].numpy()).astype(np.float32), c["act2"])
        assert F._ratio(model, ref, bound) <= 1.0
        x, adj, w, b, w2, b2, adj2, nbr, nbr2 = F._on(c, "cuda", "x", "adj", "w", "b", "w2", "b2", "adj2", "nbr", "nbr2")
        got = marl.gcn_layer_head(lib, x, adj, w, b, "relu", w2, b2, adj2, c["act2"], nbr, nbr2, precision=PRECISION[T])
        r = F._ratio(got, ref, bound)
        print(f"\n[terms head] {name} T {T}: max |got - ref64| / bound = {r:.3g}, against the model of T terms {float(np.abs(G.f64(got) - model).max()):.3g}")
        assert r <= 1.0, f"head {name} T {T}: {r:.3g} of the bound"
    for name, c in (("16 nodes", _pool16()), ("256 nodes", F.pool_case("256 nodes"))):
        ref, bound = _pool_bound(c["x"], c["adj"], c["w"], c["b"], tau)
        x, adj, w, b, nbr = F._on(c, "cuda", "x", "adj", "w", "b", "nbr")
        got = marl.gcn_layer_pool(lib, x, adj, w, b, "relu", nbr, precision=PRECISION[T])
        r = F._ratio(got, ref, bound)
        print(f"\n[terms pool] {name} T {T}: max |got - ref64| / bound = {r:.3g}")
        assert r <= 1.0, f"pool {name} T {T}: {r:.3g} of the bound"


# ---- the actor end to end ----------------------------------------------------------------------------------------------------------

def _actor_inputs(device="cuda", B=37, P=20):
    """the inputs of test_actor_fused.test_actor_infer_fused_float64_hip"""
    torch.manual_seed(9)
    topo = tm.TrussTopology.grid(8)
    N, tab = topo.N, topo.neighbor_table()
    patt = torch.tensor(F._pattern(tab), device=device)
    actor = RL.multimodes_actor(200, 2, 3).to(device)
    r = lambda *s: torch.rand(*s, device=device)
    pts = torch.rand(B, P, 4, dtype=torch.float64, device=device)
    x_p, A_p = marl.pareto_graph(pts, torch.randint(1, P + 1, (B,), device=device), torch.zeros(B, dtype=torch.long, device=device), P)
    A_n = torch.tensor(topo.normalized_adjacency()[0], device=device)
    ins = [r(B, N, 13), A_n, r(B, N, N) * patt, r(B, N, N) * patt, r(B, N, N) * patt, x_p, A_p]
    mod_in = [ins[0], A_n[None].expand(B, -1, -1)] + ins[2:]
    return actor, ins, mod_in, torch.tensor(tab, device=device), torch.tensor(marl.path_graph_table(P), device=device)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2])
def test_actor_infer_precision_hip(T, monkeypatch):
    """actor_infer(precision="bf16x2" / "bf16"), fused and not, on the inputs of test_actor_infer_fused_float64_hip (37 pairs, 16
    nodes, P = 20): EVERY layer call is held to its bound on the inputs that call received -- tau_T + 1e-6 where the bf16 envelope
    applies (the hidden layers), 1e-6 for the heads, the composite bounds for the fused head / pool calls; 13, or 8 + 2 + 1
    launches; precision="bf16x3" is torch.equal to a call without the argument; the sigmoid outputs are finite and in [0, 1].

    Measured on an MI355X, max deviation of the two action tensors (geometry / topology) from the float64 module, the same with
    fused and without (a measurement, not an assertion; the engine test below caps it): two terms 1.5e-5 / 2.1e-5 (mean signed
    -6.4e-6 / -3.5e-6), one term 3.6e-3 / 4.6e-3 (mean signed -1.7e-3 / -9.0e-4).  Worst call against its bound: hidden layers
    6.2e-5 of Mag (bound 1.23e-4) / 1.1e-2 (bound 1.56e-2), float32 layers 2.6e-8 of Mag, head calls 5.2e-4 / 8.7e-4 and the pool
    call 0.38 / 0.56 of their composite bounds."""
    lib = tm.load()
    actor, ins, mod_in, nbr, nbr_p = _actor_inputs()
    tau_hidden = TAU_T[T] + TAU32
    calls = {"layer": 0, "head": 0, "pool": 0}
    worst = {"hidden": 0.0, "f32": 0.0, "head": 0.0, "pool": 0.0}
    orig = {fn: getattr(marl, fn) for fn in ("gcn_layer", "gcn_layer_head", "gcn_layer_pool")}

    def layer(lib_, x, adj, w, bias, act, nbr_=None, out=None, accumulate=False, precision="bf16x3", w_split=None):
        calls["layer"] += 1
        out0 = out.clone() if accumulate else None
        got = orig["gcn_layer"](lib_, x, adj, w, bias, act, nbr_, out, accumulate, precision=precision, w_split=w_split)
        ref, mag = G.layer_ref(x, adj, w, bias, act, out0)
        env = precision != "f32" and gcn._bf16_envelope(x, w, nbr_)
        r = G.max_ratio(got, ref, mag)
        key = "hidden" if env else "f32"
        worst[key] = max(worst[key], r)
        assert r <= (tau_hidden if env else TAU32), f"layer call {calls['layer']} ({key}, K {x.shape[2]} C {w.shape[0]}): {r:.3g} * Mag"
        return got

    def head(lib_, x, adj, w, bias, act, w2, bias2, adj2, act2, nbr_=None, nbr2=None, precision="bf16x3", w_split=None, out=None):
        calls["head"] += 1
        got = orig["gcn_layer_head"](lib_, x, adj, w, bias, act, w2, bias2, adj2, act2, nbr_, nbr2, precision=precision, w_split=w_split, out=out)
        assert act == "relu" and gcn._bf16_envelope(x, w, nbr_)
        ref, bound = _head_bound(x, adj, w, bias, w2, bias2, adj2, act2, tau_hidden)
        r = F._ratio(got, ref, bound)
        worst["head"] = max(worst["head"], r)
        assert r <= 1.0, f"head call: {r:.3g} of the bound"
        return got

    def pool(lib_, x, adj, w, bias, act, nbr_=None, precision="bf16x3", w_split=None, out=None):
        calls["pool"] += 1
        got = orig["gcn_layer_pool"](lib_, x, adj, w, bias, act, nbr_, precision=precision, w_split=w_split, out=out)
        assert act == "relu" and gcn._bf16_envelope(x, w, nbr_)
        ref, bound = _pool_bound(x, adj, w, bias, tau_hidden)
        r = F._ratio(got, ref, bound)
        worst["pool"] = max(worst["pool"], r)
        assert r <= 1.0, f"pool call: {r:.3g} of the bound"
        return got

    with torch.no_grad():
        actor(mod_in)                                          # (materialises the lazy layers before the copy is taken)
        ref64 = copy.deepcopy(actor).double()([t.double() for t in mod_in])
        base = marl.actor_infer(lib, actor, ins, nbr=nbr, nbr_p=nbr_p)
        base_fused = marl.actor_infer(lib, actor, ins, nbr=nbr, nbr_p=nbr_p, fused=True)
        for b, f in zip(base, marl.actor_infer(lib, actor, ins, nbr=nbr, nbr_p=nbr_p, precision="bf16x3")):
            assert torch.equal(b, f)
        for b, f in zip(base_fused, marl.actor_infer(lib, actor, ins, nbr=nbr, nbr_p=nbr_p, fused=True, precision="bf16x3")):
            assert torch.equal(b, f)
        monkeypatch.setattr(gcn, "gcn_layer", layer)
        monkeypatch.setattr(gcn, "gcn_layer_head", head)
        monkeypatch.setattr(gcn, "gcn_layer_pool", pool)
        for fused, want in ((False, {"layer": 13, "head": 0, "pool": 0}), (True, {"layer": 8, "head": 2, "pool": 1})):
            calls.update(layer=0, head=0, pool=0)
            got = marl.actor_infer(lib, actor, ins, nbr=nbr, nbr_p=nbr_p, fused=fused, precision=PRECISION[T])
            assert calls == want
            for g, y, b3, what in zip(got, ref64, base_fused if fused else base, ("geometry", "topology")):
                assert bool(torch.isfinite(g).all()) and float(g.min()) >= 0.0 and float(g.max()) <= 1.0
                print(f"\n[terms actor] T {T} fused {fused} {what}: max |got - float64 module| = {float((g.double() - y).abs().max()):.3g}, "
                      f"mean signed {float((g.double() - y).mean()):.3g}, against bf16x3 {float((g - b3).abs().max()):.3g}")
    print(f"\n[terms actor] T {T}: worst call / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f" (hidden and f32 as multiples of Mag: bounds {tau_hidden:.3g} and {TAU32:.3g})")


# ---- the engine ----------------------------------------------------------------------------------------------------------------------

ACTION_CAP = {"bf16": 0.05, "bf16x2": 1e-3}                   # sanity caps on sigmoid outputs in [0, 1], not accuracy claims


@pytest.mark.gpu
def test_engines_differ_only_in_actor_precision():
    """three game steps of an 8-env, 16-node engine per precision (hidden width 40: inside the split-weight envelope), exploration
    off: status clean, front sizes in range, rewards finite; first step (the runs have not branched): the actions of "bf16x2" /
    "bf16" are within 1e-3 / 0.05 of the "bf16x3" engine's -- and not equal to them: the reduced product did run; "bf16" also
    composes with actor_path="fused".

    Measured on an MI355X, first-step actions against the bf16x3 engine's: bf16x2 2.2e-5, bf16 4.7e-3 (layers and fused alike)."""
    lib = tm.load()
    acts = {}
    for precision, path in (("bf16x3", "layers"), ("bf16x2", "layers"), ("bf16", "layers"), ("bf16", "fused")):
        with contextlib.redirect_stdout(io.StringIO()):
            eng = F._engine(lib, "cuda", B=8, num_x=8, seed=7, hidden=40, actor_path=path, actor_precision=precision)
        assert eng.actor_precision == precision and eng.actor_path == path
        seen = []
        orig = eng._act
        eng._act = lambda S, explore, _o=orig, _s=seen: (_s.append(_o(S, explore)), _s[-1])[1]
        with contextlib.redirect_stdout(io.StringIO()):
            stats = [eng.game_step_all(train=False, explore=False) for _ in range(3)]
        acts[precision, path] = seen
        for s in stats:
            assert bool(((s["n_front"] >= 1) & (s["n_front"] <= eng.P)).all())
            assert torch.isfinite(s["reward"]).all() and torch.isfinite(s["hv"]).all()
        assert int(eng.envP.status.sum()) == 0 and int(eng.envC.status.sum()) == 0
        assert 1 <= int(eng.n.min()) and int(eng.n.max()) <= eng.P
    geo3, topo3 = acts["bf16x3", "layers"][0]
    for (precision, path), seen in acts.items():
        if precision == "bf16x3":
            continue
        geo, topo = seen[0]
        d = max(float((a - b).abs().max()) for a, b in zip(geo + topo, geo3 + topo3))
        print(f"\n[terms engine] {precision} ({path}): first-step actions within {d:.3g} of the bf16x3 engine's (cap {ACTION_CAP[precision]:g})")
        assert all(a.shape == b.shape for a, b in zip(geo + topo, geo3 + topo3)) and 0.0 < d <= ACTION_CAP[precision]
