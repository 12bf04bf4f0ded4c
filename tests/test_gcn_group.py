"""Several split-weight GCN layers in one launch (truss_gcn_layer_group, csrc/truss_gcn_group.h): the operator, the wrapper
marl.gcn_layer_group, marl.actors_infer and the engine switch BatchedMARL(actor_path="grouped").

The arithmetic of every output element is that of truss_gcn_layer_terms -- only which workgroup runs which layer, and in what
order, is new -- so the acceptance test is BITWISE equality (torch.equal) with the same layers run one by one through
marl.gcn_layer / gcn_layer_head / gcn_layer_pool in chain order; no tolerance is involved.  Equality of two code paths says nothing
about the baseline they share, so the accumulating case is also held against float64 with a derived bound (T = bf16 terms):

    |out - (out0 + sum_s ref_s)| <= (tau_T + 1e-6) (|out0| + sum_s Mag_s)      tau_3 = 0, tau_2 = 2^-13, tau_1 = 2^-6
    ref_s, Mag_s = gcn_reference.layer_ref of step s: act(A_s (X_s W_s^T) + b_s) and |A_s| (|X_s| |W_s|^T) + |b_s|

Step s on its own is within (tau_T + 1e-6) Mag_s of ref_s (test_gcn_terms.py derives tau_T from the truncation of both operands;
1e-6 is the project's bound for the float32 accumulation of the MFMAs).  Each of the S - 1 accumulating steps adds one float32
rounding of the running sum, at most 2^-24 (|out0| + sum_s Mag_s) each: 4 x 6e-8 of the right-hand side for the five steps, inside
what the 1e-6 leaves (the single layers measure 1e-7 of their Mag, tests/test_gcn_float64.py)."""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import marl, ops, synthetic
import parity_common as pc
import gcn_reference as G
import test_actor_fused as F
import test_gcn_terms as TT
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL

PRECISION = TT.PRECISION                                     # {1: "bf16", 2: "bf16x2", 3: "bf16x3"}
C_OUT = 200

# name: (graph, graphs B, chains, k_in of the steps of a chain, epilogue)
CASES = {
    "a: 3 x 5 accumulating": ("grid8", 9, 3, (200, 200, 200, 200, 200), None),      # two tiles, the second with one graph
    "a0: 3 x 5, step 0 accumulates": ("grid8", 9, 3, (200, 200, 200, 200, 200), None),
    "b: 9 x 1, k_in 16": ("grid8", 5, 9, (16,), None),                                  # one slab
    "b: 9 x 1, 12 nodes": ("grid6", 21, 9, (16,), None),                                # a graph's rows straddle waves
    "c: 2 x 3, k_in 32 48 200": ("grid8", 5, 2, (32, 48, 200), None),                   # two slabs, three slabs, the full loop
    "d: 2 x 2, 9 terms": ("rand24", 6, 2, (200, 200), None),                            # KT = 9
    "d: 2 x 2, 136 nodes": ("grid68", 2, 2, (200, 200), None),                          # NW = 8, one graph per tile
    "d: 2 x 1, dense 7": ("dense7", 40, 2, (4,), None),                                 # no table
    "e: 3 pools": ("path20", 13, 3, (48,), "pool"),
    "f: 6 heads": ("grid8", 9, 6, (200,), "head"),
}


@functools.lru_cache(maxsize=None)
def group_case(name):
    """host tensors of a case from a seeded generator: chains of step dicts (x, adj, w, b, act, accumulate), epilogue dicts, the
    pattern tables, and out0 where step 0 accumulates.  Steps 1 and 2 of a chain share x (as gcn_l2_2 / gcn_l2_3 do); adjacencies
    alternate between one for all graphs and one per graph."""
    graph, B, n_chains, ks, epi = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(sorted(CASES).index(name) + 700)
    N, tab, tab2, shared = F._graph(graph)
    rn = lambda *s: torch.randn(*s, generator=g)
    prefilled = name.startswith("a0")
    chains, epis = [], []
    for c in range(n_chains):
        chain = []
        for s, K in enumerate(ks):
            per_graph = (c + s) % 2 == 1 if epi is None else epi == "head"
            x = chain[1]["x"] if s == 2 and ks[1] == K else rn(B, N, K)
            chain.append(dict(x=x, adj=F._adjacency(g, B, N, tab, shared, per_graph or shared is None and tab is not None),
                              w=rn(C_OUT, K) / K ** 0.5, b=rn(C_OUT), act="relu", accumulate=s > 0 or prefilled))
        chains.append(chain)
        if epi == "head":
            c2 = 2 + c % 2
            epis.append(dict(w2=rn(c2, C_OUT) / C_OUT ** 0.5, b2=rn(c2), adj2=F._adjacency(g, B, N, tab2, shared, False), act2="sigmoid"))
    return dict(B=B, N=N, chains=chains, epis=epis, epi=epi, nbr=torch.tensor(tab) if tab is not None else None,
                nbr2=torch.tensor(tab2) if tab2 is not None else None,
                out0=[rn(B, N, C_OUT) for _ in range(n_chains)] if prefilled else None)


def _device_case(lib, name):
    """the case on the GPU, every layer with its split-weight image"""
    c = group_case(name)
    dev = lambda t: t.to("cuda") if t is not None else None
    memo = {}
    once = lambda t: memo.setdefault(id(t), dev(t))          # (a shared x stays one tensor)
    chains = [[dict(x=once(s["x"]), adj=dev(s["adj"]), w=dev(s["w"]), bias=dev(s["b"]), act=s["act"], accumulate=s["accumulate"],
                    nbr=dev(c["nbr"])) for s in chain] for chain in c["chains"]]
    for chain in chains:
        for s in chain:
            s["w_split"] = marl.split_weights(lib, s["w"])
    epis = [dict(w2=dev(e["w2"]), bias2=dev(e["b2"]), adj2=dev(e["adj2"]), act2=e["act2"], nbr2=dev(c["nbr2"])) for e in c["epis"]]
    return c, chains, epis


def _one_by_one(lib, c, chains, epis, T):
    """the layers through the single-layer wrappers, in chain order: per chain the output (out / out2 / pool)"""
    res = []
    for i, chain in enumerate(chains):
        if c["epi"] == "head":
            s, e = chain[0], epis[i]
            res.append(marl.gcn_layer_head(lib, s["x"], s["adj"], s["w"], s["bias"], s["act"], e["w2"], e["bias2"], e["adj2"], e["act2"],
                                           s["nbr"], e["nbr2"], precision=PRECISION[T], w_split=s["w_split"]))
        elif c["epi"] == "pool":
            s = chain[0]
            res.append(marl.gcn_layer_pool(lib, s["x"], s["adj"], s["w"], s["bias"], s["act"], s["nbr"], precision=PRECISION[T], w_split=s["w_split"]))
        else:
            out = c["out0"][i].to("cuda") if c["out0"] is not None else torch.full((c["B"], c["N"], C_OUT), float("nan"), device="cuda")
            for s in chain:
                marl.gcn_layer(lib, s["x"], s["adj"], s["w"], s["bias"], s["act"], s["nbr"], out, s["accumulate"], precision=PRECISION[T],
                               w_split=s["w_split"])
            res.append(out)
    return res


def _grouped(lib, c, chains, epis, T):
    """the same in one launch; outputs NaN-filled inside poisoned buffers (F.Guarded)"""
    B, N = c["B"], c["N"]
    guards, epilogues = [], None
    if c["epi"] == "head":
        guards = [F.Guarded((B, N, e["w2"].shape[0]), "cuda") for e in epis]
        epilogues = [dict(kind="head", out2=gd.t, **e) for gd, e in zip(guards, epis)]
    elif c["epi"] == "pool":
        guards = [F.Guarded((B, C_OUT), "cuda") for _ in chains]
        epilogues = [dict(kind="pool", pool=gd.t) for gd in guards]
    else:
        guards = [F.Guarded((B, N, C_OUT), "cuda") for _ in chains]
        if c["out0"] is not None:
            for gd, o in zip(guards, c["out0"]):
                gd.t.copy_(o)
    call = [[dict(s, out=None if c["epi"] else guards[i].t) for s in chain] for i, chain in enumerate(chains)]
    marl.gcn_layer_group(lib, call, PRECISION[T], epilogues)
    torch.cuda.synchronize()
    for gd in guards:
        assert gd.intact() and not bool(torch.isnan(gd.t).any())
    return [gd.t for gd in guards]


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------

def _emu_engine(**kw):
    topo = tm.TrussTopology.grid(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 16, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    return marl.BatchedMARL(topo, 2, rl, max_front=6, lib=pc.emu_lib(), device="cpu", replay_capacity=64, batch_size=8, **kw)


def _tiny_group_call(ns, lib_id, make):
    """one plain layer through the operator: x [1, 2, 4], 40 columns"""
    return (ns.gcn_layer_group, lib_id, 0, [make(1, 2, 4)], [make(2, 2)], [None], [make(40, 4)], [None], [make(1, 2, 40)], [1], [False],
            [make(3, 224, 16, dt=torch.int16)], 1, 0, [], [], [], [], [], [], [], 3)


def test_emulator_lacks_the_entry_and_the_engine_refuses_it(monkeypatch):
    """the CPU lane emulator does not export truss_gcn_layer_group: the library object says so, the operator and the wrapper name the
    symbol, BatchedMARL(actor_path="grouped") is refused at construction -- also when TRUSS_ACTOR asks for it -- and an unknown value
    still gets "actor_path must be" """
    lib = pc.emu_lib()
    assert lib.has_gcn_group is False and "truss_gcn_layer_group" in ops.entries()
    make = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    with pytest.raises(tm.TrussError, match=r"has no truss_gcn_layer_group$"):
        ops.call(*_tiny_group_call(ops.namespace(), ops.bind(lib), make))
    with pytest.raises(tm.TrussError, match=r"has no truss_gcn_layer_group$"):
        marl.gcn_layer_group(lib, [[dict(x=make(1, 2, 4), adj=make(2, 2), w=make(40, 4), bias=None, act="relu", out=make(1, 2, 40),
                                         w_split=make(3, 224, 16, dt=torch.int16))]])
    with pytest.raises(ValueError, match="precision must be"):
        marl.gcn_layer_group(lib, [], precision="f32")
    with pytest.raises(ValueError, match=r"actor_path='grouped': .* has no truss_gcn_layer_group"):
        _emu_engine(actor_path="grouped")
    with pytest.raises(ValueError, match="actor_path must be"):
        _emu_engine(actor_path="levels")
    assert _emu_engine().actor_path == "layers"
    monkeypatch.setenv("TRUSS_ACTOR", "grouped")
    with pytest.raises(ValueError, match=r"actor_path='grouped': .* has no truss_gcn_layer_group"):
        _emu_engine()
    assert _emu_engine(actor_path="layers").actor_path == "layers"


def test_operator_meta_registration():
    make = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    call = _tiny_group_call(ops.namespace(), 0, make)
    call[0](*call[1:])


# ---- the kernels -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3])
def test_group_equals_the_layers_one_by_one_hip(T):
    """every case of the table above: the group launch is torch.equal to the same layers through the single-layer wrappers in chain
    order; its outputs come back fully written with the guard bands intact; a second call gives the same bits.  The accumulating
    case "a" (and "a0", where step 0 adds onto a prefilled out) is also inside the float64 bound of the module docstring.

    Measured on an MI355X, max |out - sum ref| / sum Mag over the chains of "a" and "a0": 3.5e-8 with three terms (bound 1e-6),
    3.5e-6 with two (bound 1.23e-4), 8.7e-4 with one (bound 1.56e-2); raw output: profiles/r11/group_tests.txt."""
    lib = tm.load()
    assert lib.has_gcn_group
    for name in sorted(CASES):
        c, chains, epis = _device_case(lib, name)
        want = _one_by_one(lib, c, chains, epis, T)
        got = _grouped(lib, c, chains, epis, T)
        again = _grouped(lib, c, chains, epis, T)
        for i, (w, g, a) in enumerate(zip(want, got, again)):
            assert torch.equal(g, w), f"{name} T {T} chain {i}: {int((g != w).sum())} elements differ, max {float((g - w).abs().max()):.3g}"
            assert torch.equal(g, a), f"{name} T {T} chain {i}: two calls differ"
        if name.startswith("a"):
            for i, chain in enumerate(c["chains"]):
                parts = [G.layer_ref(s["x"], s["adj"], s["w"], s["b"], s["act"]) for s in chain]
                ref, mag = sum(p[0] for p in parts), sum(p[1] for p in parts)
                if c["out0"] is not None:
                    ref, mag = ref + G.f64(c["out0"][i]), mag + np.abs(G.f64(c["out0"][i]))
                r = G.max_ratio(got[i], ref, mag)
                print(f"\n[group float64] {name} T {T} chain {i}: max |out - sum ref| / sum Mag = {r:.3g} (bound {TT.TAU_T[T] + TT.TAU32:.3g})")
                assert r <= TT.TAU_T[T] + TT.TAU32, f"{name} T {T} chain {i}: {r:.3g} of sum Mag from float64"


@pytest.mark.gpu
def test_group_is_capturable_hip():
    """one group call captured in a torch.cuda.graph and replayed equals the eager call (the entry allocates nothing, copies nothing
    and does not synchronise: the descriptors travel in the kernel arguments)"""
    lib = tm.load()
    c, chains, epis = _device_case(lib, "a: 3 x 5 accumulating")
    eager = _grouped(lib, c, chains, epis, 3)
    outs = [torch.full((c["B"], c["N"], C_OUT), float("nan"), device="cuda") for _ in chains]
    call = [[dict(s, out=outs[i]) for s in chain] for i, chain in enumerate(chains)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        marl.gcn_layer_group(lib, call, "bf16x3")               # warm-up: the kernel's LDS opt-in happens outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        marl.gcn_layer_group(lib, call, "bf16x3")
    for o in outs:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert torch.equal(o, e)


@pytest.mark.gpu
def test_group_refusals_hip():
    """every rule of the entry's contract, through the C entry itself: the library's code, and afterwards every output still holds
    its prefill between intact guard bands; n_chains == 0 and n_batch == 0 return 0 without writing; the unrefused block writes"""
    lib = tm.load()
    dev = "cuda"
    B, N, K, C = 2, 24, 16, 40
    tab3 = torch.tensor(marl.path_graph_table(N), device=dev)
    tab9 = torch.tensor(F._random_pattern(N, 9, 1), device=dev)
    tab10 = torch.tensor(F._random_pattern(N, 10, 3), device=dev)
    x, adj = torch.ones(B * N * 20 + 64, device=dev), torch.ones(N * N, device=dev)
    w, b = torch.ones(C, 20, device=dev), torch.ones(C, device=dev)
    w2, b2 = torch.ones(3, C, device=dev), torch.ones(3, device=dev)
    ws = torch.zeros(3, 224, 32, dtype=torch.int16, device=dev)
    n_out = B * N * C
    outs = F.Guarded((20, B, N, C), dev)                       # out of layer i: outs.t[i]
    heads, pools = F.Guarded((9, B, N, 3), dev), F.Guarded((9, B, C), dev)
    for gd in (outs, heads, pools):
        gd.t.fill_(7.0)
    st = ops.stream_of(torch.device(dev))
    out_ptr = lambda i: outs.t[i].data_ptr()

    def layer(i, **kw):
        a = dict(struct_size=ctypes.sizeof(F._LayerArgs), n_batch=B, n_nodes=N, k_in=K, c_out=C, act=1, x=x.data_ptr(), adj=adj.data_ptr(),
                 nbr=tab3.data_ptr(), k_nbr=3, w=w.data_ptr(), bias=b.data_ptr(), out=out_ptr(i), w_bf16x3=ws.data_ptr())
        a.update(kw)
        return F._LayerArgs(**a)

    def head(i, **kw):
        a = dict(struct_size=ctypes.sizeof(F._EpiArgs), kind=1, w2=w2.data_ptr(), bias2=b2.data_ptr(), adj2=adj.data_ptr(), c2=3, act2=2,
                 out2=heads.t[i].data_ptr())
        a.update(kw)
        return F._EpiArgs(**a)

    def pooled(i, **kw):
        a = dict(struct_size=ctypes.sizeof(F._EpiArgs), kind=2, pool=pools.t[i].data_ptr())
        a.update(kw)
        return F._EpiArgs(**a)

    def call(layers, n_chains, steps, terms=2, epis=None):
        la = (F._LayerArgs * max(len(layers), 1))(*layers)
        ea = (F._EpiArgs * len(epis))(*epis) if epis else None
        return lib.check(lib.dll.truss_gcn_layer_group(la, ea, n_chains, steps, terms, st), "truss_gcn_layer_group")

    plain = lambda n, **kw: [layer(i, **kw) for i in range(n)]
    nout = lambda n: [layer(i, out=None) for i in range(n)]
    EINVAL, EUNSUP = r"failed \(-1\)", r"failed \(-2\)"
    refused = [
        (plain(2), -1, 1, 2, None, EINVAL),                                                    # n_chains < 0
        (plain(2), 2, 0, 2, None, EINVAL),                                                     # steps_per_chain < 1
        (plain(17), 17, 1, 2, None, EINVAL),                                                   # more than 16 plain layers
        ([layer(i // 5) for i in range(20)], 4, 5, 2, None, EINVAL),                           # ... as 4 x 5
        (nout(9), 9, 1, 2, [pooled(i) for i in range(9)], EINVAL),                             # more than 8 chains with epilogues
        ([layer(0, out=None), layer(0, out=None)], 1, 2, 2, [pooled(0)], EINVAL),               # epilogues with two steps
        (nout(2), 2, 1, 2, [pooled(0), head(1)], EINVAL),                                      # epilogues of different kind
        ([layer(0), layer(1, n_batch=1)], 2, 1, 2, None, EINVAL),                              # n_batch differs
        ([layer(0), layer(1, n_nodes=12)], 2, 1, 2, None, EINVAL),                             # n_nodes differs
        ([layer(0, n_nodes=8), layer(1, n_nodes=8, nbr=None, k_nbr=0)], 2, 1, 2, None, EINVAL),   # table against dense
        ([layer(0), layer(1, nbr=tab9.data_ptr(), k_nbr=9)], 2, 1, 2, None, EINVAL),           # (NW, KT) = (4, 6) against (4, 9)
        ([layer(0), layer(1)], 1, 2, 2, None, EINVAL),                                          # the steps of a chain differ in out
        ([layer(0), layer(0, out_row_stride=C)], 1, 2, 2, None, EINVAL),                        # ... in out_row_stride
        ([layer(0), layer(0, c_out=36)], 1, 2, 2, None, EINVAL),                                # ... in c_out
        ([layer(0), layer(0, x=out_ptr(0) + 4 * (n_out - 16), accumulate=1)], 1, 2, 2, None, EINVAL),   # a step's x inside an earlier out
        ([layer(0), layer(1, out=out_ptr(0) + 4 * (n_out - 1))], 2, 1, 2, None, EINVAL),        # the outputs of two chains overlap
        ([layer(0), layer(1, x=out_ptr(0))], 2, 1, 2, None, EINVAL),                            # a chain's out is another chain's x
        (nout(2), 2, 1, 2, [pooled(0), pooled(1, pool=pools.t[0].data_ptr() + 4 * (B * C - 1))], EINVAL),   # ... pools overlap
        (nout(2), 2, 1, 2, [head(0), head(1, out2=heads.t[0].data_ptr())], EINVAL),             # ... head outputs overlap
        ([layer(0), layer(1, w_bf16x3=None)], 2, 1, 2, None, EINVAL),                           # no split weights
        (plain(2), 2, 1, 0, None, EINVAL), (plain(2), 2, 1, 4, None, EINVAL),                   # bf16_terms 0 and 4
        ([layer(0), layer(1, act=3)], 2, 1, 2, None, EINVAL),                                   # the checks of the single layer
        ([layer(0), layer(1, struct_size=8)], 2, 1, 2, None, EINVAL),
        ([layer(0, c_out=32), layer(1, c_out=32)], 2, 1, 2, None, EUNSUP),
        ([layer(0, k_in=18), layer(1, k_in=18)], 2, 1, 1, None, EUNSUP),
        ([layer(i, nbr=tab10.data_ptr(), k_nbr=10) for i in range(2)], 2, 1, 3, None, EUNSUP),
        ([layer(0, out=None, accumulate=1)], 1, 1, 2, [pooled(0)], EINVAL),
        (nout(1), 1, 1, 2, [head(0, c2=9)], EINVAL),
    ]
    for layers, n_chains, steps, terms, epis, code in refused:
        with pytest.raises(tm.TrussError, match=code):
            call(layers, n_chains, steps, terms, epis)
    assert call([], 0, 1) == 0 and call(plain(2, n_batch=0), 2, 1) == 0 and call([layer(0, n_batch=0, out=None)], 1, 1, 2, [pooled(0)]) == 0
    torch.cuda.synchronize()
    for gd in (outs, heads, pools):
        assert gd.intact() and torch.equal(gd.t, torch.full_like(gd.t, 7.0))
    assert torch.equal(x, torch.ones_like(x))
    assert call([layer(0), layer(0, accumulate=1), layer(1), layer(1, accumulate=1)], 2, 2) == 0     # unrefused: 2 chains of 2 steps
    torch.cuda.synchronize()
    assert outs.intact() and torch.equal(outs.t[:2], torch.full_like(outs.t[:2], 2.0))                 # relu(0 + bias), twice
    assert torch.equal(outs.t[2:], torch.full_like(outs.t[2:], 7.0))
    ns, lid = ops.namespace(), ops.bind(lib)
    t = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(tm.TrussError, match="one entry per layer"):                                       # the operator's own checks
        ops.call(ns.gcn_layer_group, lid, st, [t(1, 8, 16)], [t(8, 8)], [None], [], [None], [t(1, 8, 40)], [1], [False], [ws[:, :, :16].contiguous()],
                 1, 0, [], [], [], [], [], [], [], 3)
    with pytest.raises(tm.TrussError, match="whole chains"):
        ops.call(ns.gcn_layer_group, lid, st, [t(1, 8, 16)], [t(8, 8)], [None], [t(40, 16)], [None], [t(1, 8, 40)], [1], [False],
                 [ws[:, :, :16].contiguous()], 2, 0, [], [], [], [], [], [], [], 3)


# ---- the three actors at once ------------------------------------------------------------------------------------------------------

def _group_launches(fn):
    """(result, launches of truss_gcn_group_bf3_kernel, all device operations) of fn() under torch.profiler"""
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return res, sum(1 for e in dev if "truss_gcn_group_bf3_kernel" in e.name), len(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [20, 50])
def test_actors_infer_equals_three_fused_calls_hip(P):
    """marl.actors_infer on the inputs of test_gcn_terms._actor_inputs (37 pairs, 16 nodes, hidden width 200, heads 2 and 3) for three
    actors of different seeds: torch.equal to three actor_infer(fused=True) calls under "bf16x3", "bf16x2" and "bf16", in four
    launches of the group kernel; under "f32", and without neighbour tables, every level falls back to the per-layer calls (no group
    launch) and the result is still equal"""
    lib = tm.load()
    actor0, ins, mod_in, nbr, nbr_p = TT._actor_inputs(P=P)
    actors = [actor0]
    for seed in (21, 22):
        torch.manual_seed(seed)
        actors.append(RL.multimodes_actor(200, 2, 3).to("cuda"))
    with torch.no_grad():
        for a in actors:
            a(mod_in)                                          # materialises the lazy layers
        assert not torch.equal(actors[0].gcn_l2_1.lin.weight, actors[1].gcn_l2_1.lin.weight)
        for precision, tables, launches in (("bf16x3", True, 4), ("bf16x2", True, 4), ("bf16", True, 4), ("f32", True, 0), ("bf16x3", False, 0)):
            kw = dict(nbr=nbr if tables else None, nbr_p=nbr_p if tables else None, precision=precision)
            want = [marl.actor_infer(lib, a, ins, fused=True, **kw) for a in actors]
            marl.actors_infer(lib, actors, ins, **kw)          # (warm-up: caches, LDS opt-in)
            got, n, total = _group_launches(lambda: marl.actors_infer(lib, actors, ins, **kw))
            print(f"\n[actors_infer] P {P} {precision} tables {tables}: {n} group launches, {total} device operations in all")
            assert n == launches, f"{precision} tables {tables}: {n} launches of the group kernel"
            # four launches plus the pad of x_n, the tiling copy and contiguous(): anything near the 33 + 9 of three fused calls
            # means per-layer work has crept back into the grouped path
            assert launches == 0 or total <= 10, f"{precision}: {total} device operations in one grouped call"
            assert len(got) == 3
            for (g_geo, g_topo), (w_geo, w_topo) in zip(got, want):
                assert g_geo.shape == (37, 16, 2) and g_topo.shape == (37, 16, 3)
                assert torch.equal(g_geo, w_geo) and torch.equal(g_topo, w_topo), f"{precision} tables {tables}"


def _play(lib, game, path, train):
    """three game steps of a 6-env, 8-node engine (hidden width 40: inside the split-weight envelope); returns what the two paths
    must agree on"""
    topo = tm.TrussTopology.grid(4, "small") if game == "test" else tm.TrussTopology.grid(4)
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(11)
        rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 40, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda")
        eng = marl.BatchedMARL(topo, 6, rl, max_front=6, lib=lib, device="cuda", replay_capacity=256, batch_size=8, seed=11, game=game,
                               actor_path=path)
        b = synthetic.random_batch(topo, 6, 11)
        eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
        assert eng.actor_path == path and topo.N == 8
        stats = [eng.game_step_all(train=train, explore=True) for _ in range(3)]
    state = [eng.pts, eng.n, eng.arch_y, eng.arch_sec]
    for s in stats:
        state += [v for _, v in sorted(s.items()) if torch.is_tensor(v)]
    if train:
        rp = eng.replay
        assert rp.size > 0
        state += [rp.S[k] for k in rp.KEYS] + [ns[k] for ns in rp.NS for k in rp.KEYS] + [rp.a_geo, rp.a_topo, rp.R]
        S, NS, ag, at, R = rp.sample(8, torch.Generator(device="cuda").manual_seed(5))
        state += [S[k] for k in rp.KEYS] + [ns[k] for ns in NS for k in rp.KEYS] + [ag, at, R]
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("game, train", [("train", True), ("test", False)])
def test_engines_differ_only_in_actor_path_hip(game, train):
    """two engines with the same seed and weights, exploration on (and, in the train game, training on), one with actor_path="fused",
    one "grouped": after three game steps the archives (pts, n, arch_y, arch_sec), the step results, the replay rings and a sampled
    batch are torch.equal -- the two paths play the same game bit for bit, the exploration noise drawn in the same order"""
    lib = tm.load()
    fused, grouped = _play(lib, game, "fused", train), _play(lib, game, "grouped", train)
    assert len(fused) == len(grouped) and len(fused) >= 4
    for i, (a, b) in enumerate(zip(fused, grouped)):
        assert a.shape == b.shape and torch.equal(a, b), f"{game}: tensor {i} differs between actor_path 'fused' and 'grouped'"
