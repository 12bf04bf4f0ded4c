"""The GCN kernels against float64 references (tests/gcn_reference.py): the fused layer kernel on both of its paths (bf16x3 and
float32 matrix cores), the level kernel, the two aggregation kernels and the actor's inference path.  Every bound is
elementwise, |got - ref64| <= tau * Mag, and every tau is shown to have teeth: host mutants of the same layer on the same inputs
(a bf16x3 partial product dropped, only the first-order products, a K slab left out, the diagonal neighbourhood term left out)
must violate it in the same test.

The taus (gcn_reference.TAU) sit at least 2x above the largest max |got - ref64| / Mag measured on an MI355X over these tests;
the values are recorded next to each tau."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import gcn, marl, ops
import parity_common as pc
import gcn_reference as G
import truss2D_RL as RL

TAU = G.TAU
MEASURED: dict = {}


def _record(path, r):
    MEASURED[path] = max(MEASURED.get(path, 0.0), r)


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


def _bf16x3_taken(x, w, nbr, N):
    return w.shape[0] > 32 and x.shape[2] % 4 == 0 and x.data_ptr() % 16 == 0 and (nbr.shape[1] if nbr is not None else N) <= 9


def _layer_case(lib, device, x, adj, w, bias, act, nbr, accumulate=False, label=""):
    B, N, _ = x.shape
    C = w.shape[0]
    out0 = torch.randn(B, N, C, device=device) if accumulate else None
    ref, mag = G.layer_ref(x, adj, w, bias, act, out0)
    assert G.within(G.bf16x3_model(x, adj, w, bias, act, out0), ref, mag, TAU["bf16x3"]), f"{label}: host model of the kernel"
    muts = G.mutants(x, adj, w, bias, act, out0) if act != "sigmoid" else {}
    for precision in ("bf16x3", "f32"):
        path = "bf16x3" if precision == "bf16x3" and _bf16x3_taken(x, w, nbr, N) else "f32"
        got = marl.gcn_layer(lib, x, adj, w, bias, act, nbr, out0.clone() if accumulate else None, accumulate, precision=precision)
        r = G.max_ratio(got, ref, mag)
        _record(path, r)
        assert r <= TAU[path], f"{label} {precision} ({path} path): max |got - ref64| / Mag = {r:.3g} > {TAU[path]:g}"
        for name, m in muts.items():       # teeth: every mutant of the same layer fails the same bound
            assert not G.within(m, ref, mag, TAU[path]), f"{label}: mutant '{name}' passes the {path} bound"


def _check_gcn_layer_float64(lib, device):
    """truss_gcn_layer on both paths against float64: c_out 3 / 32 / 33 / 200 / 224, k_in 4 / 13 / 16 / 200 / 256, truss patterns
    of 12 ... 256 nodes, a 9-term pattern, dense graphs of 7 / 20 / 64 nodes, accumulation, batch sizes whose rows leave the
    last tile part-empty, weight rows spanning 1e-6 ... 1e6.

    Measured on an MI355X, max |got - ref64| / Mag: bf16x3 path 2.2e-7, float32 path 1.4e-7 (TAU 1e-6 each; the emulator's
    sequential float32 sums: 2.9e-7 / 1.7e-7).  The weakest mutant (a2 b0 dropped) measures 1.6e-6 at k_in 256."""
    torch.manual_seed(11)
    rn = lambda *s: torch.randn(*s, device=device)
    for nx, B, K, C, act, kind, acc in (
            (6, 21, 13, 200, "relu", "per_env", False),     # 12 nodes: 10 graphs per 128-row tile, the last tile holds one
            (6, 21, 16, 200, "relu", "shared", False),
            (8, 9, 200, 200, "relu", "shared", True),
            (8, 9, 200, 3, "sigmoid", "per_env", False),
            (16, 5, 4, 33, None, "per_env", False),
            (32, 3, 256, 224, None, "per_env", False),
            (64, 3, 200, 200, "relu", "per_env", True),
            (128, 2, 200, 32, "relu", "shared", False)):
        topo = tm.TrussTopology.grid(nx)
        N, tab = topo.N, topo.neighbor_table()
        nbr, patt = torch.tensor(tab, device=device), torch.tensor(_pattern(tab), device=device)
        adj = torch.tensor(topo.normalized_adjacency()[0], device=device) if kind == "shared" else torch.rand(B, N, N, device=device) * patt
        x, w, b = rn(B, N, K), rn(C, K) / K ** 0.5, rn(C)
        _layer_case(lib, device, x, adj, w, b, act, nbr, acc, f"{N} nodes K {K} C {C}")
    tab9 = _random_pattern(24, 9, 1)                                     # 9 terms per row: the bf16x3 path's limit
    adj = torch.rand(5, 24, 24, device=device) * torch.tensor(_pattern(tab9), device=device)
    _layer_case(lib, device, rn(5, 24, 200), adj, rn(200, 200) / 14.0, rn(200), "relu", torch.tensor(tab9, device=device), False, "9 terms")
    for P, B, K, C, act, acc in ((7, 40, 4, 200, "relu", False), (20, 13, 200, 224, None, True), (64, 3, 16, 33, "relu", False)):
        adj = torch.softmax(rn(B, P, P), dim=-1)
        _layer_case(lib, device, rn(B, P, K), adj, rn(C, K) / K ** 0.5, rn(C), act, None, acc, f"dense {P}")
    topo = tm.TrussTopology.grid(8)                                      # weight rows from 1e-6 to 1e6: the bound is elementwise
    nbr = torch.tensor(topo.neighbor_table(), device=device)
    w = rn(200, 200) * torch.logspace(-6, 6, 200, device=device)[:, None]
    _layer_case(lib, device, rn(9, topo.N, 200), torch.tensor(topo.normalized_adjacency()[0], device=device), w, rn(200), None, nbr,
                False, "weights 1e-6 ... 1e6")
    print(f"\n[gcn float64] max |got - ref64| / Mag per path ({lib.backend}): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(MEASURED.items())))


def test_gcn_layer_float64_emulated():
    _check_gcn_layer_float64(pc.emu_lib(), "cpu")


@pytest.mark.gpu
def test_gcn_layer_float64_hip():
    _check_gcn_layer_float64(tm.load(), "cuda")


def _check_gcn_layer_envelope(lib, device, monkeypatch):
    """The path choice at the envelope's edges: 9 terms per row take bf16x3, 10 take the float32 path in Python and are refused by
    the C ABI when split weights are passed; a misaligned x takes the float32 path (refused with split weights); a dense graph of
    65 nodes is refused on both paths.  Results within the float64 bound of their path."""
    torch.manual_seed(5)
    rn = lambda *s: torch.randn(*s, device=device)
    splits = []
    orig = marl.split_weights
    monkeypatch.setattr(gcn, "split_weights", lambda *a, **k: splits.append(1) or orig(*a, **k))
    w, b = rn(200, 200) / 14.0, rn(200)
    ws = orig(lib, w)
    for terms, want in ((9, "bf16x3"), (10, "f32")):
        tab = _random_pattern(24, terms, terms)
        nbr = torch.tensor(tab, device=device)
        adj = torch.rand(3, 24, 24, device=device) * torch.tensor(_pattern(tab), device=device)
        x = rn(3, 24, 200)
        ref, mag = G.layer_ref(x, adj, w, b, "relu")
        splits.clear()
        got = marl.gcn_layer(lib, x, adj, w, b, "relu", nbr)
        assert len(splits) == (1 if want == "bf16x3" else 0), f"{terms} terms: path"
        assert G.max_ratio(got, ref, mag) <= TAU[want]
        if want == "f32":
            with pytest.raises(tm.TrussError):
                ops.call(ops.namespace().gcn_layer, ops.bind(lib), ops.stream_of(x.device), x, adj, nbr, w, b, torch.empty_like(got), 1, False, ws)
    topo = tm.TrussTopology.grid(8)
    nbr, N = torch.tensor(topo.neighbor_table(), device=device), topo.N
    adj = torch.tensor(topo.normalized_adjacency()[0], device=device)
    x = torch.empty(4 * N * 200 + 1, device=device)[1:].view(4, N, 200)          # contiguous, 4 bytes off a 16-byte boundary
    x.copy_(rn(4, N, 200))
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    ref, mag = G.layer_ref(x, adj, w, b, None)
    splits.clear()
    got = marl.gcn_layer(lib, x, adj, w, b, None, nbr)
    assert not splits and G.max_ratio(got, ref, mag) <= TAU["f32"]
    with pytest.raises(tm.TrussError):
        ops.call(ops.namespace().gcn_layer, ops.bind(lib), ops.stream_of(x.device), x, adj, nbr, w, b, torch.empty_like(got), 0, False, ws)
    for precision in ("bf16x3", "f32"):
        with pytest.raises(tm.TrussError):
            marl.gcn_layer(lib, rn(1, 65, 200), torch.softmax(rn(65, 65), -1), w, b, None, None, precision=precision)


def test_gcn_layer_envelope_emulated(monkeypatch):
    _check_gcn_layer_envelope(pc.emu_lib(), "cpu", monkeypatch)


@pytest.mark.gpu
def test_gcn_layer_envelope_hip(monkeypatch):
    _check_gcn_layer_envelope(tm.load(), "cuda", monkeypatch)


class _LayerArgs(ctypes.Structure):          # truss_gcn_layer_args_t (include/truss_mi355.h)
    _fields_ = [("struct_size", ctypes.c_size_t)] + [(n, ctypes.c_int32) for n in ("n_batch", "n_nodes", "k_in", "c_out", "act", "accumulate", "k_nbr", "reserved")] + \
               [("x", ctypes.c_void_p), ("x_row_stride", ctypes.c_int64), ("adj", ctypes.c_void_p), ("a_batch_stride", ctypes.c_int64),
                ("nbr", ctypes.c_void_p), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("out_row_stride", ctypes.c_int64), ("w_bf16x3", ctypes.c_void_p)]


def _check_gcn_refusals(lib, device):
    """What truss_gcn_layer / truss_gcn_level refuse is one piece of host code for the product and the emulator: an activation
    code of 3, out aliasing x, and a level with a layer that accumulates -- same code, same text, nothing launched or written."""
    B, N, K, C = 1, 2, 4, 4
    x, adj, w, b = (torch.ones(*s, device=device) for s in ((B, N, K), (N, N), (C, K), (C,)))
    ns, lid, st = ops.namespace(), ops.bind(lib), ops.stream_of(x.device)
    out = torch.full((B, N, C), 7.0, device=device)
    with pytest.raises(tm.TrussError, match=r"truss_gcn_layer failed \(-1\): truss_gcn_layer: bad sizes / act"):
        ops.call(ns.gcn_layer, lid, st, x, adj, None, w, b, out, 3, False, None)
    with pytest.raises(tm.TrussError, match=r"truss_gcn_layer failed \(-1\): truss_gcn_layer: out must not alias x"):
        ops.call(ns.gcn_layer, lid, st, x, adj, None, w, b, x, 0, False, None)
    with pytest.raises(tm.TrussError, match=r"truss_gcn_level failed \(-1\): truss_gcn_level: out must not alias x"):
        ops.call(ns.gcn_level, lid, st, [x, x], [adj, adj], [], [w, w], [b, b], [out, x], [], [0, 0])
    outs = [torch.full((B, N, C), 7.0, device=device) for _ in range(2)]
    layers = (_LayerArgs * 2)(*[_LayerArgs(struct_size=ctypes.sizeof(_LayerArgs), n_batch=B, n_nodes=N, k_in=K, c_out=C, act=1, accumulate=i,
                                           x=x.data_ptr(), adj=adj.data_ptr(), w=w.data_ptr(), bias=b.data_ptr(), out=o.data_ptr())
                                for i, o in enumerate(outs)])
    with pytest.raises(tm.TrussError, match=r"failed \(-2\): truss_gcn_level: float32 product, no accumulation into out"):
        lib.check(lib.dll.truss_gcn_level(layers, 2, None, st), "truss_gcn_level")
    if device == "cuda":
        torch.cuda.synchronize()
    assert torch.equal(x, torch.ones_like(x)) and all(torch.equal(o, torch.full_like(o, 7.0)) for o in [out] + outs)


def test_gcn_refusals_emulated():
    _check_gcn_refusals(pc.emu_lib(), "cpu")


@pytest.mark.gpu
def test_gcn_refusals_hip():
    _check_gcn_refusals(tm.load(), "cuda")


def _check_sigmoid_saturation(lib, device):
    """sigmoid epilogue with pre-activations out to +-100: finite, absolute error <= 1e-6 against float64 (both paths)"""
    torch.manual_seed(6)
    topo = tm.TrussTopology.grid(8)
    nbr, N = torch.tensor(topo.neighbor_table(), device=device), topo.N
    adj = torch.tensor(topo.normalized_adjacency()[0], device=device)
    x = torch.rand(5, N, 16, device=device)
    for C in (3, 200):
        w = torch.randn(C, 16, device=device) * 0.1
        b = torch.linspace(-100.0, 100.0, C, device=device)
        ref, _ = G.layer_ref(x, adj, w, b, "sigmoid")
        for precision in ("bf16x3", "f32"):
            got = marl.gcn_layer(lib, x, adj, w, b, "sigmoid", nbr, precision=precision)
            assert torch.isfinite(got).all()
            err = float(np.abs(G.f64(got) - ref).max())
            assert err <= 1e-6, f"C {C} {precision}: {err:.3g}"


def test_sigmoid_saturation_emulated():
    _check_sigmoid_saturation(pc.emu_lib(), "cpu")


@pytest.mark.gpu
def test_sigmoid_saturation_hip():
    _check_sigmoid_saturation(tm.load(), "cuda")


def _check_gcn_level_float64(lib, device):
    """truss_gcn_level over a mix of shapes in ONE launch (dense 32 / 12 / 16 / 64 nodes, a 24-node pattern, k_in 200 / 256 / 8 /
    13 / 40 / 20, c_out 200 / 224 / 3 / 70 / 33, every activation): outputs within TAU['level'] * Mag of float64, X' = A X within
    TAU['level'] * |A| |X|; the last-K-slab and diagonal-term mutants of every relu / linear layer violate the bound.
    Measured on an MI355X: max ratio 2.8e-7 (TAU 1e-6; emulator 2.7e-7)."""
    torch.manual_seed(4)
    r = lambda *s: torch.rand(*s, device=device)
    tab = tm.TrussTopology.grid(12).neighbor_table()
    cases = [(5, 32, 200, 200, "relu", "dense"), (7, 12, 256, 224, None, "dense"), (33, 16, 8, 3, "sigmoid", "dense"),
             (9, 16, 13, 200, "relu", "shared"), (3, 24, 40, 70, "relu", "pattern"), (2, 64, 20, 33, None, "dense")]
    X, A, NBR, W, BIAS, ACT, OUT, XA = [], [], [], [], [], [], [], []
    for B, N, K, C, act, kind in cases:
        x, w, b = r(B, N, K) - 0.5, (r(C, K) - 0.5) / 4, r(C) - 0.5
        a = (torch.softmax(torch.randn(N, N, device=device), -1) if kind == "shared" else
             r(B, N, N) * torch.tensor(_pattern(tab), device=device) if kind == "pattern" else torch.softmax(torch.randn(B, N, N, device=device), -1))
        X.append(x), A.append(a), W.append(w), BIAS.append(b), ACT.append({None: 0, "relu": 1, "sigmoid": 2}[act])
        NBR.append(torch.tensor(tab, device=device) if kind == "pattern" else None)
        OUT.append(torch.full((B, N, C), float("nan"), device=device))
        XA.append(torch.full((B, N, K), float("nan"), device=device))
    ops.call(ops.namespace().gcn_level, ops.bind(lib), ops.stream_of(torch.device(device)), X, A, NBR, W, BIAS, OUT, XA, ACT)
    for (B, N, K, C, act, kind), x, a, w, b, o, xa in zip(cases, X, A, W, BIAS, OUT, XA):
        ref, mag = G.layer_ref(x, a, w, b, act)
        r_o = G.max_ratio(o, ref, mag)
        Ad = G.dense_adj(a, B, N)
        r_x = G.max_ratio(xa, Ad @ G.f64(x), np.abs(Ad) @ np.abs(G.f64(x)))
        _record("level", max(r_o, r_x))
        assert r_o <= TAU["level"] and r_x <= TAU["level"], f"case {(B, N, K, C, act, kind)}: {r_o:.3g} / X' {r_x:.3g}"
        if act != "sigmoid":
            for name in ("last K slab left out", "diagonal term left out"):
                assert not G.within(G.mutants(x, a, w, b, act)[name], ref, mag, TAU["level"]), name
    print(f"\n[gcn float64] level ({lib.backend}): max ratio {MEASURED['level']:.3g}")


def test_gcn_level_float64_emulated():
    _check_gcn_level_float64(pc.emu_lib(), "cpu")


@pytest.mark.gpu
def test_gcn_level_float64_hip():
    _check_gcn_level_float64(tm.load(), "cuda")


def _check_aggregate_float64(lib, device):
    """truss_gcn_aggregate (dense, <= 64 nodes, shared / per-env adjacency) and truss_gcn_aggregate_sparse (a truss's neighbour table)
    against float64 with |got - ref| <= TAU['agg'] (|A| |H| + |b|); the aggregation without its diagonal term violates it.
    Measured on an MI355X: max ratio 5.4e-7 (TAU 1.5e-6; emulator 5.5e-7)."""
    torch.manual_seed(8)
    code = {None: 0, "relu": 1, "sigmoid": 2}

    def check(adj, h, bias, act, got, label):
        ref, mag = G.agg_ref(adj, h, bias, act)
        r = G.max_ratio(got, ref, mag)
        _record("agg", r)
        assert r <= TAU["agg"], f"{label}: {r:.3g}"
        if act != "sigmoid":
            B, N, _ = h.shape
            Ad = G.dense_adj(adj, B, N).copy()
            Ad[:, np.arange(N), np.arange(N)] = 0.0
            mut = G.act64(Ad @ G.f64(h) + G.f64(bias), act)
            assert not G.within(mut, ref, mag, TAU["agg"]), f"{label}: mutant without the diagonal passes"

    # the first five: the slab kernel and aggregate_kernel<32>; then aggregate4<16> over 3 blocks (C4 = 5 does not divide 256: graphs
    # straddle the block boundaries) and in one block, aggregate_kernel<16> with one and two channel blocks, aggregate_kernel<64>
    for n, c, B in ((24, 70, 9), (32, 224, 5), (48, 36, 3), (64, 8, 4), (17, 4, 11),
                    (12, 20, 120), (8, 8, 70), (16, 6, 3), (9, 262, 2), (40, 6, 3)):
        h, bias = torch.randn(B, n, c, device=device), torch.randn(c, device=device)
        adj = torch.softmax(torch.randn(B, n, n, device=device), dim=-1)
        for a_, act in ((adj, "relu"), (adj[0], None), (adj, "sigmoid")):
            check(a_, h, bias, act, marl.gcn_aggregate(lib, a_, h, bias, act), f"dense {n} x {c}")
    for nx, B, C in ((8, 7, 8), (32, 5, 224), (128, 2, 12)):
        topo = tm.TrussTopology.grid(nx)
        N, tab = topo.N, topo.neighbor_table()
        nbr, patt = torch.tensor(tab, device=device), torch.tensor(_pattern(tab), device=device)
        h, bias = torch.randn(B, N, C, device=device), torch.randn(C, device=device)
        for adj, act in ((torch.tensor(topo.normalized_adjacency()[0], device=device), "relu"), (torch.rand(B, N, N, device=device) * patt, None)):
            out = torch.empty_like(h)
            ops.call(ops.namespace().gcn_aggregate_sparse, ops.bind(lib), ops.stream_of(h.device), adj, nbr, h, bias, out, code[act])
            check(adj, h, bias, act, out, f"sparse {N} x {C}")
    print(f"\n[gcn float64] aggregation ({lib.backend}): max ratio {MEASURED['agg']:.3g}")


def test_aggregate_float64_emulated():
    _check_aggregate_float64(pc.emu_lib(), "cpu")


@pytest.mark.gpu
def test_aggregate_float64_hip():
    _check_aggregate_float64(tm.load(), "cuda")


def _check_actor_infer_float64(lib, device):
    """actor_infer end to end (every layer a fused kernel, the hidden ones on the bf16x3 path) against the float64 module
    (copy.deepcopy(actor).double()): its max error is no worse than 4x that of the float32 module on the same inputs"""
    torch.manual_seed(9)
    B, P = 37, 20
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
    with torch.no_grad():
        f32 = actor(mod_in)
        a64 = copy.deepcopy(actor).double()
        ref = a64([t.double() for t in mod_in])
        got = marl.actor_infer(lib, actor, ins, nbr=torch.tensor(tab, device=device), nbr_p=torch.tensor(marl.path_graph_table(P), device=device))
    for g, f, y in zip(got, f32, ref):
        e_kernel, e_module = float((g.double() - y).abs().max()), float((f.double() - y).abs().max())
        assert e_kernel <= 4.0 * e_module, f"actor_infer max error {e_kernel:.3g} against the float32 module's {e_module:.3g}"


def test_actor_infer_float64_emulated():
    _check_actor_infer_float64(pc.emu_lib(), "cpu")


@pytest.mark.gpu
def test_actor_infer_float64_hip():
    _check_actor_infer_float64(tm.load(), "cuda")


def _check_split_weights(lib, device):
    """truss_gcn_split_w for c_out 33 / 200 / 224 and k_in 4 / 13 / 200: the [3, 224, kp] image holds, term by term, exactly the
    truncating split of the host (gcn_reference.split3), the three terms sum to the weight exactly, and the padding is zero"""
    torch.manual_seed(10)
    for C, K in ((33, 4), (224, 13), (33, 13), (224, 4), (200, 200)):
        w = torch.randn(C, K, device=device) * torch.logspace(-6, 6, C, device=device)[:, None]
        ws = marl.split_weights(lib, w)
        KP = (K + 15) // 16 * 16
        assert ws.shape == (3, 224, KP) and ws.dtype == torch.int16
        t = (ws.to(torch.int32) << 16).view(torch.float32).cpu()
        host = G.split3(w.cpu().numpy())
        for i in range(3):
            assert np.array_equal(t[i, :C, :K].numpy(), host[i]), f"C {C} K {K}: term {i}"
        assert torch.equal(t[0, :C, :K].double() + t[1, :C, :K].double() + t[2, :C, :K].double(), w.double().cpu())
        assert int(ws[:, C:, :].abs().max() if C < 224 else 0) == 0 and int(ws[:, :, K:].abs().max() if K < KP else 0) == 0
        again = torch.full_like(ws, 0x7F7F)                              # out=: the same image written into an existing buffer
        assert marl.split_weights(lib, w, out=again).data_ptr() == again.data_ptr() and torch.equal(again, ws)


def test_split_weights_emulated():
    _check_split_weights(pc.emu_lib(), "cpu")


@pytest.mark.gpu
def test_split_weights_hip():
    _check_split_weights(tm.load(), "cuda")
