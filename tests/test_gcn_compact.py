"""The GCN layer kernels on compact adjacencies (truss_gcn_layer_args_t.adj_layout = 1): adj holds the [N, Kc] rows of the compact
observation layout, term t of row i is adj[i, t] and its source row nbr[i, t].  The coefficients and their order are those of the
dense call through the same table, so every compact call must be torch.equal to the dense call on the same inputs -- on every path
of the layer: register terms and LDS-index terms, the float32 and the split-weight products at every number of bf16 terms, with and
without accumulation, the head epilogue, and a chain of the grouped launch.  One case is also held against float64 with the bound
of tests/test_gcn_float64.py, so that two equally wrong paths do not pass."""
import numpy as np
import pytest
import torch

import gcn_reference as G
import parity_common as pc
import truss_mi355 as tm
from truss_mi355 import gcn, ops

PRECISIONS = ("f32", "bf16x3", "bf16x2", "bf16")


def _pattern(tab):
    pat = np.zeros((tab.shape[0], tab.shape[0]), bool)
    for i, r in enumerate(tab):
        pat[i, r[r >= 0]] = True
    return pat


def _random_table(N, terms, seed):
    """`terms` distinct ascending columns per row, the node itself among them, the last rows two terms short (padding)"""
    rng = np.random.default_rng(seed)
    tab = np.full((N, terms), -1, np.int16)
    for i in range(N):
        n = terms - (2 if i >= N - 3 else 0)
        others = rng.choice(np.delete(np.arange(N), i), n - 1, replace=False)
        tab[i, :n] = np.sort(np.concatenate([[i], others]))
    return tab


def _compact(adj, nbr):
    """dense [.., N, N] -> the compact rows [.., N, Kc] (the layout's definition)"""
    idx = nbr.clamp(min=0).long()
    return (adj.gather(-1, idx.expand(adj.shape[:-1] + (nbr.shape[1],))) * (nbr >= 0)).contiguous()


def _case(N, B, K, C, device, table=None, seed=0):
    g = torch.Generator().manual_seed(100 * N + K + seed)
    tab = tm.TrussTopology.grid(N // 2).neighbor_table() if table is None else table
    nbr = torch.tensor(tab, device=device)
    adj = (torch.rand(B, N, N, generator=g) * torch.tensor(_pattern(tab))).to(device)
    rn = lambda *s: torch.randn(*s, generator=g).to(device)
    return dict(x=rn(B, N, K), adj=adj, adjc=_compact(adj, nbr), nbr=nbr, w=rn(C, K) / K ** 0.5, b=rn(C))


def test_layout_helpers_round_trip():
    c = _case(16, 3, 16, 40, "cpu")
    assert c["adjc"].shape == (3, 16, c["nbr"].shape[1])
    assert torch.equal(gcn.expand_compact(c["adjc"], c["nbr"]), c["adj"])
    assert torch.equal(gcn.expand_compact(c["adjc"][0], c["nbr"]), c["adj"][0])
    assert gcn.COMPACT_ADJ == ("A_s", "A_ts", "A_cs")


def test_compact_layers_on_the_emulator():
    """the CPU stand-in reads dense adjacencies only: the library says so for adj_layout 1, refuses any other value with the shared
    check, and the wrappers expand the compact rows on the host -- same bits as the dense call"""
    lib = pc.emu_lib()
    c = _case(16, 3, 16, 40, "cpu")
    ns, lid = ops.namespace(), ops.bind(lib)
    out = torch.full((3, 16, 40), -7.5)
    with pytest.raises(tm.TrussError, match="adj_layout is 0"):
        ops.call(ns.gcn_layer, lid, 0, c["x"], c["adj"], c["nbr"], c["w"], c["b"], out, 1, False, None, 2)
    with pytest.raises(tm.TrussError, match="dense adjacencies only"):
        ops.call(ns.gcn_layer, lid, 0, c["x"], c["adjc"], c["nbr"], c["w"], c["b"], out, 1, False, None, 1)
    with pytest.raises(tm.TrussError, match="compact adj"):                                   # a compact call without its table
        ops.call(ns.gcn_layer, lid, 0, c["x"], c["adjc"], None, c["w"], c["b"], out, 1, False, None, 1)
    with pytest.raises(tm.TrussError, match="compact adj"):                                   # a dense matrix handed over as compact
        ops.call(ns.gcn_layer, lid, 0, c["x"], c["adj"], c["nbr"], c["w"], c["b"], out, 1, False, None, 1)
    assert bool((out == -7.5).all())
    with pytest.raises(ValueError, match="neighbour table"):
        gcn.gcn_layer(lib, c["x"], c["adjc"], c["w"], c["b"], "relu", None, compact=True)
    dense = gcn.gcn_layer(lib, c["x"], c["adj"], c["w"], c["b"], "relu", c["nbr"], precision="f32")
    assert torch.equal(gcn.gcn_layer(lib, c["x"], c["adjc"], c["w"], c["b"], "relu", c["nbr"], precision="f32", compact=True), dense)


# ---- the kernels ----
SHAPES = [(16, 9, 200, 200), (16, 9, 16, 200), (256, 3, 200, 200), (256, 3, 16, 200)]      # N, B (256 nodes: a partial tile), K, C


@pytest.mark.gpu
@pytest.mark.parametrize("N,B,K,C", SHAPES)
def test_compact_layer_equals_dense_hip(N, B, K, C):
    lib = tm.load()
    c = _case(N, B, K, C, "cuda")
    assert c["nbr"].shape[1] <= 9
    for precision in PRECISIONS:
        for acc in (False, True):
            out0 = torch.randn(B, N, C, device="cuda") if acc else None
            d = gcn.gcn_layer(lib, c["x"], c["adj"], c["w"], c["b"], "relu", c["nbr"], out0.clone() if acc else None, acc, precision)
            k = gcn.gcn_layer(lib, c["x"], c["adjc"], c["w"], c["b"], "relu", c["nbr"], out0.clone() if acc else None, acc, precision,
                              compact=True)
            assert torch.equal(k, d), (precision, acc)
    # one adjacency for the whole batch (a_batch_stride 0)
    d = gcn.gcn_layer(lib, c["x"], c["adj"][0], c["w"], c["b"], None, c["nbr"])
    assert torch.equal(gcn.gcn_layer(lib, c["x"], c["adjc"][0].contiguous(), c["w"], c["b"], None, c["nbr"], compact=True), d)


@pytest.mark.gpu
def test_compact_layer_against_float64_hip():
    """so that two equally wrong paths do not pass: the compact call within the float64 bound of tests/test_gcn_float64.py"""
    lib = tm.load()
    c = _case(16, 9, 200, 200, "cuda")
    ref, mag = G.layer_ref(c["x"], c["adj"], c["w"], c["b"], "relu")
    for precision in ("f32", "bf16x3"):
        got = gcn.gcn_layer(lib, c["x"], c["adjc"], c["w"], c["b"], "relu", c["nbr"], precision=precision, compact=True)
        r = G.max_ratio(got, ref, mag)
        assert r <= G.TAU[precision], f"{precision}: max |got - ref64| / Mag = {r:.3g}"
    for name, m in G.mutants(c["x"], c["adj"], c["w"], c["b"], "relu").items():               # the bound has teeth on this case
        assert not G.within(m, ref, mag, G.TAU["f32"]), name


@pytest.mark.gpu
def test_compact_layer_wide_table_hip():
    """12 terms per row: beyond the register path, the coefficients go through the LDS-index path (float32 product under every
    precision)"""
    lib = tm.load()
    tab = _random_table(16, 12, 5)
    for K, C in ((200, 200), (16, 200)):
        c = _case(16, 9, K, C, "cuda", table=tab)
        assert c["nbr"].shape[1] == 12 and bool((c["nbr"] < 0).any())
        for precision in ("f32", "bf16x3"):
            for acc in (False, True):
                out0 = torch.randn(9, 16, C, device="cuda") if acc else None
                d = gcn.gcn_layer(lib, c["x"], c["adj"], c["w"], c["b"], "relu", c["nbr"], out0.clone() if acc else None, acc, precision)
                k = gcn.gcn_layer(lib, c["x"], c["adjc"], c["w"], c["b"], "relu", c["nbr"], out0.clone() if acc else None, acc, precision,
                                  compact=True)
                assert torch.equal(k, d), (K, precision, acc)
        ref, mag = G.layer_ref(c["x"], c["adj"], c["w"], c["b"], "relu")
        assert G.max_ratio(gcn.gcn_layer(lib, c["x"], c["adjc"], c["w"], c["b"], "relu", c["nbr"], precision="f32", compact=True), ref, mag) \
            <= G.TAU["f32"]


@pytest.mark.gpu
@pytest.mark.parametrize("N,B", [(16, 9), (256, 3)])
def test_compact_head_and_group_hip(N, B):
    """gcn_layer_head: only the layer's own adjacency is compact, the head's adj2 (the shared A_n) stays dense; gcn_layer_group: a
    chain of five steps that accumulate into one out, each over its own compact adjacency"""
    lib = tm.load()
    topo = tm.TrussTopology.grid(N // 2)
    A_n = torch.tensor(topo.normalized_adjacency()[0], device="cuda")
    c = _case(N, B, 200, 200, "cuda")
    g = torch.Generator().manual_seed(3)
    w2, b2 = (torch.randn(3, 200, generator=g) / 14.0).cuda(), torch.randn(3, generator=g).cuda()
    for precision in PRECISIONS:
        d = gcn.gcn_layer_head(lib, c["x"], c["adj"], c["w"], c["b"], "relu", w2, b2, A_n, "sigmoid", c["nbr"], c["nbr"], precision)
        k = gcn.gcn_layer_head(lib, c["x"], c["adjc"], c["w"], c["b"], "relu", w2, b2, A_n, "sigmoid", c["nbr"], c["nbr"], precision,
                               compact=True)
        assert torch.equal(k, d), precision
    steps = [_case(N, B, 200, 200, "cuda", seed=s) for s in range(5)]
    ws = [gcn.split_weights(lib, s["w"]) for s in steps]
    for precision in ("bf16x3", "bf16x2", "bf16"):
        outs = {}
        for compact in (False, True):
            out = torch.full((B, N, 200), -7.5, device="cuda")
            chain = [dict(x=s["x"], adj=s["adjc"] if compact else s["adj"], nbr=s["nbr"], w=s["w"], bias=s["b"], act="relu", out=out,
                          accumulate=j > 0, w_split=ws[j], compact=compact) for j, s in enumerate(steps)]
            gcn.gcn_layer_group(lib, [chain], precision)
            outs[compact] = out
        assert torch.equal(outs[True], outs[False]), precision
        one = None                                                                           # ... and the chain is the layers one by one
        for j, s in enumerate(steps):
            one = gcn.gcn_layer(lib, s["x"], s["adjc"], s["w"], s["b"], "relu", s["nbr"], one, j > 0, precision, ws[j], compact=True)
        assert torch.equal(one, outs[True]), precision


@pytest.mark.gpu
def test_adj_layout_refusals_hip():
    lib = tm.load()
    c = _case(16, 3, 200, 200, "cuda")
    ns, lid, st = ops.namespace(), ops.bind(lib), ops.stream_of(torch.device("cuda"))
    out = torch.full((3, 16, 200), -7.5, device="cuda")
    for layout in (2, -1):
        with pytest.raises(tm.TrussError, match="adj_layout is 0"):
            ops.call(ns.gcn_layer, lid, st, c["x"], c["adj"], c["nbr"], c["w"], c["b"], out, 1, False, None, layout)
    with pytest.raises(tm.TrussError, match="adj_layout is 0"):
        ops.call(ns.gcn_layer_terms, lid, st, c["x"], c["adj"], c["nbr"], c["w"], c["b"], out, 1, gcn.split_weights(lib, c["w"]), 0, None, None,
                 None, None, 0, None, None, False, 2, 2)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())
