"""Compact (neighbour-table) replay storage and the fused append / sample operators `replay_scatter` / `replay_gather`.

Data is only moved, so every comparison is bitwise (torch.equal; the operator tests also compare the int32 views, with NaN / inf
bit patterns placed inside the pattern).  The reference is the dense `DeviceReplay` and the framework-indexing implementation of
compact storage (what runs on the cpu, or with a native library that lacks the entries)."""
import contextlib
import io

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import marl, ops, pool, synthetic
from truss_mi355._lib import TrussError
import parity_common as pc
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL

KEYS = marl.DeviceReplay.KEYS
PATTERN = marl.DeviceReplay.PATTERN_KEYS


class _NoReplayOps:
    """a native library without the replay entries: compact storage then runs as framework indexing, on any device"""
    backend, has_replay_ops = "hip", False


def _mask(table):
    t = np.asarray(table)
    m = np.zeros((t.shape[0], t.shape[0]), bool)
    r, s = np.nonzero(t >= 0)
    m[r, t[r, s]] = True
    return torch.from_numpy(m)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """torch.equal on the values (where neither is NaN: NaN != NaN) and on the bit patterns (all of them, NaN payloads and signed zeros too)"""
    if a.shape != b.shape or not torch.equal(_bits(a), _bits(b)):
        return False
    ok = ~(a.isnan() | b.isnan())
    return torch.equal(a[ok], b[ok])


def _rows(lead, N, P, nbr, nbr_p, g, device="cpu", special=False):
    """observation tensors [*lead, ...]: random values on the tables' patterns, zeros elsewhere; special: a NaN, an inf and a -0.0
    at listed positions of every adjacency"""
    mn, mp = _mask(nbr), _mask(nbr_p)
    shapes = dict(x_n=(N, 13), A_s=(N, N), A_n_ts=(N, N), A_n_cs=(N, N), x_p=(P, 4), A_p=(P, P))
    out = {}
    for k in KEYS:
        t = torch.randn(*lead, *shapes[k], generator=g)
        if k in PATTERN:
            m = mp if k == "A_p" else mn
            t = torch.where(m, t, torch.zeros(()))
            if special:
                pos = torch.nonzero(m)
                flat = t.view(-1, *shapes[k])
                for j, v in enumerate((float("nan"), float("inf"), -0.0, float("-inf"))):
                    i, c = pos[(3 * j + 1) % len(pos)].tolist()
                    flat[j % flat.shape[0], i, c] = v
        out[k] = t.to(device)
    return out


def _transitions(K, N, P, nbr, nbr_p, seed, device="cpu", special=False):
    g = torch.Generator().manual_seed(seed)
    S = _rows((K,), N, P, nbr, nbr_p, g, device, special)
    NSall = _rows((3, K), N, P, nbr, nbr_p, g, device, special)
    src = torch.randint(0, 3, (K, 3), generator=g).to(device)
    sel = (torch.rand(K, generator=g) > 0.35).to(device)
    ag = torch.rand(3, K, N, 2, generator=g).to(device)       # agent-major, handed over as permuted views (as the engine does)
    at = torch.rand(3, K, N, 3, generator=g).to(device)
    R = torch.rand(K, 3, generator=g).to(device)
    return S, NSall, src, sel, ag.permute(1, 0, 2, 3), at.permute(1, 0, 2, 3), R


def _explicit(NSall, src):
    ark = torch.arange(src.shape[0], device=src.device)
    return [{k: NSall[k][src[:, a], ark] for k in KEYS} for a in range(3)]


def _assert_same_batches(a, b, batch, seed, device="cpu"):
    ga, gb = torch.Generator(device=device).manual_seed(seed), torch.Generator(device=device).manual_seed(seed)
    Sa, NSa, aga, ata, Ra = a.sample(batch, ga)
    Sb, NSb, agb, atb, Rb = b.sample(batch, gb)
    for k in KEYS:
        assert _same(Sa[k], Sb[k]), k
        for i in range(3):
            assert _same(NSa[i][k], NSb[i][k]), (k, i)
    assert _same(aga, agb) and _same(ata, atb) and _same(Ra, Rb)
    assert torch.equal(ga.get_state(), gb.get_state())


def _pair(cap, N, P, nbr, nbr_p, device="cpu", lib=None):
    return (marl.DeviceReplay(cap, N, P, device, storage="compact", nbr=nbr, nbr_p=nbr_p, lib=lib), marl.DeviceReplay(cap, N, P, device))


# ---------------------------------------------------------------- not GPU ----------------------------------------------------------------

def test_compact_add_sample_match_dense():
    topo = tm.TrussTopology.grid(4)
    N, P = topo.N, 3
    nbr, nbr_p = topo.neighbor_table(), marl.path_graph_table(P)
    c, d = _pair(32, N, P, nbr, nbr_p)
    assert c.S["A_s"].shape == (32, N, nbr.shape[1]) and c.S["A_p"].shape == (32, P, 3) and d.S["A_s"].shape == (32, N, N)
    S, NSall, src, sel, ag, at, R = _transitions(9, N, P, nbr, nbr_p, 1)
    assert c.add(sel, S, NSall, ag, at, R, src=src) == d.add(sel, S, NSall, ag, at, R, src=src) == int(sel.sum())
    S, NSall, src, sel, ag, at, R = _transitions(7, N, P, nbr, nbr_p, 2)
    NS = _explicit(NSall, src)
    assert c.add(sel, S, NS, ag, at, R) == d.add(sel, S, NS, ag, at, R) == int(sel.sum())
    assert c.size == d.size and c.head == d.head and c.capacity == d.capacity
    _assert_same_batches(c, d, 16, 5)
    for k in ("x_n", "x_p"):
        assert torch.equal(c.S[k], d.S[k])
    assert torch.equal(c.a_geo, d.a_geo) and torch.equal(c.a_topo, d.a_topo) and torch.equal(c.R, d.R)
    assert c.nbytes < d.nbytes


def test_compact_ring_behaviour():
    topo = tm.TrussTopology.grid(4)
    N, P = topo.N, 3
    nbr, nbr_p = topo.neighbor_table(), marl.path_graph_table(P)
    c, d = _pair(7, N, P, nbr, nbr_p)
    every = torch.ones(5, dtype=torch.bool)
    for seed in (1, 2):                                            # 5 + 5 rows into 7: the second add wraps around
        S, NSall, src, _, ag, at, R = _transitions(5, N, P, nbr, nbr_p, seed)
        assert c.add(every, S, NSall, ag, at, R, src=src) == d.add(every, S, NSall, ag, at, R, src=src) == 5
    assert (c.size, c.head) == (d.size, d.head) == (7, 3)
    _assert_same_batches(c, d, 12, 3)
    S, NSall, src, _, ag, at, R = _transitions(9, N, P, nbr, nbr_p, 4)   # 9 rows into 7: the first 7 are kept
    every = torch.ones(9, dtype=torch.bool)
    assert c.add(every, S, NSall, ag, at, R, src=src) == d.add(every, S, NSall, ag, at, R, src=src) == 7
    assert (c.size, c.head) == (d.size, d.head) == (7, 3)
    _assert_same_batches(c, d, 12, 6)
    before = [t.clone() for t in list(c.S.values()) + [c.a_geo, c.R]]
    assert c.add(torch.zeros(9, dtype=torch.bool), S, NSall, ag, at, R, src=src) == 0
    assert (c.size, c.head) == (7, 3)
    assert all(torch.equal(a, b) for a, b in zip(before, list(c.S.values()) + [c.a_geo, c.R]))


def test_compact_nbytes_by_formula():
    N, Kn, P, cap = 256, 9, 20, 64
    nbr = np.full((N, Kn), -1, np.int16)
    nbr[:, 0] = np.arange(N)
    c = marl.DeviceReplay(cap, N, P, "cpu", storage="compact", nbr=nbr, nbr_p=marl.path_graph_table(P))
    assert c.nbytes == 4 * cap * (4 * (13 * N + 3 * N * Kn + 4 * P + 3 * P) + 15 * N + 3)
    d = marl.DeviceReplay(cap, N, P, "cpu")
    assert d.nbytes == 4 * cap * (4 * (13 * N + 3 * N * N + 4 * P + P * P) + 15 * N + 3)


def test_storage_arguments():
    with pytest.raises(ValueError):
        marl.DeviceReplay(8, 8, 3, "cpu", storage="sparse")
    with pytest.raises(ValueError):
        marl.DeviceReplay(8, 8, 3, "cpu", storage="compact")          # no tables
    d = marl.DeviceReplay(8, 8, 3, "cpu")
    assert d.storage == "dense" and d.S["A_p"].shape == (8, 3, 3)


@pytest.mark.parametrize("name", ["grid4_small", "grid6_large", "bench_32_80"])
def test_observations_are_zero_outside_the_neighbour_table(name):
    """the condition under which compact storage is lossless, on what the (emulated) step kernel writes"""
    topo = {"grid4_small": lambda: tm.TrussTopology.grid(4, "small"), "grid6_large": lambda: tm.TrussTopology.grid(6, "large"),
            "bench_32_80": lambda: synthetic.bench_topology(16, 4)}[name]()
    if name == "bench_32_80":
        assert (topo.N, topo.E) == (32, 80)
    B = 8
    batch = synthetic.random_batch(topo, B, 11)
    env = pc.make_env(pc.emu_lib(), topo, batch)
    env.analyze(set_normalisers=True)
    outside = ~_mask(topo.neighbor_table())
    ag, at = synthetic.random_actions(2, B, topo.N, 12)
    for s in range(2):
        o = env.step(torch.tensor(ag[s]), torch.tensor(at[s]), obs=True)
        for k in ("A_s", "A_n_ts", "A_n_cs"):
            assert o[k].shape == (B, topo.N, topo.N)
            assert int(torch.count_nonzero(o[k][:, outside])) == 0, k
            assert int(torch.count_nonzero(o[k])) > 0, k


def test_pareto_graph_is_zero_outside_the_path_table():
    P = 6
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(P + 1, P, 4, generator=g, dtype=torch.float64)
    n = torch.arange(P + 1, dtype=torch.int32)                       # fronts of 0 .. P members
    index = torch.randint(0, P, (P + 1,), generator=g)
    _, A_p = marl.pareto_graph(pts, n, index, P)
    assert A_p.shape == (P + 1, P, P)
    assert int(torch.count_nonzero(A_p[:, ~_mask(marl.path_graph_table(P))])) == 0
    assert int(torch.count_nonzero(A_p[P])) == 3 * P - 2


def _engine(lib, device, B, num_x, seed=3, **kw):
    topo = tm.TrussTopology.grid(num_x)
    torch.manual_seed(seed)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 16, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)
    eng = marl.BatchedMARL(topo, B, rl, max_front=6, lib=lib, device=device, replay_capacity=256, batch_size=8, seed=seed, **kw)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng


def _shadow(eng):
    """a dense DeviceReplay that receives every `add` of the engine's replay"""
    r = eng.replay
    shadow = marl.DeviceReplay(r.capacity, eng.topo.N, eng.P, eng.device)
    orig = r.add

    def both(*a, **k):
        n = orig(*a, **k)
        assert shadow.add(*a, **k) == n
        return n

    r.add = both
    return shadow


def _check_engine(lib, device, B, num_x):
    with contextlib.redirect_stdout(io.StringIO()):
        eng = _engine(lib, device, B, num_x, replay_storage="compact")
        assert eng.replay.storage == "compact"
        shadow = _shadow(eng)
        for _ in range(3):
            eng.game_step_all(train=True, explore=True, train_iters=1)
    r = eng.replay
    assert r.size >= 1 and (r.size, r.head) == (shadow.size, shadow.head)
    _assert_same_batches(r, shadow, 8, 21, device)
    assert r.nbytes < shadow.nbytes
    return eng


def test_engine_compact_replay_matches_dense_shadow_emulated():
    eng = _check_engine(pc.emu_lib(), "cpu", 6, 4)
    assert eng.replay._lib is None                                    # the emulator has no replay entries: framework indexing
    with pytest.raises(ValueError):
        marl.BatchedMARL(eng.topo, 6, eng.rl, max_front=6, lib=pc.emu_lib(), device="cpu", replay_storage="sparse")


def test_replay_storage_from_environment(monkeypatch):
    monkeypatch.setenv("TRUSS_REPLAY_STORAGE", "compact")
    assert _engine(pc.emu_lib(), "cpu", 6, 4).replay.storage == "compact"
    monkeypatch.delenv("TRUSS_REPLAY_STORAGE")
    assert _engine(pc.emu_lib(), "cpu", 6, 4).replay.storage == "dense"


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

def _prefill(reps, seed):
    """the same earlier contents in every replay's ring (zeros in the unused slots of compact rows, as every append leaves them)"""
    g = torch.Generator().manual_seed(seed)
    a = reps[0]
    names = [("S", k) for k in KEYS] + [(i, k) for i in range(3) for k in KEYS] + [("a_geo",), ("a_topo",), ("R",)]
    for nm in names:
        get = lambda r: getattr(r, nm[0]) if len(nm) == 1 else (r.S if nm[0] == "S" else r.NS[nm[0]])[nm[1]]
        t = torch.randn(get(a).shape, generator=g)
        if len(nm) == 2 and nm[1] in a._tab:
            t = torch.where((a._tab[nm[1]][0] >= 0).cpu()[None], t, torch.zeros(()))
        for r in reps:
            get(r).copy_(t)


def _rings(r):
    return list(r.S.values()) + [t for ns in r.NS for t in ns.values()] + [r.a_geo, r.a_topo, r.R]


CASES = {
    "grid4_wrap": (lambda: tm.TrussTopology.grid(4), 3, 7, 5, 4, 2),
    "bench_32_80": (lambda: synthetic.bench_topology(16, 4), 20, 64, 40, 32, 1),
    "grid128_256_nodes": (lambda: tm.TrussTopology.grid(128), 50, 16, 12, 8, 1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_replay_operators_match_framework_indexing(case):
    make, P, cap, K, batch, rounds = CASES[case]
    topo = make()
    N, nbr, nbr_p = topo.N, topo.neighbor_table(), marl.path_graph_table(P)
    lib = tm.load()
    assert lib.has_replay_ops
    fused = marl.DeviceReplay(cap, N, P, "cuda", storage="compact", nbr=nbr, nbr_p=nbr_p, lib=lib)
    ref = marl.DeviceReplay(cap, N, P, "cuda", storage="compact", nbr=nbr, nbr_p=nbr_p, lib=_NoReplayOps())
    assert fused._lib is lib and ref._lib is None
    _prefill([fused, ref], 40)
    for rnd in range(rounds):
        S, NSall, src, _, ag, at, R = _transitions(K, N, P, nbr, nbr_p, 7 + rnd, "cuda", special=True)
        sel = torch.ones(K, dtype=torch.bool, device="cuda")          # (K rows accepted: K is the case's count)
        if rnd == 0:                                                  # permuted-view actions, next states picked through src
            assert not ag.is_contiguous()
            assert fused.add(sel, S, NSall, ag, at, R, src=src) == ref.add(sel, S, NSall, ag, at, R, src=src) == K
        else:                                                         # three dicts
            NS = _explicit(NSall, src)
            assert fused.add(sel, S, NS, ag, at, R) == ref.add(sel, S, NS, ag, at, R) == K
        assert (fused.size, fused.head) == (ref.size, ref.head)
    if rounds == 2:
        assert fused.head == (2 * K) % cap and fused.size == cap       # wrapped
    else:
        assert fused.size == K < cap                                   # rows [K, cap) were not addressed: earlier contents kept
    for a, b in zip(_rings(fused), _rings(ref)):
        assert _same(a, b)
    _assert_same_batches(fused, ref, batch, 9, "cuda")
    # the gather writes whole dense rows: outputs pre-filled with a sentinel
    i = torch.randint(0, fused.size, (batch,), device="cuda")
    outs = [torch.full((batch,) + fused._dense_shapes[k], -7.5, device="cuda") for _, k, _ in fused._fields]
    outs += [torch.full((batch,) + t.shape[1:], -7.5, device="cuda") for t in (fused.a_geo, fused.a_topo, fused.R)]
    ops.call(ops.namespace().replay_gather, ops.bind(lib), ops.stream_of(i.device), fused._rings, outs, fused._nbrs, i, cap)
    want = [ref._get(ref.S[k], k, i) for k in KEYS] + [ref._get(ref.NS[a][k], k, i) for a in range(3) for k in KEYS]
    want += [ref.a_geo[i], ref.a_topo[i], ref.R[i]]
    for a, b in zip(outs, want):
        assert _same(a, b)


@pytest.mark.gpu
def test_replay_operators_unaligned_rows_of_13_floats():
    """a 13-float field read from / written to views that are 4-byte but not 16-byte aligned: whole 16-byte pieces where a row
    happens to allow them, single words otherwise and for the tail"""
    lib = tm.load()
    ns, lid = ops.namespace(), ops.bind(lib)
    cap, K, k, head = 11, 9, 6, 8
    g = torch.Generator().manual_seed(2)
    base = torch.randn(1 + K * 13 + 3, generator=g).cuda()
    src = base[1:1 + K * 13].view(K, 13)
    assert src.data_ptr() % 16 == 4
    two = torch.randn(3, K, 25, generator=g).cuda()[:, :, 1:].view(3, K, 2, 12).permute(1, 0, 2, 3)   # [K, 3, 2, 12] strided over dims 0 and 1
    assert two.data_ptr() % 16 == 4 and not two.is_contiguous()
    ring = torch.randn(cap, 13, generator=g).cuda()
    ring2 = torch.randn(cap, 3, 2, 12, generator=g).cuda()
    want, want2 = ring.clone(), ring2.clone()
    rows = torch.tensor([7, 0, 3, 3, 8, 1], device="cuda")
    rows4 = torch.stack([rows, rows.flip(0), rows, rows])
    pos = (head + torch.arange(k, device="cuda")) % cap
    want[pos] = src[rows]
    want2[pos] = two[rows.flip(0)]
    ops.call(ns.replay_scatter, lid, ops.stream_of(torch.device("cuda")), [ring, ring2], [src, two], [None, None], [0, 1], rows4, k, head, cap)
    assert _same(ring, want) and _same(ring2, want2)
    i = torch.tensor([10, 8, 2, 8, 0], device="cuda")
    obase = torch.full((2 + 5 * 13 + 5,), -7.5, device="cuda")
    out = obase[2:2 + 5 * 13].view(5, 13)
    out2 = torch.full((5, 3, 2, 12), -7.5, device="cuda")
    ops.call(ns.replay_gather, lid, ops.stream_of(torch.device("cuda")), [ring, ring2], [out, out2], [None, None], i, cap)
    assert _same(out, want[i]) and _same(out2, want2[i])
    assert bool((obase[:2] == -7.5).all()) and bool((obase[2 + 5 * 13:] == -7.5).all())          # nothing beyond the view


@pytest.mark.gpu
def test_replay_operator_argument_checks():
    lib = tm.load()
    ns, lid = ops.namespace(), ops.bind(lib)
    N, cap, K = 20, 6, 4
    nbr = torch.full((N, 17), -1, dtype=torch.int16, device="cuda")
    nbr[:, 0] = torch.arange(N)
    ring = torch.rand(cap, N, 17, device="cuda")
    keep = ring.clone()
    src = torch.rand(K, N, N, device="cuda")
    rows = torch.arange(K, device="cuda")[None].expand(4, K).contiguous()
    with pytest.raises(TrussError, match="k_nbr"):
        ops.call(ns.replay_scatter, lid, ops.stream_of(torch.device("cuda")), [ring], [src], [nbr], [0], rows, K, 0, cap)
    out = torch.full((K, N, N), -7.5, device="cuda")
    with pytest.raises(TrussError, match="k_nbr"):
        ops.call(ns.replay_gather, lid, ops.stream_of(torch.device("cuda")), [ring], [out], [nbr], torch.arange(K, device="cuda"), cap)
    torch.cuda.synchronize()
    assert torch.equal(ring, keep) and bool((out == -7.5).all())
    with pytest.raises(TrussError):                                    # k > capacity
        big = torch.arange(cap + 1, device="cuda")[None].expand(4, cap + 1).contiguous()
        ops.call(ns.replay_scatter, lid, ops.stream_of(torch.device("cuda")), [ring[:, :, :16].contiguous()], [torch.rand(cap + 1, N, N, device="cuda")], [nbr[:, :16].contiguous()],
                 [0], big, cap + 1, 0, cap)
    with pytest.raises(TrussError):                                    # head out of range
        ops.call(ns.replay_scatter, lid, ops.stream_of(torch.device("cuda")), [keep[:, :, :16].contiguous()], [src], [nbr[:, :16].contiguous()], [0], rows, K, cap, cap)
    # no fields: nothing to do
    ops.call(ns.replay_scatter, lid, ops.stream_of(torch.device("cuda")), [], [], [], [], rows, K, 0, cap)
    ops.call(ns.replay_gather, lid, ops.stream_of(torch.device("cuda")), [], [], [], torch.arange(K, device="cuda"), cap)
    torch.cuda.synchronize()
    assert torch.equal(ring, keep)


@pytest.mark.gpu
def test_replay_gather_in_a_captured_graph():
    topo = tm.TrussTopology.grid(4)
    N, P, cap, batch = topo.N, 3, 16, 6
    nbr, nbr_p = topo.neighbor_table(), marl.path_graph_table(P)
    lib = tm.load()
    rep = marl.DeviceReplay(cap, N, P, "cuda", storage="compact", nbr=nbr, nbr_p=nbr_p, lib=lib)
    S, NSall, src, _, ag, at, R = _transitions(cap, N, P, nbr, nbr_p, 5, "cuda")
    rep.add(torch.ones(cap, dtype=torch.bool, device="cuda"), S, NSall, ag, at, R, src=src)
    ns, lid = ops.namespace(), ops.bind(lib)
    mk = lambda: [torch.full((batch,) + rep._dense_shapes[k], -7.5, device="cuda") for _, k, _ in rep._fields] + \
        [torch.full((batch,) + t.shape[1:], -7.5, device="cuda") for t in (rep.a_geo, rep.a_topo, rep.R)]
    idx, outs = torch.zeros(batch, dtype=torch.int64, device="cuda"), mk()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # (warm-up outside the capture)
        ops.call(ns.replay_gather, lid, ops.stream_of(idx.device), rep._rings, outs, rep._nbrs, idx, cap)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.call(ns.replay_gather, lid, ops.stream_of(idx.device), rep._rings, outs, rep._nbrs, idx, cap)
    new = torch.tensor([3, 15, 0, 7, 7, 9], device="cuda")
    idx.copy_(new)
    graph.replay()
    eager = mk()
    ops.call(ns.replay_gather, lid, ops.stream_of(idx.device), rep._rings, eager, rep._nbrs, new, cap)
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert _same(a, b)
    assert _same(outs[1], S["A_s"][new])


@pytest.mark.gpu
def test_engine_compact_replay_matches_dense_shadow_hip():
    eng = _check_engine(tm.load(), "cuda", 64, 8)
    assert eng.replay._lib is not None                                 # the fused operators did run


@pytest.mark.gpu
def test_mixed_engine_compact_replay_matches_dense_shadows_hip():
    lib = tm.load()
    torch.manual_seed(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 16, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda")
    classes = pool.grid_classes([4, 6], [48, 32])                      # 8 and 12 nodes
    eng = marl.MixedMARL(classes, rl, bucket_envs=8, max_front=6, lib=lib, device="cuda", replay_capacity=256, batch_size=8, seed=2,
                         replay_storage="compact")
    per_class = []
    for k, e in enumerate(eng.engines):
        full = synthetic.random_batch(e.topo, classes[eng.class_ids[k]][1], 9 + k)
        per_class.append({key: v[eng.global_ids(k)] for key, v in full.items()})
    eng.reset(per_class)
    shadows = [_shadow(e) for e in eng.engines]
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(3):
            eng.game_step_all(train=True, explore=True, train_iters=2)
    assert [e.topo.N for e in eng.engines] == [8, 12]
    for e, sh in zip(eng.engines, shadows):
        assert e.replay.storage == "compact" and e.replay._lib is not None and e.replay.size >= 1
        assert (e.replay.size, e.replay.head) == (sh.size, sh.head)
        _assert_same_batches(e.replay, sh, 8, 22, "cuda")
        assert e.replay.nbytes < sh.nbytes


@pytest.mark.gpu
def test_fused_dense_replay_matches_indexing():
    """DeviceReplay(fused=True): dense storage through the same two launches (plain fields only)"""
    topo = tm.TrussTopology.grid(6)
    N, P, cap, K = topo.N, 5, 16, 10
    nbr, nbr_p = topo.neighbor_table(), marl.path_graph_table(P)
    f, d = marl.DeviceReplay(cap, N, P, "cuda", fused=True, lib=tm.load()), marl.DeviceReplay(cap, N, P, "cuda")
    assert f._lib is not None and d._lib is None
    for seed in (1, 2):
        S, NSall, src, sel, ag, at, R = _transitions(K, N, P, nbr, nbr_p, seed, "cuda")
        assert f.add(sel, S, NSall, ag, at, R, src=src) == d.add(sel, S, NSall, ag, at, R, src=src)
    assert (f.size, f.head) == (d.size, d.head)
    for a, b in zip(_rings(f), _rings(d)):
        assert _same(a, b)
    _assert_same_batches(f, d, 8, 3, "cuda")
    with pytest.raises(TrussError):
        marl.DeviceReplay(cap, N, P, "cpu", fused=True)
