"""The compact observation layout downstream of the kernels: `DeviceReplay.add(compact_in=True)` and `BatchedMARL(obs_layout=
"compact")`.  Nothing may change but the layout in which the node-graph adjacencies travel: a replay fed compact-in rows holds the
rings of one fed the dense rows, and an engine that observes compactly plays the game of the dense engine bit for bit -- archives,
rewards, replay rings, sampled batches -- in the train game (with updates) and in the design game.  On the CPU through the lane
emulator (layers expanded on the host, framework replay), on the GPU with every native path on."""
import contextlib
import io

import pytest
import torch

import master_DDPG_truss2D_MO as M
import parity_common as pc
import test_replay_compact as TR
import truss2D_RL as RL
import truss_mi355 as tm
from truss_mi355 import marl, ops, synthetic

KEYS = marl.DeviceReplay.KEYS
NODE = marl.DeviceReplay.NODE_GRAPH_KEYS


def _gather(t, nbr):
    """dense [.., N, N] -> compact [.., N, Kc]: the layout's definition"""
    nb = torch.as_tensor(nbr).to(t.device)
    got = t.gather(-1, nb.clamp(min=0).long().expand(t.shape[:-1] + (nb.shape[1],)))
    return torch.where(nb >= 0, got, torch.zeros((), device=t.device)).contiguous()


def _compact_rows(d, nbr):
    return {k: _gather(v, nbr) if k in NODE else v for k, v in d.items()}


def _rings(r):
    return list(r.S.values()) + [t for ns in r.NS for t in ns.values()] + [r.a_geo, r.a_topo, r.R]


def _same_rings(a, b):
    assert (a.size, a.head) == (b.size, b.head)
    for i, (x, y) in enumerate(zip(_rings(a), _rings(b))):
        assert TR._same(x, y), i


def _check_replay(device, lib=None):
    topo = tm.TrussTopology.grid(4)
    N, P = topo.N, 3
    nbr, nbr_p = topo.neighbor_table(), marl.path_graph_table(P)
    mk = lambda: marl.DeviceReplay(7, N, P, device, storage="compact", nbr=nbr, nbr_p=nbr_p, lib=lib)
    dense_in, compact_in = mk(), mk()
    for seed, explicit in ((1, False), (2, True), (3, False)):                       # 7 slots: the third append wraps
        S, NSall, src, sel, ag, at, R = TR._transitions(5, N, P, nbr, nbr_p, seed, device, special=True)
        Sc, NSc = _compact_rows(S, nbr), _compact_rows(NSall, nbr)
        if explicit:
            n = dense_in.add(sel, S, TR._explicit(NSall, src), ag, at, R)
            assert compact_in.add(sel, Sc, TR._explicit(NSc, src), ag, at, R, compact_in=True) == n
        else:
            n = dense_in.add(sel, S, NSall, ag, at, R, src=src)
            assert compact_in.add(sel, Sc, NSc, ag, at, R, src=src, compact_in=True) == n
    _same_rings(dense_in, compact_in)
    TR._assert_same_batches(dense_in, compact_in, 16, 5, device)
    return topo, (S, NSall, src, sel, ag, at, R), (Sc, NSc)


def test_replay_compact_in_matches_dense_in():
    topo, (S, NSall, src, sel, ag, at, R), (Sc, NSc) = _check_replay("cpu")
    N, P = topo.N, 3
    nbr, nbr_p = topo.neighbor_table(), marl.path_graph_table(P)
    with pytest.raises(ValueError, match="compact_in needs storage='compact'"):
        marl.DeviceReplay(7, N, P, "cpu").add(sel, Sc, NSc, ag, at, R, src=src, compact_in=True)
    c = marl.DeviceReplay(7, N, P, "cpu", storage="compact", nbr=nbr, nbr_p=nbr_p)
    with pytest.raises(ValueError, match="compact_in: A_s must end in"):              # dense rows announced as compact
        c.add(sel, S, NSall, ag, at, R, src=src, compact_in=True)
    assert c.size == 0


# ---- the engine ----
def _engine(lib, device, B, topo, seed=3, game="train", **kw):
    torch.manual_seed(seed)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 16, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)
    eng = marl.BatchedMARL(topo, B, rl, max_front=6, lib=lib, device=device, replay_capacity=256, batch_size=8, seed=seed, game=game, **kw)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng


def _play(lib, device, B, topo, layout, steps, game="train", **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        rs = {} if game == "test" else dict(replay_storage="compact")
        eng = _engine(lib, device, B, topo, game=game, obs_layout=layout, **rs, **kw)
        assert eng.obs_layout == layout
        outs = [eng.game_step_all(train=game == "train", explore=True, train_iters=1) for _ in range(steps)]
    return eng, outs


def _same_game(a, b, oa, ob, device, train=True, min_replay=1):
    for x, y in ((a.pts, b.pts), (a.arch_y, b.arch_y), (a.arch_sec, b.arch_sec), (a.n, b.n), (a.ref_points, b.ref_points)):
        assert torch.equal(x, y)
    for u, v in zip(oa, ob):
        for k in ("hv", "n_front", "reward"):
            assert torch.equal(u[k], v[k]), k
        assert u["replay_added"] == v["replay_added"]
        if "G_U" in u:
            assert torch.equal(u["G_U"], v["G_U"])
    if train:
        assert a.replay.size >= min_replay
        _same_rings(a.replay, b.replay)
        if a.replay.size:
            TR._assert_same_batches(a.replay, b.replay, 8, 21, device)
        for pa, pb in zip((p for ag in a.rl.agents for p in ag.actor_model.parameters()), (p for ag in b.rl.agents for p in ag.actor_model.parameters())):
            assert torch.equal(pa, pb)                                                        # ... and the same updates came of it


def test_engine_compact_equals_dense_emulated():
    lib = pc.emu_lib()
    topo = tm.TrussTopology.grid(4)
    d, od = _play(lib, "cpu", 6, topo, "dense", 3)
    c, oc = _play(lib, "cpu", 6, topo, "compact", 3)
    assert c.envP.obs_buffers("compact")["A_s"].shape[2] == topo.neighbor_table().shape[1] < topo.N
    _same_game(d, c, od, oc, "cpu")


def test_design_game_compact_equals_dense_emulated():
    lib = pc.emu_lib()
    topo = tm.TrussTopology.grid(4, "small")
    d, od = _play(lib, "cpu", 4, topo, "dense", 2, game="test")
    c, oc = _play(lib, "cpu", 4, topo, "compact", 2, game="test")
    _same_game(d, c, od, oc, "cpu", train=False)


def test_engine_option_and_refusals(monkeypatch):
    lib = pc.emu_lib()
    topo = tm.TrussTopology.grid(4)
    with contextlib.redirect_stdout(io.StringIO()):
        assert _engine(lib, "cpu", 4, topo).obs_layout == "dense"                              # the default
        with pytest.raises(ValueError, match="replay_storage='compact'"):                      # a training engine with a dense replay
            _engine(lib, "cpu", 4, topo, obs_layout="compact")
        with pytest.raises(ValueError, match="obs_layout must be"):
            _engine(lib, "cpu", 4, topo, obs_layout="csr")
        monkeypatch.setenv("TRUSS_OBS_LAYOUT", "compact")
        assert _engine(lib, "cpu", 4, topo, replay_storage="compact").obs_layout == "compact"
        assert _engine(lib, "cpu", 4, topo, replay_storage="compact", obs_layout="dense").obs_layout == "dense"   # the argument wins
        monkeypatch.delenv("TRUSS_OBS_LAYOUT")
        monkeypatch.setattr(lib, "has_obs_compact", False)
        with pytest.raises(ValueError, match="truss_topo_neighbors"):
            _engine(lib, "cpu", 4, topo, replay_storage="compact", obs_layout="compact")


# ---- the same on the hardware ----
@pytest.mark.gpu
def test_replay_scatter_compact_in_hip():
    """the fused append: compact-in fields travel as plain fields of `replay_scatter`; the rings equal the dense-in rings bit for bit"""
    lib = tm.load()
    assert lib.has_replay_ops
    _check_replay("cuda", lib)


NATIVE = dict(pair_path="hip", archive_path="hip", reward_path="hip", actor_path="grouped")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small_roof eager", "small_roof replayed", "64 nodes replayed"])
def test_engine_compact_equals_dense_hip(case):
    """compact against dense with all native paths on: the same game bit for bit over 3 steps with training, the update eager and
    replayed from its captured graph (it reads dense samples either way).  (The random 64-node designs have no feasible candidate
    within three steps: that game appends nothing and so never updates; its archives, rewards and empty rings are compared, the
    replay and the updates are exercised by the small_roof cases.)"""
    lib = tm.load()
    topo, B = (tm.TrussTopology.grid(32), 3) if case.startswith("64") else (tm.TrussTopology.grid(8, "small"), 6)
    games = []
    for layout in ("dense", "compact"):
        with contextlib.redirect_stdout(io.StringIO()):
            eng = _engine(lib, "cuda", B, topo, obs_layout=layout, replay_storage="compact", tune_update_gemms=False, **NATIVE)
            eng.use_train_graph = case.endswith("replayed")
            outs = [eng.game_step_all(train=True, explore=True, train_iters=1) for _ in range(3)]
        torch.cuda.synchronize()
        games.append((eng, outs))
    (d, od), (c, oc) = games
    assert c.envC.obs_buffers("compact")["A_s"].shape[2] == topo.neighbor_table().shape[1] and c.envC.N == topo.N
    _same_game(d, c, od, oc, "cuda", min_replay=0 if case.startswith("64") else 1)


@pytest.mark.gpu
def test_design_game_compact_equals_dense_hip():
    lib = tm.load()
    topo = tm.TrussTopology.grid(8, "small")
    kw = dict(tune_update_gemms=False, **NATIVE)
    d, od = _play(lib, "cuda", 6, topo, "dense", 2, game="test", **kw)
    c, oc = _play(lib, "cuda", 6, topo, "compact", 2, game="test", **kw)
    torch.cuda.synchronize()
    _same_game(d, c, od, oc, "cuda", train=False)
