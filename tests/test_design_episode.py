"""The design game of the reference's test copies on the batched engine (`BatchedMARL(..., game="test")`, truss_mi355/marl.py):
symmetry coin per move (D6), one cull per game step over up to 4 x 50 rows, untruncated final cull, G_U.

Action replay: the actions the engine's actors produced are recorded (BatchedMARL._act) and replayed through a host model of
the test game built from the float64 oracle (oracle.env_step, with the same coin function), the drop-in culls
(utils.simple_cull_final + the D3 truncation, restated here) and the host reward block -- the actors' own numerics stay
out of the comparison."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import marl, reward as RW, synthetic
import parity_common as pc
from oracle import truss_oracle as O
import utils as U
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL


# ---- the coin, restated in numpy (uint64 arithmetic) ----
def _sm64(z):
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _coins(seed, env, step, member):
    """[K, 3] uint8: top bit of splitmix64(splitmix64(seed) ^ (env << 26 | step << 10 | member << 2 | agent))"""
    key = ((np.asarray(env, np.uint64)[:, None] << np.uint64(26)) | np.uint64(step << 10)
           | (np.asarray(member, np.uint64)[:, None] << np.uint64(2)) | np.arange(3, dtype=np.uint64)[None, :])
    return (_sm64(key ^ _sm64(np.array([seed], np.uint64))) >> np.uint64(63)).astype(np.uint8)


def test_coin_matches_numpy_restatement():
    env, mem = np.arange(0, 5000, 7), np.arange(0, 5000, 7) % 50
    got = marl.design_coins(12345, torch.tensor(env), 17, torch.tensor(mem)).numpy()
    np.testing.assert_array_equal(got, _coins(12345, env, 17, mem))
    assert 0.45 < got.mean() < 0.55


# ---- engine + host model ----
def _rl(device, hidden, seed):
    torch.manual_seed(seed)
    return RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, hidden, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)


def _engine(lib, device, topo, B, seed=3, hidden=16, rl=None, **kw):
    rl = rl or _rl(device, hidden, seed)
    eng = marl.BatchedMARL(topo, B, rl, lib=lib, device=device, seed=seed, game="test", **kw)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng, b


def _record(eng):
    """wrap the engine's actors and cull: actions per game step (chunks in order), archive after every cull"""
    rec = dict(act={}, arch=[], cull_in=[])
    act0, cull0 = eng._act, eng._design_cull

    def act(S, explore):
        g, t = act0(S, explore)
        rec["act"].setdefault(eng.game_step, []).append(([x.detach().cpu().numpy().copy() for x in g],
                                                         [x.detach().cpu().numpy().copy() for x in t]))
        return g, t

    def cull(candP, candY, candS, final):
        rec["cull_in"].append((eng.pts.clone(), eng.n.clone(), candP.clone(), final))
        out = cull0(candP, candY, candS, final)
        rec["arch"].append((eng.pts.cpu().numpy().copy(), eng.n.cpu().numpy().copy(), eng.arch_y.cpu().numpy().copy(),
                            eng.arch_sec.cpu().numpy().copy()))
        return out

    eng._act, eng._design_cull = act, cull
    return rec


def _d3(rows, order, max_front):
    """D3: both ends + the max_front - 2 interior rows of largest crowding distance (ties: earlier position), in front order"""
    nf = len(order)
    if max_front is None or nf <= max_front:
        return order
    f = [rows[k] for k in order]
    d = [math.sqrt((f[k][0] - f[k + 1][0]) ** 2 + (f[k][1] - f[k + 1][1]) ** 2) for k in range(nf - 1)]
    cr = [d[0]] + [d[k - 1] + d[k] for k in range(1, nf - 1)] + [d[-1]]
    keep = {0, nf - 1} | set(sorted(range(1, nf - 1), key=lambda k: -cr[k])[:max_front - 2])
    return [order[k] for k in range(nf) if k in keep]


def _host_cull(rows, max_front):
    """rows: list of [o1, o2, c1, c2] (feasible ones only matter) -> input rows of the front in the kernel's order
    (obj1, obj2, first of identical rows), truncated by D3 unless max_front is None"""
    feas = [k for k, r in enumerate(rows) if not (r[2] > 1 or r[3] > 1)]
    fr = U.simple_cull_final([list(rows[k]) for k in feas])[0]
    first = {}
    for k in feas:
        first.setdefault(tuple(rows[k]), k)
    order = sorted((first[tuple(r)] for r in fr), key=lambda k: (rows[k][0], rows[k][1], k))
    return _d3(rows, order, max_front)


def _host_episode(topo, batch, rec, seed, P, T):
    """the test game replayed on the host: per step (archive, n, y, sec, R, G_U), final front"""
    ot = pc.oracle_topology(topo)
    load = pc.oracle_load(ot, batch)
    B = batch["y"].shape[0]
    int_obj = O.initial_objectives(ot, batch["x"], batch["y"], batch["sec"], batch["target"])
    arch = [[(np.array([1.0, 1.0, 0.0, 0.0]), batch["y"][b], batch["sec"][b])] for b in range(B)]
    R, GU, steps, final = np.zeros((B, 3)), np.zeros(B), [], None
    tied = np.zeros(B, bool)
    pick = lambda a, idx: np.asarray(a)[idx] if np.ndim(a) else a
    for s in range(T):
        gs = s + 1
        n0 = [len(a) for a in arch]
        pairs = [(m, b) for m in range(max(n0)) for b in range(B) if m < n0[b]]      # the engine's member-major pair order
        pm, pb = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        chunks = rec["act"][gs]
        geo = [np.concatenate([c[0][a] for c in chunks]) for a in range(3)]
        top = [np.concatenate([c[1][a] for c in chunks]) for a in range(3)]
        assert geo[0].shape[0] == len(pairs)
        coin = _coins(seed, pb, gs, pm)
        py = np.stack([arch[b][m][1] for m, b in pairs])
        ps = np.stack([arch[b][m][2] for m, b in pairs])
        outs = [O.env_step(ot, batch["x"][pb], py, ps, None, None, geo[a], top[a], coin[:, a].astype(np.float64), batch["target"][pb],
                           load[pb], pick(batch["y_max"], pb), pick(batch["d_min"], pb), pick(batch["max_def"], pb),
                           pick(batch["is_roof"], pb), int_obj[pb]) for a in range(3)]
        cand = {}
        for k, (m, b) in enumerate(pairs):
            front = [list(r[0]) for r in arch[b]]
            pts3 = [list(np.asarray(outs[a]["point"][k], np.float64)) for a in range(3)]
            r0, r1, r2, gu = M.difference_reward(front, front, tuple(arch[b][m][0][:2]), pts3, [1.0, 1.0], n0[b])[:4]
            x1 = [r[0] for r in front] + [p[0] for p in pts3 if max(p) <= 1.0]
            tied[b] |= len(set(x1)) < len(x1) or len(x1) > P          # ... or a front the host truncates with random.sample (D3)
            R[b] += (r0, r1, r2)
            GU[b] += gu
            for a in range(3):
                cand[(b, m, a)] = (np.array(pts3[a]), outs[a]["y"][k], outs[a]["sec"][k])
        last = gs == T
        new = []
        for b in range(B):
            rows = list(arch[b]) + [cand[(b, m, a)] for m in range(n0[b]) for a in range(3)]
            keep = _host_cull([list(r[0]) for r in rows], None if last else P)
            fr = [(np.concatenate([np.minimum(rows[k][0][:2], 1.0), rows[k][0][2:]]), rows[k][1], rows[k][2]) for k in keep]
            new.append(fr)
        if last:
            final = new
        else:
            arch = new
        steps.append([list(a) for a in new])
    return steps, final, R, GU, tied


def _check_replay(lib, device, topo, B, end_step, pair_capacity=None):
    eng, batch = _engine(lib, device, topo, B, pair_capacity=pair_capacity)
    rec = _record(eng)
    with contextlib.redirect_stdout(io.StringIO()):
        out = eng.design_episode(end_step=end_step, explore=False)
    T = end_step
    assert out["hv"].shape == (T, B) and out["n_front"].shape == (T, B) and len(rec["arch"]) == T
    old = U.MAX_FRONT
    U.MAX_FRONT = eng.P                                # the test copies' MAX_FRONT (truss2D_ENV.configure) in the host reward block
    try:
        steps, final, R, GU, tied = _host_episode(topo, batch, rec, eng.seed, eng.P, T)
    finally:
        U.MAX_FRONT = old
    hv, nf = out["hv"].cpu().numpy(), out["n_front"].cpu().numpy()
    for t in range(T - 1):
        pts, n, y, sec = rec["arch"][t]
        for b in range(B):
            want = steps[t][b]
            assert n[b] == len(want) == nf[t, b], (t, b)
            np.testing.assert_allclose(pts[b, :n[b]], np.stack([w[0] for w in want]), rtol=0, atol=1e-9, err_msg=f"step {t} env {b}")
            np.testing.assert_array_equal(y[b, :n[b]], np.stack([w[1] for w in want]).astype(np.float32))
            np.testing.assert_array_equal(sec[b, :n[b]], np.stack([w[2] for w in want]))
            # the HV of the kernel against the drop-in's on the same archive points
            assert abs(hv[t, b] - U.union_rectangles_fastest([list(r) for r in pts[b, :n[b]]], +1, -1, ref_point=[1, 1])) <= 1e-12
    fin = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out["final"].items()}
    assert fin["points"].shape == (B, 4 * eng.P, 4)
    for b in range(B):
        want = final[b]
        n = fin["n"][b]
        assert n == len(want) == nf[T - 1, b], b
        np.testing.assert_allclose(fin["points"][b, :n], np.stack([w[0] for w in want]), rtol=0, atol=1e-9)
        np.testing.assert_array_equal(fin["y"][b, :n], np.stack([w[1] for w in want]).astype(np.float32))
        np.testing.assert_array_equal(fin["sec"][b, :n], np.stack([w[2] for w in want]))
        assert np.all(fin["points"][b, n:] == 0)
        assert abs(hv[T - 1, b] - U.union_rectangles_fastest([list(r) for r in fin["points"][b, :n]], +1, -1, ref_point=[1, 1])) <= 1e-12
    # the reward's front metrics (std_cd, sum_distance) depend on the order of rows with EQUAL obj1 (clipped archive rows at 1.0),
    # which the reference leaves to Python's set iteration (utils.py:53-60), and on the host's random truncation of fronts longer
    # than MAX_FRONT (D3): R and G_U are compared on the envs where neither occurred
    ok = ~tied
    assert ok.sum() >= B // 8
    np.testing.assert_allclose(out["R"].cpu().numpy()[ok], R[ok], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["G_U"].cpu().numpy()[ok], GU[ok], rtol=0, atol=1e-9)
    assert torch.isfinite(out["R"]).all() and torch.isfinite(out["G_U"]).all()
    assert int(nf[:-1].max()) >= 2                     # the archives grew
    return eng, out


def test_design_replay_emulated():
    _check_replay(pc.emu_lib(), "cpu", tm.TrussTopology.grid(4, "small"), 6, 5, pair_capacity=8)


def test_design_replay_large_emulated():
    _check_replay(pc.emu_lib(), "cpu", tm.TrussTopology.grid(6, "large"), 4, 4)


def test_engine_rejects_bad_game_emulated():
    rl = _rl("cpu", 16, 0)
    with pytest.raises(ValueError):
        marl.BatchedMARL(tm.TrussTopology.grid(4), 2, rl, lib=pc.emu_lib(), device="cpu", game="test")    # no mirror tables
    with pytest.raises(ValueError):
        marl.BatchedMARL(tm.TrussTopology.grid(4, "small"), 2, rl, lib=pc.emu_lib(), device="cpu", game="test", max_front=65)
    eng, _ = _engine(pc.emu_lib(), "cpu", tm.TrussTopology.grid(4, "small"), 2)
    assert eng.P == 50 and eng.Gm == 50
    with pytest.raises(ValueError):
        eng.game_step_all(train=True)
    tr = marl.BatchedMARL(tm.TrussTopology.grid(4, "small"), 2, rl, lib=pc.emu_lib(), device="cpu")
    assert tr.game == "train" and tr.P == 20 and tr.Gm == 14


@pytest.mark.gpu
@pytest.mark.parametrize("num_x,variant,end_step", [(8, "small", 6), (16, "large", 5)])
def test_design_replay_hip(num_x, variant, end_step):
    """01_small_roof and 02_large_bridge layouts, B = 64, explore off"""
    _check_replay(tm.load(), "cuda", tm.TrussTopology.grid(num_x, variant), 64, end_step)


def _mirrored(topo, y, sec):
    """[K] bool: every mirror pair of the variant's tables holds equal heights and sections"""
    sn, se = topo.sym_nodes, topo.sym_elems
    return (y[:, sn[:, 0]] == y[:, sn[:, 1]]).all(axis=1) & (sec[:, se[:, 0]] == sec[:, se[:, 1]]).all(axis=1)


@pytest.mark.gpu
def test_design_episode_properties_hip():
    topo = tm.TrussTopology.grid(8, "small")
    B, T = 4096, 8
    eng, batch = _engine(tm.load(), "cuda", topo, B, seed=11, hidden=32)
    rec = _record(eng)
    coins = []
    orig = marl.design_coins
    marl.design_coins = lambda *a: coins.append(orig(*a)) or coins[-1]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            out = eng.design_episode(end_step=T, explore=True)
    finally:
        marl.design_coins = orig
    c = torch.cat([x.flatten() for x in coins]).float()
    assert c.numel() > 100000 and abs(float(c.mean()) - 0.5) < 0.01
    nf = out["n_front"].cpu().numpy()
    assert nf[:-1].min() >= 1 and nf[:-1].max() <= 50 and nf[:-1].max() == 50
    for t in range(T - 1):
        pts, n, y, sec = rec["arch"][t]
        live = np.arange(eng.P)[None, :] < n[:, None]
        assert np.isfinite(pts[live]).all() and np.all(pts[live][:, :2] <= 1.0) and np.all(pts[live][:, 2:] <= 1.0)
        moved = live & ~(pts[:, :, 2] == 0.0) & ~(pts[:, :, 3] == 0.0)          # not the reset design [1, 1, 0, 0]
        moved &= ~np.all(y == batch["y"][:, None, :].astype(np.float32), axis=2)
        assert moved.sum() > 0 and _mirrored(topo, y[moved], sec[moved]).all(), t
    for k in ("hv", "R", "G_U"):
        assert torch.isfinite(out[k]).all(), k
    fin = out["final"]
    assert int(fin["n"].max()) > 50                    # untruncated: the final front may exceed MAX_FRONT
    pts0, n0, candP, final = rec["cull_in"][-1]
    assert final
    pts0, n0, candP = pts0.cpu().numpy(), n0.cpu().numpy(), candP.cpu().numpy()
    fp, fn = fin["points"].cpu().numpy(), fin["n"].cpu().numpy()
    for b in np.random.default_rng(0).choice(B, 48, replace=False):
        rows = [list(r) for r in pts0[b, :n0[b]]] + [list(r) for r in candP[b]]
        fr = U.simple_cull_final([r for r in rows if not (r[2] > 1 or r[3] > 1)])[0]
        got = sorted(tuple(r) for r in fp[b, :fn[b]])
        want = sorted((min(r[0], 1.0), min(r[1], 1.0), r[2], r[3]) for r in fr)
        assert got == want, b


@pytest.mark.gpu
def test_design_episode_pair_capacity_invariance_hip():
    """explore off: the episode does not depend on how the pairs are chunked.  Actor inference runs per (env, member) pair in
    the fused GCN kernels, so archives, HV and the final front are compared bitwise."""
    topo = tm.TrussTopology.grid(8, "small")
    outs = []
    for cap in (None, 300):
        eng, _ = _engine(tm.load(), "cuda", topo, 256, seed=5, pair_capacity=cap)
        with contextlib.redirect_stdout(io.StringIO()):
            outs.append(eng.design_episode(end_step=6, explore=False))
    a, b = outs
    assert torch.equal(a["n_front"], b["n_front"])
    assert torch.equal(a["hv"], b["hv"])
    # R and G_U are per-env sums over (member, agent) rows (index_add_: float64 atomics, chunk-dependent order): equal to rounding
    for k in ("R", "G_U"):
        torch.testing.assert_close(a[k], b[k], rtol=1e-12, atol=1e-12)
    for k in ("points", "y", "sec", "n"):
        assert torch.equal(a["final"][k], b["final"][k]), k


@pytest.mark.gpu
def test_design_coin_matters_hip():
    topo = tm.TrussTopology.grid(8, "small")
    res = []
    orig = marl.design_coins
    for force in (False, True):
        eng, _ = _engine(tm.load(), "cuda", topo, 128, seed=9)
        if force:
            marl.design_coins = lambda *a: torch.zeros_like(orig(*a))
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                res.append(eng.design_episode(end_step=4, explore=False))
        finally:
            marl.design_coins = orig
    assert not torch.equal(res[0]["final"]["y"], res[1]["final"]["y"])
    assert not torch.equal(res[0]["hv"], res[1]["hv"])


@pytest.mark.gpu
def test_mixed_design_episode_hip():
    """two "large" classes, each with its own symmetric topology; coins keyed by global env ids"""
    classes = [(tm.TrussTopology.grid(4, "large"), 40), (tm.TrussTopology.grid(8, "large"), 24)]
    rl = _rl("cuda", 16, 4)
    mix = marl.MixedMARL(classes, rl, bucket_envs=8, lib=tm.load(), device="cuda", game="test", seed=4)
    assert [e.env_ids.tolist() for e in mix.engines] == [list(range(40)), list(range(40, 64))]
    per = []
    for k, e in enumerate(mix.engines):
        b = synthetic.random_batch(e.topo, e.B, 20 + k)
        per.append(dict(b))
    mix.reset(per)
    calls = []
    orig = RW.difference_reward

    def spy(*a, **kw):
        o = orig(*a, **kw)
        calls.append(([t.clone() if torch.is_tensor(t) else t for t in a], [x.clone() for x in o]))
        return o

    marl.RW.difference_reward = spy
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            out = mix.design_episode(end_step=4, explore=True)
    finally:
        marl.RW.difference_reward = orig
    assert out["hv"].shape == (4, 64) and out["R"].shape == (64, 3) and out["G_U"].shape == (64,)
    for e, o in zip(mix.engines, out["per_class"]):
        nf = o["n_front"].cpu().numpy()
        assert nf[:-1].min() >= 1 and nf[:-1].max() <= 50
        assert torch.isfinite(o["hv"]).all() and torch.isfinite(o["R"]).all()
        n = e.n.cpu().numpy()
        pts = e.pts.cpu().numpy()
        for b in range(e.B):
            rows = pts[b, :n[b]]
            assert list(rows[:, 0]) == sorted(rows[:, 0])
            assert not any(rows[j, 0] < rows[i, 0] and rows[j, 1] < rows[i, 1] for i in range(n[b]) for j in range(n[b]))
    for args, outs in (calls[0], calls[-1]):
        front, nf_, pf, npf, parent, points, ref, n_pf = [a.cpu().numpy() if torch.is_tensor(a) else a for a in args[:8]]
        for b in range(0, front.shape[0], 5):
            want = M.difference_reward([list(r) for r in front[b, :nf_[b]]], [list(r) for r in pf[b, :npf[b]]], tuple(parent[b]),
                                       [list(p) for p in points[b]], list(ref[b]), int(n_pf[b]))
            np.testing.assert_allclose(outs[0][b].cpu().numpy(), want[:3], rtol=1e-9, atol=1e-11)
            np.testing.assert_allclose(float(outs[1][b]), want[3], rtol=1e-9, atol=1e-11)
