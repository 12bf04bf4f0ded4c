"""The difference reward of a game step as one launch (`truss_reward`, csrc/truss_reward.h; reward.difference_reward(path="hip"),
BatchedMARL(reward_path="hip")): against the per-env host path, against the existing batched path (three truss_front launches +
torch operators) on the same device, bounds / reproducibility, argument checks, the engine switch.

Tolerances.  Against the host path: rtol 1e-9 / atol 1e-11, those of tests/test_reward_batched.py (the host sums the union area
in another order and partly in float32-promoted Python floats).  Against the batched torch path: both do the same float64
operations in the same order, so a few ulp (2^-52 ~ 2.2e-16 relative on values of order 1..10) is the expected difference; the
parts are held to 1e-12 absolute (the project's front tolerance), R / G_U / xmax / ymax to rtol 1e-12, atol 1e-12."""
import contextlib
import io

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import marl, ops, reward as RW, synthetic
import parity_common as pc
import utils as U
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL


# ---- generators (copies: no import from other test files) ---------------------------------------------------------------------
def _host_case(seed=21, B=48, P=20):
    """the generator of tests/test_reward_batched.py::_check_reward: genuine non-dominated archives of 1-8 rows, pf_hv of 1-8 rows,
    continuous draws (no ties); `want` is the per-env host result"""
    rng = np.random.default_rng(seed)
    front = np.zeros((B, P, 4)); nfr = np.zeros(B, np.int32)
    pfhv = np.zeros((B, P, 4)); npf = np.zeros(B, np.int32)
    parent = np.zeros((B, 2)); points = np.zeros((B, 3, 4)); ref = np.zeros((B, 2))
    want = []
    for b in range(B):
        k = int(rng.integers(1, 9))
        raw = rng.uniform(0.2, 1.0, size=(k, 4)); raw[:, 2:] = rng.uniform(0.3, 0.99, size=(k, 2))
        fr = U.simple_cull_final([list(r) for r in raw])[0]
        nfr[b] = len(fr); front[b, :len(fr)] = np.array(fr)
        m = int(rng.integers(1, 9))
        hvrows = rng.uniform(0.2, 1.0, size=(m, 4)); hvrows[:, 2:] = 0.5
        npf[b] = m; pfhv[b, :m] = hvrows
        par = fr[int(rng.integers(0, len(fr)))]
        parent[b] = par[:2]
        pts = rng.uniform(0.15, 1.05, size=(3, 4)); pts[:, 2:] = rng.uniform(0.4, 1.06, size=(3, 2))
        points[b] = pts
        ref[b] = rng.uniform(0.9, 1.0, size=2)
        want.append(M.difference_reward([list(r) for r in fr], [list(r) for r in hvrows], tuple(par[:2]),
                                        [list(p) for p in pts], list(ref[b]), m))
    case = dict(front=front, nfr=nfr, pfhv=pfhv, npfhv=npf, parent=parent, points=points, ref=ref, npf=npf.copy(), max_front=20)
    return case, want


_HOST = None


def _host():
    global _HOST
    if _HOST is None:
        _HOST = _host_case()
    return _HOST


def _chain(rng, n, lo=0.05, hi=0.95):
    """n mutually non-dominated rows: obj1 ascending, obj2 descending, feasible"""
    x = np.sort(rng.uniform(lo, hi, n)); y = np.sort(rng.uniform(lo, hi, n))[::-1]
    return np.stack([x, y, np.full(n, 0.5), np.full(n, 0.5)], axis=1)


def _grid_case():
    """objectives on a 1/20 grid: ties in obj1 / obj2, duplicates; pair 0's agent 1 equals an archive row exactly"""
    rng = np.random.default_rng(5)
    B, P = 40, 20
    front = rng.uniform(0.05, 1.0, size=(B, P, 4)); front[:, :, 2:] = rng.uniform(0.2, 1.0, size=(B, P, 2))
    front[:, :, :2] = np.round(front[:, :, :2] * 20) / 20
    nfr = rng.integers(1, P + 1, size=B).astype(np.int32)
    pfhv = rng.uniform(0.05, 1.0, size=(B, P, 4)); pfhv[:, :, 2:] = 0.5
    pfhv[:, :, :2] = np.round(pfhv[:, :, :2] * 20) / 20
    npfhv = rng.integers(1, P + 1, size=B).astype(np.int32)
    points = rng.uniform(0.05, 1.05, size=(B, 3, 4)); points[:, :, 2:] = rng.uniform(0.4, 1.04, size=(B, 3, 2))
    points[:, :, :2] = np.round(points[:, :, :2] * 20) / 20
    points[0, 1] = front[0, 0]
    points[1, 0] = points[1, 2] = front[1, 0]                         # two agents on the same archive row
    assert np.all(points[0, 1] <= 1.0)
    parent = front[np.arange(B), 0, :2].copy()
    ref = rng.uniform(0.9, 1.0, size=(B, 2))
    return dict(front=front, nfr=nfr, pfhv=pfhv, npfhv=npfhv, parent=parent, points=points, ref=ref, npf=npfhv.copy(), max_front=20)


def _full_wave_case():
    """P = 61 non-dominated archive rows + three feasible non-dominated points: 64 rows on the full set's wave, 63 on the others;
    truncation to max_front = 61 is active in all four (pair 3 has one infeasible agent: 63 / 62 rows)"""
    rng = np.random.default_rng(6)
    B, P = 5, 61
    front = np.zeros((B, P, 4)); points = np.zeros((B, 3, 4))
    for b in range(B):
        ch = _chain(rng, P + 3)
        pick = np.sort(rng.choice(np.arange(1, P + 2), size=3, replace=False))
        points[b] = ch[pick]
        front[b] = np.delete(ch, pick, axis=0)
    points[3, 1, 2] = 1.3
    nfr = np.full(B, P, np.int32)
    pfhv = front.copy(); npfhv = np.full(B, P, np.int32)
    parent = front[:, 30, :2].copy()
    ref = rng.uniform(0.9, 1.0, size=(B, 2))
    return dict(front=front, nfr=nfr, pfhv=pfhv, npfhv=npfhv, parent=parent, points=points, ref=ref, npf=npfhv.copy(), max_front=61)


def _p50_case():
    """P = 50, max_front = 50, archives of 1 / 49 / 50 rows: truncation from 53 and 52 rows"""
    rng = np.random.default_rng(7)
    B, P = 9, 50
    front = np.zeros((B, P, 4)); points = np.zeros((B, 3, 4))
    nfr = np.array([1, 49, 50] * 3, np.int32)
    for b in range(B):
        ch = _chain(rng, nfr[b] + 3)
        pick = np.sort(rng.choice(np.arange(nfr[b] + 3), size=3, replace=False))
        points[b] = ch[pick]
        front[b, :nfr[b]] = np.delete(ch, pick, axis=0)
    pfhv = front.copy()
    parent = front[:, 0, :2].copy()
    ref = rng.uniform(0.9, 1.0, size=(B, 2))
    return dict(front=front, nfr=nfr, pfhv=pfhv, npfhv=nfr.copy(), parent=parent, points=points, ref=ref, npf=nfr.copy(), max_front=50)


def _edge_case():
    """per pair: no agent feasible; exactly one; all three dominated by the archive; an empty archive with the one feasible point at
    (1, 1) (the special case); an empty archive and no feasible point (n_pf = 0: IEEE results, no special case)"""
    rng = np.random.default_rng(8)
    B, P = 5, 8
    front = np.zeros((B, P, 4)); nfr = np.array([4, 4, 3, 0, 0], np.int32)
    for b in range(3):
        front[b, :nfr[b]] = _chain(rng, nfr[b], 0.3, 0.9)
    front[2, 0, :2] = [0.1, 0.1]
    points = rng.uniform(0.2, 0.9, size=(B, 3, 4))
    points[0, :, 2] = [1.5, 1.01, 2.0]
    points[1, 0, 3] = 1.2; points[1, 2, 0] = 1.0001                   # (an objective above 1 is infeasible for the reward as well)
    points[2, :, :2] = rng.uniform(0.5, 0.9, size=(3, 2))
    points[3] = [[1.0, 1.0, 0.4, 0.4], [0.5, 0.5, 1.5, 0.2], [0.5, 0.5, 0.2, 1.5]]
    points[4, :, 3] = 1.5
    pfhv = front.copy(); npfhv = nfr.copy()
    pfhv[3, :2] = _chain(rng, 2); npfhv[3] = 2
    npf = np.array([4, 4, 3, 2, 0], np.int32)
    parent = rng.uniform(0.3, 0.9, size=(B, 2))
    ref = rng.uniform(0.9, 1.0, size=(B, 2))
    return dict(front=front, nfr=nfr, pfhv=pfhv, npfhv=npfhv, parent=parent, points=points, ref=ref, npf=npf, max_front=8)


def _clipped_pfhv_case():
    """pf_hv with infeasible rows and objectives above 1: hv_all takes every row and clips it"""
    case, _ = _host_case(seed=23, B=16)
    rng = np.random.default_rng(9)
    case["pfhv"] = rng.uniform(0.1, 1.3, size=case["pfhv"].shape)
    case["pfhv"][:, :, 2:] = rng.uniform(0.2, 1.5, size=case["pfhv"][:, :, 2:].shape)
    case["npfhv"] = rng.integers(1, 21, size=16).astype(np.int32)
    case["npf"] = case["npfhv"].copy()
    return case


def _tensors(case, device):
    t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=device)
    i32 = torch.int32
    return (t(case["front"]), t(case["nfr"], i32), t(case["pfhv"]), t(case["npfhv"], i32), t(case["parent"]), t(case["points"]),
            t(case["ref"]), t(case["npf"], i32))


def _torch_parts(args, max_front, lib):
    """the parts of the existing batched path: what reward.difference_reward computes before its element-wise block"""
    front_no, n_front_no, pf_hv, n_pf_hv, parent, points, ref_points, n_pf = args
    feas = (points <= 1.0).all(dim=2)
    B = points.shape[0]
    use4 = feas[None].repeat(4, 1, 1)
    for i in range(3):
        use4[i, :, i] = False
    rep = lambda t: t[None].expand(4, *t.shape).reshape(4 * B, *t.shape[1:])
    pts, n = RW._append(rep(front_no), rep(n_front_no), rep(points), use4.reshape(4 * B, 3))
    four = RW.front_hv(pts.contiguous(), n, rep(ref_points).contiguous(), max_front, lib)
    hv4 = four["hv_front"].view(4, B)
    met = four["metrics"].view(4, B, -1)[3]
    cv = RW.front_hv(pf_hv, n_pf_hv, ref_points, 0, lib)["hv_all"]
    rcv = RW.front_hv(pf_hv, n_pf_hv, None, 0, lib)["hv_all"]
    return torch.stack([hv4[0], hv4[1], hv4[2], hv4[3], cv, rcv, met[:, 3], met[:, 4]], dim=1)


def _compare_paths(case, alias=False):
    lib = tm.load()
    args = list(_tensors(case, "cuda"))
    if alias:
        args[2], args[3] = args[0], args[1]                           # pf_hv IS front_no (what the engine passes)
    mf = case["max_front"]
    want = RW.difference_reward(*args, max_front=mf, lib=lib, path="torch")
    want_parts = _torch_parts(args, mf, lib)
    got = RW.difference_reward_parts(*args, max_front=mf, lib=lib)
    plain = RW.difference_reward(*args, max_front=mf, lib=lib, path="hip")
    names = ("R", "G_U", "xmax", "ymax")
    dp = (got[4] - want_parts).abs()
    print("parts: max abs difference", float(torch.nan_to_num(dp, nan=0.0).max()))
    for nm, g, w in zip(names, got[:4], want):
        print(nm, "max abs difference", float(torch.nan_to_num((g - w).abs(), nan=0.0).max()))
    torch.testing.assert_close(got[4], want_parts, rtol=0, atol=1e-12, equal_nan=True)
    for nm, g, w, p in zip(names, got[:4], want, plain):
        assert g.shape == w.shape and g.dtype == torch.float64, nm
        torch.testing.assert_close(g, w, rtol=1e-12, atol=1e-12, equal_nan=True, msg=lambda m, nm=nm: f"{nm}: {m}")
        assert torch.equal(torch.nan_to_num(g, nan=-7.0), torch.nan_to_num(p, nan=-7.0)), nm    # with / without parts: the same launch
    return got


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fused_reward_against_the_host_path():
    """1: all 48 pairs of the generator of test_reward_batched against master_DDPG_truss2D_MO.difference_reward"""
    case, want = _host()
    R, GU, xm, ym = RW.difference_reward(*_tensors(case, "cuda"), max_front=20, lib=tm.load(), path="hip")
    R, GU, xm, ym = R.cpu().numpy(), GU.cpu().numpy(), xm.cpu().numpy(), ym.cpu().numpy()
    assert R.shape == (48, 3) and len(want) == 48
    for b in range(48):
        r0, r1, r2, gu, xmax, ymax = want[b]
        np.testing.assert_allclose(R[b], [r0, r1, r2], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose([GU[b], xm[b], ym[b]], [gu, xmax, ymax], rtol=1e-9, atol=1e-11)


@pytest.mark.gpu
def test_fused_reward_against_the_batched_path_continuous():
    """2a"""
    _compare_paths(_host()[0])


@pytest.mark.gpu
def test_fused_reward_against_the_batched_path_grid_ties_and_duplicates():
    """2b"""
    case = _grid_case()
    assert np.array_equal(case["points"][0, 1], case["front"][0, 0])
    _compare_paths(case)


@pytest.mark.gpu
def test_fused_reward_against_the_batched_path_full_wave():
    """2c: 64 / 63 rows, truncation to 61"""
    got = _compare_paths(_full_wave_case())
    assert torch.isfinite(got[0]).all()


@pytest.mark.gpu
def test_fused_reward_against_the_batched_path_max_front_50():
    """2d"""
    _compare_paths(_p50_case())


@pytest.mark.gpu
def test_fused_reward_against_the_batched_path_edge_cases():
    """2e"""
    got = _compare_paths(_edge_case())
    parts = got[4].cpu().numpy()
    assert parts[3, 3] == 0.0 and parts[4, 3] == 0.0                  # (1, 1) alone: hypervolume 0; the empty set: 0
    assert np.all(parts[0, :4] == parts[0, 3])                        # no agent feasible: the four sets are the archive
    assert not np.isfinite(got[0][4].cpu().numpy()).any()             # n_pf = 0: IEEE, as the torch path


@pytest.mark.gpu
def test_fused_reward_against_the_batched_path_pf_hv_alias_and_clipping():
    """2f"""
    _compare_paths(_host()[0], alias=True)
    _compare_paths(_clipped_pfhv_case())


@pytest.mark.gpu
def test_fused_reward_is_reproducible_and_stays_in_bounds():
    """3: K = 37; outputs inside larger sentinel-filled buffers"""
    lib = tm.load()
    case, _ = _host()
    K, pad, S = 37, 5, -12345.0
    args = [a[:K].contiguous() for a in _tensors(case, "cuda")]
    ns, lid = ops.namespace(), ops.bind(lib)

    def run():
        bufs = [torch.full((K + 2 * pad, c), S, dtype=torch.float64, device="cuda") for c in (3, 1, 1, 1, 8)]
        R = bufs[0][pad:pad + K]
        GU, xm, ym = (b[:, 0][pad:pad + K] for b in bufs[1:4])
        Q = bufs[4][pad:pad + K]
        assert all(v.is_contiguous() for v in (R, GU, xm, ym, Q))
        ops.call(ns.reward, lid, 0, 20, *args, R, GU, xm, ym, Q)
        torch.cuda.synchronize()
        return bufs

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        assert torch.all(x[:pad] == S) and torch.all(x[pad + K:] == S)
        assert torch.all(x[pad:pad + K] != S)
    full = RW.difference_reward_parts(*_tensors(case, "cuda"), max_front=20, lib=lib)
    assert torch.equal(a[0][pad:pad + K], full[0][:K]) and torch.equal(a[4][pad:pad + K], full[4][:K])   # a pair's result does not depend on K


@pytest.mark.gpu
def test_fused_reward_argument_checks():
    """4: every bad call raises and writes nothing"""
    lib = tm.load()
    case, _ = _host()
    args = list(_tensors(case, "cuda"))
    K = 48
    f64 = torch.float64
    z = lambda *s: torch.zeros(*s, dtype=f64, device="cuda")
    with pytest.raises(ValueError, match="P \\+ 3 <= 64"):
        RW.difference_reward(z(K, 62, 4), args[1], z(K, 62, 4), args[3], *args[4:], max_front=20, lib=lib, path="hip")
    with pytest.raises(tm.TrussError, match="max_front"):
        RW.difference_reward(*args, max_front=1, lib=lib, path="hip")
    with pytest.raises(tm.TrussError, match="front_no must be Double"):
        RW.difference_reward(args[0].float(), *args[1:], max_front=20, lib=lib, path="hip")
    ns, lid = ops.namespace(), ops.bind(lib)
    S = -3.0
    outs = lambda: [torch.full((K, 3), S, dtype=f64, device="cuda")] + [torch.full((K,), S, dtype=f64, device="cuda") for _ in range(3)]
    o = outs()
    with pytest.raises(tm.TrussError, match="points must be contiguous"):
        bad = args[5].permute(1, 0, 2).contiguous().permute(1, 0, 2)
        assert bad.shape == (K, 3, 4) and not bad.is_contiguous()
        ops.call(ns.reward, lid, 0, 20, *args[:5], bad, *args[6:], *o, None)
    with pytest.raises(tm.TrussError, match="R must be \\[K, 3\\]"):
        ops.call(ns.reward, lid, 0, 20, *args, torch.full((K, 4), S, dtype=f64, device="cuda"), *o[1:], None)
    with pytest.raises(tm.TrussError, match="max_front"):
        ops.call(ns.reward, lid, 0, 1, *args, *o, None)
    torch.cuda.synchronize()
    assert all(torch.all(t == S) for t in o)
    # no pairs: returns cleanly
    e = [a[:0].contiguous() for a in args]
    R, GU, xm, ym = RW.difference_reward(*e, max_front=20, lib=lib, path="hip")
    assert R.shape == (0, 3) and GU.shape == xm.shape == ym.shape == (0,)


def _agents(device, seed, hidden=16):
    torch.manual_seed(seed)
    return RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, hidden, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)


def _engine(lib, device, reward_path, rl=None, B=6, num_x=4, seed=3):
    topo = tm.TrussTopology.grid(num_x)
    eng = marl.BatchedMARL(topo, B, rl or _agents(device, seed), max_front=6, lib=lib, device=device, replay_capacity=256, batch_size=8,
                           seed=seed, tune_update_gemms=False, reward_path=reward_path)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng


def _same_step(a, b):
    torch.testing.assert_close(a["reward"], b["reward"], rtol=1e-12, atol=0)
    assert torch.equal(a["hv"], b["hv"]) and torch.equal(a["n_front"], b["n_front"]) and a["replay_added"] == b["replay_added"]


def _same_archive(ea, eb):
    for name in ("pts", "arch_y", "arch_sec", "n"):
        assert torch.equal(getattr(ea, name), getattr(eb, name)), name


@pytest.mark.gpu
def test_engine_plays_the_same_game_with_the_fused_reward():
    """5: 8 nodes, B = 6, max_front = 6, three game steps without exploration or training.  The two engines share one set of
    agents (nothing trains): the networks' lazily created weights depend on the generator state at their first forward pass, so two
    sets made from one seed are not the same networks."""
    lib = tm.load()
    rl = _agents("cuda", 3)
    with contextlib.redirect_stdout(io.StringIO()):
        et, eh = _engine(lib, "cuda", "torch", rl), _engine(lib, "cuda", "hip", rl)
        assert (et.reward_path, eh.reward_path) == ("torch", "hip")
        for _ in range(3):
            _same_step(et.game_step_all(train=False, explore=False), eh.game_step_all(train=False, explore=False))
            _same_archive(et, eh)
    assert int(eh.n.max()) >= 1


@pytest.mark.gpu
def test_mixed_engine_forwards_reward_path():
    """5, through MixedMARL: two size classes (8 and 16 nodes), the keyword reaches every class's engine (one set of agents for
    both mixes, as above)"""
    from truss_mi355 import pool
    lib = tm.load()
    mixes = []
    rl = _agents("cuda", 4)
    with contextlib.redirect_stdout(io.StringIO()):
        for path in ("torch", "hip"):
            classes = pool.grid_classes([4, 8], [6, 5])
            mix = marl.MixedMARL(classes, rl, bucket_envs=3, max_front=6, lib=lib, device="cuda", replay_capacity=128, batch_size=4, seed=2,
                                 tune_update_gemms=False, reward_path=path)
            per_class = []
            for k, e in enumerate(mix.engines):
                full = synthetic.random_batch(e.topo, classes[mix.class_ids[k]][1], 9 + k)
                per_class.append({key: v[mix.global_ids(k)] for key, v in full.items()})
            mix.reset(per_class)
            assert len(mix.engines) == 2 and all(e.reward_path == path for e in mix.engines)
            mixes.append(mix)
        for _ in range(3):
            ot, oh = (m.game_step_all(train=False, explore=False) for m in mixes)
            for a, b in zip(ot["per_class"], oh["per_class"]):
                _same_step(a, b)
            for ea, eb in zip(mixes[0].engines, mixes[1].engines):
                _same_archive(ea, eb)


# ---- CPU (the lane emulator has no truss_reward) -----------------------------------------------------------------------------
def test_path_argument_on_the_emulator():
    """6"""
    lib = pc.emu_lib()
    assert not lib.has_reward
    case, _ = _host()
    args = _tensors(case, "cpu")
    base = RW.difference_reward(*args, max_front=20, lib=lib)
    same = RW.difference_reward(*args, max_front=20, lib=lib, path="torch")
    for a, b in zip(base, same):
        assert torch.equal(a, b)
    with pytest.raises(tm.TrussError, match="truss_reward"):
        RW.difference_reward(*args, max_front=20, lib=lib, path="hip")
    with pytest.raises(tm.TrussError, match="has no truss_reward"):     # the operator itself, handed a library without the entry
        o = [torch.zeros(48, 3, dtype=torch.float64)] + [torch.zeros(48, dtype=torch.float64) for _ in range(3)]
        ops.call(ops.namespace().reward, ops.bind(lib), 0, 20, *args, *o, None)
    with pytest.raises(ValueError, match="path must be"):
        RW.difference_reward(*args, max_front=20, lib=lib, path="other")


def test_engine_reward_path_on_the_emulator(monkeypatch):
    """7"""
    lib = pc.emu_lib()
    monkeypatch.delenv("TRUSS_REWARD", raising=False)
    with contextlib.redirect_stdout(io.StringIO()):
        assert _engine(lib, "cpu", None).reward_path == "torch"
        with pytest.raises(ValueError, match="no truss_reward"):
            _engine(lib, "cpu", "hip")
        with pytest.raises(ValueError, match="reward_path must be"):
            _engine(lib, "cpu", "bogus")
        monkeypatch.setenv("TRUSS_REWARD", "hip")
        with pytest.raises(ValueError, match="no truss_reward"):
            _engine(lib, "cpu", None)
        assert _engine(lib, "cpu", "torch").reward_path == "torch"     # an explicit choice wins over the environment


def test_reward_operator_meta_registration():
    """8"""
    ns = ops.namespace()
    K, P = 3, 20
    m = lambda *s, dt=torch.float64: torch.empty(*s, dtype=dt, device="meta")
    n = lambda: m(K, dt=torch.int32)
    ns.reward(0, 0, 20, m(K, P, 4), n(), m(K, P, 4), n(), m(K, 2), m(K, 3, 4), m(K, 2), n(), m(K, 3), m(K), m(K), m(K), m(K, 8))
    ns.reward(0, 0, 20, m(K, P, 4), n(), m(K, P, 4), n(), m(K, 2), m(K, 3, 4), m(K, 2), n(), m(K, 3), m(K), m(K), m(K), None)
    sch = str(ns.reward.default._schema)
    for out in ("Tensor(a!) R", "Tensor(d!) ymax", "Tensor(e!)? parts"):
        assert out in sch, out
