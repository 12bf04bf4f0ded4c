"""The set-up of a chunk of (env, member) pairs of a game step as one launch (`truss_pair_setup`, csrc/truss_pairs.h; marl.pair_setup,
BatchedMARL(pair_path="hip")).

Two references, neither of them the code under test:
  (a) the torch block: the set-up block of `BatchedMARL.game_step_all` / `_obs` / `pareto_graph` / `design_coins` as the default engine
      runs it, lifted into this file (`_torch_block`) and run on the device under test;
  (b) a host model per pair in float64 / Python integers (`_host_model`): plain loops, 1 / math.sqrt(deg), splitmix64 on Python
      integers masked to 64 bits.
The CPU tests hold (a) against (b) on the very inputs the GPU tests use, and check that the inputs are what they claim to be.

Tolerances.  Everything but A_p is a copy, one conversion or one float32 division of exactly representable operands: equal.  A_p is a
product of two table entries: against the float64 value A64, a correctly rounded float32 table carries 2^-24 relative per factor and
the float32 product another 2^-24 -- 3 x 2^-24 A64 (the second-order terms are below 2^-47).  On the CPU the framework's own pow may be
one ulp off per factor (2^-23 each instead of 2^-24): 5 x 2^-24.
"""
import contextlib
import ctypes
import io
import math

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import _lib, marl, ops, synthetic
import parity_common as pc
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL

#          B, P,  N,  E,  K, rep, coins
CASES = {
    "misaligned": (5, 3, 7, 13, 11, 3, False),        # every row stride off the 16-byte grid, K > B: envs repeat
    "smallest": (4, 2, 1, 1, 1, 1, True),
    "small_roof": (9, 20, 16, 36, 40, 3, False),
    "design": (6, 50, 16, 36, 25, 1, True),
    "odd_N": (3, 20, 33, 64, 8, 3, True),
}
COIN_SETTINGS = ((0, 0), (2 ** 63 - 1, 65535))        # (seed, game_step)
NPARAM = 8
PAD = 2                                                # rows behind the ones a call writes, in every output buffer
SENT_F, SENT_I, SENT_U8 = -777.25, -777, 0xA5
MASK = (1 << 64) - 1


# ---- (b): the host model -------------------------------------------------------------------------------------------------------------
def _sm64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _host_coin(seed, env_id, game_step, member, agent):
    key = ((env_id << 26) | (game_step << 10) | (member << 2) | agent) & MASK
    return _sm64(key ^ _sm64(seed & MASK)) >> 63


def _host_model(c, rep, setting):
    """every output of the set-up for the case's pairs, in float64 / Python integers; x_p / A_p as float64 [K, ...] (one copy)"""
    B, P = c["pts"].shape[:2]
    K = len(c["idx"])
    out = dict(p0=np.zeros((K, P, 4)), nn0=np.zeros(K, np.int32), parent_obj=np.zeros((K, 2)), ref=np.zeros((K, 2)),
               x_p=np.zeros((K, P, 4)), x_p_frac=np.zeros(K, np.float32), A_p=np.zeros((K, P, P)),
               coin=None if setting is None else np.zeros(3 * K, np.uint8))
    par = {k: [] for k in ("x", "target", "params", "y", "sec")}
    for k in range(K):
        b, m = int(c["idx"][k]), int(c["ms"][k])
        n = int(c["n"][b])
        par["x"].append(c["c_x"][b]); par["target"].append(c["c_target"][b]); par["params"].append(c["c_params"][b])
        par["y"].append(c["arch_y"][b, m]); par["sec"].append(c["arch_sec"][b, m])
        out["p0"][k] = c["pts"][b]
        out["nn0"][k] = n
        out["parent_obj"][k] = c["pts"][b, m, :2]
        out["ref"][k] = c["ref_points"][b]
        out["x_p_frac"][k] = np.float32(n) / np.float32(P)
        for i in range(n):
            out["x_p"][k, i] = (c["pts"][b, i, 0], c["pts"][b, i, 1], 1.0 if i == m else 0.0, float(out["x_p_frac"][k]))
        deg = [1 + (i > 0) + (i + 1 < n) for i in range(n)]
        for i in range(n):
            for j in range(max(0, i - 1), min(n, i + 2)):
                out["A_p"][k, i, j] = (1.0 / math.sqrt(deg[i])) * (1.0 / math.sqrt(deg[j]))
        if setting is not None:
            for a in range(3):
                out["coin"][a * K + k] = _host_coin(setting[0], int(c["env_ids"][b]), setting[1], m, a)
    out["par"] = {k: np.stack(v) for k, v in par.items()}
    out["cand"] = {k: np.concatenate([v, v, v], axis=0) for k, v in out["par"].items()}
    return out


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def _case(name):
    """arrays of case `name`: archives with n[b] live rows (n over P, 1, P - 1, 2 as far as B reaches) and finite garbage behind them,
    pairs that cover member 0, member n - 1 and an interior member as far as K and n reach, shuffled with envs repeating, env ids
    around 2^37.  In the cases with coins the env ids are moved until (b) has both coin values under both settings."""
    B, P, N, E, K, rep, coins = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    sizes = list(dict.fromkeys(min(max(v, 1), P) for v in (P, 1, P - 1, 2)))
    n = np.array([sizes[b % len(sizes)] for b in range(B)], np.int32)
    live = np.arange(P)[None, :] < n[:, None]
    garbage = lambda shape: rng.uniform(1.0, 900.0, shape) * rng.choice([-1.0, 1.0], shape)
    pts = np.where(live[:, :, None], rng.uniform(0.05, 1.0, (B, P, 4)), garbage((B, P, 4)))
    arch_y = np.where(live[:, :, None], rng.uniform(-3.0, 3.0, (B, P, N)), garbage((B, P, N))).astype(np.float32)
    arch_sec = np.where(live[:, :, None], rng.integers(1, 60, (B, P, E)), rng.integers(1000, 9000, (B, P, E))).astype(np.int32)
    # the pairs: the wanted members of the envs in order of falling n first, then random live members, cut to K, shuffled
    want = []
    for b in sorted(range(B), key=lambda b: -int(n[b])):
        nb = int(n[b])
        want += [(b, m) for m in dict.fromkeys((nb // 2 if nb >= 3 else 0, nb - 1, 0))]
    want = want[:K]
    while len(want) < K:
        b = int(rng.integers(0, B))
        want.append((b, int(rng.integers(0, n[b]))))
    order = rng.permutation(K)
    idx = np.array([want[i][0] for i in order], np.int64)
    ms = np.array([want[i][1] for i in order], np.int64)
    c = dict(pts=pts, n=n, arch_y=arch_y, arch_sec=arch_sec, c_x=rng.uniform(0.0, 30.0, (B, N)).astype(np.float32),
             c_target=rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32), c_params=rng.uniform(-2.0, 2.0, (B, NPARAM)),
             ref_points=rng.uniform(0.2, 1.0, (B, 2)), idx=idx, ms=ms)
    base = (1 << 37) + 12345
    for shift in range(64):
        c["env_ids"] = (base + shift * 1001 + rng.permutation(B) * 77).astype(np.int64)
        if not coins or all(len(set(_host_model(c, rep, s)["coin"].tolist())) == 2 for s in COIN_SETTINGS):
            break
    return c


_CACHE = {}


def _cached(name):
    """(arrays, {setting: host model}) of a case, made once"""
    if name not in _CACHE:
        c = _case(name)
        rep, coins = CASES[name][5:]
        _CACHE[name] = (c, {s: _host_model(c, rep, s) for s in (COIN_SETTINGS if coins else (None,))})
    return _CACHE[name]


def _t(c, device):
    return {k: torch.tensor(v, device=device) for k, v in c.items()}


# ---- (a): the torch block, as the default engine runs it -----------------------------------------------------------------------------
def _tridiagonal(P, dev):
    i = torch.arange(P, device=dev)
    return ((i[:, None] - i[None, :]).abs() <= 1).float()


def _pareto_graph(pts, n, index, max_front):
    B, P, _ = pts.shape
    dev = pts.device
    ar = torch.arange(P, device=dev)
    vf = (ar[None, :] < n[:, None]).float()
    x = torch.stack([pts[:, :, 0].float(), pts[:, :, 1].float(), (ar[None, :] == index[:, None]).float(),
                     (n.float() / max_front)[:, None].expand(B, P)], dim=2) * vf[:, :, None]
    z = torch.zeros((B, 1), dtype=torch.float32, device=dev)
    deg = vf * (1.0 + torch.cat([z, vf[:, :-1]], dim=1) + torch.cat([vf[:, 1:], z], dim=1))
    d = torch.where(deg > 0, deg.pow(-0.5), 0.0)
    return x, _tridiagonal(P, dev) * d[:, :, None] * d[:, None, :]


_SM64 = (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)


def _splitmix64(z):
    s64 = lambda c: c - (1 << 64) if c >= 1 << 63 else c
    srl = lambda v, k: (v >> k) & ((1 << (64 - k)) - 1)
    z = z + s64(_SM64[0])
    z = (z ^ srl(z, 30)) * s64(_SM64[1])
    z = (z ^ srl(z, 27)) * s64(_SM64[2])
    return z ^ srl(z, 31)


def _design_coins(seed, env_ids, game_step, members):
    dev = env_ids.device
    key = (env_ids.to(torch.int64)[:, None] << 26) | (int(game_step) << 10) | (members.to(torch.int64)[:, None] << 2) \
        | torch.arange(3, dtype=torch.int64, device=dev)[None, :]
    h0 = _splitmix64(torch.tensor(int(seed), dtype=torch.int64, device=dev))
    return (_splitmix64(key ^ h0) < 0).to(torch.uint8)


def _torch_block(t, rep, setting):
    idx, ms = t["idx"], t["ms"]
    K, P = int(idx.numel()), t["pts"].shape[1]
    ark = torch.arange(K, device=idx.device)
    p0, nn0 = t["pts"][idx].contiguous(), t["n"][idx].contiguous()
    par = dict(x=t["c_x"][idx], target=t["c_target"][idx], params=t["c_params"][idx], y=t["arch_y"][idx, ms], sec=t["arch_sec"][idx, ms])
    cand = {k: v.repeat(3, 1) for k, v in par.items()}
    x_p, A_p = _pareto_graph(p0, nn0, ms, P)
    if rep > 1:
        x_p, A_p = x_p.repeat(rep, 1, 1), A_p.repeat(rep, 1, 1)
    coin = None
    if setting is not None:
        coin = _design_coins(setting[0], t["env_ids"][idx], setting[1], ms).t().contiguous().view(-1)
    return dict(par=par, cand=cand, p0=p0, nn0=nn0, parent_obj=p0[ark, ms, :2].contiguous(), ref=t["ref_points"][idx].contiguous(),
                x_p=x_p, A_p=A_p, coin=coin)


# ---- the code under test -------------------------------------------------------------------------------------------------------------
def _sentinel_bufs(name, device):
    """output buffers of a case, PAD rows longer than what a call writes, filled with a sentinel"""
    B, P, N, E, K, rep, coins = CASES[name]
    f32, f64, i32, u8 = torch.float32, torch.float64, torch.int32, torch.uint8
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=device)
    rows = lambda r: dict(x=full((r, N), SENT_F, f32), target=full((r, N), SENT_F, f32), params=full((r, NPARAM), SENT_F, f64),
                          y=full((r, N), SENT_F, f32), sec=full((r, E), SENT_I, i32))
    out = dict(p0=full((K + PAD, P, 4), SENT_F, f64), nn0=full((K + PAD,), SENT_I, i32), parent_obj=full((K + PAD, 2), SENT_F, f64),
               ref=full((K + PAD, 2), SENT_F, f64), x_p=full((rep * K + PAD, P, 4), SENT_F, f32), A_p=full((rep * K + PAD, P, P), SENT_F, f32))
    if coins:
        out["coin"] = full((3 * K + PAD,), SENT_U8, u8)
    return rows(K + PAD), rows(3 * K + PAD), out


def _flat(res):
    """name -> tensor of everything a set-up returns"""
    d = {k: v for k, v in res.items() if k not in ("par", "cand") and v is not None}
    d.update({f"par_{k}": v for k, v in res["par"].items()})
    d.update({f"cand_{k}": v for k, v in res["cand"].items()})
    return d


def _rows_written(name):
    B, P, N, E, K, rep, coins = CASES[name]
    w = dict(p0=K, nn0=K, parent_obj=K, ref=K, x_p=rep * K, A_p=rep * K, coin=3 * K)
    w.update({f"par_{k}": K for k in ("x", "target", "params", "y", "sec")})
    w.update({f"cand_{k}": 3 * K for k in ("x", "target", "params", "y", "sec")})
    return w


def _run(lib, name, t, setting, dtab, frac_tab=None):
    """marl.pair_setup into sentinel buffers: (name -> the rows written, name -> the rows behind them)"""
    rep = CASES[name][5]
    par, cand, out = _sentinel_bufs(name, t["pts"].device)
    res = marl.pair_setup(lib, t["idx"], t["ms"], t["pts"], t["n"], t["arch_y"], t["arch_sec"], t["c_x"], t["c_target"], t["c_params"],
                          t["ref_points"], rep=rep, dtab=dtab, frac_tab=frac_tab,
                          coins=None if setting is None else (setting[0], t["env_ids"], setting[1]), par=par, cand=cand, out=out)
    w = _rows_written(name)
    flat = _flat(res)
    return {k: v[:w[k]] for k, v in flat.items()}, {k: v[w[k]:] for k, v in flat.items()}


def _sentinels_intact(behind):
    for k, v in behind.items():
        assert v.shape[0] == PAD, k
        s = SENT_U8 if v.dtype == torch.uint8 else SENT_I if v.dtype == torch.int32 else SENT_F
        assert bool((v == s).all()), f"{k}: rows behind the written ones were touched"


def _settings(name):
    return COIN_SETTINGS if CASES[name][6] else (None,)


def _against_host(got, want, a_tol, name):
    """`got` (name -> numpy array of the rows written) against the host model"""
    B, P, N, E, K, rep, coins = CASES[name]
    for k in ("x", "target", "params", "y", "sec"):
        assert np.array_equal(got[f"par_{k}"], want["par"][k]), f"par_{k}"
        assert np.array_equal(got[f"cand_{k}"], want["cand"][k]), f"cand_{k}"
    for k in ("p0", "nn0", "parent_obj", "ref"):
        assert np.array_equal(got[k], want[k]), k
    if want["coin"] is not None:
        assert np.array_equal(got["coin"], want["coin"]), "coin"
    x64, a64 = np.concatenate([want["x_p"]] * rep), np.concatenate([want["A_p"]] * rep)
    assert got["x_p"].dtype == np.float32 and got["A_p"].dtype == np.float32
    for at in np.argwhere(got["x_p"] != x64.astype(np.float32))[:6]:          # (what differs, before the assertion)
        print(f"\n[{name}] x_p{at.tolist()}: got {got['x_p'][tuple(at)]!r}, float32 of the host model {np.float32(x64[tuple(at)])!r}")
    assert np.array_equal(got["x_p"], x64.astype(np.float32)), "x_p is not float32(the float64 value)"
    frac = np.concatenate([want["x_p_frac"]] * rep)
    nn = np.concatenate([want["nn0"]] * rep)
    for r in range(rep * K):
        assert np.array_equal(got["x_p"][r, :nn[r], 3], np.full(nn[r], frac[r], np.float32)), "x_p column 3"
    assert np.all(got["x_p"][x64 == 0.0] == 0.0) and np.all(got["A_p"][a64 == 0.0] == 0.0), "a zero of the host model is not an exact zero"
    err = np.abs(got["A_p"].astype(np.float64) - a64)
    print(f"\n[{name}] max |A_p - A64| / A64 = {np.max(err[a64 > 0] / a64[a64 > 0]) / 2.0 ** -24:.3f} x 2^-24 (bound {a_tol})")
    assert np.all(err <= a_tol * 2.0 ** -24 * a64), "A_p"


# ---- 5: (a) against (b) on the CPU, and the inputs themselves ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_torch_block_agrees_with_the_host_model_on_the_cpu(name):
    B, P, N, E, K, rep, coins = CASES[name]
    c, wants = _cached(name)
    # what the generator promises
    assert c["idx"].shape == (K,) and c["ms"].shape == (K,) and np.all(c["ms"] < c["n"][c["idx"]]) and np.all(c["ms"] >= 0)
    assert K == 1 or len(set(c["idx"].tolist())) < K, "no env repeats"
    assert K < 3 or list(c["idx"]) != sorted(c["idx"]), "the pairs are sorted by env"
    assert set(c["n"].tolist()) == set(list(dict.fromkeys(min(max(v, 1), P) for v in (P, 1, P - 1, 2)))[:B])
    dead = np.arange(P)[None, :] >= c["n"][:, None]
    assert dead.any() and (~dead).any(), "both dead and live rows"
    for k in ("pts", "arch_y", "arch_sec"):
        assert np.all(np.isfinite(c[k])) and np.all(c[k][dead] != 0), f"{k}: the rows behind the front hold finite garbage, not zeros"
    assert np.all(c["env_ids"] >= 1 << 37) and len(set(c["env_ids"].tolist())) == B
    members = {(int(m), int(c["n"][b])) for b, m in zip(c["idx"], c["ms"])}
    assert any(m == 0 for m, _ in members)
    if K >= 3:
        assert any(m == n - 1 and n >= 2 for m, n in members) and (P < 3 or any(0 < m < n - 1 for m, n in members))
    for s, want in wants.items():
        assert (s is None) == (not coins)
        if coins:
            assert set(want["coin"].tolist()) == {0, 1}, "the case's coins come out one-sided"
        ref = _torch_block(_t(c, "cpu"), rep, s)
        got = {k: v.numpy() for k, v in _flat(ref).items()}
        _against_host(got, want, 5, name)


def test_the_cases_cover_every_archive_size_and_member_position():
    """over all cases: n = 1, 2, P - 1, P occur, and pairs at member 0, at member n - 1 and inside"""
    seen_n, seen_m = set(), set()
    for name in CASES:
        c, _ = _cached(name)
        P = CASES[name][1]
        for b, m in zip(c["idx"], c["ms"]):
            n = int(c["n"][b])
            seen_n |= {k for k, v in (("1", 1), ("2", 2), ("P-1", P - 1), ("P", P)) if n == v}
            seen_m |= {"first"} if m == 0 else set()
            seen_m |= {"last"} if m == n - 1 and n >= 2 else set()
            seen_m |= {"inside"} if 0 < m < n - 1 else set()
    assert seen_n == {"1", "2", "P-1", "P"} and seen_m == {"first", "last", "inside"}


# ---- 6: a library without the entry ---------------------------------------------------------------------------------------------------
def _agents(device, seed, hidden=16):
    torch.manual_seed(seed)
    return RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, hidden, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)


def _engine(lib, device, pair_path, rl=None, B=6, num_x=4, seed=3, game="train", max_front=6, **kw):
    topo = tm.TrussTopology.grid(num_x, "small") if game == "test" else tm.TrussTopology.grid(num_x)
    eng = marl.BatchedMARL(topo, B, rl or _agents(device, seed), max_front=max_front, lib=lib, device=device, replay_capacity=256, batch_size=8,
                           seed=seed, tune_update_gemms=False, pair_path=pair_path, game=game, **kw)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng


def test_pair_path_on_the_emulator(monkeypatch):
    lib = pc.emu_lib()
    assert not lib.has_pair_setup and _lib.PAIR_MAXP == 256
    assert "truss_pair_setup" in ops.entries()
    c, _ = _cached("smallest")
    t = _t(c, "cpu")
    args = (t["idx"], t["ms"], t["pts"], t["n"], t["arch_y"], t["arch_sec"], t["c_x"], t["c_target"], t["c_params"], t["ref_points"])
    with pytest.raises(tm.TrussError, match="has no truss_pair_setup"):
        marl.pair_setup(lib, *args, rep=1, dtab=[0.0, 1.0, 0.5, 0.25])
    par, cand, out = _sentinel_bufs("smallest", "cpu")
    with pytest.raises(tm.TrussError, match="has no truss_pair_setup$"):          # the operator itself, handed a library without the entry
        ops.call(ops.namespace().pair_setup, ops.bind(lib), 0, 1, 0, 0, [0.0, 1.0, 0.5, 0.25], *args, t["env_ids"], None,
                 *[par[k] for k in ("x", "target", "params", "y", "sec")], *[cand[k] for k in ("x", "target", "params", "y", "sec")],
                 out["p0"], out["nn0"], out["parent_obj"], out["ref"], out["x_p"], out["A_p"], out["coin"])
    monkeypatch.delenv("TRUSS_PAIRS", raising=False)
    with contextlib.redirect_stdout(io.StringIO()):
        assert _engine(lib, "cpu", None).pair_path == "torch"
        with pytest.raises(ValueError, match="no truss_pair_setup"):
            _engine(lib, "cpu", "hip")
        with pytest.raises(ValueError, match="pair_path must be"):
            _engine(lib, "cpu", "nonsense")
        monkeypatch.setenv("TRUSS_PAIRS", "hip")
        with pytest.raises(ValueError, match="no truss_pair_setup"):               # None reads the environment
            _engine(lib, "cpu", None)
        assert _engine(lib, "cpu", "torch").pair_path == "torch"                   # an explicit choice wins over the environment


def test_pair_operator_meta_registration():
    ns = ops.namespace()
    B, P, N, E, K = 3, 5, 4, 6, 7
    m = lambda *s, dt=torch.float64: torch.empty(*s, dtype=dt, device="meta")
    i32, i64, f32, u8 = torch.int32, torch.int64, torch.float32, torch.uint8
    ins = [m(K, dt=i64), m(K, dt=i64), m(B, P, 4), m(B, dt=i32), m(B, P, N, dt=f32), m(B, P, E, dt=i32), m(B, N, dt=f32), m(B, N, dt=f32),
           m(B, NPARAM), m(B, 2)]
    rows = lambda r: [m(r, N, dt=f32), m(r, N, dt=f32), m(r, NPARAM), m(r, N, dt=f32), m(r, E, dt=i32)]
    outs = rows(K) + rows(3 * K) + [m(K, P, 4), m(K, dt=i32), m(K, 2), m(K, 2), m(3 * K, P, 4, dt=f32), m(3 * K, P, P, dt=f32)]
    ns.pair_setup(0, 0, 3, 0, 0, [0.0, 1.0, 0.7, 0.5], *ins, m(B, dt=i64), m(P + 1, dt=f32), *outs, m(3 * K, dt=u8))
    ns.pair_setup(0, 0, 3, 0, 0, [0.0, 1.0, 0.7, 0.5], *ins, None, None, *outs, None)
    sch = str(ns.pair_setup.default._schema)
    for out in ("Tensor(a!) par_x", "Tensor(j!) cand_sec", "Tensor(p!) A_p", "Tensor(q!)? coin", "Tensor? env_ids", "Tensor? frac_tab", "float[] dtab"):
        assert out in sch, out


# ---- 1: the operator against (a) -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_the_torch_block(name):
    """torch.equal on every output (-0 equals +0 there: the block multiplies dead rows by zero, the kernel writes +0), with the tables
    the engine uses: what the framework computes on this device for [1, 2, 3] ** -0.5 and for n / P, n = 0..P (a GPU divides a tensor
    by a host scalar as a product with the rounded reciprocal: two roundings, not the one division test 2 holds the kernel to
    without the table); the rows behind the written ones keep their sentinel"""
    lib = tm.load()
    c, _ = _cached(name)
    t = _t(c, "cuda")
    P = CASES[name][1]
    dtab = [0.0] + torch.tensor([1.0, 2.0, 3.0], device="cuda").pow(-0.5).tolist()
    frac_tab = torch.arange(P + 1, dtype=torch.int32, device="cuda").float() / P
    for s in _settings(name):
        got, behind = _run(lib, name, t, s, dtab, frac_tab)
        ref = _flat(_torch_block(t, CASES[name][5], s))
        assert set(got) == set(ref)
        for k in sorted(ref):
            assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
            bad = torch.nonzero(got[k] != ref[k])
            for at in bad[:6].tolist():                                     # (what differs, before the assertion)
                print(f"\n[{name} {s}] {k}{at}: got {got[k][tuple(at)].item()!r}, torch block {ref[k][tuple(at)].item()!r}")
            assert torch.equal(got[k], ref[k]), f"{name} {s}: {k} differs in {bad.shape[0]} elements"
        _sentinels_intact(behind)
    for k, v in c.items():                                                  # the inputs are as they were
        assert np.array_equal(t[k].cpu().numpy(), v), k


# ---- 2: the operator against (b) -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_against_the_host_model(name):
    lib = tm.load()
    c, wants = _cached(name)
    t = _t(c, "cuda")
    dtab = [0.0] + [float(np.float32(1.0 / math.sqrt(d))) for d in (1, 2, 3)]       # the test's own, correctly rounded
    for s, want in wants.items():
        if s is not None:
            assert set(want["coin"].tolist()) == {0, 1}
        got, behind = _run(lib, name, t, s, dtab)
        _against_host({k: v.cpu().numpy() for k, v in got.items()}, want, 3, name)
        _sentinels_intact(behind)


@pytest.mark.gpu
def test_one_launch_and_fresh_outputs():
    """a set-up call is one launch of truss_pair_kernel and no other device operation; without preallocated outputs it returns new
    tensors of the documented shapes"""
    from torch.profiler import profile, ProfilerActivity
    lib = tm.load()
    name = "design"
    B, P, N, E, K, rep, coins = CASES[name]
    c, wants = _cached(name)
    t = _t(c, "cuda")
    dtab = [0.0] + [float(np.float32(1.0 / math.sqrt(d))) for d in (1, 2, 3)]
    s = COIN_SETTINGS[1]
    call = lambda: marl.pair_setup(lib, t["idx"], t["ms"], t["pts"], t["n"], t["arch_y"], t["arch_sec"], t["c_x"], t["c_target"], t["c_params"],
                                   t["ref_points"], rep=rep, dtab=dtab, coins=(s[0], t["env_ids"], s[1]))
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = call()
        torch.cuda.synchronize()
    dev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(dev) == 1 and "truss_pair_kernel" in dev[0], dev
    assert res["x_p"].shape == (rep * K, P, 4) and res["A_p"].shape == (rep * K, P, P) and res["coin"].shape == (3 * K,)
    assert res["par"]["y"].shape == (K, N) and res["cand"]["sec"].shape == (3 * K, E) and res["p0"].shape == (K, P, 4)
    _against_host({k: v.cpu().numpy() for k, v in _flat(res).items()}, wants[s], 3, name)


# ---- 3: refusals through the raw entry -------------------------------------------------------------------------------------------------
def _raw_args(name, t, par, cand, out, **over):
    B, P, N, E, K, rep, coins = CASES[name]
    a = _lib.PairArgs()
    a.struct_size = ctypes.sizeof(_lib.PairArgs)
    a.n_pairs, a.n_envs, a.max_points, a.n_y, a.n_sec, a.n_param, a.rep = K, B, P, N, E, NPARAM, rep
    a.seed, a.game_step = 5, 7
    a.dtab[:] = [0.0, 1.0, 0.70710677, 0.57735026]
    for f in ("idx", "ms", "pts", "n", "arch_y", "arch_sec", "c_x", "c_target", "c_params", "ref_points", "env_ids"):
        setattr(a, f, t[f].data_ptr())
    for k in ("x", "target", "params", "y", "sec"):
        setattr(a, f"par_{k}", par[k].data_ptr())
        setattr(a, f"cand_{k}", cand[k].data_ptr())
    for k, v in out.items():
        setattr(a, k, v.data_ptr())
    for f, v in over.items():
        setattr(a, f, v)
    return a


@pytest.mark.gpu
def test_argument_checks_refuse_and_write_nothing():
    lib = tm.load()
    name = "odd_N"
    c, _ = _cached(name)
    t = _t(c, "cuda")
    par, cand, out = _sentinel_bufs(name, "cuda")
    # size_t, eight 32-bit words, two 64-bit scalars, four floats, twenty-nine pointers: truss_pair_args_t
    assert ctypes.sizeof(_lib.PairArgs) == 8 + 8 * 4 + 2 * 8 + 4 * 4 + 29 * 8

    def raw(match, **over):
        rc = lib.dll.truss_pair_setup(ctypes.byref(_raw_args(name, t, par, cand, out, **over)), None)
        assert rc == -1
        with pytest.raises(tm.TrussError, match=match):
            lib.check(rc, "truss_pair_setup")

    raw("struct_size", struct_size=8)
    raw("x_p is NULL", x_p=None)
    raw("cand_sec is NULL", cand_sec=None)
    raw("idx is NULL", idx=None)
    raw("env_ids is NULL", env_ids=None)                                    # coins asked for
    raw("output ref overlaps input frac_tab", frac_tab=out["ref"].data_ptr())
    # the train game's shape: no coin, no env ids -- every other pointer is still required
    train = dict(coin=None, env_ids=None)
    assert lib.dll.truss_pair_setup(ctypes.byref(_raw_args(name, t, par, cand, out, n_pairs=0, **train)), None) == 0
    for f in ("x_p", "A_p", "p0", "nn0", "parent_obj", "ref", "par_x", "par_params", "par_sec", "cand_target", "cand_y", "cand_sec", "pts",
              "arch_sec", "ms"):
        raw(f"{f} is NULL", **train, **{f: None})
    raw("output par_y overlaps input arch_y", **train, par_y=t["arch_y"].data_ptr())
    raw("flags must be 0", flags=1)
    raw("rep must be 1 or 3", rep=2)
    raw("rep must be 1 or 3", rep=0)
    raw("n_pairs < 0", n_pairs=-1)
    raw("max_points", max_points=0)
    raw("max_points", max_points=257)
    raw("n_y / n_sec / n_param", n_sec=0)
    raw("output par_y overlaps input arch_y", par_y=t["arch_y"].data_ptr())
    # (the aliased range lies inside the buffer it is pointed into, so that no third buffer can be the one the check names)
    raw("output parent_obj overlaps input pts", parent_obj=t["pts"].data_ptr() + 32)
    raw("output cand_x overlaps output par_x", par_x=cand["x"].data_ptr() + 4)
    raw("output parent_obj overlaps output nn0", nn0=out["parent_obj"].data_ptr())
    raw("par_params is not aligned", par_params=par["params"].data_ptr() + 4)
    # through the wrapper and the operator
    args = (t["idx"], t["ms"], t["pts"], t["n"], t["arch_y"], t["arch_sec"], t["c_x"], t["c_target"], t["c_params"], t["ref_points"])
    with pytest.raises(ValueError, match="rep must be 1 or 3"):
        marl.pair_setup(lib, *args, rep=2, dtab=[0.0, 1.0, 0.5, 0.25], par=par, cand=cand, out=out)
    with pytest.raises(tm.TrussError, match="output par_y overlaps input arch_y"):
        marl.pair_setup(lib, *args, rep=3, dtab=[0.0, 1.0, 0.5, 0.25], par=dict(par, y=t["arch_y"].view(-1, 33)), cand=cand, out=out)
    with pytest.raises(tm.TrussError, match="pts must be Double"):
        marl.pair_setup(lib, args[0], args[1], t["pts"].float(), *args[3:], rep=3, dtab=[0.0, 1.0, 0.5, 0.25], par=par, cand=cand, out=out)
    with pytest.raises(tm.TrussError, match="x_p must be"):
        marl.pair_setup(lib, *args, rep=3, dtab=[0.0, 1.0, 0.5, 0.25], par=par, cand=cand, out=dict(out, x_p=out["x_p"][:5]))
    # no pairs: success, nothing launched
    assert lib.dll.truss_pair_setup(ctypes.byref(_raw_args(name, t, par, cand, out, n_pairs=0)), None) == 0
    res = marl.pair_setup(lib, t["idx"][:0], t["ms"][:0], *args[2:], rep=3, dtab=[0.0, 1.0, 0.5, 0.25], par=par, cand=cand)
    assert res["x_p"].shape == (0, 20, 4) and res["A_p"].shape == (0, 20, 20) and res["p0"].shape == (0, 20, 4) and res["coin"] is None
    torch.cuda.synchronize()
    for group in (par, cand, out):
        for k, v in group.items():
            s = SENT_U8 if v.dtype == torch.uint8 else SENT_I if v.dtype == torch.int32 else SENT_F
            assert bool((v == s).all()), k
    for k, v in c.items():
        assert np.array_equal(t[k].cpu().numpy(), v), k


# ---- 4: the same game ----------------------------------------------------------------------------------------------------------------
def _play(lib, pair_path, game="train", **kw):
    """three game steps with exploration (and, in the train game, training) of a 6-env, 8-node engine with its own agents of a fixed
    seed (hidden width 40: inside the split-weight envelope of the grouped actor path); returns what two pair paths must agree on"""
    test = game == "test"
    with contextlib.redirect_stdout(io.StringIO()):
        eng = _engine(lib, "cuda", pair_path, _agents("cuda", 11, hidden=40), seed=11, game=game, **kw)
        assert eng.pair_path == pair_path and eng.topo.N == 8 and eng.B == 6
        stats, chunks = [], []
        for _ in range(3):
            chunks.append(-(-int(eng.n.sum()) // eng.cap) if not test else 0)
            stats.append(eng.game_step_all(train=not test, explore=True))
    state = [eng.pts, eng.n, eng.arch_y, eng.arch_sec]
    for s in stats:
        state += [v for _, v in sorted(s.items()) if torch.is_tensor(v)]
    if test:
        assert all("G_U" in s for s in stats)
        with contextlib.redirect_stdout(io.StringIO()):
            ep = eng.design_episode(end_step=eng.game_step + 1, explore=True)          # two more steps, the second one final
        state += [ep["hv"], ep["n_front"], ep["R"], ep["G_U"]] + [v for _, v in sorted(ep["final"].items())]
    else:
        assert max(chunks) >= 2, f"no game step needed two chunks of pairs ({chunks})"
        rp = eng.replay
        assert rp.size > 0
        state += [rp.S[k] for k in rp.KEYS] + [ns[k] for ns in rp.NS for k in rp.KEYS] + [rp.a_geo, rp.a_topo, rp.R]
        S, NS, ag, at, R = rp.sample(8, torch.Generator(device="cuda").manual_seed(5))
        state += [S[k] for k in rp.KEYS] + [ns[k] for ns in NS for k in rp.KEYS] + [ag, at, R]
    return state


def _same_game(lib, **kw):
    a, b = _play(lib, "torch", **kw), _play(lib, "hip", **kw)
    assert len(a) == len(b) and len(a) >= 4
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v), f"tensor {i} differs between pair_path 'torch' and 'hip'"


@pytest.mark.gpu
@pytest.mark.parametrize("others", ["defaults", "all_hip"])
def test_engines_differ_only_in_pair_path_train_game(others):
    """pair_capacity 6 (the smallest an engine of 6 envs takes): a step with more than 6 live members runs in two or more chunks"""
    kw = dict(pair_capacity=6)
    if others == "all_hip":
        kw.update(reward_path="hip", archive_path="hip", replay_storage="compact", actor_path="grouped")
    _same_game(tm.load(), **kw)


@pytest.mark.gpu
def test_engines_differ_only_in_pair_path_design_game():
    _same_game(tm.load(), game="test", max_front=50)
