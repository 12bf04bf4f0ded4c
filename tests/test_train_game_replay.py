"""The train game of the batched engine (`BatchedMARL.game_step_all(train=True)`, truss_mi355/marl.py: parents' analysis, three actors,
3 K candidate steps, difference reward, archive cull per chunk, replay append) against a float64 host model, step by step.

Action replay, as in tests/test_design_episode.py: the actions the engine's actors produced (after exploration noise) are recorded
per chunk (BatchedMARL._act) and replayed through a host model that restates the game from the module docstring of marl.py (D1-D5):
pair order and chunks, candidates and observations from the float64 oracle (oracle.env_step / fem_solve / state_data), the reward
block of the drop-in master script, culls from utils.simple_cull_final + the D3 truncation, the accepted flags (D2), the next-state
pick (D4), the Pareto graph from the drop-in pareto_state_data + pad_pareto_graph, and the replay ring.  The host model calls neither
the engine nor truss_mi355.reward nor any native entry -- the actors' own numerics stay out of the comparison.

After every game step the engine's archives, counters and step results are compared with the host's, and the replay ring row by
row (clamped actions, rewards, the observation tensors of the state and of the three next states, the Pareto graph).
Every case asserts on the host trace that the mechanism it is for was live, and three mutants of the host model (one cull per game
step, D4 off, accepted flags from a cull that ignores the candidates' feasibility) must fail the comparisons of the chunks case.

Mutant 3: an infeasible candidate is never a row of a front, by index or by value, so dropping "is feasible" from "is feasible and
is a row of the chunk's front" alone changes nothing; the mutant therefore judges "is a row of the front" on a cull in which the
candidates' constraints do not count (what accepted flags computed without the feasibility term would see), the archive itself
still coming from the right cull.
"""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import marl, pool, synthetic
import parity_common as pc
from oracle import truss_oracle as O
import utils as U
import master_DDPG_truss2D_MO as M
import truss2D_ENV as ENV
import truss2D_RL as RL

OBS = ("x_n", "A_s", "A_n_ts", "A_n_cs")
ALL_HIP = dict(reward_path="hip", archive_path="hip", replay_storage="compact", actor_path="fused")
SETTINGS = {"defaults": {}, "reward_hip": dict(reward_path="hip"), "archive_hip": dict(archive_path="hip"), "all_hip": ALL_HIP}

# the smallest shapes at which each mechanism is live.  batch_seed: synthetic.random_batch; seed: the agents' weights and the engine's
# noise stream.  The seeds were searched over 0 .. 9 with the host model, so that the case's conditions (`_conditions`, and at most
# half of the reward units tied) hold on the emulator's trace and on the MI355X's, which differ (weights and noise are drawn on
# the device); about a quarter of the seeds leave more than half of the units tied (two archive rows clipped to obj1 = 1.0).
CASES = {
    "chunks": dict(num_x=4, B=6, steps=5, batch_seed=3, seed=5, max_front=20, pair_capacity=8, replay_capacity=256),
    "fold": dict(num_x=4, B=6, steps=5, batch_seed=3, seed=5, max_front=61, pair_capacity=8, replay_capacity=256),
    "truncate": dict(num_x=4, B=8, steps=5, batch_seed=0, seed=4, max_front=4, pair_capacity=8, replay_capacity=256),
    "wrap": dict(num_x=4, B=6, steps=5, batch_seed=3, seed=5, max_front=20, pair_capacity=8, replay_capacity=16),
    "nodes16": dict(num_x=8, B=64, steps=5, batch_seed=3, seed=4),
}


# ---- engine, recording ----
def _rl(device, seed, hidden=16):
    torch.manual_seed(seed)
    return RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, hidden, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)


def _engine(lib, device, case, **setting):
    c = CASES[case]
    topo = tm.TrussTopology.grid(c["num_x"])
    kw = {k: c[k] for k in ("max_front", "pair_capacity", "replay_capacity") if k in c}
    eng = marl.BatchedMARL(topo, c["B"], _rl(device, c["seed"]), lib=lib, device=device, batch_size=8, seed=c["seed"], **kw, **setting)
    b = synthetic.random_batch(topo, c["B"], c["batch_seed"])
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng, b


def _record(eng):
    """wrap the engine's actors: the actions of every chunk of every game step, after exploration noise"""
    rec = {}
    act0 = eng._act

    def act(S, explore):
        g, t = act0(S, explore)
        rec.setdefault(eng.game_step, []).append(([x.detach().cpu().numpy().copy() for x in g],
                                                  [x.detach().cpu().numpy().copy() for x in t]))
        return g, t

    eng._act = act
    return rec


def _snapshot(eng, out):
    np_ = lambda v: v.detach().cpu().numpy().copy() if torch.is_tensor(v) else v
    return dict(pts=np_(eng.pts), n=np_(eng.n), y=np_(eng.arch_y), sec=np_(eng.arch_sec), out={k: np_(v) for k, v in out.items()},
                size=eng.replay.size, head=eng.replay.head, ring=_ring(eng))


def _ring(eng):
    """the rows 0 .. size - 1 of the engine's replay ring as dense numpy tensors (compact storage: through DeviceReplay._get, what
    `sample` returns)"""
    r = eng.replay
    i = torch.arange(r.size, device=r.R.device)
    get = lambda d: {k: r._get(d[k], k, i).cpu().numpy() for k in r.KEYS}
    return dict(S=get(r.S), NS=[get(ns) for ns in r.NS], geo=r.a_geo[i].cpu().numpy(), topo=r.a_topo[i].cpu().numpy(), R=r.R[i].cpu().numpy())


def _play(engines, step, T):
    """T game steps (train=True, explore=True, no updates) -> per engine (recorded actions, snapshot per step, ring after the last)"""
    recs = [_record(e) for e in engines]
    snaps = [[] for _ in engines]
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(T):
            outs = step()
            for s, e, o in zip(snaps, engines, outs):
                s.append(_snapshot(e, o))
    return [dict(rec=r, snaps=s, ring=s[-1]["ring"]) for r, s in zip(recs, snaps)]


# ---- host model ----
@contextlib.contextmanager
def _max_front(P):
    """MAX_FRONT of the drop-in reward block (utils) and Pareto graph (truss2D_ENV) set to the engine's, as truss2D_ENV.configure does"""
    old = U.MAX_FRONT, ENV.MAX_FRONT
    U.MAX_FRONT = ENV.MAX_FRONT = P
    try:
        yield
    finally:
        U.MAX_FRONT, ENV.MAX_FRONT = old


def _d3(rows, order, max_front):
    """D3 (tests/test_front_wide.py::_d3): both ends + the max_front - 2 interior rows of largest crowding distance (ties: earlier
    position), in front order"""
    nf = len(order)
    if nf <= max_front:
        return list(order)
    f = [rows[k] for k in order]
    d = [math.sqrt((f[k][0] - f[k + 1][0]) ** 2 + (f[k][1] - f[k + 1][1]) ** 2) for k in range(nf - 1)]
    cr = [d[0]] + [d[k - 1] + d[k] for k in range(1, nf - 1)] + [d[-1]]
    keep = {0, nf - 1} | set(sorted(range(1, nf - 1), key=lambda k: -cr[k])[:max_front - 2])
    return [order[k] for k in range(nf) if k in keep]


def _front_order(rows):
    """rows [o1, o2, c1, c2] -> the input rows of the front of the feasible ones (utils.simple_cull_final), the first of identical
    rows, ordered by (obj1, obj2, input row)"""
    feas = [k for k, r in enumerate(rows) if not (r[2] > 1 or r[3] > 1)]
    fr = U.simple_cull_final([list(rows[k]) for k in feas])[0]
    first = {}
    for k in feas:
        first.setdefault(tuple(rows[k]), k)
    return sorted((first[tuple(r)] for r in fr), key=lambda k: (rows[k][0], rows[k][1], k))


def _sum_distance(rows):
    """sum_distance of utils.simple_cull_final on archive rows (a front already).  The drop-in sorts the front by obj1 alone and
    leaves rows of EQUAL obj1 (objectives clipped to 1.0) in the iteration order of a Python set (utils.py:53-60); there the rows are
    handed over one at a time in the kernel's documented order (obj1, obj2), so that the reference is defined for every archive"""
    if len({r[0] for r in rows}) == len(rows):
        return U.simple_cull_final(rows)[4]
    fr = sorted(rows, key=lambda r: (r[0], r[1]))
    assert len(U.simple_cull_final(rows)[0]) == len(fr)
    return sum(U.simple_cull_final([fr[k], fr[k + 1]])[4] for k in range(len(fr) - 1))


def _reward_truncates(front, pts3, P):
    """the host reward block cuts a front with random.sample (utils.py:120-142): one of its four culls (leave one agent out x 3, all)
    has more than MAX_FRONT non-dominated rows"""
    feas = [max(p) <= 1.0 for p in pts3]
    if len(front) + sum(feas) <= P:
        return False
    sets = [[j for j in range(3) if j != i and feas[j]] for i in range(3)] + [[j for j in range(3) if feas[j]]]
    return any(len(U.simple_cull_final([list(r) for r in front] + [list(pts3[j]) for j in s])[0]) > P for s in sets)


class _Host:
    """the train game on the host.  mutant: None, or 1 = one cull per game step instead of one per chunk, 2 = every agent's next state
    is its own candidate (no D4), 3 = accepted flags from a cull that ignores the candidates' feasibility (module docstring)"""

    def __init__(self, topo, batch, P, pair_capacity, replay_capacity, mutant=None):
        self.ot = pc.oracle_topology(topo)
        self.batch, self.B, self.P, self.mutant = batch, batch["y"].shape[0], P, mutant
        B = self.B
        self.load = pc.oracle_load(self.ot, batch)
        self.int_obj = O.initial_objectives(self.ot, batch["x"], batch["y"], batch["sec"], batch["target"])
        self.Gm = max(1, min(P, (64 - P) // 3))
        self.cap = max(pair_capacity or min(B * self.Gm, 4 * B), B)
        self.arch = [[(np.array([1.0, 1.0, 0.0, 0.0]), batch["y"][b].astype(np.float32), batch["sec"][b].astype(np.int32))] for b in range(B)]
        self.capacity, self.ring, self.head, self.size = replay_capacity, {}, 0, 0
        self.stats = dict(chunks=[], groups=[], truncated_culls=0, rejected_feasible=0, d4_pairs=0, d4_accepted=0, wrapped=False,
                          culls=0, max_front_len=0)

    def _graph(self, front, index):
        x, A = ENV.pareto_state_data(front, index=index)
        x, A = M.pad_pareto_graph(x, A, size=self.P)
        return np.asarray(x, np.float64), np.asarray(A, np.float64)

    def step(self, chunks_rec):
        """one game step on the recorded actions -> dict(arch, R [B, 3], tied [B], added, size, head)"""
        ot, bt, B, P, Gm, st = self.ot, self.batch, self.B, self.P, self.Gm, self.stats
        start = [list(a) for a in self.arch]
        n0 = [len(a) for a in start]
        front0 = [[[float(v) for v in r[0]] for r in a] for a in start]
        chunks = []
        for g0 in range(0, max(n0), Gm):                                  # member groups; inside a group the pairs are member-major
            pairs = [(m, b) for m in range(g0, g0 + Gm) for b in range(B) if m < n0[b]]
            chunks += [(g0, pairs[c:c + self.cap]) for c in range(0, len(pairs), self.cap)]
        st["chunks"].append(len(chunks))
        st["groups"].append(len(range(0, max(n0), Gm)))
        assert [len(p) for _, p in chunks] == [c[0][0].shape[0] for c in chunks_rec], "the engine's chunks are not the host's"
        flat = [p for _, ps in chunks for p in ps]
        pm, pb = np.array([p[0] for p in flat]), np.array([p[1] for p in flat])
        geo = [np.concatenate([c[0][a] for c in chunks_rec]) for a in range(3)]
        top = [np.concatenate([c[1][a] for c in chunks_rec]) for a in range(3)]
        py = np.stack([start[b][m][1] for m, b in flat])
        ps = np.stack([start[b][m][2] for m, b in flat])
        pick = lambda a: np.asarray(a)[pb] if np.ndim(a) else a
        x, target, load = bt["x"][pb], bt["target"][pb], self.load[pb]
        y_max, d_min, max_def, is_roof = pick(bt["y_max"]), pick(bt["d_min"]), pick(bt["max_def"]), pick(bt["is_roof"])
        outs = [O.env_step(ot, x, py, ps, None, None, geo[a], top[a], None, target, load, y_max, d_min, max_def, is_roof, self.int_obj[pb],
                           with_obs=True) for a in range(3)]
        # the parents' observations: analysis of the member's design
        fem = O.fem_solve(ot, x, py, ps, load)
        mu, md = O.move_range(ot, py, y_max, d_min, is_roof)
        has_load = (load[:, :, 1] != 0) | (load[:, :, 0] != 0)
        par = dict(zip(OBS, O.state_data(ot, x, py, ps, has_load, mu, md, target, fem, max_def)))
        R = np.zeros((B, 3))
        tied_env = np.zeros(B, bool)
        rows_of = []                                                       # per pair: what its replay row would hold
        for k, (m, b) in enumerate(flat):
            pts3 = [[float(v) for v in np.asarray(outs[a]["point"][k], np.float64)] for a in range(3)]
            r = M.difference_reward(front0[b], front0[b], tuple(front0[b][m][:2]), pts3, [1.0, 1.0], n0[b])[:3]
            x1 = [f[0] for f in front0[b]] + [p[0] for p in pts3 if max(p) <= 1.0]
            tied = len(set(x1)) < len(x1) or _reward_truncates(front0[b], pts3, P)
            tied_env[b] |= tied
            R[b] += r
            feas = [not (p[2] > 1 or p[3] > 1) for p in pts3]
            rows_of.append(dict(pts3=pts3, feas=feas, R=np.array(r, np.float64), tied=tied, key=(m, b)))
        added, off = 0, 0
        cull_chunks = [(0, flat)] if self.mutant == 1 else chunks
        for g0, pairs in cull_chunks:
            infront = set()
            per_env = {}
            for kl, (m, b) in enumerate(pairs):
                for a in range(3):
                    per_env.setdefault(b, []).append(((m - g0) * 3 + a, off + kl, a))
            for b in range(B):
                cl = sorted(per_env.get(b, []))                             # slot order
                na = len(self.arch[b])
                rows = list(self.arch[b]) + [(np.array(rows_of[k]["pts3"][a]), outs[a]["y"][k], outs[a]["sec"][k]) for _, k, a in cl]
                p4 = [[float(v) for v in r[0]] for r in rows]
                order = _front_order(p4)
                keep = _d3(p4, order, P)
                st["culls"] += 1
                st["truncated_culls"] += len(order) > P
                st["max_front_len"] = max(st["max_front_len"], len(order))
                if self.mutant == 3:                                        # flags from a cull without the candidates' feasibility
                    q4 = p4[:na] + [r[:2] + [0.0, 0.0] for r in p4[na:]]
                    flagged = _d3(q4, _front_order(q4), P)
                else:
                    flagged = keep
                infront |= {(k, a) for j, (_, k, a) in enumerate(cl) if na + j in flagged and (self.mutant == 3 or rows_of[k]["feas"][a])}
                self.arch[b] = [(np.concatenate([np.minimum(rows[k][0][:2], 1.0), rows[k][0][2:]]), rows[k][1], rows[k][2]) for k in keep]
            new = []
            for kl in range(len(pairs)):
                k = off + kl
                ro = rows_of[k]
                feas = ro["feas"]
                acc = [(k, a) in infront for a in range(3)]
                st["rejected_feasible"] += sum(f and not c for f, c in zip(feas, acc))
                sub = any(feas) and not all(feas)
                st["d4_pairs"] += sub
                if not any(acc):
                    continue
                st["d4_accepted"] += sub
                first_ok = feas.index(True) if any(feas) else 0
                src = [a if (feas[a] or self.mutant == 2) else first_ok for a in range(3)]           # D4
                m, b = ro["key"]
                x_p, A_p = self._graph(front0[b], m)
                new.append(dict(geo=np.stack([outs[a]["geo"][k] for a in range(3)]), topo=np.stack([outs[a]["topo"][k] for a in range(3)]),
                                R=ro["R"], tied=ro["tied"], S={o: par[o][k] for o in OBS}, NS=[{o: outs[s][o][k] for o in OBS} for s in src],
                                x_p=x_p, A_p=A_p, key=ro["key"]))
            new = new[:self.capacity]
            for j, row in enumerate(new):
                self.ring[(self.head + j) % self.capacity] = row
            st["wrapped"] |= self.head + len(new) > self.capacity
            self.head = (self.head + len(new)) % self.capacity
            self.size = min(self.capacity, self.size + len(new))
            added += len(new)
            off += len(pairs)
        return dict(arch=[list(a) for a in self.arch], R=R, tied=tied_env, added=added, size=self.size, head=self.head)


# ---- comparisons ----
def _compare_ring(ring, host, fig, t):
    """the rows of the engine's replay ring after game step t against the host ring, row by row"""
    assert ring["R"].shape[0] == host.size and sorted(host.ring) == list(range(host.size)), (t, ring["R"].shape[0], host.size)
    want = [host.ring[i] for i in range(host.size)]
    if want:
        np.testing.assert_array_equal(ring["geo"], np.stack([w["geo"] for w in want]).astype(np.float32))
        np.testing.assert_array_equal(ring["topo"], np.stack([w["topo"] for w in want]).astype(np.float32))
        ok = np.array([not w["tied"] for w in want])
        fig["rows"], fig["rows_tied"] = int(ok.sum()), int((~ok).sum())
        wR = np.stack([w["R"] for w in want]).astype(np.float32).astype(np.float64)
        dR = np.abs(ring["R"].astype(np.float64) - wR)
        if ok.any():
            fig["d_R"] = max(fig["d_R"], float(dR[ok].max()))
        assert np.all(dR[ok] <= 1e-9 + 2.0 ** -23 * np.abs(wR[ok])), float(dR[ok].max())
        for name, got, pick in [("S", ring["S"], lambda w: w["S"])] + [(f"NS{a}", ring["NS"][a], lambda w, a=a: w["NS"][a]) for a in range(3)]:
            for key in OBS:                                            # the bound of parity_common.compare_obs: 2e-6 of the column scale
                ref = np.stack([pick(w)[key] for w in want])
                assert got[key].shape == ref.shape, (t, name, key)
                scale = np.maximum(np.abs(ref).reshape(-1, ref.shape[-1]).max(axis=0), 1.0)
                err = float((np.abs(got[key] - ref) / scale).max())
                fig["d_obs"] = max(fig["d_obs"], err)
                assert err < 2e-6, (t, name, key, err)
            for key in ("x_p", "A_p"):                                 # the step-start front's graph, for the state and all next states
                ref = np.stack([w[key] for w in want])
                err = float(np.abs(got[key] - ref).max())
                fig["d_graph"] = max(fig["d_graph"], err)
                assert err <= 1e-6, (t, name, key, err)


def _compare(trace, topo, batch, P, pair_capacity, replay_capacity, mutant=None, label=None):
    """the engine's trace against the host model, game step by game step, the replay ring included.  Returns (host stats, figures;
    the row counts are those of the ring after the last step)."""
    host = _Host(topo, batch, P, pair_capacity, replay_capacity, mutant)
    B, T = host.B, len(trace["snaps"])
    fig = dict(units=0, units_tied=0, rows=0, rows_tied=0, d_arch=0.0, d_reward=0.0, d_obs=0.0, d_graph=0.0, d_R=0.0, d_hv=0.0)
    with _max_front(P):
        for t in range(T):
            h = host.step(trace["rec"][t + 1])
            s = trace["snaps"][t]
            o = s["out"]
            for b in range(B):
                want = h["arch"][b]
                n = int(s["n"][b])
                assert n == len(want) == int(o["n_front"][b]), f"step {t} env {b}: n {n}, host {len(want)}"
                wp = np.stack([w[0] for w in want])
                fig["d_arch"] = max(fig["d_arch"], float(np.abs(s["pts"][b, :n] - wp).max()))
                np.testing.assert_allclose(s["pts"][b, :n], wp, rtol=0, atol=1e-9, err_msg=f"step {t} env {b}")
                np.testing.assert_array_equal(s["y"][b, :n], np.stack([w[1] for w in want]).astype(np.float32))
                np.testing.assert_array_equal(s["sec"][b, :n], np.stack([w[2] for w in want]))
                rows = [list(r) for r in s["pts"][b, :n]]
                d_hv = abs(o["hv"][b] - U.union_rectangles_fastest(rows, +1, -1, ref_point=[1, 1]))
                d_sd = abs(o["sum_distance"][b] - _sum_distance(rows))
                fig["d_hv"] = max(fig["d_hv"], float(d_hv), float(d_sd))
                assert d_hv <= 1e-12 and d_sd <= 1e-12, (t, b, d_hv, d_sd)
            assert int(o["replay_added"]) == h["added"], f"step {t}: replay_added {o['replay_added']}, host {h['added']}"
            assert int(o["replay_size"]) == s["size"] == h["size"] and s["head"] == h["head"], (t, o["replay_size"], s["size"], s["head"], h)
            ok = ~h["tied"]
            assert ok.any(), f"step {t}: every env is tied"
            fig["units"] += int(ok.sum())
            fig["units_tied"] += int((~ok).sum())
            assert o["reward"].shape == (B, 3)
            fig["d_reward"] = max(fig["d_reward"], float(np.abs(o["reward"][ok] - h["R"][ok]).max()))
            np.testing.assert_allclose(o["reward"][ok], h["R"][ok], rtol=0, atol=1e-9, err_msg=f"step {t}")
            assert np.isfinite(o["reward"]).all()
            _compare_ring(s["ring"], host, fig, t)                        # (a ring that wraps: every row before it is overwritten)
        assert fig["units_tied"] <= (fig["units"] + fig["units_tied"]) // 2, fig
    st = host.stats
    if label:
        tot = fig["units"] + fig["units_tied"]
        print(f"\n[train game {label}] chunks per step {st['chunks']}, member groups per step {st['groups']}, culls {st['culls']} "
              f"(truncated {st['truncated_culls']}, longest front {st['max_front_len']}), rejected feasible candidates {st['rejected_feasible']}, "
              f"D4 substitutions {st['d4_pairs']} pairs ({st['d4_accepted']} in the replay), ring wrapped {st['wrapped']}; "
              f"reward units compared {fig['units']} / left out as tied {fig['units_tied']} ({fig['units_tied'] / tot:.0%}), "
              f"replay rows compared {fig['rows']} / tied {fig['rows_tied']}; largest deviation: archive rows {fig['d_arch']:.3g} (1e-9), "
              f"step rewards {fig['d_reward']:.3g} (1e-9), replay R {fig['d_R']:.3g} (1e-9 + 2^-23 |R|), hv / sum_distance {fig['d_hv']:.3g} (1e-12), "
              f"observations {fig['d_obs']:.3g} (2e-6), Pareto graph {fig['d_graph']:.3g} (1e-6)")
    return st, fig


def _conditions(case, st):
    """what the case is for was live in the host trace"""
    if case in ("chunks", "wrap"):
        assert max(st["chunks"]) >= 2 and st["d4_pairs"] >= 1 and st["rejected_feasible"] >= 1, st
    if case == "fold":
        assert max(st["groups"]) >= 2, st
    if case == "truncate":
        assert st["truncated_culls"] >= 1, st
    if case == "wrap":
        assert st["wrapped"], st


def _run_case(lib, device, case, setting="defaults"):
    c = CASES[case]
    eng, batch = _engine(lib, device, case, **SETTINGS[setting])
    trace = _play([eng], lambda: [eng.game_step_all(train=True, explore=True, train_iters=0)], c["steps"])[0]
    for k, v in SETTINGS[setting].items():
        assert getattr(eng, k) == v
    if device == "cuda" and eng.replay_storage == "compact":
        assert eng.replay._lib is not None                                  # the fused replay operators did run
    else:
        assert eng.replay._lib is None
    assert eng.P == c.get("max_front", 20) and eng.replay.capacity == c.get("replay_capacity", 32768)
    st, fig = _compare(trace, eng.topo, batch, eng.P, c.get("pair_capacity"), eng.replay.capacity, label=f"{case} {setting} {device}")
    assert st["chunks"] and eng.cap == max(c.get("pair_capacity") or min(c["B"] * eng.Gm, 4 * c["B"]), c["B"])
    _conditions(case, st)
    assert int(trace["snaps"][-1]["n"].max()) >= 2 and trace["ring"]["R"].shape[0] >= 1       # archives grew, the replay filled
    return eng, batch, trace


# ---- emulator ----
@pytest.fixture(scope="module")
def chunks_trace():
    eng, batch, trace = _run_case(pc.emu_lib(), "cpu", "chunks")
    return eng.topo, batch, trace


def test_train_game_chunks_emulated(chunks_trace):
    assert chunks_trace[2]["ring"]["R"].shape[0] >= 1


@pytest.mark.parametrize("case", ["fold", "truncate", "wrap", "nodes16"])
def test_train_game_emulated(case):
    _run_case(pc.emu_lib(), "cpu", case)


@pytest.mark.parametrize("mutant", [1, 2, 3])
def test_host_model_mutants_fail_the_chunks_case(chunks_trace, mutant):
    """teeth: one cull per game step / no D4 / accepted flags without feasibility, on the recorded trace of the chunks case"""
    topo, batch, trace = chunks_trace
    c = CASES["chunks"]
    with pytest.raises(AssertionError) as e:
        _compare(trace, topo, batch, c["max_front"], c["pair_capacity"], c["replay_capacity"], mutant=mutant)
    print(f"\n[train game mutant {mutant}] fails with: {' '.join(str(e.value).split())[:200]}")


def _run_mixed(lib, device, **setting):
    """two size classes, one set of agents: env_ids and the update=False path of every class engine"""
    classes = pool.grid_classes([4, 6], [48, 32])
    mix = marl.MixedMARL(classes, _rl(device, 4), bucket_envs=8, lib=lib, device=device, replay_capacity=1024, batch_size=8, seed=2, **setting)
    per_class = []
    for k, e in enumerate(mix.engines):
        full = synthetic.random_batch(e.topo, classes[mix.class_ids[k]][1], 9 + k)
        per_class.append({key: v[mix.global_ids(k)] for key, v in full.items()})
    mix.reset(per_class)
    assert [e.topo.N for e in mix.engines] == [8, 12] and [e.B for e in mix.engines] == [48, 32]
    traces = _play(mix.engines, lambda: mix.game_step_all(train=True, explore=True, train_iters=0)["per_class"], 3)
    for k, (e, b, tr) in enumerate(zip(mix.engines, per_class, traces)):
        st, _ = _compare(tr, e.topo, b, e.P, None, e.replay.capacity, label=f"mixed class {k} ({e.topo.N} nodes) {device}")
        assert tr["ring"]["R"].shape[0] >= 1 and int(tr["snaps"][-1]["n"].max()) >= 2
    return mix


def test_train_game_mixed_emulated():
    _run_mixed(pc.emu_lib(), "cpu")


# ---- HIP ----
@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_train_game_chunks_hip(setting):
    _run_case(tm.load(), "cuda", "chunks", setting)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["defaults", "all_hip"])
@pytest.mark.parametrize("case", ["fold", "truncate", "wrap"])
def test_train_game_hip(case, setting):
    _run_case(tm.load(), "cuda", case, setting)


@pytest.mark.gpu
def test_train_game_16_nodes_hip():
    """grid(8), B = 64, every default of the engine: the size of test_design_replay_hip"""
    _run_case(tm.load(), "cuda", "nodes16")


@pytest.mark.gpu
def test_train_game_mixed_hip():
    mix = _run_mixed(tm.load(), "cuda")
    assert all(e.replay._lib is None for e in mix.engines)
