"""Diagnostic: the dense and the compact observation layout side by side, in ONE process.

Every item is timed in blocks dense, compact, dense, compact, dense -- each block synchronised, after a warm-up of both layouts --
and reported as one JSON line: the time of every block, and the bytes a launch writes computed from the shapes.

    python tools/obs_compact_probe.py [items ...]        items: step obs actors game mixed   (default: step obs actors)

  step    the state-emitting step (TRUSS_F_EMIT_OBS) at 4096 envs of the metric topology (32 nodes / 80 elements)
  obs     truss_obs alone, and the step + truss_obs pair of a step with observations, at the 64-, 128- and 256-node classes with the
          env counts of the mixed sweep (512 / 256 / 128)
  actors  actor_infer over 4096 pairs of small_roof (16 nodes) and over 128 pairs of the 256-node class
  game    one game step without training on small_roof at 4096 envs, three alternating runs per layout
  mixed   the mixed sweep without training, three alternating runs per layout
  parent=<library>   (with obs) also the DENSE truss_obs of another build of the same ABI, blocks parent, this, parent, this, parent
"""
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mop-truss-marl_amd"), ROOT]
import numpy as np
import torch

import truss_mi355 as tm
from truss_mi355 import gcn, marl, pool, synthetic

LAYOUTS = ("dense", "compact")
ORDER = ("dense", "compact", "dense", "compact", "dense")
dev = torch.device("cuda", 0)
lib = tm.load()


def timed(fn, reps):
    """us per call over `reps` calls between two events, synchronised on both sides"""
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a0.record()
    for _ in range(reps):
        fn()
    a1.record()
    torch.cuda.synchronize()
    return a0.elapsed_time(a1) * 1e3 / reps


def blocks(calls, reps=30, warm=5):
    for fn in calls.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in calls}
    for layout in ORDER:
        out[layout].append(round(timed(calls[layout], reps), 2))
    return out


def report(name, us, nbytes, **more):
    print(json.dumps(dict(item=name, us=us, bytes_written=nbytes, **more)), flush=True)


def make_env(topo, B, seed, lib=lib):
    b = synthetic.random_batch(topo, B, seed=seed)
    e = tm.BatchedTruss(topo, B, device=dev, lib=lib)
    e.set_constants(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"])
    e.set_design(b["y"], b["sec"])
    e.analyze(set_normalisers=True)
    return e


def obs_bytes(e, layout, B):
    N, E, W = e.N, e.E, e.obs_width(layout)
    return 4 * (13 * N + 3 * N * W + 12 * N + 21 * E) * B


def item_step():
    topo, B = synthetic.bench_topology(16, 4), 4096
    e = make_env(topo, B, 1)
    ag, at = synthetic.random_actions(1, B, topo.N, 2)
    g, t = torch.tensor(ag[0], device=dev), torch.tensor(at[0], device=dev)
    y0, s0 = e.y.clone(), e.sec.clone()

    def call(layout):
        def fn():                                     # every launch steps the same design
            e.y.copy_(y0)
            e.sec.copy_(s0)
            e.step(g, t, obs=True, obs_layout=layout)
        return fn

    def copies():
        e.y.copy_(y0)
        e.sec.copy_(s0)
    base = round(timed(copies, 30), 2)
    us = blocks({k: call(k) for k in LAYOUTS})
    report("state-emitting step, 32 nodes / 80 elements, 4096 envs", us, {k: obs_bytes(e, k, B) for k in LAYOUTS}, fused=e.fused_obs,
           us_of_the_two_row_copies_included=base, Kc=e.obs_width("compact"))


def item_obs():
    for nx, B in ((32, 512), (64, 256), (128, 128)):
        topo = tm.TrussTopology.grid(nx)
        e = make_env(topo, B, nx)
        ag, at = synthetic.random_actions(1, B, topo.N, 2)
        g, t = torch.tensor(ag[0], device=dev), torch.tensor(at[0], device=dev)
        y0, s0 = e.y.clone(), e.sec.clone()
        nb = {k: obs_bytes(e, k, B) for k in LAYOUTS}
        report(f"truss_obs, {topo.N} nodes, {B} envs", blocks({k: (lambda k=k: e.observe(obs_layout=k)) for k in LAYOUTS}), nb, Kc=e.obs_width("compact"))

        def pair(layout):
            def fn():
                e.y.copy_(y0)
                e.sec.copy_(s0)
                e.step(g, t, obs=True, obs_layout=layout)
            return fn
        report(f"step + truss_obs, {topo.N} nodes, {B} envs", blocks({k: pair(k) for k in LAYOUTS}), nb, fused=e.fused_obs)
        if PARENT:                                     # the dense kernel against another build's (blocks() alternates its two keys)
            ep = make_env(tm.TrussTopology.grid(nx), B, nx, lib=tm.load(PARENT))
            us = blocks({"dense": ep.observe, "compact": e.observe})
            report(f"dense truss_obs against {PARENT}, {topo.N} nodes, {B} envs", {"other build": us["dense"], "this build": us["compact"]}, nb["dense"])


def item_actors():
    import master_DDPG_truss2D_MO as M
    import truss2D_RL as RL
    for nx, B in ((8, 4096), (128, 128)):
        topo = tm.TrussTopology.grid(nx)
        N, P = topo.N, 20
        rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, M.a_nn, M.c_nn, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=dev)
        actor = rl.agents[0].actor_model
        e = make_env(topo, B, nx)
        nbr = torch.tensor(topo.neighbor_table(), device=dev)
        nbr_p = torch.tensor(marl.path_graph_table(P), device=dev)
        A_n = torch.tensor(topo.normalized_adjacency()[0], device=dev)
        x_p, A_p = torch.rand(B, P, 4, device=dev), torch.rand(B, P, P, device=dev) * 0.1
        ins = {}
        for layout in LAYOUTS:
            o = {k: v.clone() for k, v in e.observe(obs_layout=layout).items()}
            ins[layout] = [o["x_n"], A_n, o["A_s"], o["A_n_ts"], o["A_n_cs"], x_p, A_p]
        with torch.no_grad():
            outs = {k: gcn.actor_infer(lib, actor, ins[k], nbr=nbr, nbr_p=nbr_p, fused=True, compact=k == "compact") for k in LAYOUTS}
            same = all(torch.equal(a, b) for a, b in zip(outs["dense"], outs["compact"]))
            us = blocks({k: (lambda k=k: gcn.actor_infer(lib, actor, ins[k], nbr=nbr, nbr_p=nbr_p, fused=True, compact=k == "compact")) for k in LAYOUTS},
                        reps=10, warm=3)
        W = {k: e.obs_width(k) for k in LAYOUTS}
        report(f"actor_infer (fused), {N} nodes, {B} pairs", us, {k: 4 * 3 * N * W[k] * B for k in LAYOUTS}, bytes_are="the three adjacencies read",
               outputs_equal=same)


def _with_env(layout, fn):
    old = {k: os.environ.get(k) for k in ("TRUSS_OBS_LAYOUT", "TRUSS_REPLAY_STORAGE")}
    os.environ["TRUSS_OBS_LAYOUT"], os.environ["TRUSS_REPLAY_STORAGE"] = layout, "compact"   # (the replay is not used: no training)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def item_game(mixed=False):
    import bench_configs as BC
    runs = {k: [] for k in LAYOUTS}
    for layout in ("dense", "compact") * 3:
        r = _with_env(layout, (lambda: BC.mixed_marl(train=False, dev=dev)) if mixed else (lambda: BC.marl_small_roof(4096, 4, False, dev=dev)))
        runs[layout].append(round(r["env_steps_per_s"]))
    name = "mixed sweep without training" if mixed else "game steps without training, small_roof, 4096 envs"
    print(json.dumps(dict(item=name, env_steps_per_s=runs)), flush=True)


PARENT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)

if __name__ == "__main__":
    items = [a for a in sys.argv[1:] if not a.startswith("parent=")] or ["step", "obs", "actors"]
    for it in items:
        {"step": item_step, "obs": item_obs, "actors": item_actors, "game": item_game, "mixed": lambda: item_game(True)}[it]()
