"""Diagnostic: the set-up of a chunk of (env, member) pairs of a game step as the engine's torch block (gathers of the step-start
archive and the per-env constants, copies into the parent / candidate env buffers, pareto_graph, repeat, design_coins) against one
truss_pair_setup launch (marl.pair_setup), timed in ONE process.

    python tools/pair_probe.py [OUT_DIR]        -> OUT_DIR/pair_probe.json   (default OUT_DIR: build/pair_probe)

The driver starts two child processes, one after the other, each once and under its own `timeout` (no retry; the second only if the
first ended well).  "time" reports the median wall time (host side included) of 60 synchronised calls after 10 warm-up calls per
path, in alternating blocks of 15: torch, hip, torch again, ... (the two torch medians give the spread a difference has to exceed),
and whether the two paths' outputs are equal at the timed sizes.  "launches" counts the device kernels of one call of each path with
torch.profiler (a run of its own: tracing slows the host).
Shapes (K pairs over B envs, P archive rows, n_y / n_sec words per design, rep copies of the Pareto graph, coins or not): the train
game's chunks at the small_roof widths (16 nodes / 29 elements) at 512, 4096 and 14 336 pairs, the design game's chunk (P = 50, one
copy, coins) and the 256-node class at 512 pairs.  Archives half full; pairs member-major over the live members, as the engine lists
them.  Both paths write the design rows into the same resident buffers (the env objects' in the engine) and return the rest."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mop-truss-marl_amd"))

SHAPES = (          # (label, K, B, P, n_y, n_sec, rep, coins)
    ("small_roof 512 pairs (P 20, rep 3)", 512, 128, 20, 16, 29, 3, False),
    ("small_roof 4096 pairs (P 20, rep 3)", 4096, 1024, 20, 16, 29, 3, False),
    ("small_roof 14336 pairs (P 20, rep 3)", 14336, 4096, 20, 16, 29, 3, False),
    ("design game 4096 pairs (P 50, rep 1, coins)", 4096, 1024, 50, 16, 29, 1, True),
    ("256 nodes 512 pairs (P 20, rep 3)", 512, 128, 20, 256, 636, 3, False),
)
ROUNDS, BLOCK = 4, 15          # timed calls per path: ROUNDS alternating blocks of BLOCK
NPARAM = 8


def setup(K, B, P, n_y, n_sec, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(K + B + P + n_y)
    n = np.full(B, max(P // 2, 1), np.int32)
    pts = rng.uniform(0.05, 0.95, size=(B, P, 4))
    pts[np.arange(P)[None, :] >= n[:, None]] = 0.0
    member, env = np.nonzero((np.arange(P)[None, :] < n[:, None]).T)         # member-major, as the engine lists its pairs
    assert member.size >= K
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    z = lambda rows, w, dt: torch.zeros((rows, w), dtype=dt, device=dev)
    bufs = lambda r: dict(x=z(r, n_y, f32), target=z(r, n_y, f32), params=z(r, NPARAM, f64), y=z(r, n_y, f32), sec=z(r, n_sec, i32))
    return dict(pts=t(pts, f64), n=t(n, i32), arch_y=t(rng.standard_normal((B, P, n_y)), f32), arch_sec=t(rng.integers(0, 30, size=(B, P, n_sec)), i32),
                c_x=t(rng.standard_normal((B, n_y)), f32), c_target=t(rng.standard_normal((B, n_y)), f32), c_params=t(rng.standard_normal((B, NPARAM)), f64),
                ref_points=t(rng.uniform(0.5, 1.0, size=(B, 2)), f64), env_ids=t((1 << 30) + np.arange(B), i64), idx=t(env[:K], i64),
                ms=t(member[:K], i64), par=bufs(K), cand=bufs(3 * K))


def torch_block(marl, t, rep, coins):
    """the set-up block of BatchedMARL.game_step_all / _obs (marl.py), seed 3 and game step 7 for the coins"""
    import torch
    idx, ms, par, cand = t["idx"], t["ms"], t["par"], t["cand"]
    K, P = int(idx.numel()), t["pts"].shape[1]
    ark = torch.arange(K, device=idx.device)
    p0, nn0 = t["pts"][idx].contiguous(), t["n"][idx].contiguous()
    py, ps = t["arch_y"][idx, ms], t["arch_sec"][idx, ms]
    cx, ct, cp = t["c_x"][idx], t["c_target"][idx], t["c_params"][idx]
    par["x"][:K], par["target"][:K], par["params"][:K] = cx, ct, cp
    par["y"][:K], par["sec"][:K] = py, ps
    x_p, A_p = marl.pareto_graph(p0, nn0, ms, P)
    cand["x"][:3 * K], cand["target"][:3 * K], cand["params"][:3 * K] = cx.repeat(3, 1), ct.repeat(3, 1), cp.repeat(3, 1)
    cand["y"][:3 * K], cand["sec"][:3 * K] = py.repeat(3, 1), ps.repeat(3, 1)
    coin = marl.design_coins(3, t["env_ids"][idx], 7, ms).t().contiguous().view(-1) if coins else None
    if rep > 1:
        x_p, A_p = x_p.repeat(rep, 1, 1), A_p.repeat(rep, 1, 1)
    return dict(p0=p0, nn0=nn0, parent_obj=p0[ark, ms, :2].contiguous(), ref=t["ref_points"][idx].contiguous(), x_p=x_p, A_p=A_p, coin=coin)


def paths(marl, lib, t, rep, coins, dtab):
    frac = marl.pair_frac_tab(t["pts"].shape[1], t["pts"].device)
    hip = lambda: marl.pair_setup(lib, t["idx"], t["ms"], t["pts"], t["n"], t["arch_y"], t["arch_sec"], t["c_x"], t["c_target"], t["c_params"],
                                  t["ref_points"], rep=rep, dtab=dtab, frac_tab=frac, coins=(3, t["env_ids"], 7) if coins else None, par=t["par"],
                                  cand=t["cand"])
    return {"torch": lambda: torch_block(marl, t, rep, coins), "hip": hip}


def design_rows(t):
    return [v.clone() for d in (t["par"], t["cand"]) for v in d.values()]


def child_time():
    import torch
    import truss_mi355 as tm
    from truss_mi355 import marl
    dev = torch.device("cuda")
    lib = tm.load()
    dtab = marl.pair_dtab(dev)
    out = {}
    for label, K, B, P, n_y, n_sec, rep, coins in SHAPES:
        t = setup(K, B, P, n_y, n_sec, dev)
        fn = paths(marl, lib, t, rep, coins, dtab)

        def times(f, n):
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            return ts

        for f in fn.values():
            times(f, 10)                                               # warm-up of every shape the timed calls use
        ts = {"torch": [], "hip": [], "torch_again": []}
        for _ in range(ROUNDS):                                        # alternating blocks: torch, hip, torch, ...
            for k in ts:
                ts[k] += times(fn["hip" if k == "hip" else "torch"], BLOCK)
        res = {"call_us": {k: round(statistics.median(v), 1) for k, v in ts.items()}, "calls_per_median": ROUNDS * BLOCK}
        a = fn["torch"]()
        rows_a = design_rows(t)
        for d in (t["par"], t["cand"]):
            for v in d.values():
                v.zero_()
        b = fn["hip"]()
        rows_b = design_rows(t)
        res["outputs_equal"] = all(bool(torch.equal(a[k], b[k])) for k in a if a[k] is not None) and all(
            bool(torch.equal(u, v)) for u, v in zip(rows_a, rows_b))
        out[label] = res
        del t, fn, a, b, rows_a, rows_b
        torch.cuda.empty_cache()
    print(json.dumps(out))


def child_launches():
    import torch
    from torch.profiler import profile, ProfilerActivity
    import truss_mi355 as tm
    from truss_mi355 import marl
    dev = torch.device("cuda")
    lib = tm.load()
    dtab = marl.pair_dtab(dev)
    out = {}
    for label, K, B, P, n_y, n_sec, rep, coins in SHAPES:
        if K != 4096:
            continue
        t = setup(K, B, P, n_y, n_sec, dev)
        for path, f in paths(marl, lib, t, rep, coins, dtab).items():
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                f()
                torch.cuda.synchronize()
            kern = {}
            for e in prof.key_averages():
                if e.device_type == torch.autograd.DeviceType.CUDA:
                    kern[e.key] = kern.get(e.key, 0) + e.count
            out[f"{label} path={path}"] = {"launches": sum(kern.values()), "native": {k[:60]: c for k, c in kern.items() if "truss_" in k}}
        del t
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    out_dir = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "pair_probe"))
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    env = dict(os.environ, TMPDIR="/tmp")
    result = {}
    for step, limit in (("time", "300"), ("launches", "180")):
        p = subprocess.run(["timeout", "-k", "10", limit, sys.executable, me, "--child", step], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        with open(os.path.join(out_dir, step + ".err"), "w") as f:
            f.write(p.stderr[-20000:])
        if p.returncode != 0:
            print(f"the {step} step failed with status {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
            sys.exit(1)
        result[step] = json.loads(p.stdout.strip().splitlines()[-1])
        with open(os.path.join(out_dir, "pair_probe.json"), "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        {"time": child_time, "launches": child_launches}[sys.argv[2]]()
    else:
        main()
