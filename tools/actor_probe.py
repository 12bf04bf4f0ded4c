"""Diagnostic: actor inference as 13 launches of the fused layer kernel (marl.actor_infer) against the path that keeps the Pareto pool
and the two action heads in the epilogues of the layers that feed them (actor_infer(fused=True): 11 launches, truss_gcn_layer_fused),
timed in ONE process.

    python tools/actor_probe.py [OUT_DIR]        -> OUT_DIR/actor_probe.json   (default OUT_DIR: build/actor_probe)

The driver starts two child processes, one after the other, each once and under its own `timeout` (no retry; the second only if the
first ended well).  "time" reports the median wall time (host side included) of 60 synchronised actor_infer calls after 10 warm-up
calls per path, in alternating blocks of 15: layers, fused, layers again, ... (the two layers medians give the spread a difference
has to exceed), and the largest difference between the two paths' outputs.  "launches" counts the device kernels of one call of
each path with torch.profiler (a run of its own: tracing slows the host) and lists, with their device time, the three fused launches
next to the launches they replace (the 200 -> 200 layers that feed the heads, the heads, the Pareto layer and the reduction).
Shapes: the reference's actor (hidden 200, heads 2 and 3) at the small_roof widths (16 nodes), 4096 and 14 336 (env, member) pairs
with a Pareto graph of 20 members (the train game) and 4096 pairs with 50 members (the design game).

    python tools/actor_probe.py --precision [OUT_DIR]   -> OUT_DIR/actor_precision.json

times actor_infer(precision=...) instead (one child process): per shape (4096 and 14 336 pairs, P 20), actor path (layers, fused) and
reduced precision T ("bf16x2", "bf16"), medians of 60 synchronised calls in alternating blocks  bf16x3, T, bf16x3 again,  and the
largest deviation of T's action tensors from the bf16x3 ones.

    python tools/actor_probe.py --grouped [OUT_DIR]     -> OUT_DIR/actor_grouped.json

times the THREE-actor call of BatchedMARL._act (without the noise): three actor_infer(fused=True) calls against one
marl.actors_infer call (truss_gcn_layer_group: every depth of the three actors' layers in one launch), two child processes as above.
"grouped_time": medians of 60 synchronised calls in alternating blocks  fused, grouped, fused again,  and whether the outputs are
bitwise equal; "grouped_launches": device kernels per call and their summed device time (torch.profiler), all kernels and the native
ones.  Shapes: the small_roof widths at 512, 4096 and 14 336 pairs with P = 20 and 4096 pairs with P = 50, and the 256-node class at
128 pairs."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mop-truss-marl_amd"))

SHAPES = (          # (label, pairs, P)
    ("small_roof 4096 pairs, P 20", 4096, 20),
    ("small_roof 14336 pairs, P 20", 14336, 20),
    ("small_roof 4096 pairs, P 50", 4096, 50),
)
ROUNDS, BLOCK = 4, 15          # timed calls per path: ROUNDS alternating blocks of BLOCK


GROUP_SHAPES = (    # (label, pairs, P, num_x): what BatchedMARL._act evaluates, three actors on the same inputs
    ("small_roof 512 pairs, P 20", 512, 20, 8),
    ("small_roof 4096 pairs, P 20", 4096, 20, 8),
    ("small_roof 14336 pairs, P 20", 14336, 20, 8),
    ("small_roof 4096 pairs, P 50", 4096, 50, 8),
    ("256 nodes, 128 pairs, P 20", 128, 20, 128),
    # the classes of the mixed sweep (bench_configs.mixed_marl: 1024 / 512 / 256 / 128 envs) at a pass of 4 pairs per env
    ("32 nodes, 4096 pairs, P 20", 4096, 20, 16),
    ("64 nodes, 2048 pairs, P 20", 2048, 20, 32),
    ("128 nodes, 1024 pairs, P 20", 1024, 20, 64),
    ("256 nodes, 512 pairs, P 20", 512, 20, 128),
)


def setup(B, P, dev, num_x=8):
    import numpy as np
    import torch
    import truss_mi355 as tm
    from truss_mi355 import marl
    import truss2D_RL as RL
    torch.manual_seed(B + P)
    topo = tm.TrussTopology.grid(num_x)
    N, tab = topo.N, topo.neighbor_table()
    patt = np.zeros((N, N), bool)
    for i in range(N):
        patt[i, tab[i][tab[i] >= 0]] = True
    patt = torch.tensor(patt, device=dev)
    actor = RL.multimodes_actor(200, 2, 3).to(dev)
    r = lambda *s: torch.rand(*s, device=dev)
    pts = torch.rand(B, P, 4, dtype=torch.float64, device=dev)
    x_p, A_p = marl.pareto_graph(pts, torch.randint(1, P + 1, (B,), device=dev), torch.zeros(B, dtype=torch.long, device=dev), P)
    A_n = torch.tensor(topo.normalized_adjacency()[0], device=dev)
    ins = [r(B, N, 13), A_n, r(B, N, N) * patt, r(B, N, N) * patt, r(B, N, N) * patt, x_p, A_p]
    kw = dict(nbr=torch.tensor(tab, device=dev), nbr_p=torch.tensor(marl.path_graph_table(P), device=dev))
    return actor, ins, kw


def paths(lib, actor, ins, kw):
    import torch
    from truss_mi355 import marl

    def run(fused):
        with torch.no_grad():
            return marl.actor_infer(lib, actor, ins, fused=fused, **kw)
    return {"layers": lambda: run(False), "fused": lambda: run(True)}


def child_time():
    import torch
    import truss_mi355 as tm
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for label, B, P in SHAPES:
        actor, ins, kw = setup(B, P, dev)
        fn = paths(lib, actor, ins, kw)

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
        ts = {"layers": [], "fused": [], "layers_again": []}
        for _ in range(ROUNDS):                                        # alternating blocks: layers, fused, layers, ...
            for k in ts:
                ts[k] += times(fn["fused" if k == "fused" else "layers"], BLOCK)
        res = {"call_us": {k: round(statistics.median(v), 1) for k, v in ts.items()}, "calls_per_median": ROUNDS * BLOCK}
        a, b = fn["layers"](), fn["fused"]()
        res["max_abs_difference"] = max(float((x - y).abs().max()) for x, y in zip(a, b))
        out[label] = res
        del actor, ins, kw, fn, a, b
        torch.cuda.empty_cache()
    print(json.dumps(out))


def child_precision():
    import torch
    import truss_mi355 as tm
    from truss_mi355 import marl
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for label, B, P in SHAPES[:2]:
        actor, ins, kw = setup(B, P, dev)

        def times(f, n):
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            return ts

        for fused in (False, True):
            def run(precision, fused=fused):
                with torch.no_grad():
                    return marl.actor_infer(lib, actor, ins, fused=fused, precision=precision, **kw)
            for p in ("bf16x3", "bf16x2", "bf16"):
                times(lambda: run(p), 10)
            for p in ("bf16x2", "bf16"):
                ts = {"bf16x3": [], p: [], "bf16x3_again": []}
                for _ in range(ROUNDS):
                    for k in ts:
                        ts[k] += times(lambda: run("bf16x3" if k.startswith("bf16x3") else p), BLOCK)
                a, b = run("bf16x3"), run(p)
                out[f"{label} path={'fused' if fused else 'layers'} {p}"] = {
                    "call_us": {k: round(statistics.median(v), 1) for k, v in ts.items()}, "calls_per_median": ROUNDS * BLOCK,
                    "max_abs_deviation_from_bf16x3": max(float((x - y).abs().max()) for x, y in zip(a, b)),
                    "mean_signed_deviation": [float((y - x).double().mean()) for x, y in zip(a, b)]}
        del actor, ins, kw
        torch.cuda.empty_cache()
    print(json.dumps(out))


def child_launches():
    import torch
    from torch.profiler import profile, ProfilerActivity
    import truss_mi355 as tm
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for label, B, P in SHAPES:
        actor, ins, kw = setup(B, P, dev)
        for path, f in paths(lib, actor, ins, kw).items():
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                f()
                torch.cuda.synchronize()
            kern = {}
            for e in prof.key_averages():
                if e.device_type == torch.autograd.DeviceType.CUDA:
                    us = getattr(e, "device_time_total", None)
                    us = e.cuda_time_total if us is None else us
                    c, t = kern.get(e.key, (0, 0.0))
                    kern[e.key] = (c + e.count, t + us)
            # the native launches one by one, in launch order: the fourth is gcn_l1_4 (the Pareto layer), the last four (layers) are
            # gcn_l3_1, gcn_l3_2 and the two heads; fused: the last two are the head launches
            dev_events = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "truss_" in e.name),
                                key=lambda e: e.time_range.start)
            seq = [[e.name.replace("void ", "").split("(")[0], round(e.time_range.end - e.time_range.start, 1)] for e in dev_events]
            out[f"{label} path={path}"] = {
                "launches": sum(c for c, _ in kern.values()), "device_us": round(sum(t for _, t in kern.values()), 1),
                "kernels": {k[:110]: {"count": c, "device_us": round(t, 1)} for k, (c, t) in sorted(kern.items())},
                "native_in_launch_order": seq}
        del actor, ins, kw
        torch.cuda.empty_cache()
    print(json.dumps(out))


def three_actor_paths(lib, B, P, num_x, dev):
    """what BatchedMARL._act does without the noise: the three actors on the same inputs, one after the other through
    actor_infer(fused=True), or level by level through actors_infer"""
    import torch
    from truss_mi355 import marl
    import truss2D_RL as RL
    actor, ins, kw = setup(B, P, dev, num_x)
    actors = [actor] + [RL.multimodes_actor(200, 2, 3).to(dev) for _ in range(2)]

    def fused():
        with torch.no_grad():
            return [marl.actor_infer(lib, a, ins, fused=True, **kw) for a in actors]

    def grouped():
        with torch.no_grad():
            return marl.actors_infer(lib, actors, ins, **kw)
    return {"fused": fused, "grouped": grouped}


def child_grouped_time():
    import torch
    import truss_mi355 as tm
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for label, B, P, num_x in GROUP_SHAPES:
        fn = three_actor_paths(lib, B, P, num_x, dev)

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
            times(f, 10)
        ts = {"fused": [], "grouped": [], "fused_again": []}
        for _ in range(ROUNDS):                                        # alternating blocks: fused, grouped, fused, ...
            for k in ts:
                ts[k] += times(fn["grouped" if k == "grouped" else "fused"], BLOCK)
        a, b = fn["fused"](), fn["grouped"]()
        out[label] = {"call_us": {k: round(statistics.median(v), 1) for k, v in ts.items()}, "calls_per_median": ROUNDS * BLOCK,
                      "outputs_equal": all(bool(torch.equal(x, y)) for p, q in zip(a, b) for x, y in zip(p, q))}
        del fn, a, b
        torch.cuda.empty_cache()
    print(json.dumps(out))


def child_grouped_launches():
    import torch
    from torch.profiler import profile, ProfilerActivity
    import truss_mi355 as tm
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for label, B, P, num_x in GROUP_SHAPES:
        for path, f in three_actor_paths(lib, B, P, num_x, dev).items():
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                f()
                torch.cuda.synchronize()
            kern = {}
            for e in prof.key_averages():
                if e.device_type == torch.autograd.DeviceType.CUDA:
                    us = getattr(e, "device_time_total", None)
                    us = e.cuda_time_total if us is None else us
                    c, t = kern.get(e.key, (0, 0.0))
                    kern[e.key] = (c + e.count, t + us)
            native = lambda k: "truss_" in k
            out[f"{label} path={path}"] = {
                "launches": sum(c for c, _ in kern.values()), "device_us": round(sum(t for _, t in kern.values()), 1),
                "native_launches": sum(c for k, (c, _) in kern.items() if native(k)),
                "native_device_us": round(sum(t for k, (_, t) in kern.items() if native(k)), 1),
                "kernels": {k[:110]: {"count": c, "device_us": round(t, 1)} for k, (c, t) in sorted(kern.items())}}
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    out_dir = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "actor_probe"))
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    env = dict(os.environ, TMPDIR="/tmp")
    result = {}
    precision = "--precision" in sys.argv[1:2]
    grouped = "--grouped" in sys.argv[1:2]
    if precision or grouped:
        out_dir = os.path.abspath(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "build", "actor_probe"))
        os.makedirs(out_dir, exist_ok=True)
    steps = (("precision", "300"),) if precision else (("grouped_time", "300"), ("grouped_launches", "180")) if grouped else \
        (("time", "300"), ("launches", "180"))
    name = "actor_precision.json" if precision else "actor_grouped.json" if grouped else "actor_probe.json"
    for step, limit in steps:
        p = subprocess.run(["timeout", "-k", "10", limit, sys.executable, me, "--child", step], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        with open(os.path.join(out_dir, step + ".err"), "w") as f:
            f.write(p.stderr[-20000:])
        if p.returncode != 0:
            print(f"the {step} step failed with status {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
            sys.exit(1)
        result[step] = json.loads(p.stdout.strip().splitlines()[-1])
        with open(os.path.join(out_dir, name), "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        {"time": child_time, "launches": child_launches, "precision": child_precision, "grouped_time": child_grouped_time,
         "grouped_launches": child_grouped_launches}[sys.argv[2]]()
    else:
        main()
