"""Diagnostic: two builds of the library side by side in one process, alternating rounds -- `truss_front` and the aggregation
kernels of a parent build against the build under test (profiles/r6/README.md).

    python tools/front_agg_ab.py PARENT_LIB [OUT_JSON]      # PARENT_LIB: e.g. csrc/abl/libtruss_parent.so, built from the parent commit

front_hv at 4096 envs (64 and 200 rows, max_front 50, truncation on): device events around windows of >= 0.5 s of back-to-back calls.
Aggregation: tools/agg_probe.py as it is, run in this process once per round and library.  Outputs of the two builds are compared
too (front_idx / n_front equal, metrics and hypervolumes within 1e-12, aggregation bitwise).  Pass criterion per shape:
median(new) <= median(parent) + (max - min of the parent's rounds)."""
import contextlib, io, json, os, runpy, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mop-truss-marl_amd"), ROOT]
import numpy as np
import torch
import truss_mi355 as tm
from truss_mi355 import _lib, ops, reward as RW

PARENT = os.path.abspath(sys.argv[1])
OUT = sys.argv[2] if len(sys.argv) > 2 else "front_agg_ab.json"
NEW = _lib.DEFAULT_LIB
ROUNDS = int(os.environ.get("AB_ROUNDS", "7"))
WINDOW = float(os.environ.get("AB_WINDOW", "0.7"))
B = int(os.environ.get("AB_ENVS", "4096"))
SIZES = (1, 63, 64, 65, 129, 200, 256)
dev = torch.device("cuda", 0)
res = {"rounds": ROUNDS, "window_s": WINDOW, "envs": B, "device": torch.cuda.get_device_name(0)}


def log(*a):
    print(*a, flush=True)


def sets(seed, P, B):
    """the four kinds of tests/test_front_wide.py::_sets, sizes cycling through SIZES clipped to P, B envs"""
    rng = np.random.default_rng(seed)
    sizes = [min(SIZES[(b // 4) % len(SIZES)], P) for b in range(B)]
    pts = np.zeros((B, P, 4))
    for b, s in enumerate(sizes):
        kind = b % 4
        p = rng.uniform(0.05, 1.15, size=(P, 4))
        p[:, 2:] = rng.uniform(0.2, 1.06, size=(P, 2))
        if kind >= 2:
            t = rng.uniform(0.0, 1.15, size=P)
            p[:, 0], p[:, 1] = t, np.clip(1.1 - t + rng.normal(0.0, 0.01, size=P), 0.0, None)
        if kind in (1, 3):
            p[:, :2] = np.round(p[:, :2] * 40) / 40
            k = max(1, s // 8)
            src, dst = rng.integers(0, max(1, s // 2), size=k), rng.integers(s // 2, s, size=k) if s > 1 else [0]
            p[dst] = p[src]
        p[0, 2:] = 0.5
        pts[b] = p
    return pts, np.array(sizes, np.int32), rng.uniform(0.85, 1.0, size=(B, 2))


def window(fn, n):
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a0.record()
    for _ in range(n):
        fn()
    a1.record()
    torch.cuda.synchronize()
    return a0.elapsed_time(a1) * 1e-3, a0.elapsed_time(a1) * 1e3 / n      # window seconds, us per call


def verdict(par, new):
    mp, mn, spread = statistics.median(par), statistics.median(new), max(par) - min(par)
    return dict(parent_us=par, new_us=new, parent_median=mp, new_median=mn, parent_spread=spread, ok=bool(mn <= mp + spread))


libs = {"parent": tm.load(PARENT), "new": tm.load(NEW)}
assert all(l.backend == "hip" for l in libs.values())

# ---- front ----
res["front"] = {}
for P in (64, 200):
    pts, n, ref = sets(11, P, B)
    tp, tn, tr = torch.tensor(pts, device=dev), torch.tensor(n, device=dev), torch.tensor(ref, device=dev)
    outs = {k: {kk: v.cpu().numpy() for kk, v in RW.front_hv(tp, tn, tr, max_front=50, lib=l).items()} for k, l in libs.items()}
    a, b = outs["parent"], outs["new"]
    same = dict(front_idx=bool(np.array_equal(a["front_idx"], b["front_idx"])), n_front=bool(np.array_equal(a["n_front"], b["n_front"])),
                **{k: float(np.abs(a[k] - b[k]).max()) for k in ("metrics", "hv_front", "hv_all")})
    same["ok"] = same["front_idx"] and same["n_front"] and max(same["metrics"], same["hv_front"], same["hv_all"]) <= 1e-12
    same["n_front_max"], same["cut"] = int(a["n_front"].max()), int((a["n_front"] == 50).sum())
    log("front outputs", P, same)
    pre = dict(front_idx=torch.empty((B, P), dtype=torch.int32, device=dev), n_front=torch.empty((B,), dtype=torch.int32, device=dev),
               hv_front=torch.empty((B,), dtype=torch.float64, device=dev), hv_all=torch.empty((B,), dtype=torch.float64, device=dev),
               metrics=torch.empty((B, 5), dtype=torch.float64, device=dev))
    ns, st = ops.namespace(), ops.stream_of(dev)
    calls = {}
    for k, l in libs.items():
        h = ops.bind(l)
        calls[k] = {
            "front_hv": (lambda l=l: RW.front_hv(tp, tn, tr, max_front=50, lib=l)),
            "op_only": (lambda h=h: ops.call(ns.front, h, st, 50, _lib.F_FRONT_TRUNCATE, tp, tn, tr, pre["front_idx"], pre["n_front"],
                                             pre["hv_front"], pre["hv_all"], pre["metrics"])),
        }
    entry = {"outputs": same}
    for how in ("front_hv", "op_only"):
        ncall = {}
        for k in libs:                                   # warm-up and window size
            window(calls[k][how], 50)
            _, us = window(calls[k][how], 200)
            ncall[k] = int(WINDOW / (us * 1e-6)) + 1
        n_calls = max(ncall.values())
        t, wmin = {"parent": [], "new": []}, 1e9
        for r in range(ROUNDS):
            for k in ("parent", "new"):
                sec, us = window(calls[k][how], n_calls)
                wmin = min(wmin, sec)
                t[k].append(round(us, 2))
        entry[how] = dict(calls_per_window=n_calls, shortest_window_s=round(wmin, 3), **verdict(t["parent"], t["new"]))
        log("front", P, how, json.dumps(entry[how]))
    res["front"][P] = entry

# ---- aggregation: outputs bitwise on the probe's shapes ----
agg_same = {}
torch.manual_seed(3)
for N, Bn in ((16, 10000), (20, 9000), (24, 6000), (32, 4096), (48, 2048), (64, 1024), (128, 512), (256, 256)):
    C = 224
    h, bias = torch.rand(Bn, N, C, device=dev), torch.rand(C, device=dev)
    for tag, adj in (("shared", torch.softmax(torch.randn(N, N, device=dev), -1)), ("per_graph", torch.softmax(torch.randn(Bn, N, N, device=dev), -1))):
        o = {}
        if N <= 64:
            for k, l in libs.items():
                o[k] = torch.empty_like(h)
                ops.call(ops.namespace().gcn_aggregate, ops.bind(l), ops.stream_of(dev), adj.contiguous(), h, bias, o[k], 1)
            agg_same[f"N{N}_{tag}_dense"] = bool(torch.equal(o["parent"], o["new"]))
        if N % 4 == 0:
            nbr = torch.tensor(tm.TrussTopology.grid(N // 2).neighbor_table(), device=dev)
            for act in (0, 2):
                for k, l in libs.items():
                    o[k] = torch.empty_like(h)
                    ops.call(ops.namespace().gcn_aggregate_sparse, ops.bind(l), ops.stream_of(dev), adj.contiguous(), nbr, h, bias, o[k], act)
                agg_same[f"N{N}_{tag}_sparse_act{act}"] = bool(torch.equal(o["parent"], o["new"]))
# the dense kernels the probe's shapes do not reach (channel-quad and thread-per-channel kernels), every activation
for N, C, Bn in ((12, 20, 120), (8, 8, 70), (16, 224, 4096), (16, 6, 3), (9, 262, 2), (40, 6, 3), (32, 6, 5)):
    h, bias = torch.randn(Bn, N, C, device=dev), torch.randn(C, device=dev)
    adj = torch.softmax(torch.randn(Bn, N, N, device=dev), -1)
    for act in (0, 1, 2):
        o = {}
        for k, l in libs.items():
            o[k] = torch.empty_like(h)
            ops.call(ops.namespace().gcn_aggregate, ops.bind(l), ops.stream_of(dev), adj, h, bias, o[k], act)
        agg_same[f"N{N}_C{C}_B{Bn}_dense_act{act}"] = bool(torch.equal(o["parent"], o["new"]))
res["agg_outputs_bitwise"] = agg_same
res["agg_outputs_ok"] = all(agg_same.values())
log("agg outputs bitwise equal:", res["agg_outputs_ok"], {k: v for k, v in agg_same.items() if not v})

# ---- aggregation: tools/agg_probe.py as it is, per round and library ----
probe = os.path.join(ROOT, "tools", "agg_probe.py")
runs = {"parent": [], "new": []}
for r in range(ROUNDS):
    for k, path in (("parent", PARENT), ("new", NEW)):
        _lib.DEFAULT_LIB = path
        buf = io.StringIO()
        t0 = time.time()
        with contextlib.redirect_stdout(buf):
            runpy.run_path(probe, run_name="__main__")
        runs[k].append(json.loads(buf.getvalue().strip().splitlines()[-1]))
        log("agg_probe round", r, k, f"{time.time() - t0:.1f} s")
_lib.DEFAULT_LIB = NEW
res["agg"] = {}
for key in runs["parent"][0]:
    for f in ("fused_us", "sparse_us"):
        if f in runs["parent"][0][key]:
            res["agg"][f"{key}:{f}"] = verdict([x[key][f] for x in runs["parent"]], [x[key][f] for x in runs["new"]])
for k, v in res["agg"].items():
    log("agg", k, json.dumps(v))
res["all_ok"] = bool(all(v["ok"] for v in res["agg"].values()) and res["agg_outputs_ok"] and
                     all(e["outputs"]["ok"] and e["front_hv"]["ok"] and e["op_only"]["ok"] for e in res["front"].values()))
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
log("ALL OK" if res["all_ok"] else "SOME CHECK MISSED", "->", OUT)
