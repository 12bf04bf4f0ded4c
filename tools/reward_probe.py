"""Diagnostic: reward.difference_reward, path="torch" (three truss_front launches + element-wise torch operators) against
path="hip" (one truss_reward launch), timed in ONE process.

    python tools/reward_probe.py [OUT_DIR]        -> OUT_DIR/reward_probe.json   (default OUT_DIR: build/reward_probe)

The driver starts two child processes, one after the other, each once and under its own `timeout` (no retry; the second only if the
first ended well).  "time" reports the median wall time (host side included) of 60 synchronised calls after warm-up, in
alternating blocks of 15: torch, hip, torch again, ... (the two torch medians give the spread a difference has to exceed), and the
largest absolute difference between the two paths' outputs at the timed sizes.  "launches" counts the device kernels of one call
of each path with torch.profiler (a run of its own: tracing slows the host).
Shapes: K in {512, 4096, 14 336} pairs x (P, max_front) in {(20, 20), (50, 50)}, archives half full (P / 2 mutually non-dominated
rows), pf_hv the same tensor as front_no (what the engine passes), about two thirds of the new points feasible."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mop-truss-marl_amd"))

KS = (512, 4096, 14336)
PS = ((20, 20), (50, 50))
ROUNDS, BLOCK = 4, 15          # timed calls per path: ROUNDS alternating blocks of BLOCK


def setup(K, P, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(K + P)
    n = P // 2
    x = np.sort(rng.uniform(0.05, 0.95, size=(K, n)), axis=1)
    y = np.sort(rng.uniform(0.05, 0.95, size=(K, n)), axis=1)[:, ::-1]
    front = np.zeros((K, P, 4))
    front[:, :n] = np.stack([x, y, np.full_like(x, 0.5), np.full_like(x, 0.5)], axis=2)
    points = rng.uniform(0.05, 1.0, size=(K, 3, 4))
    points[:, :, 2] = rng.uniform(0.4, 1.3, size=(K, 3))              # con1 > 1 for about a third
    t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
    nfr = t(np.full(K, n), torch.int32)
    fr = t(front)
    return (fr, nfr, fr, nfr, t(front[:, n // 2, :2]), t(points), t(rng.uniform(0.9, 1.0, size=(K, 2))), nfr)


def child_time():
    import torch
    import truss_mi355 as tm
    from truss_mi355 import reward as RW
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for P, mf in PS:
        for K in KS:
            args = setup(K, P, dev)
            fn = {p: (lambda p=p: RW.difference_reward(*args, max_front=mf, lib=lib, path=p)) for p in ("torch", "hip")}

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
                for label in ts:
                    ts[label] += times(fn["hip" if label == "hip" else "torch"], BLOCK)
            res = {"call_us": {k: round(statistics.median(v), 1) for k, v in ts.items()}, "calls_per_median": ROUNDS * BLOCK}
            a, b = fn["torch"](), fn["hip"]()
            res["max_abs_difference"] = max(float((u - v).abs().max()) for u, v in zip(a, b))
            out[f"K={K} P={P} max_front={mf}"] = res
            del args, fn
            torch.cuda.empty_cache()
    print(json.dumps(out))


def child_launches():
    import torch
    from torch.profiler import profile, ProfilerActivity
    import truss_mi355 as tm
    from truss_mi355 import reward as RW
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for P, mf in PS:
        args = setup(4096, P, dev)
        for path in ("torch", "hip"):
            f = lambda: RW.difference_reward(*args, max_front=mf, lib=lib, path=path)
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
            out[f"K=4096 P={P} max_front={mf} path={path}"] = {"launches": sum(kern.values()),
                                                               "native": {k[:60]: c for k, c in kern.items() if "truss_" in k}}
    print(json.dumps(out))


def main():
    out_dir = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "reward_probe"))
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
        with open(os.path.join(out_dir, "reward_probe.json"), "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        {"time": child_time, "launches": child_launches}[sys.argv[2]]()
    else:
        main()
