"""Diagnostic: DeviceReplay.add / .sample, dense storage (framework indexing) against compact storage (the fused replay_scatter /
replay_gather launches), timed in ONE process.

    python tools/replay_probe.py [OUT_DIR]        -> OUT_DIR/replay_probe.json   (default OUT_DIR: build/replay_probe)

The driver starts one child process, once and under its own `timeout` (no retry).  It reports the median wall time (host side
included) of 60 synchronised calls after warm-up, in alternating blocks of 15: dense, compact, dense again, ... (the two dense medians
give the spread a difference has to exceed), `nbytes` of both storages, and whether both return the same batch from the same
generator state at these sizes.  Kernel launches per call (a rocprofv3 kernel trace) are not collected yet.
Shapes: small_roof (N 16, P 20, K = 12 288 candidate rows of which about a third are accepted, capacity 32 768) and the 256-node class
of the mixed sweep (N 256, P 20, K = 512, capacity 4096; batch 32 in both)."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mop-truss-marl_amd"))

SHAPES = {"small_roof": dict(num_x=8, P=20, K=12288, capacity=32768, accept=1 / 3),
          "mixed_256_nodes": dict(num_x=128, P=20, K=512, capacity=4096, accept=1 / 3)}
BATCH = 32
ROUNDS, BLOCK = 4, 15          # timed calls per storage: ROUNDS alternating blocks of BLOCK


def setup(shape, dev):
    import numpy as np
    import torch
    import truss_mi355 as tm
    from truss_mi355 import marl
    s = SHAPES[shape]
    topo = tm.TrussTopology.grid(s["num_x"])
    N, P, K = topo.N, s["P"], s["K"]
    nbr, nbr_p = topo.neighbor_table(), marl.path_graph_table(P)
    g = torch.Generator().manual_seed(1)

    def mask(t):
        m = np.zeros((t.shape[0], t.shape[0]), bool)
        r, c = np.nonzero(t >= 0)
        m[r, t[r, c]] = True
        return torch.from_numpy(m).to(dev)

    mn, mp = mask(nbr), mask(nbr_p)
    shapes = dict(x_n=(N, 13), A_s=(N, N), A_n_ts=(N, N), A_n_cs=(N, N), x_p=(P, 4), A_p=(P, P))

    def rows(*lead):
        out = {}
        for k, sh in shapes.items():
            t = torch.rand(*lead, *sh, device=dev)
            if k in marl.DeviceReplay.PATTERN_KEYS:
                t = t * (mp if k == "A_p" else mn)
            out[k] = t
        return out

    S, NS = rows(K), rows(3, K)
    src = torch.randint(0, 3, (K, 3), generator=g).to(dev)
    sel = (torch.rand(K, generator=g) < s["accept"]).to(dev)
    ag = torch.rand(3, K, N, 2, device=dev).permute(1, 0, 2, 3)          # agent-major, permuted views: as the engine hands them over
    at = torch.rand(3, K, N, 3, device=dev).permute(1, 0, 2, 3)
    R = torch.rand(K, 3, device=dev)
    lib = tm.load()
    reps = {"dense": marl.DeviceReplay(s["capacity"], N, P, dev),
            "compact": marl.DeviceReplay(s["capacity"], N, P, dev, storage="compact", nbr=nbr, nbr_p=nbr_p, lib=lib)}
    assert reps["compact"]._lib is not None, "the native library has no replay entries"
    gen = torch.Generator(device=dev).manual_seed(2)
    add = lambda r: r.add(sel, S, NS, ag, at, R, src=src)
    sample = lambda r: r.sample(BATCH, gen)
    return lib, reps, add, sample, int(sel.sum())


def child_time():
    import torch
    dev = torch.device("cuda")
    out = {}
    for shape in SHAPES:
        lib, reps, add, sample, k = setup(shape, dev)

        def times(fn, r, n):
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(r)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            return ts

        res = {"rows_per_add": k, "batch": BATCH, "nbytes": {n: r.nbytes for n, r in reps.items()}}
        for name, fn in (("add", add), ("sample", sample)):
            for r in reps.values():
                times(fn, r, 10)                                            # warm-up of every shape the timed calls use
            ts = {"dense": [], "compact": [], "dense_again": []}
            for _ in range(ROUNDS):                                        # alternating blocks: dense, compact, dense, ...
                for label in ts:
                    ts[label] += times(fn, reps["compact" if label == "compact" else "dense"], BLOCK)
            res[name + "_us"] = {k: round(statistics.median(v), 1) for k, v in ts.items()}
            res[name + "_us"]["calls_per_median"] = ROUNDS * BLOCK
        # the two storages hold the same transitions (from the same ring position: the timed loops left different ones)
        for r in reps.values():
            r.size = r.head = 0
            add(r)
        g1, g2 = (torch.Generator(device=dev).manual_seed(5) for _ in range(2))
        A, B = reps["dense"].sample(BATCH, g1), reps["compact"].sample(BATCH, g2)
        res["same_batches"] = all(torch.equal(A[0][key], B[0][key]) and all(torch.equal(A[1][i][key], B[1][i][key]) for i in range(3))
                                  for key in A[0]) and all(torch.equal(A[j], B[j]) for j in (2, 3, 4))
        out[shape] = res
        del reps
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    out_dir = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "replay_probe"))
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    env = dict(os.environ, TMPDIR="/tmp")
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "--child", "time"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    with open(os.path.join(out_dir, "time.err"), "w") as f:
        f.write(p.stderr[-20000:])
    if p.returncode != 0:
        print(f"the timing step failed with status {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
        sys.exit(1)
    result = json.loads(p.stdout.strip().splitlines()[-1])
    with open(os.path.join(out_dir, "replay_probe.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        {"time": child_time}[sys.argv[2]]()
    else:
        main()
