"""Diagnostic: the archive update of a game step as the engine's torch block (candidate buffers, scatters, two concatenations of the
archive, one truss_front launch, gathers, accepted flags) against one truss_archive_merge launch (reward.archive_merge), timed in
ONE process.

    python tools/archive_probe.py [OUT_DIR]        -> OUT_DIR/archive_probe.json   (default OUT_DIR: build/archive_probe)

The driver starts two child processes, one after the other, each once and under its own `timeout` (no retry; the second only if the
first ended well).  "time" reports the median wall time (host side included) of 60 synchronised calls after 10 warm-up calls per
path, in alternating blocks of 15: torch, hip, torch again, ... (the two torch medians give the spread a difference has to exceed),
and whether the two paths' outputs are equal at the timed sizes.  "launches" counts the device kernels of one call of each path with
torch.profiler (a run of its own: tracing slows the host).
Shapes (B envs, P archive rows, C candidate slots, n_y / n_sec words per design): the train game's two chunk shapes at the small_roof
widths (16 nodes / 29 elements), the 256-node class at 512 envs, and the design game's step-wide cull (50, 150), truncated.  Archives
half full (P / 2 mutually non-dominated rows), every slot taken, about two thirds of the candidates ok.  Train shapes: the torch block
fills its candidate buffers through the same table of slots the fused call is handed, and both produce the replay's accepted flags.
Design shape: what BatchedMARL._design_cull does -- the candidates already lie in dense step-wide buffers (slot_row = None), marked,
and nobody asks for flags."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mop-truss-marl_amd"))

SHAPES = (          # (label, B, P, C, n_y, n_sec); "design game": dense candidate buffers
    ("small_roof 512 x (20, 42)", 512, 20, 42, 16, 29),
    ("small_roof 4096 x (20, 42)", 4096, 20, 42, 16, 29),
    ("small_roof 512 x (50, 12)", 512, 50, 12, 16, 29),
    ("small_roof 4096 x (50, 12)", 4096, 50, 12, 16, 29),
    ("256 nodes 512 x (20, 42)", 512, 20, 42, 256, 636),
    ("256 nodes 512 x (50, 12)", 512, 50, 12, 256, 636),
    ("design game 4096 x (50, 150)", 4096, 50, 150, 16, 29),
)
ROUNDS, BLOCK = 4, 15          # timed calls per path: ROUNDS alternating blocks of BLOCK


def setup(B, P, C, n_y, n_sec, dev, dense=False):
    import numpy as np
    import torch
    rng = np.random.default_rng(B + P + C + n_y)
    n = P // 2
    x = np.sort(rng.uniform(0.05, 0.95, size=(B, n)), axis=1)
    y = np.sort(rng.uniform(0.05, 0.95, size=(B, n)), axis=1)[:, ::-1]
    pts = np.zeros((B, P, 4))
    pts[:, :n] = np.stack([x, y, np.full_like(x, 0.5), np.full_like(x, 0.5)], axis=2)
    cand = rng.uniform(0.05, 1.0, size=(B * C, 4))
    cand[:, 2] = rng.uniform(0.4, 1.3, size=B * C)                    # con1 > 1 for about a third
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    slot = rng.permutation(B * C).reshape(B, C)                        # the candidates lie in another order than the slots
    if dense:
        slot = np.arange(B * C).reshape(B, C)
        cand[:, 2] = np.where(cand[:, 2] <= 1, cand[:, 2], 2.0)        # the step-wide buffers hold the marked rows
    return dict(pts=t(pts, torch.float64), n=t(np.full(B, n), torch.int32), y=t(rng.standard_normal((B, P, n_y)), torch.float32),
                sec=t(rng.integers(0, 30, size=(B, P, n_sec)), torch.int32), cand=t(cand, torch.float64),
                cy=t(rng.standard_normal((B * C, n_y)), torch.float32), cs=t(rng.integers(0, 30, size=(B * C, n_sec)), torch.int32),
                slot=t(slot, torch.int32))


def torch_block(RW, lib, t, max_front, dense=False):
    """the archive block of BatchedMARL.game_step_all (marl.py) with its replay flags, on a table of slots; dense: _design_cull"""
    import torch
    wp, wn, wy, ws, slot, points = t["pts"], t["n"], t["y"], t["sec"], t["slot"], t["cand"]
    B, P, _ = wp.shape
    C, dev = slot.shape[1], wp.device
    if dense:
        candP, candY, candS = points.view(B, C, 4), t["cy"].view(B, C, -1), t["cs"].view(B, C, -1)
    else:
        ok = (points[:, 2:4] <= 1).all(dim=1)
        candP = torch.tensor([0.0, 0.0, 2.0, 0.0], dtype=torch.float64, device=dev).expand(B, C, 4).clone()
        candY = torch.zeros((B, C, wy.shape[2]), dtype=torch.float32, device=dev)
        candS = torch.zeros((B, C, ws.shape[2]), dtype=torch.int32, device=dev)
        pmark = points.clone()
        pmark[:, 2] = torch.where(ok, pmark[:, 2], 2.0)
        eb = torch.arange(B, device=dev)[:, None].expand(B, C).reshape(-1)
        ec = torch.arange(C, device=dev)[None, :].expand(B, C).reshape(-1)
        r = slot.reshape(-1).long()
        candP[eb, ec] = pmark[r]
        candY[eb, ec] = t["cy"][r]
        candS[eb, ec] = t["cs"][r]
    origp = torch.cat([wp, candP], dim=1)
    allp = origp.clone()
    dead = torch.arange(P, device=dev)[None, :] >= wn[:, None]
    allp[:, :P, 2] = torch.where(dead, 2.0, allp[:, :P, 2])
    fr = RW.front_hv(allp, torch.full((B,), P + C, dtype=torch.int32, device=dev), None, max_front=max_front, lib=lib)
    fidx = fr["front_idx"][:, :P].long()
    take = fidx.clamp(min=0)
    ally = torch.cat([wy, candY], dim=1)
    alls = torch.cat([ws, candS], dim=1)
    rows = torch.arange(B, device=dev)[:, None]
    live = (fidx >= 0)[:, :, None]
    newp = torch.where(live, origp[rows, take], 0.0)
    newp[:, :, 0:2].clamp_(max=1.0)
    out = dict(points=newp, y=torch.where(live, ally[rows, take], 0.0), sec=torch.where(live, alls[rows, take], 0), n=fr["n_front"].clamp(max=P))
    if not dense:
        infront = torch.zeros((B, P + C), dtype=torch.bool, device=dev)
        infront.scatter_(1, take, live[:, :, 0])
        out["accepted"] = (infront[:, P:] & ok[r].view(B, C)).to(torch.uint8)
    return out


def paths(RW, lib, t, P, dense):
    C = t["slot"].shape[1]
    hip = lambda: RW.archive_merge(t["pts"], t["n"], t["y"], t["sec"], t["cand"], t["cy"], t["cs"], None if dense else t["slot"], n_slots=C,
                                   max_front=P, max_out=P, accepted=not dense, lib=lib)
    return {"torch": lambda: torch_block(RW, lib, t, P, dense), "hip": hip}


def child_time():
    import torch
    import truss_mi355 as tm
    from truss_mi355 import reward as RW
    dev = torch.device("cuda")
    lib = tm.load()
    out = {}
    for label, B, P, C, n_y, n_sec in SHAPES:
        dense = label.startswith("design game")
        t = setup(B, P, C, n_y, n_sec, dev, dense)
        fn = paths(RW, lib, t, P, dense)

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
        a, b = fn["torch"](), fn["hip"]()
        res["outputs_equal"] = all(bool(torch.equal(a[k], b[k])) for k in a)
        out[label] = res
        del t, fn, a, b
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
    for label, B, P, C, n_y, n_sec in SHAPES:
        if B != 4096:
            continue
        dense = label.startswith("design game")
        t = setup(B, P, C, n_y, n_sec, dev, dense)
        for path, f in paths(RW, lib, t, P, dense).items():
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
    out_dir = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "archive_probe"))
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
        with open(os.path.join(out_dir, "archive_probe.json"), "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        {"time": child_time, "launches": child_launches}[sys.argv[2]]()
    else:
        main()
