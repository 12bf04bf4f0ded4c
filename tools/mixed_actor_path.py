"""Diagnostic: the mixed Pareto sweep without training (bench_configs.mixed_marl: `mixed_pool_marl_no_training`) under two settings of
BatchedMARL's actor_path, selected through the environment (TRUSS_ACTOR), one child process per run, in the order A, B, A, B, A: the
runs of one setting give the spread a difference has to exceed (it is large: the archives grow over the run, so the caching
allocator keeps asking the driver for new segments inside the timed steps; every run reports its allocator counters).

    python tools/mixed_actor_path.py [OUT_DIR] [A] [B]     -> OUT_DIR/mixed_actor_path.json   (defaults: build/mixed_actor_path fused grouped)

Every child runs once, under its own `timeout`; a child that fails ends the tool."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 30          # timed game steps per run (the bench config times 3: too few to tell the settings apart)


def child():
    sys.path[:0] = [os.path.join(ROOT, "mop-truss-marl_amd"), ROOT]
    import contextlib
    import io
    import bench_configs as BC
    with contextlib.redirect_stdout(io.StringIO()):
        r = BC.mixed_marl(train=False, steps=STEPS)
    import torch
    ms = torch.cuda.memory_stats()
    out = {k: r[k] for k in ("envs_per_class", "game_steps", "env_steps", "seconds", "env_steps_per_s")}
    # the caching allocator over the whole run: segments it had to ask the driver for, cache flushes after a failed request, peak
    out["allocator"] = {"device_allocs": ms.get("num_device_alloc"), "device_frees": ms.get("num_device_free"), "alloc_retries": ms.get("num_alloc_retries"),
                        "peak_reserved_GB": round(ms.get("reserved_bytes.all.peak", 0) / 2 ** 30, 2),
                        "peak_allocated_GB": round(ms.get("allocated_bytes.all.peak", 0) / 2 ** 30, 2)}
    print(json.dumps(out))


def main():
    out_dir = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "mixed_actor_path"))
    a, b = (sys.argv[2], sys.argv[3]) if len(sys.argv) > 3 else ("fused", "grouped")
    os.makedirs(out_dir, exist_ok=True)
    runs = []
    for path in (a, b, a, b, a):
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT,
                           env=dict(os.environ, TRUSS_ACTOR=path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"the run with TRUSS_ACTOR={path} failed with status {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
            sys.exit(1)
        runs.append(dict(actor_path=path, **json.loads(p.stdout.strip().splitlines()[-1])))
        with open(os.path.join(out_dir, "mixed_actor_path.json"), "w") as f:
            json.dump(runs, f, indent=1)
    print(json.dumps(runs, indent=1))


if __name__ == "__main__":
    child() if "--child" in sys.argv[1:] else main()
