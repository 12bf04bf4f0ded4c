#!/usr/bin/env python3
"""Diagnostic: the MADDPG update of the large size classes with the node-graph adjacencies applied as dense N x N products
(BatchedMARL(level_adjacency="dense"), the default) and through the node table ("table": truss_gcn_level_aggregate), in ONE process:
per class nx (2 nx nodes) blocks dense / table / dense, each a fresh engine on the same agents and the same batch (batch 32, the
project's network widths), and per block
    the time per update, eager and as the replayed hipGraph: median of `reps` synchronised updates after warm-up, host side included;
    torch.cuda.max_memory_allocated over the block;
    kernel launches per eager update (torch.profiler);
then the aggregation kernel alone on the shapes of the critics' second level (11 layers, [32, N, 200], per-sample adjacencies), both
directions, next to its byte roof: x read once + y written once at the rate of a plain fill.
    tools/level_adjacency_probe.py [nx ...] [--reps 30] [--fill-tbs 6.3]      one JSON line per block, then one per kernel shape"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mop-truss-marl_amd"), ROOT]
import numpy as np
import torch
import truss_mi355 as tm
from truss_mi355 import marl, ops
import bench_configs

dev = "cuda"


def table_batch(topo, B, P, seed):
    """a minibatch (S, NS, A, R) in the engine's layout: A_n and the mask shared (stride 0), the sampled adjacencies row-stochastic on
    the truss's table and zero outside it"""
    N, g = topo.N, torch.Generator().manual_seed(seed)
    table = topo.neighbor_table()
    on = np.zeros((N, N), bool)
    r_, c_ = np.nonzero(table >= 0)
    on[r_, table[r_, c_]] = True
    off = ~torch.from_numpy(on)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    A = lambda: torch.softmax(torch.randn(B, N, N, generator=g).masked_fill(off, float("-inf")), -1).to(dev)
    A_p = lambda: torch.softmax(torch.randn(B, P, P, generator=g), -1).to(dev)
    a_n, mask = A()[:1].expand(B, -1, -1), torch.ones(1, N, N).to(dev).expand(B, -1, -1)
    state = lambda: [r(B, N, 13), a_n, A(), A(), A(), mask, r(B, P, 4), A_p()]
    return state(), [state() for _ in range(3)], [(r(B, N, 2), r(B, N, 3)) for _ in range(3)], r(B, 3)


def median_ms(call, reps, warm=5):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def launches(call):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def block(topo, rl, batch, adjacency, reps, P):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with contextlib.redirect_stdout(io.StringIO()):
        eng = marl.BatchedMARL(topo, 8, rl, max_front=P, device=dev, replay_capacity=64, batch_size=len(batch[3]), level_adjacency=adjacency)
        eng.use_train_graph = False
        eager = median_ms(lambda: eng._train(*batch), reps)
        n_launch = launches(lambda: eng._train(*batch))
        eng.use_train_graph = True
        eng._train(*batch)                                            # warm-up updates + capture
        captured = eng._tg is not None
        graph = median_ms(lambda: eng._train(*batch), reps) if captured else (float("nan"),) * 3
    out = dict(nodes=topo.N, level_adjacency=adjacency, eager_ms=dict(zip(("median", "min", "max"), eager)),
               graph_ms=dict(zip(("median", "min", "max"), graph)), captured=captured, launches_per_eager_update=n_launch,
               peak_allocated_mb=(torch.cuda.max_memory_allocated() - base) / 2 ** 20, reps=reps)
    del eng
    return out


def kernel_alone(topo, fill_tbs, B=32, C=200, n=11):
    table = topo.neighbor_table()
    N, nbr = topo.N, torch.from_numpy(table).to(dev)
    X = [torch.rand(B, N, C, device=dev) for _ in range(n)]
    A = [torch.rand(B, N, N, device=dev) for _ in range(n)]
    Y = [torch.empty(B, N, C, device=dev) for _ in range(n)]
    lib = tm.load()
    ns, idx, st = ops.namespace(), ops.bind(lib), ops.stream_of(torch.device(dev))
    out = []
    for transpose in (False, True):
        call = lambda: ops.call(ns.gcn_level_aggregate, idx, st, X, A, [nbr] * n, Y, [transpose] * n)
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 100
        nbytes = 2 * n * B * N * C * 4
        out.append(dict(kernel="truss_gcn_level_aggregate", nodes=N, items=n, n_ch=C, k_nbr=int(table.shape[1]), transpose=transpose,
                        us_per_launch=us, x_plus_y_mb=nbytes / 2 ** 20, byte_roof_us=nbytes / (fill_tbs * 1e12) * 1e6,
                        fraction_of_roof=nbytes / (fill_tbs * 1e12) * 1e6 / us))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("nx", nargs="*", type=int, default=[32, 64, 128])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fill-tbs", type=float, default=6.3, help="rate of a plain fill of such a footprint on this chip, TB/s (DESIGN.md 4.1b)")
    a = ap.parse_args()
    P = 20
    for nx in a.nx:
        topo = tm.TrussTopology.grid(nx)
        rl = bench_configs._maddpg(dev)
        batch = table_batch(topo, 32, P, 7)
        rl._ensure_ready(batch[0], [t for pair in batch[2] for t in pair])
        for adjacency in ("dense", "table", "dense"):
            print(json.dumps(block(topo, rl, batch, adjacency, a.reps, P)), flush=True)
        for row in kernel_alone(topo, a.fill_tbs):
            print(json.dumps(row), flush=True)
