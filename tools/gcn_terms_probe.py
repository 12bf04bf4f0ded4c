#!/usr/bin/env python3
"""Diagnostic: the split-weight GCN layer kernel on three, two and one bf16 terms per operand (marl.gcn_layer, precision "bf16x3" /
"bf16x2" / "bf16"), timed in ONE process.

    python tools/gcn_terms_probe.py [OUT.json]

Per shape and reduced precision T: back-to-back launches in alternating blocks  bf16x3, T, bf16x3  (REPS launches per block between two
events, ROUNDS rounds; the median over the rounds is reported).  The two bf16x3 columns give the spread a difference has to exceed.
Shapes: 98 304 rows of 16-node graphs 200 -> 200 (the hidden layers, KT = 6) and 16 -> 200 (the padded input layers), and a 256-node
shape (NW = 8) 200 -> 200.  Also per shape: max |out_T - out_bf16x3| / max |out_bf16x3| and the mean signed difference (truncation
biases every product towards zero)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mop-truss-marl_amd"), ROOT]
import numpy as np
import torch
import truss_mi355 as tm
from truss_mi355 import marl

lib = tm.load()
dev = "cuda"
ROWS, REPS, ROUNDS = int(os.environ.get("PROBE_ROWS", "98304")), 20, 7


def block(fn):
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record()
    for _ in range(REPS):
        fn()
    a1.record()
    torch.cuda.synchronize()
    return a0.elapsed_time(a1) * 1e3 / REPS


res = []
for nx, K, C in ((8, 200, 200), (8, 16, 200), (128, 200, 200)):
    topo = tm.TrussTopology.grid(nx)
    N, tab = topo.N, topo.neighbor_table()
    B = ROWS // N
    pat = np.zeros((N, N), bool)
    for i in range(N):
        pat[i, tab[i][tab[i] >= 0]] = True
    nbr = torch.tensor(tab, device=dev)
    adj = torch.rand(B, N, N, device=dev) * torch.tensor(pat, device=dev)
    x, w, bias = torch.randn(B, N, K, device=dev), torch.randn(C, K, device=dev) / K ** 0.5, torch.randn(C, device=dev)
    ws = marl.split_weights(lib, w)
    outs = {p: torch.empty(B, N, C, device=dev) for p in ("bf16x3", "bf16x2", "bf16")}
    run = {p: (lambda p=p: marl.gcn_layer(lib, x, adj, w, bias, "relu", nbr, outs[p], precision=p, w_split=ws)) for p in outs}
    for f in run.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    row = {"nodes": N, "graphs": B, "K": K, "C": C, "launches_per_block": REPS, "rounds": ROUNDS}
    for p in ("bf16x2", "bf16"):
        ts = {"bf16x3": [], p: [], "bf16x3_again": []}
        for _ in range(ROUNDS):
            for k in ts:
                ts[k].append(block(run["bf16x3" if k.startswith("bf16x3") else p]))
        row[p] = {"us_per_layer": {k: round(statistics.median(v), 2) for k, v in ts.items()},
                  "min_us": {k: round(min(v), 2) for k, v in ts.items()}}
        d = (outs[p] - outs["bf16x3"]).double()
        row[p]["max_dev_over_max_out"] = float(d.abs().max() / outs["bf16x3"].abs().max())
        row[p]["mean_signed_dev"] = float(d.mean())
        row[p]["mean_out"] = float(outs["bf16x3"].double().mean())
    res.append(row)
    print(json.dumps(row), flush=True)
    del x, adj, outs, run
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
