#!/usr/bin/env python3
"""Diagnostic: the fused level backward (truss_gcn_level_backward) alone -- time per launch (HIP events, back-to-back launches) for
the level shapes of the MADDPG update, next to the forward (truss_gcn_level, with X' stored) and to the library backward of the
same layers as ONE group (truss2D_RL._GcnLevel.backward without a hook: what the update runs by default):
   tools/gcn_level_bwd_probe.py"""
import os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mop-truss-marl_amd"), ROOT]
import torch
import truss_mi355 as tm
from truss_mi355 import ops
import truss2D_RL as RL

lib = tm.load()
dev = "cuda"
r = lambda *s: torch.rand(*s, device=dev)


def timed(call, n=100):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def level(n_layers, B, N, K, C, want_x, tag):
    L = range(n_layers)
    X = [r(B, N, K) - 0.3 for _ in L]
    A = [torch.softmax(torch.randn(B, N, N, device=dev), -1) for _ in L]
    W = [torch.randn(C, K, device=dev) / 14 for _ in L]
    Bs = [r(C) - 0.5 for _ in L]
    O = [torch.empty(B, N, C, device=dev) for _ in L]
    XA = [torch.empty(B * N, K, device=dev) for _ in L]
    D = [r(B, N, C) - 0.5 for _ in L]
    DW, DB = [torch.empty(C, K, device=dev) for _ in L], [torch.empty(C, device=dev) for _ in L]
    DX = [torch.empty(B, N, K, device=dev) for _ in L] if want_x else [None] * n_layers
    act = [1] * n_layers
    ns, idx, st = ops.namespace(), ops.bind(lib), ops.stream_of(torch.device(dev))
    fwd = lambda: ops.call(ns.gcn_level, idx, st, X, A, [], W, Bs, O, XA, act)
    bwd = lambda: ops.call(ns.gcn_level_backward, idx, st, A, W, act, D, O, XA, DW, DB, DX)
    t_f, t_b = timed(fwd), timed(bwd)
    # the library backward of the same layers as one group of equally shaped layers
    g = RL._Group(list(L), "relu", torch.cat(A), A, (B, N, K))
    ctx = types.SimpleNamespace(groups=[g], L=n_layers, saved_tensors=(torch.stack(O), torch.stack(XA), *W),
                                needs_input_grad=(False,) + (want_x,) * n_layers + (True,) * (2 * n_layers))
    dst = torch.stack(D)
    res = [None]

    def lib_bwd():
        res[0] = RL._GcnLevel.backward(ctx, dst)
    t_l = timed(lib_bwd, 50)
    err = max(float((res[0][1 + n_layers + i] - DW[i]).abs().max()) for i in L)
    if want_x:
        err = max(err, max(float((res[0][1 + i] - DX[i]).abs().max()) for i in L))
    print(f"{tag:46s} forward + X' {t_f:7.1f} us   backward {t_b:7.1f} us   library backward {t_l:7.1f} us   max |kernel - library| {err:.1e}")


level(1, 32, 16, 200, 200, True, "1 layer, 512 rows, K 200, C 200")
level(1, 32, 16, 13, 200, False, "1 layer, 512 rows, K 13, C 200 (dW, db only)")
level(11, 32, 16, 200, 200, True, "11 layers (critic level 2)")
level(24, 32, 16, 200, 200, True, "24 layers, 512 rows")
level(24, 96, 16, 200, 200, True, "24 layers, 1536 rows")
level(2, 32, 16, 200, 3, True, "2 heads (C 3)")
