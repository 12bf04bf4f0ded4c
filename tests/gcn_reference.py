"""Float64 references of the GCN kernels (truss_gcn_layer / _level / _aggregate / _aggregate_sparse) and host models of their
arithmetic, for the test suite.

Every kernel result is checked element by element against the float64 value of the same operation with a bound proportional
to the elementwise magnitude of the sum that produced it:

    |got - ref64| <= tau * Mag,     Mag = |A| (|X| |W|^T) + |b|  (+ |out0| when accumulating)

A float32 evaluation in any summation order stays within a small multiple of 2^-24 * Mag; an arithmetic mistake of the kernels
(a partial product of the bf16x3 split dropped, a K slab skipped, a neighbourhood term lost) does not.  To prove that a tau can
tell them apart, the tests evaluate host MUTANTS of the layer on the same inputs and require each of them to violate the bound.
"""
from __future__ import annotations

import numpy as np
import torch


def f64(t):
    """tensor / array -> float64 numpy array (on the host)"""
    if t is None:
        return None
    if torch.is_tensor(t):
        t = t.detach().cpu()
        return t.double().numpy()
    return np.asarray(t, np.float64)


def act64(z, act):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    return z


def dense_adj(adj, B, N):
    """adjacency [N, N] (shared) or [B, N, N] -> float64 [B, N, N]"""
    a = f64(adj)
    return np.broadcast_to(a, (B, N, N)) if a.ndim == 2 else a


def layer_ref(x, adj, w, bias, act, out0=None):
    """float64 act(A (X W^T) + b) (+ out0) and its magnitude |A| (|X| |W|^T) + |b| (+ |out0|).  x [B, N, K]; adj [N, N] or [B, N, N];
    w [C, K]; bias [C] or None; out0 [B, N, C] (the output before an accumulating call) or None."""
    X, W = f64(x), f64(w)
    B, N, _ = X.shape
    A = dense_adj(adj, B, N)
    b = f64(bias) if bias is not None else np.zeros(W.shape[0])
    ref = act64(A @ (X @ W.T) + b, act)
    mag = np.abs(A) @ (np.abs(X) @ np.abs(W).T) + np.abs(b)
    if out0 is not None:
        o = f64(out0)
        ref, mag = ref + o, mag + np.abs(o)
    return ref, mag


def agg_ref(adj, h, bias, act):
    """float64 act(A H + b) and |A| |H| + |b| (the aggregation kernels)"""
    H = f64(h)
    B, N, _ = H.shape
    A = dense_adj(adj, B, N)
    b = f64(bias) if bias is not None else 0.0
    return act64(A @ H + b, act), np.abs(A) @ np.abs(H) + np.abs(b)


def max_ratio(got, ref, mag):
    """max |got - ref| / Mag over the elements with Mag > 0 (an element with Mag == 0 must be exact: reported as inf otherwise)"""
    err = np.abs(f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def within(got, ref, mag, tau, abs_tol=0.0):
    """boolean: |got - ref| <= tau * Mag (+ abs_tol) everywhere"""
    return bool(np.all(np.abs(f64(got) - ref) <= tau * mag + abs_tol))


# ---- the bf16x3 arithmetic on the host ----

def split3(a):
    """float32 array -> its three bfloat16 terms (as float32 arrays) by truncation, like truss_gcn_split_w / tg_split_term:
    t0 = upper half of a, t1 = upper half of a - t0, t2 = upper half of a - t0 - t1 (both differences exact)."""
    a = np.ascontiguousarray(a, np.float32)
    top = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    t0 = top(a)
    r1 = a - t0
    t1 = top(r1)
    t2 = top(r1 - t1)
    return t0, t1, t2


def _aggregate32(x, adj):
    """X' = A X as the kernels hold it: float32 (here: rounded once from float64), [B, N, K]"""
    X = f64(x)
    B, N, _ = X.shape
    return (dense_adj(adj, B, N) @ X).astype(np.float32)


def bf16x3_pre(x, adj, w, products=("00", "01", "10", "02", "11", "20")):
    """A (X W^T) through the split: X' = A X in float32, both operands split in three terms, the listed partial products
    ("ij" = x_i w_j) summed in float64.  All six: the kernel's arithmetic (up to its float32 accumulation)."""
    xs = split3(_aggregate32(x, adj))
    ws = split3(f64(w).astype(np.float32))
    out = 0.0
    for p in products:
        out = out + xs[int(p[0])].astype(np.float64) @ ws[int(p[1])].astype(np.float64).T
    return out


def mutants(x, adj, w, bias, act, out0=None):
    """{name: float64 output} of broken variants of the layer on these inputs: the bf16x3 products with one product missing
    (a2 b0) or only the first-order ones, the exact layer with its last K slab of 16 left out, and with the diagonal term of the
    aggregation (each node's own row) left out."""
    X, W = f64(x), f64(w)
    B, N, K = X.shape
    A = dense_adj(adj, B, N)
    b = f64(bias) if bias is not None else np.zeros(W.shape[0])
    fin = lambda pre: act64(pre + b, act) + (f64(out0) if out0 is not None else 0.0)
    s0 = (K - 1) // 16 * 16
    Wd = W.copy()
    Wd[:, s0:] = 0.0
    An = A.copy()
    idx = np.arange(N)
    An[:, idx, idx] = 0.0
    return {
        "six products minus a2*b0": fin(bf16x3_pre(x, adj, w, ("00", "01", "10", "02", "11"))),
        "first-order products only": fin(bf16x3_pre(x, adj, w, ("00", "01", "10"))),
        "last K slab left out": fin(A @ (X @ Wd.T)),
        "diagonal term left out": fin(An @ (X @ W.T)),
    }


def bf16x3_model(x, adj, w, bias, act, out0=None):
    """the correct bf16x3 arithmetic on the host (six products): must satisfy the same bound as the kernel"""
    b = f64(bias) if bias is not None else 0.0
    return act64(bf16x3_pre(x, adj, w) + b, act) + (f64(out0) if out0 is not None else 0.0)


# tau per kernel path for the bound |got - ref64| <= tau * Mag (the measured values are in the docstrings of tests/test_gcn_float64.py)
TAU = {
    "bf16x3": 1e-6,     # truss_gcn_layer, product on the bf16 matrix cores (six partial products of split operands)
    "f32": 1e-6,        # truss_gcn_layer, float32 matrix cores
    "level": 1e-6,      # truss_gcn_level (float32 matrix cores), outputs and X' = A X
    "agg": 1.5e-6,      # truss_gcn_aggregate / truss_gcn_aggregate_sparse
}
