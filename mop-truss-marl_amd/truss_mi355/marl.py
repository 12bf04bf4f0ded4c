"""Batched multi-agent rollout + training loop (BASELINE configs 3-5: thousands of envs with the MADDPG
agents in the loop).  The reference's `run()` (master_DDPG_truss2D_MO.py:164-705) plays ONE truss: per game
step it lets the three agents modify every member of the Pareto archive, scores the moves with the
hypervolume-difference reward, culls the archive and trains.  Here the same game step runs for B trusses at
once, every piece on the device:

    parents' analysis + observation   BatchedTruss.analyze / observe     (truss_step, truss_obs kernels)
    three agents' actions             truss2D_RL actors on a [B, N, .] batch (rocBLAS)
    the 3 B candidate designs         one truss_step launch over 3 B envs (+ truss_obs for the next states)
    rewards                           reward.difference_reward            (truss_front kernel; reward_path="hip": truss_reward)
    archive update                    reward.front_hv + gathers
    replay + MADDPG update            device tensors, MADDPG.train_on_batch

One game step is ONE flat pass over all live (env, archive member) pairs (member-major list, in chunks of at most
`pair_capacity` pairs): one parent analysis, one actor pass per agent, one candidate launch, one reward evaluation for
all of them -- not one pass per member index, whose later, thin iterations were bound by launch overhead.

Differences from the per-env loop, all forced by batching and documented here:
  D1  the archive is culled once per chunk of pairs -- for an archive of up to 14 members (MAX_FRONT 20: the front
      kernel takes 64 rows = 20 archive rows + the 3 x 14 candidates of 14 members) that is once per game step, like the
      reference (:430); larger archives are folded in two rounds (the Pareto front of a union is the front of the
      partial fronts, so the set is the same unless the MAX_FRONT truncation intervenes); rewards use the front at
      the START of the game step, like the reference (front_no / Pf_HV, :263-368);
  D2  a transition enters the replay when its candidate is in the archive after that cull (the reference remembers the
      candidates that survive the end-of-step cull, :595-621);
  D3  truncation to MAX_FRONT is deterministic (largest crowding distance), see include/truss_mi355.h;
  D4  when an agent's move is infeasible its next state in the replay is the first feasible agent's
      (the reference draws a random survivor, :380-407); the Pareto-graph inputs (x_p, A_p) of the next
      states are those of the step-start front;
  D5  exploration noise is drawn on the device (same law as truss2D_RL.OUNoise: theta (mu - a) dt + sigma N(0,1));
  D6  (design game) the symmetry coin of each move is the top bit of a splitmix64 hash of (engine seed, global env id, game
      step, member index in the step-start archive, agent) -- `design_coins` -- instead of the reference's random.random()
      >= 0.5 per _game_modify call (test/*/truss2D_ENV.py:459-553): the same Bernoulli(0.5) law, reproducible by a host
      model and independent of `pair_capacity` and of the chunk order.

The design game (`game="test"`, the reference's test copies test/0?_*/code): trained agents modify mirror-symmetric
designs with a coin per move, the archive keeps up to MAX_FRONT = 50 members, nothing is trained (train_period = 0) and
the last step culls the archive plus all of that step's candidates WITHOUT truncation (simple_cull_final, master…:424-428).
Every chunk's candidates are collected into step-wide buffers (slot = 3 member + agent) and the step ends with ONE cull over
the P archive rows + 3 P candidates (the wide front kernel takes up to 256 rows): D1 does not apply to this game.
`design_episode` plays a whole episode.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import _lib
from . import reward as RW
from .batched import BatchedTruss
from .topology import TrussTopology


_TUNE_UPDATE_GEMMS = False


def enable_gemm_tuning(max_ms_per_shape: int = 30, filename: str | None = None):
    """Let PyTorch's TunableOp choose the library GEMM for the shapes of the MADDPG UPDATE (fixed: batch 32), timed once
    during the eager warm-up updates that precede the hipGraph capture (BatchedMARL._train).  The weight gradients of the
    GCN layers (200 x 200 outputs, K = 32 x 16 = 512) otherwise get a single 256 x 224 tile from the library's heuristic:
    118 us each, half of an update.  The inference GEMMs are left alone: their row count (live (env, member) pairs x nodes)
    changes every game step and every new shape would be tuned again (11 s for four game steps when tried).
    No-op on the CPU backend."""
    global _TUNE_UPDATE_GEMMS
    if not torch.cuda.is_available():
        return False
    t = torch.cuda.tunable
    t.enable(True)                 # use tuned solutions where a shape has one
    t.tuning_enable(False)         # ... but time new shapes only inside the update's warm-up
    t.set_max_tuning_duration(int(max_ms_per_shape))
    t.set_max_tuning_iterations(20)
    filename = filename or os.environ.get("TRUSS_GEMM_TUNE_FILE")   # keep / reuse the choices (a profiled run reads them: no tuning)
    if filename:
        t.set_filename(filename)
        if hasattr(t, "write_file_on_exit"):
            t.write_file_on_exit(True)
    elif hasattr(t, "write_file_on_exit"):
        t.write_file_on_exit(False)    # no tunableop_results*.csv in the caller's working directory
    _TUNE_UPDATE_GEMMS = True
    return True


def pareto_graph(pts, n, index, max_front):
    """Batched truss2D_ENV.pareto_state_data (:19-38) + zero padding to P nodes (master…:488-593).
    pts [B,P,4] (rows beyond n ignored), n [B], index [B] -> x_p [B,P,4], A_p [B,P,P] float32."""
    B, P, _ = pts.shape
    dev = pts.device
    ar = torch.arange(P, device=dev)
    vf = (ar[None, :] < n[:, None]).float()                                             # [B, P] 1 on the front's members
    x = torch.stack([pts[:, :, 0].float(), pts[:, :, 1].float(), (ar[None, :] == index[:, None]).float(),
                     (n.float() / max_front)[:, None].expand(B, P)], dim=2) * vf[:, :, None]
    # a path over the members with self loops, symmetrically normalised: deg_i = 1 + (left neighbour) + (right neighbour) on members
    z = torch.zeros((B, 1), dtype=torch.float32, device=dev)
    deg = vf * (1.0 + torch.cat([z, vf[:, :-1]], dim=1) + torch.cat([vf[:, 1:], z], dim=1))
    d = torch.where(deg > 0, deg.pow(-0.5), 0.0)
    return x, _tridiagonal(P, dev) * d[:, :, None] * d[:, None, :]


_TRI: dict = {}


def _tridiagonal(P, dev):
    """[P, P] ones on the three central diagonals (the path graph with self loops), cached per size and device"""
    key = (P, str(dev))
    if key not in _TRI:
        i = torch.arange(P, device=dev)
        _TRI[key] = ((i[:, None] - i[None, :]).abs() <= 1).float()
    return _TRI[key]


def gcn_aggregate(lib, adj, h, bias, act, nbr=None):
    """act(adj @ h + bias) through the fused HIP kernels `truss_gcn_aggregate` / `truss_gcn_aggregate_sparse` (inference only, float32).
    adj [N,N] (shared) or [B,N,N]; h [B,N,C] contiguous; act in {None,'relu','sigmoid'}.
    nbr: int16 [N,K] device table of the columns that can be non-zero in each row of `adj` (TrussTopology.neighbor_table());
    with it, graphs above 32 nodes sum over those K columns only (tools/agg_probe.py: 64 nodes 39 us against 74 us for the
    library's batched GEMM + bias + activation, 256 nodes 42 against 104; at 32 nodes the dense channel-quad kernel is as fast, at 16 faster)."""
    B, N, Cc = h.shape
    from . import ops
    code = {None: 0, "relu": 1, "sigmoid": 2}[act]
    if nbr is not None and N > 32 and Cc % 4 == 0 and nbr.shape[1] <= 16:
        adj = adj.contiguous()
        if adj.dim() == 3 and adj.shape[0] == 1:
            adj = adj[0]
        out = torch.empty_like(h)
        ops.call(ops.namespace().gcn_aggregate_sparse, ops.bind(lib), ops.stream_of(h.device), adj, nbr, h, bias, out, code)
        return out
    if N > 64:     # larger graphs without a pattern: a batched N x N x C GEMM (rocBLAS); the fused dense kernels cover N <= 64
        out = torch.matmul(adj, h) + bias
        return torch.relu(out) if act == "relu" else torch.sigmoid(out) if act == "sigmoid" else out
    adj = adj.contiguous()
    if adj.dim() == 3 and adj.shape[0] == 1:
        adj = adj[0]
    out = torch.empty_like(h)
    ops.call(ops.namespace().gcn_aggregate, ops.bind(lib), ops.stream_of(h.device), adj, h, bias, out, code)
    return out


def split_weights(lib, w, out=None):
    """w [C <= 224, K] float32 -> int16 [3, 224, KP] (bfloat16 bit patterns, zero padded): the exact three-term split the bf16x3 path
    of the fused layer kernel reads (`truss_gcn_split_w`; one small launch).  `layer_split_weights` caches it per GCN layer.
    out: an existing image of that shape to write (in place: capturable, its address stays)."""
    from . import ops
    C, K = w.shape
    if out is None:
        out = torch.empty((3, 224, (K + 15) // 16 * 16), dtype=torch.int16, device=w.device)
    assert out.shape == (3, 224, (K + 15) // 16 * 16) and out.dtype == torch.int16 and out.is_contiguous()
    ops.call(ops.namespace().gcn_split_w, ops.bind(lib), ops.stream_of(w.device), w, out)
    return out


def _refresh_split(lib, layer, hit):
    """rewrite a cache entry of `layer_split_weights` from the layer's current weights, in place (same buffers)"""
    w = layer.lin.weight.detach()
    _, wd, ws = hit
    if wd.data_ptr() != w.data_ptr():                    # the zero-padded copy (its pad columns stay zero)
        wd[:, :w.shape[1]].copy_(w)
    if ws is not None:
        split_weights(lib, wd, out=ws)


def layer_split_weights(lib, layer, k_pad=0):
    """(w, split_weights(w)) of a truss2D_RL.GCNConv, kept on the module and redone when its kernel has changed (training updates the
    weights in place: tensor version counter; load_state_dict / re-materialisation: data pointer).  k_pad > k_in: the kernel's input
    columns are zero-padded to k_pad first (the 13-feature input layers run at 16 so that they take the 16-byte loaders).
    A version change rewrites the entry IN PLACE: a captured update (BatchedMARL._train) refreshes the same buffers on every replay
    (`refresh_actor_caches`) -- a replay changes the weights without bumping their version counters."""
    w = layer.lin.weight
    tag = (w._version, w.data_ptr(), tuple(w.shape), k_pad)
    hit = getattr(layer, "_truss_split", None)
    if hit is not None and hit[0][1:] == tag[1:]:
        if hit[0][0] != tag[0]:
            _refresh_split(lib, layer, hit)
            hit = (tag,) + hit[1:]
            layer._truss_split = hit
        return hit[1], hit[2]
    wd = w.detach()
    if k_pad > wd.shape[1]:
        wd = torch.nn.functional.pad(wd, (0, k_pad - wd.shape[1])).contiguous()
    hit = (tag, wd, split_weights(lib, wd) if (wd.shape[0] > 32 and wd.shape[1] % 4 == 0) else None)
    layer._truss_split = hit
    return hit[1], hit[2]


def refresh_actor_caches(lib, actor):
    """rewrite every cached weight copy of `actor`'s layers (split images, zero-padded inputs) from its current weights, in
    place: the tail of the captured MADDPG update, so that inference after a replay sees the weights the replay wrote"""
    for layer in actor.modules():
        hit = getattr(layer, "_truss_split", None)
        if hit is not None:
            _refresh_split(lib, layer, hit)


PRECISIONS = ("f32", "bf16x3", "bf16x2", "bf16")
_BF16_TERMS = {"bf16x3": 3, "bf16x2": 2, "bf16": 1}         # bf16 terms per operand of the split-weight product


def _check_precision(precision, what="precision"):
    if precision not in PRECISIONS:
        raise ValueError(f"{what} must be one of {', '.join(repr(p) for p in PRECISIONS)}, got {precision!r}")
    return precision


def _bf16_envelope(x, w, nbr):
    """the split-weight kernel takes this layer (tb_gcn_bf16x3_check); every other layer runs on the float32 matrix cores under
    every precision"""
    return w.shape[0] > 32 and x.shape[2] % 4 == 0 and x.data_ptr() % 16 == 0 and (nbr.shape[1] if nbr is not None else x.shape[1]) <= 9


def gcn_layer(lib, x, adj, w, bias, act, nbr=None, out=None, accumulate=False, precision="bf16x3", w_split=None):
    """One whole GCN layer through the hand-written MFMA kernel (`truss_gcn_layer`, csrc/truss_gcn.h):
    out = act(adj @ (x @ w.T) + bias), or out += ... with `accumulate`; float32 in and out, inference (no autograd).
    x [B,N,K] contiguous; adj [N,N] (shared) or [B,N,N]; w [C,K] = nn.Linear.weight, C <= 224; nbr: int16 [N,Kn] sparsity pattern of
    adj (TrussTopology.neighbor_table(), Kn <= 16) or None for a dense adjacency of at most 64 nodes; N <= 256.
    precision "bf16x3" (default): where the shape allows (the hidden layers: C > 32, K % 4 == 0, <= 9 terms per row) the product runs
    on the bf16 matrix cores as six partial products of exactly split operands with float32 accumulation -- float32 accuracy, 2.7 x
    fewer matrix-core cycles; "f32": always the float32 matrix cores.  "bf16x2" / "bf16": the same kernel on the first two terms /
    the first term of both operands (`truss_gcn_layer_terms`; three products / one product): reduced precision for inference,
    |out - ref64| <= (2^-13 + 1e-6) Mag / (2^-6 + 1e-6) Mag with Mag = |A| (|X| |W|^T) + |b| (+ |out0|), operands truncated (every
    product biased towards zero); a layer outside that envelope runs in float32 as under every precision.
    w_split: split_weights(lib, w) if the caller keeps it (one image serves all precisions)."""
    from . import ops
    _check_precision(precision)
    B, N, K = x.shape
    C = w.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty((B, N, C), dtype=torch.float32, device=x.device)
    adj = adj.contiguous()
    if adj.dim() == 3 and adj.shape[0] == 1:
        adj = adj[0]
    code = {None: 0, "relu": 1, "sigmoid": 2}[act]
    ws = None
    if precision != "f32" and _bf16_envelope(x, w, nbr):
        ws = w_split if w_split is not None else split_weights(lib, w)
    if ws is not None and precision != "bf16x3":
        ops.call(ops.namespace().gcn_layer_terms, ops.bind(lib), ops.stream_of(x.device), x, adj, nbr, w, bias, out, code, ws, 0,
                 None, None, None, None, 0, None, None, bool(accumulate), _BF16_TERMS[precision])
        return out
    ops.call(ops.namespace().gcn_layer, ops.bind(lib), ops.stream_of(x.device), x, adj, nbr, w, bias, out, code, bool(accumulate), ws)
    return out


def _gcn_layer_fused(lib, x, adj, w, bias, act, nbr, precision, w_split, out, kind, w2=None, bias2=None, adj2=None, nbr2=None, act2=None,
                     out2=None, pool=None):
    """`truss_gcn_layer_fused`: the layer of `gcn_layer` with a consumer of its output in the epilogue of the same launch
    (precision "bf16x2" / "bf16", inside the split-weight envelope: `truss_gcn_layer_terms` with the same epilogue)"""
    from . import ops
    _check_precision(precision)
    flat = lambda a: a[0] if a.dim() == 3 and a.shape[0] == 1 else a
    adj = flat(adj.contiguous())
    code = {None: 0, "relu": 1, "sigmoid": 2}
    ws = None
    if precision != "f32" and _bf16_envelope(x, w, nbr):
        ws = w_split if w_split is not None else split_weights(lib, w)
    if adj2 is not None:
        adj2 = flat(adj2.contiguous())
    if ws is not None and precision != "bf16x3":
        ops.call(ops.namespace().gcn_layer_terms, ops.bind(lib), ops.stream_of(x.device), x, adj, nbr, w, bias, out, code[act], ws, kind,
                 w2, bias2, adj2, nbr2, code[act2], out2, pool, False, _BF16_TERMS[precision])
        return
    ops.call(ops.namespace().gcn_layer_fused, ops.bind(lib), ops.stream_of(x.device), x, adj, nbr, w, bias, out, code[act], ws, kind,
             w2, bias2, adj2, nbr2, code[act2], out2, pool)


def gcn_layer_head(lib, x, adj, w, bias, act, w2, bias2, adj2, act2, nbr=None, nbr2=None, precision="bf16x3", w_split=None, out=None):
    """A hidden GCN layer and the narrow layer that consumes it in ONE launch (`truss_gcn_layer_fused`, head epilogue):
    act2(adj2 @ (V @ w2.T) + bias2) [B, N, c2] with V = act(adj @ (x @ w.T) + bias) as `gcn_layer` computes it -- V goes from the
    accumulators through LDS into the head and is written to HBM only if `out` [B, N, C] is given.  w2 [c2 <= 8, C] =
    nn.Linear.weight of the head; adj2 / nbr2: the head's own adjacency and pattern (as adj / nbr); the rest as for `gcn_layer`."""
    out2 = torch.empty((x.shape[0], x.shape[1], w2.shape[0]), dtype=torch.float32, device=x.device)
    _gcn_layer_fused(lib, x, adj, w, bias, act, nbr, precision, w_split, out, 1, w2, bias2, adj2, nbr2, act2, out2=out2)
    return out2


def gcn_layer_pool(lib, x, adj, w, bias, act, nbr=None, precision="bf16x3", w_split=None, out=None):
    """A GCN layer and the sum of its output over the nodes of every graph in ONE launch (`truss_gcn_layer_fused`, pool epilogue):
    act(adj @ (x @ w.T) + bias).sum(dim=1) [B, C], every one of the N rows counted; the layer's output itself is written to HBM
    only if `out` [B, N, C] is given.  Arguments as for `gcn_layer`."""
    pool = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
    _gcn_layer_fused(lib, x, adj, w, bias, act, nbr, precision, w_split, out, 2, pool=pool)
    return pool


def level_forward(lib):
    """The fused forward of a whole level of GCN layers (`truss_gcn_level`, csrc/truss_gcn_level.h: one launch for every layer of
    every group) in the shape truss2D_RL._GcnLevel asks for: callable(groups, xs, ws, bs, want_grad) -> ([out_g [n, B, N, C]],
    [X'_g [n, B N, K] or None]), or None when a shape is outside the kernel's envelope (the caller then evaluates the level with
    batched library GEMMs).  Installed by BatchedMARL on the GPU (`truss2D_RL.set_level_forward`)."""
    from . import ops
    code = {None: 0, "relu": 1, "sigmoid": 2}

    def run(groups, xs, ws, bs, want_grad):
        X, ADJ, W, BIAS, OUT, XAGG, ACT, outs, xaggs = [], [], [], [], [], [], [], [], []
        for g in groups:
            n, (B, N, K), C = len(g.idx), g.shape, ws[g.idx[0]].shape[0]
            if N > 64 or C > 224 or K > 256 or xs[g.idx[0]].dtype != torch.float32:      # outside the kernel's envelope
                return None
            o = torch.empty((n, B, N, C), dtype=torch.float32, device=xs[g.idx[0]].device)
            xa = torch.empty((n, B * N, K), dtype=torch.float32, device=o.device) if want_grad else None
            for j, i in enumerate(g.idx):
                a = g.adjs[j]
                if a.dim() == 3 and (a.shape[0] == 1 or a.stride(0) == 0):
                    a = a[0]
                X.append(xs[i].detach().contiguous())
                ADJ.append(a.contiguous())
                W.append(ws[i].detach())
                BIAS.append(bs[i].detach())
                OUT.append(o[j])
                if want_grad:
                    XAGG.append(xa[j])
                ACT.append(code[g.act])
            outs.append(o)
            xaggs.append(xa)
        ops.call(ops.namespace().gcn_level, ops.bind(lib), ops.stream_of(X[0].device), X, ADJ, [], W, BIAS, OUT, XAGG, ACT)
        return outs, xaggs
    return run


def level_backward(lib):
    """The fused backward of a whole level of GCN layers (`truss_gcn_level_backward`, csrc/truss_gcn_level_bwd.h: one launch for
    every layer of every group that something flows back into) in the shape truss2D_RL._GcnLevel.backward asks for:
    callable(groups, douts, outs, xaggs, ws, need) -> (dx, dw, db), lists in request order whose entries are the `unbind` pieces of
    one stacked tensor per group and quantity ([n, B, N, K], [n, C, K], [n, C]), or None when a group is outside the kernel's
    envelope (the caller then runs the level's backward as batched library GEMMs).  Installed by
    BatchedMARL(level_backward="hip") on the GPU (`truss2D_RL.set_level_backward`)."""
    from . import ops
    code = {None: 0, "relu": 1, "sigmoid": 2}

    def run(groups, douts, outs, xaggs, ws, need):
        L = len(ws)
        todo = []
        for gi, g in enumerate(groups):
            need_w = any(need[1 + L + i] or need[1 + 2 * L + i] for i in g.idx)
            need_x = any(need[1 + i] for i in g.idx)
            if douts[gi] is None or not (need_w or need_x):
                continue                                                             # no slices in the launch
            (B, N, K), C = g.shape, outs[gi].shape[-1]
            if N > 64 or C > 224 or K > 256 or outs[gi].dtype != torch.float32 or douts[gi].dtype != torch.float32 \
                    or (need_w and xaggs[gi] is None):                              # outside the kernel's envelope
                return None
            todo.append((gi, g, need_w, need_x))
        dx, dw, db = [None] * L, [None] * L, [None] * L
        if not todo:
            return dx, dw, db
        ADJ, W, ACT, DOUT, OUT, XAGG, DW, DB, DX = [], [], [], [], [], [], [], [], []
        for gi, g, need_w, need_x in todo:
            n, (B, N, K), C = len(g.idx), g.shape, outs[gi].shape[-1]
            dev = outs[gi].device
            d = douts[gi].contiguous()
            gw = torch.empty((n, C, K), dtype=torch.float32, device=dev) if need_w else None
            gb = torch.empty((n, C), dtype=torch.float32, device=dev) if need_w else None
            gx = torch.empty((n, B, N, K), dtype=torch.float32, device=dev) if need_x else None
            for j, i in enumerate(g.idx):
                a = g.adjs[j]
                if a.dim() == 3 and (a.shape[0] == 1 or a.stride(0) == 0):
                    a = a[0]
                ADJ.append(a.contiguous())
                W.append(ws[i].detach())
                ACT.append(code[g.act])
                DOUT.append(d[j])
                OUT.append(outs[gi][j])
                XAGG.append(xaggs[gi][j] if need_w else None)
                DW.append(gw[j] if need_w else None)
                DB.append(gb[j] if need_w else None)
                DX.append(gx[j] if need_x else None)
            if need_w:
                for i, pw, pb in zip(g.idx, gw.unbind(0), gb.unbind(0)):
                    dw[i], db[i] = pw, pb
            if need_x:
                for i, piece in zip(g.idx, gx.unbind(0)):
                    dx[i] = piece                          # (one tensor passed for several layers: autograd adds per argument)
        ops.call(ops.namespace().gcn_level_backward, ops.bind(lib), ops.stream_of(OUT[0].device), ADJ, W, ACT, DOUT, OUT, XAGG, DW, DB, DX)
        return dx, dw, db
    return run


_level_backward_hook = level_backward        # (BatchedMARL's argument of the same name shadows the function)


def gcn_layer_supported(n_nodes, c_out, nbr):
    """shapes the fused layer kernel takes (include/truss_mi355.h); anything else goes through library GEMM + aggregation kernels"""
    return c_out <= 224 and n_nodes <= 256 and ((nbr is not None and nbr.shape[1] <= 16) or (nbr is None and n_nodes <= 64))


def path_graph_table(n_nodes):
    """int16 [P, 3] neighbour table of the Pareto graph: `pareto_graph` / truss2D_ENV.pareto_state_data build a PATH over the front's
    members (self loops + consecutive members), so row i of A_p is zero outside columns i - 1, i, i + 1"""
    t = np.full((n_nodes, 3), -1, np.int16)
    for i in range(n_nodes):
        t[i, 0] = i - 1 if i > 0 else -1
        t[i, 1] = i
        t[i, 2] = i + 1 if i + 1 < n_nodes else -1
    return t


def actor_infer(lib, actor, ins, nbr=None, nbr_p=None, fused=False, precision="bf16x3"):
    """truss2D_RL.multimodes_actor.forward (truss2D_RL.py:49-120) for inference, every GCN layer ONE launch of the fused MFMA
    kernel (`gcn_layer`: neighbourhood sum on the input rows, product with W^T on the matrix cores, bias + activation in the
    epilogue; H = X W never exists in HBM); the five second-level layers accumulate their sum x3 in place.  Same values as the
    module up to float32 summation order ((A X) W instead of A (X W)).
    nbr: the truss's neighbour table on the device (TrussTopology.neighbor_table()) for the layers over the node graph; nbr_p: the
    same for the Pareto graph (path_graph_table(P) when A_p comes from `pareto_graph`; None = dense, at most 64 members).  Shapes outside the kernel's envelope (a node graph without pattern above 64 nodes)
    fall back to library GEMM + `gcn_aggregate`.
    fused: the three activations that inference writes only to read them back once stay on chip (`truss_gcn_layer_fused`, 11 launches
    instead of 13): gcn_l1_4 is summed over the Pareto graph in its own epilogue (`gcn_layer_pool`), and the action heads gcn_l4_1 /
    gcn_l4_2 run in the epilogues of gcn_l3_1 / gcn_l3_2 (`gcn_layer_head`; they read lin.weight as it is).  Same values up to float32
    summation order; a layer outside the kernel's envelope takes the unfused path.
    precision: handed to every layer (`gcn_layer`): "bf16x3" (default, float32 accuracy), "f32", or the reduced "bf16x2" / "bf16"
    for the hidden layers -- the action heads and every other layer outside the split-weight envelope stay float32.  The cached
    split weights (`layer_split_weights`) are the same for all of them."""
    _check_precision(precision)
    x_n, A_n, A_s, A_ts, A_cs, x_p, A_p = ins
    materialise, g, g_pool, g_head = _actor_layer_calls(lib, A_p, nbr, nbr_p, fused, precision)
    a = actor
    if x_n.shape[2] % 4 and gcn_layer_supported(x_n.shape[1], 200, nbr):
        # 13 node features -> 16 (zero columns, matched by zero columns of the three input kernels): 16-byte loads, bf16x3 product
        for layer in (a.gcn_l1_1, a.gcn_l1_2, a.gcn_l1_3):
            materialise(layer, x_n, A_n)
        x_n = torch.nn.functional.pad(x_n, (0, 4 - x_n.shape[2] % 4))
    x11, x12, x13 = g(a.gcn_l1_1, x_n, A_n), g(a.gcn_l1_2, x_n, A_n), g(a.gcn_l1_3, x_n, A_n)
    x14 = g_pool(a.gcn_l1_4, x_p, A_p)                                                   # GlobalSumPool over the Pareto graph
    B, H = x14.shape
    x14 = x14.unsqueeze(-1).expand(B, H, x11.shape[1]).reshape(B, x11.shape[1], H)      # _tile_pool (:87-93)
    x3 = g(a.gcn_l2_1, x11, A_n)
    g(a.gcn_l2_2, x12, A_ts, out=x3, accumulate=True)
    g(a.gcn_l2_3, x12, A_cs, out=x3, accumulate=True)
    g(a.gcn_l2_4, x13, A_s, out=x3, accumulate=True)
    g(a.gcn_l2_5, x14.contiguous(), A_n, out=x3, accumulate=True)
    if not fused:
        x31, x32 = g(a.gcn_l3_1, x3, A_n), g(a.gcn_l3_2, x3, A_s)
        return g(a.gcn_l4_1, x31, A_n, "sigmoid"), g(a.gcn_l4_2, x32, A_n, "sigmoid")
    materialise(a.gcn_l3_1, x3, A_n), materialise(a.gcn_l3_2, x3, A_s)                  # (lazy layers: in the order of the unfused path)
    return g_head(a.gcn_l3_1, a.gcn_l4_1, x3, A_n, A_n), g_head(a.gcn_l3_2, a.gcn_l4_2, x3, A_s, A_n)


def _actor_layer_calls(lib, A_p, nbr, nbr_p, fused, precision):
    """the per-layer calls of `actor_infer` (and of the levels `actors_infer` does not group): (materialise, g, g_pool, g_head)"""

    def materialise(layer, x, a):                           # lazy layers: let the module materialise itself once
        if isinstance(layer.lin.weight, torch.nn.parameter.UninitializedParameter):
            with torch.no_grad():
                layer(x[:1], a[:1] if a.dim() == 3 else a)

    def g(layer, x, a, act="relu", out=None, accumulate=False):
        materialise(layer, x, a)
        w, bvec = layer.lin.weight, layer.bias
        pat = nbr_p if a is A_p else nbr
        x = x.contiguous()
        if gcn_layer_supported(x.shape[1], w.shape[0], pat):
            wd, ws = layer_split_weights(lib, layer, x.shape[2])     # (x_n arrives zero-padded to 16 features)
            return gcn_layer(lib, x, a, wd, bvec.detach(), act, pat, out, accumulate, precision=precision, w_split=ws)
        h = gcn_aggregate(lib, a, torch.nn.functional.linear(x, w).contiguous(), bvec, act, pat)
        if out is None:
            return h
        return out.add_(h) if accumulate else out.copy_(h)

    def g_pool(layer, x, a):                                # g(layer, x, a).sum(dim=1) without the [B, P, H] tensor
        materialise(layer, x, a)
        pat = nbr_p if a is A_p else nbr
        x = x.contiguous()
        if not (fused and gcn_layer_supported(x.shape[1], layer.lin.weight.shape[0], pat)):
            return g(layer, x, a).sum(dim=1)
        wd, ws = layer_split_weights(lib, layer, x.shape[2])
        return gcn_layer_pool(lib, x, a, wd, layer.bias.detach(), "relu", pat, precision=precision, w_split=ws)

    def g_head(layer, head, x, a, a2):                      # g(head, g(layer, x, a), a2, "sigmoid") without the hidden tensor
        materialise(layer, x, a)
        if isinstance(head.lin.weight, torch.nn.parameter.UninitializedParameter):
            materialise(head, x.new_zeros((1, x.shape[1], layer.lin.weight.shape[0])), a2)
        pat, pat2 = nbr_p if a is A_p else nbr, nbr_p if a2 is A_p else nbr
        x = x.contiguous()
        w2 = head.lin.weight
        if not (w2.shape[0] <= 8 and gcn_layer_supported(x.shape[1], layer.lin.weight.shape[0], pat)
                and gcn_layer_supported(x.shape[1], w2.shape[0], pat2)):
            return g(head, g(layer, x, a), a2, "sigmoid")
        wd, ws = layer_split_weights(lib, layer, x.shape[2])
        return gcn_layer_head(lib, x, a, wd, layer.bias.detach(), "relu", w2.detach(), head.bias.detach(), a2, "sigmoid", pat, pat2,
                              precision=precision, w_split=ws)

    return materialise, g, g_pool, g_head


_ACT_CODE = {None: 0, "relu": 1, "sigmoid": 2}
GROUP_MAX_STEPS, GROUP_MAX_EPI = 16, 8                      # TRUSS_GCN_GROUP_MAX_STEPS / _EPI (include/truss_mi355.h)


def gcn_layer_group(lib, chains, precision="bf16x3", epilogues=None):
    """Several split-weight GCN layers in ONE launch (`truss_gcn_layer_group`, csrc/truss_gcn_group.h): the same bits as running them
    one by one through `gcn_layer` / `gcn_layer_head` / `gcn_layer_pool` in chain order.
    chains: a list of chains of equal length; a chain is a list of steps that write the same `out`, a step a dict with the arguments of
    `gcn_layer` by name: x, adj, w, bias, act, out, w_split (required: `split_weights(lib, w)`), and optionally nbr, accumulate.
    Chains must not depend on each other; a step must not read the chain's `out`.  All layers share B, N and table-or-dense.
    epilogues: None, or one dict per chain (chains of one step; out may then be None): kind "head" with w2, bias2, adj2, act2, out2
    and optionally nbr2, or kind "pool" with pool -- all of one kind.
    precision: "bf16x3", "bf16x2" or "bf16" (this entry is the split-weight path only: no "f32", and a layer outside the
    split-weight envelope is refused by the library, not rerouted).  At most 16 plain layers, or 8 chains with epilogues."""
    from . import ops
    _check_precision(precision)
    if precision == "f32":
        raise ValueError("gcn_layer_group is the split-weight path: precision must be 'bf16x3', 'bf16x2' or 'bf16'")
    flat = lambda a: None if a is None else (lambda c: c[0] if c.dim() == 3 and c.shape[0] == 1 else c)(a.contiguous())
    steps = [s for chain in chains for s in chain]
    per_chain = len(chains[0]) if chains else 1
    assert all(len(chain) == per_chain for chain in chains) and (epilogues is None or len(epilogues) == len(chains))
    col = lambda key, default=None: [s.get(key, default) for s in steps]
    kind, epi = 0, [[] for _ in range(7)]
    if epilogues is not None:
        kinds = {e["kind"] for e in epilogues}
        assert len(kinds) <= 1 and kinds <= {"head", "pool"}, "epilogues of one kind, 'head' or 'pool'"
        kind = 1 if kinds == {"head"} else 2
        ecol = lambda key: [e.get(key) for e in epilogues]
        epi = [ecol("w2"), ecol("bias2"), [flat(a) for a in ecol("adj2")], ecol("nbr2"), [_ACT_CODE[e.get("act2")] for e in epilogues],
               ecol("out2"), ecol("pool")]
    device = steps[0]["x"].device if steps else torch.device("cpu")
    ops.call(ops.namespace().gcn_layer_group, ops.bind(lib), ops.stream_of(device), col("x"), [flat(a) for a in col("adj")], col("nbr"),
             col("w"), col("bias"), col("out"), [_ACT_CODE[s["act"]] for s in steps], [bool(s.get("accumulate", False)) for s in steps],
             col("w_split"), per_chain, kind, *epi, _BF16_TERMS[precision])


def actors_infer(lib, actors, ins, nbr=None, nbr_p=None, precision="bf16x3"):
    """`actor_infer(fused=True)` for EVERY actor of `actors` on the same inputs, level by level: [(geo_a, topo_a) for a in actors],
    bit for bit what the per-actor calls return.  The actors read the same observation tensors and their layers have the same
    shapes; within an actor the layers of one depth do not depend on each other.  So each depth is one launch of
    `truss_gcn_layer_group` for all actors -- the 3 A input layers; the A Pareto layers with the pool epilogue into one [A, B, H]
    buffer, tiled by one copy; A chains of the five second-level layers, which accumulate x3 in place; the 2 A layers that feed
    the heads, with the head epilogue -- four launches and three framework kernels (the pad of x_n, the tiling copy, and
    contiguous() where an input needs it) instead of 11 A launches and 3 A framework kernels.
    A level with a layer outside the split-weight envelope (precision "f32", a node graph without a table or with more than nine
    terms per row, a head wider than 8, a library without the entry) runs through the per-layer calls of `actor_infer`; only
    that level does.  Lazy layers are materialised actor by actor in the order of the unfused path; the cached weight images are
    those of `layer_split_weights`."""
    _check_precision(precision)
    x_n, A_n, A_s, A_ts, A_cs, x_p, A_p = ins
    materialise, g, g_pool, g_head = _actor_layer_calls(lib, A_p, nbr, nbr_p, True, precision)
    A, N = len(actors), x_n.shape[1]
    if A == 0:
        return []
    for a in actors:                                        # lazy layers, in the order consecutive actor_infer calls materialise them
        for layer in (a.gcn_l1_1, a.gcn_l1_2, a.gcn_l1_3):
            materialise(layer, x_n, A_n)
        materialise(a.gcn_l1_4, x_p, A_p)
        lazy = lambda layer: isinstance(layer.lin.weight, torch.nn.parameter.UninitializedParameter)
        for layer, src, adj in ((a.gcn_l2_1, a.gcn_l1_1, A_n), (a.gcn_l2_2, a.gcn_l1_2, A_ts), (a.gcn_l2_3, a.gcn_l1_2, A_cs),
                                (a.gcn_l2_4, a.gcn_l1_3, A_s), (a.gcn_l2_5, a.gcn_l1_4, A_n), (a.gcn_l3_1, a.gcn_l2_1, A_n),
                                (a.gcn_l3_2, a.gcn_l2_1, A_s), (a.gcn_l4_1, a.gcn_l3_1, A_n), (a.gcn_l4_2, a.gcn_l3_2, A_n)):
            if lazy(layer):                                 # (the layer's input matters by its width only)
                materialise(layer, x_n.new_zeros((1, N, src.lin.weight.shape[0])), adj)
    if x_n.shape[2] % 4 and gcn_layer_supported(N, 200, nbr):
        x_n = torch.nn.functional.pad(x_n, (0, 4 - x_n.shape[2] % 4))          # once for all actors
    x_n, x_p = x_n.contiguous(), x_p.contiguous()
    can_group = lib.has_gcn_group and precision != "f32"

    def step(layer, x, adj, pat, out=None, accumulate=False):
        """the layer as a step of `gcn_layer_group`, or None outside the envelope of the grouped launch"""
        if not gcn_layer_supported(x.shape[1], layer.lin.weight.shape[0], pat):
            return None
        wd, ws = layer_split_weights(lib, layer, x.shape[2])
        if ws is None or not _bf16_envelope(x, wd, pat):
            return None
        return dict(x=x, adj=adj, nbr=pat, w=wd, bias=layer.bias.detach(), act="relu", out=out, accumulate=accumulate, w_split=ws)

    def launch(chains, epilogues, limit):
        """one launch, or one per `limit` chains where the actors are many"""
        for i in range(0, len(chains), limit):
            gcn_layer_group(lib, chains[i:i + limit], precision, None if epilogues is None else epilogues[i:i + limit])

    def outputs(n, shape):
        return list(torch.empty((n,) + tuple(shape), dtype=torch.float32, device=x_n.device).unbind(0))

    B = x_n.shape[0]
    # depth 1, node graph: gcn_l1_1 .. gcn_l1_3 of every actor
    firsts = [(a.gcn_l1_1, a.gcn_l1_2, a.gcn_l1_3) for a in actors]
    steps = [step(layer, x_n, A_n, nbr) for trio in firsts for layer in trio] if can_group else [None]
    widths = {s["w"].shape[0] for s in steps if s is not None}
    if all(s is not None for s in steps) and len(widths) == 1:
        for s, o in zip(steps, outputs(len(steps), (B, N, widths.pop()))):
            s["out"] = o
        launch([[s] for s in steps], None, GROUP_MAX_STEPS)
        x1 = [[steps[3 * i + j]["out"] for j in range(3)] for i in range(A)]
    else:
        x1 = [[g(layer, x_n, A_n) for layer in trio] for trio in firsts]
    # depth 1, Pareto graph: gcn_l1_4 summed over the front's members, tiled over the nodes (_tile_pool, truss2D_RL.py:87-93)
    steps = [step(a.gcn_l1_4, x_p, A_p, nbr_p) for a in actors] if can_group else [None]
    widths = {s["w"].shape[0] for s in steps if s is not None}
    if all(s is not None for s in steps) and len(widths) == 1:
        H = widths.pop()
        pooled = torch.empty((A, B, H), dtype=torch.float32, device=x_n.device)
        launch([[s] for s in steps], [dict(kind="pool", pool=pooled[i]) for i in range(A)], GROUP_MAX_EPI)
        x14 = list(pooled.unsqueeze(-1).expand(A, B, H, N).reshape(A, B, N, H).unbind(0))     # one copy for all actors
    else:
        x14 = []
        for a in actors:
            p = g_pool(a.gcn_l1_4, x_p, A_p)
            x14.append(p.unsqueeze(-1).expand(p.shape[0], p.shape[1], N).reshape(p.shape[0], N, p.shape[1]).contiguous())
    # depth 2: five layers per actor that add into x3, in the order of actor_infer
    def seconds(a, x, x4, out):
        return [(a.gcn_l2_1, x[0], A_n, out, False), (a.gcn_l2_2, x[1], A_ts, out, True), (a.gcn_l2_3, x[1], A_cs, out, True),
                (a.gcn_l2_4, x[2], A_s, out, True), (a.gcn_l2_5, x4, A_n, out, True)]
    widths = {a.gcn_l2_1.lin.weight.shape[0] for a in actors}
    chains = None
    if can_group and len(widths) == 1:
        x3 = outputs(A, (B, N, widths.pop()))
        chains = [[step(layer, x.contiguous(), adj, nbr, out, acc) for layer, x, adj, out, acc in seconds(a, x1[i], x14[i], x3[i])]
                  for i, a in enumerate(actors)]
        if not all(s is not None and s["w"].shape[0] == s["out"].shape[2] for chain in chains for s in chain):
            chains = None
    if chains is not None:
        launch(chains, None, GROUP_MAX_STEPS // 5)
    else:
        x3 = []
        for i, a in enumerate(actors):
            calls = seconds(a, x1[i], x14[i], None)
            out = g(*calls[0][:3])
            for layer, x, adj, _, _ in calls[1:]:
                g(layer, x, adj, out=out, accumulate=True)
            x3.append(out)
    # depths 3 + 4: gcn_l3_1 + gcn_l4_1 over A_n, gcn_l3_2 over A_s with gcn_l4_2 over A_n
    pairs = [(layer, head, adj, x3[i]) for i, a in enumerate(actors)
             for layer, head, adj in ((a.gcn_l3_1, a.gcn_l4_1, A_n), (a.gcn_l3_2, a.gcn_l4_2, A_s))]
    steps = [step(layer, x, adj, nbr) for layer, _, adj, x in pairs] if can_group else [None]
    if all(s is not None for s in steps) and all(head.lin.weight.shape[0] <= 8 and gcn_layer_supported(N, head.lin.weight.shape[0], nbr)
                                                  for _, head, _, _ in pairs):
        epis = [dict(kind="head", w2=head.lin.weight.detach(), bias2=head.bias.detach(), adj2=A_n, nbr2=nbr, act2="sigmoid",
                     out2=torch.empty((B, N, head.lin.weight.shape[0]), dtype=torch.float32, device=x_n.device)) for _, head, _, _ in pairs]
        launch([[s] for s in steps], epis, GROUP_MAX_EPI)
        heads = [e["out2"] for e in epis]
    else:
        heads = [g_head(layer, head, x, adj, A_n) for layer, head, adj, x in pairs]
    return [(heads[2 * i], heads[2 * i + 1]) for i in range(A)]


class DeviceReplay:
    """Ring buffer of transitions in device memory (state / three next states as the eight observation
    tensors the networks take minus the topology-static A_n and mask, three agents' actions, rewards).

    storage="dense" (the default): every observation tensor is stored as it arrives; `add` / `sample` are indexing operations of the
    framework, one per tensor.
    storage="compact": the node-graph adjacencies A_s, A_n_ts, A_n_cs are stored as [capacity, N, Kn] through the truss's neighbour
    table `nbr` (int16 [N, Kn], TrussTopology.neighbor_table()) and the Pareto-graph adjacency A_p as [capacity, P, 3] through
    `nbr_p` (path_graph_table(P)); everything else as in dense storage.  `sample` still returns dense tensors, and the index draw is
    the same call on the same generator: a compact and a dense replay fed the same rows return the same batches.
    PRECONDITION (what makes compact storage lossless): every adjacency handed to `add` is exactly zero outside its table -- true of
    what the step / observation kernels and `pareto_graph` write (tests/test_replay_compact.py checks it on the emulator); entries
    outside the table would be dropped.
    On a cuda device with a native library that exports them, compact storage moves every field of a transition with ONE
    `replay_scatter` launch per `add` and ONE `replay_gather` launch per `sample` (csrc/truss_replay.h); on the cpu, or without the
    entries, the same semantics run as framework indexing (gather through the table on add, zeros + scatter on sample).
    fused=True does the same for dense storage (plain copies only); it needs the operators."""

    KEYS = ("x_n", "A_s", "A_n_ts", "A_n_cs", "x_p", "A_p")
    PATTERN_KEYS = ("A_s", "A_n_ts", "A_n_cs", "A_p")

    def __init__(self, capacity, N, P, device, storage="dense", nbr=None, nbr_p=None, lib=None, fused=False):
        if storage not in ("dense", "compact"):
            raise ValueError(f"storage must be 'dense' or 'compact', got {storage!r}")
        device = torch.device(device)
        f = lambda *s: torch.zeros((capacity,) + s, dtype=torch.float32, device=device)
        shapes = dict(x_n=(N, 13), A_s=(N, N), A_n_ts=(N, N), A_n_cs=(N, N), x_p=(P, 4), A_p=(P, P))
        self.storage, self.N, self.P = storage, N, P
        self._dense_shapes = dict(shapes)
        self._tab = {}                                        # key -> (table int16 [n, k], compact positions, dense positions)
        if storage == "compact":
            if nbr is None or nbr_p is None:
                raise ValueError("storage='compact' needs the neighbour tables nbr [N, Kn] and nbr_p [P, 3]")
            tn, tp = self._table(nbr, N, device), self._table(nbr_p, P, device)
            for k in self.PATTERN_KEYS:
                self._tab[k] = tp if k == "A_p" else tn
                shapes[k] = tuple(self._tab[k][0].shape)
        self.S = {k: f(*shapes[k]) for k in self.KEYS}
        self.NS = [{k: f(*shapes[k]) for k in self.KEYS} for _ in range(3)]
        self.a_geo, self.a_topo, self.R = f(3, N, 2), f(3, N, 3), f(3)
        self.capacity, self.size, self.head = capacity, 0, 0
        # the fused operators: compact storage takes them where they exist, fused dense storage demands them
        self._lib = None
        if device.type == "cuda" and (storage == "compact" or fused):
            lib = _lib.load() if lib is None else lib
            if lib.backend == "hip" and lib.has_replay_ops:
                self._lib = lib
        if fused and storage == "dense" and self._lib is None:
            raise _lib.TrussError("DeviceReplay(fused=True) needs a cuda device and a native library with truss_replay_scatter / truss_replay_gather")
        if self._lib is not None:
            # field lists in one fixed order: (ring tensor, key or None, table or None, row list of `rows`)
            self._fields = [(self.S[k], k, 0) for k in self.KEYS] + [(self.NS[a][k], k, 1 + a) for a in range(3) for k in self.KEYS]
            self._rings = [t for t, _, _ in self._fields] + [self.a_geo, self.a_topo, self.R]
            self._nbrs = [self._tab[k][0] if k in self._tab else None for _, k, _ in self._fields] + [None, None, None]
            self._groups = [g for _, _, g in self._fields] + [0, 0, 0]

    @staticmethod
    def _table(t, n, device):
        t = torch.as_tensor(np.asarray(t.cpu() if torch.is_tensor(t) else t), dtype=torch.int16)
        if t.dim() != 2 or t.shape[0] != n:
            raise ValueError(f"a neighbour table must be [{n}, k], got {tuple(t.shape)}")
        k = t.shape[1]
        slot = torch.nonzero(t.flatten() >= 0).flatten()                       # positions in a compact row [n * k]
        cols = (slot // k) * n + t.flatten()[slot].long()                      # ... and where they sit in the dense row [n * n]
        return t.contiguous().to(device), slot.to(device), cols.to(device)

    @property
    def nbytes(self):
        """bytes held by the buffer's tensors"""
        ts = list(self.S.values()) + [t for ns in self.NS for t in ns.values()] + [self.a_geo, self.a_topo, self.R]
        return sum(t.numel() * t.element_size() for t in ts)

    def _put(self, ring, key, pos, rows):
        """ring[pos] = rows (dense tensors [k, ...]); a pattern key of compact storage keeps the table's entries only"""
        if key in self._tab:
            _, slot, cols = self._tab[key]
            ring.view(self.capacity, -1)[pos[:, None], slot[None, :]] = rows.reshape(rows.shape[0], -1)[:, cols]
        else:
            ring[pos] = rows

    def _get(self, ring, key, i):
        if key in self._tab:
            _, slot, cols = self._tab[key]
            out = torch.zeros((i.numel(),) + self._dense_shapes[key], dtype=ring.dtype, device=ring.device)
            out.view(i.numel(), -1)[:, cols] = ring.view(self.capacity, -1)[i[:, None], slot[None, :]]
            return out
        return ring[i]

    def add(self, sel, S, NS, a_geo, a_topo, R, src=None):
        """append the transitions of the rows where sel[K] is True.  NS: three dicts (one per agent's next state), or -- with src
        [K, 3] -- ONE dict of tensors [3, K, ...] from which agent a's next state of row r is taken at [src[r, a], r].
        With the fused operators the sources are read in place, the accepted rows only, when they are float32 and strided over their
        first two dims at most (the [3, K, ...] tensors of the `src` form: contiguous); other layouts are copied whole first
        (`_rows_view`, and the `reshape` of a non-contiguous [3, K, ...] tensor)."""
        idx = torch.nonzero(sel, as_tuple=False).flatten()
        k = int(idx.numel())
        if k == 0:
            return 0
        if k > self.capacity:
            idx, k = idx[: self.capacity], self.capacity
        if self._lib is not None:
            self._add_fused(idx, k, S, NS, a_geo, a_topo, R, src)
        else:
            pos = (self.head + torch.arange(k, device=idx.device)) % self.capacity
            pick = None if src is None else src[idx]                               # [k, 3]
            if self._tab:
                for key in self.KEYS:
                    self._put(self.S[key], key, pos, S[key][idx])
                    for a in range(3):
                        self._put(self.NS[a][key], key, pos, NS[a][key][idx] if src is None else NS[key][pick[:, a], idx])
            else:
                for key in self.KEYS:
                    self.S[key][pos] = S[key][idx]
                    for a in range(3):
                        self.NS[a][key][pos] = NS[a][key][idx] if src is None else NS[key][pick[:, a], idx]
            self.a_geo[pos], self.a_topo[pos], self.R[pos] = a_geo[idx], a_topo[idx], R[idx]
        self.head = (self.head + k) % self.capacity
        self.size = min(self.capacity, self.size + k)
        return k

    @staticmethod
    def _rows_view(t):
        """`t` [K, ...] as the operators read it in place, the accepted rows only: float32, strided over dims 0 and 1 at most (a
        permuted view of an agent-major tensor).  Anything else -- another dtype, a layout strided below dim 1 -- is first copied IN
        FULL, all K rows (`.float()` / `.contiguous()`): correct, but the caller then pays for the rows that are not accepted."""
        t = t if t.dtype == torch.float32 else t.float()
        inner = lambda d0: all(t.shape[d] == 1 or t.stride(d) == int(np.prod(t.shape[d + 1:])) for d in range(d0, t.dim()))
        return t if inner(1) or (t.dim() >= 2 and inner(2) and t.stride(1) >= 0 and t.stride(0) >= 0) else t.contiguous()

    def _add_fused(self, idx, k, S, NS, a_geo, a_topo, R, src):
        from . import ops
        K = S[self.KEYS[0]].shape[0]
        if src is None:
            rows = idx[None, :].expand(4, k).contiguous()
            nxt = lambda a, key: NS[a][key]
        else:
            # agent a's next state of row r = row src[r, a] * K + r of the candidate tensors [3, K, ...] seen as [3 K, ...]
            rows = torch.cat([idx[None, :], (src[idx].to(torch.int64) * K + idx[:, None]).t()], dim=0).contiguous()
            flat = {key: NS[key].reshape(3 * K, *NS[key].shape[2:]) for key in self.KEYS}
            nxt = lambda a, key: flat[key]
        srcs = [S[key] for key in self.KEYS] + [nxt(a, key) for a in range(3) for key in self.KEYS] + [a_geo, a_topo, R]
        srcs = [self._rows_view(t) for t in srcs]
        ops.call(ops.namespace().replay_scatter, ops.bind(self._lib), ops.stream_of(self.R.device), self._rings, srcs, self._nbrs, self._groups,
                 rows, k, self.head, self.capacity)

    def sample(self, batch, generator=None):
        i = torch.randint(0, self.size, (batch,), device=self.R.device, generator=generator)
        if self._lib is not None:
            from . import ops
            new = lambda *s: torch.empty((batch,) + s, dtype=torch.float32, device=self.R.device)
            outs = [new(*self._dense_shapes[k]) for _, k, _ in self._fields] + [new(*t.shape[1:]) for t in (self.a_geo, self.a_topo, self.R)]
            ops.call(ops.namespace().replay_gather, ops.bind(self._lib), ops.stream_of(self.R.device), self._rings, outs, self._nbrs, i, self.capacity)
            nk = len(self.KEYS)
            d = lambda j: dict(zip(self.KEYS, outs[j * nk:(j + 1) * nk]))
            return d(0), [d(1 + a) for a in range(3)], outs[-3], outs[-2], outs[-1]
        if self._tab:
            pick = lambda d: {k: self._get(v, k, i) for k, v in d.items()}
        else:
            pick = lambda d: {k: v[i] for k, v in d.items()}
        return pick(self.S), [pick(ns) for ns in self.NS], self.a_geo[i], self.a_topo[i], self.R[i]


_SM64 = (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)


def _splitmix64(z):
    """splitmix64 finaliser on int64 tensors (two's complement wrap-around == uint64 arithmetic; logical shifts by mask)"""
    s64 = lambda c: c - (1 << 64) if c >= 1 << 63 else c
    srl = lambda v, k: (v >> k) & ((1 << (64 - k)) - 1)
    z = z + s64(_SM64[0])
    z = (z ^ srl(z, 30)) * s64(_SM64[1])
    z = (z ^ srl(z, 27)) * s64(_SM64[2])
    return z ^ srl(z, 31)


def design_coins(seed, env_ids, game_step, members):
    """D6: the symmetry coin of every move of the design game, uint8 [K, 3] (agent a in column a) for the pairs (env_ids[k],
    members[k]) of game step `game_step`: the top bit of splitmix64(splitmix64(seed) ^ (env << 26 | step << 10 | member << 2 | agent))
    (env < 2^38, step < 2^16, member < 256).  A pure function of those fields: the same on any device, for any pair order."""
    dev = env_ids.device
    key = (env_ids.to(torch.int64)[:, None] << 26) | (int(game_step) << 10) | (members.to(torch.int64)[:, None] << 2) \
        | torch.arange(3, dtype=torch.int64, device=dev)[None, :]
    h0 = _splitmix64(torch.tensor(int(seed), dtype=torch.int64, device=dev))
    return (_splitmix64(key ^ h0) < 0).to(torch.uint8)


def pair_dtab(device):
    """[0, 1^-1/2, 2^-1/2, 3^-1/2] as float32 values the way the framework rounds them on `device` (what `pareto_graph` gets from
    `deg.pow(-0.5)` there): the table `pair_setup` takes, so that its A_p carries the bits of `pareto_graph`.  Synchronises once."""
    return [0.0] + torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device=device).pow(-0.5).tolist()


def pair_frac_tab(max_front, device):
    """float32 [P + 1]: column 3 of the Pareto-graph features for n = 0..P as `pareto_graph` computes it on `device` (`n.float() /
    max_front`: on a GPU the framework multiplies by the rounded reciprocal of a host scalar, which is not always the correctly
    rounded quotient -- 49 / 50 comes out one ulp lower): the table `pair_setup` takes so that its x_p carries those bits."""
    return torch.arange(max_front + 1, dtype=torch.int32, device=device).float() / max_front


_PAIR_ROWS = (("x", "c_x"), ("target", "c_target"), ("params", "c_params"), ("y", "arch_y"), ("sec", "arch_sec"))


def pair_setup(lib, idx, ms, pts, n, arch_y, arch_sec, c_x, c_target, c_params, ref_points, *, rep=3, dtab=None, frac_tab=None,
               coins=None, par=None, cand=None, out=None, stream=None):
    """The set-up of K (env, member) pairs of a game step as one `truss_pair_setup` launch (include/truss_mi355.h, csrc/truss_pairs.h).

    idx, ms [K] int64 (pair k = env idx[k], member ms[k]; envs may repeat)
    pts [B,P,4] float64, n [B] int32, arch_y [B,P,N] float32, arch_sec [B,P,E] int32          the step-start archive
    c_x, c_target [B,N] float32, c_params [B,NPARAM] float64, ref_points [B,2] float64        per-env constants
    rep     1 or 3: copies of the Pareto graph (3: the candidates' next states, agent-major)
    dtab    the four float32 values [0, 1, 2, 3]^-1/2 (default: `pair_dtab(device)`, which synchronises -- callers in a loop keep it)
    frac_tab  None: column 3 of x_p is float(n) / float(P), one float32 division; or float32 [P + 1] with the value for every n
              (`pair_frac_tab(P, device)`: what the framework computes there)
    coins   None, or (seed, env_ids [B] int64, game_step): also the design game's coins (`design_coins`, agent-major)
    par / cand   dicts x, target, params, y, sec of tensors with at least K / 3 K rows to write the design rows into (the env
                 objects' resident buffers; rows behind stay as they are); None: new tensors
    out     dict of preallocated p0, nn0, parent_obj, ref, x_p, A_p, coin to write into instead of new tensors
    Returns dict(par, cand (the dicts), p0 [K,P,4], nn0 [K] int32, parent_obj [K,2], ref [K,2], x_p [rep K,P,4], A_p [rep K,P,P],
    coin [3 K] uint8 or None).  No output may overlap an input."""
    lib = lib or _lib.load()
    if not lib.has_pair_setup:
        raise _lib.TrussError(f"{lib.path} has no truss_pair_setup (the fused set-up of a chunk of pairs)")
    if rep not in (1, 3):
        raise ValueError(f"rep must be 1 or 3, got {rep!r}")
    K, (B, P), dev = int(idx.shape[0]), pts.shape[:2], pts.device
    src = dict(c_x=c_x, c_target=c_target, c_params=c_params, arch_y=arch_y, arch_sec=arch_sec)
    rows = lambda given, mult: {k: (given[k] if given is not None else torch.empty((mult * K, src[s].shape[-1]), dtype=src[s].dtype, device=dev))
                                for k, s in _PAIR_ROWS}
    par, cand = rows(par, 1), rows(cand, 3)
    out = dict(out or {})
    new = lambda key, shape, dt: out[key] if key in out else torch.empty(shape, dtype=dt, device=dev)
    res = dict(par=par, cand=cand, p0=new("p0", (K, P, 4), torch.float64), nn0=new("nn0", (K,), torch.int32),
               parent_obj=new("parent_obj", (K, 2), torch.float64), ref=new("ref", (K, 2), torch.float64),
               x_p=new("x_p", (rep * K, P, 4), torch.float32), A_p=new("A_p", (rep * K, P, P), torch.float32),
               coin=new("coin", (3 * K,), torch.uint8) if coins is not None else None)
    seed, env_ids, game_step = coins if coins is not None else (0, None, 0)
    from . import ops
    stream_i = ops.stream_of(dev) if stream is None else int(getattr(stream, "value", stream) or 0)
    ops.call(ops.namespace().pair_setup, ops.bind(lib), stream_i, int(rep), int(seed), int(game_step), list(dtab) if dtab is not None else pair_dtab(dev),
             idx, ms, pts, n, arch_y, arch_sec, c_x, c_target, c_params, ref_points, env_ids, frac_tab,
             par["x"], par["target"], par["params"], par["y"], par["sec"], cand["x"], cand["target"], cand["params"], cand["y"], cand["sec"],
             res["p0"], res["nn0"], res["parent_obj"], res["ref"], res["x_p"], res["A_p"], res["coin"])
    return res


class BatchedMARL:
    """game: "train" (the train copy: MAX_FRONT 20, no coin, culls of at most 64 rows, D1) or "test" (the design game of the
    test copies, see the module docstring: needs a topology built with `symmetry=`; MAX_FRONT 50 unless max_front says
    otherwise).  env_ids: global ids of the B envs (the coin's env field; default 0..B-1)."""

    def __init__(self, topo: TrussTopology, n_envs: int, maddpg, *, max_front: int | None = None, lib=None, device=None,
                 replay_capacity: int = 32768, batch_size: int = 32, hv_margin: float = 0.2, seed: int = 0,
                 pair_capacity: int | None = None, tune_update_gemms: bool = True, game: str = "train", env_ids=None,
                 level_backward: str | None = None, replay_storage: str | None = None, reward_path: str | None = None,
                 archive_path: str | None = None, actor_path: str | None = None, actor_precision: str | None = None,
                 pair_path: str | None = None):
        """pair_path: how a game step sets up a chunk of (env, member) pairs -- "torch" (gathers of the step-start archive, copies into the
        env objects, `pareto_graph`, `design_coins`: framework operators, the default) or "hip" (one `truss_pair_setup` launch per chunk;
        needs a library with that entry); None: "hip" if the environment has TRUSS_PAIRS=hip, else "torch".  Both play the same game,
        bit for bit.
        actor_precision: the product of the actors' hidden layers in the ROLLOUT (`actor_infer(precision=...)`): "bf16x3" (float32
        accuracy, the default), "f32", or the reduced "bf16x2" / "bf16" (two terms / one term of the bf16 split, truncated: errors of
        up to 2^-13 / 2^-6 of a layer's magnitude, every product biased towards zero; need a library with `truss_gcn_layer_terms`);
        None: the environment's TRUSS_ACTOR_PRECISION, else "bf16x3".  Composes with actor_path; the update is not affected (it
        evaluates the actors in float32 from the replayed states).
        actor_path: how the rollout evaluates an actor -- "layers" (13 launches of the fused layer kernel, the default) or "fused"
        (`actor_infer(fused=True)`: the Pareto pool and the two action heads run in the epilogues of the layers that feed them, 11
        launches; needs a library with `truss_gcn_layer_fused`) or "grouped" (`actors_infer`: the fused path for all three actors at
        once, every depth of their layers ONE launch of `truss_gcn_layer_group` -- four launches per call instead of 33, the same bits
        as "fused"; needs a library with that entry); None: the environment's TRUSS_ACTOR if it is "fused" or "grouped", else "layers".
        archive_path: how a game step updates the archives -- "torch" (candidate buffers, one `truss_front` launch and gathers by
        framework operators, the default) or "hip" (one `truss_archive_merge` launch per chunk, per step in the design game; needs a
        library with that entry; the archive then lives in two sets of buffers that swap roles); None: "hip" if the environment has
        TRUSS_ARCHIVE=hip, else "torch".  Both play the same game, bit for bit.
        reward_path: how a game step computes the difference reward of a chunk of pairs -- "torch" (three `truss_front` launches plus
        element-wise operators, the default) or "hip" (one `truss_reward` launch; needs max_front + 3 <= 64 and a library with that
        entry); None: "hip" if the environment has TRUSS_REWARD=hip, else "torch".
        replay_storage: "dense" (the default) or "compact" (`DeviceReplay`: adjacencies stored through the neighbour tables, one
        launch per append / sample on the GPU); None: "compact" if the environment has TRUSS_REPLAY_STORAGE=compact, else "dense".
        level_backward: how the update differentiates a level of GCN layers on the GPU -- "library" (batched library GEMMs, the
        default) or "hip" (one `truss_gcn_level_backward` launch per level); None: "hip" if the environment has
        TRUSS_LEVEL_BACKWARD=1, else "library".  The choice is installed process-wide for cuda tensors (like the level forward)
        and is part of an update graph from the moment it is captured."""
        if game not in ("train", "test"):
            raise ValueError(f"game must be 'train' or 'test', got {game!r}")
        if game == "test" and len(topo.sym_nodes) == 0:
            raise ValueError("game='test' modifies mirror-symmetric designs: build the topology with symmetry='small' or 'large'")
        if max_front is None:
            max_front = 50 if game == "test" else 20
        self.game = game
        self.topo, self.B, self.P = topo, int(n_envs), int(max_front)
        self.rl = maddpg
        if tune_update_gemms and (device is None or torch.device(device).type == "cuda"):
            enable_gemm_tuning()      # library GEMM per (fixed) shape of the update, chosen during its warm-up (23 -> 14 ms per update)
        if game == "test":
            # one cull per game step over the P archive rows + the 3 candidates of every member
            if 4 * self.P > _lib.FRONT_MAXP:
                raise ValueError(f"game='test': max_front {self.P} needs {4 * self.P} rows per cull, the front kernel takes {_lib.FRONT_MAXP}")
            self.Gm = self.P
        else:
            # members whose candidates fit one cull: P archive rows + 3 candidates per member <= the front kernel's 64 rows
            self.Gm = max(1, min(self.P, (64 - self.P) // 3))
        # (env, member) pairs per pass: the env objects below hold that many designs (3 x as many candidates)
        self.cap = int(pair_capacity) if pair_capacity else min(self.B * self.Gm, 4 * self.B)
        self.cap = max(self.cap, self.B)
        self.envP = BatchedTruss(topo, self.cap, device=device, lib=lib)          # archive members under study
        self.envC = BatchedTruss(topo, 3 * self.cap, device=device, lib=lib)      # their candidates, agent-major
        self.lib, self.device = self.envP.lib, self.envP.device
        if self.device.type == "cuda" and os.environ.get("TRUSS_LEVEL_FORWARD", "1") != "0":
            import truss2D_RL
            truss2D_RL.set_level_forward(level_forward(self.lib), "cuda")   # the update's forward passes: one launch per level
        if level_backward is None:
            level_backward = "hip" if os.environ.get("TRUSS_LEVEL_BACKWARD", "0") == "1" else "library"
        if level_backward not in ("library", "hip"):
            raise ValueError(f"level_backward must be 'library' or 'hip', got {level_backward!r}")
        self.level_backward = level_backward
        if replay_storage is None:
            replay_storage = "compact" if os.environ.get("TRUSS_REPLAY_STORAGE", "dense") == "compact" else "dense"
        if replay_storage not in ("dense", "compact"):
            raise ValueError(f"replay_storage must be 'dense' or 'compact', got {replay_storage!r}")
        self.replay_storage = replay_storage
        if reward_path is None:
            reward_path = "hip" if os.environ.get("TRUSS_REWARD", "torch") == "hip" else "torch"
        if reward_path not in ("torch", "hip"):
            raise ValueError(f"reward_path must be 'torch' or 'hip', got {reward_path!r}")
        if reward_path == "hip":
            if not self.lib.has_reward:
                raise ValueError(f"reward_path='hip': {self.lib.path} has no truss_reward")
            if self.P + 3 > 64:
                raise ValueError(f"reward_path='hip': max_front {self.P} + 3 new points exceed the 64 rows of a wave (truss_reward)")
        self.reward_path = reward_path
        if archive_path is None:
            archive_path = "hip" if os.environ.get("TRUSS_ARCHIVE", "torch") == "hip" else "torch"
        if archive_path not in ("torch", "hip"):
            raise ValueError(f"archive_path must be 'torch' or 'hip', got {archive_path!r}")
        if archive_path == "hip":
            if not self.lib.has_archive:
                raise ValueError(f"archive_path='hip': {self.lib.path} has no truss_archive_merge")
            if self.P + 3 * self.Gm > _lib.ARCHIVE_MAXROWS:
                raise ValueError(f"archive_path='hip': max_front {self.P} + {3 * self.Gm} candidate slots exceed the "
                                 f"{_lib.ARCHIVE_MAXROWS} rows of truss_archive_merge")
        self.archive_path = archive_path
        if pair_path is None:
            pair_path = "hip" if os.environ.get("TRUSS_PAIRS", "torch") == "hip" else "torch"
        if pair_path not in ("torch", "hip"):
            raise ValueError(f"pair_path must be 'torch' or 'hip', got {pair_path!r}")
        if pair_path == "hip":
            if not self.lib.has_pair_setup:
                raise ValueError(f"pair_path='hip': {self.lib.path} has no truss_pair_setup")
            if self.P > _lib.PAIR_MAXP:
                raise ValueError(f"pair_path='hip': max_front {self.P} exceeds the {_lib.PAIR_MAXP} rows of truss_pair_setup")
        self.pair_path = pair_path
        if actor_path is None:
            actor_path = os.environ.get("TRUSS_ACTOR", "layers")
            actor_path = actor_path if actor_path in ("fused", "grouped") else "layers"
        if actor_path not in ("layers", "fused", "grouped"):
            raise ValueError(f"actor_path must be 'layers', 'fused' or 'grouped', got {actor_path!r}")
        if actor_path == "grouped" and not self.lib.has_gcn_group:
            raise ValueError(f"actor_path='grouped': {self.lib.path} has no truss_gcn_layer_group")
        if actor_path in ("fused", "grouped") and not self.lib.has_gcn_fused:       # (a level outside the group's envelope runs fused)
            raise ValueError(f"actor_path={actor_path!r}: {self.lib.path} has no truss_gcn_layer_fused")
        self.actor_path = actor_path
        if actor_precision is None:
            actor_precision = os.environ.get("TRUSS_ACTOR_PRECISION", "bf16x3")
        _check_precision(actor_precision, "actor_precision")
        if actor_precision in ("bf16x2", "bf16") and not self.lib.has_gcn_terms:
            raise ValueError(f"actor_precision={actor_precision!r}: {self.lib.path} has no truss_gcn_layer_terms")
        self.actor_precision = actor_precision
        self._arch_spare = None       # archive_path="hip": the set of archive buffers the next merge writes (see _merge_archive)
        self._pair_dtab = self._pair_frac = None   # pair_path="hip": deg^-1/2 and n / P as the framework rounds them on this device
        #                                             (pair_dtab, pair_frac_tab; made at the first step)
        if self.device.type == "cuda":
            import truss2D_RL
            truss2D_RL.set_level_backward(_level_backward_hook(self.lib) if level_backward == "hip" else None, "cuda")
        dev, B, P, N, E = self.device, self.B, self.P, topo.N, topo.E
        A_n, mask = topo.normalized_adjacency()
        self.A_n = torch.tensor(A_n, device=dev)[None]
        self.mask = torch.tensor(mask, device=dev)[None]
        self.nbr = torch.tensor(topo.neighbor_table(), device=dev)     # sparsity pattern of every node-graph adjacency (actor inference)
        self.nbr_p = torch.tensor(path_graph_table(P), device=dev)     # ... and of the Pareto graph (a path over the front's members)
        self.pts = torch.zeros((B, P, 4), dtype=torch.float64, device=dev)
        self.arch_y = torch.zeros((B, P, N), dtype=torch.float32, device=dev)
        self.arch_sec = torch.zeros((B, P, E), dtype=torch.int32, device=dev)
        self.n = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.ref_points = torch.ones((B, 2), dtype=torch.float64, device=dev)
        self.replay = DeviceReplay(replay_capacity, N, P, dev, storage=replay_storage, nbr=self.nbr, nbr_p=self.nbr_p, lib=self.lib)
        self.batch_size, self.hv_margin = batch_size, hv_margin
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.seed = int(seed)
        self.env_ids = (torch.arange(B, dtype=torch.int64, device=dev) if env_ids is None else
                        torch.as_tensor(np.asarray(env_ids, np.int64), device=dev))
        assert self.env_ids.shape == (B,)
        self.end_step = None           # design game: the game step whose cull is the final one (design_episode sets it)
        self.final = None              # design game: the final front after that step (see _design_cull)
        self.game_step = 1
        self._steps_dev = torch.zeros((), dtype=torch.int64, device=self.device)
        self._synced = False
        self._tg, self.use_train_graph = None, True
        self.profile = None            # set to {} to accumulate synchronised wall time per segment (diagnostic)

    def _tick(self, name, t0):
        if self.profile is None:
            return t0
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        self.profile[name] = self.profile.get(name, 0.0) + (t1 - t0)
        return t1

    @property
    def env_steps(self):
        """agent modifications evaluated so far (3 per live archive member per game step)"""
        return int(self._steps_dev.item())

    # ---- episode set-up (Game_research04.__init__ / ENV.reset / run() prologue, :164-196) ----
    def reset(self, x, target, y_max, d_min, max_def, load_x, load_y, is_roof, y0, sec0):
        def tiled(a, rep):                                   # per-env arrays [B] / [B, N] -> [rep B, ...]; scalars as they are
            a = np.asarray(a, np.float64)
            if a.ndim == 0:
                return a
            a = np.broadcast_to(a, (self.B,) + a.shape[1:]) if a.shape[0] != self.B else a
            return np.tile(a, (rep,) + (1,) * (a.ndim - 1))
        # the reset analysis of the B designs (normalisers int_obj1 / int_obj2, :264-274) on a B-env object
        e0 = BatchedTruss(self.topo, self.B, device=self.device, lib=self.lib)
        e0.set_constants(*[tiled(a, 1) for a in (x, target, y_max, d_min, max_def, load_x, load_y, is_roof)])
        e0.set_design(y0, sec0)
        e0.analyze(set_normalisers=True)
        # per-env constants of the whole batch: the pair-sized env objects are re-filled with the constants of the LIVE
        # (env, member) pairs of every pass, compacted to the front (BatchedTruss n_active)
        self.c_x, self.c_target, self.c_params = e0.x.clone(), e0.target.clone(), e0.env_params.clone()
        self._y_reset, self._sec_reset = e0.y.clone(), e0.sec.clone()
        self.pts.zero_(); self.arch_y.zero_(); self.arch_sec.zero_()
        self.pts[:, 0, 0:2] = 1.0                                    # Pf = [[1, 1, 0, 0, S0, ...]] (:168)
        self.arch_y[:, 0] = self._y_reset
        self.arch_sec[:, 0] = self._sec_reset
        self.n.fill_(1)
        self.ref_points.fill_(1.0)
        self.game_step = 1
        self.final = None

    # ---- observation tensors in the networks' order ----
    def _obs(self, env, pts0, n0, index, rep=1, k=None, o=None, graph=None):
        """o: observation tensors the analysis / step call has already written (TRUSS_F_EMIT_OBS); None = observation kernel.
        graph: (x_p, A_p) of the same (pts0, n0, index) if the caller has them already (the candidates see their parent's front)"""
        k = env.B if k is None else k
        if o is None:
            o = env.observe(n_active=k)
        x_p, A_p = graph if graph is not None else pareto_graph(pts0, n0, index, self.P)
        if rep > 1:
            x_p, A_p = x_p.repeat(rep, 1, 1), A_p.repeat(rep, 1, 1)
        # views of the env's own observation buffers: the caller is done with them (actor inference, replay rows) before the same env
        # object analyses / steps again
        c = lambda key: o[key][:k]
        return dict(x_n=c("x_n"), A_s=c("A_s"), A_n_ts=c("A_n_ts"), A_n_cs=c("A_n_cs"), x_p=x_p, A_p=A_p)

    def _net_state(self, S):
        b = S["x_n"].shape[0]
        return [S["x_n"], self.A_n.expand(b, -1, -1), S["A_s"], S["A_n_ts"], S["A_n_cs"], self.mask.expand(b, -1, -1), S["x_p"], S["A_p"]]

    def _noise_vectors(self, noises):
        """(theta dt, mu, sigma) of a list of OUNoise objects as per-column device vectors (cached on the list's first object)"""
        hit = getattr(noises[0], "_dev_vectors", None)
        if hit is None or hit[0].device != self.device:
            f = lambda vals: torch.tensor(vals, dtype=torch.float32, device=self.device)
            hit = (f([nz.theta * nz.dt for nz in noises]), f([nz.mu for nz in noises]), f([nz.sigma for nz in noises]))
            noises[0]._dev_vectors = hit
        return hit

    def _act(self, S, explore):
        ins = self._net_state(S)
        actor_in = [ins[0], ins[1], ins[2], ins[3], ins[4], ins[6], ins[7]]
        geo, topo = [], []
        net_in = [actor_in[0], self.A_n[0], actor_in[2], actor_in[3], actor_in[4], actor_in[5], actor_in[6]]
        with torch.no_grad():
            grouped = None
            if self.actor_path == "grouped":                          # every actor's layers of a depth in one launch, before any noise
                grouped = actors_infer(self.lib, [ag.actor_model for ag in self.rl.agents], net_in, nbr=self.nbr, nbr_p=self.nbr_p,
                                       precision=self.actor_precision)
            for i, ag in enumerate(self.rl.agents):
                g, t = grouped[i] if grouped is not None else actor_infer(
                    self.lib, ag.actor_model, net_in, nbr=self.nbr, nbr_p=self.nbr_p, fused=self.actor_path == "fused",
                    precision=self.actor_precision)
                if explore:                                          # truss2D_RL.OUNoise.gen_noise per scalar (:41-48), all columns at once
                    for out, noises in ((g, ag.noise_geo), (t, ag.noise_topo)):
                        th_dt, mu, sg = self._noise_vectors(noises)
                        out.addcmul_(th_dt, mu - out).addcmul_(sg, torch.randn(out.shape, device=out.device, generator=self.gen))
                geo.append(g.float().contiguous())
                topo.append(t.float().contiguous())
        return geo, topo

    # ---- the MADDPG update: eager, or (one GPU) replayed as a hipGraph ----
    def _train(self, S, NS, A, R):
        """The update is thousands of small kernels at batch 32 -- launch-bound.  On the GPU it is captured once into a hipGraph
        (static input buffers, capturable Adam) and replayed -- data-parallel too: the gradient all-reduces (RCCL; one flat
        buffer for the three critics, one per actor) are captured WITH the update, every rank replaying its own copy of the same
        graph.  On the CPU backend (gloo tests) it runs eagerly."""
        if self.device.type != "cuda" or not self.use_train_graph:
            return self.rl.train_on_batch(S, NS, A, R)
        flat_in = list(S) + [t for ns in NS for t in ns] + [t for a in A for t in a] + [R]
        if self._tg is None:
            try:
                # static input buffers of the graph.  Inputs that are broadcast constants (the shared adjacency A_n, the mask: stride 0
                # over the batch) are captured as they are -- nothing to copy per update, and the passes see ONE shared adjacency
                bufs = [t if (t.dim() and t.stride(0) == 0) else t.clone() for t in flat_in]
                nS = len(S)

                def unpack(b):
                    s_ = b[:nS]
                    ns_ = [b[nS * (1 + k): nS * (2 + k)] for k in range(3)]
                    a_ = b[4 * nS: 4 * nS + 6]
                    return s_, ns_, [(a_[0], a_[1]), (a_[2], a_[3]), (a_[4], a_[5])], b[4 * nS + 6]

                # the warm-up runs real updates: weights and optimiser moments are put back afterwards (in place,
                # the graph holds their addresses), so that training is what it would have been without capture
                nets = [n for ag_ in self.rl.agents for n in (ag_.actor_model, ag_.critic_model, ag_.target_actor_model,
                                                                ag_.target_critic_model)]
                self.rl._ensure_ready(S, [A[0][0], A[0][1], A[1][0], A[1][1], A[2][0], A[2][1]])
                # the inference caches of every actor (split images, padded input weights) exist before capture: the captured
                # update rewrites them in place at its end, so that the rollout acts with the weights each replay wrote
                with torch.no_grad():
                    for ag_ in self.rl.agents:
                        actor_infer(self.lib, ag_.actor_model, [S[0][:1], self.A_n[0], S[2][:1], S[3][:1], S[4][:1], S[6][:1], S[7][:1]],
                                    nbr=self.nbr, nbr_p=self.nbr_p, fused=self.actor_path != "layers",   # (grouped: the same caches)
                                    precision=self.actor_precision)
                snap =[[p.detach().clone() for p in n.parameters()] for n in nets]
                osnap = [t.clone() for t in self.rl.critics_opt.state_tensors()]    # [] = no step taken yet (one optimiser for the three critics)
                n_loss = [len(ag_.c_loss) for ag_ in self.rl.agents]
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(side):
                    if _TUNE_UPDATE_GEMMS:
                        torch.cuda.tunable.tuning_enable(True)           # the update's GEMM shapes are fixed: pick their kernels now
                    try:
                        for _ in range(3):                               # warm-up on the capture stream
                            self.rl.train_on_batch(*unpack(bufs))
                    finally:
                        if _TUNE_UPDATE_GEMMS:
                            torch.cuda.tunable.tuning_enable(False)
                torch.cuda.current_stream(self.device).wait_stream(side)
                torch.cuda.synchronize(self.device)
                d_ = getattr(self.rl, "dist", None)
                if d_ is not None and d_.is_initialized():
                    # The process group's watchdog thread polls the events of every eagerly enqueued collective until it has seen
                    # it complete (about every 100 ms).  A poll that lands inside the capture below, on an event of the stream the
                    # captured collectives run on, aborts the process (hipErrorCapturedEvent; this PyTorch build does not hold a
                    # capture back for pending polls).  The warm-up's collectives have completed (synchronize above): wait until
                    # the watchdog has retired them.
                    time.sleep(0.5)

                def restore():      # weights, Adam moments and loss log back to the state before the warm-up
                    with torch.no_grad():
                        for n, sp in zip(nets, snap):
                            for p, v in zip(n.parameters(), sp):
                                p.copy_(v)
                        for k, t in enumerate(self.rl.critics_opt.state_tensors()):
                            t.copy_(osnap[k]) if osnap else t.zero_()
                    for ag_, nl in zip(self.rl.agents, n_loss):
                        del ag_.c_loss[nl:]

                g = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(g, stream=side):
                        self.rl.train_on_batch(*unpack(bufs))
                        with torch.no_grad():
                            for ag_ in self.rl.agents:
                                refresh_actor_caches(self.lib, ag_.actor_model)
                finally:
                    restore()       # captured or not: training continues from the pre-warm-up state
                self._tg = (g, bufs)
            except RuntimeError as e:                                    # capture is an optimisation, never a requirement
                print(f"[marl] hipGraph capture of the MADDPG update failed ({type(e).__name__}: {e}); running eagerly")
                self.use_train_graph = False
                torch.cuda.synchronize(self.device)
                return self.rl.train_on_batch(S, NS, A, R)
        g, bufs = self._tg
        # broadcast constants were captured by address: a call that brings another one (or a shape the graph was not captured
        # for) runs eagerly -- never a copy into an expanded buffer, never the captured adjacency in its place
        if any(b.dim() and b.stride(0) == 0 and (t.data_ptr() != b.data_ptr() or t.stride() != b.stride() or t.shape != b.shape)
               for b, t in zip(bufs, flat_in)):
            return self.rl.train_on_batch(S, NS, A, R)
        pairs = [(b, t) for b, t in zip(bufs, flat_in) if b is not t and b.data_ptr() != t.data_ptr()]
        torch._foreach_copy_([b for b, _ in pairs], [t for _, t in pairs])    # multi-tensor launches for the ~30 input tensors
        g.replay()

    # ---- one game step of every env (run() :198-705) ----
    def game_step_all(self, train: bool | None = None, explore: bool = True, train_iters: int = 1, update: bool = True):
        """train: push accepted transitions to the replay and (with `update`) run `train_iters` MADDPG updates from it
        (default: True in the train game; the design game does not train); update=False leaves the updates to the caller
        (MixedMARL: one set of agents over several size classes).
        Design game: every move gets its coin (D6), the step ends with one cull of the archive and all candidates, truncated to
        max_front -- or, at game step `end_step`, not truncated: the final front (`self.final`).  The result adds G_U [B]."""
        test = self.game == "test"
        if train is None:
            train = not test
        if test and train:
            raise ValueError("the design game (game='test') does not train (train_period = 0)")
        B, P, Gm = self.B, self.P, self.Gm
        pts0, n0 = self.pts.clone(), self.n.clone()                   # front_no / Pf_HV of this step (:203-209)
        y0, sec0 = self.arch_y.clone(), self.arch_sec.clone()
        added = 0
        rsum = torch.zeros((B, 3), dtype=torch.float64, device=self.device)
        tk = time.perf_counter()
        dev = self.device
        N, E = self.topo.N, self.topo.E
        arP = self._const("arP", lambda: torch.arange(P, device=dev))
        n_max = int(n0.max().item())
        if test:                      # step-wide candidate buffers, slot = 3 member + agent (empty slot = infeasible row [0, 0, 2, 0])
            gsum = torch.zeros((B,), dtype=torch.float64, device=dev)
            stepP = self._const("stepP", lambda: torch.tensor([0.0, 0.0, 2.0, 0.0], dtype=torch.float64, device=dev).expand(B, 3 * P, 4)).clone()
            stepY = torch.zeros((B, 3 * P, N), dtype=torch.float32, device=dev)
            stepS = torch.zeros((B, 3 * P, E), dtype=torch.int32, device=dev)
        for g0 in range(0, n_max, Gm):                                # member groups whose candidates fit one cull
            # live (env, member) pairs of this group, member-major: pair k = (env pb[k], member pm[k])
            livemask = (arP[None, g0:g0 + Gm] < n0[:, None])          # [B, Gm]
            pm_all, pb_all = torch.nonzero(livemask.t(), as_tuple=True)
            pm_all = pm_all + g0
            for c0 in range(0, int(pb_all.numel()), self.cap):
                tk = self._tick("other", tk)
                idx, ms = pb_all[c0:c0 + self.cap], pm_all[c0:c0 + self.cap]
                K = int(idx.numel())
                eP, eC = self.envP, self.envC
                hip_pairs = self.pair_path == "hip"
                if hip_pairs:
                    # one launch: the design rows of the parents and of their candidates straight into the env objects' buffers, the
                    # step-start archive of every pair, the Pareto graph (three times over for the next states) and the coins
                    if self._pair_dtab is None:
                        self._pair_dtab, self._pair_frac = pair_dtab(dev), pair_frac_tab(P, dev)
                    env_rows = lambda e: dict(x=e.x, target=e.target, params=e.env_params, y=e.y, sec=e.sec)
                    pq = pair_setup(self.lib, idx, ms, pts0, n0, y0, sec0, self.c_x, self.c_target, self.c_params, self.ref_points,
                                    rep=1 if test else 3, dtab=self._pair_dtab, frac_tab=self._pair_frac, par=env_rows(eP), cand=env_rows(eC),
                                    coins=(self.seed, self.env_ids, self.game_step) if test else None)
                    p0, nn0 = pq["p0"], pq["nn0"]
                    ark = torch.arange(K, device=dev) if self.archive_path == "hip" and not test else None   # (the merge's table of rows)
                    S = self._obs(eP, p0, nn0, ms, k=K, o=eP.analyze(n_active=K, obs=True), graph=(pq["x_p"][:K], pq["A_p"][:K]))
                else:
                    ark = torch.arange(K, device=dev)
                    p0, nn0 = pts0[idx].contiguous(), n0[idx].contiguous()
                    py, ps = y0[idx, ms], sec0[idx, ms]
                    cx, ct, cp = self.c_x[idx], self.c_target[idx], self.c_params[idx]
                    # parents: the members of the step-start archive (:211-221)
                    eP.x[:K], eP.target[:K], eP.env_params[:K] = cx, ct, cp
                    eP.y[:K], eP.sec[:K] = py, ps
                    S = self._obs(eP, p0, nn0, ms, k=K, o=eP.analyze(n_active=K, obs=True))   # analysis + observations: one launch
                tk = self._tick("parent analysis + obs", tk)
                geo, topo = self._act(S, explore)
                tk = self._tick("actors", tk)
                # the three agents modify the SAME parent (:249-260): one launch over 3 K envs, agent-major
                if not hip_pairs:
                    eC.x[:3 * K], eC.target[:3 * K], eC.env_params[:3 * K] = cx.repeat(3, 1), ct.repeat(3, 1), cp.repeat(3, 1)
                    eC.y[:3 * K], eC.sec[:3 * K] = py.repeat(3, 1), ps.repeat(3, 1)
                a_geo, a_topo = torch.cat(geo, 0).contiguous(), torch.cat(topo, 0).contiguous()
                coin = None
                if test:                                                                     # D6: agent-major like the candidates
                    coin = pq["coin"] if hip_pairs else design_coins(self.seed, self.env_ids[idx], self.game_step, ms).t().contiguous().view(-1)
                oC = eC.step(a_geo, a_topo, coin, clamp_inplace=True, n_active=3 * K, obs=not test)   # clamped actions go to the replay (:375);
                self._steps_dev += 3 * K                                                     # step + next-state observations: one launch
                if test:
                    NSall = None
                elif hip_pairs:                                                              # the kernel wrote the three copies
                    NSall = self._obs(eC, p0, nn0, ms, k=3 * K, o=oC, graph=(pq["x_p"], pq["A_p"]))
                else:
                    NSall = self._obs(eC, p0, nn0, ms, rep=3, k=3 * K, o=oC, graph=(S["x_p"], S["A_p"]))
                tk = self._tick("candidate step + obs", tk)
                points = eC.point[:3 * K].view(3, K, 4).permute(1, 0, 2).double().contiguous()
                cand_y = eC.y[:3 * K].view(3, K, -1).permute(1, 0, 2)
                cand_sec = eC.sec[:3 * K].view(3, K, -1).permute(1, 0, 2)
                parent_obj, ref = (pq["parent_obj"], pq["ref"]) if hip_pairs else (p0[ark, ms, :2].contiguous(), self.ref_points[idx].contiguous())
                R, G_U, _, _ = RW.difference_reward(p0, nn0, p0, nn0, parent_obj, points, ref, nn0, max_front=P, lib=self.lib, path=self.reward_path)
                rsum.index_add_(0, idx, R)
                tk = self._tick("reward", tk)
                ok = (points[:, :, 2:4] <= 1).all(dim=2)                                      # archive candidates (:372)
                if test:                                                                      # collected; culled once after the last chunk
                    gsum.index_add_(0, idx, G_U)
                    slot = (ms * 3)[:, None] + self._const("ar3", lambda: torch.arange(3, device=dev)[None, :])
                    stepP[idx[:, None], slot] = torch.cat([points[:, :, :2], torch.where(ok, points[:, :, 2], 2.0)[:, :, None],
                                                           points[:, :, 3:]], dim=2)
                    stepY[idx[:, None], slot] = cand_y
                    stepS[idx[:, None], slot] = cand_sec
                    tk = self._tick("archive update", tk)
                    continue
                # ---- archive update (D1): front of (working archive + the feasible candidates of this chunk's members) ----
                C3 = 3 * Gm
                slot = ((ms - g0) * 3)[:, None] + self._const("ar3", lambda: torch.arange(3, device=dev)[None, :])   # [K, 3] candidate slot of (pair, agent)
                if self.archive_path == "hip":
                    # one launch: the candidates are handed over as they lie (agent-major rows a K + k of the candidate env's tensors)
                    # through a [B, C3] table of rows, -1 = empty slot
                    slot_row = torch.full((B, C3), -1, dtype=torch.int32, device=dev)
                    slot_row[idx[:, None], slot] = (self._const("ar3", lambda: torch.arange(3, device=dev)[None, :]) * K + ark[:, None]).int()
                    acc = self._merge_archive(eC.point[:3 * K].double(), eC.y[:3 * K], eC.sec[:3 * K], slot_row, C3, accepted=train)
                else:
                    candP = self._const("candP", lambda: torch.tensor([0.0, 0.0, 2.0, 0.0], dtype=torch.float64, device=dev).expand(B, C3, 4)).clone()
                    #                                                                               (empty slot = infeasible row: [0, 0, 2, 0])
                    candY = torch.zeros((B, C3, N), dtype=torch.float32, device=dev)
                    candS = torch.zeros((B, C3, E), dtype=torch.int32, device=dev)
                    pmark = points.clone()
                    pmark[:, :, 2] = torch.where(ok, pmark[:, :, 2], 2.0)
                    candP[idx[:, None], slot] = pmark
                    candY[idx[:, None], slot] = cand_y
                    candS[idx[:, None], slot] = cand_sec
                    wp, wy, ws, wn = self.pts, self.arch_y, self.arch_sec, self.n
                    origp = torch.cat([wp, candP], dim=1)
                    allp = origp.clone()
                    dead = arP[None, :] >= wn[:, None]
                    allp[:, :P, 2] = torch.where(dead, 2.0, allp[:, :P, 2])                          # infeasible marker
                    fr = RW.front_hv(allp, self._const("full_front", lambda: torch.full((B,), P + C3, dtype=torch.int32, device=dev)), None,
                                     max_front=P, lib=self.lib)
                    fidx = fr["front_idx"][:, :P].long()
                    take = fidx.clamp(min=0)
                    ally = torch.cat([wy, candY], dim=1)
                    alls = torch.cat([ws, candS], dim=1)
                    rows = self._const("rows", lambda: torch.arange(B, device=dev)[:, None])
                    live = (fidx >= 0)[:, :, None]
                    newp = torch.where(live, origp[rows, take], 0.0)
                    newp[:, :, 0:2].clamp_(max=1.0)                                                   # :434-436
                    self.pts = newp
                    self.arch_y = torch.where(live, ally[rows, take], 0.0)
                    self.arch_sec = torch.where(live, alls[rows, take], 0)
                    self.n = fr["n_front"].clamp(max=P)                                           # (int32 already)
                tk = self._tick("archive update", tk)
                # ---- replay (D2): one row per pair with an accepted candidate ----
                if train:
                    if self.archive_path == "hip":
                        accepted = acc[idx[:, None], slot].bool()                            # [K, 3]: one gather from the kernel's flags
                    else:
                        infront = torch.zeros((B, P + C3), dtype=torch.bool, device=dev)
                        infront.scatter_(1, take, live[:, :, 0])
                        accepted = infront[idx[:, None], P + slot] & ok                      # [K, 3]
                    first_ok = torch.argmax(ok.int(), dim=1)                                   # D4
                    # next state of agent a = its own candidate where that is feasible, else the first feasible one (D4): the rows are
                    # picked from the agent-major candidate tensors inside `add`, for the accepted pairs only
                    src = torch.where(ok, torch.arange(3, device=dev)[None, :], first_ok[:, None])   # [K, 3]
                    NSv = {k: NSall[k].view(3, K, *NSall[k].shape[1:]) for k in DeviceReplay.KEYS}
                    ag = a_geo.view(3, K, -1, 2).permute(1, 0, 2, 3)
                    at = a_topo.view(3, K, -1, 3).permute(1, 0, 2, 3)
                    added += self.replay.add(accepted.any(dim=1), S, NSv, ag, at, R.float(), src=src)
                tk = self._tick("replay", tk)
        # ---- end of the game step (:430-473, 642) ----
        if test:
            final = self.end_step is not None and self.game_step >= self.end_step
            fin = self._design_cull(stepP, stepY, stepS, final)
            tk = self._tick("archive update", tk)
        if test and final:
            hv = dict(hv_front=fin["hv"], metrics=fin["metrics"])
            n_out = fin["n"].clone()
        else:
            hv = RW.front_hv(self.pts.contiguous(), self.n, None, 0, self.lib)
            n_out = self.n.clone()
        self.ref_points = torch.clamp(self.ref_points + self.hv_margin, max=1.0)
        self.game_step += 1
        if update:
            self.train_from_replay(train_iters if train else 0)
        tk = self._tick("train", tk)
        out = dict(hv=hv["hv_front"], n_front=n_out, sum_distance=hv["metrics"][:, 3], reward=rsum, replay_added=added,
                   replay_size=self.replay.size)
        if test:
            out["G_U"] = gsum
        return out

    def _design_cull(self, candP, candY, candS, final):
        """Design game: the ONE cull of a game step, over the archive (P rows, dead rows marked infeasible) + the step's 3 P
        candidate slots.  Truncated to max_front (D3) and written to the archive; at the final step not truncated (simple_cull_final,
        master…:424-428, 680): the archive is left as it was and `self.final` = dict(points [B, 4P, 4] (objectives clipped to <= 1
        like the archive's, :683-686), y [B, 4P, N], sec [B, 4P, E], n [B], hv [B], metrics [B, 5]), rows beyond n zero."""
        B, P, dev = self.B, self.P, self.device
        if self.archive_path == "hip":          # one launch on the dense step-wide buffers: slot c of env b is row b 3P + c
            N, E = candY.shape[2], candS.shape[2]
            cand = (candP.view(B * 3 * P, 4), candY.view(B * 3 * P, N), candS.view(B * 3 * P, E))
            if not final:
                self._merge_archive(*cand, None, 3 * P, accepted=False)
                return None
            fr = RW.archive_merge(self.pts.contiguous(), self.n, self.arch_y.contiguous(), self.arch_sec.contiguous(), *cand, None, n_slots=3 * P,
                                  max_front=0, max_out=4 * P, accepted=False, extras=True, lib=self.lib)
            self.final = dict(points=fr["points"], y=fr["y"], sec=fr["sec"], n=fr["n"], hv=fr["hv_front"], metrics=fr["metrics"])
            return self.final
        arP = self._const("arP", lambda: torch.arange(P, device=dev))
        origp = torch.cat([self.pts, candP], dim=1)
        allp = origp.clone()
        allp[:, :P, 2] = torch.where(arP[None, :] >= self.n[:, None], 2.0, allp[:, :P, 2])   # infeasible marker
        fr = RW.front_hv(allp, self._const("step_rows", lambda: torch.full((B,), 4 * P, dtype=torch.int32, device=dev)), None,
                         max_front=0 if final else P, lib=self.lib)
        rows = self._const("rows", lambda: torch.arange(B, device=dev)[:, None])
        fidx = fr["front_idx"] if final else fr["front_idx"][:, :P]
        fidx = fidx.long()
        take, live = fidx.clamp(min=0), (fidx >= 0)[:, :, None]
        newp = torch.where(live, origp[rows, take], 0.0)
        newp[:, :, 0:2].clamp_(max=1.0)                                                     # :434-436
        newy = torch.where(live, torch.cat([self.arch_y, candY], dim=1)[rows, take], 0.0)
        news = torch.where(live, torch.cat([self.arch_sec, candS], dim=1)[rows, take], 0)
        if final:
            self.final = dict(points=newp, y=newy, sec=news, n=fr["n_front"], hv=fr["hv_front"], metrics=fr["metrics"])
        else:
            self.pts, self.arch_y, self.arch_sec, self.n = newp, newy, news, fr["n_front"]
        return self.final if final else None

    def _merge_archive(self, cand_points, cand_y, cand_sec, slot_row, n_slots, accepted):
        """archive_path="hip": one `truss_archive_merge` launch from the current archive buffers into the spare set, truncated to
        max_front; the two sets then swap roles (the entry refuses to write over its inputs).  Returns accepted [B, n_slots] uint8
        (None unless asked for)."""
        P = self.P
        cur = dict(points=self.pts.contiguous(), y=self.arch_y.contiguous(), sec=self.arch_sec.contiguous(), n=self.n)
        if self._arch_spare is None:
            self._arch_spare = {k: torch.empty_like(v) for k, v in cur.items()}
        res = RW.archive_merge(cur["points"], cur["n"], cur["y"], cur["sec"], cand_points, cand_y, cand_sec, slot_row, n_slots=n_slots,
                               max_front=P, max_out=P, accepted=accepted, out=self._arch_spare, lib=self.lib)
        self.pts, self.arch_y, self.arch_sec, self.n = res["points"], res["y"], res["sec"], res["n"]
        self._arch_spare = cur
        return res.get("accepted")

    def design_episode(self, end_step: int = 500, explore: bool = True):
        """One episode of the design game (game="test") from the state `reset` left: game steps game_step .. end_step, the last
        one ending in the untruncated final cull.  Returns device tensors: hv [T, B] and n_front [T, B] per step (hyperS and
        numHV of master…:662-664; the last row is the final front's), R [B, 3] and G_U [B] summed over the episode (R0..R2, Gr of
        cal_success.py), and final = dict(points, y, sec, n, hv, metrics) (see _design_cull)."""
        if self.game != "test":
            raise ValueError("design_episode plays the design game: build the engine with game='test'")
        T = int(end_step) - self.game_step + 1
        if T < 1:
            raise ValueError(f"end_step {end_step} is before the current game step {self.game_step}")
        B, dev = self.B, self.device
        hv = torch.empty((T, B), dtype=torch.float64, device=dev)
        nf = torch.empty((T, B), dtype=torch.int32, device=dev)
        R = torch.zeros((B, 3), dtype=torch.float64, device=dev)
        G_U = torch.zeros((B,), dtype=torch.float64, device=dev)
        self.end_step = int(end_step)
        try:
            for t in range(T):
                o = self.game_step_all(train=False, explore=explore)
                hv[t], nf[t] = o["hv"], o["n_front"]
                R += o["reward"]
                G_U += o["G_U"]
        finally:
            self.end_step = None
        return dict(hv=hv, n_front=nf, R=R, G_U=G_U, final=self.final)

    def _const(self, name, make):
        """small constant device tensors of the game step (index ranges, fill patterns), made once"""
        c = self.__dict__.setdefault("_consts", {})
        if name not in c:
            c[name] = make()
        return c[name]

    def train_from_replay(self, train_iters: int = 1):
        """`train_iters` MADDPG updates on batches sampled from this engine's replay (when it holds a batch; collective
        decision under data parallelism).  Returns the number of updates run."""
        train = train_iters > 0
        ready = train and self.replay.size >= self.batch_size
        d = getattr(self.rl, "dist", None)
        if train and d is not None and d.is_initialized() and d.get_world_size() > 1:
            # data parallel: every rank plays its own envs and replay; the update is collective
            # (fused gradient all-reduce inside train_on_batch), so all ranks must agree to run it
            flag = torch.tensor([1 if ready else 0], device=self.device)
            d.all_reduce(flag, op=d.ReduceOp.MIN)
            ready = bool(flag.item())
        if ready:
            if not self._synced:
                with torch.no_grad():                                     # materialise lazy layers, then one broadcast
                    S, NS, ag, at, R = self.replay.sample(2, self.gen)
                    A = [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)]
                    st = self._net_state(S)
                    self.rl._ensure_ready(st, [A[0][0], A[0][1], A[1][0], A[1][1], A[2][0], A[2][1]])
                self.rl.sync_parameters()
                self._synced = True
            for _ in range(train_iters):
                S, NS, ag, at, R = self.replay.sample(self.batch_size, self.gen)
                A = [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)]
                self._train(self._net_state(S), [self._net_state(ns) for ns in NS], A, R)
            return train_iters
        return 0


class MixedMARL:
    """The batched rollout over a MIX of truss sizes with ONE set of agents (BASELINE configs[4]; the reference trains one
    MADDPG on a different truss every episode, master…:807-825; its GCN layers do not depend on the node count).

    One `BatchedMARL` engine per size class -- archives, env objects and replay have the class's shapes -- all sharing
    `maddpg`.  Envs are dealt to ranks in buckets like `MixedTrussPool` (pool.deal_buckets): every rank plays the same
    class mix.  A game step plays every class; the updates of the step then draw their batches from the classes'
    replays in turn (a batch is of one class: its tensors have that class's shapes)."""

    def __init__(self, classes, maddpg, *, bucket_envs=64, rank=0, world=1, **engine_kw):
        """engine_kw go to every class's BatchedMARL (game="test": every class brings its own symmetric topology; the coin's env
        field is the env's global id, `global_ids`, where class c's envs are numbered after those of classes 0..c-1)"""
        from .pool import deal_buckets
        self.classes = [(t, int(n)) for t, n in classes]
        self.share = deal_buckets([n for _, n in self.classes], bucket_envs, world)
        self.class_ids, self.ranges, self.engines = [], [], []
        for c, (topo, _) in enumerate(self.classes):
            n_local = sum(hi - lo for lo, hi in self.share[rank][c])
            if n_local:
                self.class_ids.append(c)
                self.ranges.append(self.share[rank][c])
                kw = dict(engine_kw)
                if kw.get("game", "train") == "test":
                    kw["env_ids"] = sum(n for _, n in self.classes[:c]) + self.global_ids(len(self.engines))
                self.engines.append(BatchedMARL(topo, n_local, maddpg, **kw))
        self.rl = maddpg
        self._turn = 0

    def global_ids(self, k):
        return np.concatenate([np.arange(lo, hi) for lo, hi in self.ranges[k]])

    @property
    def env_steps(self):
        return sum(e.env_steps for e in self.engines)

    def reset(self, per_class):
        """per_class[k]: dict(x, target, y_max, d_min, max_def, load_x, load_y, is_roof, y, sec) of this rank's k-th class"""
        for e, b in zip(self.engines, per_class):
            e.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])

    def design_episode(self, end_step: int = 500, explore: bool = True):
        """BatchedMARL.design_episode of every class (game="test"): per_class = their results; hv / n_front [T, B_local] and
        R / G_U concatenated over the classes in engine order"""
        outs = [e.design_episode(end_step=end_step, explore=explore) for e in self.engines]
        cat = lambda k, d: torch.cat([o[k] for o in outs], dim=d)
        return dict(per_class=outs, hv=cat("hv", 1), n_front=cat("n_front", 1), R=cat("R", 0), G_U=cat("G_U", 0))

    def game_step_all(self, train: bool | None = None, explore: bool = True, train_iters: int = 1):
        if train is None:
            train = self.engines[0].game != "test"
        outs = [e.game_step_all(train=train, explore=explore, update=False) for e in self.engines]
        done = 0
        if train:
            for _ in range(train_iters):                       # one class per update, in turn
                for _try in range(len(self.engines)):
                    e = self.engines[self._turn % len(self.engines)]
                    self._turn += 1
                    if e.train_from_replay(1):
                        done += 1
                        break
        return dict(per_class=outs, updates=done, hv=torch.cat([o["hv"] for o in outs]), n_front=torch.cat([o["n_front"] for o in outs]))
