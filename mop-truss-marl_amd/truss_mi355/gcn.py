"""Host glue of the GCN kernels (csrc/truss_gcn*.h) and the inference of the actors on them.

    one layer                gcn_layer / gcn_layer_head / gcn_layer_pool / gcn_layer_group, gcn_aggregate; split_weights
    one level of the update  level_forward / level_backward / level_aggregate (the hooks truss2D_RL._GcnLevel calls)
    an actor, three actors   actor_infer / actors_infer, which both read ONE statement of the network (`_ACTOR_*`)
"""
from __future__ import annotations

import torch

from . import ops
from .pairs import path_graph_table  # noqa: F401  (the table `nbr_p` of the Pareto graph that actor_infer takes)

_ACT_CODE = {None: 0, "relu": 1, "sigmoid": 2}


def _adj(a, expanded=False):
    """an adjacency as the operators take it: contiguous, and [N, N] where one serves the batch (a batch of one; `expanded`: of stride 0 too)"""
    if a is not None and a.dim() == 3 and (a.shape[0] == 1 or (expanded and a.stride(0) == 0)):
        a = a[0]
    return None if a is None else a.contiguous()


COMPACT_ADJ = ("A_s", "A_ts", "A_cs")                      # the actor inputs the compact observation layout covers (A_n, A_p stay dense)


def expand_compact(adj, nbr):
    """compact rows [.., N, Kc] of the table nbr [N, Kc] (the compact observation layout, TRUSS_F_OBS_COMPACT) -> the dense [.., N, N]
    matrix: zeros, and every slot's value at its column.  The unused slots hold +0 and add it to column 0."""
    N, idx = adj.shape[-2], nbr.clamp(min=0).long()
    dense = adj.new_zeros(adj.shape[:-1] + (N,))
    return dense.scatter_add_(-1, idx.expand_as(adj), adj * (nbr >= 0))


def _native_compact(lib):
    """the layer kernels of `lib` read compact adjacencies themselves (adj_layout 1); elsewhere they are expanded on the host"""
    return lib.backend == "hip" and lib.has_obs_compact


def gcn_aggregate(lib, adj, h, bias, act, nbr=None):
    """act(adj @ h + bias) through the fused HIP kernels `truss_gcn_aggregate` / `truss_gcn_aggregate_sparse` (inference only, float32).
    adj [N,N] (shared) or [B,N,N]; h [B,N,C] contiguous; act in {None,'relu','sigmoid'}.
    nbr: int16 [N,K] device table of the columns that can be non-zero in each row of `adj` (TrussTopology.neighbor_table());
    with it, graphs above 32 nodes sum over those K columns only (tools/agg_probe.py: 64 nodes 39 us against 74 us for the
    library's batched GEMM + bias + activation, 256 nodes 42 against 104; at 32 nodes the dense channel-quad kernel is as fast, at 16 faster)."""
    B, N, Cc = h.shape
    sparse = nbr is not None and N > 32 and Cc % 4 == 0 and nbr.shape[1] <= 16
    if N > 64 and not sparse:     # larger graphs without a pattern: a batched N x N x C GEMM (rocBLAS); the fused dense kernels cover N <= 64
        out = torch.matmul(adj, h) + bias
        return torch.relu(out) if act == "relu" else torch.sigmoid(out) if act == "sigmoid" else out
    out = torch.empty_like(h)
    op = ops.namespace().gcn_aggregate_sparse if sparse else ops.namespace().gcn_aggregate
    ops.call(op, ops.bind(lib), ops.stream_of(h.device), _adj(adj), *((nbr,) if sparse else ()), h, bias, out, _ACT_CODE[act])
    return out


def split_weights(lib, w, out=None):
    """w [C <= 224, K] float32 -> int16 [3, 224, KP] (bfloat16 bit patterns, zero padded): the exact three-term split the bf16x3 path
    of the fused layer kernel reads (`truss_gcn_split_w`; one small launch).  `layer_split_weights` caches it per GCN layer.
    out: an existing image of that shape to write (in place: capturable, its address stays)."""
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


def _split_image(lib, x, w, nbr, precision, w_split):
    """the split image of `w` that the layer reads under `precision` (the caller's `w_split`, else a new one), or None where the layer
    runs on the float32 matrix cores"""
    if precision == "f32" or not _bf16_envelope(x, w, nbr):
        return None
    return w_split if w_split is not None else split_weights(lib, w)


def _layout(lib, adj, nbr, compact):
    """(adj, adj_layout) as the operators take a layer's adjacency: a compact one as it is where the kernels read it, else expanded"""
    if not compact:
        return adj, 0
    if nbr is None:
        raise ValueError("a compact adjacency needs its neighbour table (nbr)")
    return (adj, 1) if _native_compact(lib) else (expand_compact(adj, nbr), 0)


def _launch_layer(lib, x, adj, w, bias, act, nbr, precision, w_split, out, accumulate=False, kind=0, w2=None, bias2=None, adj2=None,
                  nbr2=None, act2=None, out2=None, pool=None, compact=False):
    """one layer launch: `truss_gcn_layer` (kind 0) or `truss_gcn_layer_fused` (kind 1: head epilogue, 2: pool epilogue) under
    "bf16x3" / "f32"; `truss_gcn_layer_terms`, which takes both, under "bf16x2" / "bf16" inside the split-weight envelope.
    compact: adj holds the [.., N, Kn] rows of `nbr` (adj_layout 1 of the C ABI); adj2 is always dense"""
    _check_precision(precision)
    ws = _split_image(lib, x, w, nbr, precision, w_split)
    adj, layout = _layout(lib, adj, nbr, compact)
    ns, layer = ops.namespace(), (ops.bind(lib), ops.stream_of(x.device), x, _adj(adj), nbr, w, bias, out, _ACT_CODE[act])
    epilogue = (kind, w2, bias2, _adj(adj2), nbr2, _ACT_CODE[act2], out2, pool)
    if ws is not None and precision != "bf16x3":
        ops.call(ns.gcn_layer_terms, *layer, ws, *epilogue, bool(accumulate), _BF16_TERMS[precision], layout)
    elif kind:
        ops.call(ns.gcn_layer_fused, *layer, ws, *epilogue, layout)
    else:
        ops.call(ns.gcn_layer, *layer, bool(accumulate), ws, layout)


def gcn_layer(lib, x, adj, w, bias, act, nbr=None, out=None, accumulate=False, precision="bf16x3", w_split=None, compact=False):
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
    w_split: split_weights(lib, w) if the caller keeps it (one image serves all precisions).
    compact: adj is [N,Kn] / [B,N,Kn], the rows of the compact observation layout through `nbr` (required then): term t of row i is
    adj[i, t], its source row nbr[i, t] -- the same coefficients in the same order, so the result is bit for bit that of the dense
    call.  A library whose kernels do not read that layout gets the adjacency expanded to dense first (`expand_compact`)."""
    if out is None:
        assert not accumulate
        out = torch.empty((x.shape[0], x.shape[1], w.shape[0]), dtype=torch.float32, device=x.device)
    _launch_layer(lib, x, adj, w, bias, act, nbr, precision, w_split, out, accumulate, compact=compact)
    return out


def _gcn_layer_fused(lib, x, adj, w, bias, act, nbr, precision, w_split, out, kind, w2=None, bias2=None, adj2=None, nbr2=None, act2=None,
                     out2=None, pool=None, compact=False):
    """`truss_gcn_layer_fused`: the layer of `gcn_layer` with a consumer of its output in the epilogue of the same launch
    (precision "bf16x2" / "bf16", inside the split-weight envelope: `truss_gcn_layer_terms` with the same epilogue)"""
    _launch_layer(lib, x, adj, w, bias, act, nbr, precision, w_split, out, False, kind, w2, bias2, adj2, nbr2, act2, out2, pool, compact)


def gcn_layer_head(lib, x, adj, w, bias, act, w2, bias2, adj2, act2, nbr=None, nbr2=None, precision="bf16x3", w_split=None, out=None,
                   compact=False):
    """A hidden GCN layer and the narrow layer that consumes it in ONE launch (`truss_gcn_layer_fused`, head epilogue):
    act2(adj2 @ (V @ w2.T) + bias2) [B, N, c2] with V = act(adj @ (x @ w.T) + bias) as `gcn_layer` computes it -- V goes from the
    accumulators through LDS into the head and is written to HBM only if `out` [B, N, C] is given.  w2 [c2 <= 8, C] =
    nn.Linear.weight of the head; adj2 / nbr2: the head's own adjacency and pattern (as adj / nbr); the rest as for `gcn_layer`
    (compact: the layout of adj only -- adj2 is dense)."""
    out2 = torch.empty((x.shape[0], x.shape[1], w2.shape[0]), dtype=torch.float32, device=x.device)
    _gcn_layer_fused(lib, x, adj, w, bias, act, nbr, precision, w_split, out, 1, w2, bias2, adj2, nbr2, act2, out2=out2, compact=compact)
    return out2


def gcn_layer_pool(lib, x, adj, w, bias, act, nbr=None, precision="bf16x3", w_split=None, out=None):
    """A GCN layer and the sum of its output over the nodes of every graph in ONE launch (`truss_gcn_layer_fused`, pool epilogue):
    act(adj @ (x @ w.T) + bias).sum(dim=1) [B, C], every one of the N rows counted; the layer's output itself is written to HBM
    only if `out` [B, N, C] is given.  Arguments as for `gcn_layer`."""
    pool = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
    _gcn_layer_fused(lib, x, adj, w, bias, act, nbr, precision, w_split, out, 2, pool=pool)
    return pool


GROUP_MAX_STEPS, GROUP_MAX_EPI = 16, 8                      # TRUSS_GCN_GROUP_MAX_STEPS / _EPI (include/truss_mi355.h)


def gcn_layer_group(lib, chains, precision="bf16x3", epilogues=None):
    """Several split-weight GCN layers in ONE launch (`truss_gcn_layer_group`, csrc/truss_gcn_group.h): the same bits as running them
    one by one through `gcn_layer` / `gcn_layer_head` / `gcn_layer_pool` in chain order.
    chains: a list of chains of equal length; a chain is a list of steps that write the same `out`, a step a dict with the arguments of
    `gcn_layer` by name: x, adj, w, bias, act, out, w_split (required: `split_weights(lib, w)`), and optionally nbr, accumulate,
    compact (the step's adj holds the compact rows of its nbr).
    Chains must not depend on each other; a step must not read the chain's `out`.  All layers share B, N and table-or-dense.
    epilogues: None, or one dict per chain (chains of one step; out may then be None): kind "head" with w2, bias2, adj2, act2, out2
    and optionally nbr2, or kind "pool" with pool -- all of one kind.
    precision: "bf16x3", "bf16x2" or "bf16" (this entry is the split-weight path only: no "f32", and a layer outside the
    split-weight envelope is refused by the library, not rerouted).  At most 16 plain layers, or 8 chains with epilogues."""
    _check_precision(precision)
    if precision == "f32":
        raise ValueError("gcn_layer_group is the split-weight path: precision must be 'bf16x3', 'bf16x2' or 'bf16'")
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
        epi = [ecol("w2"), ecol("bias2"), [_adj(a) for a in ecol("adj2")], ecol("nbr2"), [_ACT_CODE[e.get("act2")] for e in epilogues],
               ecol("out2"), ecol("pool")]
    device = steps[0]["x"].device if steps else torch.device("cpu")
    laid = [_layout(lib, s["adj"], s.get("nbr"), s.get("compact", False)) for s in steps]
    ops.call(ops.namespace().gcn_layer_group, ops.bind(lib), ops.stream_of(device), col("x"), [_adj(a) for a, _ in laid], col("nbr"),
             col("w"), col("bias"), col("out"), [_ACT_CODE[s["act"]] for s in steps], [bool(s.get("accumulate", False)) for s in steps],
             col("w_split"), per_chain, kind, *epi, _BF16_TERMS[precision], [l for _, l in laid] if any(l for _, l in laid) else [])


def level_forward(lib):
    """The fused forward of a whole level of GCN layers (`truss_gcn_level`, csrc/truss_gcn_level.h: one launch for every layer of
    every group) in the shape truss2D_RL._GcnLevel asks for: callable(groups, xs, ws, bs, want_grad) -> ([out_g [n, B, N, C]],
    [X'_g [n, B N, K] or None]), or None when a shape is outside the kernel's envelope (the caller then evaluates the level with
    batched library GEMMs).  Installed by BatchedMARL on the GPU (`truss2D_RL.set_level_forward`)."""

    def run(groups, xs, ws, bs, want_grad):
        X, ADJ, W, BIAS, OUT, XAGG, ACT, outs, xaggs = [], [], [], [], [], [], [], [], []
        for g in groups:
            n, (B, N, K), C = len(g.idx), g.shape, ws[g.idx[0]].shape[0]
            if N > 64 or C > 224 or K > 256 or xs[g.idx[0]].dtype != torch.float32:      # outside the kernel's envelope
                return None
            o = torch.empty((n, B, N, C), dtype=torch.float32, device=xs[g.idx[0]].device)
            xa = torch.empty((n, B * N, K), dtype=torch.float32, device=o.device) if want_grad else None
            for j, i in enumerate(g.idx):
                X.append(xs[i].detach().contiguous())
                ADJ.append(_adj(g.adjs[j], expanded=True))
                W.append(ws[i].detach())
                BIAS.append(bs[i].detach())
                OUT.append(o[j])
                if want_grad:
                    XAGG.append(xa[j])
                ACT.append(_ACT_CODE[g.act])
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
                ADJ.append(_adj(g.adjs[j], expanded=True))
                W.append(ws[i].detach())
                ACT.append(_ACT_CODE[g.act])
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


def level_aggregate(lib):
    """The neighbour sums of the pattern groups of a level (`truss_gcn_level_aggregate`, csrc/truss_gcn_level_agg.h: ONE call for every
    layer of every group of a level and direction) in the shape truss2D_RL._aggregate asks for: callable(groups, xs, transpose) ->
    [y_g [n, B N, K]], one stacked tensor per group whose slices the launch writes, or None for anything but float32 (the caller
    then gathers and sums with framework operators).  Installed by BatchedMARL(level_adjacency="table") on the GPU
    (`truss2D_RL.set_level_aggregate`)."""

    def run(groups, xs, transpose):
        X, ADJ, NBR, Y, ys = [], [], [], [], []
        for g, xg in zip(groups, xs):
            n, (B, N, K), dev = len(g.idx), g.shape, xg[0].device
            if any(x.dtype != torch.float32 for x in xg) or any(a.dtype != torch.float32 for a in g.adjs):
                return None
            nbr = g.pattern.on(dev)
            y = torch.empty((n, B * N, K), dtype=torch.float32, device=dev)
            for j, x in enumerate(xg):
                X.append(x.detach().contiguous())
                ADJ.append(_adj(g.adjs[j], expanded=True))
                NBR.append(nbr)
                Y.append(y[j].view(x.shape))                # (x is [B, N, K] forward, [B N, K] backward: the operator wants equal shapes)
            ys.append(y)
        ops.call(ops.namespace().gcn_level_aggregate, ops.bind(lib), ops.stream_of(X[0].device), X, ADJ, NBR, Y, [bool(transpose)] * len(X))
        return ys
    return run


def gcn_layer_supported(n_nodes, c_out, nbr):
    """shapes the fused layer kernel takes (include/truss_mi355.h); anything else goes through library GEMM + aggregation kernels"""
    return c_out <= 224 and n_nodes <= 256 and ((nbr is not None and nbr.shape[1] <= 16) or (nbr is None and n_nodes <= 64))


# ---- the actor: truss2D_RL.multimodes_actor.forward (truss2D_RL.py:49-120), stated once ----
_ACTOR_INPUTS = ("x_n", "A_n", "A_s", "A_ts", "A_cs", "x_p", "A_p")         # the order of the network's input list
# depth 1 (layer, input, adjacency), relu: three layers over the node graph, and gcn_l1_4 over the Pareto graph, whose output is summed
# over the front's members (GlobalSumPool) and tiled over the nodes (`_tile_pool`)
_ACTOR_FIRST = (("gcn_l1_1", "x_n", "A_n"), ("gcn_l1_2", "x_n", "A_n"), ("gcn_l1_3", "x_n", "A_n"), ("gcn_l1_4", "x_p", "A_p"))
# depth 2 (layer, the depth-1 layer it reads, adjacency), relu: x3 = their sum, accumulated in this order
_ACTOR_SECOND = (("gcn_l2_1", "gcn_l1_1", "A_n"), ("gcn_l2_2", "gcn_l1_2", "A_ts"), ("gcn_l2_3", "gcn_l1_2", "A_cs"),
                 ("gcn_l2_4", "gcn_l1_3", "A_s"), ("gcn_l2_5", "gcn_l1_4", "A_n"))
# depths 3 + 4 (layer, head, adjacency, head adjacency): relu layers that read x3, each feeding its sigmoid action head
_ACTOR_HEADS = (("gcn_l3_1", "gcn_l4_1", "A_n", "A_n"), ("gcn_l3_2", "gcn_l4_2", "A_s", "A_n"))


def _tile_pool(pooled, n_nodes):
    """truss2D_RL._tile_pool (:87-93) on the last axis: [..., H] -> N copies stacked behind it -> reshaped (not transposed) to [..., N, H]"""
    lead, H = pooled.shape[:-1], pooled.shape[-1]
    return pooled.unsqueeze(-1).expand(*lead, H, n_nodes).reshape(*lead, n_nodes, H)


def _materialise(actor, t):
    """let the lazy layers of `actor` materialise themselves, in the order of the module's forward (weight initialisation consumes the
    global generator in that order); a layer's input matters by its width only.  t: the network's inputs by name."""
    width = lambda src: t[src].shape[2] if src in t else getattr(actor, src).lin.weight.shape[0]
    for name, src, adj in (_ACTOR_FIRST + _ACTOR_SECOND + tuple((layer, _ACTOR_SECOND[0][0], adj) for layer, _, adj, _ in _ACTOR_HEADS)
                           + tuple((head, layer, adj2) for layer, head, _, adj2 in _ACTOR_HEADS)):
        layer, a = getattr(actor, name), t[adj]
        if isinstance(layer.lin.weight, torch.nn.parameter.UninitializedParameter):
            n = a.shape[-2]                                  # (a compact adjacency [.., N, Kc] stands in as an empty [1, N, N])
            with torch.no_grad():
                layer(a.new_zeros((1, n, width(src))), (a[:1] if a.dim() == 3 else a) if a.shape[-1] == n else a.new_zeros((1, n, n)))


def actor_infer(lib, actor, ins, nbr=None, nbr_p=None, fused=False, precision="bf16x3", compact=False):
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
    split weights (`layer_split_weights`) are the same for all of them.
    compact: A_s, A_ts and A_cs of `ins` are [B, N, Kc] rows of the compact observation layout through `nbr` (A_n and A_p stay
    dense): the layers over them read the rows as they are (`gcn_layer(compact=True)`), bit for bit the dense result; a layer outside
    `gcn_layer_supported` gets the dense matrix back first (`expand_compact`) and takes the fallback it always took."""
    return _actors_forward(lib, [actor], ins, nbr, nbr_p, fused, precision, group=False, compact=compact)[0]


def actors_infer(lib, actors, ins, nbr=None, nbr_p=None, precision="bf16x3", compact=False):
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
    those of `layer_split_weights`.  compact: as for `actor_infer`."""
    return _actors_forward(lib, actors, ins, nbr, nbr_p, True, precision, group=True, compact=compact)


def _actors_forward(lib, actors, ins, nbr, nbr_p, fused, precision, group, compact=False):
    """the walk of `actor_infer` / `actors_infer` over `_ACTOR_*`, depth by depth: with `group`, a depth whose layers are all inside
    the envelope of `gcn_layer_group` is one launch of it for all actors; otherwise the depth runs layer by layer"""
    _check_precision(precision)
    A = len(actors)
    if A == 0:
        return []
    t = dict(zip(_ACTOR_INPUTS, ins))
    for a in actors:
        _materialise(a, t)
    B, N, dev = t["x_n"].shape[0], t["x_n"].shape[1], t["x_n"].device
    if t["x_n"].shape[2] % 4 and gcn_layer_supported(N, 200, nbr):
        # 13 node features -> 16 (zero columns, matched by zero columns of the three input kernels): 16-byte loads, bf16x3 product
        t["x_n"] = torch.nn.functional.pad(t["x_n"], (0, 4 - t["x_n"].shape[2] % 4))      # once for all actors
    t["x_n"], t["x_p"] = t["x_n"].contiguous(), t["x_p"].contiguous()
    pat = lambda adj: nbr_p if adj == "A_p" else nbr
    group = group and lib.has_gcn_group and precision != "f32"
    if compact and nbr is None:
        raise ValueError("compact adjacencies need the neighbour table (nbr)")
    cmp = lambda adj: bool(compact) and adj in COMPACT_ADJ       # this input holds compact rows
    layout = lambda adj: {"compact": True} if cmp(adj) else {}   # (a dense layer is called as it always was)
    dense = {}                                                   # ... and its dense form, where a fallback needs it (once per input)

    def as_dense(adj):
        if not cmp(adj):
            return t[adj]
        if adj not in dense:
            dense[adj] = expand_compact(t[adj], nbr)
        return dense[adj]

    def g(layer, x, adj, act="relu", out=None, accumulate=False):
        w, x = layer.lin.weight, x.contiguous()
        if gcn_layer_supported(x.shape[1], w.shape[0], pat(adj)):
            wd, ws = layer_split_weights(lib, layer, x.shape[2])     # (x_n arrives zero-padded to 16 features)
            return gcn_layer(lib, x, t[adj], wd, layer.bias.detach(), act, pat(adj), out, accumulate, precision=precision, w_split=ws,
                             **layout(adj))
        h = gcn_aggregate(lib, as_dense(adj), torch.nn.functional.linear(x, w).contiguous(), layer.bias, act, pat(adj))
        if out is None:
            return h
        return out.add_(h) if accumulate else out.copy_(h)

    def g_pool(layer, x, adj):                              # g(layer, x, adj).sum(dim=1) without the [B, P, H] tensor
        if not (fused and gcn_layer_supported(x.shape[1], layer.lin.weight.shape[0], pat(adj))):
            return g(layer, x, adj).sum(dim=1)
        wd, ws = layer_split_weights(lib, layer, x.shape[2])
        return gcn_layer_pool(lib, x, as_dense(adj), wd, layer.bias.detach(), "relu", pat(adj), precision=precision, w_split=ws)

    def g_head(layer, head, x, adj, adj2):                  # g(head, g(layer, x, adj), adj2, "sigmoid") without the hidden tensor
        w2 = head.lin.weight
        if not (fused and w2.shape[0] <= 8 and gcn_layer_supported(x.shape[1], layer.lin.weight.shape[0], pat(adj))
                and gcn_layer_supported(x.shape[1], w2.shape[0], pat(adj2))):
            return g(head, g(layer, x, adj), adj2, "sigmoid")
        wd, ws = layer_split_weights(lib, layer, x.shape[2])
        return gcn_layer_head(lib, x, t[adj], wd, layer.bias.detach(), "relu", w2.detach(), head.bias.detach(), as_dense(adj2), "sigmoid",
                              pat(adj), pat(adj2), precision=precision, w_split=ws, **layout(adj))

    def step(layer, x, adj, out=None, accumulate=False):
        """the layer as a step of `gcn_layer_group`, or None outside the envelope of the grouped launch"""
        if not gcn_layer_supported(x.shape[1], layer.lin.weight.shape[0], pat(adj)):
            return None
        wd, ws = layer_split_weights(lib, layer, x.shape[2])
        if ws is None or not _bf16_envelope(x, wd, pat(adj)):
            return None
        return dict(x=x, adj=t[adj], nbr=pat(adj), w=wd, bias=layer.bias.detach(), act="relu", out=out, accumulate=accumulate, w_split=ws,
                    compact=cmp(adj))

    def grouped(steps):                                     # the steps if all are inside the envelope and of one width, else None
        ok = group and all(s is not None for s in steps) and len({s["w"].shape[0] for s in steps}) == 1
        return steps if ok else None

    def launch(chains, epilogues, limit):                   # one launch, or one per `limit` chains where the actors are many
        for i in range(0, len(chains), limit):
            gcn_layer_group(lib, chains[i:i + limit], precision, None if epilogues is None else epilogues[i:i + limit])

    def outputs(n, shape):
        return list(torch.empty((n,) + tuple(shape), dtype=torch.float32, device=dev).unbind(0))

    # depth 1, node graph
    nodes, (pooled_layer, px, padj) = _ACTOR_FIRST[:3], _ACTOR_FIRST[3]
    steps = grouped([step(getattr(a, name), t[x], adj) for a in actors for name, x, adj in nodes] if group else [None])
    if steps is not None:
        for s, o in zip(steps, outputs(len(steps), (B, N, steps[0]["w"].shape[0]))):
            s["out"] = o
        launch([[s] for s in steps], None, GROUP_MAX_STEPS)
        outs = [s["out"] for s in steps]
    else:
        outs = [g(getattr(a, name), t[x], adj) for a in actors for name, x, adj in nodes]
    h = [{name: outs[len(nodes) * i + j] for j, (name, _, _) in enumerate(nodes)} for i in range(A)]   # per actor: layer -> its output
    # depth 1, Pareto graph
    steps = grouped([step(getattr(a, pooled_layer), t[px], padj) for a in actors] if group else [None])
    if steps is not None:
        pooled = torch.empty((A, B, steps[0]["w"].shape[0]), dtype=torch.float32, device=dev)
        launch([[s] for s in steps], [dict(kind="pool", pool=pooled[i]) for i in range(A)], GROUP_MAX_EPI)
        tiled = _tile_pool(pooled, N).unbind(0)                                             # one copy for all actors
    else:
        tiled = [_tile_pool(g_pool(getattr(a, pooled_layer), t[px], padj), N).contiguous() for a in actors]
    for i in range(A):
        h[i][pooled_layer] = tiled[i]
    # depth 2: the layers of an actor add into its x3, a chain
    chains = None
    if group and len({getattr(a, _ACTOR_SECOND[0][0]).lin.weight.shape[0] for a in actors}) == 1:
        x3 = outputs(A, (B, N, getattr(actors[0], _ACTOR_SECOND[0][0]).lin.weight.shape[0]))
        chains = [[step(getattr(a, name), h[i][src].contiguous(), adj, x3[i], j > 0) for j, (name, src, adj) in enumerate(_ACTOR_SECOND)]
                  for i, a in enumerate(actors)]
        if not all(s is not None and s["w"].shape[0] == s["out"].shape[2] for chain in chains for s in chain):
            chains = None
    if chains is not None:
        launch(chains, None, GROUP_MAX_STEPS // len(_ACTOR_SECOND))
    else:
        x3 = []
        for i, a in enumerate(actors):
            out = None
            for j, (name, src, adj) in enumerate(_ACTOR_SECOND):
                out = g(getattr(a, name), h[i][src], adj, out=out, accumulate=j > 0)
            x3.append(out)
    # depths 3 + 4
    pairs = [(getattr(a, layer), getattr(a, head), adj, adj2, x3[i]) for i, a in enumerate(actors) for layer, head, adj, adj2 in _ACTOR_HEADS]
    steps = [step(layer, x, adj) for layer, _, adj, _, x in pairs] if group else [None]
    if all(s is not None for s in steps) and all(head.lin.weight.shape[0] <= 8 and gcn_layer_supported(N, head.lin.weight.shape[0], pat(adj2))
                                                  for _, head, _, adj2, _ in pairs):
        epis = [dict(kind="head", w2=head.lin.weight.detach(), bias2=head.bias.detach(), adj2=as_dense(adj2), nbr2=pat(adj2), act2="sigmoid",
                     out2=torch.empty((B, N, head.lin.weight.shape[0]), dtype=torch.float32, device=dev)) for _, head, _, adj2, _ in pairs]
        launch([[s] for s in steps], epis, GROUP_MAX_EPI)
        heads = [e["out2"] for e in epis]
    else:
        heads = [g_head(layer, head, x, adj, adj2) for layer, head, adj, adj2, x in pairs]
    return [tuple(heads[len(_ACTOR_HEADS) * i:len(_ACTOR_HEADS) * (i + 1)]) for i in range(A)]
