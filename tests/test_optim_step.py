"""`truss_optim_step` (csrc/truss_optim.h): the per-tensor gradient clip and Adam of the MADDPG update as one native call -- the C
entry, `torch.ops.truss_mi355.optim_step`, the hook `truss2D_RL.set_optimizer_step` / `truss_mi355.optim.optimizer_step` and
BatchedMARL(optimizer_path="hip") -- against a float64 model of the arithmetic the header states, stage by stage.

Bounds (derived, not measured; u = 2^-24, first order in u):
  clip      c = g * min(1, 1 / (norm + 1e-12)) with norm = (float) sqrt(sum g^2 in float64): norm's rounding to float32 u, + 1e-12f one
            more, the reciprocal 2 u (as `_adam_bounds` of tests/test_update_float64.py counts a device reciprocal), the product u; one
            to spare.  The float64 sum of exact squares contributes nothing at this order:          |c - c64| <= 6 u |c64|
  moments and weights, from the kernel's OWN clipped gradient (its `clipped` output): the bounds of tests/test_update_float64.py
  (`_adam_bounds`, `_fresh_bound`), restated:
            |dm'| <= u (|m'| + 3 (1 - b1) |c - m|)      |dv'| <= 4 u v'      |dw'| <= u (|w'| + 15 |dw| + 3 T)
            with T = (lr / bc1) (1 - b1) |c - m| / (sqrt(v') / sqrt(bc2) + eps);    the fresh Adam's first step: |dw'| <= u (|w'| + 7 |dw|)
Shared inputs: tensors of 1, 3, 7, 200, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 5 and 40 000 elements (below, at and
above a workgroup's 256 threads and its chunk, more than one chunk, ten chunks), gradients scaled per tensor to norms 3, 0.3 and 1 in
rotation (clipped, not clipped, at the threshold), a run of exact zeros in one tensor (where the second moment is zero too: the
only place eps decides the step), t in {1, 2, 1000} with zero moments at t = 1, lr in {1e-3, 1e-7}, eps 1e-8 (Adam) / 1e-7 (first step).
"""
import contextlib
import copy
import ctypes as C
import io
import math

import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import _lib, marl, ops, optim, synthetic
import master_DDPG_truss2D_MO as M
import parity_common as pc
import truss2D_RL as RL
import update_reference as UR

U = 2.0 ** -24
B1, B2 = 0.9, 0.999
CHUNK = _lib.OPTIM_CHUNK
SIZES = [1, 3, 7, 200, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 40000]
ZERO_TENSOR, ZERO_RUN = SIZES.index(2 * CHUNK + 5), slice(4000, 4300)        # the zeros straddle the tensor's first chunk boundary
ADAM_CASES = [(t, lr, 1e-8) for t in (1, 2, 1000) for lr in (1e-3, 1e-7)]
FIRST_CASES = [(None, lr, 1e-7) for lr in (1e-3, 1e-7)]
MUTANTS = ("no clip", "one clip for the whole vector", "sign", "eps x 10", "bias correction frozen at t = 1",
           "sqrt missing from the second correction", "lr x 10 on the first step")
f64 = lambda t: t.detach().double().cpu()


# ---- the inputs, the float64 model and its bounds, the float32 restatement ------------------------------------------------------------

_INPUTS = {}


def _inputs(sizes=tuple(SIZES)):
    """-> dict(sizes, g [per tensor], w, m, v [flat]) float32 on the CPU, made once; m and v are the moments of the t > 1 cases"""
    if sizes not in _INPUTS:
        gen = torch.Generator().manual_seed(7)
        gs = []
        for i, n in enumerate(sizes):
            x = torch.randn(n, generator=gen, dtype=torch.float64)
            if sizes == tuple(SIZES) and i == ZERO_TENSOR:
                x[ZERO_RUN] = 0.0
            gs.append((x * ((3.0, 0.3, 1.0)[i % 3] / float(x.norm()))).float())
        total = sum(sizes)
        w = (0.1 * torch.randn(total, generator=gen)).float()
        m = (0.01 * torch.randn(total, generator=gen)).float()
        v = (1e-4 * torch.rand(total, generator=gen)).float()
        if sizes == tuple(SIZES):
            o = sum(sizes[:ZERO_TENSOR])
            v[o + ZERO_RUN.start:o + ZERO_RUN.stop] = 0.0
        _INPUTS[sizes] = dict(sizes=list(sizes), g=gs, w=w, m=m, v=v)
    return _INPUTS[sizes]


def _moments(inp, t):
    z = torch.zeros_like(inp["m"])
    return (z, z.clone()) if t in (None, 1) else (inp["m"], inp["v"])


def _clip64(gs, mutant=None):
    """float32 gradient tensors -> (float64 clipped tensors, float64 norms)"""
    gs = [f64(g) for g in gs]
    norms = [float(g.norm()) for g in gs]
    if mutant == "no clip":
        return gs, norms
    if mutant == "one clip for the whole vector":
        f = min(1.0, 1.0 / (math.sqrt(sum(n * n for n in norms)) + 1e-12))
        return [g * f for g in gs], norms
    return [g * min(1.0, 1.0 / (n + 1e-12)) for g, n in zip(gs, norms)], norms


def _adam64(w, m, v, c, t, lr, eps, mutant=None):
    """float64 flat vectors -> (w', m', v', dw)"""
    m2 = m + (1.0 - B1) * (c - m)
    v2 = v * B2 + (1.0 - B2) * c * c
    tc = 1 if mutant == "bias correction frozen at t = 1" else t
    bc2 = 1.0 - B2 ** tc
    corr = bc2 if mutant == "sqrt missing from the second correction" else math.sqrt(bc2)
    dw = -lr / (1.0 - B1 ** tc) * m2 / (v2.sqrt() / corr + (10.0 * eps if mutant == "eps x 10" else eps))
    if mutant == "sign":
        dw = -dw
    return w + dw, m2, v2, dw


def _fresh64(w, c, lr, eps, mutant=None):
    dw = -(10.0 * lr if mutant == "lr x 10 on the first step" else lr) * c / (c.abs() + (10.0 * eps if mutant == "eps x 10" else eps))
    if mutant == "sign":
        dw = -dw
    return w + dw, dw


def _adam_bounds(w, m, v, c, t, lr, eps):
    w2, m2, v2, dw = _adam64(w, m, v, c, t, lr, eps)
    lead = (1.0 - B1) * (c - m).abs()
    T = lr / (1.0 - B1 ** t) * lead / (v2.sqrt() / math.sqrt(1.0 - B2 ** t) + eps)
    return {"w": U * (w2.abs() + 15.0 * dw.abs() + 3.0 * T), "m": U * (m2.abs() + 3.0 * lead), "v": 4.0 * U * v2}


def _fresh_bound(w, c, lr, eps):
    w2, dw = _fresh64(w, c, lr, eps)
    return U * (w2.abs() + 7.0 * dw.abs())


def _worst(err, bound):
    """max err / bound (an element whose bound is 0 must be exact)"""
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _figures(gs, w, m, v, t, lr, eps, got, mutant=None):
    """error / bound of every stage of one step: got = dict(c [flat], w, and for Adam m, v) float32 results, the moments and weights
    against the float64 step from got's OWN clipped gradient.  mutant: the float64 model is the broken one, the bounds stay those
    of the correct arithmetic."""
    c64 = torch.cat(_clip64(gs, mutant)[0])
    good = torch.cat(_clip64(gs)[0])
    fig = {"clip": _worst((f64(got["c"]) - c64).abs(), 6.0 * U * good.abs())}
    c, w_, m_, v_ = f64(got["c"]), f64(w), f64(m), f64(v)
    if t is None:
        w2, _ = _fresh64(w_, c, lr, eps, mutant)
        fig["fresh"] = _worst((f64(got["w"]) - w2).abs(), _fresh_bound(w_, c, lr, eps))
    else:
        w2, m2, v2, _ = _adam64(w_, m_, v_, c, t, lr, eps, mutant)
        bound = _adam_bounds(w_, m_, v_, c, t, lr, eps)
        for q, want in (("w", w2), ("m", m2), ("v", v2)):
            fig[q] = _worst((f64(got[q]) - want).abs(), bound[q])
    return fig


def restatement(params, flat_grad, lr, eps, betas=None, step=None, exp_avg=None, exp_avg_sq=None, clipped=None):
    """the kernels' arithmetic in float32 torch operations (one rounding each, nothing fused), with the contract of a
    `set_optimizer_step` hook: params and the moments are updated in place, flat_grad is left alone"""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=flat_grad.device)
    with torch.no_grad():
        sizes = [p.numel() for p in params]
        c = torch.empty_like(flat_grad)
        for g, o in zip(flat_grad.split(sizes), c.split(sizes)):
            norm = g.double().pow(2).sum().sqrt().float()
            torch.mul(g, torch.minimum(f32(1.0), f32(1.0) / (norm + f32(1e-12))), out=o)
        if clipped is not None:
            clipped.copy_(c)
        if step is None:
            upd = f32(-lr) * (c / (c.abs() + f32(eps)))
        else:
            b1, b2 = betas
            t, m, v = float(step), exp_avg, exp_avg_sq
            m.copy_(m + f32(1.0 - b1) * (c - m))
            v.copy_(v * f32(b2) + (f32(1.0 - b2) * c) * c)
            den = v.sqrt() / f32(math.sqrt(1.0 - b2 ** t)) + f32(eps)
            upd = ((f32(1.0) / den) * m) * f32(-lr / (1.0 - b1 ** t))
        for p, u_ in zip(params, upd.split(sizes)):
            p.copy_(p + u_.view_as(p))


def _run_restatement(inp, t, lr, eps):
    m, v = (x.clone() for x in _moments(inp, t))
    ps = [x.clone() for x in inp["w"].split(inp["sizes"])]
    c = torch.empty_like(inp["w"])
    restatement(ps, torch.cat(inp["g"]), lr, eps, betas=(B1, B2), step=None if t is None else torch.tensor(float(t), dtype=torch.float64),
                exp_avg=m, exp_avg_sq=v, clipped=c)
    return dict(c=c, w=torch.cat(ps), m=m, v=v)


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------

def test_restatement_stays_inside_the_bounds_and_mutants_do_not():
    """the float32 restatement of the kernels' arithmetic (the CPU hook of the next test) against the float64 model on the shared
    inputs: every stage of every case inside its bound; every mutant of the float64 model at least 10 x outside on at least one case
    (not on all: eps x 10 shows only where v' is zero, the frozen correction not at t = 1).
    Largest error / bound measured on the CPU: clip 0.22, w 1.00, m 0.99, v 0.68, fresh 0.99 (half an ulp of the result is the
    leading term of the w, m and fresh bounds)."""
    inp = _inputs()
    runs = [(case, _run_restatement(inp, *case)) for case in ADAM_CASES + FIRST_CASES]
    worst = {}
    for (t, lr, eps), got in runs:
        m, v = _moments(inp, t)
        for q, r in _figures(inp["g"], inp["w"], m, v, t, lr, eps, got).items():
            worst[q] = max(worst.get(q, 0.0), r)
            assert r <= 1.0, f"t={t} lr={lr}: {q} at {r:.3g} of its bound"
    print("\n[restatement against float64] largest error / bound: " + ", ".join(f"{q} {r:.3g}" for q, r in worst.items()))
    assert set(worst) == {"clip", "w", "m", "v", "fresh"}
    for mutant in MUTANTS:
        far = 0.0
        for (t, lr, eps), got in runs:
            m, v = _moments(inp, t)
            far = max(far, max(_figures(inp["g"], inp["w"], m, v, t, lr, eps, got, mutant).values()))
        print(f"[mutant '{mutant}'] largest error / bound over the cases: {far:.3g}")
        assert far >= 10.0, f"mutant '{mutant}' stays within 10 x the bounds on every case"


def _batch(seed, B, N, P, device):
    """a minibatch (S, NS, A, R) as tests/test_update_float64._batch builds it (one shared adjacency and mask)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g).to(device)
    A = lambda n: torch.softmax(torch.randn(B, n, n, generator=g), -1).to(device)
    a_n, mask = A(N)[:1].expand(B, -1, -1), torch.ones(1, N, N).to(device).expand(B, -1, -1)
    state = lambda: [r(B, N, 13), a_n, A(N), A(N), A(N), mask, r(B, P, 4), A(P)]
    return state(), [state() for _ in range(3)], [(r(B, N, 2), r(B, N, 3)) for _ in range(3)], r(B, 3)


def _maddpg(device, lr=1e-4, B=5, N=12, P=20, H=40, C=8):
    torch.manual_seed(5)
    rl = RL.MADDPG(lr, M.ep, M.epd, M.gamma, H, C, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)
    batches = [_batch(20 + k, B, N, P, device) for k in range(3)]
    S, NS, A, R = batches[0]
    rl._ensure_ready(S, [t for a in A for t in a])
    return rl, batches


def _weights(rl):
    return [p for ag in rl.agents for net in (ag.actor_model, ag.critic_model) for p in net.parameters()]


def test_the_hook_is_what_the_update_runs(monkeypatch):
    """`set_optimizer_step(restatement, "cpu")`: three `train_on_batch` calls at (B, N, P, H) = (5, 12, 20, 40) call the hook four
    times each -- the three critics' parameters with the optimiser's own moment tensors and its incremented step, then every actor
    in agent order with lr * 0.1 and eps 1e-7 -- and neither `critics_opt.step` nor `_fresh_adam_step`; the weights agree with a
    hook-free run from the same state at rtol 1e-4 (atol 2e-6 at lr 1e-4, as test_gcn_level_backward compares two update paths);
    p.grad keeps the unclipped gradient; removing the hook restores the present path."""
    assert hasattr(RL, "set_optimizer_step")
    rl, batches = _maddpg("cpu")
    rl_ref = copy.deepcopy(rl)
    start = [p.detach().clone() for p in _weights(rl)]
    calls, spied = [], []
    fresh = RL._fresh_adam_step
    monkeypatch.setattr(RL, "_fresh_adam_step", lambda *a, **k: spied.append("fresh") or fresh(*a, **k))

    def hook(params, flat_grad, lr, eps, betas=None, step=None, exp_avg=None, exp_avg_sq=None):
        before = flat_grad.clone()
        calls.append(dict(params=list(params), lr=lr, eps=eps, betas=betas, step=None if step is None else float(step), m=exp_avg, v=exp_avg_sq,
                          unclipped=torch.equal(flat_grad, torch.cat([p.grad.reshape(-1) for p in params]))))
        restatement(params, flat_grad, lr, eps, betas, step, exp_avg, exp_avg_sq)
        assert torch.equal(flat_grad, before)

    RL.set_optimizer_step(hook, "cpu")
    orig = rl.critics_opt.step                                      # (the optimiser exists: `_ensure_ready` made it)
    monkeypatch.setattr(rl.critics_opt, "step", lambda *a, **kw: spied.append("critics") or orig(*a, **kw), raising=False)
    try:
        for b in batches:
            rl.train_on_batch(*b)
    finally:
        RL.set_optimizer_step(None, "cpu")
    assert "cpu" not in RL._OPTIMIZER_STEP
    assert spied == [] and len(calls) == 12
    critics = [p for ag in rl.agents for p in ag.critic_model.parameters()]
    for k in range(3):
        c0, actors = calls[4 * k], calls[4 * k + 1:4 * k + 4]
        assert len(c0["params"]) == len(critics) and all(a is b for a, b in zip(c0["params"], critics))
        assert c0["step"] == k + 1 and c0["m"] is rl.critics_opt.exp_avg and c0["v"] is rl.critics_opt.exp_avg_sq
        assert c0["lr"] == rl.agents[0].lr and c0["eps"] == 1e-7 and tuple(c0["betas"]) == (B1, B2) and c0["unclipped"]
        for i, (a, ag) in enumerate(zip(actors, rl.agents)):
            own = list(ag.actor_model.parameters())
            assert len(a["params"]) == len(own) and all(x is y for x, y in zip(a["params"], own))
            assert a["step"] is None and a["m"] is None and a["v"] is None and a["unclipped"]
            assert a["lr"] == ag.lr * 0.1 and a["eps"] == 1e-7
    assert float(rl.critics_opt.step_t) == 3.0 and [t.data_ptr() for t in rl.critics_opt.state_tensors()] == \
        [rl.critics_opt.step_t.data_ptr(), calls[0]["m"].data_ptr(), calls[0]["v"].data_ptr()]
    for b in batches:
        rl_ref.train_on_batch(*b)
    assert spied == ["fresh"] * 9                                   # the hook-free run took the present path (the spy on `step` is rl's own)
    assert max(float((p.detach() - s).abs().max()) for p, s in zip(_weights(rl), start)) > 1e-4
    for p, q in zip(_weights(rl), _weights(rl_ref)):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=2e-6)
    for a, b in zip(rl.critics_opt.state_tensors(), rl_ref.critics_opt.state_tensors()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-9)
    del spied[:]
    rl.train_on_batch(*batches[0])                                  # the hook removed: the present path, looked up at call time
    assert spied == ["critics", "fresh", "fresh", "fresh"] and len(calls) == 12 and float(rl.critics_opt.step_t) == 4.0


def test_plumbing(monkeypatch):
    """the operator is in the table and registered; the lane emulator does not export the entry: the operator refuses by its name,
    and BatchedMARL(optimizer_path="hip") on that library at construction; "torch" is the default, TRUSS_OPTIMIZER=hip selects "hip"
    where the argument is not given, an unknown value is refused"""
    assert "truss_optim_step" in ops.entries()
    ns = ops.namespace()
    for key in ("CPU", "CUDA", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("truss_mi355::optim_step", key)
    assert C.sizeof(_lib.OptimTensor) == 24 and C.sizeof(_lib.OptimArgs) == 112
    emu = pc.emu_lib()
    assert emu.backend == "emu" and not emu.has_optim_step
    w, g = torch.ones(5), torch.ones(5)
    with pytest.raises(tm.TrussError, match="has no truss_optim_step"):
        ops.call(ns.optim_step, ops.bind(emu), 0, _lib.OPTIM_FIRST_STEP, [w], g, None, None, None, 1e-3, B1, B2, 1e-7,
                 torch.zeros(1, dtype=torch.float64), None, None)
    assert bool((w == 1).all())
    with pytest.raises(tm.TrussError, match="has no truss_optim_step"):
        optim.optimizer_step(emu)
    topo = tm.TrussTopology.grid(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 8, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    mk = lambda **kw: marl.BatchedMARL(topo, 2, rl, max_front=6, lib=emu, device="cpu", replay_capacity=8, batch_size=2, **kw)
    monkeypatch.delenv("TRUSS_OPTIMIZER", raising=False)
    assert mk().optimizer_path == "torch" and mk(optimizer_path="torch").optimizer_path == "torch"
    with pytest.raises(ValueError, match="has no truss_optim_step"):
        mk(optimizer_path="hip")
    monkeypatch.setenv("TRUSS_OPTIMIZER", "hip")
    with pytest.raises(ValueError, match="has no truss_optim_step"):
        mk()
    assert mk(optimizer_path="torch").optimizer_path == "torch"
    monkeypatch.setenv("TRUSS_OPTIMIZER", "1")
    assert mk().optimizer_path == "torch"
    with pytest.raises(ValueError, match="optimizer_path must be"):
        mk(optimizer_path="fused")
    assert "cpu" not in RL._OPTIMIZER_STEP


# ---- on the GPU: the C entry ------------------------------------------------------------------------------------------------------

GUARD = 12345.0


def _c_call(lib, mode, ptrs, offsets, numels, grad, m, v, step, lr, eps, partials, clipped=None, norms=None, struct_size=None,
            betas=(B1, B2)):
    """truss_optim_step through ctypes on torch's current stream -> the return code (synchronised)"""
    n = len(ptrs)
    ts = (_lib.OptimTensor * max(n, 1))()
    for i in range(n):
        ts[i].p, ts[i].offset, ts[i].numel = ptrs[i], offsets[i], numels[i]
    dp = lambda t: None if t is None else t.data_ptr()
    a = _lib.OptimArgs()
    a.struct_size = C.sizeof(_lib.OptimArgs) if struct_size is None else struct_size
    a.mode, a.n_tensors, a.tensors = mode, n, C.cast(ts, C.POINTER(_lib.OptimTensor))
    a.grad, a.exp_avg, a.exp_avg_sq, a.step = dp(grad), dp(m), dp(v), dp(step)
    a.lr, a.beta1, a.beta2, a.eps = lr, betas[0], betas[1], eps
    a.partials, a.clipped, a.norms = dp(partials), dp(clipped), dp(norms)
    rc = lib.dll.truss_optim_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _layout(sizes, views):
    """offsets of the tensors in the flat vectors -- gaps between the ranges, every second tensor off the 16-byte grid -- and the
    parameters: separate allocations, or views at odd element offsets of one buffer with guard words around them"""
    offsets, o = [], 3
    for i, n in enumerate(sizes):
        o += (-o) % 4 + (0 if i % 2 == 0 else 1 + i % 3)
        offsets.append(o)
        o += n
    total = o + 5
    if not views:
        return offsets, total, None, [torch.empty(n, device="cuda") for n in sizes]
    starts, q = [], 1
    for n in sizes:
        starts.append(q)
        q += n + 1 + (q + n) % 2             # one or two guard words: every start odd
    buf = torch.full((q + 3,), GUARD, device="cuda")
    assert all(s % 2 == 1 for s in starts)
    return offsets, total, buf, [buf[s:s + n] for s, n in zip(starts, sizes)]


def _scatter(total, offsets, pieces, fill):
    out = torch.full((total,), fill, dtype=torch.float32)
    for o, x in zip(offsets, pieces):
        out[o:o + x.numel()] = x
    return out


def _gather(flat, offsets, sizes):
    return torch.cat([flat[o:o + n] for o, n in zip(offsets, sizes)]).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("views", [False, True], ids=["separate", "views"])
@pytest.mark.parametrize("mode", ["adam", "first"])
def test_kernels_against_float64_stage_by_stage(mode, views):
    """both modes on the shared inputs, the parameters as separate allocations and as views at odd element offsets of one buffer:
    `norms` and `clipped` against the float64 clip, m', v', w' against the float64 step from `clipped`, everything outside the
    tensors' ranges (guard words, the gaps of m, v and clipped) and `grad` untouched, a second call from the same inputs gives the
    same bits, and so does a call with clipped = norms = NULL.  Both access widths run: every second range starts off the 16-byte grid.
    Largest error / bound measured on an MI355X, all four cases alike (profiles/r18/optim_step_tests.txt): clip 0.22, w 1.00, m 0.99,
    v 0.68, fresh 0.99 -- the figures of the CPU restatement to every digit printed."""
    lib = tm.load()
    inp = _inputs()
    sizes = inp["sizes"]
    offsets, total, buf, params = _layout(sizes, views)
    assert any(o % 4 == 0 for o, n in zip(offsets, sizes) if n > CHUNK) and any(o % 4 for o, n in zip(offsets, sizes) if n > CHUNK)
    split = lambda flat: list(flat.split(sizes))
    grad = _scatter(total, offsets, inp["g"], GUARD).cuda()
    grad0 = grad.clone()
    partials = torch.zeros(optim.n_chunks(sizes), dtype=torch.float64, device="cuda")
    c64, n64 = _clip64(inp["g"])
    worst = {}
    for t, lr, eps in (ADAM_CASES if mode == "adam" else FIRST_CASES):
        m0, v0 = _moments(inp, t)
        step = None if t is None else torch.tensor(float(t), dtype=torch.float64, device="cuda")
        results = []
        for outputs in (True, True, False):
            for p, x in zip(params, split(inp["w"])):
                p.copy_(x)
            m = _scatter(total, offsets, split(m0), GUARD).cuda() if t is not None else None
            v = _scatter(total, offsets, split(v0), GUARD).cuda() if t is not None else None
            clipped = torch.full((total,), GUARD, device="cuda") if outputs else None
            norms = torch.full((len(sizes) + 2,), GUARD, device="cuda") if outputs else None
            rc = _c_call(lib, _lib.OPTIM_ADAM if t is not None else _lib.OPTIM_FIRST_STEP, [p.data_ptr() for p in params], offsets, sizes,
                         grad, m, v, step, lr, eps, partials, clipped, norms)
            assert rc == 0, lib.dll.truss_last_error()
            results.append(dict(w=torch.cat([p.reshape(-1) for p in params]).cpu(), m=m, v=v, clipped=clipped, norms=norms))
        first, again, bare = results
        assert torch.equal(grad, grad0)
        for q in ("w", "m", "v", "clipped", "norms"):
            if first[q] is not None:
                assert torch.equal(first[q], again[q]), f"{q}: a second call gives other bits"
        assert torch.equal(first["w"], bare["w"]) and (t is None or (torch.equal(first["m"], bare["m"]) and torch.equal(first["v"], bare["v"])))
        # outside the tensors' ranges nothing is written
        inside = torch.zeros(total, dtype=torch.bool)
        for o, n in zip(offsets, sizes):
            inside[o:o + n] = True
        for q in ("m", "v", "clipped"):
            if first[q] is not None:
                assert bool((first[q].cpu()[~inside] == GUARD).all()), f"{q} written outside the tensors' ranges"
        assert bool((first["norms"][len(sizes):] == GUARD).all())
        if buf is not None:
            keep = torch.ones(buf.numel(), dtype=torch.bool)
            for p in params:
                s = p.storage_offset()
                keep[s:s + p.numel()] = False
            assert bool((buf.cpu()[keep] == GUARD).all()), "guard words around the parameters overwritten"
        norms = f64(first["norms"][:len(sizes)])
        assert float(((norms - torch.tensor(n64)).abs() / torch.tensor(n64)).max()) <= U
        got = dict(c=_gather(first["clipped"], offsets, sizes), w=first["w"])
        if t is not None:
            got.update(m=_gather(first["m"], offsets, sizes), v=_gather(first["v"], offsets, sizes))
        for q, r in _figures(inp["g"], inp["w"], m0, v0, t, lr, eps, got).items():
            worst[q] = max(worst.get(q, 0.0), r)
            assert r <= 1.0, f"t={t} lr={lr}: {q} at {r:.3g} of its bound"
    print(f"\n[kernels against float64, {mode}, {'views' if views else 'separate'}] largest error / bound: " + ", ".join(f"{q} {r:.3g}" for q, r in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["adam", "first"])
def test_more_tensors_than_one_launch_pair(mode):
    """TRUSS_OPTIM_MAX_TENSORS + 3 tensors of 1..5 elements through the operator (the offsets are the running sum of the sizes): two
    launch pairs in one call, the same checks"""
    lib = tm.load()
    sizes = tuple(1 + i % 5 for i in range(_lib.OPTIM_MAX_TENSORS + 3))
    inp = _inputs(sizes)
    t, lr, eps = (2, 1e-3, 1e-8) if mode == "adam" else (None, 1e-3, 1e-7)
    m0, v0 = _moments(inp, t)
    params = [x.clone().cuda() for x in inp["w"].split(list(sizes))]
    grad = torch.cat(inp["g"]).cuda()
    m, v = (m0.clone().cuda(), v0.clone().cuda()) if t is not None else (None, None)
    clipped, norms = torch.empty_like(grad), torch.empty(len(sizes), device="cuda")
    step = None if t is None else torch.tensor(float(t), dtype=torch.float64, device="cuda")
    optim.optim_step(lib, params, grad, lr, eps, betas=(B1, B2), step=step, exp_avg=m, exp_avg_sq=v, clipped=clipped, norms=norms)
    torch.cuda.synchronize()
    assert torch.equal(grad.cpu(), torch.cat(inp["g"]))
    n64 = torch.tensor(_clip64(inp["g"])[1])
    assert float(((f64(norms) - n64).abs() / n64).max()) <= U
    got = dict(c=clipped.cpu(), w=torch.cat(params).cpu())
    if t is not None:
        got.update(m=m.cpu(), v=v.cpu())
    fig = _figures(inp["g"], inp["w"], m0, v0, t, lr, eps, got)
    print(f"\n[{len(sizes)} tensors, {mode}] error / bound: " + ", ".join(f"{q} {r:.3g}" for q, r in fig.items()))
    assert all(r <= 1.0 for r in fig.values()), fig


@pytest.mark.gpu
def test_refusals_write_nothing():
    """TRUSS_EINVAL with every output as it was: a bad struct_size, an unknown mode, numel = 0, overlapping and descending ranges, a
    missing moment pointer in ADAM mode, an output overlapping grad; at the operator a non-contiguous and a float64 parameter;
    n_tensors = 0 is TRUSS_OK and writes nothing either"""
    lib = tm.load()
    fill = lambda n, dt=torch.float32: torch.full((n,), GUARD, dtype=dt, device="cuda")
    w = [fill(8), fill(8)]
    grad, m, v, clipped, norms, partials = fill(32), fill(32), fill(32), fill(32), fill(2), fill(2, torch.float64)
    step = torch.tensor(1.0, dtype=torch.float64, device="cuda")
    outs = w + [grad, m, v, clipped, norms, partials]
    ptrs = [x.data_ptr() for x in w]
    call = lambda mode=_lib.OPTIM_ADAM, offsets=(0, 8), numels=(8, 8), m_=m, ptrs_=ptrs, clipped_=clipped, **kw: \
        _c_call(lib, mode, list(ptrs_), list(offsets), list(numels), grad, m_, v, step, 1e-3, 1e-8, partials, clipped_, norms, **kw)
    refused = {
        "struct_size": call(struct_size=C.sizeof(_lib.OptimArgs) - 8),
        "mode": call(mode=2),
        "numel = 0": call(numels=(8, 0)),
        "overlapping ranges": call(offsets=(0, 7)),
        "descending ranges": call(offsets=(8, 0)),
        "missing moment": call(m_=None),
        "clipped overlaps grad": call(clipped_=grad[4:]),
        "a parameter overlaps grad": call(ptrs_=[ptrs[0], grad[8:].data_ptr()]),
        "beta outside [0, 1)": call(betas=(1.0, B2)),
        "lr not finite": _c_call(lib, _lib.OPTIM_ADAM, ptrs, [0, 8], [8, 8], grad, m, v, step, float("nan"), 1e-8, partials, clipped, norms),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    assert b"truss_optim_step" in lib.dll.truss_last_error()
    assert _c_call(lib, _lib.OPTIM_ADAM, [], [], [], grad, m, v, step, 1e-3, 1e-8, partials, clipped, norms) == 0
    assert _c_call(lib, _lib.OPTIM_FIRST_STEP, [], [], [], None, None, None, None, 1e-3, 1e-8, None) == 0
    strided = torch.full((8, 2), GUARD, device="cuda")[:, 0]
    with pytest.raises(tm.TrussError, match="contiguous"):
        optim.optim_step(lib, [w[0], strided], grad[:16], 1e-3, 1e-7, partials=partials)
    with pytest.raises(tm.TrussError, match="Float"):
        optim.optim_step(lib, [w[0], fill(8, torch.float64)], grad[:16], 1e-3, 1e-7, partials=partials)
    with pytest.raises(tm.TrussError, match="grad has"):
        optim.optim_step(lib, w, grad, 1e-3, 1e-7, partials=partials)
    torch.cuda.synchronize()
    assert all(bool((x == GUARD).all()) for x in outs + [strided])


@pytest.mark.gpu
def test_against_the_torch_path():
    """the shared inputs (contiguous: the offsets are the running sum) through the kernels and through `_clip_flat` +
    `SharedStepAdam.step` / `_fresh_adam_step` on the GPU: both inside the float64 bounds of the step from their own clipped
    gradient; the kernels' clip inside 6 u per element, the torch path's -- a float32 sum of n squares -- inside the
    ((n + 1) / 2 + 4) u ||c64|| per tensor of tests/test_update_float64.py.  The number of differing elements is printed (measured
    on an MI355X: between 0 and 1722 of 61 464 weights, profiles/r18/optim_step_tests.txt)."""
    lib = tm.load()
    inp = _inputs()
    sizes = inp["sizes"]
    grad = torch.cat(inp["g"]).cuda()
    c64 = _clip64(inp["g"])[0]
    for t, lr, eps in ADAM_CASES + FIRST_CASES:
        m0, v0 = _moments(inp, t)
        step = None if t is None else torch.tensor(float(t), dtype=torch.float64, device="cuda")
        hp = [x.clone().cuda() for x in inp["w"].split(sizes)]
        hm, hv = (m0.clone().cuda(), v0.clone().cuda()) if t is not None else (None, None)
        hc = torch.empty_like(grad)
        optim.optim_step(lib, hp, grad, lr, eps, betas=(B1, B2), step=step, exp_avg=hm, exp_avg_sq=hv, clipped=hc)
        tp = [x.clone().cuda() for x in inp["w"].split(sizes)]
        tc = RL._clip_flat(grad.clone(), tp)
        if t is None:
            RL._fresh_adam_step(tp, lr, eps, tc.clone())
            tm_, tv = None, None
        else:
            opt = RL.SharedStepAdam(tp, lr=lr, eps=eps, betas=(B1, B2))
            opt.step_t = torch.tensor(float(t - 1), dtype=torch.float64, device="cuda")
            opt.exp_avg, opt.exp_avg_sq = m0.clone().cuda(), v0.clone().cuda()
            opt.step(tc.clone())
            tm_, tv = opt.exp_avg, opt.exp_avg_sq
        torch.cuda.synchronize()
        for c, c_ in zip(tc.cpu().split(sizes), c64):
            assert float((f64(c) - c_).norm()) <= ((c.numel() + 1) / 2.0 + 4.0) * U * float(c_.norm())
        line = []
        for name, c, ps, m, v in (("hip", hc, hp, hm, hv), ("torch", tc, tp, tm_, tv)):
            got = dict(c=c.cpu(), w=torch.cat(ps).cpu())
            if t is not None:
                got.update(m=m.cpu(), v=v.cpu())
            fig = _figures(inp["g"], inp["w"], m0, v0, t, lr, eps, got)
            if name == "torch":
                del fig["clip"]                  # (held per tensor above)
            assert all(r <= 1.0 for r in fig.values()), (name, t, lr, fig)
            line.append(f"{name} " + " ".join(f"{q} {r:.2g}" for q, r in fig.items()))
        differ = int((torch.cat(hp) != torch.cat(tp)).sum())
        print(f"[t={t} lr={lr}] {'; '.join(line)}; weights that differ between the two paths: {differ} of {grad.numel()}")


def _device_kernels(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.gpu
def test_one_hook_call_is_two_launches():
    """the hook on the critics' list (144 tensors) of a small MADDPG: one truss_optim_norm_kernel, one truss_optim_apply_kernel and
    no other device operation -- for the Adam step and for an actor's first step"""
    lib = tm.load()
    rl, _ = _maddpg("cuda")
    critics = [p for ag in rl.agents for p in ag.critic_model.parameters()]
    assert len(critics) == 144 <= _lib.OPTIM_MAX_TENSORS
    hook = optim.optimizer_step(lib)
    flat = torch.randn(sum(p.numel() for p in critics), device="cuda")
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    step = torch.ones((), dtype=torch.float64, device="cuda")
    actor = list(rl.agents[0].actor_model.parameters())
    aflat = torch.randn(sum(p.numel() for p in actor), device="cuda")
    hook(critics, flat, 1e-3, 1e-7, betas=(B1, B2), step=step, exp_avg=m, exp_avg_sq=v)     # (the first call makes the scratch)
    hook(actor, aflat, 1e-4, 1e-7)
    torch.cuda.synchronize()
    for names in (_device_kernels(lambda: hook(critics, flat, 1e-3, 1e-7, betas=(B1, B2), step=step, exp_avg=m, exp_avg_sq=v)),
                  _device_kernels(lambda: hook(actor, aflat, 1e-4, 1e-7))):
        assert len(names) == 2 and sum("truss_optim_norm_kernel" in n for n in names) == 1 and \
            sum("truss_optim_apply_kernel" in n for n in names) == 1, names


# ---- on the GPU: the engine --------------------------------------------------------------------------------------------------------

def _engine(lib, optimizer_path):
    with contextlib.redirect_stdout(io.StringIO()):
        topo = tm.TrussTopology.grid(4)
        torch.manual_seed(5)
        rl = RL.MADDPG(1e-3, M.ep, M.epd, M.gamma, 40, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda")
        eng = marl.BatchedMARL(topo, 64, rl, max_front=6, lib=lib, device="cuda", replay_capacity=256, batch_size=8, seed=5,
                               optimizer_path=optimizer_path)
        b = synthetic.random_batch(topo, 64, 5)
        eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return topo, rl, eng


@pytest.mark.gpu
def test_engine_with_the_option():
    """two BatchedMARL engines (the topology of test_marl_batched.test_train_graph_update_deltas_match_eager: 64 envs, hidden 40, lr
    1e-3, batch 8) that differ only in optimizer_path, from equal weights and batches: three eager updates agree at rtol 1e-4 (atol
    2e-6); with the option, the optimiser's state after the capture equals its state before the warm-up (restore works on the hook's
    in-place updates), three replayed updates give the eager ones' weight deltas within 0.05 (as test_gcn_level_backward holds replay
    against eager), and against `update_reference.Update64` run free from the same snapshot the replayed deltas are within 4 x what
    the "torch" engine's replay reaches, never above 1e-3 (the rule of test_replayed_update_against_float64).
    Measured on an MI355X (profiles/r18/optim_step_tests.txt): replayed against float64, actors 3.8e-05 3.6e-05 2.9e-05 and critics
    3.7e-06 4.4e-06 3.6e-06 with the option, 3.4e-05 3.6e-05 2.9e-05 and 3.7e-06 4.5e-06 3.6e-06 without; with the option the replayed
    deltas equal the eager ones bit for bit."""
    lib = tm.load()
    prev = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda"), RL._OPTIMIZER_STEP.get("cuda")
    try:
        figures = {}
        eager_weights = {}
        for path in ("torch", "hip"):
            topo, rl, eng = _engine(lib, path)
            assert eng.optimizer_path == path and ("cuda" in RL._OPTIMIZER_STEP) == (path == "hip")
            with contextlib.redirect_stdout(io.StringIO()):
                eng.game_step_all(train=True, explore=True, update=False)           # fills the replay; no update yet
            gen = torch.Generator(device="cuda")
            gen.manual_seed(1)
            fixed = []
            for _ in range(3):
                S, NS, ag, at, R = eng.replay.sample(eng.batch_size, gen)
                fixed.append((eng._net_state(S), [eng._net_state(ns) for ns in NS], [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)], R))
            eng.use_train_graph = False
            eng._train(*fixed[0])                                                  # one eager update: the optimiser has a state
            torch.cuda.synchronize()
            names, own = UR.names_of(rl), UR.tensors_of(rl)
            state = [t for k in UR.KINDS for ts in own[k] for t in ts] + rl.critics_opt.state_tensors()
            snap = [t.detach().clone() for t in state]
            start = {k: [[p.detach().clone() for p in ps] for ps in own[k]] for k in UR.KINDS}
            opt0 = [f64(t) for t in rl.critics_opt.state_tensors()]
            assert float(opt0[0]) == 1.0

            def run(graph):
                with torch.no_grad():
                    for t, v in zip(state, snap):
                        t.copy_(v)
                eng.use_train_graph = graph
                for b_ in fixed:
                    eng._train(*b_)
                torch.cuda.synchronize()
                cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
                return {k: [cat([f64(p) - f64(v) for p, v in zip(ps, vs)]) for ps, vs in zip(own[k], start[k])] for k in ("actor", "critic")}

            d_eager = run(False)
            eager_weights[path] = [p.detach().clone() for p in _weights(rl)]
            assert float(rl.critics_opt.step_t) == 4.0
            def one(graph):
                with torch.no_grad():
                    for t, v in zip(state, snap):
                        t.copy_(v)
                eng.use_train_graph = graph
                eng._train(*fixed[0])
                torch.cuda.synchronize()
                return [t.detach().clone() for t in rl.critics_opt.state_tensors()]

            o_eager = one(False)
            o_graph = one(True)                                                    # warm-up, capture, restore, one replay
            assert eng._tg is not None, "the update was not captured"
            # restored to the state before the warm-up, then ONE replayed step: the eager step's state (three warm-up steps on top
            # would leave t = 5 and other moments)
            assert float(o_graph[0]) == float(o_eager[0]) == 2.0
            torch.testing.assert_close(o_graph[1], o_eager[1], rtol=1e-3, atol=1e-8)
            torch.testing.assert_close(o_graph[2], o_eager[2], rtol=1e-3, atol=1e-10)
            assert [t.data_ptr() for t in rl.critics_opt.state_tensors()] == [t.data_ptr() for t in state[-3:]]
            d_graph = run(True)
            assert float(rl.critics_opt.step_t) == 4.0
            P = UR.params64(names, start)
            opt = {"t": int(opt0[0]), "m": opt0[1].clone(), "v": opt0[2].clone()}
            model = UR.Update64(rl.gamma, 1e-3)
            for b_ in fixed:
                model.update(P, opt, UR.batch64(b_))
            P0 = UR.params64(names, start)
            cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
            d64 = {k: [cat(p.values()) - cat(p0.values()) for p, p0 in zip(P[k], P0[k])] for k in ("actor", "critic")}
            rel = lambda d, ref: {k: [float((a - r).norm() / r.norm()) for a, r in zip(d[k], ref[k])] for k in d}
            figures[path] = dict(graph64=rel(d_graph, d64), eager64=rel(d_eager, d64), graph_eager=rel(d_graph, d_eager))
            assert min(float(d.abs().max()) for k in d64 for d in d64[k]) > 1e-4
            fmt = lambda r: ", ".join(f"{k} " + " ".join(f"{x:.3g}" for x in xs) for k, xs in r.items())
            print(f"\n[engine, optimizer_path={path}] ||dW - dW64|| / ||dW64||: replayed {fmt(figures[path]['graph64'])}; eager {fmt(figures[path]['eager64'])}"
                  f"\n  replayed against eager: {fmt(figures[path]['graph_eager'])}")
        for p, q in zip(eager_weights["hip"], eager_weights["torch"]):
            torch.testing.assert_close(p, q, rtol=1e-4, atol=2e-6)
        hip, ref = figures["hip"], figures["torch"]
        for k in ("actor", "critic"):
            assert max(hip["graph_eager"][k]) <= 0.05
            tau = min(4.0 * max(ref["graph64"][k]), 1e-3)
            assert max(hip["graph64"][k]) <= tau, f"replayed {k}: {hip['graph64'][k]} > {tau:.3g}"
    finally:
        RL.set_level_forward(prev[0], "cuda")
        RL.set_level_backward(prev[1], "cuda")
        RL.set_optimizer_step(prev[2], "cuda")
