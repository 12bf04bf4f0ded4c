"""Tracking target networks of the MADDPG update: `MADDPG(target_update="polyak" / "hard")`, the framework path
`truss2D_RL._target_update_torch`, the native entry `truss_target_update` (csrc/truss_target.h), `torch.ops.truss_mi355.target_update`,
the hook `truss2D_RL.set_target_update` / `truss_mi355.target.target_hook` and BatchedMARL(target_path="hip") -- against a float64
model of the arithmetic the header states.

Bound (derived, not measured; u = 2^-24, first order in u, valid with or without the product contracted into an FMA; the float64
model takes the float32 values of t and p as exact inputs):
  tau < 0.5        t' = t + (float) tau (p - t): one rounding of the difference, one of tau to float32, one of the product (each
                   relative to tau |p - t|), one of the sum (relative to t'), one to spare:      |t' - t'64| <= u (|t'64| + 4 tau |p - t|)
  0.5 <= tau < 1   t' = p - (p - t) (float) (1 - tau): the same count with (1 - tau) for tau:     |t' - t'64| <= u (|t'64| + 4 (1 - tau) |p - t|)
  tau == 1, and a gate that does not fire: bitwise.
Shared inputs: two "agents" with pairs of 1, 3, 7, 200, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 5 and 40 000 elements
each (below, at and above a workgroup's 256 threads and its chunk, more than one chunk, ten chunks), p ~ 0.1 N(0, 1),
t = p + 0.05 N(0, 1), one run of elements with t == p exactly across the first chunk boundary of the 2 CHUNK + 5 pair; tau in
{0.005, 0.3, 0.5, 0.75, 1}; gates: step None, (step, period) in {(3, 1), (3, 3), (4, 3), (1000, 100), (1001, 100)}.
"""
import contextlib
import copy
import ctypes as C
import io

import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import _lib, marl, ops, synthetic, target
import master_DDPG_truss2D_MO as M
import parity_common as pc
import truss2D_RL as RL

U = 2.0 ** -24
CHUNK = _lib.TARGET_CHUNK
SIZES = [1, 3, 7, 200, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 40000]
N_AGENT = len(SIZES)                         # the shared list is these sizes twice: "agent" 0, then "agent" 1
EQ_PAIR, EQ_RUN = SIZES.index(2 * CHUNK + 5), slice(4000, 4300)      # t == p across the pair's first chunk boundary
TAUS = (0.005, 0.3, 0.5, 0.75, 1.0)
GATES = [None, (3, 1), (3, 3), (4, 3), (1000, 100), (1001, 100)]
MUTANTS = ("tau x 10", "t and p swapped", "plain formula with tau rounded to bfloat16", "the gate fires one update late",
           "agent 0's targets fed from agent 1's networks")
f64 = lambda t: t.detach().double().cpu().reshape(-1)
bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)
same_bits = lambda a, b: torch.equal(bits(a), bits(b))


# ---- the inputs, the float64 model and its bound --------------------------------------------------------------------------------------

_INPUTS = {}


def _inputs(sizes=tuple(SIZES + SIZES)):
    """-> (t, p): lists of float32 tensors on the CPU, made once and never modified"""
    if sizes not in _INPUTS:
        gen = torch.Generator().manual_seed(11)
        ps = [(0.1 * torch.randn(n, generator=gen, dtype=torch.float64)).float() for n in sizes]
        ts = [(p.double() + 0.05 * torch.randn(p.numel(), generator=gen, dtype=torch.float64)).float() for p in ps]
        if sizes == tuple(SIZES + SIZES):
            ts[EQ_PAIR][EQ_RUN] = ps[EQ_PAIR][EQ_RUN]
        _INPUTS[sizes] = (ts, ps)
    return _INPUTS[sizes]


def _fires(gate, late=False):
    return gate is None or (gate[0] - (1 if late else 0)) % gate[1] == 0


def _lerp64(t, p, tau):
    """the float64 lerp of float64 vectors, by the branch the header states"""
    if tau == 1.0:
        return p.clone()
    return t + tau * (p - t) if tau < 0.5 else p - (p - t) * (1.0 - tau)


def _bound(t, p, tau):
    if tau == 1.0:
        return torch.zeros_like(t)
    return U * (_lerp64(t, p, tau).abs() + 4.0 * (tau if tau < 0.5 else 1.0 - tau) * (p - t).abs())


def _model(ts, ps, tau, gate, mutant=None):
    """float32 lists -> the flat float64 result of one call.  mutant: one of MUTANTS, the model is the broken one."""
    t, p = torch.cat([f64(x) for x in ts]), torch.cat([f64(x) for x in ps])
    if mutant == "agent 0's targets fed from agent 1's networks":
        half = len(ps) // 2
        p = torch.cat([f64(x) for x in ps[half:] + ps[half:]])
    if not _fires(gate, late=mutant == "the gate fires one update late"):
        return t
    if mutant == "tau x 10":
        return t + 10.0 * tau * (p - t)
    if mutant == "t and p swapped":
        return _lerp64(p, t, tau)
    if mutant == "plain formula with tau rounded to bfloat16":
        return t + float(torch.tensor(tau).bfloat16()) * (p - t)
    return _lerp64(t, p, tau)


def _worst(err, bound):
    """max err / bound (an element whose bound is 0 must be exact)"""
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _figure(ts, ps, tau, gate, got, mutant=None):
    """error / bound of a result (list of float32 tensors) against the (mutant) model; the bound stays that of the correct
    arithmetic, and is zero -- bitwise -- where the gate does not fire"""
    t, p = torch.cat([f64(x) for x in ts]), torch.cat([f64(x) for x in ps])
    bound = _bound(t, p, tau) if _fires(gate) else torch.zeros_like(t)
    return _worst((torch.cat([f64(x).reshape(-1) for x in got]) - _model(ts, ps, tau, gate, mutant)).abs(), bound)


def _step(gate, device="cpu"):
    return None if gate is None else torch.tensor(float(gate[0]), dtype=torch.float64, device=device)


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------

def test_framework_path_stays_inside_the_bound_and_mutants_do_not():
    """`_target_update_torch` on the shared inputs against the float64 model: every element inside the bound for every tau and gate
    (bitwise at tau = 1 and where the gate does not fire: the old bits, the sign of a zero included), the sources untouched; every
    mutant of the model at least 10 x outside on at least one case.
    The third mutant as the issue words it -- the formula of the upper branch at tau = 0.75 replaced by plain t + tau (p - t) with
    tau rounded to bfloat16 -- cannot be seen there: 0.75 (like 0.5 and 1) is a bfloat16 number and the two formulae agree in exact
    arithmetic.  It is applied at every tau instead, 0.75 included, and shows at 0.005 and 0.3.
    Measured on the CPU: largest error / bound 0.997 (half an ulp of the result is the bound's leading term); the mutants at
    1.1e8, 8.3e8, 1.1e4, 1.3e7 and 1.3e10 of the bound."""
    ts, ps = _inputs()
    runs, worst = [], 0.0
    for tau in TAUS:
        for gate in GATES:
            got, src = [x.clone() for x in ts], [x.clone() for x in ps]
            got[0][0] = -0.0 if not _fires(gate) else got[0][0]               # (a zero's sign survives an unfired gate)
            ins = [x.clone() for x in got]
            RL._target_update_torch(got, src, tau, 1 if gate is None else gate[1], _step(gate))
            assert all(same_bits(a, b) for a, b in zip(src, ps)), "a source was written"
            r = _figure(ins, ps, tau, gate, got)
            worst = max(worst, r)
            assert r <= 1.0, f"tau={tau} gate={gate}: at {r:.3g} of the bound"
            if tau == 1.0 and _fires(gate):
                assert all(same_bits(a, b) for a, b in zip(got, ps))
            if not _fires(gate):
                assert all(same_bits(a, b) for a, b in zip(got, ins))
            runs.append((tau, gate, ins, got))
    print(f"\n[framework path against float64] largest error / bound: {worst:.3g}")
    for mutant in MUTANTS:
        # (only where the bound is not zero -- tau < 1 and the gate fires -- so that the figure is a finite multiple of it)
        far = max(_figure(ins, ps, tau, gate, got, mutant) for tau, gate, ins, got in runs if tau < 1.0 and _fires(gate))
        print(f"[mutant '{mutant}'] largest error / bound over the cases: {far:.3g}")
        assert far >= 10.0, f"mutant '{mutant}' stays within 10 x the bound on every case"


def _batch(seed, B, N, P, device):
    """a minibatch (S, NS, A, R) as tests/test_optim_step._batch builds it (one shared adjacency and mask)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g).to(device)
    A = lambda n: torch.softmax(torch.randn(B, n, n, generator=g), -1).to(device)
    a_n, mask = A(N)[:1].expand(B, -1, -1), torch.ones(1, N, N).to(device).expand(B, -1, -1)
    state = lambda: [r(B, N, 13), a_n, A(N), A(N), A(N), mask, r(B, P, 4), A(P)]
    return state(), [state() for _ in range(3)], [(r(B, N, 2), r(B, N, 3)) for _ in range(3)], r(B, 3)


def _maddpg(device, lr=1e-4, B=5, N=12, P=20, H=40, C=8, seed=5, **kw):
    torch.manual_seed(seed)
    rl = RL.MADDPG(lr, M.ep, M.epd, M.gamma, H, C, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device, **kw)
    batches = [_batch(20 + k, B, N, P, device) for k in range(3)]
    S, NS, A, R = batches[0]
    rl._ensure_ready(S, [t for a in A for t in a])
    return rl, batches


def _nets(rl):
    """(online, target) network pairs in the order the update walks them"""
    return [(ag.actor_model, ag.target_actor_model) for ag in rl.agents] + [(ag.critic_model, ag.target_critic_model) for ag in rl.agents]


def _online(rl):
    return [p for src, _ in _nets(rl) for p in src.parameters()]


def _targets(rl):
    return [p for _, dst in _nets(rl) for p in dst.parameters()]


def _clone(ts):
    return [t.detach().clone() for t in ts]


def test_maddpg_default_mode_leaves_the_targets_alone():
    """three `train_on_batch` calls in the default mode (and with "fixed" spelled out): every target tensor is what it was -- the
    guard of today's behaviour -- while the online weights move"""
    for kw in ({}, dict(target_update="fixed")):
        rl, batches = _maddpg("cpu", **kw)
        assert rl.target_update == "fixed"
        before, start = _clone(_targets(rl)), _clone(_online(rl))
        for b in batches:
            rl.train_on_batch(*b)
        assert all(torch.equal(a, b) for a, b in zip(_targets(rl), before))
        assert max(float((a.detach() - b).abs().max()) for a, b in zip(_online(rl), start)) > 1e-5


def test_maddpg_polyak_and_hard():
    """"polyak" (tau = OneAgent.tau = 0.005, every update): after each of three calls every target is within the bound of the
    float64 lerp of its previous value and the online value that call left; "hard" with period 2: unchanged, bit for bit, after
    calls 1 and 3, equal to the online networks after call 2; the arguments that are refused"""
    rl, batches = _maddpg("cpu", target_update="polyak")
    assert rl.target_tau == rl.agents[0].tau == 0.005 and rl.target_period == 1 and len(_targets(rl)) == 222
    for k, b in enumerate(batches):
        prev = _clone(_targets(rl))
        rl.train_on_batch(*b)
        r = _figure(prev, _online(rl), 0.005, None, _targets(rl))
        assert r <= 1.0, f"call {k + 1}: at {r:.3g} of the bound"
        assert not any(torch.equal(a, b) for a, b in zip(_targets(rl), prev))
    rl, batches = _maddpg("cpu", target_update="hard", target_period=2)
    assert rl.target_tau == 1.0
    for k, b in enumerate(batches):
        prev = _clone(_targets(rl))
        rl.train_on_batch(*b)
        assert float(rl.critics_opt.step_t) == k + 1
        if k == 1:
            assert all(same_bits(a, b) for a, b in zip(_targets(rl), _online(rl)))
            assert not any(torch.equal(a, b) for a, b in zip(_targets(rl), prev))
        else:
            assert all(same_bits(a, b) for a, b in zip(_targets(rl), prev))
    mk = lambda **kw: RL.MADDPG(1e-4, M.ep, M.epd, M.gamma, 8, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, **kw)
    with pytest.raises(ValueError, match="target_period"):
        mk(target_update="hard")
    for tau in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="target_tau"):
            mk(target_update="polyak", target_tau=tau)
    with pytest.raises(ValueError, match="target_period"):
        mk(target_update="polyak", target_period=0)
    with pytest.raises(ValueError, match="target_update"):
        mk(target_update="soft")


def test_the_hook_is_what_the_update_runs():
    """`set_target_update(fn, "cpu")`: a polyak MADDPG calls the hook once per `train_on_batch` with the 222 target and online
    tensors (contiguous float32, paired by position), its tau and period and the optimiser's step counter itself; a default-mode
    MADDPG never calls it; removing the hook restores the framework path"""
    calls = []
    RL.set_target_update(lambda *a: calls.append(a), "cpu")
    try:
        rl, batches = _maddpg("cpu")
        rl.train_on_batch(*batches[0])
        assert calls == []
        rl, batches = _maddpg("cpu", target_update="polyak", target_tau=0.3, target_period=4)
        before = _clone(_targets(rl))
        rl.train_on_batch(*batches[0])
        assert len(calls) == 1
        targets, sources, tau, period, step = calls[0]
        assert tau == 0.3 and period == 4 and step is rl.critics_opt.step_t and step.dtype == torch.float64 and step.dim() == 0
        assert len(targets) == len(sources) == 222
        for t, s, a, b in zip(targets, sources, _targets(rl), _online(rl)):
            assert t.data_ptr() == a.data_ptr() and s.data_ptr() == b.data_ptr() and t.shape == s.shape
            assert t.is_contiguous() and s.is_contiguous() and t.dtype == s.dtype == torch.float32 and not t.requires_grad
        assert all(torch.equal(a, b) for a, b in zip(_targets(rl), before))       # (this hook does nothing)
    finally:
        RL.set_target_update(None, "cpu")
    assert "cpu" not in RL._TARGET_UPDATE


def test_plumbing(monkeypatch):
    """the operator is in the table and registered; the lane emulator does not export the entry: the operator refuses by its name,
    and so do `target_hook` and BatchedMARL(target_path="hip") on that library, at construction; "torch" is the default,
    TRUSS_TARGET_PATH=hip selects "hip" where the argument is not given, an unknown value is refused"""
    assert "truss_target_update" in ops.entries()
    ns = ops.namespace()
    for key in ("CPU", "CUDA", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("truss_mi355::target_update", key)
    assert C.sizeof(_lib.TargetPair) == 24 and C.sizeof(_lib.TargetArgs) == 48
    emu = pc.emu_lib()
    assert emu.backend == "emu" and not emu.has_target_update
    t, p = torch.ones(5), torch.zeros(5)
    with pytest.raises(tm.TrussError, match="has no truss_target_update"):
        ops.call(ns.target_update, ops.bind(emu), 0, [t], [p], 0.5, 1, None)
    with pytest.raises(tm.TrussError, match="has no truss_target_update"):
        target.target_update(emu, [t], [p], 0.5)
    assert bool((t == 1).all())
    with pytest.raises(tm.TrussError, match="has no truss_target_update"):
        target.target_hook(emu)
    topo = tm.TrussTopology.grid(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 8, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu", target_update="polyak")
    mk = lambda **kw: marl.BatchedMARL(topo, 2, rl, max_front=6, lib=emu, device="cpu", replay_capacity=8, batch_size=2, **kw)
    monkeypatch.delenv("TRUSS_TARGET_PATH", raising=False)
    assert mk().target_path == "torch" and mk(target_path="torch").target_path == "torch"
    with pytest.raises(ValueError, match="has no truss_target_update"):
        mk(target_path="hip")
    monkeypatch.setenv("TRUSS_TARGET_PATH", "hip")
    with pytest.raises(ValueError, match="has no truss_target_update"):
        mk()
    assert mk(target_path="torch").target_path == "torch"
    monkeypatch.setenv("TRUSS_TARGET_PATH", "1")
    assert mk().target_path == "torch"
    with pytest.raises(ValueError, match="target_path must be"):
        mk(target_path="fused")
    assert "cpu" not in RL._TARGET_UPDATE


def test_checkpoints(tmp_path):
    """with tracking targets the round trip restores them bit for bit (and the online networks); a file written in the default
    mode has today's keys only and loads with the targets set to the online networks"""
    rl, batches = _maddpg("cpu", target_update="polyak", target_tau=0.3)
    rl.train_on_batch(*batches[0])
    assert not any(torch.equal(a, b) for a, b in zip(_targets(rl), _online(rl)))
    rl.save_weights(str(tmp_path / "track_"))
    sd = torch.load(str(tmp_path / "track_Agent1_pickle.pt"), weights_only=True)
    assert set(sd) == {"actor", "critic", "target_actor", "target_critic"}
    other, _ = _maddpg("cpu", seed=6, target_update="polyak")
    assert not any(torch.equal(a, b) for a, b in zip(_targets(other), _targets(rl)))
    other.load_weights(str(tmp_path / "track_"))
    assert all(same_bits(a, b) for a, b in zip(_targets(other), _targets(rl)))
    assert all(same_bits(a, b) for a, b in zip(_online(other), _online(rl)))
    plain, batches = _maddpg("cpu")
    plain.train_on_batch(*batches[0])
    plain.save_weights(str(tmp_path / "plain_"))
    for i in (1, 2, 3):
        assert set(torch.load(str(tmp_path / f"plain_Agent{i}_pickle.pt"), weights_only=True)) == {"actor", "critic"}
    other.load_weights(str(tmp_path / "plain_"))
    assert all(same_bits(a, b) for a, b in zip(_online(other), _online(plain)))
    assert all(same_bits(a, b) for a, b in zip(_targets(other), _online(plain)))


# ---- on the GPU: the C entry ------------------------------------------------------------------------------------------------------

GUARD = 12345.0


def _c_call(lib, t_ptrs, p_ptrs, numels, tau, period, step, struct_size=None, n_pairs=None, null_pairs=False):
    """truss_target_update through ctypes on torch's current stream -> the return code (synchronised)"""
    n = len(t_ptrs)
    qs = (_lib.TargetPair * max(n, 1))()
    for i in range(n):
        qs[i].t, qs[i].p, qs[i].numel = t_ptrs[i], p_ptrs[i], numels[i]
    a = _lib.TargetArgs()
    a.struct_size = C.sizeof(_lib.TargetArgs) if struct_size is None else struct_size
    a.n_pairs = n if n_pairs is None else n_pairs
    a.pairs = None if null_pairs else C.cast(qs, C.POINTER(_lib.TargetPair))
    a.tau, a.period, a.step = tau, period, None if step is None else step.data_ptr()
    rc = lib.dll.truss_target_update(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _views(sizes):
    """views at odd element offsets of one buffer (never 16-byte aligned: the word-by-word path), one or two guard words between them"""
    starts, q = [], 1
    for n in sizes:
        starts.append(q)
        q += n + 1 + (q + n) % 2
    buf = torch.full((q + 3,), GUARD, device="cuda")
    assert all(s % 2 == 1 for s in starts)
    return buf, [buf[s:s + n] for s, n in zip(starts, sizes)]


def _guards_intact(buf, views):
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    for v in views:
        keep[v.storage_offset():v.storage_offset() + v.numel()] = False
    return bool((buf.cpu()[keep] == GUARD).all())


@pytest.mark.gpu
@pytest.mark.parametrize("views", [False, True], ids=["separate", "views"])
def test_kernel_against_float64(views):
    """the C entry on the shared inputs, targets and sources as separate allocations (16-byte accesses wherever the chunk length
    allows) and as views one float into flat buffers (word by word): every tau, step NULL and every (step, period) -- inside the
    bound on every element where the gate fires, bitwise p at tau = 1, the targets bitwise untouched where it does not; the sources
    and the guard words bitwise untouched in every case.
    Largest error / bound measured on an MI355X: 0.997 with both layouts (profiles/r23/README.md)."""
    lib = tm.load()
    ts, ps = _inputs()
    sizes = [x.numel() for x in ts]
    if views:
        tbuf, tv = _views(sizes)
        pbuf, pv = _views(sizes)
    else:
        tv, pv = [torch.empty(n, device="cuda") for n in sizes], [torch.empty(n, device="cuda") for n in sizes]
        assert all(x.data_ptr() % 16 == 0 for x in tv + pv)
    for x, v in zip(ps, pv):
        v.copy_(x)
    worst = 0.0
    for tau in TAUS:
        for gate in GATES:
            for x, v in zip(ts, tv):
                v.copy_(x)
            rc = _c_call(lib, [v.data_ptr() for v in tv], [v.data_ptr() for v in pv], sizes, tau, 1 if gate is None else gate[1], _step(gate, "cuda"))
            assert rc == 0, lib.dll.truss_last_error()
            got = [v.cpu() for v in tv]
            assert all(same_bits(v, x) for v, x in zip(pv, ps)), "a source was written"
            if views:
                assert _guards_intact(tbuf, tv) and _guards_intact(pbuf, pv), "guard words overwritten"
            if not _fires(gate):
                assert all(same_bits(a, b) for a, b in zip(got, ts)), f"tau={tau} gate={gate}: written although the gate does not fire"
                continue
            if tau == 1.0:
                assert all(same_bits(a, b) for a, b in zip(got, ps))
            r = _figure(ts, ps, tau, gate, got)
            worst = max(worst, r)
            assert r <= 1.0, f"tau={tau} gate={gate}: at {r:.3g} of the bound"
    print(f"\n[kernel against float64, {'views' if views else 'separate'}] largest error / bound: {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", [_lib.TARGET_MAX_PAIRS + 1, 2 * _lib.TARGET_MAX_PAIRS + 10])
def test_more_pairs_than_one_launch(n_pairs):
    """161 and 330 pairs of 1..37 elements in rotation through the operator: the second and third launches of a list see their own
    descriptors (every pair has data of its own)"""
    lib = tm.load()
    sizes = tuple(1 + i % 37 for i in range(n_pairs))
    ts, ps = _inputs(sizes)
    tv, pv = [x.clone().cuda() for x in ts], [x.clone().cuda() for x in ps]
    step = torch.tensor(6.0, dtype=torch.float64, device="cuda")
    target.target_update(lib, tv, pv, 0.3, 4, step)                    # 6 mod 4: not due
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(tv, ts))
    target.target_update(lib, tv, pv, 0.3, 3, step)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(pv, ps))
    r = _figure(ts, ps, 0.3, (6, 3), [v.cpu() for v in tv])
    print(f"\n[{n_pairs} pairs] error / bound: {r:.3g}")
    assert r <= 1.0
    target.target_update(lib, tv, pv, 1.0, 1, None)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(tv, ps))


@pytest.mark.gpu
def test_refusals_write_nothing():
    """every TRUSS_EINVAL case of the header with a canary in every target: the return code, the entry's name in the message, the
    canaries and the sources intact (all refusals come from the host-side check: nothing reaches the device); at the operator a
    non-contiguous and a float64 tensor and unequal sizes; n_pairs = 0 is TRUSS_OK and writes nothing either"""
    lib = tm.load()
    fill = lambda n, dt=torch.float32: torch.full((n,), GUARD, dtype=dt, device="cuda")
    buf = fill(64)
    t, p = [buf[0:8], buf[16:24]], [buf[32:40], buf[48:56]]
    step = torch.tensor(1.0, dtype=torch.float64, device="cuda")
    tp, pp, n8 = [x.data_ptr() for x in t], [x.data_ptr() for x in p], [8, 8]
    call = lambda t_=tp, p_=pp, n_=n8, tau=0.5, period=1, **kw: _c_call(lib, list(t_), list(p_), list(n_), tau, period, step, **kw)
    refused = {
        "struct_size": call(struct_size=C.sizeof(_lib.TargetArgs) - 8),
        "n_pairs < 0": call(n_pairs=-1),
        "NULL pairs": call(null_pairs=True),
        "NULL t": call(t_=[tp[0], None]),
        "NULL p": call(p_=[None, pp[1]]),
        "numel = 0": call(n_=[8, 0]),
        "numel = 2^31": call(n_=[8, 2 ** 31]),
        "tau = 0": call(tau=0.0),
        "tau > 1": call(tau=1.5),
        "tau nan": call(tau=float("nan")),
        "period = 0": call(period=0),
        "a target overlaps its own source": call(p_=[buf[4:12].data_ptr(), pp[1]]),
        "a target overlaps another pair's source": call(p_=[pp[0], buf[7:15].data_ptr()]),
        "a target overlaps another target": call(t_=[tp[0], buf[7:15].data_ptr()]),
        "a target is its source": call(p_=[tp[0], pp[1]]),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    assert b"truss_target_update" in lib.dll.truss_last_error()
    assert call(p_=[pp[0], pp[0]]) == 0                                 # two targets may follow one source
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())                                   # (every element is GUARD: the lerp of equal values changes nothing)
    assert _c_call(lib, [], [], [], 0.5, 1, step) == 0 and _c_call(lib, [], [], [], 0.5, 1, None, null_pairs=True) == 0
    strided = torch.full((8, 2), GUARD, device="cuda")[:, 0]
    with pytest.raises(tm.TrussError, match=r"targets\[1\] must be contiguous"):
        target.target_update(lib, [t[0], strided], p, 0.5)
    with pytest.raises(tm.TrussError, match=r"sources\[1\] must be Float"):
        target.target_update(lib, t, [p[0], fill(8, torch.float64)], 0.5)
    with pytest.raises(tm.TrussError, match="elements"):
        target.target_update(lib, t, [p[0], fill(9)], 0.5)
    with pytest.raises(tm.TrussError, match="sources"):
        target.target_update(lib, t, p[:1], 0.5)
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all()) and bool((strided == GUARD).all())


# ---- on the GPU: the hook ----------------------------------------------------------------------------------------------------------

def _device_kernels(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.gpu
def test_hook_on_a_maddpg_is_two_launches():
    """the hook on the 222 real tensors of a small MADDPG (the targets pulled away from the online weights first): inside the bound,
    and so is the framework path from the same values; one hook call is exactly ceil(222 / 160) = 2 device operations, both
    truss_target_update_kernel; a `train_on_batch` in the default mode issues no such kernel"""
    lib = tm.load()
    prev = RL._TARGET_UPDATE.get("cuda")
    try:
        rl, batches = _maddpg("cuda")
        hook = target.target_hook(lib)
        assert hook is target.target_hook(lib)
        gen = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for t in _targets(rl):
                t.add_((0.05 * torch.randn(t.shape, generator=gen)).cuda())
        t0, p0 = _clone(_targets(rl)), _clone(_online(rl))
        assert len(t0) == 222 and -(-222 // _lib.TARGET_MAX_PAIRS) == 2
        step = torch.tensor(4.0, dtype=torch.float64, device="cuda")
        mine, theirs = _clone(t0), _clone(t0)
        hook(mine, p0, 0.005, 2, step)
        RL._target_update_torch(theirs, p0, 0.005, 2, step)
        torch.cuda.synchronize()
        rh, rt = _figure(t0, p0, 0.005, (4, 2), mine), _figure(t0, p0, 0.005, (4, 2), theirs)
        differ = sum(int((a != b).sum()) for a, b in zip(mine, theirs))
        print(f"\n[hook on 222 tensors] error / bound: hip {rh:.3g}, torch {rt:.3g}; elements that differ between the two: {differ}")
        assert rh <= 1.0 and rt <= 1.0
        names = _device_kernels(lambda: hook(mine, p0, 0.005, 2, step))
        assert len(names) == 2 and all("truss_target_update_kernel" in n for n in names), names
        RL.set_target_update(hook, "cuda")
        assert rl.target_update == "fixed"
        names = _device_kernels(lambda: rl.train_on_batch(*batches[0]))
        assert names and not any("truss_target_update_kernel" in n for n in names)
    finally:
        RL.set_target_update(prev, "cuda")


# ---- on the GPU: the engine --------------------------------------------------------------------------------------------------------

def _engine(lib, target_path, **rl_kw):
    with contextlib.redirect_stdout(io.StringIO()):
        topo = tm.TrussTopology.grid(4)
        torch.manual_seed(5)
        rl = RL.MADDPG(1e-3, M.ep, M.epd, M.gamma, 40, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda", **rl_kw)
        eng = marl.BatchedMARL(topo, 64, rl, max_front=6, lib=lib, device="cuda", replay_capacity=256, batch_size=8, seed=5,
                               target_path=target_path, tune_update_gemms=False)
        b = synthetic.random_batch(topo, 64, 5)
        eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
        eng.game_step_all(train=True, explore=True, update=False)               # fills the replay; no update yet
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    fixed = []
    for _ in range(3):
        S, NS, ag, at, R = eng.replay.sample(eng.batch_size, gen)
        fixed.append((eng._net_state(S), [eng._net_state(ns) for ns in NS], [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)], R))
    rl._ensure_ready(fixed[0][0], [t for a in fixed[0][2] for t in a])
    return rl, eng, fixed


def _hooks():
    return RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda"), RL._OPTIMIZER_STEP.get("cuda"), RL._CRITIC_TAIL.get("cuda"), \
        RL._TARGET_UPDATE.get("cuda")


def _put_back(prev):
    RL.set_level_forward(prev[0], "cuda")
    RL.set_level_backward(prev[1], "cuda")
    RL.set_optimizer_step(prev[2], "cuda")
    RL.set_critic_tail(prev[3], "cuda")
    RL.set_target_update(prev[4], "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["torch", "hip"])
def test_engine_polyak(path):
    """a BatchedMARL engine (TrussTopology.grid(4), 64 envs, hidden 40, batch 8, lr 1e-3, three fixed batches) over a MADDPG with
    target_update="polyak", tau = 0.005, from one start state three updates eagerly and three through the captured graph:
    (a) after the capturing `_train` call the targets reflect exactly ONE update of the start state -- the warm-up's three are
        restored, and `step_t` is 1;
    (b) after every update, eager or replayed, every target is within the bound of the lerp of its previous value and the online
        weights that update left;
    (d) the replayed targets agree with the eager ones within what the bound allows two evaluations from online weights that
        themselves differ by d: allowance_k = (1 - tau) allowance_{k-1} + bound_eager + bound_replay + tau |d_k|;
    (e) a fixed-mode MADDPG started from the same state (a deep copy) has the same critic losses in update 1 and other ones in
        update 2: the TD target reads the moved weights.  (The issue words this as two engines; the mode is the MADDPG's and the
        engine adds nothing to an eager update, so the fixed-mode side is the deep copy driven through `train_on_batch` on the
        polyak engine's own batches -- one start state by construction rather than by two seeded set-ups.)
    Whether the replayed targets equal the eager ones bit for bit is printed; on an MI355X they did, on both paths (profiles/r23/README.md)."""
    lib = tm.load()
    prev = _hooks()
    try:
        rl, eng, fixed = _engine(lib, path, target_update="polyak")
        assert eng.target_path == path and ("cuda" in RL._TARGET_UPDATE) == (path == "hip") and rl.critics_opt.step_t is None
        state = [p for src, dst in _nets(rl) for n in (src, dst) for p in n.parameters()]
        snap, t_snap = _clone(state), _clone(_targets(rl))
        assert all(same_bits(a, b) for a, b in zip(_targets(rl), _online(rl)))  # the initial hard copy
        rl_fixed = copy.deepcopy(rl)
        rl_fixed.target_update = "fixed"

        def run(graph):
            with torch.no_grad():
                for t, v in zip(state, snap):
                    t.copy_(v)
                for t in rl.critics_opt.state_tensors():
                    t.zero_()
            for ag in rl.agents:
                del ag.c_loss[:]
            eng.use_train_graph = graph
            hist = []
            for k, b in enumerate(fixed):
                before = _clone(_targets(rl))
                eng._train(*b)
                torch.cuda.synchronize()
                assert float(rl.critics_opt.step_t) == k + 1
                r = _figure(before, _online(rl), 0.005, None, _targets(rl))
                assert r <= 1.0, f"{'replayed' if graph else 'eager'} update {k + 1}: at {r:.3g} of the bound"
                assert not all(torch.equal(a, b) for a, b in zip(_targets(rl), before))
                hist.append((before, _clone(_online(rl)), _clone(_targets(rl)), r))
            # (a replay runs no host code: only the eager run logs its critic losses)
            return hist, None if graph else [torch.stack([ag.c_loss[k] for ag in rl.agents]).cpu() for k in range(3)]

        eager, loss = run(False)
        replayed, _ = run(True)              # the first call warms up (three updates), captures, restores and replays once
        assert eng._tg is not None, "the update was not captured"
        # (a) is the k = 0 pass through `run`: the bound against the lerp of the START state's targets, and step_t == 1
        assert all(same_bits(a, b) for a, b in zip(replayed[0][0], t_snap))
        cat = lambda ts: torch.cat([f64(t).reshape(-1) for t in ts])
        allow, bitwise = 0.0, True
        for k, ((tb_e, p_e, t_e, _), (tb_r, p_r, t_r, _)) in enumerate(zip(eager, replayed)):
            allow = (1.0 - 0.005) * allow + _bound(cat(tb_e), cat(p_e), 0.005) + _bound(cat(tb_r), cat(p_r), 0.005) + 0.005 * (cat(p_e) - cat(p_r)).abs()
            r = _worst((cat(t_e) - cat(t_r)).abs(), allow)
            bitwise = bitwise and all(same_bits(a, b) for a, b in zip(t_e, t_r))
            assert r <= 1.0, f"update {k + 1}: replayed against eager targets at {r:.3g} of the allowance"
        print(f"\n[engine, polyak, target_path={path}] error / bound: eager {max(h[3] for h in eager):.3g}, replayed {max(h[3] for h in replayed):.3g}; "
              f"replayed targets equal the eager ones bit for bit: {bitwise}")
        # (e)
        for b in fixed[:2]:
            rl_fixed.train_on_batch(*b)
        torch.cuda.synchronize()
        loss_fixed = [torch.stack([ag.c_loss[k] for ag in rl_fixed.agents]).cpu() for k in range(2)]
        assert all(same_bits(a, b) for a, b in zip(_targets(rl_fixed), t_snap))
        torch.testing.assert_close(loss_fixed[0], loss[0], rtol=1e-5, atol=0)
        assert bool((loss_fixed[1] != loss[1]).all()), (loss_fixed[1], loss[1])
        print(f"  critic losses of update 2: fixed {loss_fixed[1].tolist()}, polyak {loss[1].tolist()}")
    finally:
        _put_back(prev)


@pytest.mark.gpu
def test_engine_hard_period_two_in_one_graph():
    """(c) target_update="hard", period 2, target_path="hip", four replays of ONE captured graph: the targets are bitwise unchanged
    after replays 1 and 3 and bitwise equal to the online networks after replays 2 and 4 -- the gate lives on the device"""
    lib = tm.load()
    prev = _hooks()
    try:
        rl, eng, fixed = _engine(lib, "hip", target_update="hard", target_period=2)
        assert "cuda" in RL._TARGET_UPDATE
        graph = None
        for k in range(4):
            before = _clone(_targets(rl))
            eng._train(*fixed[k % 3])
            torch.cuda.synchronize()
            assert eng._tg is not None, "the update was not captured"
            graph = graph or eng._tg[0]
            assert eng._tg[0] is graph and float(rl.critics_opt.step_t) == k + 1
            if k % 2 == 0:
                assert all(same_bits(a, b) for a, b in zip(_targets(rl), before)), f"replay {k + 1} moved the targets"
                assert not all(torch.equal(a, b) for a, b in zip(_targets(rl), _online(rl)))
            else:
                assert all(same_bits(a, b) for a, b in zip(_targets(rl), _online(rl))), f"replay {k + 1} did not copy"
                assert not all(torch.equal(a, b) for a, b in zip(_targets(rl), before))
    finally:
        _put_back(prev)
