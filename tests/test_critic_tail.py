"""`truss_critic_tail` / `truss_critic_tail_backward` (csrc/truss_critic_tail.h): the end of a critic pass of the MADDPG update -- 11 sum
pools, their concatenation, three dense layers -- as native launches: the C entries, `torch.ops.truss_mi355.critic_tail[_backward]`, the
hook `truss2D_RL.set_critic_tail` / `truss_mi355.critic_tail.tail_hook` and BatchedMARL(critic_tail="hip"), against a float64 model of
the arithmetic the header states, stage by stage: every stage from the previous stage's OWN float32 output.

Bounds (derived, not measured; u = 2^-24, gamma_k = k u / (1 - k u); a sum of k terms in any order is within gamma_{k-1} of the sum
of their absolute values, a dot product of k terms within gamma_k, one more for a bias added last):
  p     |p - p64|   <= gamma_{N-1} sum_n |O|                         z1    |z1 - relu(W1 p + b1)| <= gamma_{K1+1} (|W1| |p| + |b1|)
  z2    likewise, k = Q + 1                                          q     likewise, k = Q + 1        (relu does not increase an error)
  dz2   one rounding: u |dq w3|                                      dz1   gamma_Q (|dz2| |W2|)       dp  gamma_Q (|dz1| |W1|)
  d_w1, d_w2, d_w3   gamma_{B+1} sum_b |terms|  (B - 1 additions and the product; one to spare)       d_b1, d_b2, d_b3   gamma_B sum_b |terms|
  d_o   dp copied: every node's row equals dp bit for bit.
relu'(0): where a relu's float64 pre-activation (from the run's own input of that layer) is within its bound of zero, the model takes
the side the float32 run took, nowhere else; at most 2 % of a case's relu elements may be that close.
Inputs: O = relu(randn), Glorot-scaled weights, randn / 10 biases, randn dq, all seeded.
"""
import contextlib
import copy
import ctypes as C
import io

import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import _lib, critic_tail as CT, marl, ops, synthetic
import master_DDPG_truss2D_MO as M
import parity_common as pc
import truss2D_RL as RL
import update_reference as UR

U = 2.0 ** -24
POISON = 12345.0
gamma = lambda k: k * U / (1.0 - k * U)
f64 = lambda t: t.detach().double().cpu()
# (items, B, N, L, H, Q) of the issue; CPU_SHAPES: the ones the float32 restatement runs on the CPU in a second or so
SHAPES = [(1, 1, 1, 1, 4, 1), (3, 5, 12, 11, 40, 40), (1, 7, 33, 11, 72, 24), (2, 3, 64, 11, 200, 200), (1, 2, 66, 3, 24, 8),
          (1, 4, 16, 11, 6, 5), (3, 96, 16, 11, 200, 200), (1, 2, 256, 11, 200, 200)]
CPU_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[4], SHAPES[5], (1, 3, 9, 11, 200, 200)]
MUTANTS = ("mean instead of sum", "no relu mask on dz1", "W2 not transposed in the backward", "b1 dropped", "dp in the wrong layer slot")
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")

# ---- inputs, the float64 model with its bounds, the float32 restatement -----------------------------------------------------------------

_ITEMS = {}


def _item(seed, B, N, L, H, Q):
    """float32 CPU tensors of one item, made once per (seed, shape) and never modified"""
    key = (seed, B, N, L, H, Q)
    if key not in _ITEMS:
        g = torch.Generator().manual_seed(1000 + seed)
        r = lambda *s: torch.randn(*s, generator=g)
        glorot = lambda o, i: r(o, i) * (2.0 / (o + i)) ** 0.5
        _ITEMS[key] = dict(B=B, N=N, L=L, H=H, Q=Q, o=[torch.relu(r(B, N, H)) for _ in range(L)], w1=glorot(Q, L * H), b1=r(Q) / 10,
                           w2=glorot(Q, Q), b2=r(Q) / 10, w3=glorot(1, Q).reshape(Q), b3=r(1) / 10, dq=r(B))
    return _ITEMS[key]


def _items(shape):
    n, B, N, L, H, Q = shape
    return [_item(j, B, N, L, H, Q) for j in range(n)]


def _worst(err, bound):
    """max err / bound (an element whose bound is 0 must be exact)"""
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _figures(it, got, mutant=None):
    """error / bound of every stage present in `got` (float32 results of one item: p, z1, z2, q; dz2, dz1, d_o (list, None: not asked
    for), d_w1 .. d_b3), each stage from got's own previous stage -> (figures, relu elements taken from the float32 run, relu elements).
    mutant: the float64 model is the broken one, the bounds stay those of the correct arithmetic."""
    B, N, L, H, Q = it["B"], it["N"], it["L"], it["H"], it["Q"]
    o, w1, b1, w2, b2, w3, b3, dq = ([f64(t) for t in it["o"]], *(f64(it[k]) for k in PARAMS), f64(it["dq"]))
    fig = {}
    hold = lambda name, x, want, bound: fig.__setitem__(name, _worst((f64(x).reshape(want.shape) - want).abs(), bound))
    stack = torch.stack(o, dim=1)                                              # [B, L, N, H]
    p64 = (stack.mean(dim=2) if mutant == "mean instead of sum" else stack.sum(dim=2)).flatten(1)
    hold("p", got["p"], p64, gamma(N - 1) * stack.abs().sum(dim=2).flatten(1))
    p, z1, z2 = f64(got["p"]), f64(got["z1"]), f64(got["z2"])
    a1 = p @ w1.T + (0.0 if mutant == "b1 dropped" else b1)
    bnd1 = gamma(L * H + 1) * (p.abs() @ w1.abs().T + b1.abs())
    hold("z1", z1, torch.relu(a1), bnd1)
    a2 = z1 @ w2.T + b2
    bnd2 = gamma(Q + 1) * (z1.abs() @ w2.abs().T + b2.abs())
    hold("z2", z2, torch.relu(a2), bnd2)
    hold("q", got["q"], z2 @ w3 + b3, gamma(Q + 1) * (z2.abs() @ w3.abs() + b3.abs()))
    if "dz2" not in got:
        return fig, 0, 2 * B * Q
    # the relu masks: the model's own side, except within the bound of zero, where the float32 run decides
    close1, close2 = a1.abs() <= bnd1, a2.abs() <= bnd2
    m1, m2 = torch.where(close1, z1 > 0, a1 > 0).double(), torch.where(close2, z2 > 0, a2 > 0).double()
    dz2_64 = dq[:, None] * w3[None, :] * m2
    hold("dz2", got["dz2"], dz2_64, U * dz2_64.abs())
    dz2 = f64(got["dz2"])
    dz1_64 = dz2 @ (w2.T if mutant == "W2 not transposed in the backward" else w2) * (1.0 if mutant == "no relu mask on dz1" else m1)
    hold("dz1", got["dz1"], dz1_64, gamma(Q) * (dz2.abs() @ w2.abs()) * m1)
    dz1 = f64(got["dz1"])
    dp64, dp_bound = (dz1 @ w1).view(B, L, H), gamma(Q) * (dz1.abs() @ w1.abs()).view(B, L, H)
    worst = 0.0
    for i, d in enumerate(got["d_o"]):
        if d is not None:
            d = f64(d).view(B, N, H)
            assert torch.equal(d, d[:, :1].expand(B, N, H)), f"d_o[{i}]: the nodes' rows differ"
            slot = (i + 1) % L if mutant == "dp in the wrong layer slot" else i
            worst = max(worst, _worst((d[:, 0] - dp64[:, slot]).abs(), dp_bound[:, i]))
    fig["dp"] = worst
    outer = lambda a, x: (a.T @ x, gamma(B + 1) * (a.abs().T @ x.abs()))
    for name, (want, bound) in (("d_w1", outer(dz1, p)), ("d_b1", (dz1.sum(0), gamma(B) * dz1.abs().sum(0))), ("d_w2", outer(dz2, z1)),
                                ("d_b2", (dz2.sum(0), gamma(B) * dz2.abs().sum(0))), ("d_w3", (dq @ z2, gamma(B + 1) * (dq.abs() @ z2.abs()))),
                                ("d_b3", (dq.sum().reshape(1), gamma(B) * dq.abs().sum().reshape(1)))):
        if got.get(name) is not None:
            hold(name, got[name], want, bound)
    return fig, int(close1.sum() + close2.sum()), 2 * B * Q


def _dot32(w, x):
    """rows of w [R, K] against x [S, K] in the kernels' order, float32: lane l of 64 adds the products of its quads l, l + 64, ...
    in ascending k, the 64 partial sums are added pairwise in six levels -> [S, R]"""
    R, K = w.shape
    t = x[:, None, :] * w[None, :, :]
    pad = (-K) % 256
    t = torch.cat([t, torch.zeros(x.shape[0], R, pad)], dim=2).view(x.shape[0], R, -1, 64, 4)
    acc = torch.zeros(x.shape[0], R, 64)
    for rnd in range(t.shape[2]):
        for j in range(4):
            acc = acc + t[:, :, rnd, :, j]
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def restatement(it, need_o=None):
    """the kernels' arithmetic in float32 torch operations on the CPU (one rounding each, nothing fused) -> the dict `_figures` takes"""
    B, N, L, H, Q = it["B"], it["N"], it["L"], it["H"], it["Q"]
    ps = []
    for o in it["o"]:
        acc = o[:, 0]
        for n in range(1, N):
            acc = acc + o[:, n]
        ps.append(acc)
    p = torch.cat(ps, dim=1)
    z1 = torch.relu(_dot32(it["w1"], p) + it["b1"])
    z2 = torch.relu(_dot32(it["w2"], z1) + it["b2"])
    q = _dot32(it["w3"][None], z2)[:, 0] + it["b3"]
    dq = it["dq"]
    dz2 = torch.where(z2 > 0, dq[:, None] * it["w3"][None, :], torch.zeros(()))
    acc = torch.zeros(B, Q)
    for k in range(Q):
        acc = acc + dz2[:, k, None] * it["w2"][k][None, :]
    dz1 = torch.where(z1 > 0, acc, torch.zeros(()))
    dp = torch.zeros(B, L * H)
    for j in range(Q):
        dp = dp + dz1[:, j, None] * it["w1"][j][None, :]

    def over_b(term):
        acc = torch.zeros_like(term(0))
        for b in range(B):
            acc = acc + term(b)
        return acc

    need_o = [True] * L if need_o is None else need_o
    return dict(p=p, z1=z1, z2=z2, q=q, dz2=dz2, dz1=dz1,
                d_o=[dp[:, i * H:(i + 1) * H][:, None, :].expand(B, N, H).clone() if n else None for i, n in enumerate(need_o)],
                d_w1=over_b(lambda b: dz1[b][:, None] * p[b][None, :]), d_b1=over_b(lambda b: dz1[b]),
                d_w2=over_b(lambda b: dz2[b][:, None] * z1[b][None, :]), d_b2=over_b(lambda b: dz2[b]),
                d_w3=over_b(lambda b: dq[b] * z2[b]), d_b3=over_b(lambda b: dq[b].reshape(1)))


STAGES = {"p", "z1", "z2", "q", "dz2", "dz1", "dp", "d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3"}


def _hold_case(items, gots, title):
    """every stage of every item inside its bound, at most 2 % of the case's relu elements decided by the float32 run"""
    worst, taken, total = {}, 0, 0
    for it, got in zip(items, gots):
        fig, t, n = _figures(it, got)
        taken, total = taken + t, total + n
        for k, r in fig.items():
            worst[k] = max(worst.get(k, 0.0), r)
    print(f"[{title}] largest error / bound: " + ", ".join(f"{k} {r:.2g}" for k, r in worst.items()) +
          f"; relu elements within their bound of zero: {taken} of {total}")
    assert all(r <= 1.0 for r in worst.values()), (title, worst)
    assert taken <= 0.02 * total, f"{title}: {taken} of {total} relu elements within their bound of zero"
    return worst


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------

def test_restatement_stays_inside_the_bounds_and_mutants_do_not():
    """the float32 restatement of the kernels' stated order against the float64 model on CPU_SHAPES: every stage of every item inside
    its bound, at most 2 % of the relu elements within their bound of zero (the float32 run decides their side); every mutant of the
    model at least 10 x outside its bound on at least one case.
    Measured on the CPU: largest error / bound 0.96 for dz2 (a single rounding), 0.64 for dz1 at the one-element shape, 0.62 for d_w1,
    0.55 for q, everything else below 0.5; at most 2 of a case's 1200 relu elements within their bound of zero; the mutants between
    1.9e6 x and infinitely far outside."""
    runs = [(shape, _items(shape)) for shape in CPU_SHAPES]
    runs = [(shape, items, [restatement(it) for it in items]) for shape, items in runs]
    seen = set()
    for shape, items, gots in runs:
        seen |= set(_hold_case(items, gots, f"restatement {shape}"))
    assert seen == STAGES
    for mutant in MUTANTS:
        far = max(max(_figures(it, got, mutant)[0].values()) for _, items, gots in runs for it, got in zip(items, gots))
        print(f"[mutant '{mutant}'] largest error / bound over the cases: {far:.3g}")
        assert far >= 10.0, f"mutant '{mutant}' stays within 10 x the bounds on every case"


def _batch(seed, B, N, P, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g).to(device)
    A = lambda n: torch.softmax(torch.randn(B, n, n, generator=g), -1).to(device)
    a_n, mask = A(N)[:1].expand(B, -1, -1), torch.ones(1, N, N).to(device).expand(B, -1, -1)
    state = lambda: [r(B, N, 13), a_n, A(N), A(N), A(N), mask, r(B, P, 4), A(P)]
    return state(), [state() for _ in range(3)], [(r(B, N, 2), r(B, N, 3)) for _ in range(3)], r(B, 3)


def _maddpg(device, B=5, N=12, P=20, H=40, Cq=8, lr=1e-3):
    torch.manual_seed(5)
    rl = RL.MADDPG(lr, M.ep, M.epd, M.gamma, H, Cq, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)
    batches = [_batch(20 + k, B, N, P, device) for k in range(3)]
    S, NS, A, R = batches[0]
    rl._ensure_ready(S, [t for a in A for t in a])
    return rl, batches


class _Counting(CT.TorchTail):
    def __init__(self):
        self.calls = []

    def forward(self, items, save):
        self.calls.append(("forward", len(items), list(save)))
        return super().forward(items, save)

    def backward(self, items, states, dqs, needs):
        self.calls.append(("backward", len(items), [(sum(a), sum(b)) for a, b in needs]))
        return super().backward(items, states, dqs, needs)


def test_hook_protocol_on_the_cpu(monkeypatch):
    """`set_critic_tail(hook, "cpu")` with the framework-operator hook: three critics through `run_networks` together, trained, frozen
    (differentiated with respect to the action inputs) and under no_grad -- outputs and every gradient `torch.equal` to the unhooked
    generators; the hook is called once per step with three items, saves nothing under no_grad, is asked for the parameters'
    gradients of trained passes only and for six of the eleven level outputs of a frozen one; a critic outside the envelope falls
    back to the present path."""
    assert hasattr(RL, "set_critic_tail")
    rl, batches = _maddpg("cpu")
    S, NS, A, R = batches[0]
    critics = [ag.critic_model for ag in rl.agents]
    acts = lambda: [t.clone().requires_grad_(True) for a in A for t in a]

    def run(kind):
        xs = acts()
        if kind == "no_grad":
            with torch.no_grad():
                return RL.run_networks([RL._critic_steps(c, S + xs) for c in critics]), []
        qs = RL.run_networks([RL._critic_steps(c, S + xs, frozen=(kind == "frozen")) for c in critics])
        wrt = xs if kind == "frozen" else [p for c in critics for p in c.parameters()]
        return qs, torch.autograd.grad(torch.cat(qs, dim=1).pow(2).sum(), wrt, allow_unused=(kind == "frozen"))

    plain = {k: run(k) for k in ("trained", "frozen", "no_grad")}
    hook = _Counting()
    RL.set_critic_tail(hook, "cpu")
    try:
        for kind, (qs0, grads0) in plain.items():
            del hook.calls[:]
            qs, grads = run(kind)
            assert all(torch.equal(a, b) for a, b in zip(qs, qs0)) and len(grads) == len(grads0)
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads, grads0)), kind
            if kind == "no_grad":
                assert hook.calls == [("forward", 3, [False] * 3)]
            elif kind == "trained":
                assert hook.calls == [("forward", 3, [True] * 3), ("backward", 3, [(11, 6)] * 3)]
            else:
                assert hook.calls == [("forward", 3, [True] * 3), ("backward", 3, [(6, 0)] * 3)]
        # outside the envelope: the generator evaluates the tail itself
        del hook.calls[:]
        monkeypatch.setattr(RL, "CRITIC_TAIL_MAX_HIDDEN", 39)
        qs, grads = run("trained")
        assert hook.calls == [] and all(torch.equal(a, b) for a, b in zip(qs + list(grads), plain["trained"][0] + list(plain["trained"][1])))
        monkeypatch.undo()
        # a whole update: the same weights as without the hook, bit for bit
        rl_ref = copy.deepcopy(rl)
        del hook.calls[:]
        rl.train_on_batch(*batches[0])
        assert [c[:2] for c in hook.calls] == [("forward", 3), ("forward", 3), ("backward", 3)] + [("forward", 1), ("backward", 1)] * 3
    finally:
        RL.set_critic_tail(None, "cpu")
    assert "cpu" not in RL._CRITIC_TAIL
    rl_ref.train_on_batch(*batches[0])
    ws = lambda r: [p for ag in r.agents for net in (ag.actor_model, ag.critic_model) for p in net.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(ws(rl), ws(rl_ref)))


def test_plumbing(monkeypatch):
    """the operators are in the table and registered, the argument blocks have the header's sizes; the lane emulator does not export
    the entries: the operators refuse by the names of their symbols, `tail_hook` and BatchedMARL(critic_tail="hip") on that library
    at construction; "torch" is the default, TRUSS_CRITIC_TAIL=hip selects "hip" where the argument is not given"""
    assert {"truss_critic_tail", "truss_critic_tail_backward"} <= set(ops.entries())
    ns = ops.namespace()
    for op in ("critic_tail", "critic_tail_backward"):
        for key in ("CPU", "CUDA", "Meta"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"truss_mi355::{op}", key)
    assert C.sizeof(_lib.CriticTailArgs) == 240 and C.sizeof(_lib.CriticTailBwd) == 408
    assert [n for n, _ in _lib._LATER_ENTRIES][-2:] == ["truss_critic_tail", "truss_critic_tail_backward"]
    emu = pc.emu_lib()
    assert emu.backend == "emu" and not emu.has_critic_tail
    it = _item(0, 2, 3, 2, 4, 3)
    q = torch.full((2, 1), POISON)
    with pytest.raises(tm.TrussError, match="has no truss_critic_tail$"):
        ops.call(ns.critic_tail, ops.bind(emu), 0, it["o"], [2], *([it[k]] for k in PARAMS), [q], [], [], [])
    with pytest.raises(tm.TrussError, match="has no truss_critic_tail_backward$"):
        ops.call(ns.critic_tail_backward, ops.bind(emu), 0, [2], [3], [it["dq"]], [], [torch.zeros(2, 3)], [torch.zeros(2, 3)], [it["w1"]],
                 [it["w2"]], [it["w3"]], [], [], [], [], [], [], [], [], [], [])
    assert bool((q == POISON).all())
    with pytest.raises(tm.TrussError, match="has no truss_critic_tail"):
        CT.tail_hook(emu)
    topo = tm.TrussTopology.grid(4)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, 8, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cpu")
    mk = lambda **kw: marl.BatchedMARL(topo, 2, rl, max_front=6, lib=emu, device="cpu", replay_capacity=8, batch_size=2, **kw)
    monkeypatch.delenv("TRUSS_CRITIC_TAIL", raising=False)
    assert mk().critic_tail == "torch" and mk(critic_tail="torch").critic_tail == "torch"
    with pytest.raises(ValueError, match="has no truss_critic_tail"):
        mk(critic_tail="hip")
    monkeypatch.setenv("TRUSS_CRITIC_TAIL", "hip")
    with pytest.raises(ValueError, match="has no truss_critic_tail"):
        mk()
    assert mk(critic_tail="torch").critic_tail == "torch"
    assert marl._option("critic_tail", None, "TRUSS_CRITIC_TAIL", ("torch", "hip")) == "hip"
    monkeypatch.setenv("TRUSS_CRITIC_TAIL", "1")
    assert mk().critic_tail == "torch"
    with pytest.raises(ValueError, match="critic_tail must be"):
        mk(critic_tail="fused")
    assert "cpu" not in RL._CRITIC_TAIL


# ---- on the GPU: the entries through the operators -------------------------------------------------------------------------------------

def _poison(*shape):
    return torch.full(shape, POISON, device="cuda")


def _run_hip(lib, items, save=None, need_o=None, need_p=None, offset=0):
    """the operators on `items` with poison-filled outputs of the caller's -> the dicts `_figures` takes (what was not asked for:
    None, after checking that its buffer was left alone).  offset: every o[i] and w1 starts that many floats into its allocation."""
    J = len(items)
    save = [True] * J if save is None else save
    need_o = [[True] * it["L"] for it in items] if need_o is None else need_o
    need_p = [[True] * 6 for _ in items] if need_p is None else need_p
    ns, lid, st = ops.namespace(), ops.bind(lib), ops.stream_of(torch.device("cuda"))

    def dev(t):
        buf = torch.empty(t.numel() + offset, device="cuda")
        buf[offset:].copy_(t.reshape(-1))
        return buf[offset:].view(t.shape)

    d = [dict(o=[dev(t) for t in it["o"]], dq=it["dq"].cuda(), **{k: dev(it[k]) if k == "w1" else it[k].cuda() for k in PARAMS}) for it in items]
    keep = [{k: t.clone() for k, t in x.items() if k != "o"} for x in d]
    q = [_poison(it["B"], 1) for it in items]
    st_ = [[_poison(it["B"], it["L"] * it["H"]) for it in items], [_poison(it["B"], it["Q"]) for it in items], [_poison(it["B"], it["Q"]) for it in items]]
    opt = lambda bufs, flags: [b if f else None for b, f in zip(bufs, flags)]
    ops.call(ns.critic_tail, lid, st, [t for x in d for t in x["o"]], [it["L"] for it in items], *([x[k] for x in d] for k in PARAMS), q,
             opt(st_[0], save), opt(st_[1], save), opt(st_[2], save))
    torch.cuda.synchronize()
    gots = []
    for j, it in enumerate(items):
        got = dict(q=q[j].cpu())
        for k, bufs in zip(("p", "z1", "z2"), st_):
            if save[j]:
                got[k] = bufs[j].cpu()
            else:
                assert bool((bufs[j] == POISON).all()), f"item {j}: {k} written without save"
        gots.append(got)
    live = [j for j in range(J) if save[j]]
    if live:
        sub = [items[j] for j in live]
        d_o = [[_poison(it["B"], it["N"], it["H"]) for _ in range(it["L"])] for it in sub]
        dz = [[_poison(it["B"], it["Q"]) for it in sub] for _ in range(2)]
        d_p = [[_poison(*it[k].shape) for it in sub] for k in PARAMS]
        any_p = [any(need_p[j]) for j in live]
        ops.call(ns.critic_tail_backward, lid, st, [it["L"] for it in sub], [it["N"] for it in sub], [d[j]["dq"] for j in live],
                 [st_[0][j] for j in live], [st_[1][j] for j in live], [st_[2][j] for j in live], [d[j]["w1"] for j in live],
                 [d[j]["w2"] for j in live], [d[j]["w3"] for j in live], [t for j in live for t in d[j]["o"]],
                 [b if f else None for bufs, j in zip(d_o, live) for b, f in zip(bufs, need_o[j])], opt(dz[0], any_p), opt(dz[1], any_p),
                 *([b if need_p[j][k] else None for b, j in zip(d_p[k], live)] for k in range(6)))
        torch.cuda.synchronize()
        for n, j in enumerate(live):
            got = gots[j]
            got["d_o"] = [b.cpu() if f else None for b, f in zip(d_o[n], need_o[j])]
            assert all(f or bool((b == POISON).all()) for b, f in zip(d_o[n], need_o[j])), f"item {j}: a d_o nobody asked for was written"
            for k, name in enumerate(PARAMS):
                got["d_" + name] = d_p[k][n].cpu() if need_p[j][k] else None
                assert need_p[j][k] or bool((d_p[k][n] == POISON).all()), f"item {j}: d_{name} written although not asked for"
            if any_p[n]:
                got["dz1"], got["dz2"] = dz[0][n].cpu(), dz[1][n].cpu()
            else:
                assert bool((dz[0][n] == POISON).all() and (dz[1][n] == POISON).all()), f"item {j}: scratch written without launch B"
    for x, k0 in zip(d, keep):
        assert all(torch.equal(x[k], v) for k, v in k0.items()), "an input was modified"
    return gots


def _same(a, b):
    return all((x is None and y is None) or (isinstance(x, list) and all((s is None and t is None) or torch.equal(s, t) for s, t in zip(x, y)))
               or (torch.is_tensor(x) and torch.equal(x, y)) for x, y in ((a[k], b[k]) for k in a))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_float64(shape):
    """forward with save and the full backward through the operators on the issue's shapes, every stage inside its bound of the float64
    model from the kernels' own previous stage, at most 2 % of the relu elements within their bound of zero; inputs untouched; a
    second call gives equal bits; with every o[i] and w1 one float off the 16-byte grid (the word path) the bounds hold as well.
    Measured on an MI355X (profiles/r20/critic_tail_tests.txt): largest error / bound dz2 0.99 (a single rounding), d_w1 0.67, dz1 0.64,
    d_w2 0.60, q 0.55, everything else at or below 0.5 -- per shape the CPU restatement's figures to every digit printed, on both
    paths; at most 205 of 115 200 relu elements (the target pass) within their bound of zero."""
    lib = tm.load()
    items = _items(shape)
    first = _run_hip(lib, items)
    _hold_case(items, first, f"kernels {shape}")
    again = _run_hip(lib, items)
    assert all(_same(a, b) for a, b in zip(first, again)), "a second call gives other bits"
    _hold_case(items, _run_hip(lib, items, offset=1), f"kernels {shape}, word path")


@pytest.mark.gpu
def test_mixed_call_leaves_alone_what_nobody_asked_for():
    """one call over three items of different sizes: the second frozen (d_o for six of its eleven layers, no parameter gradient: no
    launch B, its scratch untouched), the third without save (p, z1, z2 untouched, no backward).  Everything asked for is inside its
    bound; the frozen item's d_o equal, bit for bit, those of the same item run with everything asked for (where dz1 is written
    out and held to its bound); every buffer nobody asked for keeps its poison."""
    lib = tm.load()
    items = [_item(3, 5, 12, 11, 40, 40), _item(4, 3, 64, 11, 200, 200), _item(5, 7, 33, 4, 72, 24)]
    six = [False, False, False, False] + [True] * 6 + [False]
    gots = _run_hip(lib, items, save=[True, True, False], need_o=[[True] * 11, six, [True] * 4], need_p=[[True] * 6, [False] * 6, [True] * 6])
    assert "dz1" not in gots[1] and "p" not in gots[2] and "d_o" not in gots[2]
    full = _run_hip(lib, [items[1]])[0]
    _hold_case(items[:1] + [items[1]], [gots[0], full], "mixed call: the trained item, the frozen item run in full")
    assert all((a is None) == (not f) and (a is None or torch.equal(a, b)) for a, b, f in zip(gots[1]["d_o"], full["d_o"], six))
    assert all(torch.equal(gots[1][k], full[k]) for k in ("p", "z1", "z2", "q"))
    saved = _run_hip(lib, [items[2]])[0]                   # the item without save: its q is that of a run that saves
    _hold_case([items[2]], [saved], "mixed call: the third item run with save")
    assert set(gots[2]) == {"q"} and torch.equal(gots[2]["q"], saved["q"])
    # a parameter gradient alone, and more items than one launch takes
    one = _run_hip(lib, [items[0]], need_o=[[False] * 11], need_p=[[False, True, False, False, False, False]])[0]
    assert torch.equal(one["d_b1"], gots[0]["d_b1"]) and one["d_w1"] is None
    many = [_item(j, 2, 5, 3, 8, 6) for j in range(_lib.CRITIC_TAIL_MAX + 2)]
    _hold_case(many, _run_hip(lib, many), f"{len(many)} items: two launches per entry")


def _c_forward(lib, it, dev, out, **over):
    a = _lib.CriticTailArgs()
    a.struct_size = C.sizeof(_lib.CriticTailArgs)
    a.n_batch, a.n_nodes, a.n_layers, a.n_hidden, a.n_q, a.save = it["B"], it["N"], it["L"], it["H"], it["Q"], 1
    for i in range(min(it["L"], 16)):
        a.o[i] = dev["o"][i % len(dev["o"])].data_ptr()
    for k in PARAMS:
        setattr(a, k, dev[k].data_ptr())
    a.q, a.p, a.z1, a.z2 = (out[k].data_ptr() for k in ("q", "p", "z1", "z2"))
    for k, v in over.items():
        setattr(a, k, v)
    rc = lib.dll.truss_critic_tail(C.byref(a), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
def test_refusals_write_nothing():
    """the C entries: L = 17, Q = 257 and L H = 4100 are TRUSS_EUNSUPPORTED; a NULL w1, a bad struct_size, d_o[i] aliasing o[i] or another
    input of the call and an output overlapping another are TRUSS_EINVAL; nothing is written.  n_items = 0 and n_batch = 0 are TRUSS_OK and
    write nothing either; the operator refuses a float64 and a non-contiguous tensor."""
    lib = tm.load()
    it = _item(0, 2, 3, 2, 4, 3)
    dev = dict(o=[t.cuda() for t in it["o"]], **{k: it[k].cuda() for k in PARAMS})
    big = {k: torch.zeros(n, device="cuda") for k, n in (("w1", 257 * 4100), ("b1", 257), ("w2", 257 * 257), ("b2", 257), ("w3", 257), ("b3", 1))}
    out = {k: _poison(4100 * 2) for k in ("q", "p", "z1", "z2")}
    shape = lambda **kw: dict(it, **kw)
    codes = {
        "L = 17": _c_forward(lib, shape(L=17), dict(dev, **big), out),
        "Q = 257": _c_forward(lib, shape(Q=257), dict(dev, **big), out),
        "L H = 4100": _c_forward(lib, shape(L=10, H=410), dict(dev, **big), out),
        "H = 257": _c_forward(lib, shape(H=257), dict(dev, **big), out),
        "NULL w1": _c_forward(lib, it, dev, out, w1=None),
        "struct_size": _c_forward(lib, it, dev, out, struct_size=C.sizeof(_lib.CriticTailArgs) - 8),
        "q overlaps p": _c_forward(lib, it, dev, out, q=out["p"].data_ptr() + 4),
        "p is o[0]": _c_forward(lib, it, dev, out, p=dev["o"][0].data_ptr()),
    }
    assert codes == {"L = 17": -2, "Q = 257": -2, "L H = 4100": -2, "H = 257": -2, "NULL w1": -1, "struct_size": -1, "q overlaps p": -1,
                     "p is o[0]": -1}, codes
    assert b"truss_critic_tail" in lib.dll.truss_last_error()
    assert _c_forward(lib, shape(B=0), dev, out) == 0
    assert lib.dll.truss_critic_tail(None, 0, None) == 0 and lib.dll.truss_critic_tail_backward(None, 0, None) == 0
    # the backward
    z = torch.rand(2, 3, device="cuda")
    dq, d_o = torch.rand(2, device="cuda"), _poison(2, 3, 4)
    b = _lib.CriticTailBwd()
    b.struct_size = C.sizeof(_lib.CriticTailBwd)
    b.n_batch, b.n_nodes, b.n_layers, b.n_hidden, b.n_q, b.dq_stride = 2, 3, 2, 4, 3, 1
    b.dq, b.p, b.z1, b.z2, b.w1, b.w2, b.w3 = (t.data_ptr() for t in (dq, out["p"], z, z, dev["w1"], dev["w2"], dev["w3"]))
    call = lambda: (lib.dll.truss_critic_tail_backward(C.byref(b), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)), torch.cuda.synchronize())[0]
    w1_0, o_0 = dev["w1"].clone(), dev["o"][0].clone()
    b.d_o[0] = dev["w1"].data_ptr()
    assert call() == -1                                    # d_o[0] aliases w1
    b.o[0], b.d_o[0] = dev["o"][0].data_ptr(), dev["o"][0].data_ptr()
    assert call() == -1                                    # d_o[0] aliases o[0], which the forward pooled
    b.d_o[0], b.d_o[1] = d_o.data_ptr(), d_o.data_ptr() + 16
    assert call() == -1                                    # two outputs overlap
    b.d_o[1], b.d_b1 = None, out["z1"].data_ptr()
    assert call() == -1                                    # a parameter gradient without the scratch
    b.d_b1, b.struct_size = None, 8
    assert call() == -1
    b.struct_size, b.n_layers = C.sizeof(_lib.CriticTailBwd), 17
    assert call() == -2
    b.n_layers, b.dq_stride = 2, -1
    assert call() == -1
    b.dq_stride, b.d_o[0] = 1, None
    assert call() == 0                                     # nothing asked for: nothing launched
    assert b"truss_critic_tail_backward" in lib.dll.truss_last_error()
    ns, lid = ops.namespace(), ops.bind(lib)
    args = lambda **kw: [kw.get("o", dev["o"]), [2]] + [[kw.get(k, dev[k])] for k in PARAMS] + [[out["q"][:2]], [], [], []]
    with pytest.raises(tm.TrussError, match="Float"):
        ops.call(ns.critic_tail, lid, 0, *args(w2=dev["w2"].double()))
    with pytest.raises(tm.TrussError, match="contiguous"):
        ops.call(ns.critic_tail, lid, 0, *args(o=[dev["o"][0], torch.rand(2, 4, 3, device="cuda").transpose(1, 2)]))
    with pytest.raises(tm.TrussError, match=r"w1 must be \[Q, L H\]"):
        ops.call(ns.critic_tail, lid, 0, *args(w1=dev["w1"][:, :7].contiguous()))
    torch.cuda.synchronize()
    assert all(bool((t == POISON).all()) for t in list(out.values()) + [d_o]) and torch.equal(dev["w1"], w1_0) and torch.equal(dev["o"][0], o_0)


# ---- on the GPU: the update with the option --------------------------------------------------------------------------------------------

def _device_kernels(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.gpu
@pytest.mark.parametrize("hip_backward", [True, False], ids=["level_backward=hip", "level_backward=library"])
@pytest.mark.parametrize("case", ["5x12", "3x64", "2x66"])
def test_update_stage_by_stage_against_float64(case, hip_backward, monkeypatch):
    """three eager updates with the level hooks and the tail hook installed, at (B, N, P, H) = (5, 12, 20, 40), (3, 64, 50, 200) and
    (2, 66, 6, 24) of tests/test_update_float64.py, teacher-forced against `update_reference.Update64` with that file's machinery: every
    layer output, loss and gradient within 4 x what the default path (no hook at all) reaches from the same snapshots, capped at 1e-5
    (outputs, losses) and 1e-4 (gradients); clip and optimiser inside their derived bounds.  The tail hook served every critic pass
    (nine per update, in five calls) -- at N = 66 too, where both level hooks hand every level back to the library path."""
    import test_update_float64 as TU
    lib = tm.load()
    rl, batches = TU._setup(case, "cuda")
    rl_lib = copy.deepcopy(rl)
    spies = TU._Spies(monkeypatch)
    entry = spies.watch(rl)
    inner, served = CT.tail_hook(lib), []

    class Logged:
        def forward(self, items, save):
            served.append(len(items))
            return inner.forward(items, save)

        backward = staticmethod(inner.backward)

    prev = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda"), RL._CRITIC_TAIL.get("cuda")
    RL.set_level_forward(marl.level_forward(lib), "cuda")
    RL.set_level_backward(marl.level_backward(lib) if hip_backward else None, "cuda")
    RL.set_critic_tail(Logged(), "cuda")
    try:
        recs = TU._run_updates(entry, batches)
        n_served = list(served)
        RL.set_level_forward(None, "cuda")
        RL.set_level_backward(None, "cuda")
        RL.set_critic_tail(None, "cuda")
        libs = TU._library_records(spies, rl_lib, recs, batches)
    finally:
        RL.set_level_forward(prev[0], "cuda")
        RL.set_level_backward(prev[1], "cuda")
        RL.set_critic_tail(prev[2], "cuda")
    assert n_served == [3, 3, 1, 1, 1] * 3 and served == n_served
    names, title = UR.names_of(rl), f"critic tail, {case}, {'hip' if hip_backward else 'library'} level backward"
    batches64 = [UR.batch64(b) for b in batches]
    ref = TU._staged(UR.Update64(rl.gamma, TU.LR), recs, batches64, names)
    fig, zeros = TU._ratios(ref, recs, names)
    lib_ref = TU._staged(UR.Update64(rl.gamma, TU.LR), libs, batches64, names)
    lib_fig, _ = TU._ratios(lib_ref, libs, names)
    fig["out"], fig["clip"], fig["opt"], lib_fig["out"] = ref["out"], ref["clip"], ref["opt"], lib_ref["out"]
    assert ref["signs"][1] == 0 and lib_ref["signs"][1] == 0
    TU._report(f"{title}: default path against float64", lib_fig)
    TU._report(f"{title}: update under test against float64", fig)
    assert not zeros
    TU._assert_within(fig, TU._taus(lib_fig, title), title)


def _engine(lib, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        topo = tm.TrussTopology.grid(4)
        torch.manual_seed(5)
        rl = RL.MADDPG(1e-3, M.ep, M.epd, M.gamma, 40, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda")
        eng = marl.BatchedMARL(topo, 64, rl, max_front=6, lib=lib, device="cuda", replay_capacity=256, batch_size=8, seed=5, **kw)
        b = synthetic.random_batch(topo, 64, 5)
        eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
        eng.game_step_all(train=True, explore=True, update=False)           # fills the replay; no update yet
    return rl, eng


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer_path", ["torch", "hip"])
@pytest.mark.parametrize("level_backward", ["library", "hip"])
def test_engine_with_the_option(level_backward, optimizer_path):
    """two BatchedMARL engines (64 envs, hidden 40, lr 1e-3, batch 8) that differ only in critic_tail, from equal weights and batches,
    for both level backwards and both optimiser paths: the option installs and removes the hook; an eager update with it is five
    truss_critic_tail_kernel launches, four of launch A and one of launch B, and fewer device kernels than without; weights after three
    eager updates agree at rtol 1e-4 (atol 2e-6, as test_optim_step compares two update paths); the captured update, replayed three
    times from the same snapshot, gives the eager run's weights bit for bit."""
    lib = tm.load()
    prev = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda"), RL._OPTIMIZER_STEP.get("cuda"), RL._CRITIC_TAIL.get("cuda")
    weights = lambda rl: [p for ag in rl.agents for net in (ag.actor_model, ag.critic_model) for p in net.parameters()]
    try:
        eager, launches = {}, {}
        for path in ("torch", "hip"):
            rl, eng = _engine(lib, level_backward=level_backward, optimizer_path=optimizer_path, critic_tail=path)
            assert eng.critic_tail == path and ("cuda" in RL._CRITIC_TAIL) == (path == "hip")
            gen = torch.Generator(device="cuda")
            gen.manual_seed(1)
            fixed = []
            for _ in range(3):
                S, NS, ag, at, R = eng.replay.sample(eng.batch_size, gen)
                fixed.append((eng._net_state(S), [eng._net_state(ns) for ns in NS], [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)], R))
            eng.use_train_graph = False
            eng._train(*fixed[0])                                                  # one eager update: the optimiser has a state
            torch.cuda.synchronize()
            own = UR.tensors_of(rl)
            state = [t for k in UR.KINDS for ts in own[k] for t in ts] + rl.critics_opt.state_tensors()
            snap = [t.detach().clone() for t in state]

            def run(graph):
                with torch.no_grad():
                    for t, v in zip(state, snap):
                        t.copy_(v)
                eng.use_train_graph = graph
                for b_ in fixed:
                    eng._train(*b_)
                torch.cuda.synchronize()
                return [p.detach().clone() for p in weights(rl)]

            replayed = run(True)                                   # warm-up (the library GEMMs are chosen here), capture, three replays
            assert eng._tg is not None, "the update was not captured"
            eager[path] = run(False)
            differ = [float((a - b).abs().max()) for a, b in zip(replayed, eager[path]) if not torch.equal(a, b)]
            print(f"\n[engine, critic_tail={path}] weight tensors that differ between replay and eager: {len(differ)} of {len(replayed)}"
                  + (f", by at most {max(differ):.3g}" if differ else ""))
            if path == "hip":
                assert not differ, "the replayed update differs from the eager one"
            names = _device_kernels(lambda: eng._train(*fixed[0]))
            launches[path] = (len(names), [sum(k in n for n in names) for k in ("truss_critic_tail_kernel", "truss_critic_tail_bwd_kernel",
                                                                                "truss_critic_tail_bwd_params_kernel")])
        print(f"\n[engine, level_backward={level_backward}, optimizer_path={optimizer_path}] device kernels per eager update: "
              f"torch {launches['torch'][0]}, hip {launches['hip'][0]}")
        assert launches["torch"][1] == [0, 0, 0] and launches["hip"][1] == [5, 4, 1]
        assert launches["hip"][0] < launches["torch"][0]
        for p, q in zip(eager["hip"], eager["torch"]):
            torch.testing.assert_close(p, q, rtol=1e-4, atol=2e-6)
    finally:
        RL.set_level_forward(prev[0], "cuda")
        RL.set_level_backward(prev[1], "cuda")
        RL.set_optimizer_step(prev[2], "cuda")
        RL.set_critic_tail(prev[3], "cuda")
