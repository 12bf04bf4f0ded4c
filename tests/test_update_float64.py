"""The MADDPG update (`truss2D_RL.MADDPG.train_on_batch`) stage by stage against the float64 host model of tests/update_reference.py:
on the CPU (float32 library GEMMs; this validates the host model where there is no GPU), on the GPU through the level kernels
(`marl.level_forward`, `marl.level_backward`) and as the hipGraph `BatchedMARL._train` replays.

The comparison is teacher-forced.  Spies on `rl.critics_opt.step` and on `truss2D_RL._fresh_adam_step` (both looked up at call time
by the eager update) snapshot, before calling through, the networks' parameters, the optimiser's state, every `p.grad` of the
network being stepped (the unclipped gradient: the update clips a flat copy) and the flat gradient handed in.  From each snapshot,
cast to float64, the host model evaluates that stage alone, so an error is named by the first stage and tensor outside its bound.
A wrapper around `truss2D_RL.gcn_level` (looked up at call time by `run_networks`) keeps every layer's output of every stage:

  outputs     every GCN layer of every network a stage evaluates, ||out - out64|| / ||out64||           <= tau(out)
              (the forward half of every stage; needed besides the losses and gradients: the gradient of actor 1 does not
              depend on WHICH actor 0 the critic saw unless a relu of the critic's dense head changes side -- the three action
              branches meet only there -- so the mutant "actor 1 sees the un-stepped actor 0" shows in the forward half alone)
  losses      c_loss[-1] of each agent, |l - l64| / |l64|                                            <= tau(loss)
  gradients   every parameter tensor of the three critics, and of actor i at its own stage,
              ||g - g64|| / ||g64||   (the TD stage enters through y in the critics' losses and gradients) <= tau(critic / actor gradient)
  clip        the flat gradient the optimiser received against the float64 clip of the update's OWN unclipped p.grad, per tensor
              ||c - c64|| / ||c64|| <= ((n + 1) / 2 + 4) u: a float32 sum of n squares in any order is within (n - 1) u of its value,
              the squares add u, the square root halves that and adds a rounding of its own, and + 1e-12, the reciprocal and the
              product add one each (u = 2^-24; n = the tensor's size)
  optimiser   weights (critics: and both moments) after the step against the float64 step applied to the update's OWN pre-step
              weights, moments and clipped gradient -- the Adam arithmetic alone, element by element, see `_adam_bounds`

tau(out), tau(loss), tau(critic gradient), tau(actor gradient) are measured per shape in the test itself: 4 x the largest ratio the
float32 library path (the same stage from the same snapshot with both hooks removed and no optimiser step taken: `torch.bmm`)
reaches against float64 -- the margin tests/test_gcn_level_backward.py gives the kernels over the library, for a different but
equally valid summation order -- and never above 1e-4 (gradients) / 1e-5 (losses, outputs).  No tensor is left out: no float64
gradient tensor may be exactly zero.

relu'(0).  A pre-activation that is zero to within float32 rounding comes out on either side of zero, and one such element moves a
row of its kernel's gradient by about 1e-3 of the tensor (seen at 3x64 on the CPU before this was handled: ratio 1.3e-3 for the two
tensors of one layer, 3e-7 for every other).  The model therefore takes the sign the float32 run had for the elements inside the
band of float32 rounding around zero, keeps its own everywhere else, and counts both; a disagreement OUTSIDE the band fails the
test (update_reference.Net).  The library path's figures are taken against the model with the library's own signs.

Shapes (B, N, P, H, critic width): the smallest at which the level kernels' tiling has its edges.
  5x12   (5, 12, 20, 40, 8)    N does not divide the 128-row tile (10 graphs, 120 live rows), B below one tile, 3 B = 15 a full tile
                               and a tail tile, C = 40 leaves a column block of 8, K = 40 a partial slab
  7x33   (7, 33, 6, 72, 24)    odd N (3 graphs per tile, 99 live rows), a tail tile of one graph, K = 72: 8 k's in a second slab
  3x64   (3, 64, 50, 200, 64)  N at the envelope's limit (2 graphs per tile, a tail of one), a 50-member front, the project's hidden
                               width 200 = 3 x 64 + 8
  2x66   (2, 66, 6, 24, 8)     N > 64: both hooks hand back every level that holds an N-node group -- in this update that is every
                               level (the front's layers share their level with N-node ones), so the update runs on the library path
                               with the hooks installed
  5x12-materialised            the first shape with per-sample adjacencies and masks (the others pass ONE shared adjacency and ONE
                               mask, stride 0 over the batch, the same tensors in S and the three NS, as the engine hands them over)
Three updates on three batches at lr 1e-3: the online networks leave their targets, Adam runs at t = 2 and t = 3.

Measured (largest ratios over the three updates; the full -s output of the GPU tests on an MI355X is profiles/r13/update_float64_tests.txt):
see the docstrings of the tests.
"""
import contextlib
import copy
import io

import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import marl, synthetic
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL
import update_reference as UR

LR = 1e-3
U = 2.0 ** -24
CAPS = {"loss": 1e-5, "out": 1e-5, "cgrad": 1e-4, "agrad": 1e-4}
CASES = {"5x12": (5, 12, 20, 40, 8, True), "7x33": (7, 33, 6, 72, 24, True), "3x64": (3, 64, 50, 200, 64, True),
         "2x66": (2, 66, 6, 24, 8, True), "5x12-materialised": (5, 12, 20, 40, 8, False)}


# ---- set-up: the networks, the batches, the spies -----------------------------------------------------------------------------------

def _batch(seed, B, N, P, device, shared):
    """a minibatch (S, NS, A, R) as tests/test_gcn_level_backward._gpu_batch builds it; shared: the adjacency A_n and the mask are
    ONE tensor each, expanded over the batch (stride 0), and the same tensor in S and in the three NS"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g).to(device)
    A = lambda n: torch.softmax(torch.randn(B, n, n, generator=g), -1).to(device)
    if shared:
        a_n, mask = A(N)[:1].expand(B, -1, -1), torch.ones(1, N, N).to(device).expand(B, -1, -1)
        state = lambda: [r(B, N, 13), a_n, A(N), A(N), A(N), mask, r(B, P, 4), A(P)]
    else:
        state = lambda: [r(B, N, 13), A(N), A(N), A(N), A(N), torch.ones(B, N, N).to(device), r(B, P, 4), A(P)]
    return state(), [state() for _ in range(3)], [(r(B, N, 2), r(B, N, 3)) for _ in range(3)], r(B, 3)


def _setup(case, device):
    B, N, P, H, C, shared = CASES[case]
    torch.manual_seed(5)
    rl = RL.MADDPG(LR, M.ep, M.epd, M.gamma, H, C, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)
    batches = [_batch(20 + k, B, N, P, device, shared) for k in range(3)]
    S, NS, A, R = batches[0]
    if shared:
        assert S[1].stride(0) == 0 and S[5].stride(0) == 0 and all(ns[1].data_ptr() == S[1].data_ptr() for ns in NS)
    rl._ensure_ready(S, [t for a in A for t in a])
    return rl, batches


def _snap(rl, kinds=UR.KINDS):
    return {k: [[p.detach().clone() for p in ps] for ps in v] for k, v in UR.tensors_of(rl).items() if k in kinds}


def _load(rl, snap):
    own = UR.tensors_of(rl)
    with torch.no_grad():
        for k, per_agent in snap.items():
            for ts, vs in zip(own[k], per_agent):
                for t, v in zip(ts, vs):
                    t.copy_(v)


class _Spies:
    """records of the updates of the watched MADDPG objects, one dict per update:
         pre (all twelve networks), opt_pre, grads (per critic, unclipped), flat (clipped), post / opt_post (after the step),
         actors: per stage  pre (actors and critics: the targets never change), grads, flat, post
       step=False: the optimiser steps are recorded but NOT taken (a stage evaluated from a loaded snapshot, nothing moves)"""

    def __init__(self, monkeypatch):
        self.mp, self.watched, self.fresh, self.level, self.layers = monkeypatch, [], RL._fresh_adam_step, RL.gcn_level, {}
        monkeypatch.setattr(RL, "_fresh_adam_step", self._actor_step)
        monkeypatch.setattr(RL, "gcn_level", self._level)         # (`run_networks` looks it up at call time)

    def _level(self, reqs, cache=None):
        """the level operation, whatever evaluates it: every layer's output, per stage and network"""
        res = self.level(reqs, cache)
        for (layer, _, _, act), o in zip(reqs, res):
            hit = self.layers.get(layer.lin.weight.data_ptr())
            if hit is not None:
                entry, kind, agent, name = hit
                entry["seen"].setdefault((kind, agent), {})[name] = o.detach().cpu()
        return res

    def watch(self, rl, step=True):
        entry = dict(rl=rl, step=step, recs=[], seen={})
        self.watched.append(entry)
        for kind, attr in zip(UR.KINDS, UR.ATTRS):
            for agent, ag in enumerate(rl.agents):
                for name, p in getattr(ag, attr).named_parameters():
                    if name.endswith(".lin.weight"):
                        self.layers[p.data_ptr()] = (entry, kind, agent, name[:-len(".lin.weight")])
        opt = rl.critics_opt
        orig = opt.step

        def critic_step(flat_grad=None):
            rec = dict(pre=_snap(rl), opt_pre=[t.clone() for t in opt.state_tensors()], flat=flat_grad.clone(), actors=[],
                       grads=[[p.grad.clone() for p in ps] for ps in UR.tensors_of(rl)["critic"]], seen=entry["seen"])
            entry["seen"] = {}
            entry["recs"].append(rec)
            if entry["step"]:
                orig(flat_grad)
                rec["post"], rec["opt_post"] = _snap(rl, ("critic",))["critic"], [t.clone() for t in opt.state_tensors()]

        self.mp.setattr(opt, "step", critic_step, raising=False)
        return entry

    def _actor_step(self, params, lr, eps, flat_grad=None):
        for e in self.watched:
            for i, ag in enumerate(e["rl"].agents):
                if params[0] is next(iter(ag.actor_model.parameters())):
                    rec = dict(agent=i, pre=_snap(e["rl"], ("actor", "critic")), grads=[p.grad.clone() for p in params],
                               flat=flat_grad.clone(), lr=lr, eps=eps, seen=e["seen"])
                    e["seen"] = {}
                    e["recs"][-1]["actors"].append(rec)
                    if e["step"]:
                        self.fresh(params, lr, eps, flat_grad)
                        rec["post"] = [p.detach().clone() for p in params]
                    return
        return self.fresh(params, lr, eps, flat_grad)


def _run_updates(entry, batches):
    rl = entry["rl"]
    for b in batches:
        rl.train_on_batch(*b)
        entry["recs"][-1]["loss"] = [ag.c_loss[-1].clone() for ag in rl.agents]
    assert len(entry["recs"]) == len(batches) and all([a["agent"] for a in r["actors"]] == [0, 1, 2] for r in entry["recs"])
    return entry["recs"]


def _library_records(spies, rl_lib, recs, batches):
    """every stage again, from the snapshot it started from, by `rl_lib` (a copy of the networks) with NO hook installed and no
    optimiser step taken: the float32 library path's losses and gradients for the same stage"""
    e = spies.watch(rl_lib, step=False)
    out = []
    for rec, b in zip(recs, batches):
        _load(rl_lib, rec["pre"])
        rl_lib.train_on_batch(*b)
        mine = e["recs"][-1]
        lib = dict(pre=rec["pre"], loss=[ag.c_loss[-1].clone() for ag in rl_lib.agents], grads=mine["grads"], seen=mine["seen"], actors=[])
        for i, arec in enumerate(rec["actors"]):
            _load(rl_lib, arec["pre"])
            rl_lib.train_on_batch(*b)
            mine = e["recs"][-1]["actors"][i]
            lib["actors"].append(dict(pre=arec["pre"], grads=mine["grads"], seen=mine["seen"]))
        out.append(lib)
        del e["recs"][:]
    return out


# ---- the staged float64 values, the bounds of the optimiser arithmetic, the ratios ------------------------------------------------

def _cat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _worst(err, bound):
    """max err / bound (an element whose bound is 0 must be exact)"""
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _adam_bounds(exact, w, m, v, g, t):
    """element-wise bounds of the float32 SharedStepAdam step against the float64 step from the same float32 w, m, v, g.
    u = 2^-24 bounds the relative error of a correctly rounded operation and of a constant's conversion to float32; sqrt, division
    and reciprocal on the device are taken as good to one ulp (2 u).
      m' = lerp(m, g, 1 - b1) = m + (1 - b1) (g - m): the difference, the weight's conversion and the product put 3 u on the term
           (1 - b1) |g - m|, the sum u on |m'|:                             |dm'| <= u (|m'| + 3 (1 - b1) |g - m|)
      v' = v b2 + (1 - b2) g g: 2 u on the first term (conversion, product), 3 u on the second (conversion, two products), both
           non-negative, one more for the sum:                              |dv'| <= 4 u v'
      dw = (-lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps): sqrt(v') carries 4 u / 2 + 2 u = 4 u; / sqrt(bc2) its conversion and the
           division, 3 u; + eps a conversion and a rounding, 2 u; the reciprocal 2 u; times m' one; times the converted scalar two:
           14 u |dw|, and |dm'| scaled like m' itself: u |dw| + 3 u T with T = (lr / bc1) (1 - b1) |g - m| / (sqrt(v') / sqrt(bc2) + eps)
      w' = w + dw: one rounding of the weight:                              |dw'| <= u (|w'| + 15 |dw| + 3 T)
    (to first order in u).  A wrong sign, learning rate, eps or bias correction changes dw by a factor: orders above 15 u |dw|."""
    w2, m2, v2, dw = exact.adam(w, m, v, g, t)
    lead = (1.0 - UR.B1) * (g - m).abs()
    T = exact.lr / (1.0 - UR.B1 ** t) * lead / (v2.sqrt() / (1.0 - UR.B2 ** t) ** 0.5 + UR.EPS)
    return {"w": U * (w2.abs() + 15.0 * dw.abs() + 3.0 * T), "m": U * (m2.abs() + 3.0 * lead), "v": 4.0 * U * v2}


def _fresh_bound(exact, w, g):
    """the fresh Adam's first step p += -lr' g / (|g| + eps) in float32: + eps a conversion and a rounding (2 u), the division 2 u,
    the converted factor -lr' and its product 2 u, the final sum u on the weight and u on the term: |dw'| <= u (|w'| + 7 |dw|)"""
    w2, dw = exact.fresh_adam(w, g)
    return U * (w2.abs() + 7.0 * dw.abs())


def _clip_figures(out, labels, own, clipped64, flat):
    k = 0
    for label, g, c64 in zip(labels, own, clipped64):
        n = g.numel()
        c = flat[k:k + n].view_as(g)
        k += n
        bound = ((n + 1) / 2.0 + 4.0) * U * float(c64.norm())
        err = float((c - c64).norm())
        out.append((label, err / bound if bound > 0 else (float("inf") if err > 0 else 0.0)))
    assert k == flat.numel()


def _staged(model, recs, batches64, names):
    """the host model's value of every stage of every recorded update, each from the update's own state at that moment:
    {"loss": [u] tensor [3], "cgrad": [u][i][k], "agrad": [u][i][k], "clip": [(label, error / bound)], "opt": [(label, error / bound)]}"""
    exact = UR.Update64(model.gamma, model.lr)             # the bounds are those of the correct arithmetic, whatever `model` is
    ref = dict(loss=[], out=[], cgrad=[], agrad=[], clip=[], opt=[])

    def outputs(stage):
        ref["out"] += [(f"update {u} {stage} {label}", r) for label, r in model.take_outputs()]

    for u, (rec, (S, NS, A, R)) in enumerate(zip(recs, batches64)):
        P = UR.params64(names, rec["pre"])
        losses, cg = model.critic_stage(P, S, A, model.td_target(P, NS, R, rec["seen"]), rec["seen"])
        outputs("TD+critics")
        ref["loss"].append(losses)
        ref["cgrad"].append([[g[n] for n in names["critic"]] for g in cg])
        ref["agrad"].append([])
        if "flat" not in rec:                              # the library path's records: losses and gradients only
            for i, arec in enumerate(rec["actors"]):
                _, ag = model.actor_stage(UR.params64(names, arec["pre"]), S, i, None, arec["seen"])
                outputs(f"actor{i}")
                ref["agrad"][-1].append([ag[n] for n in names["actor"]])
            continue
        own = [UR.f64(g) for gs in rec["grads"] for g in gs]
        flat = UR.f64(rec["flat"])
        _clip_figures(ref["clip"], [f"update {u} critic {i} {n}" for i in range(3) for n in names["critic"]], own, model.clip(own), flat)
        w = _cat([t for c in P["critic"] for t in c.values()])
        t0, m, v = (float(rec["opt_pre"][0]), UR.f64(rec["opt_pre"][1]), UR.f64(rec["opt_pre"][2])) if rec["opt_pre"] else \
            (0.0, torch.zeros_like(w), torch.zeros_like(w))
        assert t0 == u, "one shared step counter, one step per update"
        w2, m2, v2, _ = model.adam(w, m, v, flat, u + 1)
        bound = _adam_bounds(exact, w, m, v, flat, u + 1)
        got = {"w": _cat([UR.f64(t) for c in rec["post"] for t in c]), "m": UR.f64(rec["opt_post"][1]), "v": UR.f64(rec["opt_post"][2])}
        assert float(rec["opt_post"][0]) == u + 1
        for q, want in (("w", w2), ("m", m2), ("v", v2)):
            ref["opt"].append((f"update {u} critics {q}", _worst((got[q] - want).abs(), bound[q])))
        stale = {"critic": P["critic"], "actor0": UR.params64(names, rec["actors"][0]["pre"])["actor"][0]}
        for i, arec in enumerate(rec["actors"]):
            Pa = UR.params64(names, arec["pre"])
            _, ag = model.actor_stage(Pa, S, i, stale, arec["seen"])
            outputs(f"actor{i}")
            ref["agrad"][-1].append([ag[n] for n in names["actor"]])
            own = [UR.f64(g) for g in arec["grads"]]
            flat = UR.f64(arec["flat"])
            _clip_figures(ref["clip"], [f"update {u} actor {i} {n}" for n in names["actor"]], own, model.clip(own), flat)
            w = _cat(Pa["actor"][i].values())
            w2, _ = model.fresh_adam(w, flat)
            ref["opt"].append((f"update {u} actor {i} w", _worst((_cat([UR.f64(t) for t in arec["post"]]) - w2).abs(),
                                                                 _fresh_bound(exact, w, flat))))
    ref["signs"] = model.sign_counts()
    return ref


def _ratios(ref, recs, names):
    """-> ({"loss" | "cgrad" | "agrad": [(label, ratio)]}, labels of the float64 gradient tensors that are exactly zero)"""
    out, zeros = dict(loss=[], cgrad=[], agrad=[]), []

    def tensors(q, label, got, want, ns):
        for n, g, g64 in zip(ns, got, want):
            if float(g64.abs().max()) == 0.0:
                zeros.append(f"{label} {n}")
            out[q].append((f"{label} {n}", float((UR.f64(g) - g64).norm() / g64.norm())))

    for u, rec in enumerate(recs):
        for i in range(3):
            l64 = float(ref["loss"][u][i])
            out["loss"].append((f"update {u} critic {i}", abs(float(rec["loss"][i]) - l64) / abs(l64)))
            tensors("cgrad", f"update {u} critic {i}", rec["grads"][i], ref["cgrad"][u][i], names["critic"])
            tensors("agrad", f"update {u} actor {i}", rec["actors"][i]["grads"], ref["agrad"][u][i], names["actor"])
    return out, zeros


def _report(title, fig):
    """the ratios, one line per update and network"""
    print(f"\n[{title}]")
    for q, rows in fig.items():
        groups = {}
        for label, r in rows:
            key = " ".join(label.split(" ")[:4]) if q in ("cgrad", "agrad", "clip", "out") else " ".join(label.split(" ")[:2])
            groups.setdefault(key, []).append(r)
        for key, rs in groups.items():           # (layer outputs and clips: the largest of each network; everything else in full)
            print(f"  {q:5s} {key}: max {max(rs):.3g}  " + (f"of {len(rs)}" if q in ("out", "clip") else "all " + " ".join(f"{r:.1e}" for r in rs)))


def _taus(lib, title):
    tau = {}
    for q, cap in CAPS.items():
        worst = max(r for _, r in lib[q])
        tau[q] = min(4.0 * worst, cap)
        print(f"[{title}] tau({q}) = 4 x {worst:.3g} = {4.0 * worst:.3g} (cap {cap:g}{': BINDS' if 4.0 * worst >= cap else ''})")
    return tau


def _assert_within(fig, tau, title):
    for q, rows in fig.items():
        bound = tau.get(q, 1.0)                     # clip, opt: error / derived bound
        bad = [(label, r) for label, r in rows if not r <= bound]
        assert not bad, f"{title}: {q} outside its bound {bound:.3g}, first: {bad[0][0]} at {bad[0][1]:.3g} ({len(bad)} of {len(rows)})"


_CPU = {}


def _cpu_run(case, monkeypatch):
    """three float32 updates on the CPU, recorded (once per case)"""
    if case not in _CPU:
        rl, batches = _setup(case, "cpu")
        recs = _run_updates(_Spies(monkeypatch).watch(rl), batches)
        _CPU[case] = (recs, [UR.batch64(b) for b in batches], UR.names_of(rl), rl.gamma)
    return _CPU[case]


def _figures(model, recs, batches64, names):
    ref = _staged(model, recs, batches64, names)
    fig, zeros = _ratios(ref, recs, names)
    fig["out"], fig["clip"], fig["opt"] = ref["out"], ref["clip"], ref["opt"]
    return fig, zeros, ref["signs"]


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_host_model_agrees_with_the_cpu_update(case, monkeypatch):
    """float32 `train_on_batch` on the CPU (library GEMMs, no hook) against the host model, stage by stage over three updates: here
    the library path IS the path under test, so what is asserted is that its ratios stay within the caps of tau (1e-5 outputs and losses,
    1e-4 gradients; measured: 4 x to 200 x inside), that the clip and the optimiser arithmetic stay within their derived bounds, that no float64 gradient tensor is
    exactly zero, that the norm clip is active and that Adam ran at t = 2 and 3.
    Largest ratios measured on the CPU (output | loss | critic gradient | actor gradient; clip, optimiser as fractions of their bounds):
      5x12 1.7e-07 | 4.9e-07 | 1.3e-06 | 4.1e-07; 0.20, 0.99      7x33 2.2e-07 | 4.1e-07 | 5.0e-07 | 7.1e-07; 0.20, 0.99
      3x64 2.9e-07 | 2.4e-06 | 2.5e-06 | 4.2e-07; 0.20, 0.99      2x66 2.4e-07 | 1.2e-06 | 9.4e-07 | 3.7e-07; 0.20, 0.98
      5x12-materialised 1.8e-07 | 1.4e-06 | 1.8e-06 | 6.5e-07; 0.16, 0.99
    (the optimiser's bound is dominated by the one rounding of the weight, 2^-24 |w'|, which some element of 10^5 nearly reaches; the
    clip's 0.20 is the one-element bias of the critics' output layer: one rounding against a bound of five).  relu elements whose sign
    was taken from the float32 run: 0, 1, 2, 0, 1 of some 10^5 .. 10^7 per case."""
    recs, batches64, names, gamma = _cpu_run(case, monkeypatch)
    fig, zeros, (taken, conflicts) = _figures(UR.Update64(gamma, LR), recs, batches64, names)
    _report(f"cpu {case}: float32 update against float64", fig)
    print(f"[cpu {case}] relu elements within rounding of zero whose sign was taken from the float32 run: {taken}; disagreements outside the band: {conflicts}")
    assert conflicts == 0
    assert not zeros, f"float64 gradient tensors that are exactly zero (nothing to compare): {zeros}"
    _assert_within(fig, _taus(fig, f"cpu {case}"), f"cpu {case}")
    assert max(float(g.norm()) for rec in recs for gs in rec["grads"] for g in gs) > 1.0          # the clip does scale something
    assert [float(rec["opt_pre"][0]) if rec["opt_pre"] else 0.0 for rec in recs] == [0.0, 1.0, 2.0]
    online, target = recs[-1]["pre"]["critic"][0], recs[-1]["pre"]["tcritic"][0]
    assert any(not torch.equal(a, b) for a, b in zip(online, target))                                # the networks have left their targets


@pytest.mark.parametrize("mutant", UR.MUTANTS)
def test_host_model_mutants_fail(mutant, monkeypatch):
    """the bounds can tell: every mutant of the host model (update_reference.MUTANTS) leaves at least one compared quantity of the
    smallest shape at >= 10 x its tau (tau = 4 x the correct model's largest ratio for losses and gradients, the derived bound for
    the clip and the optimiser arithmetic).  Measured, the worst quantity over its tau: gamma dropped 7.0e+04 (critic gradient),
    / 3 dropped 5.0e+05 (loss), online networks 1.9e+06 (critic gradient), agent order 1.0e+06 (output), pre-step critic 7.9e+05
    (actor gradient), un-stepped actor 0 2.8e+04 (output; the gradients do not move: 0.25), no clip 1.8e+06, one clip 3.6e+08 (clip),
    frozen bias correction 7.4e+05, actors' 0.1 dropped 2.2e+07 (optimiser), sum for mean 4.8e+05 (actor gradient)."""
    recs, batches64, names, gamma = _cpu_run("5x12", monkeypatch)
    good, _, _ = _figures(UR.Update64(gamma, LR), recs, batches64, names)
    tau = {q: min(4.0 * max(r for _, r in good[q]), cap) for q, cap in CAPS.items()}
    bad, _, _ = _figures(UR.Update64(gamma, LR, mutant), recs, batches64, names)
    worst = {q: max(r for _, r in rows) / tau.get(q, 1.0) for q, rows in bad.items()}
    print(f"\n[mutant '{mutant}'] worst ratio / tau: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) >= 10.0, f"mutant '{mutant}' stays within 10 x tau everywhere: {worst}"


# ---- on the GPU, through the level kernels ---------------------------------------------------------------------------------------

def _inside(g, ws):
    return g.shape[1] <= 64 and g.shape[2] <= 256 and ws[g.idx[0]].shape[0] <= 224


def _logged_forward(fn, log):
    """the forward hook with a call log: (groups, groups inside the envelope, want_grad, X' present for every group, handed back?)"""
    def hook(groups, xs, ws, bs, want_grad):
        res = fn(groups, xs, ws, bs, want_grad)
        kept = res is not None and all(x is not None for x in res[1])
        log.append((len(groups), sum(_inside(g, ws) for g in groups), bool(want_grad), kept, res is None))
        return res
    return hook


def _logged_backward(fn, log):
    """the backward hook with a call log: (groups, differentiable groups, groups it returned every gradient for, handed back?)"""
    def hook(groups, douts, outs, xaggs, ws, need):
        L = len(ws)
        res = fn(groups, douts, outs, xaggs, ws, need)
        live = covered = 0
        for gi, g in enumerate(groups):
            nw = any(need[1 + L + i] or need[1 + 2 * L + i] for i in g.idx)
            nx = any(need[1 + i] for i in g.idx)
            if douts[gi] is None or not (nw or nx):
                continue
            live += 1
            if res is not None:
                dx, dw, db = res
                ok = all(dw[i] is not None and db[i] is not None for i in g.idx) if nw else True
                covered += bool(ok and (all(dx[i] is not None for i in g.idx) if nx else True))
        log.append((len(groups), live, covered, res is None))
        return res
    return hook


def _gpu_update(case, hip_backward, monkeypatch):
    B, N, P, H, C, shared = CASES[case]
    lib = tm.load()
    rl, batches = _setup(case, "cuda")
    rl_lib = copy.deepcopy(rl)
    spies = _Spies(monkeypatch)
    entry = spies.watch(rl)
    flog, blog = [], []
    prev = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda")
    RL.set_level_forward(_logged_forward(marl.level_forward(lib), flog), "cuda")
    RL.set_level_backward(_logged_backward(marl.level_backward(lib), blog) if hip_backward else None, "cuda")
    try:
        recs = _run_updates(entry, batches)
        n_f, n_b = len(flog), len(blog)
        RL.set_level_forward(None, "cuda")
        RL.set_level_backward(None, "cuda")
        libs = _library_records(spies, rl_lib, recs, batches)
    finally:
        RL.set_level_forward(prev[0], "cuda")
        RL.set_level_backward(prev[1], "cuda")
    assert n_f > 0 and len(flog) == n_f and len(blog) == n_b                 # the hooks ran, and not for the library's figures
    if N <= 64:
        # every group inside the envelope: no level handed back; the passes without a graph ran with X' absent, the others kept it
        assert all(inside == n and not back for n, inside, _, _, back in flog), flog
        assert any(not want for _, _, want, _, _ in flog) and all(kept == want for _, _, want, kept, _ in flog), flog
    else:
        assert all(inside < n and back for n, inside, _, _, back in flog), flog      # an N-node group in every level: handed back
    if hip_backward:
        assert n_b > 0
        if N <= 64:
            assert all(live >= 1 and covered == live and not back for _, live, covered, back in blog), blog
            assert any(live < n for n, live, _, _ in blog), blog       # frozen groups shared a level (a launch) with trained ones
        else:
            assert all(back for _, live, _, back in blog if live), blog
    names, title = UR.names_of(rl), f"gpu {case}, hip forward + {'hip' if hip_backward else 'library'} backward"
    batches64 = [UR.batch64(b) for b in batches]
    ref = _staged(UR.Update64(rl.gamma, LR), recs, batches64, names)
    fig, zeros = _ratios(ref, recs, names)
    lib_ref = _staged(UR.Update64(rl.gamma, LR), libs, batches64, names)
    lib_fig, _ = _ratios(lib_ref, libs, names)
    fig["out"], fig["clip"], fig["opt"], lib_fig["out"] = ref["out"], ref["clip"], ref["opt"], lib_ref["out"]
    print(f"\n[{title}] relu elements within rounding of zero whose sign was taken from the float32 run (under test, library): "
          f"{ref['signs'][0]}, {lib_ref['signs'][0]}; disagreements outside the band: {ref['signs'][1]}, {lib_ref['signs'][1]}")
    assert ref["signs"][1] == 0 and lib_ref["signs"][1] == 0
    _report(f"{title}: library path against float64", lib_fig)
    _report(f"{title}: update under test against float64", fig)
    assert not zeros, f"float64 gradient tensors that are exactly zero (nothing to compare): {zeros}"
    _assert_within(fig, _taus(lib_fig, title), title)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_update_hip_forward_and_backward(case, monkeypatch):
    """both hooks installed (BatchedMARL(level_backward="hip")): three updates stage by stage against float64, tau measured from the
    library path on the same snapshots; the logs show that both hooks ran, that no level inside the envelope was handed back, that
    frozen groups shared a level with trained ones and that the passes under no_grad ran without X'.
    Largest ratios measured on an MI355X, under test / library path (tau = 4 x the latter; profiles/r13/update_float64_tests.txt):
                          output             loss               critic gradient    actor gradient
      5x12                1.4e-07 / 1.6e-07  2.3e-06 / 2.5e-06  4.2e-06 / 1.9e-06  7.6e-07 / 6.0e-07
      7x33                1.2e-07 / 2.0e-07  5.1e-07 / 5.1e-07  4.1e-07 / 4.7e-07  2.7e-07 / 4.0e-07
      3x64                2.2e-07 / 3.9e-07  4.1e-06 / 4.1e-06  3.5e-06 / 3.8e-06  1.2e-06 / 1.2e-06
      2x66                2.9e-07 / 2.9e-07  1.2e-06 / 1.2e-06  1.5e-06 / 1.5e-06  6.7e-07 / 6.7e-07   (handed back: the library path, bit for bit)
      5x12-materialised   1.5e-07 / 1.7e-07  1.0e-06 / 9.5e-07  9.1e-07 / 1.3e-06  6.4e-07 / 7.4e-07
    clip <= 0.20 and optimiser <= 0.997 of their bounds.  One tau sits at its cap: the loss at 3x64, where the library path itself is
    at 4.1e-06 (Q is a sum over 64 nodes x 2 200 features and the loss a mean of squared differences of such sums); the kernels' loss
    is held to 1e-05 there."""
    _gpu_update(case, True, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_update_hip_forward_library_backward(case, monkeypatch):
    """the forward hook only (the engine's default): the same comparison.
    Largest ratios measured on an MI355X, under test / library path (profiles/r13/update_float64_tests.txt):
                          output             loss               critic gradient    actor gradient
      5x12                1.4e-07 / 1.6e-07  2.2e-06 / 1.5e-06  4.6e-06 / 7.1e-06  6.8e-07 / 6.8e-07
      7x33                1.2e-07 / 2.0e-07  3.7e-07 / 4.7e-07  3.7e-07 / 4.3e-07  4.1e-07 / 4.0e-07
      3x64                2.2e-07 / 3.9e-07  4.1e-06 / 4.1e-06  3.5e-06 / 3.8e-06  1.2e-06 / 1.2e-06   (tau(loss) at its cap, as above)
      2x66                2.9e-07 / 2.9e-07  1.2e-06 / 1.2e-06  1.5e-06 / 1.5e-06  6.7e-07 / 6.7e-07
      5x12-materialised   1.6e-07 / 1.7e-07  1.0e-06 / 1.1e-06  9.1e-07 / 1.7e-06  7.4e-07 / 7.6e-07
    clip <= 0.24 and optimiser <= 0.997 of their bounds."""
    _gpu_update(case, False, monkeypatch)


# ---- the engine path: the update replayed as a hipGraph ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("level_backward", ["hip", None], ids=["hip", "default"])
def test_replayed_update_against_float64(level_backward):
    """`BatchedMARL._train` replaying its captured update (the engine of test_marl_batched.test_train_graph_update_deltas_match_eager:
    64 envs, hidden 40, lr 1e-3, batch 8, one game step to capture) three times on fixed replay batches, from a snapshot of weights,
    targets and optimiser state.  No spy runs inside a replay, so what is compared is the weight delta of every network with the host
    model run FREE over the same three updates from the snapshot: ||dW - dW64|| / ||dW64|| <= 4 x the largest figure of the eager
    library path (hooks removed) for that kind of network, and never above 1e-3 (the suite's replay-against-eager bound is 0.05).
    The eager update with the engine's hooks is held to the same bound, and its nine c_loss entries (a replay runs no Python: it
    appends none, which the test also asserts) to 4 x the library path's largest loss ratio over these and the other batches, never
    above 1e-5.  Negative control: the float64 deltas of other batches fail the bound for every network.
    Measured on an MI355X (profiles/r13/update_float64_tests.txt; the figures move in the third digit from run to run), per network:
      replayed           actors 3.3e-05 3.2e-05 3.1e-05, critics 3.9e-06 4.2e-06 4.3e-06   (level_backward "hip" and default alike)
      eager, hooks       the replay's figures to every digit printed
      eager library      actors 3.3e-05 3.2e-05 3.1e-05, critics 3.9e-06 4.2e-06 4.3e-06   (tau: actors 1.3e-04, critics 1.7e-05)
      other batches      0.36 .. 1.7
      c_loss             eager with hooks 1.1e-06 (1.1e-06 .. 1.5e-06 over five runs), eager library 6.8e-07 | 4.3e-07 on these
                         batches (4.3e-07 .. 6.8e-07 over five runs) and 1.9e-06 | 1.6e-06 on the other ones: tau 7.7e-06 | 6.5e-06"""
    lib = tm.load()
    prev = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda")
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            topo = tm.TrussTopology.grid(4)
            torch.manual_seed(5)
            rl = RL.MADDPG(LR, M.ep, M.epd, M.gamma, 40, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device="cuda")
            kw = {} if level_backward is None else {"level_backward": level_backward}
            eng = marl.BatchedMARL(topo, 64, rl, max_front=6, lib=lib, device="cuda", replay_capacity=256, batch_size=8, seed=5, **kw)
            b = synthetic.random_batch(topo, 64, 5)
            eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
            eng.game_step_all(train=True, explore=True, train_iters=1)
        assert eng._tg is not None and eng.level_backward == (level_backward or "library")
        hooks = RL._LEVEL_FORWARD.get("cuda"), RL._LEVEL_BACKWARD.get("cuda")
        assert hooks[0] is not None and (hooks[1] is not None) == (level_backward == "hip")
        names, own = UR.names_of(rl), UR.tensors_of(rl)
        state = [t for k in UR.KINDS for ts in own[k] for t in ts] + rl.critics_opt.state_tensors()
        snap = [t.detach().clone() for t in state]
        start = _snap(rl)
        opt0 = [UR.f64(t) for t in rl.critics_opt.state_tensors()]

        def batches(seed):
            g = torch.Generator(device="cuda")
            g.manual_seed(seed)
            out = []
            for _ in range(3):
                S, NS, ag, at, R = eng.replay.sample(eng.batch_size, g)
                out.append((eng._net_state(S), [eng._net_state(ns) for ns in NS], [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)], R))
            return out

        calls = []
        orig = rl.train_on_batch
        rl.train_on_batch = lambda *a: calls.append(1) or orig(*a)

        def run(bs, graph):
            """-> ({kind: [per agent: flat float64 weight delta]}, the c_loss entries the run appended [update][agent])"""
            with torch.no_grad():
                for t, v in zip(state, snap):
                    t.copy_(v)
            eng.use_train_graph = graph
            n0 = len(rl.agents[0].c_loss)
            for b_ in bs:
                eng._train(*b_)
            torch.cuda.synchronize()
            losses = [[float(ag.c_loss[k]) for ag in rl.agents] for k in range(n0, len(rl.agents[0].c_loss))]
            return {k: [_cat([UR.f64(p) - UR.f64(v) for p, v in zip(ps, vs)]) for ps, vs in zip(own[k], start[k])] for k in ("actor", "critic")}, losses

        def free64(bs):
            P = UR.params64(names, start)
            opt = {"t": int(opt0[0]), "m": opt0[1].clone(), "v": opt0[2].clone()}
            model = UR.Update64(rl.gamma, LR)
            losses = [model.update(P, opt, UR.batch64(b_)) for b_ in bs]
            P0 = UR.params64(names, start)
            return {k: [_cat(p.values()) - _cat(p0.values()) for p, p0 in zip(P[k], P0[k])] for k in ("actor", "critic")}, losses

        fixed = batches(1)
        d_graph, l_graph = run(fixed, True)
        assert eng._tg is not None and eng.use_train_graph and not calls and l_graph == []        # replayed: no Python ran
        d_eager, l_eager = run(fixed, False)
        assert len(calls) == 3 and len(l_eager) == 3
        RL.set_level_forward(None, "cuda")
        RL.set_level_backward(None, "cuda")
        d_lib, l_lib = run(fixed, False)
        other = batches(2)
        _, l_lib_other = run(other, False)
        RL.set_level_forward(hooks[0], "cuda")
        RL.set_level_backward(hooks[1], "cuda")
        d64, l64 = free64(fixed)
        d64_other, l64_other = free64(other)
        rel = lambda d, ref: {k: [float((a - r).norm() / r.norm()) for a, r in zip(d[k], ref[k])] for k in d}
        rel_l = lambda ls, ref=l64: max(abs(l - float(r)) / abs(float(r)) for row, ref_row in zip(ls, ref) for l, r in zip(row, ref_row))
        r_lib, r_eager, r_graph, r_other = rel(d_lib, d64), rel(d_eager, d64), rel(d_graph, d64), rel(d_graph, d64_other)
        tau = {k: min(4.0 * max(r_lib[k]), 1e-3) for k in r_lib}
        # (the library's loss figure over both sets of batches: the largest of nine values moves by half from run to run)
        worst_l = max(rel_l(l_lib), rel_l(l_lib_other, l64_other))
        tau_l = min(4.0 * worst_l, CAPS["loss"])
        fmt = lambda r: ", ".join(f"{k} " + " ".join(f"{v:.3g}" for v in vs) for k, vs in r.items())
        print(f"\n[replayed update, level_backward={eng.level_backward}] ||dW - dW64|| / ||dW64|| per network"
              f"\n  eager library: {fmt(r_lib)}\n  eager, engine's hooks: {fmt(r_eager)}\n  replayed: {fmt(r_graph)}"
              f"\n  replayed against the float64 deltas of other batches: {fmt(r_other)}"
              f"\n  tau: " + ", ".join(f"{k} {v:.3g}" for k, v in tau.items()) +
              f"\n  c_loss, largest relative error: eager library {rel_l(l_lib):.3g} (other batches {rel_l(l_lib_other, l64_other):.3g}), eager with the engine's hooks {rel_l(l_eager):.3g}, tau {tau_l:.3g}")
        assert min(float(d.abs().max()) for k in d64 for d in d64[k]) > 1e-4
        for k in tau:
            assert 4.0 * max(r_lib[k]) < 1e-3, f"tau({k}) would sit at its cap"
            assert max(r_graph[k]) <= tau[k], f"replayed {k}: {r_graph[k]} > {tau[k]:.3g}"
            assert max(r_eager[k]) <= tau[k], f"eager {k}: {r_eager[k]} > {tau[k]:.3g}"
            assert min(r_other[k]) > tau[k]
        assert 4.0 * worst_l < CAPS["loss"] and rel_l(l_eager) <= tau_l
    finally:
        RL.set_level_forward(prev[0], "cuda")
        RL.set_level_backward(prev[1], "cuda")
