"""Float64 host model of one MADDPG update (truss2D_RL.MADDPG.train_on_batch), for the test suite.

Restated from the order of operations of the original training loop and from the `train_on_batch` docstring, in plain
`torch.float64` on the CPU: every GCN layer is act(A (X W^T) + b) written out, the gradients come from float64 autograd over that
per-layer forward, the clip and the two Adam steps are written out by hand.  Nothing of the level machinery of truss2D_RL
(`run_networks`, `gcn_level`, `_GcnLevel`), nor its optimiser helpers, is imported: the model shares only the parameter NAMES of
the modules (`named_parameters`) with the code it checks.

One update, for three agents i with critics Q_i, actors pi_i, their targets Q'_i, pi'_i and a minibatch (S, NS_0..2, A, R):

  TD stage       a'_j = pi'_j(NS_f) for every next state f and agent j;  q_i^f = Q'_i(NS_f, a' in agent i's order);
                 y_i = R_i + gamma (q_i^0 + q_i^1 + q_i^2) / 3          (the terminal branch never fires in the original)
  critic stage   L_i = mean_b (Q_i(S, A in agent i's order) - y_i)^2;  g = dL_i / d(parameters of Q_i);  every gradient TENSOR
                 scaled by min(1, 1 / (||g|| + 1e-12));  Adam (lr, betas 0.9 / 0.999, eps 1e-7) with ONE step counter for the three
                 critics and moments carried from update to update
  actor stage i  (i = 0, 1, 2 one after the other)  L = -mean_b Q_i(S, pi_0(S), pi_1(S), pi_2(S) in agent i's order) through the
                 critic i that has just stepped and the actors < i that have just stepped;  g = dL / d(parameters of pi_i) only;
                 the same clip;  the first step of a fresh Adam at lr * 0.1:  p -= lr * 0.1 * g / (|g| + 1e-7)

agent i's order of (self, other1, other2) is (0, 1, 2), (1, 0, 2), (2, 0, 1).

`Update64(gamma, lr, mutant=...)` evaluates a deliberately broken variant (MUTANTS) instead: the tests require each of them to
fall outside the bounds the correct model satisfies.
"""
from __future__ import annotations

import torch

KINDS = ("actor", "critic", "tactor", "tcritic")
ATTRS = ("actor_model", "critic_model", "target_actor_model", "target_critic_model")

MUTANTS = (
    "gamma dropped",
    "/ 3 dropped",
    "TD target from the online networks",
    "agent 1's order (1, 2, 0)",
    "actor loss through the pre-step critic",
    "actor 1 sees the un-stepped actor 0",
    "no clip",
    "flat vector clipped as one tensor",
    "bias correction frozen at t = 1",
    "actor learning-rate factor 0.1 dropped",
    "loss mean taken as a sum",
)

B1, B2, EPS = 0.9, 0.999, 1e-7


def names_of(rl):
    """{kind: parameter names of that kind of network, in `parameters()` order} (the same for the three agents)"""
    return {k: [n for n, _ in getattr(rl.agents[0], a).named_parameters()] for k, a in zip(KINDS, ATTRS)}


def tensors_of(rl):
    """{kind: [per agent: the parameter tensors of that network, in `parameters()` order]}"""
    return {k: [list(getattr(ag, a).parameters()) for ag in rl.agents] for k, a in zip(KINDS, ATTRS)}


def f64(t):
    return t.detach().to("cpu", torch.float64)


def params64(names, tensors):
    """{kind: [per agent: {name: float64 CPU tensor}]} from tensors laid out as `tensors_of` gives them"""
    return {k: [dict(zip(names[k], [f64(t) for t in ts])) for ts in tensors[k]] for k in tensors}


def batch64(batch):
    S, NS, A, R = batch
    return [f64(t) for t in S], [[f64(t) for t in ns] for ns in NS], [(f64(g), f64(t)) for g, t in A], f64(R)


# ---- the networks, layer by layer ------------------------------------------------------------------------------------------------
# The model can be shown what the float32 run it is compared with computed: `seen` = {layer name: that layer's output}.
#   * Every such output is compared with the model's own, ||out - out64|| / ||out64|| (`Update64.take_outputs`): the forward half
#     of every stage, layer by layer -- which is also the only place where the weights a frozen actor was evaluated with show (the
#     critic's branches for the three actions meet only in its dense layers, so through the gradient they show only where a dense
#     relu changes side).
#   * relu'(0) is not defined, and a float32 evaluation puts a pre-activation that is zero to within its rounding error on either
#     side of it: at the widths of the project a few of the millions of relu elements of an update are in that position, and each
#     of them moves one row of a kernel's gradient by about a thousandth.  Both gradients are right.  So, as
#     tests/test_gcn_level_backward.py does with the layer's given output, the model takes the SIGN the float32 run had for the
#     elements inside the band |z| <= BAND (K + N + 2) 2^-24 Mag, Mag = |A| (|X| |W|^T) + |b| -- the worst-case error of a float32
#     evaluation in any order, times BAND for the levels below (their outputs are this layer's inputs).  Outside the band the model
#     keeps its own sign; an element there on which the two disagree is a finding (both are counted: `Update64.sign_counts`).

BAND = 4.0


class Net:
    """the parameters {name: tensor} of one network and, optionally, the layer outputs a float32 run of it had"""

    def __init__(self, p, seen=None, rows=None, counts=None, outputs=None, tag=""):
        self.p, self.seen, self.rows, self.tag = p, seen, rows, tag    # rows: the slice of the float32 run's batch this evaluation covers
        self.counts = [0, 0] if counts is None else counts      # band elements whose sign was taken from `seen`; disagreements outside
        self.outputs = [] if outputs is None else outputs       # (label, ||seen - out64|| / ||out64||)

    def layer(self, name, x, adj, act="relu"):
        w, b = self.p[name + ".lin.weight"], self.p[name + ".bias"]
        z = adj @ (x @ w.T) + b
        seen = None if self.seen is None else self.seen.get(name)
        if seen is not None:
            seen = f64(seen if self.rows is None else seen[self.rows])
        if act != "relu":
            out = torch.sigmoid(z) if act == "sigmoid" else z
        elif seen is None:
            out = torch.relu(z)
        else:
            with torch.no_grad():
                mag = adj.abs() @ (x.abs() @ w.abs().T) + b.abs()
                band = z.abs() <= BAND * (w.shape[1] + x.shape[1] + 2) * 2.0 ** -24 * mag
                own, theirs = z > 0, seen > 0
                self.counts[0] += int((band & (theirs != own)).sum())
                self.counts[1] += int((~band & (theirs != own)).sum())
                on = torch.where(band, theirs, own)
            out = torch.where(on, z, torch.zeros_like(z))
        if seen is not None:
            err, den = float((seen - out.detach()).norm()), float(out.detach().norm())
            self.outputs.append((f"{self.tag} {name}", err / den if den > 0 else (float("inf") if err > 0 else 0.0)))
        return out


def _tiled(pooled, n):
    """[B, H] -> n copies stacked on a new LAST axis, that memory read as [B, n, H] (a reshape, not a transpose)"""
    B, H = pooled.shape
    return pooled.repeat_interleave(n, dim=1).reshape(B, n, H)


def actor64(net, s):
    """s = [x_n, A_n, A_s, A_n_ts, A_n_cs, mask, x_p, A_p] -> (geometry action [B, N, 2], topology action [B, N, 3])"""
    x_n, A_n, A_s, A_ts, A_cs, _, x_p, A_p = s
    h1, h2, h3 = (net.layer(f"gcn_l1_{k}", x_n, A_n) for k in (1, 2, 3))
    front = _tiled(net.layer("gcn_l1_4", x_p, A_p).sum(dim=1), x_n.shape[1])
    h = (net.layer("gcn_l2_1", h1, A_n) + net.layer("gcn_l2_2", h2, A_ts) + net.layer("gcn_l2_3", h2, A_cs) +
         net.layer("gcn_l2_4", h3, A_s) + net.layer("gcn_l2_5", front, A_n))
    return (net.layer("gcn_l4_1", net.layer("gcn_l3_1", h, A_n), A_n, "sigmoid"),
            net.layer("gcn_l4_2", net.layer("gcn_l3_2", h, A_s), A_n, "sigmoid"))


def critic64(net, s, acts):
    """acts = [self geo, self topo, other1 geo, other1 topo, other2 geo, other2 topo] -> Q [B, 1]"""
    x_n, A_n, A_s, A_ts, A_cs, _, x_p, A_p = s
    p = net.p
    h1, h2, h3 = (net.layer(f"l1.{k}", x_n, A_n) for k in (0, 1, 2))
    front = _tiled(net.layer("l1.3", x_p, A_p).sum(dim=1), x_n.shape[1])
    ha = [net.layer(f"l1.{4 + k}", a, A_n) for k, a in enumerate(acts)]
    second = [net.layer("l2.0", h1, A_n), net.layer("l2.1", h2, A_ts), net.layer("l2.2", h2, A_cs), net.layer("l2.3", h3, A_s)]
    second += [net.layer(f"l2.{4 + k}", h, A_n) for k, h in enumerate(ha)]
    second.append(net.layer("l2.10", front, A_n))
    q = torch.cat([h.sum(dim=1) for h in second], dim=1)                 # eleven sum pools side by side
    q = torch.relu(q @ p["dense_1.weight"].T + p["dense_1.bias"])
    q = torch.relu(q @ p["dense_2.weight"].T + p["dense_2.bias"])
    return q @ p["dense_out.weight"].T + p["dense_out.bias"]


def _leaves(p):
    return {k: v.detach().clone().requires_grad_() for k, v in p.items()}


def _in_order(pairs, order):
    return [t for j in order for t in pairs[j]]


# ---- the update ------------------------------------------------------------------------------------------------------------------

class Update64:
    """the stages of one update in float64; every stage takes the state it starts from and returns its quantities"""

    def __init__(self, gamma, lr, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.gamma, self.lr, self.mutant = float(gamma), float(lr), mutant
        self.orders = [(0, 1, 2), (1, 2, 0) if mutant == "agent 1's order (1, 2, 0)" else (1, 0, 2), (2, 0, 1)]
        self._counts, self._outputs = [0, 0], []

    def _reduce(self, t):
        return t.sum() if self.mutant == "loss mean taken as a sum" else t.mean()

    def _net(self, p, seen, kind, agent, rows=None):
        tag = f"{kind}{agent}" + ("" if rows is None else f"[{rows.start}:{rows.stop}]")
        return Net(p, None if seen is None else seen.get((kind, agent)), rows, self._counts, self._outputs, tag)

    def take_outputs(self):
        """[(network and layer, ||out - out64|| / ||out64||)] of the layers evaluated with a float32 output to compare, since the last call"""
        out, self._outputs[:] = list(self._outputs), []
        return out

    def sign_counts(self):
        """(relu elements inside the band whose sign was taken from the float32 run, disagreements outside the band) so far"""
        return tuple(self._counts)

    def td_target(self, P, NS, R, seen=None):
        """y [B, 3] from the target networks (P["tactor"], P["tcritic"]) and the three next states.  seen: {(kind, agent): {layer:
        out > 0}} of the float32 run, whose target passes cover the three next states as ONE batch of 3 B samples"""
        online = self.mutant == "TD target from the online networks"
        actors, critics = (P["actor"], P["critic"]) if online else (P["tactor"], P["tcritic"])
        nb = R.shape[0]
        with torch.no_grad():
            total = 0.0
            for f, ns in enumerate(NS):
                rows = slice(f * nb, (f + 1) * nb)
                nxt = [actor64(self._net(a, seen, "tactor", j, rows), ns) for j, a in enumerate(actors)]
                total = total + torch.cat([critic64(self._net(c, seen, "tcritic", i, rows), ns, _in_order(nxt, self.orders[i]))
                                           for i, c in enumerate(critics)], dim=1)
            g = 1.0 if self.mutant == "gamma dropped" else self.gamma
            return R + g * (total if self.mutant == "/ 3 dropped" else total / 3.0)

    def critic_stage(self, P, S, A, y, seen=None):
        """-> (the three losses [3], per agent {name: gradient of its loss w.r.t. its critic's parameter})"""
        losses, grads = [], []
        for i, c in enumerate(P["critic"]):
            w = _leaves(c)
            loss = self._reduce((critic64(self._net(w, seen, "critic", i), S, _in_order(A, self.orders[i])) - y[:, i:i + 1]) ** 2)
            g = torch.autograd.grad(loss, list(w.values()))
            losses.append(loss.detach())
            grads.append(dict(zip(w.keys(), g)))
        return torch.stack(losses), grads

    def actor_stage(self, P, S, i, stale=None, seen=None):
        """-> (loss, {name: its gradient w.r.t. actor i's parameter}) at the state P the update has reached when agent i's actor is
        stepped.  stale = {"critic": the critics before their step, "actor0": actor 0 before its step} (used by two mutants only)"""
        w = _leaves(P["actor"][i])
        actors = [w if j == i else a for j, a in enumerate(P["actor"])]
        if self.mutant == "actor 1 sees the un-stepped actor 0" and i == 1:
            actors[0] = stale["actor0"]
        critic = stale["critic"][i] if self.mutant == "actor loss through the pre-step critic" else P["critic"][i]
        preds = [actor64(self._net(a, seen, "actor", j), S) for j, a in enumerate(actors)]
        loss = -self._reduce(critic64(self._net(critic, seen, "critic", i), S, _in_order(preds, self.orders[i])))
        g = torch.autograd.grad(loss, list(w.values()))
        return loss.detach(), dict(zip(w.keys(), g))

    def clip(self, grads):
        """a list of gradient tensors -> each scaled to L2 norm <= 1 on its own"""
        if self.mutant == "no clip":
            return [g.clone() for g in grads]
        if self.mutant == "flat vector clipped as one tensor":
            f = min(1.0, 1.0 / (float(torch.cat([g.reshape(-1) for g in grads]).norm()) + 1e-12))
            return [g * f for g in grads]
        return [g * min(1.0, 1.0 / (float(g.norm()) + 1e-12)) for g in grads]

    def adam(self, w, m, v, g, t):
        """step number t (1 for the first) of the critics' Adam on flat vectors -> (w', m', v', the update term w' - w)"""
        m2 = B1 * m + (1.0 - B1) * g
        v2 = B2 * v + (1.0 - B2) * g * g
        tc = 1 if self.mutant == "bias correction frozen at t = 1" else t
        dw = -self.lr / (1.0 - B1 ** tc) * m2 / (v2.sqrt() / (1.0 - B2 ** tc) ** 0.5 + EPS)
        return w + dw, m2, v2, dw

    def fresh_adam(self, w, g):
        """the first step of a new Adam at lr * 0.1 (zero moments: the corrected moments are g and g^2) -> (w', w' - w)"""
        lr = self.lr * (1.0 if self.mutant == "actor learning-rate factor 0.1 dropped" else 0.1)
        dw = -lr * g / (g.abs() + EPS)
        return w + dw, dw

    # ---- free-running: a whole update from a state, carrying that state on --------------------------------------------------------

    def update(self, P, opt, batch):
        """one whole update: P (as `params64` gives it) is replaced in place by the stepped state; opt = {"t", "m", "v"} (flat
        over the three critics' parameters, agent by agent; t = steps taken so far) likewise.  -> the three critic losses"""
        S, NS, A, R = batch
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
        y = self.td_target(P, NS, R)
        losses, cg = self.critic_stage(P, S, A, y)
        stale = {"critic": [dict(c) for c in P["critic"]], "actor0": dict(P["actor"][0])}
        flat = cat(self.clip([g for i in range(3) for g in cg[i].values()]))
        opt["t"] += 1
        w, opt["m"], opt["v"], _ = self.adam(cat([t for c in P["critic"] for t in c.values()]), opt["m"], opt["v"], flat, opt["t"])
        _scatter(w, P["critic"])
        for i in range(3):
            _, ag = self.actor_stage(P, S, i, stale)
            w, _ = self.fresh_adam(cat(P["actor"][i].values()), cat(self.clip(list(ag.values()))))
            _scatter(w, [P["actor"][i]])
        return losses


def _scatter(flat, dicts):
    """a flat vector back into the tensors of a list of {name: tensor}, in order"""
    k = 0
    for d in dicts:
        for name, t in d.items():
            d[name] = flat[k:k + t.numel()].view_as(t).clone()
            k += t.numel()
    assert k == flat.numel()
