"""Diagnostic: the tail of a critic pass of the MADDPG update (11 sum pools, concatenation, three dense layers) as framework operators
against truss_critic_tail / truss_critic_tail_backward (truss_mi355.critic_tail, BatchedMARL(critic_tail="hip")), both paths in ONE
process, in blocks torch, hip, torch, hip, torch: the torch figures give the spread a difference has to exceed.

    python tools/critic_tail_probe.py [OUT_DIR [VARIANT_LIB ...]]   -> OUT_DIR/critic_tail_probe.json   (default OUT_DIR: build/critic_tail_probe)

(a) "update": the update at batch 32 on small_roof replayed as a hipGraph by two engines that differ only in critic_tail (both with
    level_backward="hip" and optimizer_path="hip"): 200 replays per block (the engine's `_train`: the copies into the graph's input
    buffers and the replay), ms per update of each block; and the device kernels of one eager update of each path.
(b) "tail": the tail alone at the reference's widths (11 layers of 200 channels, 200 dense units, 16 nodes): the three online
    critics' pass at batch 32, forward and backward with every gradient, and the three target critics' pass at batch 96, forward
    only -- median wall time of 60 synchronised calls per block (host side included) after 10 warm-up calls, and the device time of
    each kernel of one call (torch.profiler, a run of its own).  Every VARIANT_LIB (a build of the library with another
    -DTRUSS_CRITIC_TAIL_SAMPLES) is timed the same way.
(c) "resources": the lines of the build's kernel resource report for the three kernels."""
import contextlib
import io
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mop-truss-marl_amd"))

CALLS, WARM, REPLAYS = 60, 10, 200


def kernels(fn):
    import torch
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name, e.device_time if hasattr(e, "device_time") else e.cuda_time) for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA]


def median_ms(fn):
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def engine(path, B=512):
    import numpy as np
    import torch
    import bench_configs
    import truss_mi355 as tm
    from truss_mi355 import marl
    nx = 8
    topo = tm.TrussTopology.grid(nx)
    torch.manual_seed(3)
    eng = marl.BatchedMARL(topo, B, bench_configs._maddpg("cuda"), max_front=20, device="cuda", replay_capacity=32768, batch_size=32,
                           level_backward="hip", optimizer_path="hip", critic_tail=path)
    x = np.tile(np.arange(nx) * 5.0, 2)
    tar = np.concatenate([np.zeros(nx), 2.0 + 2.0 * np.abs(np.linspace(-1, 1, nx))])
    y0 = np.concatenate([np.zeros(nx), np.full(nx, 8.0)]).astype(np.float32)
    eng.reset(x[None].repeat(B, 0), tar[None].repeat(B, 0), 8.0, 0.3, 0.001 * 5.0 * (nx - 1), 0.0, -120000.0 * 8 / nx, 1.0,
              y0[None].repeat(B, 0), np.full((B, topo.E), 4, np.int32))
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(2):
            eng.game_step_all(train=True)                      # lazy layers, GEMM selection, the capture of the update
    torch.cuda.synchronize()
    assert eng._tg is not None, "the update was not captured"
    S, NS, ag, at, R = eng.replay.sample(eng.batch_size, eng.gen)
    batch = (eng._net_state(S), [eng._net_state(ns) for ns in NS], [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)], R)
    return eng, batch


def update(eng_t, bt, eng_h, bh):
    import torch
    import truss2D_RL as RL
    from truss_mi355 import critic_tail

    def block(eng, batch):
        eng.use_train_graph = True
        for _ in range(10):
            eng._train(*batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPLAYS):
            eng._train(*batch)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / REPLAYS

    blocks = [("torch", block(eng_t, bt)), ("hip", block(eng_h, bh)), ("torch", block(eng_t, bt)), ("hip", block(eng_h, bh)),
              ("torch", block(eng_t, bt))]
    launches = {}
    for path, eng, batch in (("torch", eng_t, bt), ("hip", eng_h, bh)):
        RL.set_critic_tail(critic_tail.tail_hook(eng.lib) if path == "hip" else None, "cuda")
        eng.rl.train_on_batch(*batch)
        torch.cuda.synchronize()
        ks = kernels(lambda: eng.rl.train_on_batch(*batch))
        launches[path] = dict(all=len(ks), critic_tail=sum("truss_critic_tail" in k for k, _ in ks))
    RL.set_critic_tail(None, "cuda")
    return dict(ms_per_update=[dict(path=p, ms=round(v, 4)) for p, v in blocks], eager_launches=launches)


def tail(lib, variants):
    import torch
    import truss_mi355 as tm
    from truss_mi355 import critic_tail as CT
    N, L, H, Q = 16, 11, 200, 200
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)

    def items(B):
        return [([torch.relu(r(B, N, H)) for _ in range(L)], [r(Q, L * H) * (2.0 / (Q + L * H)) ** 0.5, r(Q) / 10, r(Q, Q) * (1.0 / Q) ** 0.5, r(Q) / 10,
                                                            r(1, Q) * (2.0 / (Q + 1)) ** 0.5, r(1) / 10]) for _ in range(3)]

    online, target = items(32), items(96)
    dqs = [r(32, 1) for _ in range(3)]
    needs = [([True] * L, [True] * 6)] * 3
    ref = CT.TorchTail()

    def torch_train():
        for (outs, params), dq in zip(online, dqs):
            leaves = [t.requires_grad_(True) for t in outs + params]
            torch.autograd.grad(ref._q(leaves[:L], leaves[L:]), leaves, dq)

    def torch_target():
        with torch.no_grad():
            for outs, params in target:
                ref._q(outs, params)

    def hip_fns(hook):
        def train():
            _, states = hook.forward(online, [True] * 3)
            hook.backward(online, states, dqs, needs)
        return train, lambda: hook.forward(target, [False] * 3)

    h_train, h_target = hip_fns(CT.tail_hook(lib))
    out = {}
    for name, t_fn, h_fn in (("online critics, batch 32, forward + backward", torch_train, h_train),
                             ("target critics, batch 96, forward", torch_target, h_target)):
        blocks = [("torch", median_ms(t_fn)), ("hip", median_ms(h_fn)), ("torch", median_ms(t_fn)), ("hip", median_ms(h_fn)), ("torch", median_ms(t_fn))]
        kt, kh = kernels(t_fn), kernels(h_fn)
        out[name] = dict(median_ms=[dict(path=p, ms=round(v, 4)) for p, v in blocks], launches=dict(torch=len(kt), hip=len(kh)),
                         torch_device_us=round(sum(d for _, d in kt), 1), hip_kernels_us=[(k.split("(")[0][:48], d) for k, d in kh])
    for path in variants:
        v_train, v_target = hip_fns(CT.tail_hook(tm.load(path)))
        out[os.path.basename(path)] = {
            "online critics, batch 32, forward + backward": dict(median_ms=round(median_ms(v_train), 4),
                                                                 kernels_us=[(k.split("(")[0][:48], d) for k, d in kernels(v_train)]),
            "target critics, batch 96, forward": dict(median_ms=round(median_ms(v_target), 4),
                                                      kernels_us=[(k.split("(")[0][:48], d) for k, d in kernels(v_target)])}
    return out


def resources(lib):
    rep = os.path.join(os.path.dirname(lib.path), "libtruss_mi355.resources.txt")
    if not os.path.exists(rep):
        return None
    out, name = {}, None
    for line in open(rep):
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2) if "truss_critic_tail" in m.group(2) else None
        elif name:
            out.setdefault(name, {})[m.group(1)] = m.group(2)
    return out


def main():
    import truss_mi355 as tm
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "critic_tail_probe")
    os.makedirs(out_dir, exist_ok=True)
    eng_t, bt = engine("torch")
    eng_h, bh = engine("hip")
    res = dict(update=update(eng_t, bt, eng_h, bh), tail=tail(tm.load(), sys.argv[2:]), resources=resources(tm.load()))
    with open(os.path.join(out_dir, "critic_tail_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
