"""Diagnostic: the optimiser steps of the MADDPG update as framework operators (`_clip_flat` + `SharedStepAdam.step` /
`_fresh_adam_step`) against one truss_optim_step call each (truss_mi355.optim, BatchedMARL(optimizer_path="hip")), both paths in ONE
process, in blocks torch, hip, torch: the two torch figures give the spread a difference has to exceed.

    python tools/optim_probe.py [OUT_DIR]        -> OUT_DIR/optim_probe.json   (default OUT_DIR: build/optim_probe)

(a) "steps": the critics' step (three critics, 144 tensors) and one actor's step alone, at the reference's widths (a_nn = c_nn = 200)
    for small_roof (16 nodes): median wall time of 60 synchronised calls per block (host side included) after 10 warm-up calls,
    device kernels per call (torch.profiler, a run of its own), and the device time of truss_optim_apply_kernel with the bytes/s it
    stands for (g, m, v, w read, m, v, w written: 28 bytes per parameter; the first step of an actor: 12).
(b) "update": the update at batch 32 on small_roof replayed as a hipGraph by two engines that differ only in optimizer_path: 200
    replays per block (the engine's `_train`: the copies into the graph's input buffers and the replay), ms per update of each
    block; and the device kernels of one eager update of each path."""
import contextlib
import io
import json
import os
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
                           optimizer_path=path)
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


def steps(eng_hip):
    import torch
    import truss2D_RL as RL
    from truss_mi355 import optim
    rl, hook = eng_hip.rl, optim.optimizer_step(eng_hip.lib)
    out = {}
    lists = {"critics": [p for ag in rl.agents for p in ag.critic_model.parameters()], "actor": list(rl.agents[0].actor_model.parameters())}
    for name, ps in lists.items():
        n = sum(p.numel() for p in ps)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        flat = torch.randn(n, device="cuda", generator=gen) * 0.05
        if name == "critics":
            opt = RL.SharedStepAdam(ps, lr=1e-7, eps=1e-7)
            opt.step(torch.zeros_like(flat))                   # makes the state
            t_fn = lambda: opt.step(RL._clip_flat(flat, ps))
            h_fn = lambda: RL.SharedStepAdam.step(opt, flat, fused=hook)
            per = 28
        else:
            t_fn = lambda: RL._fresh_adam_step(ps, 1e-8, 1e-7, RL._clip_flat(flat, ps))
            h_fn = lambda: hook(ps, flat, 1e-8, 1e-7)
            per = 12
        blocks = [("torch", median_ms(t_fn)), ("hip", median_ms(h_fn)), ("torch", median_ms(t_fn))]
        kt, kh = kernels(t_fn), kernels(h_fn)
        apply_us = []
        for _ in range(10):
            apply_us += [d for k, d in kernels(h_fn) if "truss_optim_apply_kernel" in k]
        a_us = statistics.median(apply_us)
        out[name] = dict(tensors=len(ps), parameters=n, median_ms=[dict(path=p, ms=round(v, 4)) for p, v in blocks],
                         launches=dict(torch=len(kt), hip=len(kh)), hip_kernels_us={k.split("(")[0][:48]: d for k, d in kh},
                         apply_kernel_us=a_us, apply_bytes=per * n, apply_TB_per_s=round(per * n / (a_us * 1e-6) / 1e12, 3))
    return out


def update(eng_t, bt, eng_h, bh):
    import torch
    import truss2D_RL as RL
    from truss_mi355 import optim

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
        RL.set_optimizer_step(optim.optimizer_step(eng.lib) if path == "hip" else None, "cuda")
        eng.rl.train_on_batch(*batch)
        torch.cuda.synchronize()
        ks = kernels(lambda: eng.rl.train_on_batch(*batch))
        launches[path] = dict(all=len(ks), optim=sum("truss_optim" in k for k, _ in ks))
    RL.set_optimizer_step(None, "cuda")
    return dict(ms_per_update=[dict(path=p, ms=round(v, 4)) for p, v in blocks], eager_launches=launches)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "optim_probe")
    os.makedirs(out_dir, exist_ok=True)
    eng_t, bt = engine("torch")
    eng_h, bh = engine("hip")
    res = dict(update=update(eng_t, bt, eng_h, bh), steps=steps(eng_h))
    with open(os.path.join(out_dir, "optim_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
