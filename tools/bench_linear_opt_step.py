#!/usr/bin/env python3
"""Times one optimizer step of NetLinear trained with SGD, Adam or RMSprop with momentum 0.9 (what the Triangle scheduler makes of the
reference's RMSprop; rmsprop_momentum='follow') in both step forms on the same GPU, in the same process,
alternating them: torch autograd (IID_model._step, what linear_step='autograd' runs) and the native HIP step
(fused_opt.FusedLinearOptTrainer, linear_step='native', full-batch steps replayed from a captured graph).

Input: a seeded synthetic feature store, 100 000 sequences x 3 mimic views, k = 6 (F = 4096 features), batch 512 (m = 1024 rows a
step).  For every (optimizer, n_clusters) of --optimizers x --clusters one JSON line: us per step of each form (median of the rounds,
and the rounds), whether the native median clears the autograd median by more than the autograd rounds' own spread (max - min),
launches and library products per step (torch.profiler).  The RMSprop case also times the default fused step at the same shape
(fused.FusedLinearTrainer, the momentum ignored; whole epochs of its own graph replays): the price of following the reference, no bar.

Usage:  python tools/bench_linear_opt_step.py [--rounds R] [--steps S] [--out FILE]      (--out: the lines are also appended to FILE)
"""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Store:
    def __init__(self, n, n_views, f, dev, seed=0):
        import torch
        g = torch.Generator(device=dev).manual_seed(seed)
        self.n, self.f, self.n_views = n, f, n_views
        self.n_pairs = n * n_views
        self.feats = torch.rand(((n_views + 1) * n, f), device=dev, generator=g)
        self.mean = self.feats[:n].double().mean(0)
        self.scale = self.feats[:n].double().std(0).clamp_min(1e-3)
        self.inv_scale = 1.0 / self.scale


def make_optimizer(name, params):
    import torch
    if name == "SGD":                                        # reference models.py:89-92
        return torch.optim.SGD(params, lr=1e-3, weight_decay=0.01, momentum=0.9)
    if name == "RMSprop":                                    # models.py:87-88 as CyclicLR (models.py:99) leaves it at construction
        return torch.optim.RMSprop(params, lr=1e-3, weight_decay=0.01, momentum=0.9)
    return torch.optim.Adam(params, lr=1e-3)


def bench(opt_name, C, st, a, dev):
    import numpy as np
    import torch
    from torch.profiler import profile, ProfilerActivity
    from idelucs_amd import models
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    F, B = st.f, a.batch
    m = 2 * B

    torch.manual_seed(0)
    net_a = NetLinear(F, C).to(dev)
    net_a.apply(models.weights_init)
    auto = types.SimpleNamespace(net=net_a, optimizer=make_optimizer(opt_name, net_a.parameters()), weight=0.25, l=2.8)

    torch.manual_seed(0)
    net_n = NetLinear(F, C).to(dev)
    net_n.apply(models.weights_init)
    tr = FusedLinearOptTrainer(net_n, make_optimizer(opt_name, net_n.parameters()), 0.25, 2.8, seed=0)
    tr.begin_voter(0)
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    per = 16
    bf = tr.buffers(m)

    def native_prologue():
        tr.ctl[1:2].zero_()
        tr._gather(st, bf)

    def native_eager(n):
        for i in range(n):
            tr.step_on_batch(bf, batch_advance=B, next_from=st, xi=i % 2)

    native_prologue()
    x_auto = bf.xs[0].clone()                            # the autograd form steps on the same (first) batch
    net_a.train()

    def autograd_steps(n):
        for _ in range(n):
            models.IID_model._step(auto, x_auto)

    native_eager(2)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        native_eager(per)

    def native_steps(n):                                 # (n // per replays from a fresh prologue: n * B <= n_pairs)
        for _ in range(n // per):
            g.replay()

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    default, t_def = None, []
    if opt_name == "RMSprop":                            # the default step of this shape: RMSprop without the momentum
        from idelucs_amd.fused import FusedLinearTrainer
        torch.manual_seed(0)
        net_d = NetLinear(F, C).to(dev)
        net_d.apply(models.weights_init)
        default = FusedLinearTrainer(net_d, 1e-3, 0.25, 2.8, seed=0)
        default.begin_voter(0)
        gen_d = torch.Generator(device=dev).manual_seed(1)
        n_default = [1]

        def default_epoch(n):
            n_default[0] = default.run_epoch(st, B, generator=gen_d)[1]
        default_epoch(0)                                 # (warm: the capture)

    autograd_steps(8)
    native_prologue()
    native_steps(per * 2)
    steps = max(per, min(a.steps, st.n_pairs // B - 1) // per * per)
    t_auto, t_nat = [], []
    for _ in range(a.rounds):                            # alternating, same box, same process
        t_auto.append(timed(autograd_steps, steps))
        native_prologue()
        t_nat.append(timed(native_steps, steps))
        if default is not None:
            t_def.append(timed(default_epoch, 1) / n_default[0])

    def launches(fn, n):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(n)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                 and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(names) / n, sum("Cijk" in s for s in names) / n

    native_prologue()
    l_auto, lib_auto = launches(autograd_steps, 4)
    l_nat, lib_nat = launches(native_eager, 4)
    us_a, us_n = float(np.median(t_auto)), float(np.median(t_nat))
    spread = max(t_auto) - min(t_auto)
    res = {"tool": "bench_linear_opt_step", "optimizer": opt_name, "m": m, "F": F, "C": C, "n_pairs": st.n_pairs, "steps_per_round": steps,
           "autograd_us_per_step": round(us_a, 2), "native_us_per_step": round(us_n, 2), "speedup": round(us_a / us_n, 2),
           "autograd_rounds_us": [round(t, 2) for t in t_auto], "native_rounds_us": [round(t, 2) for t in t_nat],
           "autograd_spread_us": round(spread, 2), "native_below_autograd_by_more_than_its_spread": bool(us_a - us_n > spread),
           "launches_per_step": {"autograd": l_auto, "native": l_nat}, "library_gemms_per_step": {"autograd": lib_auto, "native": lib_nat},
           "device": torch.cuda.get_device_name(0)}
    if default is not None:
        res.update({"default_fused_us_per_step": round(float(np.median(t_def)), 2), "default_fused_rounds_us": [round(t, 2) for t in t_def],
                    "default_fused_steps_per_round": n_default[0]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--clusters", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--optimizers", nargs="+", default=["SGD", "Adam"], choices=["SGD", "Adam", "RMSprop"])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    dev = torch.device("cuda")
    st = Store(a.n, 3, 4 ** 6, dev, seed=7)
    for opt_name in a.optimizers:
        for C in a.clusters:
            line = json.dumps(bench(opt_name, C, st, a, dev))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
