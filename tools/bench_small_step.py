#!/usr/bin/env python3
"""Times one optimizer step of model_size='small' (myNet + RMSprop) in both step forms on the same GPU, in the same process,
alternating them: torch autograd (IID_model._step, what small_step='autograd' runs) and the native HIP step
(fused_small.FusedSmallTrainer, small_step='native', full-batch steps replayed from its captured graph).

Input: a seeded synthetic feature store at the cfg2 size with reduce=True -- 100 000 sequences x 3 mimic views, k = 6 canonical rows
(F = 2080 features), C = 20 clusters, batch 512 (m = 1024 rows a step).  Prints one JSON line: us per step of each form, launches
per step (torch.profiler), the algorithmic FLOP of a step (from the shapes) and the native step's share of the 157.3 TF/s fp32
matrix peak.

--momentum MU: RMSprop with a momentum buffer in both forms (torch's momentum=MU; the native step's momentum form, what
rmsprop_momentum='follow' trains under the Triangle scheduler), whether the native median clears the autograd median by more than the
autograd rounds' own spread, and beside them the default momentum-free native step in the same rounds.

--optimizer SGD|Adam: the optimizer objects of reference models.py:89-92 in both forms (torch's SGD(momentum 0.9, weight_decay 0.01) /
Adam under autograd; fused_small.FusedSmallOptTrainer, small_opt_step='native'), the same acceptance figure, and the default RMSprop
native step beside them in the same rounds.

Usage:  python tools/bench_small_step.py [--rounds R] [--steps S] [--momentum MU | --optimizer SGD|Adam] [--out FILE]
"""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MATRIX = 157.3e12


def step_flop(m, F, C):
    """Algorithmic FLOP of one step: the four layers forward (2 m n_in n_out each), their weight gradients (as many) and the input
    gradients of all but the first layer; InfoNCE's S = f f^T and (E + E^T) f; the IIC joint."""
    layers = [(F, 400), (400, 128), (128, 64), (128, C)]
    fwd = sum(2 * m * a * b for a, b in layers)
    dgrad = sum(2 * m * a * b for a, b in layers[1:])
    nce = 2 * (2 * m * m * 64)
    iic = 2 * (m // 2) * C * C
    return 2 * fwd + dgrad + nce + iic


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--clusters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--momentum", type=float, default=None)
    ap.add_argument("--optimizer", choices=["SGD", "Adam"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.optimizer is not None and a.momentum is not None:
        ap.error("--momentum is RMSprop's: not with --optimizer")
    import numpy as np
    import torch
    from torch.profiler import profile, ProfilerActivity
    from idelucs_amd import _lib, models
    from idelucs_amd.PytorchUtils import myNet
    from idelucs_amd.fused_small import FusedSmallOptTrainer, FusedSmallTrainer
    _lib.require_gpu()
    dev = torch.device("cuda")
    k, C, B = 6, a.clusters, a.batch
    F = (4 ** k + 4 ** (k // 2)) // 2
    m = 2 * B
    st = Store(a.n, 3, F, dev, seed=7)

    torch.manual_seed(0)
    net_a = myNet(F, C).to(dev)
    net_a.apply(models.weights_init)

    def optimizer(params):
        if a.optimizer == "SGD":
            return torch.optim.SGD(params, lr=1e-3, weight_decay=0.01, momentum=0.9)
        if a.optimizer == "Adam":
            return torch.optim.Adam(params, lr=1e-3)
        return torch.optim.RMSprop(params, lr=1e-3, weight_decay=0.01, momentum=a.momentum or 0.0)
    opt = optimizer(net_a.parameters())
    auto = types.SimpleNamespace(net=net_a, optimizer=opt, weight=0.25, l=2.8)
    perm = torch.randperm(st.n_pairs, device=dev)

    torch.manual_seed(0)
    net_n = myNet(F, C).to(dev)
    net_n.apply(models.weights_init)
    if a.optimizer is not None:
        tr = FusedSmallOptTrainer(net_n, optimizer(net_n.parameters()), 0.25, 2.8, seed=0)
    else:
        tr = FusedSmallTrainer(net_n, 1e-3, 0.25, 2.8, seed=0, momentum=a.momentum)
    tr.begin_voter(0)
    tr._perm = perm
    per = 16
    bf = tr.buffers(m)
    plain = None
    if a.momentum is not None or a.optimizer is not None:        # the default step beside it: the momentum-free RMSprop launch, its own buffers and graph
        torch.manual_seed(0)
        net_p = myNet(F, C).to(dev)
        net_p.apply(models.weights_init)
        plain = FusedSmallTrainer(net_p, 1e-3, 0.25, 2.8, seed=0)
        plain.begin_voter(0)
        plain._perm = perm
        bf_p = plain.buffers(m)

    def native_prologue():
        tr.ctl[1:2].zero_()
        tr._gather(st, bf, B)

    native_prologue()
    x_auto = bf.xs[0].clone()                            # the autograd form steps on the same (first) batch

    def autograd_steps(n):
        for _ in range(n):
            models.IID_model._step(auto, x_auto)

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(per):
            tr.step_on_batch(bf, xi=i % 2, next_from=st)

    def native_steps(n):                                 # (n // per replays from a fresh prologue: n * B <= n_pairs)
        for _ in range(n // per):
            g.replay()

    if plain is not None:
        def plain_prologue():
            plain.ctl[1:2].zero_()
            plain._gather(st, bf_p, B)
        plain_prologue()
        g_p = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_p):
            for i in range(per):
                plain.step_on_batch(bf_p, xi=i % 2, next_from=st)

        def plain_steps(n):
            for _ in range(n // per):
                g_p.replay()

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    autograd_steps(8)
    native_prologue()
    native_steps(per * 2)
    steps = max(per, min(a.steps, st.n_pairs // B - 1) // per * per)
    t_auto, t_nat, t_plain = [], [], []
    if plain is not None:
        plain_prologue()
        plain_steps(per * 2)
    for _ in range(a.rounds):                            # alternating, same box, same process
        t_auto.append(timed(autograd_steps, steps))
        native_prologue()
        t_nat.append(timed(native_steps, steps))
        if plain is not None:
            plain_prologue()
            t_plain.append(timed(plain_steps, steps))

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
    l_nat = launches(lambda n: [tr.step_on_batch(bf, xi=i % 2, next_from=st) for i in range(n)], 4)[0]
    flop = step_flop(m, F, C)
    us_a, us_n = float(np.median(t_auto)), float(np.median(t_nat))
    extra = {}
    if plain is not None:
        spread = max(t_auto) - min(t_auto)
        extra = {"momentum": a.momentum, "optimizer": a.optimizer or "RMSprop", "autograd_spread_us": round(spread, 2),
                 "native_below_autograd_by_more_than_its_spread": bool(us_a - us_n > spread),
                 "default_native_us_per_step": round(float(np.median(t_plain)), 2), "default_native_rounds_us": [round(t, 2) for t in t_plain]}
    line = json.dumps({**extra, "tool": "bench_small_step", "m": m, "F": F, "C": C, "n_pairs": st.n_pairs, "steps_per_round": steps,
                      "autograd_us_per_step": round(us_a, 2), "native_us_per_step": round(us_n, 2), "speedup": round(us_a / us_n, 2),
                      "autograd_rounds_us": [round(t, 2) for t in t_auto], "native_rounds_us": [round(t, 2) for t in t_nat],
                      "launches_per_step": {"autograd": l_auto, "native": l_nat}, "library_gemms_per_step_autograd": lib_auto,
                      "flop_per_step": flop, "native_tflops": round(flop / (us_n * 1e-6) / 1e12, 2),
                      "native_share_of_fp32_matrix_peak": round(flop / (us_n * 1e-6) / PEAK_FP32_MATRIX, 4),
                      "device": torch.cuda.get_device_name(0)})
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
