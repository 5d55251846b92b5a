#!/usr/bin/env python3
"""Times an epoch of L voters of the fine-grained mode (NetLinear(4096, 200) + RMSprop, the two-plane step of n_clusters > 48) one after the
other and in lockstep, on the same GPU, in the same process, alternating the two: the sequential leg is one FusedLinearTrainer serving the
voters in turn (what training.train_voter runs; replays of its captured graph), the lockstep leg fused.BatchedLinearTrainer (the eight
launches of the step recorded per voter and run once for all of them).

Input: a seeded synthetic feature store of 100 000 rows x 4 views x 4096 features, C = 200, batch 512 (m = 1024 rows a step, 585 full batches +
a partial one an epoch).  Prints one JSON line per L in {2, 3, 4, 5, 8}: the median ms of a voter-epoch in both legs, every round, us per step
and voter, and whether lockstep clears the rule for training.voter_lanes' default (its median below the sequential median by more than the
sequential rounds' own spread, max - min).

Usage:  python tools/bench_lockstep_rows.py [--rounds R] [--lanes 2,3,4,5,8]
        python tools/bench_lockstep_rows.py --only-lockstep 5 --epochs 2      (the lockstep leg alone, for a kernel trace)
        python tools/bench_lockstep_rows.py --only-sequential 5               (the sequential leg alone: also runs on a tree without the lockstep form)
"""
import argparse
import copy
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lanes", default="2,3,4,5,8")
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--clusters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--only-lockstep", dest="only", type=int, default=0)
    ap.add_argument("--only-sequential", dest="only_seq", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    from idelucs_amd import _lib, models
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.fused import FusedLinearTrainer, BatchedLinearTrainer
    _lib.require_gpu()
    dev = torch.device("cuda")
    F, C, B = 4096, a.clusters, a.batch
    st = Store(a.n, 3, F, dev, seed=7)
    n_steps = -(-st.n_pairs // B)
    torch.manual_seed(0)
    net0 = NetLinear(F, C).to(dev)
    net0.apply(models.weights_init)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def lockstep_of(L):
        bt = BatchedLinearTrainer([copy.deepcopy(net0) for _ in range(L)], 1e-3, 0.25, 2.8, seed=0)
        gens = [torch.Generator(device=dev).manual_seed(100 + l) for l in range(L)]
        for l, t in enumerate(bt.trainers):
            t.begin_voter(l)
        return bt, (lambda: bt.run_epoch(st, B, gens))

    if a.only:
        bt, epoch = lockstep_of(a.only)
        for _ in range(a.epochs):
            epoch()
        torch.cuda.synchronize()
        assert bt._planes_step and not bt.planes_overflowed()
        return

    # the sequential leg: one trainer, the voters in turn (each a begin_voter and an epoch, as training.train_voter does)
    lone = FusedLinearTrainer(copy.deepcopy(net0), 1e-3, 0.25, 2.8, seed=0)
    gen = torch.Generator(device=dev).manual_seed(99)

    def sequential(L):
        for l in range(L):
            lone.begin_voter(l)
            lone.run_epoch(st, B, generator=gen)

    sequential(1)                                       # warm-up: allocations, the captured graph
    assert lone._form(lone.buffers(2 * B), st) == "planes_rows" and not lone.planes_overflowed()
    if a.only_seq:
        L = a.only_seq
        t_seq = [timed(lambda: sequential(L)) / L for _ in range(a.rounds)]
        print(json.dumps({"tool": "bench_lockstep_rows", "lanes": L, "C": C, "sequential_ms_per_voter_epoch": round(float(np.median(t_seq)), 3),
                          "sequential_rounds_ms": [round(t, 3) for t in t_seq]}), flush=True)
        return
    for L in [int(x) for x in a.lanes.split(",")]:
        bt, epoch = lockstep_of(L)
        epoch()                                         # warm-up: the recorded program, the captured graph
        torch.cuda.synchronize()
        assert bt._planes_step and not bt.planes_overflowed()
        t_seq, t_lock = [], []
        for _ in range(a.rounds):                       # alternating, same box, same process
            t_seq.append(timed(lambda: sequential(L)) / L)
            t_lock.append(timed(epoch) / L)
        med_s, med_l = float(np.median(t_seq)), float(np.median(t_lock))
        spread = max(t_seq) - min(t_seq)
        print(json.dumps({"tool": "bench_lockstep_rows", "lanes": L, "C": C, "m": 2 * B, "F": F, "steps_per_epoch": n_steps,
                          "sequential_ms_per_voter_epoch": round(med_s, 3), "lockstep_ms_per_voter_epoch": round(med_l, 3),
                          "sequential_rounds_ms": [round(t, 3) for t in t_seq], "lockstep_rounds_ms": [round(t, 3) for t in t_lock],
                          "sequential_us_per_step_and_voter": round(med_s * 1e3 / n_steps, 2),
                          "lockstep_us_per_step_and_voter": round(med_l * 1e3 / n_steps, 2),
                          "sequential_spread_ms": round(spread, 3), "lockstep_is_default_by_the_rule": bool(med_l < med_s - spread),
                          "device": torch.cuda.get_device_name(0)}), flush=True)
        del bt, epoch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
