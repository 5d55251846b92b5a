#!/usr/bin/env python3
"""Times an epoch of the lone voter's default step (NetLinear(4096, 20) + RMSprop, cfg2's shape, six launches a step) under the cache policies of its bulk
output stores (csrc/store_policy.h, IDELUCS_DEV=store_wt=<mask>): every store plain (mask 0), each site alone write-through (1 the next batch's planes,
2 layer 1's partial sums, 4 W1 and square_avg, 8 W1's planes), then -- in a second pass against mask 0 -- the union of the sites that won.  Same GPU, same
process, legs alternating.

Input: a seeded synthetic feature store of 100 000 rows x 4 views x 4096 features, batch 512 (m = 1024 rows a step; 585 full batches + a partial one an epoch:
586 steps a leg).  Prints one JSON line a pass: every round, the median ms of an epoch and the spread (max - min) of each leg, us per step, and for each leg
whether it clears the rule for the default -- its median below the mask-0 median by more than three times the larger of the two spreads.

Usage:  python tools/bench_store_policy.py [--rounds R] [--masks 0,1,2,4,8] [--out profiles/store_policy_ab.jsonl]
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_lockstep_rows import Store      # noqa: E402  (the seeded synthetic store)


def _set_mask(mask):
    keep = [kv for kv in os.environ.get("IDELUCS_DEV", "").split(",") if kv and kv.split("=")[0] != "store_wt"]
    os.environ["IDELUCS_DEV"] = ",".join(keep + ["store_wt=%d" % mask])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--clusters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--masks", default="0,1,2,4,8")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from idelucs_amd import _lib, fused, models
    from idelucs_amd.PytorchUtils import NetLinear
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

    epochs = {}

    def leg(mask):
        if mask in epochs:
            return epochs[mask]
        _set_mask(mask)
        assert int(_lib.lib.idl_store_wt_mask()) == mask
        tr = fused.FusedLinearTrainer(copy.deepcopy(net0), 1e-3, 0.25, 2.8, seed=0)
        gen = torch.Generator(device=dev).manual_seed(99)

        def epoch(tr=tr, gen=gen, mask=mask):
            _set_mask(mask)                                 # (the eager steps beside the captured graph read it at their launches)
            tr.begin_voter(0)
            tr.run_epoch(st, B, generator=gen)

        epoch()                                             # warm-up: allocations, the captured graph (which keeps this leg's mask)
        torch.cuda.synchronize()
        assert tr._form(tr.buffers(2 * B), st) == "planes" and tr._sums_fwd and not tr.planes_overflowed()
        epochs[mask] = epoch
        return epoch

    def one_pass(name, masks):
        fns = {m_: leg(m_) for m_ in masks}
        t = {m_: [] for m_ in masks}
        for _ in range(a.rounds):                           # alternating, same box, same process
            for m_ in masks:
                t[m_].append(timed(fns[m_]))
        out = {"tool": "bench_store_policy", "pass": name, "C": C, "m": 2 * B, "F": F, "steps_per_epoch": n_steps, "rounds": a.rounds,
               "device": torch.cuda.get_device_name(0)}
        med = {m_: float(np.median(t[m_])) for m_ in masks}
        spread = {m_: max(t[m_]) - min(t[m_]) for m_ in masks}
        won = []
        for m_ in masks:
            rec = {"epoch_ms_median": round(med[m_], 3), "spread_ms": round(spread[m_], 3), "us_per_step": round(med[m_] * 1e3 / n_steps, 2),
                   "rounds_ms": [round(x, 3) for x in t[m_]]}
            if m_ != 0 and 0 in med:
                rec["gain_ms"] = round(med[0] - med[m_], 3)
                rec["is_default_by_the_rule"] = bool(med[m_] < med[0] - 3.0 * max(spread[0], spread[m_]))
                if rec["is_default_by_the_rule"]:
                    won.append(m_)
            out["mask_%d" % m_] = rec
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        return won

    masks = [int(x, 0) for x in a.masks.split(",")]
    won = one_pass("sites", masks)
    union = 0
    for m_ in won:
        union |= m_
    if len(won) > 1:
        one_pass("union", [0, union])
    print(json.dumps({"tool": "bench_store_policy", "sites_that_won": won, "union": union}), flush=True)


if __name__ == "__main__":
    main()
