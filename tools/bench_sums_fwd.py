#!/usr/bin/env python3
"""Times an epoch of the lone voter's two-plane step (NetLinear(4096, 20) + RMSprop, cfg2's shape) with the forward middle as a launch of its own
(fused.VARIANTS['sums_fwd'] = 0: seven launches a step) and inside the launch that adds layer 1's partial sums (sums_fwd = 1, 8 rows a workgroup: six
launches), on the same GPU, in the same process, alternating the legs.

Input: a seeded synthetic feature store of 100 000 rows x 4 views x 4096 features, batch 512 (m = 1024 rows a step; 585 full batches + a partial one an epoch:
586 steps a leg).  Prints one JSON line: every round, the median ms of an epoch and the spread (max - min) of each leg, us per step, and for the merged leg
whether it clears the rule for the default -- its median below the seven-launch median by more than three times the larger of the two spreads.

Usage:  python tools/bench_sums_fwd.py [--rounds R]
        python tools/bench_sums_fwd.py --only 0        (one leg alone: "0" or "8"; "0" also runs on a tree without the merged launch)
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_lockstep_rows import Store      # noqa: E402  (the seeded synthetic store)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--clusters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--only", default="")
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
    legs = [a.only] if a.only else ["0", "8"]

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    epochs = {}
    for leg in legs:
        if "sums_fwd" in fused.VARIANTS:
            fused.VARIANTS["sums_fwd"] = "0" if leg == "0" else "1"
        elif leg != "0":
            raise SystemExit("this tree has no merged launch: --only 0")
        tr = fused.FusedLinearTrainer(copy.deepcopy(net0), 1e-3, 0.25, 2.8, seed=0)
        gen = torch.Generator(device=dev).manual_seed(99)

        def epoch(tr=tr, gen=gen):
            tr.begin_voter(0)
            tr.run_epoch(st, B, generator=gen)

        epoch()                                             # warm-up: allocations, the captured graph
        torch.cuda.synchronize()
        assert tr._form(tr.buffers(2 * B), st) == "planes" and not tr.planes_overflowed()
        assert bool(getattr(tr, "_sums_fwd", False)) == (leg != "0")
        epochs[leg] = epoch
    t = {leg: [] for leg in legs}
    for _ in range(a.rounds):                               # alternating, same box, same process
        for leg in legs:
            t[leg].append(timed(epochs[leg]))
    out = {"tool": "bench_sums_fwd", "C": C, "m": 2 * B, "F": F, "steps_per_epoch": n_steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    med = {leg: float(np.median(t[leg])) for leg in legs}
    spread = {leg: max(t[leg]) - min(t[leg]) for leg in legs}
    for leg in legs:
        name = "seven_launches" if leg == "0" else "merged_rows%s" % leg
        out[name] = {"epoch_ms_median": round(med[leg], 3), "spread_ms": round(spread[leg], 3), "us_per_step": round(med[leg] * 1e3 / n_steps, 2),
                     "rounds_ms": [round(x, 3) for x in t[leg]]}
        if leg != "0" and "0" in med:
            out[name]["gain_ms"] = round(med["0"] - med[leg], 3)
            out[name]["is_default_by_the_rule"] = bool(med[leg] < med["0"] - 3.0 * max(spread["0"], spread[leg]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
