#!/usr/bin/env python3
"""Times a training epoch of NetLinear + RMSprop (fused.FusedLinearTrainer.run_epoch, graph replays included) on the resident feature
store and on the streamed one (utils.StreamedFeatureStore: every batch vectorised from the packed bases by one added launch a step), on
the same GPU, in the same process, alternating the routes after a warm-up.

Routes: 'resident' -- the default step of the shape (the two-plane form where it applies): the yardstick -- and 'streamed', the same step
form with the added launch; 'resident_fp32' / 'streamed_fp32' -- the same pair with IDELUCS_PLANES=0 (the fp32 tiles).  Shapes: cfg2's
(100 000 x 10 kbp, k = 6, batch 512) and 20 000 x 10 kbp at k = 8, batch 256, on seeded synthetic bases.  Per shape one JSON line: epoch
ms and us per step of every route (device events, median of --rounds, and the rounds), the added launch's own time (median of
--launches back-to-back launches of one batch: planes only, as the two-plane form asks for it, and fp32), and the peak device memory of
build + one epoch above the level before, per store.

Usage:  python tools/bench_streamed_store.py [--rounds 7] [--out profiles/streamed_store.jsonl] [--shapes k6 k8]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"k6": dict(n=100_000, length=10_000, k=6, batch=512, n_clusters=20),
          "k8": dict(n=20_000, length=10_000, k=8, batch=256, n_clusters=20)}


def synthetic_input(n, L, dev, seed=0):
    """n sequences of L uniform random bases as the vectoriser's packed device input (64 bases a slot: 16 bytes of 2-bit codes, 8 of invalid bits)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    slots = (L + 63) // 64
    codes = torch.empty(n * slots * 4, dtype=torch.int32, device=dev)
    step = 1 << 26
    for lo in range(0, codes.numel(), step):
        hi = min(lo + step, codes.numel())
        codes[lo:hi] = torch.randint(-2 ** 31, 2 ** 31 - 1, (hi - lo,), dtype=torch.int32, device=dev, generator=g)
    mask = torch.zeros((n, slots, 2), dtype=torch.int32, device=dev)
    if L % 64:                   # bases past the end of the sequence are invalid
        w = [0, 0]
        for j in range(L % 64, 64):
            w[j // 32] |= 1 << (31 - (j % 32))
        for i in (0, 1):
            mask[:, -1, i] = w[i] - (1 << 32) if w[i] >= 2 ** 31 else w[i]

    class DeviceInput:
        pass
    d = DeviceInput()
    d.n, d.codes, d.mask = n, codes.view(torch.uint8), mask.view(-1).view(torch.uint8)
    d.slot_off = torch.arange(0, (n + 1) * slots, slots, dtype=torch.int64, device=dev)
    d.lengths = torch.full((n,), L, dtype=torch.int64, device=dev)
    d.max_len = d.min_len = L
    d.total_len = n * L
    return d


def bench(name, sh, a, dev):
    import numpy as np
    import torch
    from idelucs_amd import _lib, models, utils as U
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.fused import FusedLinearTrainer
    n, k, B, C = sh["n"], sh["k"], sh["batch"], sh["n_clusters"]
    F = 4 ** k
    din = synthetic_input(n, sh["length"], dev)
    tfs = U.mimic_transforms(3)
    edits, eo = U._philox_edits(din, [t.spec() for t in tfs], 0)
    ranges = U._edit_ranges(eo, len(tfs) * n)

    def level():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        return torch.cuda.memory_allocated()

    def trainer(planes):
        os.environ["IDELUCS_PLANES"] = planes
        torch.manual_seed(0)
        net = NetLinear(F, C).to(dev)
        net.apply(models.weights_init)
        tr = FusedLinearTrainer(net, 1e-3, 0.25, 2.8, seed=0)
        tr.begin_voter(0)
        return tr

    peaks, stores, trainers, gens = {}, {}, {}, {}
    # ---- streamed: the scaler from one chunked pass over view 0, then an epoch (the capture included)
    base = level()
    mean, scale = U.col_stats_of_view0(din, k, edits, ranges)
    stores["streamed"] = U.StreamedFeatureStore(None, None, din, edits, ranges, mean, scale, k, len(tfs))
    trainers["streamed"] = trainer("1")
    gens["streamed"] = torch.Generator(device=dev).manual_seed(1)
    n_batches = trainers["streamed"].run_epoch(stores["streamed"], B, generator=gens["streamed"])[1]
    torch.cuda.synchronize()
    peaks["streamed"] = torch.cuda.max_memory_allocated() - base
    # ---- resident: the whole store, its scaler, an epoch
    base = level()
    feats = U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_FREQ_F32, len(tfs), edits, eo)
    rmean, rscale = U.col_stats(feats[0])
    stores["resident"] = stores["resident_fp32"] = U.FeatureStore(None, None, feats, rmean, rscale, k, False)
    assert torch.equal(rmean, mean) and torch.equal(rscale, scale), "the chunked scaler fit differs from idl_col_stats"
    trainers["resident"] = trainer("1")
    gens["resident"] = torch.Generator(device=dev).manual_seed(1)
    trainers["resident"].run_epoch(stores["resident"], B, generator=gens["resident"])
    torch.cuda.synchronize()
    peaks["resident"] = torch.cuda.max_memory_allocated() - base
    stores["streamed_fp32"] = stores["streamed"]
    for r in ("resident_fp32", "streamed_fp32"):
        trainers[r] = trainer("0")
        gens[r] = torch.Generator(device=dev).manual_seed(1)
    routes = ["resident", "streamed", "resident_fp32", "streamed_fp32"]
    bf = trainers["streamed"].buffers(2 * B)
    forms = {r: trainers[r]._form(trainers[r].buffers(2 * B), stores[r]) for r in routes}

    def epoch(route):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        trainers[route].run_epoch(stores[route], B, generator=gens[route])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for r in routes:                                     # warm-up: every route's capture and one replayed epoch
        epoch(r)
        epoch(r)
    t = {r: [] for r in routes}
    for _ in range(a.rounds):                            # alternating, same box, same process
        for r in routes:
            t[r].append(epoch(r))

    # ---- the added launch alone: one batch from the packed bases, back to back
    st, tr = stores["streamed"], trainers["streamed"]
    tr.ctl[1:2].zero_()
    ph, pl = (torch.empty((2 * B, F), dtype=torch.int16, device=dev) for _ in range(2))
    pflag = torch.zeros(1, dtype=torch.int32, device=dev)
    t_launch, t_launch_planes = [], []
    for dst, y, kw in ((t_launch, bf.xs[1], {}), (t_launch_planes, None, dict(planes=(ph, pl), flag=pflag))):
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                st.pairs_at(tr._perm, tr.ctl[1:], B, B, st.n_pairs, y, **kw)
            e1.record()
            torch.cuda.synchronize()
            dst.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    # ... and the resident store's own assembly of a batch as a launch of its own, for scale
    t_gather = []
    rs = stores["resident"]
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            rs.gather_pairs(tr._perm[:B], out=bf.xs[1])
        e1.record()
        torch.cuda.synchronize()
        t_gather.append(e0.elapsed_time(e1) * 1e3 / a.launches)

    med = {r: float(np.median(t[r])) for r in routes}
    res = {"tool": "bench_streamed_store", "shape": name, "n": n, "length": sh["length"], "k": k, "F": F, "batch": B, "n_clusters": C,
           "n_pairs": st.n_pairs, "steps_per_epoch": n_batches, "rounds": a.rounds, "step_form": forms,
           "epoch_ms": {r: round(med[r], 3) for r in routes}, "us_per_step": {r: round(med[r] * 1e3 / n_batches, 2) for r in routes},
           "epoch_rounds_ms": {r: [round(x, 3) for x in t[r]] for r in routes},
           "streamed_over_resident": round(med["streamed"] / med["resident"], 4),
           "streamed_fp32_over_resident_fp32": round(med["streamed_fp32"] / med["resident_fp32"], 4),
           "added_launch_us": {"planes_only": round(float(np.median(t_launch_planes)), 2), "fp32": round(float(np.median(t_launch)), 2)},
           "added_launch_rounds_us": {"planes_only": [round(x, 2) for x in t_launch_planes], "fp32": [round(x, 2) for x in t_launch]},
           "resident_gather_launch_us": round(float(np.median(t_gather)), 2),
           "peak_memory_mb": {r: round(peaks[r] / 1e6, 1) for r in peaks}, "resident_feats_mb": round(feats.numel() * 4 / 1e6, 1),
           "packed_input_mb": round((din.codes.numel() + din.mask.numel() + edits.numel() * 4 + ranges.numel() * 8) / 1e6, 1),
           "device": torch.cuda.get_device_name(0)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--shapes", nargs="+", default=["k6", "k8"], choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    dev = torch.device("cuda")
    for name in a.shapes:
        line = json.dumps(bench(name, SHAPES[name], a, dev))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
