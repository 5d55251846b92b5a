#!/usr/bin/env python3
"""Times the k = 8 / 9 vectoriser (csrc/vectorise_slices.h) against a device fill of the same bytes, in the same process.

Shapes: 20 000 x 10 kbp x 4 views at k = 8 and 5 000 x 10 kbp x 4 views at k = 9 (21 GB of float32 rows each), with device-drawn
mimic edits and without.  The kernel and the fill alternate inside one timed loop (device events, a warm-up of every shape first);
the yardstick is the fill's rate on this box in this run, not a nominal bandwidth.  With --epoch, one training epoch at k = 8 on
the store just built is timed too, for each step form that runs there (the two-plane form and IDELUCS_PLANES=0's fp32 tiles).

    python tools/bench_vectorise_large_k.py [--reps 5] [--epoch] [--out profiles/r10_vectorise_large_k.txt]
"""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, reps):
    """Best and median ms of each callable, the callables alternating within every repetition."""
    import torch
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            ms[i].append(s.elapsed_time(e))
    return [(min(m), sorted(m)[len(m) // 2]) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--shapes", default="8:20000,9:5000")
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from idelucs_amd import _lib, utils as U
    _lib.require_gpu()
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    dev = torch.device("cuda")
    lines = [f"# {torch.cuda.get_device_name(0)}; ms per launch: best (median) of {a.reps}, kernel and fill alternating"]
    P, L = 4, a.length
    for item in a.shapes.split(","):
        k, n = (int(t) for t in item.split(":"))
        din = bench.synth_packed(n, L, dev, seed=7)
        edits, edit_off = U._philox_edits(din, [t.spec() for t in U.mimic_transforms(P - 1)], 3)
        out = torch.empty((P, n, 4 ** k), dtype=torch.float32, device=dev)
        gb = out.numel() * 4 / 1e9
        plain = lambda: U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_FREQ_F32, P, out=out)
        mimic = lambda: U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_FREQ_F32, P, edits, edit_off, out=out)
        fill = lambda: out.fill_(1.0)
        (tp, mp), (te, me), (tf, mf) = timed([plain, mimic, fill], a.reps)
        lines.append(f"k={k} n={n} L={L} views={P} rows={gb:.2f} GB: no edits {tp:.2f} ({mp:.2f}) ms = {gb / tp * 1e3:.0f} GB/s; "
                     f"with edits {te:.2f} ({me:.2f}) ms = {gb / te * 1e3:.0f} GB/s; fill {tf:.2f} ({mf:.2f}) ms = {gb / tf * 1e3:.0f} GB/s; "
                     f"kernel / fill = {te / tf:.2f}")
        print(lines[-1], flush=True)
        if a.epoch and k == 8:
            import copy
            from idelucs_amd import models
            from idelucs_amd.PytorchUtils import NetLinear
            from idelucs_amd.fused import FusedLinearTrainer
            mimic()
            mean, scale = U.col_stats(out[0])
            store = U.FeatureStore(None, None, out, mean, scale, k, False)
            torch.manual_seed(3)
            net0 = NetLinear(4 ** k, 5).to(dev); net0.apply(models.weights_init)
            for planes in ("1", "0"):
                os.environ["IDELUCS_PLANES"] = planes
                tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=5)
                gen = torch.Generator(device=dev); gen.manual_seed(7)
                form = tr._form(tr.buffers(512), store)
                (t1, m1), = timed([lambda: tr.run_epoch(store, 256, use_graph=True, generator=gen)], 3)
                lines.append(f"k={k} epoch of {store.n_pairs} pairs, batch 256, step form '{form}': {t1:.1f} ({m1:.1f}) ms")
                print(lines[-1], flush=True)
                del tr
            del store, net0
        del out, din, edits, edit_off
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
