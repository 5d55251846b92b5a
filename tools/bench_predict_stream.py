#!/usr/bin/env python3
"""Times predict's inputs on the resident route (float64 rows [N, F] -> idl_col_stats -> idl_standardise) against the streamed route
(utils.feature_chunks_of_input: two passes over the packed bases, a chunk of rows at a time) at a shape where both fit.

Default shape: 20 000 x 10 kbp at k = 8 (the float64 rows are 10.5 GB, the float32 result 5.2 GB).  The streamed route runs with the chunk
budgets 1, 2, 4, 8 and 16 GiB (utils.PREDICT_STREAM_CHUNK_BYTES; 16 GiB is one chunk here).  All routes alternate inside every
repetition, after a warm-up of each, in which every streamed chunk is also compared with the resident rows bit for bit; times are device
events around work that ends in a synchronise, FASTA parsing excluded (the packed bases are generated on the device).  Per route: median,
best and worst of the repetitions, and the spread (worst - best) / median.

    python tools/bench_predict_stream.py [--reps 7] [--n 20000] [--length 10000] [--k 8] [--out profiles/predict_stream.txt]
"""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--budgets", default="1,2,4,8,16", help="chunk budgets in GiB")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from idelucs_amd import _lib, utils as U
    _lib.require_gpu()
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    dev = torch.device("cuda")
    n, k, f = a.n, a.k, 4 ** a.k
    din = bench.synth_packed(n, a.length, dev, seed=7, n_rate=1e-4)
    budgets = [int(b) for b in a.budgets.split(",")]

    def resident():
        f64 = U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_FREQ_F64)[0]
        mean, scale = U.col_stats(f64)
        return U.standardise(f64, mean, scale)

    def streamed(gib, want=None):
        rows = min(32768, max(256, (gib << 30) // (8 * f)))          # utils.predict_chunk_rows with this budget
        chunks = 0
        for lo, hi, x in U.feature_chunks_of_input(din, k, chunk_rows=rows):
            chunks += 1
            if want is not None:
                assert torch.equal(x, want[lo:hi]), (gib, lo, hi)
        return min(rows, n), chunks

    routes = [("resident", resident)] + [(f"streamed {g} GiB", (lambda g=g: streamed(g))) for g in budgets]
    want = resident()                                   # warm-up of every route; the streamed chunks against the resident rows
    shapes = {g: streamed(g, want) for g in budgets}
    del want
    torch.cuda.synchronize()              # (the allocator keeps every route's blocks: no timed repetition pays a fresh allocation)
    ms = {name: [] for name, _ in routes}
    peak = {}
    for rep in range(a.reps):
        for name, fn in routes:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn()
            e.record()
            torch.cuda.synchronize()
            del r
            ms[name].append(s.elapsed_time(e))
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    lines = [f"# {torch.cuda.get_device_name(0)} {arch}; predict inputs of {n} x {a.length} bp at k = {k} (F = {f}); ms: median (best .. worst) of {a.reps} "
             f"repetitions, the routes alternating; spread = (worst - best) / median; peak = device memory above the level before the call"]
    for name, _ in routes:
        m = sorted(ms[name])
        med = m[len(m) // 2]
        extra = ""
        if name != "resident":
            rows, chunks = shapes[int(name.split()[1])]
            extra = f"; {rows} rows per chunk, {chunks} chunks"
        lines.append(f"{name}: {med:.1f} ms ({m[0]:.1f} .. {m[-1]:.1f}), spread {100 * (m[-1] - m[0]) / med:.1f} %, peak {peak[name] / 2 ** 30:.2f} GiB{extra}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
