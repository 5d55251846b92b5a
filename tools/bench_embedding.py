#!/usr/bin/env python3
"""Stage times of the embedding behind --plot (posthoc.umap_embedding_device): kNN graph, calibration + union, layout, on blob
data (20 blobs in 64-d, centres N(0, 1) per coordinate, spread 1) at 10^5 and 10^6 points, one process, median of 3.
Appends one JSON line per size to profiles/<round>_embedding.jsonl.  There is no bar on these times (nothing to compare with:
umap-learn is absent); DESIGN.md section 7 records them.
  python tools/bench_embedding.py [--sizes 100000,1000000] [--reps 3] [--round rNN]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from idelucs_amd import posthoc



def next_round():
    """rNN after the highest round that has a file in profiles/."""
    import re
    seen = [int(m.group(1)) for f in os.listdir(os.path.join(ROOT, "profiles")) for m in [re.match(r"r(\d+)_", f)] if m]
    return "r%02d" % (max(seen, default=0) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="100000,1000000"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--round", type=str, default=None, help="default: the round after the highest rNN_ file in profiles/"); ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", f"{a.round or next_round()}_embedding.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    posthoc.umap_embedding_device(np.random.default_rng(0).normal(size=(4096, 64)).astype(np.float32), n_epochs=10)      # warm-up: library load, torch kernels
    for n in (int(s) for s in a.sizes.split(",")):
        rng = np.random.default_rng(7)
        centres = rng.normal(size=(20, 64)).astype(np.float32)
        x = centres[rng.integers(0, 20, size=n)] + rng.standard_normal(size=(n, 64), dtype=np.float32)
        runs = []
        for rep in range(a.reps):
            stats = {}
            t0 = time.perf_counter()
            y = posthoc.umap_embedding_device(x, stats=stats)
            stats["total_s"] = time.perf_counter() - t0
            assert y.shape == (n, 2) and np.all(np.isfinite(y))
            runs.append(stats)
            print(f"n = {n} rep {rep}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in stats.items()), flush=True)
        med = {k: statistics.median(r[k] for r in runs) for k in ("knn_s", "graph_s", "layout_s", "total_s")}
        rec = {"n": n, "d": 64, "n_neighbors": posthoc.UMAP_NEIGHBORS, "n_epochs": posthoc.umap_default_epochs(n), "entries": runs[0]["entries"],
               "graph_path": runs[0]["graph_path"], "reps": a.reps, "median_s": med, "layout_ms_per_epoch": 1e3 * med["layout_s"] / posthoc.umap_default_epochs(n),
               "max_abs_coordinate": float(np.abs(y).max()), "device": torch.cuda.get_device_name(0)}
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
