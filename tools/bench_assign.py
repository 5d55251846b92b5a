#!/usr/bin/env python3
"""Times what FittedEnsemble.assign costs (idelucs_amd/ensemble.py):

  1. idl_nn_rows -- every query's exact nearest corpus row, float64 from the difference vector -- at (m, n) = (10^5, 10^6) points of 64
     coordinates, against the float32 Gram-form chunked search fine_grained_clusters(mode="approx") runs in torch (|q|^2 + |x|^2 - 2 q x^T
     on a chunk of queries, clamped at 0, min over the row; chunks of 4096 queries here: a [4096, 10^6] float32 block is 16 GB).  Same GPU,
     same process, legs alternating; the median of the rounds, their spread, and the share of queries for which the float32 search names
     another neighbour than the exact one.  The points: a seeded mixture of 64 Gaussian blobs (centres of scale 3, widths 0.2 .. 0.8);
     the queries are fresh draws from the same mixture.
  2. assign end to end on tests/data/Influenza-A.fas (949 records, k = 6) in both modes, from the file on disk to the labels on the host:
     an ensemble of 5 voters x 5 clusters and a fine-grained one (--n_clusters 0), trained here for a few epochs with --save_model.

Prints one JSON line per part and appends them to --out.

Usage:  python tools/bench_assign.py [--m 100000] [--n 1000000] [--rounds 5] [--out profiles/assign.jsonl]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _points(n, seed, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    gc = torch.Generator(device=dev).manual_seed(12345)                # the mixture is the same for corpus and queries
    centres = torch.randn(64, 64, device=dev, generator=gc) * 3.0
    width = torch.rand(64, device=dev, generator=gc) * 0.6 + 0.2
    which = torch.randint(0, 64, (n,), device=dev, generator=g)
    return (centres[which] + torch.randn(n, 64, device=dev, generator=g) * width[which][:, None]).contiguous()


def gram_search(q, x, x2, chunk=4096):
    """fine_grained_clusters(mode="approx")'s search of the nearest sampled point, in its own words."""
    import torch
    near = torch.empty(len(q), dtype=torch.int64, device=q.device)
    dist = torch.empty(len(q), dtype=torch.float32, device=q.device)
    for lo in range(0, len(q), chunk):
        xb = q[lo:lo + chunk]
        d2 = ((xb * xb).sum(1)[:, None] + x2[None, :] - 2.0 * (xb @ x.t())).clamp_min_(0.0)
        m = d2.min(1)
        near[lo:lo + chunk] = m.indices
        dist[lo:lo + chunk] = m.values.sqrt_()
    return near, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from idelucs_amd import _lib, ensemble
    from idelucs_amd.__main__ import main as cli
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    lines = []

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    # ---- 1. the search
    x, q = _points(a.n, 1, dev), _points(a.m, 2, dev)
    x2 = (x * x).sum(1)
    legs = {"idl_nn_rows": lambda: ensemble.nn_rows(q, x), "gram_f32": lambda: gram_search(q, x, x2)}
    out = {name: fn() for name, fn in legs.items()}                   # warm-up: allocations, the library's GEMM choice
    t = {name: [] for name in legs}
    for _ in range(a.rounds):                                         # alternating, same box, same process
        for name, fn in legs.items():
            ms, out[name] = timed(fn)
            t[name].append(ms)
    exact_idx, exact_d2 = out["idl_nn_rows"]
    near, dist = out["gram_f32"]
    other = near != exact_idx.long()
    # of those, the ones whose float32 choice is truly further away (not another row at the same exact distance)
    far = torch.zeros_like(other)
    if bool(other.any()):
        rows = other.nonzero().squeeze(1)
        d_alt = ((q[rows].double() - x[near[rows]].double()) ** 2).sum(1)
        far[rows] = d_alt > exact_d2[rows]
    rec = {"tool": "bench_assign", "part": "nn_rows", "m": a.m, "n": a.n, "d": 64, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "slices": int(_lib.lib.idl_nn_rows_slices(a.m, a.n))}
    for name in legs:
        rec[name] = {"ms_median": round(float(np.median(t[name])), 2), "spread_ms": round(max(t[name]) - min(t[name]), 2),
                     "rounds_ms": [round(v, 2) for v in t[name]]}
    rec["pairs_per_s_idl_nn_rows"] = round(a.m * a.n / (rec["idl_nn_rows"]["ms_median"] * 1e-3), -6)
    rec["gram_f32_names_another_neighbour"] = round(float(other.double().mean()), 6)
    rec["gram_f32_neighbour_truly_further"] = round(float(far.double().mean()), 6)
    rec["queries_at_gram_distance_0"] = int((dist == 0).sum())
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    del x, q, x2, out, near, dist, exact_idx, exact_d2
    torch.cuda.empty_cache()

    # ---- 2. assign end to end
    fasta = os.path.join(ROOT, "tests", "data", "Influenza-A.fas")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for mode, extra in (("ensemble", ["--n_clusters", "5", "--n_voters", "5"]), ("fine", ["--n_clusters", "0", "--n_voters", "2"])):
                model_dir = os.path.join(tmp, "model_" + mode)
                with contextlib.redirect_stdout(io.StringIO()):
                    cli(["--sequence_file", fasta, "--k", "6", "--batch_sz", "256", "--n_epochs", str(a.epochs), "--save_model", model_dir] + extra)
                ens = ensemble.FittedEnsemble.load(model_dir)
                ens.assign(fasta, dev)                                # warm-up
                ts = []
                for _ in range(a.rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    names, y, conf = ens.assign(fasta, dev)
                    ts.append(1e3 * (time.perf_counter() - t0))
                rec = {"tool": "bench_assign", "part": "assign", "mode": mode, "file": "Influenza-A.fas", "records": len(names), "k": 6,
                       "voters_saved": len(ens.states), "clusters_named": int(len(set(y.tolist()))), "rounds": a.rounds,
                       "ms_median": round(float(np.median(ts)), 2), "spread_ms": round(max(ts) - min(ts), 2), "rounds_ms": [round(v, 2) for v in ts],
                       "file_bytes": os.path.getsize(model_dir + "/ensemble.pt"), "device": torch.cuda.get_device_name(0)}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
        finally:
            os.chdir(cwd)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
