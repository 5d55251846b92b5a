#!/usr/bin/env python3
"""Times myNet's eval forward (model_size='small') on both predict paths and layer 1 on both of its launches:

  l1_fwd          idl_small_l1_fwd (the training step's layer 1: 16 rows x 80 units a workgroup, every lane its own global reads);
  l1_predict      idl_small_predict_l1 (128 rows x 400 units a workgroup, the operands' K stages shared through LDS);
                  both on the predictor's blocks (at most 32 768 rows), into the same scratch;
  torch           self.net(x) in 32 768-row chunks and torch.max of the outputs, as IID_model._predict_outputs + predict do (hipBLASLt);
  native          predict_native.NativeSmallPredictor.forward(x): idl_small_predict_l1 + idl_small_predict_mid per block.

n rows of F' standardised entries resident on the device (default 100 000, 20 classes), at k = 4, 5, 6, 7 (F' = 136, 512, 2080, 8192).  Same GPU,
same process, the four legs alternating after a warm-up of all; every round is `reps` passes between two device events.  Reports the median of
the rounds with their spread, whether the new layer 1 qualifies at that width (k = 6: its median below l1_fwd's by more than the larger of the two
spreads; elsewhere: not above it beyond the spread), the ratio of the two whole paths, and how far their outputs are apart.  There is no speed bar
against torch: the native path's claim is reproducibility.

Prints one JSON line per k and appends it to --out.

Usage:  python tools/bench_small_predict.py [--n 100000] [--ks 4,5,6,7] [--c 20] [--rounds 5] [--reps 20] [--out profiles/small_predict_native.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def n_features(k):
    return (4 ** k + 4 ** (k // 2)) // 2 if k % 2 == 0 else (4 ** k) // 2


def bench_k(a, k):
    import numpy as np
    import torch
    from idelucs_amd import _lib, predict_native as P
    from idelucs_amd.models import weights_init
    from idelucs_amd.PytorchUtils import myNet
    dev = torch.device("cuda", 0)
    F = n_features(k)
    g = torch.Generator(device=dev).manual_seed(1)
    net = myNet(F, a.c).to(dev).eval()
    net.apply(lambda mod: weights_init(mod, g))
    with torch.no_grad():
        for lin in (net.layers[0], net.layers[3], net.instance, net.classifier[1]):
            lin.bias.copy_(torch.randn(lin.bias.shape, device=dev, generator=g) * 0.1)
    x = torch.randn((a.n, F), device=dev, generator=g)
    pred = P.NativeSmallPredictor(net)
    blk = P.small_block_rows(F)
    a1 = torch.empty((min(blk, a.n), P.SH1), dtype=torch.float32, device=dev)
    W1 = net.layers[0].weight
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def l1_leg(fn):
        def leg():
            for lo in range(0, a.n, blk):
                r = min(blk, a.n - lo)
                _lib.check(fn(ptr(x[lo:]), ptr(W1), r, F, ptr(a1), stream()))
            return a1
        return leg

    def torch_leg():
        outs, lats = [], []
        with torch.no_grad():
            for i in range(0, a.n, 32768):
                o, l = net(x[i:i + 32768])
                outs.append(o)
                lats.append(l)
            prob, unit = torch.max(torch.cat(outs), 1)
        return torch.cat(lats), prob, unit

    def native_leg():
        lat, prob, unit, _ = pred.forward(x)
        return lat, prob, unit

    legs = {"l1_fwd": l1_leg(_lib.lib.idl_small_l1_fwd), "l1_predict": l1_leg(_lib.lib.idl_small_predict_l1), "torch": torch_leg, "native": native_leg}
    out = {}
    for name, fn in legs.items():                                     # warm-up: code objects, allocations, the library's GEMM choice
        res = fn()
        out[name] = res.clone() if name.startswith("l1") else res     # (l1: the LAST block's a1, for the comparison below)
    for fn in legs.values():
        fn()
    t = {name: [] for name in legs}
    for _ in range(a.rounds):                                         # alternating, same box, same process
        for name, fn in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[name].append(e0.elapsed_time(e1) / a.reps)
    rec = {"tool": "bench_small_predict", "k": k, "n": a.n, "F": F, "C": a.c, "block_rows": blk, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for name in legs:
        rec[name] = {"ms_median": round(float(np.median(t[name])), 4), "spread_ms": round(max(t[name]) - min(t[name]), 4),
                     "rounds_ms": [round(v, 4) for v in t[name]]}
    old, new = rec["l1_fwd"], rec["l1_predict"]
    spread = max(old["spread_ms"], new["spread_ms"])
    rec["l1_spread_ms"] = spread
    rec["l1_ratio_fwd_over_predict"] = round(old["ms_median"] / new["ms_median"], 3)
    rec["l1_predict_below_by_more_than_spread"] = bool(old["ms_median"] - new["ms_median"] > spread)
    rec["l1_predict_not_above_beyond_spread"] = bool(new["ms_median"] <= old["ms_median"] + spread)
    rec["l1_tflops_predict"] = round(2.0 * a.n * F * P.SH1 / (new["ms_median"] * 1e-3) / 1e12, 2)
    rec["l1_tflops_fwd"] = round(2.0 * a.n * F * P.SH1 / (old["ms_median"] * 1e-3) / 1e12, 2)
    rec["ratio_native_over_torch"] = round(rec["native"]["ms_median"] / rec["torch"]["ms_median"], 3)
    rec["rounds_overlap_native_torch"] = bool(max(min(t["native"]), min(t["torch"])) <= min(max(t["native"]), max(t["torch"])))
    rec["input_gbytes_per_s_native"] = round(4.0 * a.n * F / (rec["native"]["ms_median"] * 1e-3) / 1e9, 1)
    (lat_t, prob_t, unit_t), (lat_n, prob_n, unit_n) = out["torch"], out["native"]
    rec["max_abs_latent_difference"] = float((lat_t - lat_n).abs().max())
    rec["max_abs_prob_difference"] = float((prob_t - prob_n).abs().max())
    rec["units_differing"] = int((unit_t != unit_n.long()).sum())
    rec["max_abs_a1_difference_between_layer1s"] = float((out["l1_fwd"] - out["l1_predict"]).abs().max())
    rec["a1_entries_differing_between_layer1s"] = int((out["l1_fwd"] != out["l1_predict"]).sum())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--ks", type=str, default="4,5,6,7")
    ap.add_argument("--c", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_predict_native.jsonl"))
    a = ap.parse_args()
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    for k in (int(s) for s in a.ks.split(",")):
        rec = bench_k(a, k)
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
