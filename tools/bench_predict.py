#!/usr/bin/env python3
"""Times NetLinear's eval forward on both of IID_model's predict paths:

  torch    self.net(x) in 32 768-row chunks and torch.max of the outputs, as IID_model._predict_outputs + predict do (nn.Linear: hipBLASLt);
  native   predict_native.NativeLinearPredictor.forward(x): idl_l1_fwd + idl_predict_mid in 32 768-row blocks.

Both produce the latent, the largest softmax value and its class of n rows of F standardised entries that are resident on the device
(default 100 000 x 4096, 20 classes: 1.6 GB of inputs).  Same GPU, same process, legs alternating after a warm-up of both; every round is
`reps` forwards between two device events.  Reports the median of the rounds with their spread, which path is faster and by how much, and how
far the two paths' outputs are apart (they sum in different orders).  There is no speed bar: the native path's claim is reproducibility.

Prints one JSON line and appends it to --out.

Usage:  python tools/bench_predict.py [--n 100000] [--f 4096] [--c 20] [--rounds 5] [--reps 5] [--out profiles/predict_native.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--f", type=int, default=4096)
    ap.add_argument("--c", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_native.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.models import weights_init
    from idelucs_amd.predict_native import NativeLinearPredictor
    from idelucs_amd.PytorchUtils import NetLinear
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    net = NetLinear(a.f, a.c).to(dev).eval()
    net.apply(lambda mod: weights_init(mod, g))
    with torch.no_grad():
        for lin in (net.layers[0], net.layers[3], net.classifier[2]):
            lin.bias.copy_(torch.randn(lin.bias.shape, device=dev, generator=g) * 0.1)
    x = torch.randn((a.n, a.f), device=dev, generator=g)
    pred = NativeLinearPredictor(net)

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

    legs = {"torch": torch_leg, "native": native_leg}
    out = {name: fn() for name, fn in legs.items()}                   # warm-up: code objects, allocations, the library's GEMM choice
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
    rec = {"tool": "bench_predict", "n": a.n, "F": a.f, "C": a.c, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name in legs:
        rec[name] = {"ms_median": round(float(np.median(t[name])), 3), "spread_ms": round(max(t[name]) - min(t[name]), 3),
                     "rounds_ms": [round(v, 3) for v in t[name]]}
    fast, slow = sorted(legs, key=lambda name: rec[name]["ms_median"])
    rec["faster"] = fast
    rec["ratio_slower_over_faster"] = round(rec[slow]["ms_median"] / rec[fast]["ms_median"], 3)
    # the spread decides whether the difference is one: the rounds of the two legs must not overlap
    rec["rounds_overlap"] = bool(max(t[fast]) >= min(t[slow]))
    flops = 2.0 * a.n * (a.f * 512 + 512 * 64 + 64 * a.c)
    rec["tflops_native"] = round(flops / (rec["native"]["ms_median"] * 1e-3) / 1e12, 2)
    rec["tflops_torch"] = round(flops / (rec["torch"]["ms_median"] * 1e-3) / 1e12, 2)
    rec["input_gbytes_per_s_native"] = round(4.0 * a.n * a.f / (rec["native"]["ms_median"] * 1e-3) / 1e9, 1)
    (lat_t, prob_t, unit_t), (lat_n, prob_n, unit_n) = out["torch"], out["native"]
    rec["max_abs_latent_difference"] = float((lat_t - lat_n).abs().max())
    rec["max_abs_prob_difference"] = float((prob_t - prob_n).abs().max())
    rec["units_differing"] = int((unit_t != unit_n.long()).sum())
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
