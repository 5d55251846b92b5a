#!/usr/bin/env python3
"""Bit identity of NetLinear's opt-in native step (fused_opt.FusedLinearOptTrainer, last launch idl_opt_step_gather_wgrad) across two
builds of the library AND the package: two eager epochs of the trainer per case on a feature store, a network and a permutation that all
come from fixed seeds, then a sha256 of every tensor the steps leave behind -- the six parameters, both state sets, dW2 (grads[2]), out,
ctl, the two step words and the batch buffer bf.x.  Prints one JSON line per case.

The trainer is driven, not the C entry: the entry's form differs between the builds this tool compares, the trainer's interface does not.
Cases: SGD, Adam and RMSprop with momentum 0.9, crossed with five routes to the last launch (ROUTES below: which operand loop of the dW2 tile
runs, who assembles the next batch, a partial last batch).  The second epoch starts with whichever parity of the step words the first left.

tests/linear_opt_last_launch_parent.jsonl is this tool's output on the tree and library of the commit before the last launch's arguments
became structs (a copy of this file run from that tree's tools/, which puts that tree first on sys.path);
tests/test_gpu_linear_opt_last_launch_bits.py replays the cases on the current tree and compares line for line.  Some routes take library
GEMMs, whose bits belong to the machine and the library version: record and replay on the same machine in the same session when comparing
two builds.

Usage:  python tools/linear_opt_last_launch_bits.py [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = ("SGD", "Adam", "RMSprop")
# (batch_sz, F, C, rows of the store): what the route reaches
ROUTES = [(16, 256, 5, 64),       # both middle launches early, r1 transposed, 8 rows a wave: the scalar transposed loop
          (256, 256, 5, 256),     # transposed, 128 rows a wave: the 128-row transposed loop
          (24, 68, 5, 64),        # early, general form: the row-major loop with a clamped tail
          (9, 68, 60, 64),        # not early: the last launch assembles the next batch; a partial last batch advances the offset itself
          (24, 68, 60, 64)]       # 48 < C <= 200 with the fused InfoNCE kernels
CASES = [(kind, b, F, C, n) for kind in KINDS for (b, F, C, n) in ROUTES]
MIMICS, EPOCHS, LR, WEIGHT, LAMB = 3, 2, 1e-3, 0.25, 2.8


def case_name(kind, b, F, C, n):
    return f"{kind} batch_sz={b} F={F} C={C} rows={n}"


def _optimizer(kind, params):
    import torch
    if kind == "SGD":
        return torch.optim.SGD(params, lr=LR, momentum=0.9, weight_decay=0.01)
    if kind == "Adam":
        return torch.optim.Adam(params, lr=LR, weight_decay=0.01)
    return torch.optim.RMSprop(params, lr=LR, momentum=0.9, weight_decay=0.01)


def run_case(kind, b, F, C, n, dev):
    """Two eager epochs -> {tensor name: sha256 of its bytes afterwards}."""
    import numpy as np
    import torch
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    from idelucs_amd.utils import FeatureStore
    rs = np.random.RandomState([KINDS.index(kind), b, F, C, n])
    fh = rs.random_sample((MIMICS + 1, n, F)).astype(np.float32)
    sh = np.maximum(fh[0].astype(np.float64).std(0), 1e-3)
    feats, mean, scale = (torch.from_numpy(v).to(dev) for v in (fh, fh[0].astype(np.float64).mean(0), sh))
    store = FeatureStore(None, None, feats, mean, scale, 4, False)
    net = NetLinear(F, C)
    with torch.no_grad():
        for p in net.parameters():            # (the network from the numpy seed too: torch's initialisers are not part of the case)
            p.copy_(torch.from_numpy((rs.standard_normal(tuple(p.shape)) * (0.05 if p.dim() == 2 else 0.01)).astype(np.float32)))
    net = net.to(dev)
    tr = FusedLinearOptTrainer(net, _optimizer(kind, net.parameters()), WEIGHT, LAMB, seed=5)
    tr.begin_voter(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + CASES.index((kind, b, F, C, n)))
    for _ in range(EPOCHS):
        tr.sync_hyper()
        tr.run_epoch(store, b, use_graph=False, generator=gen)
    torch.cuda.synchronize()
    named = ([(f"param{i}", t) for i, t in enumerate(tr.params)] + [(f"state1_{i}", t) for i, t in enumerate(tr.state1)]
             + [(f"state2_{i}", t) for i, t in enumerate(tr.state2)]
             + [("grad2", tr.grads[2]), ("out", tr.out), ("ctl", tr.ctl), ("steps", tr.steps), ("x", tr.buffers(2 * b).x)])
    return {k: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest() for k, t in named}


def case_line(case, dev):
    return json.dumps({"case": case_name(*case), "sha256": run_case(*case, dev)}, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    dev = torch.device("cuda")
    lines = [case_line(c, dev) for c in CASES]
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
