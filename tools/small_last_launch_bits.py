#!/usr/bin/env python3
"""Bit identity of the small step's last launch across two builds of the library: one launch of each of its four forms
(idl_small_wgrad_rms, idl_small_wgrad_rms_momentum, idl_small_wgrad_opt with SGD and with Adam) per shape, once without and once with
the riding assembly of the next batch, on operands built on the CPU from a fixed numpy seed, gradients kept.  Prints one JSON line per
case with a sha256 of every tensor the launch writes: the eight parameters, both state sets, the eight gradients, out, ctl, the step
words and the next batch.  (The launch sums in a fixed order and has no atomics, so a case's line depends on the kernels' arithmetic
alone: two builds whose lines agree compute the same bits.)

tests/small_last_launch_parent.jsonl is this tool's output on the library as it was before the four kernels were put on one tile body
(IDELUCS_LIB_PATH=<that build> python tools/small_last_launch_bits.py --out tests/small_last_launch_parent.jsonl);
tests/test_gpu_small_last_launch_bits.py replays the cases on the current build and compares line for line.  (That recording was made when the
entries took the next batch and the optimizer's state as loose arguments; the calls below are the struct forms of the same launches.)

Usage:  python tools/small_last_launch_bits.py [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H1, H2, LAT = 400, 128, 64
FORMS = ("rms", "momentum", "SGD", "Adam")
SHAPES = [(2, 1, 1),              # waves with an empty K share
          (18, 63, 31),           # K tail; F narrower than a column tile
          (34, 136, 200),         # partial third column tile; partial row tiles in C
          (66, 2080, 256),        # the product's F; C = MAX_C
          (1022, 63, 5)]          # many U = 8 trips with a tail
CASES = [(form, m, F, C, rider) for form in FORMS for (m, F, C) in SHAPES for rider in (0, 1)]
STORE_ROWS, VIEWS, AT, STEP, STEPS_TAKEN = 64, 3, 17, 5, 3
HYPER_RMS = [1e-3, 0.99, 1e-8, 0.01, 1.0 - 0.99, 0.9]           # lr, alpha, eps, weight decay, 1 - alpha, momentum
HYPER_OPT = {"SGD": [1e-3, 0.9, 0.0, 0.0, 0.01], "Adam": [1e-3, 0.9, 0.999, 1e-8, 0.01]}
SENTINEL = -777.0


def case_name(form, m, F, C, rider):
    return f"{form} m={m} F={F} C={C} rider={rider}"


def run_case(form, m, F, C, rider, dev):
    """One launch -> {tensor name: sha256 of its bytes after the launch}."""
    import numpy as np
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.fused import _p, _stream
    rs = np.random.RandomState([FORMS.index(form), m, F, C, rider])
    f32 = lambda shape, scale=1.0: torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).to(dev)
    shapes = [(H1, F), (H1,), (H2, H1), (H2,), (LAT, H2), (LAT,), (C, H2), (C,)]
    params = [f32(s, 0.1) for s in shapes]
    # state 1: RMSprop's square_avg (>= 0), SGD's momentum_buffer, Adam's exp_avg; state 2: RMSprop's momentum_buffer, Adam's exp_avg_sq (>= 0)
    state1 = [f32(s, 0.1).abs_() if form in ("rms", "momentum") else f32(s, 0.1) for s in shapes]
    state2 = [f32(s, 0.1).abs_() if form == "Adam" else f32(s, 0.1) for s in shapes]
    grads = [torch.full(s, SENTINEL, dtype=torch.float32, device=dev) for s in shapes]
    widths = (("x", F), ("dr1", H1), ("a1", H1), ("da2", H2), ("a2", H2), ("dh", LAT), ("d2", H2), ("dlogits", C))
    ops = [f32((m, w)) for _, w in widths]
    loss_rows = torch.from_numpy((rs.random_sample(m) * 6).astype(np.float32)).to(dev)
    out = torch.tensor([9.0, 3.5, 9.0, 0.75], dtype=torch.float32, device=dev)
    ctl = torch.tensor([STEP, AT], dtype=torch.int64, device=dev)
    steps = torch.tensor([STEPS_TAKEN, -1], dtype=torch.int64, device=dev)
    y_next = torch.full((m, F), SENTINEL, dtype=torch.float32, device=dev)
    gather = None
    if rider:
        n, n_pairs = STORE_ROWS, STORE_ROWS * VIEWS
        fh = rs.random_sample(((VIEWS + 1) * n, F)).astype(np.float32)
        sh = np.maximum(fh[:n].astype(np.float64).std(0), 1e-3)
        feats, mean, scale, inv_scale = (torch.from_numpy(v).to(dev) for v in (fh, fh[:n].astype(np.float64).mean(0), sh, 1.0 / sh))
        perm = torch.from_numpy(rs.permutation(n_pairs).astype(np.int64)).to(dev)
        gather = _lib.idl_next_batch_t(feats=_p(feats), n=n, f=F, view_stride=n * F, pair_idx=_p(perm), base=_p(ctl[1:]), base_add=0, n_pairs=n_pairs,
                                       batch=m // 2, mean=_p(mean), scale=_p(scale), inv_scale=_p(inv_scale), y=_p(y_next), part=0, part_end=1, parts=1)
    arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])
    tail = (_p(ctl), *[_p(o) for o in ops], m, F, C, _p(loss_rows), 0.75, 0.25, _p(out), gather, _stream())
    L = _lib.lib
    if form == "rms":
        hyper = torch.tensor(HYPER_RMS[:5], dtype=torch.float32, device=dev)
        _lib.check(L.idl_small_wgrad_rms(arr(params), arr(grads), arr(state1), _p(hyper), *tail))
    elif form == "momentum":
        hyper = torch.tensor(HYPER_RMS, dtype=torch.float32, device=dev)
        _lib.check(L.idl_small_wgrad_rms_momentum(arr(params), arr(grads), arr(state1), arr(state2), _p(hyper), *tail))
    else:
        hyper = torch.tensor(HYPER_OPT[form], dtype=torch.float64, device=dev)
        kind = 1 if form == "SGD" else 2
        opt = _lib.idl_opt_state_t(kind, arr(state1), arr(state2), _p(hyper), _p(steps[0:]), _p(steps[1:]))
        _lib.check(L.idl_small_wgrad_opt(opt, arr(params), arr(grads), *tail))
    torch.cuda.synchronize()
    named = ([(f"param{i}", t) for i, t in enumerate(params)] + [(f"state1_{i}", t) for i, t in enumerate(state1)]
             + [(f"state2_{i}", t) for i, t in enumerate(state2)] + [(f"grad{i}", t) for i, t in enumerate(grads)]
             + [("out", out), ("ctl", ctl), ("steps", steps), ("next", y_next)])
    return {k: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for k, t in named}


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
