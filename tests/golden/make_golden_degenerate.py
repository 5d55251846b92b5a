#!/usr/bin/env python3
"""Generate tests/golden/iic_degenerate.npz from the REAL reference (build container only; make_golden.py names where it lies).  Pins reference
idelucs/LossFunctions.py:20-46 where it REPLACES cells and marginals of the joint by EPS (the in-place assignments at :36-38): the four input regimes
of tests/test_gpu_loss_regimes.py (dead, disjoint, onehot, collapsed) at (B, C) = (16, 5) and (64, 20) --

    <regime>.B<B>.C<C>.logits   fp32 [2B, C]; rows b and b + B are a pair
    <regime>.B<B>.C<C>.loss     float64: the reference's IID_loss(softmax(logits[:B]), softmax(logits[B:]), lamb=2.8), softmax in float64
    <regime>.B<B>.C<C>.g1 / g2  float64 [B, C]: its gradients with respect to the two logit tensors

Only the reference's LossFunctions.py is imported (at generation time; nothing is built).  The archive is written with fixed time stamps, so a second run
reproduces the file byte for byte.

Usage:  python tests/golden/make_golden_degenerate.py
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF                                    # noqa: E402
from test_gpu_loss_regimes import REGIMES, regime_logits       # noqa: E402

SHAPES = ((16, 5), (64, 20))
LAMB = 2.8


def save_npz(path, arrays):
    """np.savez_compressed with every member's time stamp fixed (numpy stamps them with the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    import torch
    spec = importlib.util.spec_from_file_location("reference_LossFunctions", os.path.join(REF, "idelucs", "LossFunctions.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = {}
    for B, C in SHAPES:
        for name in REGIMES:
            a = regime_logits(name, B, C)
            a1 = torch.from_numpy(a[:B]).double().requires_grad_(True)
            a2 = torch.from_numpy(a[B:]).double().requires_grad_(True)
            loss = ref.IID_loss(torch.softmax(a1, dim=1), torch.softmax(a2, dim=1), lamb=LAMB)
            loss.backward()
            tag = f"{name}.B{B}.C{C}"
            g[tag + ".logits"] = a
            g[tag + ".loss"] = np.float64(loss.item())
            g[tag + ".g1"] = a1.grad.numpy().copy()
            g[tag + ".g2"] = a2.grad.numpy().copy()
            print(f"{tag}: loss {loss.item()!r}, max |gradient| {max(a1.grad.abs().max().item(), a2.grad.abs().max().item()):.3e}")
    out = os.path.join(HERE, "iic_degenerate.npz")
    save_npz(out, g)
    print("iic_degenerate.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
