#!/usr/bin/env python3
"""Generate tests/golden/small_optimizers.npz + small_optimizers.json from the REAL reference (build container only; same scratch build
as make_golden.py).  Pins model_size='small' (reference models.py:59-66: myNet, k = 2: 10 -> 400 -> 128 -> 64 / 5) trained with what
models.py:89-92 configures besides RMSprop:

  * SGD(lr, weight_decay=0.01, momentum=0.9) and Adam(lr): three optimizer steps of IID_model's OWN optimizer object on a fixed batch of 9
    pairs, dropout off, from the same seeded weights -- the initial weights, the loss of every step, the biases after every step, every
    tensor after the last (of W2 [128, 400] every 8th row, as small_k5.npz thins its big gradients: keeps the file small);
  * a float64 twin of the same three steps (the same module objects in double; the reference's info_nce_loss keeps its own cast to
    float32): per optimizer and tensor, the share of entries where the reference's float32 result lies outside rtol 1e-4 / atol 1e-6 of
    the twin -- how far float32 arithmetic alone moves these steps.  The tests hold this library's steps to those tolerances with no
    entry outside for SGD and 2e-3 of a tensor's entries for Adam (tests/test_gpu_optimizers.py::_close_but_for_flips: Adam's first
    steps are sign-like, lr g / (|g| + eps)); a weight seed is kept only if the reference's own share is 0 for SGD and at most 1e-3,
    half that allowance, for Adam.

Usage:  python tests/golden/make_golden_small_optimizers.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import build_reference   # noqa: E402

FIN, C, B, K = 10, 5, 9, 2
STEPS = 3
FIRST_SEED = 41
CAP = {"SGD": 0.0, "Adam": 1e-3}
THIN = 8


def model_args(opt):
    return {'sequence_file': None, 'GT_file': None, 'n_clusters': C, 'k': K, 'model_size': 'small', 'n_mimics': 3, 'batch_sz': B,
            'optimizer': opt, 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None}


def thin(name, v):
    return v[::THIN].copy() if name == "layers.3.weight" else v.copy()


def main():
    build_reference()
    import torch
    import torch.nn as nn
    from idelucs import models as M
    from idelucs.LossFunctions import IID_loss, info_nce_loss
    torch.manual_seed(2024)
    x1 = torch.randn(B, FIN)
    x2 = x1 + 0.1 * torch.randn(B, FIN)

    def run(opt, seed, double):
        """Three steps of the reference's IID_model -> (initial weights, losses, parameters after every step)."""
        model = M.IID_model(model_args(opt))
        assert model.n_features == FIN
        for mod in model.net.modules():
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
        torch.manual_seed(seed)
        model.net.apply(M.weights_init)
        init = {n_: p.numpy().copy() for n_, p in model.net.state_dict().items()}
        a, b = x1, x2
        if double:              # (the optimizer holds the parameter objects: .double() converts them in place)
            model.net.double()
            a, b = x1.double(), x2.double()
        model.net.eval()
        losses, params = [], []
        for _ in range(STEPS):
            model.optimizer.zero_grad()
            z1, h1 = model.net(a.view(-1, 1, FIN)); z2, h2 = model.net(b.view(-1, 1, FIN))
            loss = (1 - model.weight) * info_nce_loss(h1, h2, 0.85) + model.weight * IID_loss(z1, z2, lamb=model.l)
            loss.backward()
            model.optimizer.step()
            losses.append(float(loss.item()))
            params.append({n_: p.detach().numpy().copy() for n_, p in model.net.named_parameters()})
        defaults = {k: (v if not isinstance(v, tuple) else list(v)) for k, v in model.optimizer.defaults.items()
                    if isinstance(v, (int, float, bool, tuple))}
        return init, losses, params, defaults

    seed = FIRST_SEED
    while True:
        runs, shares = {}, {}
        for opt in ("SGD", "Adam"):
            runs[opt] = run(opt, seed, double=False)
            twin = run(opt, seed, double=True)
            shares[opt] = [{n_: float((~np.isclose(runs[opt][2][it][n_], twin[2][it][n_], rtol=1e-4, atol=1e-6)).mean())
                            for n_ in runs[opt][2][it]} for it in range(STEPS)]
            runs[opt] += (twin[1],)
        worst = {opt: max(max(o.values()) for o in shares[opt]) for opt in shares}
        if all(worst[opt] <= CAP[opt] for opt in worst):
            break
        print(f"weight seed {seed} leaves {worst} of a tensor outside its float64 twin: next seed")
        seed += 1

    g = {"x1": x1.numpy().copy(), "x2": x2.numpy().copy()}
    meta = {"B": B, "F": FIN, "C": C, "k": K, "steps": STEPS, "weight_seed": seed, "cap": CAP, "rtol": 1e-4, "atol": 1e-6,
            "thinned": {"layers.3.weight": THIN}}
    for n_, v in runs["SGD"][0].items():
        assert np.array_equal(v, runs["Adam"][0][n_])
        g[f"w.{n_}"] = v
    for opt in ("SGD", "Adam"):
        init, losses, params, defaults, losses64 = runs[opt]
        for it in range(STEPS):
            g[f"{opt}.step{it}.loss"] = np.float32(losses[it])
            for n_, v in params[it].items():                    # (biases after every step, everything after the last)
                if it == STEPS - 1 or v.ndim == 1:
                    g[f"{opt}.step{it}.p.{n_}"] = thin(n_, v)
        meta[f"{opt}.defaults"] = defaults
        meta[f"{opt}.share_outside_float64_twin"] = shares[opt]
        meta[f"{opt}.loss_float64"] = losses64
    np.savez_compressed(os.path.join(HERE, "small_optimizers.npz"), **g)
    json.dump(meta, open(os.path.join(HERE, "small_optimizers.json"), "w"), indent=1)
    print("small_optimizers.npz:", os.path.getsize(os.path.join(HERE, "small_optimizers.npz")), "bytes; seed", seed, "worst shares", worst)
    for opt in ("SGD", "Adam"):
        print(opt, "losses", runs[opt][1], "float64", runs[opt][4])


if __name__ == "__main__":
    main()
