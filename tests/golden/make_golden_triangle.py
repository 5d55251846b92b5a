#!/usr/bin/env python3
"""Generate tests/golden/triangle.npz + triangle.json from the REAL reference (build container only; same scratch build as
make_golden.py).  Pins what reference idelucs/models.py:87-88 becomes under the Triangle scheduler of models.py:99: CyclicLR's
cycle_momentum (on by default) writes a momentum into the RMSprop group -- 0.9 at construction, then 0.88, 0.86 ... 0.80, 0.82 ... --
so torch trains RMSprop WITH a momentum buffer.

  * model_size='linear' (NetLinear 16 -> 512 -> 64 -> 5) and model_size='small' (myNet, k = 2: 10 -> 400 -> 128 -> 64 / 7), B = 9,
    dropout off, fresh weights from a fixed seed, three batches drawn as the optimizers fixture draws them;
  * two epochs through the reference's own contrastive_training_epoch: the (lr, momentum) of the group at construction and after each
    epoch's scheduler step, the epoch losses, the biases after each epoch, every tensor after epoch 2;
  * the (lr, momentum) trace of 30 scheduler steps;
  * a float64 twin of each run (the same module objects in double): per tensor, the share of entries of the float32 run outside
    rtol = 1e-3, atol = 1e-6 of the twin -- how far float32 arithmetic alone moves these sign-like steps.  The tests allow 5e-3 of a
    tensor's entries outside; a weight seed is kept only if the reference's own figure is at most 2e-3.

Usage:  python tests/golden/make_golden_triangle.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import build_reference   # noqa: E402

B = 9
SHAPES = {"linear": dict(k=2, C=5, F=16), "small": dict(k=2, C=7, F=10)}
TWIN_CAP = 2e-3
FIRST_SEED = 31


def model_args(size):
    s = SHAPES[size]
    return {'sequence_file': None, 'GT_file': None, 'n_clusters': s["C"], 'k': s["k"], 'model_size': size, 'n_mimics': 3, 'batch_sz': B,
            'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': 'Triangle'}


def main():
    build_reference()
    import torch
    import torch.nn as nn
    from idelucs import models as M
    g, meta = {}, {"B": B, "shapes": SHAPES, "twin_cap": TWIN_CAP}

    def hyper(model):
        grp = model.optimizer.param_groups[0]
        return [float(grp['lr']), float(grp['momentum'])]

    def run(size, seed, batches, double):
        """Two epochs of the reference's IID_model -> (initial weights, hyper trace, epoch losses, parameters after each epoch)."""
        model = M.IID_model(model_args(size))
        assert model.n_features == SHAPES[size]["F"]
        for mod in model.net.modules():
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
        torch.manual_seed(seed)
        model.net.apply(M.weights_init)
        init = {n_: p.numpy().copy() for n_, p in model.net.state_dict().items()}
        saved = M.dtype
        if double:              # (the optimizer holds the parameter objects: .double() converts them in place)
            model.net.double()
            M.dtype = torch.DoubleTensor
        try:
            model.dataloader = [{'true': a, 'modified': b} for a, b in batches]
            trace, losses, params = [hyper(model)], [], []
            for _ in range(2):
                losses.append(model.contrastive_training_epoch())
                trace.append(hyper(model))
                params.append({n_: p.detach().numpy().copy() for n_, p in model.net.named_parameters()})
        finally:
            M.dtype = saved
        state = model.optimizer.state[next(iter(model.net.parameters()))]
        assert "momentum_buffer" in state and "square_avg" in state, sorted(state)
        return init, trace, losses, params

    for size, s in SHAPES.items():
        torch.manual_seed(2024)
        batches = []
        for i in range(3):
            x1 = torch.randn(B, s["F"]); x2 = x1 + 0.1 * torch.randn(B, s["F"])
            batches.append((x1, x2))
            g[f"{size}.x1.{i}"] = x1.numpy().copy(); g[f"{size}.x2.{i}"] = x2.numpy().copy()
        seed = FIRST_SEED
        while True:
            init, trace, losses, params = run(size, seed, batches, double=False)
            _, trace64, losses64, params64 = run(size, seed, batches, double=True)
            outside = [{n_: float((~np.isclose(params[e][n_], params64[e][n_], rtol=1e-3, atol=1e-6)).mean()) for n_ in params[e]}
                       for e in range(2)]
            worst = max(max(o.values()) for o in outside)
            if worst <= TWIN_CAP:
                break
            print(f"{size}: weight seed {seed} leaves {worst:.2e} of a tensor outside its float64 twin: next seed")
            seed += 1
        assert trace == trace64
        for n_, v in init.items():
            g[f"{size}.w.{n_}"] = v
        g[f"{size}.hyper"] = np.array(trace, np.float64)                   # [3, 2]: at construction, after epoch 1, after epoch 2
        g[f"{size}.epoch_loss"] = np.array(losses, np.float32)
        for e in range(2):
            for n_, v in params[e].items():                                # (biases after every epoch, everything after the last)
                if e == 1 or v.ndim == 1:
                    g[f"{size}.epoch{e + 1}.p.{n_}"] = v
        meta[f"{size}.weight_seed"] = seed
        meta[f"{size}.share_outside_float64_twin"] = outside
        meta[f"{size}.epoch_loss_float64"] = [float(v) for v in losses64]

    # ---- the (lr, momentum) of 30 scheduler steps, driven as contrastive_training_epoch drives them (models.py:137-140)
    model = M.IID_model(model_args("linear"))
    trace = []
    for e in range(30):
        model.optimizer.zero_grad()
        for p in model.net.parameters():
            p.grad = torch.zeros_like(p)
        model.optimizer.step()
        model.scheduler.step()
        trace.append(hyper(model))
    meta["at_construction"] = hyper(M.IID_model(model_args("linear")))
    meta["lr_trace"] = [t[0] for t in trace]
    meta["momentum_trace"] = [t[1] for t in trace]
    np.savez_compressed(os.path.join(HERE, "triangle.npz"), **g)
    json.dump(meta, open(os.path.join(HERE, "triangle.json"), "w"), indent=1)
    print("triangle.npz:", os.path.getsize(os.path.join(HERE, "triangle.npz")), "bytes")
    print({k: v for k, v in meta.items() if "trace" not in k})
    print("momentum:", [round(v, 4) for v in meta["momentum_trace"][:12]])


if __name__ == "__main__":
    main()
