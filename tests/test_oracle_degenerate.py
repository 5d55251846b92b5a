"""Pins idelucs_amd.LossFunctions.IID_loss (torch.where) to the reference's in-place assignment (idelucs/LossFunctions.py:36-38) in the only regime
where the two could differ: joints with cells and marginals below EPS (tests/golden/make_golden_degenerate.py; the regimes of
tests/test_gpu_loss_regimes.py, whose float64 references go through this function or restate it on the joint).  CPU only, float64."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

REGIMES = ("dead", "disjoint", "onehot", "collapsed")


@pytest.mark.parametrize("B,C", [(16, 5), (64, 20)])
@pytest.mark.parametrize("name", REGIMES)
def test_iid_loss_equals_the_reference_where_cells_are_replaced(name, B, C):
    """The value to 1e-12 relative (collapsed, whose loss is ~ 1e-12: 1e-15 absolute), the gradients with respect to both logit tensors to rtol 1e-9,
    atol 1e-15; and the fixture is what it claims to be: cells are replaced in every regime, marginals in all but "disjoint", where replaced
    cells lie between two marginals that are not."""
    import sys
    import torch
    from idelucs_amd.LossFunctions import IID_loss, compute_joint
    g = np.load(os.path.join(GOLDEN, "iic_degenerate.npz"))
    tag = f"{name}.B{B}.C{C}"
    a = g[tag + ".logits"]
    assert a.dtype == np.float32 and a.shape == (2 * B, C)
    a1 = torch.from_numpy(a[:B]).double().requires_grad_(True)
    a2 = torch.from_numpy(a[B:]).double().requires_grad_(True)
    z1, z2 = torch.softmax(a1, dim=1), torch.softmax(a2, dim=1)
    with torch.no_grad():
        P = compute_joint(z1, z2)
        cell, marg = P < sys.float_info.epsilon, P.sum(1) < sys.float_info.epsilon
        assert bool(cell.any())
        if name == "disjoint":
            assert bool((cell & ~marg[:, None] & ~marg[None, :]).any())
        else:
            assert bool(marg.any())
    loss = IID_loss(z1, z2, lamb=2.8)
    loss.backward()
    want = float(g[tag + ".loss"])
    assert abs(loss.item() - want) <= (1e-15 if name == "collapsed" else 1e-12 * abs(want)), (loss.item(), want)
    np.testing.assert_allclose(a1.grad.numpy(), g[tag + ".g1"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(a2.grad.numpy(), g[tag + ".g2"], rtol=1e-9, atol=1e-15)
