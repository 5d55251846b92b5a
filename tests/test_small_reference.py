"""tests/small_ref.py against torch autograd, on the host: the float64 stages the GPU tests (test_gpu_small_stages.py) hold the small
model's step kernels to, composed around a float64 InfoNCE / IIC written with autograd, give the gradients of the reference step
(test_gpu_small_step._autograd_step: myNet in float64 under loss.backward()) to 1e-12, dropout off and on; the RMSprop restatement is
torch.optim.RMSprop's, both forms; and the two bars do what their derivations say on cases done by hand."""
import sys

import numpy as np
import pytest

import small_ref as R

TEMPERATURE, WEIGHT, LAMB = 0.85, 0.25, 2.8          # what _autograd_step is written for


def _net(F, C, seed):
    import torch
    from idelucs_amd.PytorchUtils import myNet
    from idelucs_amd.models import weights_init
    torch.manual_seed(seed)
    net = myNet(F, C)
    net.apply(weights_init)
    with torch.no_grad():                                # (weights_init leaves the biases at a constant: make every term matter)
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape))
    return net


def _params(net):
    l1, l2, li, lc = net.layers[0], net.layers[3], net.instance, net.classifier[1]
    return [l1.weight, l1.bias, l2.weight, l2.bias, li.weight, li.bias, lc.weight, lc.bias]


def losses_with_autograd(f, z):
    """The two losses of models.py:129 on the stage outputs f [m, 64] (normalised latent) and z [m, C], float64, differentiated by
    autograd down to what idl_small_mid_bwd takes: -> (loss, G [m, 64], dP0 [C, C], nce_coef) with
    d loss / d f = nce_coef (G - 2 f_partner) and d loss / d z = z_partner dP0 (dP0 = d loss / d (z1^T z2), symmetric)."""
    import torch
    f = torch.from_numpy(f).requires_grad_(True)
    z = torch.from_numpy(z).requires_grad_(True)
    m = f.shape[0]
    b = m // 2
    s = (f @ f.t()) / TEMPERATURE
    r = torch.arange(m)
    pos = s[r, (r + b) % m]
    s = s.masked_fill(r.unsqueeze(0) == r.unsqueeze(1), float("-inf"))
    nce = (torch.logsumexp(s, dim=1) - pos).mean()
    J = z[:b].t() @ z[b:]
    J.retain_grad()
    P = (J + J.t()) / 2.0
    P = P / P.sum()
    p_i, p_j = P.sum(dim=1, keepdim=True), P.sum(dim=0, keepdim=True)
    eps = torch.full((), sys.float_info.epsilon, dtype=torch.float64)
    P, p_j, p_i = torch.where(P < eps, eps, P), torch.where(p_j < eps, eps, p_j), torch.where(p_i < eps, eps, p_i)
    iic = (-P * (torch.log(P) - LAMB * torch.log(p_j) - LAMB * torch.log(p_i))).sum()
    loss = (1.0 - WEIGHT) * nce + WEIGHT * iic
    loss.backward()
    nce_coef = (1.0 - WEIGHT) / (m * TEMPERATURE)
    G = f.grad.numpy() / nce_coef + 2.0 * f.detach().numpy()[R.partner(m)]
    return float(loss.detach()), G, J.grad.numpy(), nce_coef


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("C", [5, 49])
@pytest.mark.parametrize("m", [2, 18, 34])
def test_composed_stages_reproduce_autograd(m, C, dropout):
    import torch
    import test_gpu_small_step as sml
    F = 23
    net = _net(F, C, seed=m + C)
    g = torch.Generator().manual_seed(7 * m + C)
    x = torch.randn((m, F), generator=g)
    masks = (torch.rand((m, 400), generator=g) < 0.5, torch.rand((m, 128), generator=g) < 0.5) if dropout else None
    loss_ref, sml_grads = sml._autograd_step(net, x, masks=masks, float64_grads=True)
    sml_grads = [t.numpy() for t in sml_grads]
    assert all(t.dtype == np.float64 for t in sml_grads)
    W1, b1, W2, b2, Wi, bi, Wc, bc = _params(net)
    a1, a2, d2, f, inv, z = R.mid_fwd(R.l1_fwd(x, W1), b1, W2, b2, Wi, bi, Wc, bc, masks)
    loss, G, dP0, nce_coef = losses_with_autograd(f, z)
    assert abs(loss - loss_ref) <= 1e-12 * abs(loss_ref)
    variants = [dict(G_parts=G, dP0=dP0, dzs=None),
                dict(G_parts=np.stack([0.25 * G, 0.5 * G, 0.25 * G]), dP0=None, dzs=z @ dP0)]
    for v in variants:
        dlogits, dh, da2, dr1 = R.mid_bwd(z, f, inv, v["G_parts"], v["dP0"], a1, a2, W2, Wi, Wc, nce_coef,
                                          mask2=masks[1] if dropout else None, train=dropout, dzs=v["dzs"])
        got = R.wgrads(x, dr1, a1, da2, a2, dh, d2, dlogits)
        for name, a, want in zip(sml.NAMES, got, sml_grads):
            scale = np.abs(want).max()
            err = np.abs(a - want).max()
            print(f"{name}: {err:.2e} against a largest entry of {scale:.2e}")
            assert err <= 1e-12 * scale + 1e-300, name
    if m == 2:          # one pair: the only other row is the positive, InfoNCE and its gradient vanish
        assert np.abs(sml_grads[4]).max() == 0.0 and np.abs(got[4]).max() == 0.0


@pytest.mark.parametrize("momentum", [None, 0.9])
def test_rmsprop_restatement_is_torchs(momentum):
    import torch
    g = torch.Generator().manual_seed(3)
    p = torch.randn((7, 5), generator=g, dtype=torch.float64)
    shadow = p.clone().requires_grad_(True)
    opt = torch.optim.RMSprop([shadow], lr=1e-3, weight_decay=0.01, momentum=momentum or 0.0)
    hyper = [1e-3, 0.99, 1e-8, 0.01, 1.0 - 0.99] + ([momentum] if momentum else [])
    pn, v = p.numpy().copy(), np.zeros((7, 5))
    buf = np.zeros((7, 5)) if momentum else None
    for _ in range(3):
        gr = torch.randn((7, 5), generator=g, dtype=torch.float64)
        shadow.grad = gr.clone()
        opt.step()
        out = R.rmsprop(pn, v, gr, hyper, buf)
        pn, v = out[0], out[1]
        if momentum:
            buf = out[2]
            np.testing.assert_allclose(buf, opt.state[shadow]["momentum_buffer"].numpy(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(pn, shadow.detach().numpy(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(v, opt.state[shadow]["square_avg"].numpy(), rtol=1e-13, atol=0)


def test_product_bound_on_a_case_done_by_hand():
    """[1, -2] . [3, 4]: sum |a||b| = 11, K = 2: (2 + 16) 2^-23 11 + 2^-126."""
    b = R.product_bound(np.array([[1.0, -2.0]]), np.array([[3.0], [4.0]]))
    assert b.shape == (1, 1) and b[0, 0] == 18 * 2.0 ** -23 * 11 + 2.0 ** -126
    assert R.product_bound(np.zeros((1, 3)), np.ones((3, 1)))[0, 0] == 2.0 ** -126
    assert R.product_bound(np.ones((1, 2)), np.ones((2, 1)), K=100)[0, 0] == 116 * 2.0 ** -23 * 2 + 2.0 ** -126


@pytest.mark.parametrize("momentum", [None, 0.9])
def test_rmsprop_bound_holds_a_float32_update_and_not_a_wrong_one(momentum):
    """The bar holds numpy's own float32 evaluation of the update (one rounding an operation), and is missed by an update whose
    running average took alpha = 0.98, whose rate is 1 % off, or whose weight decay was left out."""
    rng = np.random.default_rng(5)
    f32 = np.float32
    hyper = np.array([1e-3, 0.99, 1e-8, 0.01, 1.0 - 0.99] + ([momentum] if momentum else []), dtype=f32)
    p, g = rng.standard_normal(4000).astype(f32), (rng.standard_normal(4000) * 10.0 ** rng.uniform(-9, 1, 4000)).astype(f32)
    v = ((0.5 + rng.random(4000)) * (np.abs(g) + 0.01 * np.abs(p)).astype(np.float64) ** 2).astype(f32)
    v[::7] = 0
    g[::11] = 0
    buf = rng.standard_normal(4000).astype(f32) if momentum else None

    def step32(h, wd=True):
        gi = g + h[3] * p if wd else g
        v1 = v * h[1] + h[4] * gi * gi
        r = gi / (np.sqrt(v1) + h[2])
        if buf is None:
            return p - h[0] * r, v1
        b1 = buf * h[5] + r
        return p - h[0] * b1, v1, b1

    want, bars = R.rmsprop(p, v, g, hyper, buf), R.rmsprop_bound(p, v, g, hyper, buf)
    for got, w, bar in zip(step32(hyper), want, bars):
        assert got.dtype == f32
        ratio = np.abs(got.astype(np.float64) - w) / bar
        print("float32 evaluation: worst error / bar", ratio.max())
        assert ratio.max() <= 0.5                # (the bar is twice the first-order bound)
    wrong = hyper.copy()
    wrong[1] = 0.98
    assert (np.abs(step32(wrong)[1].astype(np.float64) - want[1]) > bars[1]).mean() > 0.5
    wrong = hyper.copy()
    wrong[0] *= 1.01
    assert (np.abs(step32(wrong)[0].astype(np.float64) - want[0]) > bars[0]).mean() > 0.5
    assert (np.abs(step32(hyper, wd=False)[0].astype(np.float64) - want[0]) > bars[0]).mean() > 0.5
