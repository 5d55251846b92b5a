"""GPU tests of the native SGD / Adam step of model_size='small' (idelucs_amd/fused_small.py: FusedSmallOptTrainer + csrc/small_step.hip:
small_wgrad_opt_kernel): the C ABI against torch.optim, the reference's goldens (tests/golden/make_golden_small_optimizers.py ->
small_optimizers.npz / .json), three consecutive steps against float64 autograd (dropout off and on), graph replay against eager launches,
the launch budget, IID_model routing / schedulers / carried state, the quality of a 10-epoch run against the autograd form and the CLI."""
import copy
import ctypes
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN
import test_gpu_small_step as sml          # helpers only: NAMES, the random myNet, the feature store

pytestmark = pytest.mark.gpu

NAMES = sml.NAMES
KIND = {"SGD": 1, "Adam": 2}
LR, LR1, WD = 1e-3, 2.5e-3, 0.01
SECOND, SECOND1 = 0.9, 0.8                  # SGD's momentum / Adam's beta1: at construction, and as a scheduler leaves it after the first step


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda")


def _optimizer(opt, params):
    """The optimizer objects of reference models.py:89-92."""
    import torch
    if opt == "SGD":
        return torch.optim.SGD(params, lr=LR, weight_decay=WD, momentum=SECOND)
    return torch.optim.Adam(params, lr=LR)


def _trainer(net, opt, seed=5):
    from idelucs_amd.fused_small import FusedSmallOptTrainer
    tr = FusedSmallOptTrainer(net, _optimizer(opt, net.parameters()), weight=0.25, lamb=2.8, seed=seed)
    tr.keep_grads = True
    tr.begin_voter(0)
    return tr


def _within(have, want, name, rel=1e-5):
    """have within rel of want's largest magnitude (the bar of tests/test_gpu_linear_opt_step.py)."""
    err, top = (have - want).abs().max().item(), want.abs().max().item()
    print(f"  {name}: max error {err / max(top, 1e-30):.2e} of the tensor's max")
    assert err <= rel * top + 1e-30, (name, err, top)


def _state_names(opt):
    return ("momentum_buffer",) if opt == "SGD" else ("exp_avg", "exp_avg_sq")


def _set_second(group, opt, value):
    if opt == "SGD":
        group['momentum'] = value
    else:
        group['betas'] = (value, group['betas'][1])


def _second(group, opt):
    return group['momentum'] if opt == "SGD" else group['betas'][0]


# ------------------------------------------------------------------------------------------------ 1. the C ABI, called directly
def _abi_operands(dev, m, F, C=7, seed=0):
    import torch
    H1, H2, LAT = 400, 128, 64
    gen = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
    shapes = [(H1, F), (H1,), (H2, H1), (H2,), (LAT, H2), (LAT,), (C, H2), (C,)]
    return rnd, [rnd(*s) for s in shapes]


def _arr(ts):
    return (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("opt,start", [("SGD", 0), ("Adam", 0), ("Adam", 5)])
@pytest.mark.parametrize("m", [18, 64])
@pytest.mark.parametrize("F", [10, 136])
def test_small_wgrad_opt_matches_torch_optim(dev, opt, start, m, F):
    """idl_small_wgrad_opt on random layer inputs and output gradients (C = 7; m = 18: a K tail and waves with an empty share; F = 10:
    narrower than a column tile, F = 136: a third, partial one): the gradients it writes against float64 products, and three consecutive
    updates -- the rate and the momentum / beta1 changed after the first, the two step words swapped from launch to launch -- against
    torch.optim.SGD(momentum, weight_decay=0.01) / torch.optim.Adam fed those gradients: parameters and every state tensor.  Adam from a
    step count of 0 starts from zero biases (t = 1 shows the bias correction in full); from a count of 5, on torch's state after five
    steps on zero gradients (zero moments, step = 5)."""
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.fused import _p, _stream
    C = 7
    rnd, params = _abi_operands(dev, m, F, C, seed=31 * m + F + start)
    if opt == "Adam" and start == 0:
        for b in params[1::2]:
            b.zero_()
    st1, st2, grads = ([torch.zeros_like(p) for p in params] for _ in range(3))
    shadow = [p.clone().requires_grad_(True) for p in params]
    sopt = _optimizer(opt, shadow)
    for _ in range(start):
        for p in shadow:
            p.grad = torch.zeros_like(p)
        sopt.step()
    assert all(torch.equal(a.detach(), b) for a, b in zip(shadow, params))
    grp = sopt.param_groups[0]
    hyper = torch.tensor([LR, SECOND, 0.999 if opt == "Adam" else 0.0, 1e-8 if opt == "Adam" else 0.0, grp['weight_decay']],
                         dtype=torch.float64, device=dev)
    steps = torch.tensor([start, 0], dtype=torch.int64, device=dev)
    ctl = torch.tensor([9, 0], dtype=torch.int64, device=dev)
    pp, gp, s1p, s2p = _arr(params), _arr(grads), _arr(st1), (_arr(st2) if opt == "Adam" else None)
    for it in range(3):
        if it == 1:
            grp['lr'] = LR1
            _set_second(grp, opt, SECOND1)
            hyper[0:1].fill_(LR1)
            hyper[1:2].fill_(SECOND1)
        x, a1, a2, d2 = rnd(m, F), rnd(m, 400), rnd(m, 128), rnd(m, 128)
        dr1, da2, dh, dlogits = rnd(m, 400), rnd(m, 128), rnd(m, 64), rnd(m, C)
        par = it % 2
        _lib.check(_lib.lib.idl_small_wgrad_opt(
            _lib.idl_opt_state_t(KIND[opt], s1p, s2p, _p(hyper), _p(steps[par:]), _p(steps[1 - par:])), pp, gp, _p(ctl),
            _p(x), _p(dr1), _p(a1), _p(da2), _p(a2), _p(dh), _p(d2), _p(dlogits), m, F, C,
            None, 0.0, 0.0, None, None, _stream()))
        torch.cuda.synchronize()
        print(f"{opt} m = {m}, F = {F}, step {start + it + 1}, lr {hyper[0].item()}, momentum / beta1 {hyper[1].item()}:")
        for i, (dy, xin) in enumerate(((dr1, x), (da2, a1), (dh, a2), (dlogits, d2))):
            _within(grads[2 * i].double(), dy.double().t() @ xin.double(), NAMES[2 * i] + " gradient", rel=2e-3)
            _within(grads[2 * i + 1].double(), dy.double().sum(0), NAMES[2 * i + 1] + " gradient", rel=2e-3)
        for p, g_ in zip(shadow, grads):
            p.grad = g_.clone()
        sopt.step()
        for i, n_ in enumerate(NAMES):
            state = sopt.state[shadow[i]]
            _within(params[i], shadow[i].detach(), n_ + " parameter")
            for sname, have in zip(_state_names(opt), (st1[i], st2[i])):
                _within(have, state[sname], f"{n_} {sname}")
        assert ctl.tolist() == [9 + it + 1, 0]
        assert steps[1 - par].item() == start + it + 1
    assert sorted(steps.tolist()) == [start + 2, start + 3]
    if opt == "SGD":
        assert all(float(v.abs().sum()) == 0.0 for v in st2)             # state2 == NULL: nothing of it is touched


def test_small_wgrad_opt_refuses_what_it_cannot_run(dev):
    """Every refusal is an argument check in front of the launch: nothing runs."""
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.fused import _p, _stream
    m, F, C = 18, 10, 7
    rnd, params = _abi_operands(dev, m, F, C)
    st1, st2, grads = ([torch.zeros_like(p) for p in params] for _ in range(3))
    before = [p.clone() for p in params]
    hyper = torch.tensor([LR, SECOND, 0.999, 1e-8, 0.0], dtype=torch.float64, device=dev)
    steps = torch.zeros(2, dtype=torch.int64, device=dev)
    ctl = torch.zeros(2, dtype=torch.int64, device=dev)
    ops = [rnd(m, F), rnd(m, 400), rnd(m, 400), rnd(m, 128), rnd(m, 128), rnd(m, 64), rnd(m, 128), rnd(m, C)]

    def call(kind, s2, step_in, step_out):
        return _lib.lib.idl_small_wgrad_opt(_lib.idl_opt_state_t(kind, _arr(st1), s2, _p(hyper), step_in, step_out), _arr(params), _arr(grads), _p(ctl),
                                            *[_p(t) for t in ops], m, F, C, None, 0.0, 0.0, None, None, _stream())
    assert call(2, None, _p(steps), _p(steps[1:])) != 0                  # Adam without exp_avg_sq
    assert "state2" in _lib.last_error()
    assert call(1, None, _p(steps), _p(steps)) != 0                      # the step count read and written in one word
    assert call(2, _arr(st2), _p(steps), _p(steps)) != 0
    assert call(1, None, _p(ctl), _p(steps)) != 0                        # ... or read from a word the launch writes
    for kind in (0, 3):
        assert call(kind, _arr(st2), _p(steps), _p(steps[1:])) != 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, params)) and ctl.tolist() == [0, 0] and steps.tolist() == [0, 0]
    assert call(1, None, _p(steps), _p(steps[1:])) == 0                  # SGD takes state2 == NULL
    torch.cuda.synchronize()
    assert ctl.tolist() == [1, 0] and steps.tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ 2. the reference's goldens
def _close_but_for_flips(got, want, name, rtol=1e-4, atol=1e-6, frac=2e-3):
    """tests/test_gpu_optimizers.py's rule: everything agrees to rounding but for a share `frac` of sign-like first steps."""
    bad = ~np.isclose(got, want, rtol=rtol, atol=atol)
    print(f"  {name}: {bad.mean():.2e} of the entries outside, max difference {np.abs(got - want).max():.2e}")
    assert bad.mean() <= frac, (name, float(bad.mean()), float(np.abs(got - want).max()))


def _golden_args(opt, **kw):
    a = {'sequence_file': None, 'GT_file': None, 'n_clusters': 5, 'k': 2, 'model_size': 'small', 'n_mimics': 3, 'batch_sz': 9,
         'optimizer': opt, 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 1, 'n_voters': 1}
    a.update(kw)
    return a


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_three_steps_match_the_reference_goldens(dev, opt):
    """small_optimizers.npz: the reference's IID_model(small, k = 2: myNet(10, 5)), m = 18, dropout off, three steps of its own SGD / Adam
    on a fixed batch.  The native step and, with the same bars, the autograd step it replaces: loss 3e-4 relative, tensors rtol 1e-4 /
    atol 1e-6 with no entry outside for SGD and 2e-3 of a tensor's for Adam (the reference's own float32 run against its float64 twin
    leaves none outside at this seed: small_optimizers.json)."""
    import torch
    from idelucs_amd import models
    from idelucs_amd.fused_small import FusedSmallOptTrainer
    g = np.load(os.path.join(GOLDEN, "small_optimizers.npz"))
    x = torch.cat([torch.from_numpy(g["x1"]), torch.from_numpy(g["x2"])]).to(dev)
    frac = 2e-3 if opt == "Adam" else 0.0

    def compare(it, loss, params, form):
        ref = float(g[f"{opt}.step{it}.loss"])
        print(f"{opt} {form} step {it}: loss {loss:.7f} reference {ref:.7f}")
        assert abs(loss - ref) <= 3e-4 * abs(ref), (form, opt, it, loss, ref)
        for n_, p in zip(NAMES, params):
            key = f"{opt}.step{it}.p.{n_}"
            if key in g.files:
                got = p.detach().cpu().numpy()
                if got.shape != g[key].shape:                       # (the fixture keeps every 8th row of W2)
                    got = got[::8]
                _close_but_for_flips(got, g[key], f"{form} {key}", frac=frac)

    def load(model):
        model.net.load_state_dict({n: torch.from_numpy(g[f"w.{n}"]) for n in model.net.state_dict()})

    model = models.IID_model(_golden_args(opt, small_opt_step='native'))
    assert model._use_small and model._small_opt
    load(model)
    tr = FusedSmallOptTrainer(model.net, model.optimizer, model.weight, model.l, seed=0)
    model._small = tr
    model.begin_voter(0)
    load(model)                                                     # (begin_voter draws fresh weights)
    bf = tr.buffers(18)
    for it in range(3):
        bf.x.copy_(x)
        tr.step_on_batch(bf, train=False)
        torch.cuda.synchronize()
        compare(it, tr.out[0].item(), tr.params, "native")
    assert tr.step_count() == 3 and tr.ctl.tolist() == [3, 0]

    model = models.IID_model(_golden_args(opt))
    assert not model._use_small and not model._small_opt
    load(model)
    model.net.eval()
    params = [dict(model.net.named_parameters())[n_] for n_ in NAMES]
    for it in range(3):
        loss = model._step(x)
        compare(it, loss.item(), params, "autograd")


# ------------------------------------------------------------------------------------------------ 3. against float64 autograd
def _same_branch(want, have, pre, bound, name):
    """The units the float64 forward puts above zero (want) and the ones the trainer did (have) are the same set, but for units whose float64
    pre-activation lies within fp32 rounding of zero: |pre| <= 1e-5 x sum |x_k| |w_k| (some 170 fp32 epsilons of the dot product's terms),
    and no more than 1e-4 of all units (tests/test_gpu_linear_opt_step.py's rule; one unit where that is less than one: the smallest shape
    here has 4096 units in layer 2)."""
    mism = want != have
    n = int(mism.sum().item())
    print(f"  {name}: {n} of {mism.numel()} units at a kink" + (f" (|pre| / bound <= {float((pre.abs()[mism] / bound[mism]).max()):.1e})" if n else ""))
    if n:
        assert bool((pre.abs()[mism] <= 1e-5 * bound[mism]).all()), (name, n, float((pre.abs()[mism] / bound[mism]).max()))
        assert n <= max(1, 1e-4 * mism.numel()), (name, n)


def _autograd_step(net, x, kept, masks=None):
    """The reference step (models.py:117-133) on a float64 copy of net, dropout off or the given keep masks x 2 in place of nn.Dropout,
    differentiating the branch the trainer took: kept = (a1 > 0, a2 > 0) of its step on the same parameters (a1 after ReLU and Dropout, a2
    after LeakyReLU).  ReLU and LeakyReLU have no derivative at 0, and a unit whose pre-activation is zero to fp32 rounding falls on either
    side of it in two correct forwards; _same_branch checks that the two forwards differ at such units only.  -> (loss, [8 gradients])."""
    import torch
    import torch.nn.functional as Fn
    from idelucs_amd.LossFunctions import IID_loss
    ref = copy.deepcopy(net).double()
    x = x.double()
    l1, l2, li, lc = ref.layers[0], ref.layers[3], ref.instance, ref.classifier[1]
    ps = [l1.weight, l1.bias, l2.weight, l2.bias, li.weight, li.bias, lc.weight, lc.bias]
    scale = 2.0 if masks is not None else 1.0
    pre1 = Fn.linear(x, l1.weight, l1.bias)
    with torch.no_grad():
        want1 = (pre1 > 0) & masks[0] if masks is not None else pre1 > 0
        _same_branch(want1, kept[0], pre1, Fn.linear(x.abs(), l1.weight.abs(), l1.bias.abs()), "layer 1")
    a1 = pre1 * kept[0].double() * scale
    pre2 = Fn.linear(a1, l2.weight, l2.bias)
    with torch.no_grad():
        _same_branch(pre2 > 0, kept[1], pre2, Fn.linear(a1.abs(), l2.weight.abs(), l2.bias.abs()), "layer 2")
    a2 = pre2 * torch.where(kept[1], 1.0, 0.01).double()
    h = Fn.linear(a2, li.weight, li.bias)
    d2 = a2 * masks[1].double() * 2.0 if masks is not None else a2
    z = torch.softmax(Fn.linear(d2, lc.weight, lc.bias), dim=1)
    b = x.shape[0] // 2
    f = Fn.normalize(h, dim=1)                          # info_nce_loss (LossFunctions.py:65-98) without its cast to float32
    s = (f @ f.t()) / 0.85
    r = torch.arange(2 * b, device=s.device)
    pos = s[r, (r + b) % (2 * b)]
    s = s.masked_fill(r.unsqueeze(0) == r.unsqueeze(1), float("-inf"))
    nce = (torch.logsumexp(s, dim=1) - pos).mean()
    loss = 0.75 * nce + 0.25 * IID_loss(z[:b], z[b:], lamb=2.8)
    loss.backward()
    return float(loss.item()), [p.grad.detach().float().clone() for p in ps]


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("F,m,C", [(10, 32, 5), (136, 64, 20), (2080, 256, 200)])
def test_three_full_batch_steps_match_autograd_and_torch_optim(dev, opt, F, m, C, dropout):
    """Three consecutive full-batch steps on one batch, dropout off and on with the trainer's own masks (voter 3's stream): the loss (rel
    2e-4) and every gradient (2e-3 of its largest entry: the constant bars of tests/test_gpu_small_step.py) against float64 autograd from
    the parameters the step started from, and the parameters against torch's optimizer fed the trainer's gradients (1e-5)."""
    import torch
    net = sml._random_net(F, C, dev, seed=F + m + C)
    x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(F * 7 + m + C))
    tr = _trainer(net, opt)
    if dropout:
        tr.begin_voter(3)
    bf = tr.buffers(m)
    shadow = [p.detach().clone().requires_grad_(True) for p in tr.params]
    sopt = _optimizer(opt, shadow)
    for it in range(3):
        before = copy.deepcopy(net)
        step = int(tr.ctl[0].item())
        assert step == ((3 << 24) if dropout else 0) + it
        masks = tr.dropout_masks(step, m) if dropout else None
        bf.x.copy_(x)
        tr.step_on_batch(bf, train=dropout)
        torch.cuda.synchronize()
        loss_ref, grads_ref = _autograd_step(before, x, (bf.a1 > 0, bf.a2 > 0), masks=masks)
        got = tr.out[0].item()
        print(f"{opt} F={F} m={m} C={C} dropout={dropout} step {it}: loss {got:.7f} autograd {loss_ref:.7f}")
        assert abs(got - loss_ref) <= 2e-4 * abs(loss_ref), (it, got, loss_ref)
        for i, n_ in enumerate(NAMES):
            have, want = tr.gradient(i), grads_ref[i]
            err = (have - want).abs().max().item()
            print(f"  {n_}: max gradient error {err / want.abs().max().item():.2e} of the gradient's max")
            assert err <= 2e-3 * want.abs().max().item() + 1e-12, (it, n_, err, want.abs().max().item())
        for p, i in zip(shadow, range(8)):
            p.grad = tr.gradient(i).clone()
        sopt.step()
        for n_, p, want in zip(NAMES, tr.params, shadow):
            _within(p.detach(), want.detach(), n_ + " parameter")
    assert tr.step_count() == 3


# ------------------------------------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("n,n_full,captures", [(248, 11, 1), (268, 12, 2)])
def test_epochs_replayed_from_the_graph_equal_eager_launches(dev, opt, n, n_full, captures):
    """Three epochs in batches of 64 pairs, the hyperparameters changed between them through the torch group + sync_hyper(): parameters,
    states, step words, losses, out and ctl bit-identical to eager launches.  744 pairs: an odd number of full batches (11: one replay of
    10 and an eager step) and a partial last batch of 40 -- 12 steps an epoch, every epoch starts with the step words in the same roles.
    804 pairs: 12 full batches and a partial one of 36 -- 13 steps, so the second epoch starts with the words in the other roles (a second
    graph) and the third replays the first one's."""
    import torch
    st = sml._Store(n, 3, 136, dev, seed=2)
    assert divmod(st.n_pairs, 64)[0] == n_full and st.n_pairs % 64 != 0
    runs = []
    for use_graph in (True, False):
        net = sml._random_net(136, 20, dev, seed=4)
        tr = _trainer(net, opt, seed=6)
        tr.keep_grads = False
        grp = tr.optimizer.param_groups[0]
        gen = torch.Generator(device=dev).manual_seed(123)
        losses, parities = [], []
        for epoch in range(3):
            grp['lr'] = LR * (1 + epoch)
            _set_second(grp, opt, SECOND - 0.05 * epoch)
            tr.sync_hyper()
            parities.append(tr._tpar)
            total, nb = tr.run_epoch(st, 64, generator=gen, use_graph=use_graph)
            assert nb == n_full + 1
            losses.append(total.clone())
        torch.cuda.synchronize()
        assert parities == ([0, 0, 0] if captures == 1 else [0, 1, 0])
        assert len(tr._graphs) == (captures if use_graph else 0)
        assert tr.hyper64[:2].tolist() == [LR * 3, SECOND - 0.1]
        assert tr.step_count() == 3 * (n_full + 1) and tr.ctl.tolist() == [3 * (n_full + 1), 64 * n_full]
        assert all(bool(torch.isfinite(t)) for t in losses)
        assert all(float(v.abs().sum()) > 0 for v in tr.state_tensors())
        runs.append([p.detach().clone() for p in tr.params] + [v.clone() for v in tr.state_tensors()] + losses
                    + [tr.steps.clone(), tr.out.clone(), tr.ctl.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. launches
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_full_batch_step_launch_budget(dev, opt):
    """A full-batch step at n_clusters <= 48 is 6 launches, none of them a library GEMM, the last one the new kernel (counted as
    tests/test_gpu_small_step.py::test_full_batch_step_launch_budget counts)."""
    import torch
    from torch.profiler import profile, ProfilerActivity
    F, B, C = 136, 128, 20
    st = sml._Store(512, 3, F, dev, seed=1)
    tr = _trainer(sml._random_net(F, C, dev), opt, seed=2)
    tr.keep_grads = False
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    tr.ctl[1:2].zero_()
    bf = tr.buffers(2 * B)
    tr._gather(st, bf, B)
    for i in range(2):                                   # (warm: nothing lazily initialised inside the profile)
        tr.step_on_batch(bf, xi=i % 2, next_from=st)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(4):
            tr.step_on_batch(bf, xi=i % 2, next_from=st)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
             and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    print(f"{opt} C = {C}: {len(names) / 4:.1f} launches a step")
    assert not [n for n in names if "Cijk" in n], names
    assert len(names) == 6 * 4, (len(names), names)
    for k in ("small_l1_fwd_kernel", "small_mid_fwd_kernel", "small_mid_bwd_kernel", "small_wgrad_opt_kernel"):
        assert sum(k in n for n in names) == 4, (k, names)
    assert not [n for n in names if "small_wgrad_rms_kernel" in n or "small_wgrad_momentum_kernel" in n], names
    assert tr.step_count() == 6


# ------------------------------------------------------------------------------------------------ 6. IID_model
def _args(**kw):
    a = {'sequence_file': os.path.join(DATA, "Influenza-A.fas"), 'GT_file': None, 'n_clusters': 5, 'k': 6, 'model_size': 'small',
         'n_mimics': 3, 'batch_sz': 256, 'optimizer': 'Adam', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None,
         'n_epochs': 3, 'n_voters': 1, 'small_opt_step': 'native'}
    a.update(kw)
    return a


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_iid_model_native_small_opt_trains_and_predicts(dev, opt):
    import torch
    from idelucs_amd import models
    from idelucs_amd.fused_small import FusedSmallOptTrainer
    m = models.IID_model(_args(k=4, optimizer=opt))
    assert m._use_small and m._small_opt and not m._use_fused and not m._use_linopt
    assert m.lane()._small_opt                           # the key travels to the lanes of an ensemble
    m.build_dataloader()
    m.begin_voter(0)
    losses = [m.contrastive_training_epoch() for _ in range(3)]
    print(f"{opt}: epoch losses {losses}")
    assert isinstance(m._small, FusedSmallOptTrainer) and m._small.kind == KIND[opt] and m._fused is None and m._linopt is None
    assert all(np.isfinite(losses)), losses
    if opt == "Adam":
        assert losses[2] < losses[0], losses
    assert m._small.step_count() == 3 * 12               # 2847 pairs in batches of 256: 11 full + 1 partial
    y, p, lat = m.predict()
    assert y.shape == (949,) and lat.shape == (949, 64) and np.all(np.isfinite(lat))
    snaps = []                                           # voter v is the same run whenever it trains; two voters differ
    for v in (1, 1, 2):
        m.begin_voter(v)
        for _ in range(2):
            m.contrastive_training_epoch()
        snaps.append([p.detach().clone() for p in m.net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[1]))
    assert not all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[2]))


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_small_without_the_key_stays_on_autograd(dev, opt, monkeypatch):
    from idelucs_amd import models, fused_small

    def refuse(*a, **kw):
        raise AssertionError("a FusedSmallOptTrainer was built")
    monkeypatch.setattr(fused_small.FusedSmallOptTrainer, "__init__", refuse)
    a = _args(k=4, optimizer=opt)
    del a['small_opt_step']
    for args in (a, _args(k=4, optimizer=opt, small_opt_step=None), _args(k=4, optimizer=opt, small_opt_step='autograd')):
        m = models.IID_model(args)
        assert m._use_small is False and m._small_opt is False and m._use_fused is False
        m.build_dataloader()
        m.begin_voter(0)
        assert np.isfinite(m.contrastive_training_epoch())
        assert m._small is None
    # the key is not looked at for RMSprop (its key is small_step) or for model_size='linear', whatever it holds
    for kw in (dict(optimizer='RMSprop'), dict(model_size='linear'), dict(model_size='linear', optimizer='RMSprop')):
        for val in ('native', 'fast'):
            m = models.IID_model(_args(k=4, small_opt_step=val, **{'optimizer': opt, **kw}))
            assert m._small_opt is False and m._use_small is False
    m = models.IID_model(_args(k=4, optimizer='RMSprop', small_step='native', small_opt_step='native'))
    assert m._use_small and not m._small_opt
    m = models.IID_model(_args(k=4, model_size='linear', optimizer='RMSprop', small_opt_step='native'))
    assert m._use_fused


@pytest.mark.parametrize("kw", [dict(small_opt_step='fast'), dict(n_clusters=257), dict(batch_sz=1025),
                                dict(optimizer='SGD', small_opt_step='fast'), dict(optimizer='SGD', n_clusters=257),
                                dict(optimizer='SGD', batch_sz=1025)])
def test_unsupported_native_configurations_raise(dev, kw):
    from idelucs_amd import models
    with pytest.raises(ValueError, match="small_opt_step"):
        models.IID_model(_args(k=4, **kw))


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_small_step_native_still_refuses_sgd_and_adam(dev, opt):
    from idelucs_amd import models
    for extra in (dict(), dict(small_opt_step='native')):
        with pytest.raises(ValueError, match="small_step='native' supports optimizer='RMSprop'.*small_opt_step='native'"):
            models.IID_model(_args(k=4, optimizer=opt, small_step='native', **extra))


def test_trainer_refuses_what_the_launch_does_not_do(dev):
    import torch
    from idelucs_amd.fused_small import FusedSmallOptTrainer
    net = sml._random_net(10, 5, dev)
    for make in (lambda p: torch.optim.SGD(p, lr=LR, momentum=0.9, nesterov=True), lambda p: torch.optim.SGD(p, lr=LR, momentum=0.9, dampening=0.1),
                 lambda p: torch.optim.Adam(p, lr=LR, amsgrad=True), lambda p: torch.optim.SGD(p, lr=LR, maximize=True),
                 lambda p: torch.optim.Adam(p, lr=LR, maximize=True), lambda p: torch.optim.RMSprop(p, lr=LR)):
        with pytest.raises(ValueError, match="FusedSmallOptTrainer"):
            FusedSmallOptTrainer(net, make(net.parameters()), weight=0.25, lamb=2.8)


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_triangle_drives_the_native_step_as_the_autograd_one(dev, opt):
    """Under the Triangle scheduler CyclicLR cycles the rate and SGD's momentum / Adam's beta1: what reaches hyper64 for each epoch's steps
    equals the autograd path's group values for that epoch."""
    from idelucs_amd import models
    traces = {}
    for mode in ("autograd", "native"):
        m = models.IID_model(_args(k=4, optimizer=opt, scheduler='Triangle', small_opt_step=mode))
        m.build_dataloader()
        m.begin_voter(0)
        tr = []
        for _ in range(6):
            grp = m.optimizer.param_groups[0]
            ran_with = [grp['lr'], _second(grp, opt)]            # the values this epoch's steps run with
            m.contrastive_training_epoch()
            if mode == "native":
                have = m._small.hyper64[:2].tolist()
                assert have == ran_with, (have, ran_with)
            tr.append(ran_with)
        traces[mode] = tr
    print(f"{opt} Triangle: (lr, momentum / beta1) per epoch {traces['native']}")
    assert traces["native"] == traces["autograd"], traces
    assert len({t[0] for t in traces["native"]}) > 1 and len({t[1] for t in traces["native"]}) > 1       # (both do cycle)


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_voter_state_carry_keeps_the_state_and_the_step_count(dev, opt, monkeypatch):
    import torch
    from idelucs_amd import models
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "carry")
    m = models.IID_model(_args(k=4, optimizer=opt))
    m.build_dataloader()
    m.begin_voter(0)
    m.contrastive_training_epoch()
    tr = m._small
    before = [v.clone() for v in tr.state_tensors()]
    count = tr.step_count()
    assert count == 12 and all(float(v.abs().sum()) > 0 for v in before)      # 2847 pairs in batches of 256: 11 full + 1 partial
    assert len(before) == (8 if opt == "SGD" else 16)
    m.begin_voter(1)
    assert all(torch.equal(a, b) for a, b in zip(before, tr.state_tensors())) and tr.step_count() == count
    m.contrastive_training_epoch()
    assert tr.step_count() == 2 * count
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "fresh")
    m.begin_voter(2)
    assert all(float(v.abs().sum()) == 0.0 for v in tr.state_tensors()) and tr.step_count() == 0 and tr.steps.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. quality
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_native_small_opt_quality_matches_autograd(dev, opt):
    """Influenza-A, k = 6, 5 clusters, 10 epochs, batch 256, the same 8 seeds through both step forms: the native form's mean ACC is not
    below the autograd form's by more than 3 standard errors of the difference of the two means, computed from the two samples (the rule
    of test_native_momentum_quality_matches_autograd)."""
    import pandas as pd
    import idelucs_amd
    from idelucs_amd import models
    df = pd.read_csv(os.path.join(DATA, "Influenza-A_GT.tsv"), sep="\t")
    u = {v: i for i, v in enumerate(sorted(set(df.cluster_id)))}
    gt = np.array([u[v] for v in df.cluster_id])
    acc = {}
    for mode in ("autograd", "native"):
        acc[mode] = []
        for seed in range(8):
            m = models.IID_model(_args(k=6, optimizer=opt, n_epochs=10, small_opt_step=mode, seed=seed))
            m.build_dataloader()
            m.begin_voter(0)
            for _ in range(10):
                m.contrastive_training_epoch()
            acc[mode].append(idelucs_amd.cluster_acc(gt, m.predict()[0])[1])
    a, n = np.array(acc["autograd"]), np.array(acc["native"])
    se = float(np.sqrt(a.var(ddof=1) / len(a) + n.var(ddof=1) / len(n)))
    print(f"{opt} ACC over 8 seeds: autograd", np.round(a, 4), round(float(a.mean()), 4), "| native", np.round(n, 4), round(float(n.mean()), 4),
          "| 3 standard errors of the difference", round(3 * se, 4))
    assert n.mean() >= a.mean() - 3 * se, (acc, se)


# ------------------------------------------------------------------------------------------------ 8. CLI
def test_cli_small_opt_native_writes_reference_outputs(tmp_path, monkeypatch, capsys):
    import pandas as pd
    from idelucs_amd.__main__ import main
    monkeypatch.chdir(tmp_path)
    out_dir = main(["--sequence_file", os.path.join(DATA, "influenza_64.fas"), "--n_clusters", "5", "--n_epochs", "3", "--n_voters", "2",
                    "--batch_sz", "64", "--k", "6", "--model_size", "small", "--optimizer", "Adam", "--small_opt_step", "native"])
    assert "small_opt_step \t -> native" in capsys.readouterr().out
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 64
    row = open(tmp_path / "ALL_RESULTS.tsv").read().splitlines()[-1]
    assert "'small_opt_step': 'native'" in row
