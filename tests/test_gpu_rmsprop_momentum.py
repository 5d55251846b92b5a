"""GPU tests of the native RMSprop steps that follow the momentum CyclicLR writes into the optimizer (args['rmsprop_momentum'] =
'follow'; csrc/opt_step.hip kind 3, idl_small_wgrad_rms_momentum): the C ABI against torch.optim.RMSprop, the reference's goldens
(tests/golden/make_golden_triangle.py -> triangle.npz / .json) with the momentum-free steps told apart, full-batch steps against
float64 autograd, graph replay against eager launches, the launch budget, IID_model routing, quality and the CLI."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN
import test_gpu_linear_opt_step as lin          # helpers only: the nets, stores, float64 autograd step and launch profile of the SGD / Adam tests
import test_gpu_small_step as sml

pytestmark = pytest.mark.gpu

KIND_RMSPROP = 3
LR, WD, ALPHA, EPS = 1e-3, 0.01, 0.99, 1e-8
# what a scheduler leaves after the first step in the tests below (CyclicLR's fourth momentum, another rate)
MU0, MU1, LR1 = 0.9, 0.82, 2.5e-3


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda")


def _rmsprop(params, momentum=MU0):
    """The optimizer object of reference models.py:87-88 as CyclicLR (models.py:99) leaves it at construction."""
    import torch
    return torch.optim.RMSprop(params, lr=LR, weight_decay=WD, momentum=momentum)


def _lin_trainer(net, seed=5, momentum=MU0):
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    tr = FusedLinearOptTrainer(net, _rmsprop(net.parameters(), momentum), weight=0.25, lamb=2.8, seed=seed)
    tr.begin_voter(0)
    return tr


def _small_trainer(net, seed=5, momentum=MU0):
    from idelucs_amd.fused_small import FusedSmallTrainer
    tr = FusedSmallTrainer(net, lr=LR, weight=0.25, lamb=2.8, seed=seed, momentum=momentum)
    tr.begin_voter(0)
    return tr


def _within(have, want, name, rel=1e-5):
    """have within rel of want's largest magnitude (the bar tests/test_gpu_linear_opt_step.py holds kinds 1 and 2 to)."""
    err, top = (have - want).abs().max().item(), want.abs().max().item()
    print(f"  {name}: max error {err / max(top, 1e-30):.2e} of the tensor's max")
    assert err <= rel * top, (name, err, top)


def _shadow_check(sopt, shadow, params, sq, buf, names, mu):
    """torch's RMSprop has stepped `shadow` on the same gradients: parameters and both states.  (With momentum 0 torch keeps no buffer:
    the kernel's is then this step's g' / avg, which torch's addcdiv_ forms and does not keep -- it is checked through the parameters.)"""
    for i, n_ in enumerate(names):
        state = sopt.state[shadow[i]]
        _within(params[i].detach(), shadow[i].detach(), n_ + " parameter")
        _within(sq[i], state["square_avg"], n_ + " square_avg")
        if mu > 0:
            _within(buf[i], state["momentum_buffer"], n_ + " momentum_buffer")


# ------------------------------------------------------------------------------------------------ 1. the C ABI, called directly
@pytest.mark.parametrize("mu", [MU0, 0.0])
@pytest.mark.parametrize("wg_m,transposed", [(40, 0), (128, 1)])
def test_opt_step_kind_3_matches_torch_rmsprop(dev, mu, wg_m, transposed):
    """idl_opt_step_gather_wgrad(kind 3) on four tensors, one per code path -- 4096 elements (16-byte streaming), 1001 (scalar), 64 with 17
    stacked partials (the first and a chunk of 16), a 16 x 32 tile computed in the launch (wg_m = 40: uneven wave shares and a K tail; 128 with the
    operand transposed) -- three consecutive steps, the momentum and the rate changed after the first, against torch.optim.RMSprop fed
    the same gradients from the same start."""
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.fused import _p, _stream
    gen = torch.Generator(device=dev).manual_seed(77 + wg_m)
    sizes, parts = [4096, 1001, 64, 16 * 32], [1, 1, 17, 1]
    names = ["streamed 4096", "scalar 1001", "17 partials", "in-launch tile"]
    params = [torch.randn(n, device=dev, generator=gen) for n in sizes]
    sq = [torch.zeros_like(p) for p in params]
    buf = [torch.zeros_like(p) for p in params]
    grads = [torch.zeros((q, n), device=dev) if q > 1 else torch.zeros(n, device=dev) for n, q in zip(sizes, parts)]
    wg_grad = torch.zeros(16 * 32, device=dev)
    shadow = [p.clone().requires_grad_(True) for p in params]
    sopt = _rmsprop(shadow, mu)
    hyper = torch.tensor([LR, mu, ALPHA, EPS, WD], dtype=torch.float64, device=dev)
    steps = torch.zeros(2, dtype=torch.int64, device=dev)
    ctl = torch.tensor([5, 100], dtype=torch.int64, device=dev)
    arr = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])
    pp, gp, s1, s2 = arr(params), arr(grads), arr(sq), arr(buf)
    sz, pt = (ctypes.c_int64 * 4)(*sizes), (ctypes.c_int32 * 4)(*parts)
    for it in range(3):
        if it == 1:
            lr1, mu1 = LR1, (MU1 if mu > 0 else 0.0)
            sopt.param_groups[0]['lr'], sopt.param_groups[0]['momentum'] = lr1, mu1
            hyper.copy_(torch.tensor([lr1, mu1, ALPHA, EPS, WD], dtype=torch.float64))
        for g_ in grads:
            g_.copy_(torch.randn(g_.shape, device=dev, generator=gen))
        dy = torch.randn((wg_m, 16), device=dev, generator=gen)
        x = torch.randn((wg_m, 32), device=dev, generator=gen)
        xk = x.t().contiguous() if transposed else x
        par = it % 2
        tail = _lib.idl_opt_tail_t(count=4, params=pp, grads=gp, grad_parts=pt, sizes=sz, ctl=_p(ctl), skip_index=-1, wg_index=3, wg_dy=_p(dy),
                                   wg_x=_p(xk), wg_x_transposed=transposed, wg_m=wg_m, wg_n_out=16, wg_n_in=32, wg_grad=_p(wg_grad), batch_advance=7)
        opt = _lib.idl_opt_state_t(KIND_RMSPROP, s1, s2, _p(hyper), _p(steps[par:]), _p(steps[1 - par:]))
        _lib.check(_lib.lib.idl_opt_step_gather_wgrad(tail, opt, None, _stream()))
        torch.cuda.synchronize()
        want = (dy.double().t() @ x.double()).reshape(-1)
        _within(wg_grad.double(), want, f"step {it} dy^T x", rel=2e-3)          # (the gradient bar of the step tests)
        fed = [grads[0], grads[1], None, wg_grad]
        # the stacked partials added in ascending order, as the kernel adds them
        acc = grads[2][0].clone()
        for q in range(1, 17):
            acc += grads[2][q]
        fed[2] = acc
        for p, g_ in zip(shadow, fed):
            p.grad = g_.clone()
        sopt.step()
        print(f"step {it}, momentum {hyper[1].item()}:")
        _shadow_check(sopt, shadow, params, sq, buf, names, mu)
        # the step words swap roles and the counters advance as for kinds 1 and 2
        assert steps[1 - par].item() == it + 1
        assert ctl.tolist() == [5 + it + 1, 100 + 7 * (it + 1)]
    assert sorted(steps.tolist()) == [2, 3]


@pytest.mark.parametrize("mu", [MU0, 0.0])
@pytest.mark.parametrize("m", [18, 64])
@pytest.mark.parametrize("F", [10, 136])
def test_small_wgrad_rms_momentum_matches_torch_rmsprop(dev, mu, m, F):
    """idl_small_wgrad_rms_momentum on random layer inputs and output gradients (C = 7): the gradients it writes against float64
    products, and three consecutive updates, the momentum and the rate changed after the first, against torch.optim.RMSprop fed those
    gradients."""
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.fused import _p, _stream
    C, H1, H2, LAT = 7, 400, 128, 64
    gen = torch.Generator(device=dev).manual_seed(31 * m + F)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
    shapes = [(H1, F), (H1,), (H2, H1), (H2,), (LAT, H2), (LAT,), (C, H2), (C,)]
    params = [rnd(*s) for s in shapes]
    sq, buf, grads = ([torch.zeros_like(p) for p in params] for _ in range(3))
    shadow = [p.clone().requires_grad_(True) for p in params]
    sopt = _rmsprop(shadow, mu)
    hyper = torch.tensor([LR, ALPHA, EPS, WD, 1.0 - ALPHA, mu], dtype=torch.float32, device=dev)
    ctl = torch.tensor([9, 0], dtype=torch.int64, device=dev)
    arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])
    pp, gp, vp, mp = arr(params), arr(grads), arr(sq), arr(buf)
    for it in range(3):
        if it == 1:
            lr1, mu1 = LR1, (MU1 if mu > 0 else 0.0)
            sopt.param_groups[0]['lr'], sopt.param_groups[0]['momentum'] = lr1, mu1
            hyper[0:1].fill_(lr1)
            hyper[5:6].fill_(mu1)
        x, a1, a2, d2 = rnd(m, F), rnd(m, H1), rnd(m, H2), rnd(m, H2)
        dr1, da2, dh, dlogits = rnd(m, H1), rnd(m, H2), rnd(m, LAT), rnd(m, C)
        _lib.check(_lib.lib.idl_small_wgrad_rms_momentum(
            pp, gp, vp, mp, _p(hyper), _p(ctl), _p(x), _p(dr1), _p(a1), _p(da2), _p(a2), _p(dh), _p(d2), _p(dlogits), m, F, C,
            None, 0.0, 0.0, None, None, _stream()))
        torch.cuda.synchronize()
        print(f"m = {m}, F = {F}, step {it}, momentum {hyper[5].item()}:")
        for i, (dy, xin) in enumerate(((dr1, x), (da2, a1), (dh, a2), (dlogits, d2))):
            _within(grads[2 * i].double(), dy.double().t() @ xin.double(), sml.NAMES[2 * i] + " gradient", rel=2e-3)
            _within(grads[2 * i + 1].double(), dy.double().sum(0), sml.NAMES[2 * i + 1] + " gradient", rel=2e-3)
        for p, g_ in zip(shadow, grads):
            p.grad = g_.clone()
        sopt.step()
        _shadow_check(sopt, shadow, params, sq, buf, sml.NAMES, mu)
        assert ctl.tolist() == [9 + it + 1, 0]


# ------------------------------------------------------------------------------------------------ 2. the reference's goldens
@pytest.fixture(scope="module")
def tri():
    return np.load(os.path.join(GOLDEN, "triangle.npz")), json.load(open(os.path.join(GOLDEN, "triangle.json")))


def _golden_args(size, C, **kw):
    a = {'sequence_file': None, 'GT_file': None, 'n_clusters': C, 'k': 2, 'model_size': size, 'n_mimics': 3, 'batch_sz': 9,
         'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': 'Triangle', 'n_epochs': 2, 'n_voters': 1}
    a.update(kw)
    return a


def _golden_run(model, tr, g, size, names, before_epoch, dev):
    """Two epochs of three golden batches stepped by hand (dropout off), the scheduler stepped by IID_model._finish_epoch between them.
    before_epoch(epoch) hands the optimizer group's values to the trainer and checks them.  Yields (epoch, its loss, the parameters after it)."""
    import torch
    model.net.load_state_dict({n: torch.from_numpy(g[f"{size}.w.{n}"]) for n in model.net.state_dict()})
    xs = [torch.cat([torch.from_numpy(g[f"{size}.x1.{i}"]), torch.from_numpy(g[f"{size}.x2.{i}"])]).to(dev) for i in range(3)]
    bf = tr.buffers(18)
    losses = []
    for epoch in range(2):
        before_epoch(epoch)
        tr.out[1] = 0.0
        for i in range(3):
            bf.x.copy_(xs[i])
            tr.step_on_batch(bf, train=False)
        loss = tr.out[1] / 2                                     # reference models.py:135: divided by the last batch index
        losses.append(model._finish_epoch(loss, sync=False).item())
        snap = {n_: p.detach().cpu().numpy().copy() for n_, p in zip(names, tr.params)}
        yield epoch, losses[-1], snap


@pytest.mark.parametrize("size", ["linear", "small"])
def test_two_triangle_epochs_match_the_reference_and_differ_from_the_momentum_free_step(dev, tri, size):
    """triangle.npz: the reference's IID_model with RMSprop under the Triangle scheduler, NetLinear(16, 5) / myNet(10, 7), m = 18 (the
    unfused branch), dropout off, two epochs of three batches.  The native steps built on an IID_model with rmsprop_momentum='follow'
    run with the golden (lr, momentum) and land on the reference's parameters; the same run on today's momentum-free steps is more than
    10 x further away in every weight matrix.

    The reference's own float32 run against its float64 twin leaves at most 1.2e-3 of a tensor's entries outside rtol 1e-3, atol 1e-6
    (triangle.json); the cap here is the project's 5e-3 for sign-like first steps."""
    import torch
    from idelucs_amd import models
    from idelucs_amd.fused import FusedLinearTrainer
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    from idelucs_amd.fused_small import FusedSmallTrainer
    g, meta = tri
    C = meta["shapes"][size]["C"]
    names = lin.NAMES if size == "linear" else sml.NAMES
    extra = dict(small_step='native') if size == "small" else {}

    def compare(snap, epoch):
        for n_ in names:
            key = f"{size}.epoch{epoch + 1}.p.{n_}"
            if key in g.files:
                bad = ~np.isclose(snap[n_], g[key], rtol=1e-3, atol=1e-6)
                print(f"  {key}: {bad.mean():.2e} of the entries outside, max difference {np.abs(snap[n_] - g[key]).max():.2e}")
                assert bad.mean() <= 5e-3, (key, float(bad.mean()))

    # ---- the new steps
    model = models.IID_model(_golden_args(size, C, rmsprop_momentum='follow', **extra))
    grp = model.optimizer.param_groups[0]
    if size == "linear":
        assert model._use_linopt and not model._use_fused
        tr = FusedLinearOptTrainer(model.net, model.optimizer, model.weight, model.l, seed=0)
        assert tr.kind == KIND_RMSPROP
        model._linopt = tr
        on_device = lambda: tr.hyper64[:2].tolist()
        hand_over = tr.sync_hyper
    else:
        assert model._use_small and model._small_momentum
        tr = FusedSmallTrainer(model.net, model.lr, model.weight, model.l, seed=0, momentum=grp['momentum'])
        model._small = tr
        on_device = lambda: [tr.hyper[0].item(), tr.hyper[5].item()]
        hand_over = lambda: (tr.set_lr(grp['lr']), tr.set_momentum(grp['momentum']))
    model.begin_voter(0)

    def before_epoch(epoch):
        hand_over()
        have, want = on_device(), g[f"{size}.hyper"][epoch]
        print(f"epoch {epoch + 1}: (lr, momentum) on the device {have}, golden {want.tolist()}")
        assert all(abs(a - b) <= 1e-6 * abs(b) for a, b in zip(have, want)), (have, want)
    for epoch, loss, snap in _golden_run(model, tr, g, size, names, before_epoch, dev):
        ref = float(g[f"{size}.epoch_loss"][epoch])
        print(f"{size} epoch {epoch + 1}: loss {loss:.7f} reference {ref:.7f}")
        assert abs(loss - ref) <= 5e-4 * abs(ref), (epoch, loss, ref)
        compare(snap, epoch)
    assert [grp['lr'], grp['momentum']] == g[f"{size}.hyper"][2].tolist()
    followed = snap

    # ---- today's steps, the momentum ignored
    model = models.IID_model(_golden_args(size, C, **extra))
    grp = model.optimizer.param_groups[0]
    if size == "linear":
        assert model._use_fused
        old = FusedLinearTrainer(model.net, model.lr, model.weight, model.l, seed=0)
        model._fused = old
    else:
        old = FusedSmallTrainer(model.net, model.lr, model.weight, model.l, seed=0)
        model._small = old
    model.begin_voter(0)
    for epoch, loss, snap in _golden_run(model, old, g, size, names, lambda e: old.set_lr(grp['lr']), dev):
        pass
    for n_ in names:
        want = g[f"{size}.epoch2.p.{n_}"]
        if want.ndim == 2:
            near, far = np.abs(followed[n_] - want).mean(), np.abs(snap[n_] - want).mean()
            print(f"  {n_}: mean |difference| to the golden {near:.3e} with the momentum, {far:.3e} without ({far / near:.1e} x)")
            assert far > 10 * near, (n_, near, far)


# ------------------------------------------------------------------------------------------------ 3. against autograd and torch.optim
@pytest.mark.parametrize("F,m,C", [(256, 512, 5), (4096, 1024, 20), (1024, 512, 200)])
def test_three_full_batch_steps_match_autograd_and_torch_rmsprop(dev, F, m, C):
    """The scheme of test_gpu_linear_opt_step._three_steps (pipelined steps, float64 autograd on the branch the trainer took, the
    trainer's gradients through torch's optimizer), the momentum and the rate changed after the first step."""
    import torch
    net = lin._random_net(F, C, dev, seed=F + m + C)
    st = lin._store(F, dev)
    x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(F * 7 + m + C))
    tr = _lin_trainer(net)
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    bf = tr.buffers(m)
    shadow = [p.detach().clone().requires_grad_(True) for p in tr.params]
    sopt = _rmsprop(shadow)
    for it in range(3):
        if it == 1:
            for o in (tr.optimizer, sopt):
                o.param_groups[0]['momentum'], o.param_groups[0]['lr'] = MU1, LR1
            tr.sync_hyper()
        before = copy.deepcopy(net)
        bf.xs[0].copy_(x)
        tr.step_on_batch(bf, train=False, batch_advance=m // 2, next_from=st, xi=0)
        torch.cuda.synchronize()
        loss_ref, grads_ref = lin._autograd_step(before, x, (tr.layer1_output(bf) > 0, bf.r2 > 0))
        got = tr.out[0].item()
        print(f"RMSprop F={F} m={m} C={C} step {it}: loss {got:.7f} autograd {loss_ref:.7f}")
        assert abs(got - loss_ref) <= 2e-4 * abs(loss_ref), (it, got, loss_ref)
        for i, n_ in enumerate(lin.NAMES):
            _within(tr.gradient(i), grads_ref[i], n_ + " gradient", rel=2e-3)
        for p, i in zip(shadow, range(6)):
            p.grad = tr.gradient(i).clone()
        sopt.step()
        _shadow_check(sopt, shadow, tr.params, tr.state1, tr.state2, lin.NAMES, MU0)
    assert tr.step_count() == 3


# ------------------------------------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("C", [20, 200])
def test_linear_epochs_replayed_from_the_graph_equal_eager_launches(dev, C):
    """1560 pairs in batches of 128: 12 full batches and a partial one of 24, three epochs (13 steps each: the second epoch starts with the
    step words in the other roles), the momentum changed between epochs as CyclicLR changes it.  Bit-identical to eager launches."""
    import torch
    st = lin._Store(520, 3, 256, dev, seed=2)
    runs = []
    for use_graph in (True, False):
        tr = _lin_trainer(lin._random_net(256, C, dev, seed=4), seed=6)
        gen = torch.Generator(device=dev).manual_seed(123)
        losses = []
        for mu, lr in ((0.9, 1e-3), (0.88, 2e-3), (0.86, 3e-3)):
            tr.optimizer.param_groups[0]['momentum'], tr.optimizer.param_groups[0]['lr'] = mu, lr
            tr.sync_hyper()
            total, nb = tr.run_epoch(st, 128, generator=gen, use_graph=use_graph)
            assert nb == 13
            losses.append(total.clone())
        torch.cuda.synchronize()
        assert len(tr._graphs) == (2 if use_graph else 0) and getattr(tr, "n_captures", 0) == (2 if use_graph else 0)
        assert tr.step_count() == 39 and tr.ctl.tolist() == [39, 1560]
        assert all(bool(torch.isfinite(t)) for t in losses) and all(float(v.abs().sum()) > 0 for v in tr.state_tensors())
        assert len(tr.state_tensors()) == 12
        runs.append([p.detach().clone() for p in tr.params] + [v.clone() for v in tr.state_tensors()] + losses
                    + [tr.steps.clone(), tr.out.clone(), tr.ctl.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_small_epochs_replayed_from_the_graph_equal_eager_launches(dev):
    """1500 pairs in batches of 256 (5 full batches and a partial one of 220), three epochs, the momentum changed between them."""
    import torch
    st = sml._Store(500, 3, 512, dev, seed=2)
    runs = []
    for use_graph in (True, False):
        tr = _small_trainer(sml._random_net(512, 20, dev, seed=4), seed=6)
        gen = torch.Generator(device=dev).manual_seed(123)
        losses = []
        for mu, lr in ((0.9, 1e-3), (0.88, 2e-3), (0.86, 3e-3)):
            tr.set_lr(lr)
            tr.set_momentum(mu)
            total, nb = tr.run_epoch(st, 256, generator=gen, use_graph=use_graph)
            assert nb == 6
            losses.append(total.clone())
        torch.cuda.synchronize()
        assert len(tr._graphs) == (1 if use_graph else 0)
        assert all(bool(torch.isfinite(t)) for t in losses) and all(float(v.abs().sum()) > 0 for v in tr.square_avg + tr.momentum_buffer)
        runs.append([p.detach().clone() for p in tr.params] + tr.square_avg + tr.momentum_buffer + losses + [tr.out.clone(), tr.ctl.clone()])
        assert tr.ctl.tolist() == [18, 1280]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. launches
def test_linear_full_batch_step_launch_budget(dev):
    F, m = 4096, 1024
    st = lin._store(F, dev)
    tr = _lin_trainer(lin._random_net(F, 20, dev), seed=2)
    names = lin._kernel_names(lin._pipelined(tr, st, m, dev), 4)
    print(f"RMSprop with momentum, C = 20: {len(names) / 4:.1f} launches a step")
    assert not [n for n in names if "Cijk" in n], names
    assert 0 < len(names) <= 7 * 4, (len(names), names)
    for k in ("opt_step_kernel<3>", "wgrad_q16", "l1_fwd_kernel"):
        assert sum(k in n for n in names) == 4, (k, names)
    # n_clusters = 200: no more launches and no more library products than the SGD form
    tr = _lin_trainer(lin._random_net(F, 200, dev), seed=2)
    names = lin._kernel_names(lin._pipelined(tr, st, m, dev), 4)
    sgd = lin._trainer(lin._random_net(F, 200, dev), "SGD", seed=2)
    sgd_names = lin._kernel_names(lin._pipelined(sgd, st, m, dev), 4)
    lib, sgd_lib = sum("Cijk" in n for n in names), sum("Cijk" in n for n in sgd_names)
    print(f"C = 200: {len(names) / 4:.1f} launches a step ({lib / 4:.1f} library products); the SGD form {len(sgd_names) / 4:.1f} ({sgd_lib / 4:.1f})")
    assert len(names) <= len(sgd_names) and lib <= sgd_lib, (names, sgd_names)
    assert sum("opt_step_kernel<3>" in n for n in names) == 4, names


def test_small_full_batch_step_launch_budget(dev):
    import torch
    F, B = 2080, 512
    st = sml._Store(2048, 3, F, dev, seed=1)
    tr = _small_trainer(sml._random_net(F, 20, dev), seed=2)
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    tr.ctl[1:2].zero_()
    bf = tr.buffers(2 * B)
    tr._gather(st, bf, B)
    names = lin._kernel_names(lambda i: tr.step_on_batch(bf, xi=i % 2, next_from=st), 4)
    print(f"small, C = 20: {len(names) / 4:.1f} launches a step")
    assert not [n for n in names if "Cijk" in n], names
    assert len(names) == 6 * 4, (len(names), names)
    for k in ("small_l1_fwd_kernel", "small_mid_fwd_kernel", "small_mid_bwd_kernel", "small_wgrad_momentum_kernel"):
        assert sum(k in n for n in names) == 4, (k, names)
    assert not [n for n in names if "small_wgrad_rms_kernel" in n], names


# ------------------------------------------------------------------------------------------------ 6. IID_model
def _args(**kw):
    a = {'sequence_file': os.path.join(DATA, "Influenza-A.fas"), 'GT_file': None, 'n_clusters': 5, 'k': 4, 'model_size': 'linear',
         'n_mimics': 3, 'batch_sz': 256, 'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': 'Triangle',
         'n_epochs': 3, 'n_voters': 1}
    a.update(kw)
    return a


def _epochs(args, n):
    from idelucs_amd import models
    m = models.IID_model(args)
    m.build_dataloader()
    m.begin_voter(0)
    return m, [m.contrastive_training_epoch() for _ in range(n)]


@pytest.mark.parametrize("size", ["linear", "small"])
def test_without_the_key_or_with_ignore_nothing_changes(dev, size):
    from idelucs_amd import models
    extra = dict(model_size='small', small_step='native') if size == "small" else {}
    base, want = _epochs(_args(**extra), 3)
    for val in (None, 'ignore'):
        m, losses = _epochs(_args(rmsprop_momentum=val, **extra), 3)
        assert losses == want, (val, losses, want)              # bit for bit
        if size == "linear":
            assert m._use_fused and not m._use_linopt and m._fused is not None and m._linopt is None
        else:
            assert m._use_small and not m._small_momentum and not m._small.with_momentum and m._small.hyper.numel() == 5
    # 'follow' without the Triangle scheduler: the momentum is 0 for the whole run, nothing is rerouted
    for sched in (None, 'None', 'Plateau'):
        m = models.IID_model(_args(rmsprop_momentum='follow', scheduler=sched, **extra))
        assert m.optimizer.param_groups[0]['momentum'] == 0
        assert (m._use_fused, m._use_linopt, m._small_momentum) == (size == "linear", False, False)


@pytest.mark.parametrize("size", ["linear", "small"])
def test_follow_routes_to_the_momentum_steps_and_hands_over_the_groups_values(dev, size, monkeypatch):
    from idelucs_amd import fused, models
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    extra = dict(model_size='small', small_step='native') if size == "small" else {}
    m = models.IID_model(_args(rmsprop_momentum='follow', **extra))
    m.build_dataloader()
    m.begin_voter(0)
    grp = m.optimizer.param_groups[0]
    trace = []
    for epoch in range(6):
        want = [grp['lr'], grp['momentum'], grp['alpha'], grp['eps'], grp['weight_decay']]
        loss = m.enqueue_epoch()
        if size == "linear":
            assert isinstance(m._linopt, FusedLinearOptTrainer) and m._linopt.kind == KIND_RMSPROP and m._fused is None
            have = m._linopt.hyper64.tolist()
        else:
            assert m._small.with_momentum and m._fused is None and m._linopt is None
            h = m._small.hyper.tolist()
            have = [h[0], h[5], h[1], h[2], h[3]]
        assert all(abs(a - b) <= 1e-6 * abs(b) for a, b in zip(have, want)), (epoch, have, want)
        assert np.isfinite(m._finish_epoch(loss))
        trace.append((grp['lr'], grp['momentum']))
    print(f"{size}: (lr, momentum) after each epoch {trace}")
    assert len({t[1] for t in trace}) > 1
    # the autograd path's scheduler writes the same values
    if size == "linear":
        monkeypatch.setitem(fused.VARIANTS, "fused", "0")
        a = models.IID_model(_args(rmsprop_momentum='follow'))
        assert not a._use_fused and not a._use_linopt
    else:
        a = models.IID_model(_args(rmsprop_momentum='follow', model_size='small', small_step='autograd'))
        assert not a._use_small
    a.build_dataloader()
    a.begin_voter(0)
    auto = []
    for _ in range(6):
        a.contrastive_training_epoch()
        auto.append((a.optimizer.param_groups[0]['lr'], a.optimizer.param_groups[0]['momentum']))
    assert a._linopt is None and a._small is None and a._fused is None
    assert auto == trace, (auto, trace)
    assert "momentum_buffer" in a.optimizer.state[next(iter(a.net.parameters()))]


def test_the_key_is_validated_for_rmsprop_only(dev):
    from idelucs_amd import models
    for kw in (dict(), dict(model_size='small', small_step='native'), dict(scheduler=None)):
        with pytest.raises(ValueError, match="rmsprop_momentum"):
            models.IID_model(_args(rmsprop_momentum='cycle', **kw))
    for opt in ("SGD", "Adam"):
        for val in ('follow', 'cycle'):
            for step in ('native', 'autograd'):
                m = models.IID_model(_args(optimizer=opt, rmsprop_momentum=val, linear_step=step))
                assert not m._use_fused and not m._small_momentum and m._use_linopt == (step == 'native')
        m = models.IID_model(_args(optimizer=opt, rmsprop_momentum='follow', linear_step='native'))
        m.build_dataloader()
        m.begin_voter(0)
        assert np.isfinite(m.contrastive_training_epoch()) and m._linopt.kind in (1, 2)


def test_trainer_refuses_centered_and_maximize(dev):
    import torch
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    net = lin._random_net(256, 5, dev)
    for kw in (dict(centered=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="centered and maximize"):
            FusedLinearOptTrainer(net, torch.optim.RMSprop(net.parameters(), lr=1e-3, momentum=0.9, **kw), 0.25, 2.8)
    with pytest.raises(ValueError, match="momentum"):
        sml._trainer(sml._random_net(136, 5, dev)).set_momentum(0.9)


@pytest.mark.parametrize("size", ["linear", "small"])
def test_voter_state_carry_keeps_both_states_and_the_step_count(dev, size, monkeypatch):
    import torch
    from idelucs_amd import models
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "carry")
    extra = dict(model_size='small', small_step='native') if size == "small" else {}
    m = models.IID_model(_args(rmsprop_momentum='follow', **extra))
    m.build_dataloader()
    m.begin_voter(0)
    m.contrastive_training_epoch()
    tr = m._linopt if size == "linear" else m._small
    state = (lambda: tr.state_tensors()) if size == "linear" else (lambda: tr.square_avg + tr.momentum_buffer)
    count = (lambda: tr.step_count()) if size == "linear" else (lambda: int(tr.ctl[0].item()) & 0xFFFFFF)
    before = [v.clone() for v in state()]
    assert len(before) == 2 * len(tr.params) and all(float(v.abs().sum()) > 0 for v in before)
    assert count() == 12                                        # 2847 pairs in batches of 256: 11 full + 1 partial
    mom = m.optimizer.param_groups[0]['momentum']
    m.begin_voter(1)
    assert all(torch.equal(a, b) for a, b in zip(before, state()))
    assert m.optimizer.param_groups[0]['momentum'] == mom       # (the one optimizer and scheduler serve every voter)
    if size == "linear":
        assert tr.step_count() == 12
        m.contrastive_training_epoch()
        assert tr.step_count() == 24
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "fresh")
    m.begin_voter(2)
    assert all(float(v.abs().sum()) == 0.0 for v in state())
    assert m.optimizer.param_groups[0]['momentum'] == 0.9
    if size == "linear":
        assert tr.step_count() == 0 and tr.steps.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. quality
@pytest.mark.parametrize("size", ["linear", "small"])
def test_native_momentum_quality_matches_autograd(dev, size, monkeypatch):
    """Influenza-A, k = 6, 5 clusters, batch 256, Triangle, 10 epochs (one full cycle), the same 8 seeds through the native form that
    follows the momentum and through the autograd form: the native mean ACC is not below the autograd mean by more than 3 standard
    errors of the difference of the two means (the rule of test_native_adam_quality_matches_autograd).  The momentum-free native form's
    sample is printed beside them, without a bar."""
    import pandas as pd
    import idelucs_amd
    from idelucs_amd import fused, models
    df = pd.read_csv(os.path.join(DATA, "Influenza-A_GT.tsv"), sep="\t")
    u = {v: i for i, v in enumerate(sorted(set(df.cluster_id)))}
    gt = np.array([u[v] for v in df.cluster_id])
    forms = {"follow": dict(rmsprop_momentum='follow'), "ignore": dict(rmsprop_momentum='ignore'), "autograd": dict(rmsprop_momentum='follow')}
    acc = {}
    for form, kw in forms.items():
        if size == "small":
            kw = dict(kw, model_size='small', small_step='autograd' if form == "autograd" else 'native')
        acc[form] = []
        with monkeypatch.context() as mp:
            if form == "autograd" and size == "linear":
                mp.setitem(fused.VARIANTS, "fused", "0")
            for seed in range(8):
                m = models.IID_model(_args(k=6, n_epochs=10, seed=seed, **kw))
                if form == "autograd":
                    assert not (m._use_fused or m._use_linopt or m._use_small)
                elif form == "follow":
                    assert m._use_linopt or m._small_momentum
                m.build_dataloader()
                m.begin_voter(0)
                try:
                    for _ in range(10):
                        m.contrastive_training_epoch()
                except models.PlanesOverflow:           # (the default two-plane step at these rates; training.train_voter reruns such a voter)
                    assert form == "ignore"
                    acc[form].append(float("nan"))
                    continue
                acc[form].append(idelucs_amd.cluster_acc(gt, m.predict()[0])[1])
    a, n, i = (np.array(acc[k]) for k in ("autograd", "follow", "ignore"))
    se = float(np.sqrt(a.var(ddof=1) / len(a) + n.var(ddof=1) / len(n)))
    print(f"{size}: ACC over 8 seeds: autograd", np.round(a, 4), round(float(a.mean()), 4), "| native, momentum followed", np.round(n, 4),
          round(float(n.mean()), 4), "| 3 standard errors of the difference", round(3 * se, 4),
          "| native, momentum ignored (no bar)", np.round(i, 4), round(float(np.nanmean(i)), 4))
    assert n.mean() >= a.mean() - 3 * se, (acc, se)


# ------------------------------------------------------------------------------------------------ 8. CLI
def test_cli_follow_writes_reference_outputs(tmp_path, monkeypatch, capsys):
    import pandas as pd
    from idelucs_amd.__main__ import main
    monkeypatch.chdir(tmp_path)
    out_dir = main(["--sequence_file", os.path.join(DATA, "influenza_64.fas"), "--n_clusters", "5", "--n_epochs", "3", "--n_voters", "2",
                    "--batch_sz", "64", "--k", "6", "--scheduler", "Triangle", "--rmsprop_momentum", "follow"])
    assert "rmsprop_momentum \t -> follow" in capsys.readouterr().out
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 64
    row = open(tmp_path / "ALL_RESULTS.tsv").read().splitlines()[-1]
    assert "'rmsprop_momentum': 'follow'" in row
