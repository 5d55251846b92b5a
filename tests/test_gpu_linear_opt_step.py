"""GPU tests of the native SGD / Adam step of NetLinear (idelucs_amd/fused_opt.py + csrc/opt_step.hip): the reference's goldens,
full-batch steps against float64 autograd and torch's own optimizers (three consecutive steps), dropout on, graph replay against
eager launches, the launch budget, IID_model / scheduler / carried-state / CLI integration and the quality of a 10-epoch run against
the autograd form."""
import copy
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN
from linear_dropout_ref import _autograd_step, masks as restated_masks

pytestmark = pytest.mark.gpu

NAMES = ["layers.0.weight", "layers.0.bias", "layers.3.weight", "layers.3.bias", "classifier.2.weight", "classifier.2.bias"]


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
        return torch.optim.SGD(params, lr=1e-3, weight_decay=0.01, momentum=0.9)
    return torch.optim.Adam(params, lr=1e-3)


def _trainer(net, opt, seed=5):
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    tr = FusedLinearOptTrainer(net, _optimizer(opt, net.parameters()), weight=0.25, lamb=2.8, seed=seed)
    tr.begin_voter(0)
    return tr


def _random_net(F, C, dev, seed=0):
    import torch
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.models import weights_init
    torch.manual_seed(seed)
    net = NetLinear(F, C)
    net.apply(weights_init)
    return net.to(dev)


class _Store:
    """A feature store with the fields of utils.FeatureStore the trainer reads (n sequences, n_views mimic views, f features)."""

    def __init__(self, n, n_views, f, dev, seed=0):
        import torch
        g = torch.Generator(device=dev).manual_seed(seed)
        self.n, self.f, self.n_views = n, f, n_views
        self.n_pairs = n * n_views
        self.feats = torch.rand(((n_views + 1) * n, f), device=dev, generator=g)
        self.mean = self.feats[:n].double().mean(0)
        self.scale = self.feats[:n].double().std(0).clamp_min(1e-3)
        self.inv_scale = 1.0 / self.scale


_STORES = {}


def _store(F, dev):
    if F not in _STORES:
        _STORES.clear()
        _STORES[F] = _Store(1024, 3, F, dev, seed=1)
    return _STORES[F]


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
def _close_but_for_flips(got, want, name, rtol=1e-4, atol=1e-6, frac=2e-3):
    bad = ~np.isclose(got, want, rtol=rtol, atol=atol)
    assert bad.mean() <= frac, (name, float(bad.mean()), float(np.abs(got - want).max()))


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_three_steps_match_the_reference_goldens(dev, opt):
    """optimizers.npz: NetLinear(16, 5), m = 18 (not a multiple of 16: the unfused branch), dropout off, three steps -- the bars
    tests/test_gpu_optimizers.py::test_sgd_and_adam_steps_vs_reference applies to the autograd path."""
    import torch
    from idelucs_amd.PytorchUtils import NetLinear
    g = np.load(os.path.join(GOLDEN, "optimizers.npz"))
    net = NetLinear(16, 5)
    net.load_state_dict({n: torch.from_numpy(g[f"init11.w.{n}"]) for n in net.state_dict()})
    net = net.to(dev)
    tr = _trainer(net, opt)
    bf = tr.buffers(18)
    x = torch.cat([torch.from_numpy(g["x1.0"]), torch.from_numpy(g["x2.0"])]).to(dev)
    for it in range(3):
        bf.x.copy_(x)
        tr.step_on_batch(bf, train=False)
        torch.cuda.synchronize()
        ref = float(g[f"{opt}.step{it}.loss"])
        print(f"{opt} step {it}: loss {tr.out[0].item():.7f} reference {ref:.7f}")
        assert abs(tr.out[0].item() - ref) <= 3e-4 * abs(ref), (opt, it, tr.out[0].item(), ref)
        for n_, p in zip(NAMES, tr.params):
            key = f"{opt}.step{it}.p.{n_}"
            if key in g.files:
                _close_but_for_flips(p.detach().cpu().numpy(), g[key], key, frac=2e-3 if opt == "Adam" else 0.0)
    assert tr.step_count() == 3 and tr.ctl.tolist() == [3, 0]


# ------------------------------------------------------------------------------------------------ 2. against autograd and torch.optim
def _three_steps(dev, opt, F, m, C, change_after_first=False):
    import torch
    net = _random_net(F, C, dev, seed=F + m + C)
    st = _store(F, dev)
    x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(F * 7 + m + C))
    tr = _trainer(net, opt)
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    bf = tr.buffers(m)
    shadow = [p.detach().clone().requires_grad_(True) for p in tr.params]
    sopt = _optimizer(opt, shadow)
    for it in range(3):
        if change_after_first and it == 1:              # as a scheduler would leave them (CyclicLR cycles momentum / beta1)
            for o in (tr.optimizer, sopt):
                if opt == "SGD":
                    o.param_groups[0]['momentum'] = 0.8
                else:
                    o.param_groups[0]['betas'] = (0.8, 0.999)
                o.param_groups[0]['lr'] = 2.5e-3
            tr.sync_hyper()
        before = copy.deepcopy(net)
        bf.xs[0].copy_(x)
        tr.step_on_batch(bf, train=False, batch_advance=m // 2, next_from=st, xi=0)      # a pipelined step: the form an epoch's full batches take
        torch.cuda.synchronize()
        loss_ref, grads_ref = _autograd_step(before, x, (tr.layer1_output(bf) > 0, bf.r2 > 0))
        got = tr.out[0].item()
        print(f"{opt} F={F} m={m} C={C} step {it}: loss {got:.7f} autograd {loss_ref:.7f}")
        assert abs(got - loss_ref) <= 2e-4 * abs(loss_ref), (it, got, loss_ref)
        for i, n_ in enumerate(NAMES):
            have, want = tr.gradient(i), grads_ref[i]
            err = (have - want).abs().max().item()
            print(f"  {n_}: max gradient error {err / want.abs().max().item():.2e} of the gradient's max")
            assert err <= 2e-3 * want.abs().max().item() + 1e-12, (it, n_, err, want.abs().max().item())
        # the trainer's own gradients through torch's optimizer from the same start: 1e-5 of the tensor's largest magnitude
        for p, i in zip(shadow, range(6)):
            p.grad = tr.gradient(i).clone()
        sopt.step()
        for n_, p, want in zip(NAMES, tr.params, shadow):
            err = (p.detach() - want.detach()).abs().max().item()
            print(f"  {n_}: max parameter error {err / want.detach().abs().max().item():.2e} of the tensor's max")
            assert err <= 1e-5 * want.detach().abs().max().item(), (it, n_, err)
    assert tr.step_count() == 3


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("F", [256, 1024, 4096])
@pytest.mark.parametrize("m", [512, 1024])
@pytest.mark.parametrize("C", [5, 20, 48, 200])
def test_three_full_batch_steps_match_autograd_and_torch_optim(dev, opt, F, m, C):
    _three_steps(dev, opt, F, m, C)


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("F,m,C", [(4096, 1024, 20), (1024, 512, 200)])
def test_three_steps_with_hyperparameters_a_scheduler_changed(dev, opt, F, m, C):
    _three_steps(dev, opt, F, m, C, change_after_first=True)


# ------------------------------------------------------------------------------------------------ 3. dropout on
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("F,m,C", [(4096, 1024, 20), (1024, 512, 200), (256, 512, 5)])
def test_dropout_step_matches_autograd_with_the_trainers_masks(dev, opt, F, m, C):
    """Voter 3's first step.  The mask after layer 1 is drawn with NetLinear's existing layer id and stream (idl_relu_dropout_fwd, layer 1,
    the trainer's seed and counter) and must be the host restatement's (linear_dropout_ref.masks); the classifier's IS the restatement's,
    which the step's own masked latent must follow (a kept, active unit is one whose output is > 0)."""
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.fused import _p, _stream
    net = _random_net(F, C, dev, seed=3)
    st = _store(F, dev)
    x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    tr = _trainer(net, opt)
    tr.begin_voter(3)
    assert tr.ctl[0].item() == 3 << 24
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    ones = torch.ones((m, 512), device=dev)
    _lib.check(_lib.lib.idl_relu_dropout_fwd(_p(ones), ones.numel(), 1, tr.seed, _p(tr.ctl), 1, _stream()))
    mask1 = ones > 0
    assert abs(mask1.float().mean().item() - 0.5) < 0.01
    # ... and both masks are the host restatement's of (seed, voter 3's first step word): the latent's is passed as restated, so the step's
    # own r2 > 0 must be (h > 0) & that mask (_same_branch)
    want1, mask2 = (torch.from_numpy(a).to(dev) for a in restated_masks(tr.seed, 3 << 24, m))
    assert torch.equal(mask1, want1)
    p0 = copy.deepcopy(net)
    bf = tr.buffers(m)
    bf.xs[0].copy_(x)
    tr.step_on_batch(bf, train=True, batch_advance=m // 2, next_from=st, xi=0)
    torch.cuda.synchronize()
    loss_ref, grads_ref = _autograd_step(p0, x, (tr.layer1_output(bf) > 0, bf.r2 > 0), masks=(mask1, mask2))
    got = tr.out[0].item()
    print(f"{opt} F={F} m={m} C={C}: loss {got:.7f} autograd with the trainer's masks {loss_ref:.7f}")
    assert abs(got - loss_ref) <= 2e-4 * abs(loss_ref), (got, loss_ref)
    for i, n_ in enumerate(NAMES):
        have, want = tr.gradient(i), grads_ref[i]
        err = (have - want).abs().max().item()
        print(f"  {n_}: max gradient error {err / want.abs().max().item():.2e} of the gradient's max")
        assert err <= 2e-3 * want.abs().max().item() + 1e-12, (n_, err, want.abs().max().item())
    shadow = [p.detach().clone().requires_grad_(True) for p in p0.parameters()]
    for p, i in zip(shadow, range(6)):
        p.grad = tr.gradient(i).clone()
    _optimizer(opt, shadow).step()
    for n_, p, want in zip(NAMES, tr.params, shadow):
        err = (p.detach() - want.detach()).abs().max().item()
        assert err <= 1e-5 * want.detach().abs().max().item(), (n_, err)


# ------------------------------------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("opt,C", [("SGD", 20), ("Adam", 20), ("Adam", 200)])
def test_epochs_replayed_from_the_graph_equal_eager_launches(dev, opt, C):
    """1560 pairs in batches of 128: 12 full batches and a partial last batch of 24, three epochs.  An epoch is 13 steps, so the second
    starts with the two step words in the other roles (2 eager steps, a second capture, one replay of 10) and the third replays the first
    one's graph (one replay of 10, 2 eager steps).  Parameters, state, step words, out and ctl bit-identical to eager launches."""
    import torch
    st = _Store(520, 3, 256, dev, seed=2)
    runs = []
    for use_graph in (True, False):
        net = _random_net(256, C, dev, seed=4)
        tr = _trainer(net, opt, seed=6)
        gen = torch.Generator(device=dev).manual_seed(123)
        losses = []
        for _ in range(3):
            total, nb = tr.run_epoch(st, 128, generator=gen, use_graph=use_graph)
            assert nb == 13
            losses.append(total.clone())
        torch.cuda.synchronize()
        assert len(tr._graphs) == (2 if use_graph else 0)
        assert getattr(tr, "n_captures", 0) == (2 if use_graph else 0)
        runs.append([p.detach().clone() for p in tr.params] + [v.clone() for v in tr.state_tensors()] + losses
                    + [tr.steps.clone(), tr.out.clone(), tr.ctl.clone()])
        assert tr.step_count() == 39 and tr.ctl.tolist() == [39, 1560]
        assert all(bool(torch.isfinite(t)) for t in losses)
        assert all(float(v.abs().sum()) > 0 for v in tr.state_tensors())
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_last_launch_assembles_the_next_batch_where_the_middle_launches_cannot(dev, opt):
    """Batches of 100 pairs (m = 200, not a multiple of 16): the middle launches carry no batch assembly, the offset moves mid-step and the
    new launch's gather blocks write the next batch into the x buffer.  After each of three pipelined steps that buffer equals what
    idl_gather_pairs_at assembles at the offset; then two epochs (15 full batches, a partial one of 60) graph against eager, bit for bit."""
    import torch
    st = _Store(520, 3, 256, dev, seed=3)
    tr = _trainer(_random_net(256, 20, dev, seed=4), opt, seed=6)
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    tr.ctl[1:2].zero_()
    bf = tr.buffers(200)
    tr._gather(st, bf)
    first = bf.x.clone()
    for i in range(3):
        tr.step_on_batch(bf, batch_advance=100, next_from=st, xi=i % 2)
        torch.cuda.synchronize()
        assert tr.ctl[1].item() == 100 * (i + 1)
        got = bf.x.clone()
        tr._gather(st, bf)                              # the same rows through the stand-alone gather
        torch.cuda.synchronize()
        assert torch.equal(got, bf.x) and not torch.equal(got, first)
    runs = []
    for use_graph in (True, False):
        tr = _trainer(_random_net(256, 20, dev, seed=4), opt, seed=6)
        gen = torch.Generator(device=dev).manual_seed(321)
        losses = []
        for _ in range(2):
            total, nb = tr.run_epoch(st, 100, generator=gen, use_graph=use_graph)
            assert nb == 16
            losses.append(total.clone())
        torch.cuda.synchronize()
        assert getattr(tr, "n_captures", 0) == (1 if use_graph else 0)
        assert tr.step_count() == 32 and tr.ctl.tolist() == [32, 1560] and all(bool(torch.isfinite(t)) for t in losses)
        runs.append([p.detach().clone() for p in tr.params] + [v.clone() for v in tr.state_tensors()] + losses + [tr.steps.clone(), tr.out.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. launches
def _kernel_names(step, n):
    import torch
    from torch.profiler import profile, ProfilerActivity
    for i in range(2):                                   # (warm: nothing lazily initialised inside the profile)
        step(i)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(n):
            step(i)
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def _pipelined(tr, st, m, dev):
    import torch
    tr._perm = torch.randperm(st.n_pairs, device=dev)
    tr.ctl[1:2].zero_()
    bf = tr.buffers(m)
    tr._gather(st, bf)
    return lambda i: tr.step_on_batch(bf, batch_advance=m // 2, next_from=st, xi=i % 2)


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_full_batch_step_launch_budget(dev, opt, monkeypatch):
    from idelucs_amd.fused import FusedLinearTrainer
    F, m = 4096, 1024
    st = _store(F, dev)
    tr = _trainer(_random_net(F, 20, dev), opt, seed=2)
    names = _kernel_names(_pipelined(tr, st, m, dev), 4)
    print(f"{opt} C = 20: {len(names) / 4:.1f} launches a step")
    assert not [n for n in names if "Cijk" in n], names
    assert 0 < len(names) <= 7 * 4, (len(names), names)
    for k in ("opt_step_kernel", "wgrad_q16", "l1_fwd_kernel"):
        assert sum(k in n for n in names) == 4, (k, names)
    # n_clusters = 200: no more launches and no more library products than the RMSprop trainer's general form at this shape
    tr = _trainer(_random_net(F, 200, dev), opt, seed=2)
    names = _kernel_names(_pipelined(tr, st, m, dev), 4)
    monkeypatch.setenv("IDELUCS_PLANES", "0")
    rms = FusedLinearTrainer(_random_net(F, 200, dev), 1e-3, 0.25, 2.8, seed=2)
    rms.begin_voter(0)
    assert rms._form(rms.buffers(m), st) == "general"
    rms_names = _kernel_names(_pipelined(rms, st, m, dev), 4)
    lib, rms_lib = sum("Cijk" in n for n in names), sum("Cijk" in n for n in rms_names)
    print(f"{opt} C = 200: {len(names) / 4:.1f} launches a step ({lib / 4:.1f} library products); RMSprop's general form {len(rms_names) / 4:.1f} ({rms_lib / 4:.1f})")
    assert len(names) <= len(rms_names) and lib <= rms_lib, (names, rms_names)
    assert sum("opt_step_kernel" in n for n in names) == 4, names


# ------------------------------------------------------------------------------------------------ 6. IID_model
def _args(**kw):
    a = {'sequence_file': os.path.join(DATA, "Influenza-A.fas"), 'GT_file': None, 'n_clusters': 5, 'k': 6, 'model_size': 'linear',
         'n_mimics': 3, 'batch_sz': 256, 'optimizer': 'Adam', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None,
         'n_epochs': 3, 'n_voters': 1, 'linear_step': 'native'}
    a.update(kw)
    return a


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_iid_model_native_linear_trains_and_predicts(dev, opt):
    import torch
    from idelucs_amd import models
    from idelucs_amd.fused_opt import FusedLinearOptTrainer
    m = models.IID_model(_args(optimizer=opt))
    assert m._use_linopt and not m._use_fused and not m._use_small
    m.build_dataloader()
    m.begin_voter(0)
    losses = [m.contrastive_training_epoch() for _ in range(3)]
    print(f"{opt}: epoch losses {losses}")
    assert isinstance(m._linopt, FusedLinearOptTrainer) and m._fused is None and m._small is None
    assert all(np.isfinite(losses)), losses
    if opt == "Adam":
        assert losses[2] < losses[0], losses
    y, p, lat = m.predict()
    assert y.dtype == np.int64 and y.shape == (949,) and p.dtype == np.float64 and p.shape == (949,)
    assert lat.dtype == np.float64 and lat.shape == (949, 64) and np.all(np.isfinite(lat))
    probs = m.calculate_probs()
    assert probs.dtype == np.float64 and probs.shape == (949, 5)
    snaps = []                                           # voter v is the same run whenever it trains; two voters differ
    for v in (1, 1, 2):
        m.begin_voter(v)
        for _ in range(2):
            m.contrastive_training_epoch()
        snaps.append([p.detach().clone() for p in m.net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[1]))
    assert not all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[2]))


@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_linear_without_the_key_stays_on_autograd(dev, opt, monkeypatch):
    from idelucs_amd import models, fused_opt

    def refuse(*a, **kw):
        raise AssertionError("a FusedLinearOptTrainer was built")
    monkeypatch.setattr(fused_opt.FusedLinearOptTrainer, "__init__", refuse)
    a = _args(k=4, optimizer=opt)
    del a['linear_step']
    for args in (a, _args(k=4, optimizer=opt, linear_step=None), _args(k=4, optimizer=opt, linear_step='autograd')):
        m = models.IID_model(args)
        assert m._use_linopt is False and m._use_fused is False
        m.build_dataloader()
        m.begin_voter(0)
        assert np.isfinite(m.contrastive_training_epoch())
        assert m._linopt is None
    # the key is ignored for RMSprop (its step is native already) and for model_size='small', whatever it holds
    for kw in (dict(optimizer='RMSprop'), dict(model_size='small', optimizer='RMSprop'), dict(model_size='small')):
        for val in ('native', 'fast'):
            m = models.IID_model(_args(k=4, linear_step=val, **{'optimizer': opt, **kw}))
            assert m._use_linopt is False
    m = models.IID_model(_args(k=4, optimizer='RMSprop', linear_step='native'))
    assert m._use_fused
    m = models.IID_model(_args(k=4, model_size='small', optimizer=opt, linear_step='native'))
    m.build_dataloader()
    m.begin_voter(0)
    assert np.isfinite(m.contrastive_training_epoch()) and m._linopt is None and m._small is None


@pytest.mark.parametrize("kw", [dict(linear_step='fast'), dict(n_clusters=257), dict(optimizer='SGD', linear_step='fast'),
                                dict(optimizer='SGD', n_clusters=257)])
def test_unsupported_native_configurations_raise(dev, kw):
    from idelucs_amd import models
    with pytest.raises(ValueError, match="linear_step"):
        models.IID_model(_args(k=4, **kw))


# ------------------------------------------------------------------------------------------------ 7. schedulers
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("sched", ["Plateau", "Triangle"])
def test_schedulers_drive_the_native_step_as_the_autograd_one(dev, opt, sched):
    from idelucs_amd import models

    def second(grp):
        return grp['momentum'] if opt == "SGD" else grp['betas'][0]
    traces = {}
    for mode in ("autograd", "native"):
        m = models.IID_model(_args(k=4, optimizer=opt, scheduler=sched, linear_step=mode))
        m.build_dataloader()
        m.begin_voter(0)
        lr, mom = [], []
        for _ in range(6):
            m.contrastive_training_epoch()
            lr.append(m.optimizer.param_groups[0]['lr'])
            mom.append(second(m.optimizer.param_groups[0]))
        if m._linopt is not None:                      # the values the next epoch's steps run with
            m.enqueue_epoch()
            grp = m.optimizer.param_groups[0]
            h = m._linopt.hyper64.tolist()
            want = ([grp['lr'], grp['momentum'], 0.0, 0.0, grp['weight_decay']] if opt == "SGD"
                    else [grp['lr'], grp['betas'][0], grp['betas'][1], grp['eps'], grp['weight_decay']])
            assert grp['lr'] == lr[-1] and second(grp) == mom[-1]
            for a, b in zip(h, want):
                assert abs(a - b) <= 1e-6 * abs(b), (h, want)
        traces[mode] = (lr, mom)
    print(f"{opt} {sched}: lr {traces['native'][0]} second {traces['native'][1]}")
    assert traces["native"][0] == traces["autograd"][0], traces
    if sched == "Triangle":
        assert traces["native"][1] == traces["autograd"][1], traces
        assert len(set(traces["native"][1])) > 1, traces     # (CyclicLR does cycle momentum / beta1)


# ------------------------------------------------------------------------------------------------ 8. carried state
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
def test_voter_state_carry_keeps_the_state_and_the_step_count(dev, opt, monkeypatch):
    import torch
    from idelucs_amd import models
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "carry")
    m = models.IID_model(_args(k=4, optimizer=opt))
    m.build_dataloader()
    m.begin_voter(0)
    m.contrastive_training_epoch()
    tr = m._linopt
    before = [v.clone() for v in tr.state_tensors()]
    count = tr.step_count()
    assert count == 12 and all(float(v.abs().sum()) > 0 for v in before)      # 2847 pairs in batches of 256: 11 full + 1 partial
    m.begin_voter(1)
    assert all(torch.equal(a, b) for a, b in zip(before, tr.state_tensors())) and tr.step_count() == count
    m.contrastive_training_epoch()
    assert tr.step_count() == 2 * count
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "fresh")
    m.begin_voter(2)
    assert all(float(v.abs().sum()) == 0.0 for v in tr.state_tensors()) and tr.step_count() == 0 and tr.steps.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 9. quality
def test_native_adam_quality_matches_autograd(dev):
    """Influenza-A, k = 6, 5 clusters, 10 epochs, batch 256, Adam, the same 8 seeds through both step forms: the native form's mean ACC is
    not below the autograd form's by more than 3 standard errors of the difference of the two means (the rule of
    test_end_to_end_quality_anchor), computed from the two samples."""
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
            m = models.IID_model(_args(k=6, n_epochs=10, linear_step=mode, seed=seed))
            m.build_dataloader()
            m.begin_voter(0)
            for _ in range(10):
                m.contrastive_training_epoch()
            acc[mode].append(idelucs_amd.cluster_acc(gt, m.predict()[0])[1])
    a, n = np.array(acc["autograd"]), np.array(acc["native"])
    se = float(np.sqrt(a.var(ddof=1) / len(a) + n.var(ddof=1) / len(n)))
    print("ACC over 8 seeds: autograd", np.round(a, 4), round(float(a.mean()), 4), "| native", np.round(n, 4), round(float(n.mean()), 4),
          "| 3 standard errors of the difference", round(3 * se, 4))
    assert n.mean() >= a.mean() - 3 * se, (acc, se)


# ------------------------------------------------------------------------------------------------ 10. CLI
def test_cli_linear_native_writes_reference_outputs(tmp_path, monkeypatch, capsys):
    import pandas as pd
    from idelucs_amd.__main__ import main
    monkeypatch.chdir(tmp_path)
    out_dir = main(["--sequence_file", os.path.join(DATA, "influenza_64.fas"), "--n_clusters", "5", "--n_epochs", "3", "--n_voters", "2",
                    "--batch_sz", "64", "--k", "6", "--optimizer", "Adam", "--linear_step", "native"])
    assert "linear_step \t -> native" in capsys.readouterr().out
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 64
    row = open(tmp_path / "ALL_RESULTS.tsv").read().splitlines()[-1]
    assert "'linear_step': 'native'" in row
