"""GPU tests of the native training step of model_size='small' (idelucs_amd/fused_small.py + csrc/small_step.hip): the first step
against the reference's goldens, full-batch steps against torch autograd (dropout off and on), the dropout streams, graph replay
against eager launches, the launch budget, IID_model / CLI integration and the quality of a 10-epoch run against the autograd form."""
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

NAMES = ["layers.0.weight", "layers.0.bias", "layers.3.weight", "layers.3.bias", "instance.weight", "instance.bias",
         "classifier.1.weight", "classifier.1.bias"]


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda")


def _trainer(net, seed=5):
    from idelucs_amd.fused_small import FusedSmallTrainer
    tr = FusedSmallTrainer(net, lr=1e-3, weight=0.25, lamb=2.8, seed=seed)
    tr.keep_grads = True
    tr.begin_voter(0)
    return tr


def _random_net(F, C, dev, seed=0):
    import torch
    from idelucs_amd.PytorchUtils import myNet
    from idelucs_amd.models import weights_init
    torch.manual_seed(seed)
    net = myNet(F, C)
    net.apply(weights_init)
    return net.to(dev)


def _autograd_step(net, x, masks=None, float64_grads=False):
    """The reference step (models.py:117-133) written out on a float64 copy of net: dropout off, or the given keep masks x 2 in place
    of nn.Dropout.  -> (loss, [8 gradients as float32]).  (float64: the bars below then measure the step's own rounding, not the sum
    of two fp32 implementations'.)  float64_grads: the gradients as autograd left them (tests/test_small_reference.py)."""
    import copy
    import torch
    import torch.nn.functional as Fn
    from idelucs_amd.LossFunctions import IID_loss
    ref = copy.deepcopy(net).double()
    x = x.double()
    l1, l2, li, lc = ref.layers[0], ref.layers[3], ref.instance, ref.classifier[1]
    ps = [l1.weight, l1.bias, l2.weight, l2.bias, li.weight, li.bias, lc.weight, lc.bias]
    a1 = torch.relu(Fn.linear(x, l1.weight, l1.bias))
    if masks is not None:
        a1 = a1 * masks[0].double() * 2.0
    a2 = Fn.leaky_relu(Fn.linear(a1, l2.weight, l2.bias), 0.01)
    h = Fn.linear(a2, li.weight, li.bias)
    d2 = a2 * masks[1].double() * 2.0 if masks is not None else a2
    z = torch.softmax(Fn.linear(d2, lc.weight, lc.bias), dim=1)
    b = x.shape[0] // 2
    # info_nce_loss (LossFunctions.py:65-98) without its cast to float32
    f = Fn.normalize(h, dim=1)
    s = (f @ f.t()) / 0.85
    r = torch.arange(2 * b, device=s.device)
    pos = s[r, (r + b) % (2 * b)]
    s = s.masked_fill(r.unsqueeze(0) == r.unsqueeze(1), float("-inf"))
    nce = (torch.logsumexp(s, dim=1) - pos).mean()
    loss = 0.75 * nce + 0.25 * IID_loss(z[:b], z[b:], lamb=2.8)
    loss.backward()
    return float(loss.item()), [(p.grad.detach() if float64_grads else p.grad.detach().float()).clone() for p in ps]


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
def test_first_step_matches_reference_nets_small(dev):
    """myNet(10, 7), m = 18 (a K tail of 10 and an m that is not a multiple of 32), dropout off: the bars of
    test_fused_step_matches_reference."""
    import torch
    from idelucs_amd.PytorchUtils import myNet
    g = np.load(os.path.join(GOLDEN, "nets.npz"))
    net = myNet(10, 7)
    net.load_state_dict({k[len("small.w."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("small.w.")})
    net = net.to(dev)
    tr = _trainer(net)
    bf = tr.buffers(18)
    bf.x.copy_(torch.cat([torch.from_numpy(g["small.x1"]), torch.from_numpy(g["small.x2"])]).to(dev))
    tr.step_on_batch(bf, train=False)
    torch.cuda.synchronize()
    ref = float(g["small.step0.loss"])
    assert abs(tr.out[0].item() - ref) <= 2e-4 * abs(ref), (tr.out[0].item(), ref)
    for i, n_ in enumerate(NAMES):
        np.testing.assert_allclose(tr.gradient(i).cpu().numpy(), g[f"small.step0.g.{n_}"], rtol=2e-3, atol=2e-6, err_msg=n_)
    for n_, p in zip(NAMES, tr.params):
        bad = ~np.isclose(p.detach().cpu().numpy(), g[f"small.step0.p.{n_}"], rtol=1e-3, atol=1e-6)
        assert bad.mean() < 2e-3, (n_, bad.mean())
    tr.step_on_batch(bf, train=False)
    ref1 = float(g["small.step1.loss"])
    assert abs(tr.out[0].item() - ref1) <= 5e-4 * abs(ref1), (tr.out[0].item(), ref1)
    assert abs(tr.out[1].item() - (tr.out[0].item() + ref)) < 1e-3
    assert tr.ctl.tolist() == [2, 0]


def test_first_step_matches_reference_small_k5(dev):
    """myNet(512, 5) on the reference's canonical 5-mer rows of 32 Influenza records (m = 32), dropout off."""
    import torch
    from idelucs_amd.PytorchUtils import myNet
    g = np.load(os.path.join(GOLDEN, "small_k5.npz"))
    net = myNet(512, 5)
    net.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")})
    net = net.to(dev)
    tr = _trainer(net)
    bf = tr.buffers(32)
    bf.x.copy_(torch.from_numpy(g["x"]).to(dev))
    tr.step_on_batch(bf, train=False)
    torch.cuda.synchronize()
    ref = float(g["loss"])
    assert abs(tr.out[0].item() - ref) <= 2e-4 * abs(ref), (tr.out[0].item(), ref)
    for i, n_ in enumerate(NAMES):
        got = tr.gradient(i).cpu().numpy()
        if got.ndim == 2 and got.shape[0] >= 128:        # (the fixture keeps every 8th row of the two big weight gradients)
            got = got[::8]
        np.testing.assert_allclose(got, g[f"g.{n_}"], rtol=2e-3, atol=2e-6, err_msg=n_)
    for n_, p in zip(NAMES, tr.params):
        if f"p.{n_}" in g.files:
            bad = ~np.isclose(p.detach().cpu().numpy(), g[f"p.{n_}"], rtol=1e-3, atol=1e-6)
            assert bad.mean() < 2e-3, (n_, bad.mean())


# ------------------------------------------------------------------------------------------------ 2. against torch autograd
def _check_against_autograd(tr, p0, loss_ref, grads_ref):
    import torch
    assert abs(tr.out[0].item() - loss_ref) <= 2e-4 * abs(loss_ref), (tr.out[0].item(), loss_ref)
    for i, n_ in enumerate(NAMES):
        got, want = tr.gradient(i), grads_ref[i]
        err = (got - want).abs().max().item()
        print(f"{n_}: max error {err:.2e}, the gradient's max {want.abs().max().item():.2e}")
        assert err <= 2e-3 * want.abs().max().item() + 1e-12, (n_, err, want.abs().max().item())
    # RMSprop on the trainer's own gradients (torch.optim.RMSprop from the same starting parameters): rel 1e-5
    ps = [p.clone().requires_grad_(True) for p in p0]
    for p, gr in zip(ps, tr.grads):
        p.grad = gr.clone()
    torch.optim.RMSprop(ps, lr=1e-3, weight_decay=0.01).step()
    for n_, p, want in zip(NAMES, tr.params, ps):
        err = (p.detach() - want.detach()).abs().max().item()
        assert err <= 1e-5 * want.detach().abs().max().item(), (n_, err)


@pytest.mark.parametrize("F", [136, 512, 2080, 8192])
@pytest.mark.parametrize("m", [512, 1024])
@pytest.mark.parametrize("C", [5, 20, 48, 200])
def test_full_batch_step_matches_autograd(dev, F, m, C):
    import torch
    net = _random_net(F, C, dev, seed=F + m + C)
    p0 = [p.detach().clone() for p in net.parameters()]
    x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(F * 7 + m + C))
    loss_ref, grads_ref = _autograd_step(net, x)
    tr = _trainer(net)
    bf = tr.buffers(m)
    bf.x.copy_(x)
    tr.step_on_batch(bf, train=False)
    torch.cuda.synchronize()
    _check_against_autograd(tr, p0, loss_ref, grads_ref)


# ------------------------------------------------------------------------------------------------ 3. dropout on
@pytest.mark.parametrize("F,m,C", [(2080, 1024, 20), (512, 512, 200), (136, 512, 5)])
def test_dropout_step_matches_autograd_with_the_trainers_masks(dev, F, m, C):
    import torch
    net = _random_net(F, C, dev, seed=3)
    p0 = [p.detach().clone() for p in net.parameters()]
    x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    tr = _trainer(net)
    tr.begin_voter(3)
    masks = tr.dropout_masks(int(tr.ctl[0].item()), m)
    loss_ref, grads_ref = _autograd_step(net, x, masks=masks)
    bf = tr.buffers(m)
    bf.x.copy_(x)
    tr.step_on_batch(bf, train=True)
    torch.cuda.synchronize()
    _check_against_autograd(tr, p0, loss_ref, grads_ref)


# ------------------------------------------------------------------------------------------------ 3b. the partial last batch
# An epoch's last batch is any even m from 2 up.  m % 32 != 0 takes the unfused InfoNCE route (one part of G), and with it every
# n_clusters > 48 reads dP0 and the partner's z from global memory in the middle backward; m = 96 keeps the fused InfoNCE kernels at
# a size no full batch has.  F alternates over the (m, C) grid so that every m and every C meets both widths.
RAGGED_M, RAGGED_C, RAGGED_F = [2, 18, 34, 62, 96, 440], [5, 49, 130, 201, 256], [136, 512]


def _crossed_a_kink(p0, x, masks, bf):
    """True when the step's float32 forward put a hidden unit on the other side of 0 than float64 does.  ReLU' and LeakyReLU' jump
    there, so that unit then takes the other slope in the backward, and with a handful of rows one unit is a large share of its
    rows of dW1, dW2: not an error of the step, and not what a comparison with autograd can judge (tests/test_gpu_small_stages.py
    takes every sign from the kernel's own activations and has no such case).  A sign may differ only where the float64
    pre-activation is within a float32 forward's rounding of 0 -- the product bound of small_ref.py, (K + 16) 2^-23 sum |a||b|, plus
    layer 1's own error carried through |W2|; anywhere else it is an error, and is raised as one."""
    import torch
    x, W1, b1, W2, b2 = (t.detach().double() for t in (x, *p0[:4]))      # (p0: the parameters before the step, in myNet's order)
    u = 2.0 ** -23
    keep = masks[0].double() * 2.0 if masks is not None else torch.ones((x.shape[0], W1.shape[0]), dtype=torch.float64, device=x.device)
    v1 = x @ W1.t() + b1
    e1 = (x.shape[1] + 16) * u * (x.abs() @ W1.abs().t() + b1.abs())
    a1 = torch.relu(v1) * keep
    v2 = a1 @ W2.t() + b2
    e2 = (W2.shape[1] + 16) * u * (a1.abs() @ W2.abs().t() + b2.abs()) + (e1 * keep) @ W2.abs().t()
    off1, off2 = (bf.a1 > 0) != (a1 > 0), (bf.a2 > 0) != (v2 > 0)
    assert bool((v1.abs()[off1] <= e1[off1]).all()) and bool((v2.abs()[off2] <= e2[off2]).all())
    return bool(off1.any()) or bool(off2.any())


def _ragged_step(dev, m, C, F, dropout):
    import torch
    for draw in range(4):                                # (the first draw but for m = 2, C = 201, F = 512 with dropout: one unit of
        #                                                  layer 2 lies 1.3e-6 from 0 there and the float32 forward lands beyond it)
        net = _random_net(F, C, dev, seed=F + m + C)
        p0 = [p.detach().clone() for p in net.parameters()]
        tr = _trainer(net)
        tr.begin_voter(2)
        masks = tr.dropout_masks(int(tr.ctl[0].item()), m) if dropout else None
        x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(F * 7 + m + C + 1000 * draw))
        loss_ref, grads_ref = _autograd_step(net, x, masks=masks)
        bf = tr.buffers(m)
        bf.x.copy_(x)
        tr.step_on_batch(bf, train=dropout)
        torch.cuda.synchronize()
        if not _crossed_a_kink(p0, x, masks, bf):
            return tr, bf, p0, loss_ref, grads_ref
        print(f"draw {draw}: a hidden unit crossed 0 in float32, next draw")
    raise AssertionError("four draws of x in a row put a hidden unit across 0")


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("m,C,F", [(m, C, RAGGED_F[(i + j) % 2]) for i, m in enumerate(RAGGED_M) for j, C in enumerate(RAGGED_C)])
def test_partial_batch_step_matches_autograd(dev, m, C, F, dropout):
    """step_on_batch against float64 autograd at the shapes of a partial last batch, dropout off and on with the trainer's own masks:
    the bars of the full-batch tests (the sharp, per-stage bars are tests/test_gpu_small_stages.py's)."""
    import torch
    tr, bf, p0, loss_ref, grads_ref = _ragged_step(dev, m, C, F, dropout)
    assert bf.nce_fused == (m % 32 == 0) and (bf.dzs is not None) == (48 < C <= 200)
    for t in [tr.out] + tr.grads + [p.detach() for p in tr.params] + tr.square_avg:
        assert bool(torch.isfinite(t).all())
    _check_against_autograd(tr, p0, loss_ref, grads_ref)
    assert tr.ctl.tolist() == [(2 << 24) + 1, 0]
    if m == 2:
        _check_one_pair(tr, p0, grads_ref)


def _check_one_pair(tr, p0, grads_ref):
    """m = 2 is one pair: each row's only other row is its positive, so InfoNCE is 0 and its gradient (the instance head's, which nothing
    else reaches) exactly 0; and the parameters are those of RMSprop fed the reference's gradients.

    The parameter bar.  With R = tests/small_ref.py and the trainer's float32 hyperparameters, |p - R.rmsprop(p0, 0, g_ref)| <=
    |p - R.rmsprop(p0, 0, g)| + |R.rmsprop(p0, 0, g) - R.rmsprop(p0, 0, g_ref)|, g the step's own gradient.  The first term is one float32
    update: R.rmsprop_bound.  The second: the first update moves p by lr g' / (sqrt(1 - alpha) |g'| + eps), g' = g + wd p, a function of
    g' whose slope eps / (sqrt(1 - alpha) |g'| + eps)^2 is largest at the smaller |g'| where the two agree in sign and at most 1 / eps
    where they do not: lr slope |g - g_ref|, with the two gradients this test has just compared."""
    import small_ref as R
    # (the loss itself is lse - s_partner / T of two sums each rounded a few times at |s| / T <= 1 / 0.85: 0 to 4 * 2^-23 / 0.85)
    print(f"InfoNCE of one pair: {tr.out[2].item():.3e}")
    assert abs(tr.out[2].item()) <= 4 * 2.0 ** -23 / 0.85
    assert float(tr.gradient(4).abs().max()) == 0.0 and float(tr.gradient(5).abs().max()) == 0.0
    assert float(grads_ref[4].abs().max()) == 0.0 and float(grads_ref[5].abs().max()) == 0.0
    h = R.f64(tr.hyper)
    for n_, p, start, g_ref, g_got in zip(NAMES, tr.params, p0, grads_ref, tr.grads):
        start, g_ref, g_got = R.f64(start), R.f64(g_ref), R.f64(g_got)
        zero = np.zeros_like(start)
        want, own = R.rmsprop(start, zero, g_ref, h)[0], R.rmsprop_bound(start, zero, g_got, h)[0]
        gi_ref, gi_got = g_ref + h[3] * start, g_got + h[3] * start
        low = np.where(gi_ref * gi_got > 0, np.minimum(np.abs(gi_ref), np.abs(gi_got)), 0.0)
        bar = own + h[0] * h[2] / (np.sqrt(h[4]) * low + h[2]) ** 2 * np.abs(gi_got - gi_ref)
        worst = (np.abs(R.f64(p) - want) / bar).max()
        print(f"{n_}: parameter error / bar {worst:.3f}")
        assert worst <= 1.0, (n_, worst)


def test_full_batch_step_at_256_clusters_matches_autograd(dev):
    """C = 256 (above the 200 the fine-grained mode uses, the most the kernels take), m = 512: a full batch on the fused InfoNCE
    kernels with dP0 read from global memory in the middle backward."""
    import torch
    tr, bf, p0, loss_ref, grads_ref = _ragged_step(dev, 512, 256, 136, False)
    assert bf.nce_fused and bf.dzs is None
    _check_against_autograd(tr, p0, loss_ref, grads_ref)


def test_dropout_mask_statistics(dev):
    from idelucs_amd.fused_small import FusedSmallTrainer
    net = _random_net(2080, 20, dev)
    tr = _trainer(net, seed=17)
    m = 1024
    a1, a2 = tr.dropout_masks(0, m)
    for mk in (a1, a2):
        assert abs(mk.float().mean().item() - 0.5) <= 0.01
    b1, b2 = tr.dropout_masks(0, m)
    assert bool((a1 == b1).all()) and bool((a2 == b2).all())            # same (seed, voter, step): same masks
    for step in (1, 1 << 24):                                            # the next step; voter 1's first step
        c1, c2 = tr.dropout_masks(step, m)
        for x, y in ((a1, c1), (a2, c2)):
            diff = (x != y).float().mean().item()
            assert 0.45 <= diff <= 0.55, (step, diff)
    other = FusedSmallTrainer(net, lr=1e-3, weight=0.25, lamb=2.8, seed=18)    # another seed: other masks
    d1, _ = other.dropout_masks(0, m)
    assert 0.45 <= (a1 != d1).float().mean().item() <= 0.55


# ------------------------------------------------------------------------------------------------ 4. graph replay
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


def test_epoch_replayed_from_the_graph_equals_eager_launches(dev):
    """n = 1500 pairs in batches of 256: full batches replayed from the captured graph, a partial last batch of 220; two epochs
    (the second replays the cached graph).  Parameters, running averages and losses bit-identical to eager launches."""
    import torch
    st = _Store(500, 3, 512, dev, seed=2)
    runs = []
    for use_graph in (True, False):
        net = _random_net(512, 20, dev, seed=4)
        tr = _trainer(net, seed=6)
        tr.keep_grads = False
        gen = torch.Generator(device=dev).manual_seed(123)
        losses = []
        for _ in range(2):
            total, nb = tr.run_epoch(st, 256, generator=gen, use_graph=use_graph)
            assert nb == 6
            losses.append(total.clone())
        torch.cuda.synchronize()
        assert len(tr._graphs) == (1 if use_graph else 0)
        runs.append(([p.detach().clone() for p in tr.params], [v.clone() for v in tr.square_avg], losses, tr.out.clone(), tr.ctl.clone()))
    (pa, va, la, oa, ca), (pb, vb, lb, ob, cb) = runs
    for x, y in zip(pa + va + la + [oa, ca], pb + vb + lb + [ob, cb]):
        assert torch.equal(x, y)
    assert ca.tolist() == [12, 1280]                   # (the partial batch does not advance the offset)
    assert all(bool(torch.isfinite(t)) for t in la)


# ------------------------------------------------------------------------------------------------ 5. launches
@pytest.mark.parametrize("C", [20, 200])
def test_full_batch_step_launch_budget(dev, C):
    import torch
    from torch.profiler import profile, ProfilerActivity
    F, B = 2080, 512
    st = _Store(2048, 3, F, dev, seed=1)
    tr = _trainer(_random_net(F, C, dev), seed=2)
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
    print(f"C = {C}: {len(names) / 4:.1f} launches a step")
    assert not [n for n in names if "Cijk" in n], names
    assert 0 < len(names) <= 8 * 4, (len(names), names)
    for k in ("small_l1_fwd_kernel", "small_mid_fwd_kernel", "small_mid_bwd_kernel", "small_wgrad_rms_kernel"):
        assert sum(k in n for n in names) == 4, (k, names)


# ------------------------------------------------------------------------------------------------ 6. IID_model
def _args(**kw):
    a = {'sequence_file': os.path.join(DATA, "Influenza-A.fas"), 'GT_file': None, 'n_clusters': 5, 'k': 6, 'model_size': 'small',
         'n_mimics': 3, 'batch_sz': 256, 'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None,
         'n_epochs': 3, 'n_voters': 1, 'small_step': 'native'}
    a.update(kw)
    return a


@pytest.mark.parametrize("k", [4, 5, 6])
def test_iid_model_native_small_trains_and_predicts(dev, k):
    import torch
    from idelucs_amd import models
    from idelucs_amd.fused_small import FusedSmallTrainer
    m = models.IID_model(_args(k=k))
    m.build_dataloader()
    m.begin_voter(0)
    losses = [m.contrastive_training_epoch() for _ in range(3)]
    assert isinstance(m._small, FusedSmallTrainer) and m._fused is None
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    y, p, lat = m.predict()
    assert y.dtype == np.int64 and y.shape == (949,) and p.dtype == np.float64 and p.shape == (949,)
    assert lat.dtype == np.float64 and lat.shape == (949, 64) and np.all(np.isfinite(lat))
    probs = m.calculate_probs()
    assert probs.dtype == np.float64 and probs.shape == (949, 5)
    # voter v is the same run whenever it trains; two voters differ
    snaps = []
    for v in (1, 1, 2):
        m.begin_voter(v)
        for _ in range(2):
            m.contrastive_training_epoch()
        snaps.append([p.detach().clone() for p in m.net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[1]))
    assert not all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[2]))


@pytest.mark.parametrize("sched", ["Plateau", "Triangle"])
def test_schedulers_drive_the_native_step_as_the_autograd_one(dev, sched):
    from idelucs_amd import models
    traces = {}
    for mode in ("autograd", "native"):
        m = models.IID_model(_args(k=4, scheduler=sched, small_step=mode))
        m.build_dataloader()
        m.begin_voter(0)
        tr = []
        for _ in range(6):
            m.contrastive_training_epoch()
            tr.append(m.optimizer.param_groups[0]['lr'])
        if m._small is not None:                       # the rate the next epoch's steps run with
            m.enqueue_epoch()
            assert abs(m._small.hyper[0].item() - tr[-1]) <= 1e-6 * tr[-1]
        traces[mode] = tr
    assert traces["native"] == traces["autograd"], traces


def test_voter_state_carry_keeps_the_running_averages(dev, monkeypatch):
    import torch
    from idelucs_amd import models
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "carry")
    m = models.IID_model(_args(k=4))
    m.build_dataloader()
    m.begin_voter(0)
    m.contrastive_training_epoch()
    before = [v.clone() for v in m._small.square_avg]
    m.begin_voter(1)
    assert all(torch.equal(a, b) for a, b in zip(before, m._small.square_avg))
    monkeypatch.setenv("IDELUCS_VOTER_STATE", "fresh")
    m.begin_voter(2)
    assert all(float(v.abs().sum()) == 0.0 for v in m._small.square_avg)


def test_small_without_the_key_stays_on_autograd(dev, monkeypatch):
    from idelucs_amd import models, fused_small

    def refuse(*a, **kw):
        raise AssertionError("a FusedSmallTrainer was built")
    monkeypatch.setattr(fused_small.FusedSmallTrainer, "__init__", refuse)
    a = _args(k=4)
    del a['small_step']
    for args in (a, _args(k=4, small_step=None), _args(k=4, small_step='autograd')):
        m = models.IID_model(args)
        assert m._use_small is False and m._use_fused is False
        m.build_dataloader()
        m.begin_voter(0)
        assert np.isfinite(m.contrastive_training_epoch())
        assert m._small is None
    m = models.IID_model(_args(k=4, model_size='linear', small_step='native'))      # the key is ignored for the linear model
    assert m._use_small is False


@pytest.mark.parametrize("kw", [dict(optimizer='SGD'), dict(optimizer='Adam'), dict(n_clusters=257), dict(batch_sz=1025),
                                dict(small_step='fast')])
def test_unsupported_native_configurations_raise(dev, kw):
    from idelucs_amd import models
    with pytest.raises(ValueError, match="small_step"):
        models.IID_model(_args(k=4, **kw))


# ------------------------------------------------------------------------------------------------ 7. quality
def test_native_small_quality_matches_autograd(dev):
    """Influenza-A, k = 6, 5 clusters, 10 epochs, batch 256, the same 8 seeds through both step forms: the native form's mean ACC is
    at least the autograd form's - 0.03."""
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
            m = models.IID_model(_args(k=6, n_epochs=10, small_step=mode, seed=seed))
            m.build_dataloader()
            m.begin_voter(0)
            for _ in range(10):
                m.contrastive_training_epoch()
            acc[mode].append(idelucs_amd.cluster_acc(gt, m.predict()[0])[1])
    print("ACC over 8 seeds: autograd", np.round(acc["autograd"], 4), np.mean(acc["autograd"]),
          "| native", np.round(acc["native"], 4), np.mean(acc["native"]))
    assert np.mean(acc["native"]) >= np.mean(acc["autograd"]) - 0.03, acc


# ------------------------------------------------------------------------------------------------ 8. CLI
def test_cli_small_native_writes_reference_outputs(tmp_path, monkeypatch, capsys):
    import pandas as pd
    from idelucs_amd.__main__ import main
    monkeypatch.chdir(tmp_path)
    out_dir = main(["--sequence_file", os.path.join(DATA, "influenza_64.fas"), "--n_clusters", "5", "--n_epochs", "3", "--n_voters", "2",
                    "--batch_sz", "64", "--k", "6", "--model_size", "small", "--small_step", "native"])
    assert "small_step \t -> native" in capsys.readouterr().out
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 64
    row = open(tmp_path / "ALL_RESULTS.tsv").read().splitlines()[-1]
    assert "'small_step': 'native'" in row
