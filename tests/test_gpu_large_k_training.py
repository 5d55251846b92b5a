"""GPU tests of everything behind the vectoriser at the feature widths of k = 8 and 9 (F = 65 536 and 262 144; model_size='small':
32 896): the scaler, the gather and the batch assembly riding in the step's middle launches; one training step of NetLinear and of
myNet against float64 autograd; graph replay; IID_model and the CLI end to end."""
import copy
import os
import random

import numpy as np
import pytest

from conftest import DATA, GOLDEN
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F8, F9 = 4 ** 8, 4 ** 9


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------ scaler, gather, riding assembly
@pytest.mark.parametrize("n", [3, 300])
def test_scaler_and_gather_vs_oracle_at_k8_width(dev, n):
    """test_scaler_and_gather_vs_oracle's requirements at f = 65 536."""
    import torch
    from idelucs_amd import _lib, utils as U
    from idelucs_amd.utils import _ptr, _stream_ptr
    rng = np.random.default_rng(9 + n)
    f = F8
    x32 = (rng.random((n, f)) * 1e-3).astype(np.float32)
    x32[:, 0] = 0.25                                   # a zero-variance column -> scale 1
    mean, scale = U.col_stats(torch.from_numpy(x32).to(dev))
    m_ref, s_ref = O.scaler_fit(x32)
    np.testing.assert_allclose(mean.cpu().numpy(), m_ref, rtol=1e-13, atol=0)
    np.testing.assert_allclose(scale.cpu().numpy(), s_ref, rtol=1e-9, atol=0)
    assert scale[0].item() == 1.0
    dm, ds = torch.from_numpy(m_ref).to(dev), torch.from_numpy(s_ref).to(dev)
    y = U.standardise(torch.from_numpy(x32).to(dev), dm, ds).cpu().numpy()
    assert np.array_equal(y, O.scaler_transform(x32, m_ref, s_ref))
    x64 = x32.astype(np.float64) * 1.0000001
    m64, s64 = O.scaler_fit(x64)
    y = U.standardise(torch.from_numpy(x64).to(dev), torch.from_numpy(m64).to(dev), torch.from_numpy(s64).to(dev)).cpu().numpy()
    assert np.array_equal(y, O.scaler_transform(x64, m64, s64).astype(np.float32))
    # gather_pairs == standardise + the reference's pair layout
    P = 4
    feats = np.concatenate([x32[None], (rng.random((P - 1, n, f)) * 1e-3).astype(np.float32)])
    st = U.FeatureStore(None, None, torch.from_numpy(feats).to(dev), dm, ds, 8, False)
    b = min(70, (P - 1) * n)
    idx = rng.permutation((P - 1) * n)[:b].astype(np.int64)
    y = st.gather_pairs(torch.from_numpy(idx).to(dev)).cpu().numpy()
    want_true = O.scaler_transform(feats[0][idx % n], m_ref, s_ref)
    want_mod = O.scaler_transform(feats[1 + idx // n, idx % n], m_ref, s_ref)
    assert np.array_equal(y[:b], want_true) and np.array_equal(y[b:], want_mod)
    y2 = torch.empty_like(torch.from_numpy(y)).to(dev)
    didx = torch.from_numpy(idx).to(dev)
    _lib.check(_lib.lib.idl_gather_pairs_at(_ptr(st.feats), st.n, st.f, st.n * st.f, _ptr(didx), None, b, _ptr(st.mean), _ptr(st.scale),
                                            _ptr(st.inv_scale), _ptr(y2), _stream_ptr()))
    assert np.array_equal(y2.cpu().numpy(), y)


def test_riding_batch_assembly_is_the_gather_at_k8_width(dev):
    """test_batch_assembly_riding_in_the_middle_launches_is_the_gather at F = 65 536 (a batch of 2 x 64 rows): bit for bit."""
    import torch
    from idelucs_amd import _lib, utils as U
    from idelucs_amd.fused import _p, _stream, _DR1_FP32
    L = _lib.lib
    torch.manual_seed(9)
    P, n, F, B, C, m = 4, 40, F8, 64, 20, 128
    feats = (torch.rand((P, n, F), device=dev) * 1e-3).contiguous()
    mean, scale = U.col_stats(feats[0]); inv_scale = (1.0 / scale).contiguous()
    n_pairs = (P - 1) * n                                   # 120 pairs: the batch at offset 72 has only 48 of its 64 rows
    perm = torch.cat([torch.randperm(n_pairs, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)])
    ctl = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    want = torch.full((m, F), -7.0, device=dev)
    base = ctl[1:].clone(); base += B
    _lib.check(L.idl_gather_pairs_at(_p(feats), n, F, n * F, _p(perm), _p(base), B, _p(mean), _p(scale), _p(inv_scale), _p(want), _stream()))
    got = torch.full((m, F), -7.0, device=dev)
    a1 = torch.randn(m, 512, device=dev); W2 = torch.randn(64, 512, device=dev) * 0.06; b2 = torch.zeros(64, device=dev)
    W3 = torch.randn(C, 64, device=dev) * 0.2; b3 = torch.zeros(C, device=dev)
    f = torch.empty(m, 64, device=dev); inv = torch.empty(m, device=dev); r2 = torch.empty(m, 64, device=dev); z = torch.empty(m, C, device=dev)
    next_batch = lambda p0, p1: _lib.idl_next_batch_t(feats=_p(feats), n=n, f=F, view_stride=n * F, pair_idx=_p(perm), base=_p(ctl[1:]), base_add=B,
                                                      n_pairs=n_pairs, batch=B, mean=_p(mean), scale=_p(scale), inv_scale=_p(inv_scale), y=_p(got),
                                                      part=p0, part_end=p1, parts=8)
    _lib.check(L.idl_mid_fwd_gather(_p(a1), None, 0, _p(W2), _p(b2), _p(W3), _p(b3), m, C, 1, 3, _p(ctl), _p(f), _p(inv), _p(r2), _p(z),
                                    next_batch(0, 3), _stream()))
    parts = L.idl_col_sum_parts(); gp = L.idl_nce_fused_parts()
    G = torch.randn(gp, m, 64, device=dev); dP0 = torch.randn(C, C, device=dev); dP0 = dP0 + dP0.t()
    dlg = torch.empty(m, C, device=dev); dlat = torch.empty(m, 64, device=dev); dr1 = torch.empty(m, 512, device=dev)
    p1 = torch.empty(parts, 512, device=dev); p2 = torch.empty(parts, 64, device=dev); p3 = torch.empty(parts, C, device=dev)
    _lib.check(L.idl_mid_bwd_gather(_p(z), _p(r2), _p(f), _p(inv), _p(G), gp, _p(dP0), _p(W3), _p(W2), _p(a1), m, C, 1, 1e-3, _p(dlg), _p(dlat),
                                    _p(dr1), _p(p1), _p(p2), _p(p3), None, 0, *_DR1_FP32, next_batch(3, 8), _stream()))
    torch.cuda.synchronize()
    live = n_pairs - (8 + B)                                  # rows of each half that exist in the pair list
    assert 0 < live < B
    for half in (0, B):
        assert torch.equal(got[half:half + live], want[half:half + live])
        assert torch.all(got[half + live:half + B] == -7.0)   # beyond the end of the list: untouched
    assert ctl.tolist() == [0, 8]


# ------------------------------------------------------------------------------------------------ one step against float64 autograd
def _store_and_net(dev, n, F, C, seed=3):
    """test_gpu_encoder._cfg2_store_and_net at another width: 4 views x n frequency-like rows and a NetLinear(F, C)."""
    import torch
    from idelucs_amd import utils as U, models
    from idelucs_amd.PytorchUtils import NetLinear
    g = torch.Generator(device=dev); g.manual_seed(seed)
    P = 4
    base = torch.rand((1, n, F), device=dev, generator=g) + 0.5
    feats = torch.empty((P, n, F), device=dev)
    for v in range(P):                                         # (a view at a time: the temporaries stay one view wide)
        feats[v] = base[0] * (1.0 + 0.05 * torch.randn((n, F), device=dev, generator=g))
        feats[v] /= feats[v].sum(1, keepdim=True)
    mean, scale = U.col_stats(feats[0])
    store = U.FeatureStore(None, None, feats, mean, scale, 8, False)
    torch.manual_seed(seed)
    net = NetLinear(F, C).to(dev); net.apply(models.weights_init)
    return store, net


def _nce(h, b):
    """info_nce_loss (LossFunctions.py:65-98) without its cast to float32 (tests/test_gpu_small_step.py: _autograd_step)."""
    import torch
    import torch.nn.functional as Fn
    f = Fn.normalize(h, dim=1)
    s = (f @ f.t()) / 0.85
    r = torch.arange(2 * b, device=s.device)
    pos = s[r, (r + b) % (2 * b)]
    s = s.masked_fill(r.unsqueeze(0) == r.unsqueeze(1), float("-inf"))
    return (torch.logsumexp(s, dim=1) - pos).mean()


def _autograd(net, x, dtype):
    """The reference step (models.py:117-133), dropout off, on a copy of net in `dtype` -> (loss, gradients as float64)."""
    from idelucs_amd.LossFunctions import IID_loss
    ref = copy.deepcopy(net).to(dtype).eval()
    z, h = ref(x.to(dtype))
    b = x.shape[0] // 2
    loss = 0.75 * _nce(h, b) + 0.25 * IID_loss(z[:b], z[b:], lamb=2.8)
    loss.backward()
    return float(loss.item()), [p.grad.detach().double() for p in ref.parameters()]


def _check_step(name, loss, grads, x, net):
    """The bars of the existing step tests (loss rel 2e-4, every gradient within 2e-3 of its largest entry) against FLOAT64 autograd.
    Layer 1 sums 16-64 times the terms it sums at k = 6, so where such a constant bar does not fit, the measure is torch's own fp32
    step on the same operands: its error against the float64 step is measured here, and the kernels stay within 4 times that."""
    l64, g64 = _autograd(net, x, __import__("torch").float64)
    l32, g32 = _autograd(net, x, __import__("torch").float32)
    e_k, e_t = abs(loss - l64), abs(l32 - l64)
    print(f"{name}: loss {loss:.7f} (float64 {l64:.7f}): error {e_k:.2e}, torch fp32 {e_t:.2e}")
    assert e_k <= max(2e-4 * abs(l64), 4 * e_t), (name, loss, l64, l32)
    for i, (got, want, t32) in enumerate(zip(grads, g64, g32)):
        top = want.abs().max().item()
        e_k, e_t = (got.double() - want).abs().max().item(), (t32 - want).abs().max().item()
        print(f"{name}: gradient {i}: max error {e_k / top:.2e} of its max, torch fp32 {e_t / top:.2e}")
        assert e_k <= max(2e-3 * top + 1e-12, 4 * e_t), (name, i, e_k, e_t, top)


def _rmsprop_follows(params, p0, grads, names=None):
    """RMSprop on the trainer's own gradients (torch.optim.RMSprop from the same starting parameters): test_default_fused_step_at_cfg2_shape_vs_autograd's bar."""
    import torch
    ps = [p.clone().requires_grad_(True) for p in p0]
    for p, gr in zip(ps, grads):
        p.grad = gr.clone()
    torch.optim.RMSprop(ps, lr=1e-3, weight_decay=0.01).step()
    for i, (p, q) in enumerate(zip(params, ps)):
        bad = ~torch.isclose(p.detach(), q.detach(), rtol=1e-5, atol=1e-7)
        assert bad.float().mean().item() < (2e-3 if p.dim() == 1 else 1e-5), (i, bad.float().mean().item())


@pytest.mark.parametrize("F,planes", [(F8, "1"), (F8, "0"), (F9, "1")])
def test_netlinear_step_vs_float64_autograd(dev, monkeypatch, F, planes):
    """NetLinear(F, 5), m = 256 (the smallest two-plane shape), dropout off: the default form (the two-plane step) and, at F = 65 536,
    IDELUCS_PLANES=0 (the fp32 tiles)."""
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", planes)
    B, C = 128, 5
    store, net = _store_and_net(dev, 100, F, C)
    p0 = [p.detach().clone() for p in net.parameters()]
    ref_net = copy.deepcopy(net)
    tr = FusedLinearTrainer(net, lr=1e-3, weight=0.25, lamb=2.8, seed=5)
    tr._keep_w1_grad = True
    gen = torch.Generator(device=dev); gen.manual_seed(9)
    tr._perm = torch.randperm(store.n_pairs, device=dev, generator=gen)
    tr.ctl[1] = 0; tr.out[1] = 0.0
    bf = tr.buffers(2 * B)
    assert tr._form(bf, store) == ("planes" if planes == "1" else "tiles"), tr._form(bf, store)
    tr._gather(store, bf)
    x = bf.xs[0].clone()
    tr._full_step(store, bf, train=False, pipelined=True, xi=0)
    torch.cuda.synchronize()
    assert not tr.planes_overflowed()
    grads = [tr.gradient(i).clone() for i in range(6)]
    _check_step(f"NetLinear F={F} planes={planes}", tr.out[0].item(), grads, x, ref_net)
    _rmsprop_follows(tr.params, p0, grads)
    assert tr.ctl.tolist() == [1, B]
    # the next batch, assembled by spare workgroups of the two middle launches
    want_next = store.gather_pairs(tr._perm[B:2 * B])
    pb = getattr(bf, "_planes", None)
    if pb is not None and not pb["x32"][1]:
        from idelucs_amd import _lib
        k = int(_lib.lib.idl_planes_exponent(0))
        back = (pb["xh"][1].view(torch.float16).double() + pb["xl"][1].view(torch.float16).double()) * 2.0 ** -k
        err = (back - want_next.double()).abs()
        assert pb["valid"][1] and bool((err <= torch.clamp(want_next.double().abs() * 2.0 ** -21, min=2.0 ** (-25 - k))).all())
    else:
        assert torch.equal(bf.xs[1], want_next)


def test_small_native_step_vs_float64_autograd_at_k8_width(dev):
    """myNet(32 896, 5): the canonical 8-mer width of model_size='small', m = 64, dropout off."""
    import torch
    import test_gpu_small_step as S
    F, m, C = (F8 + 2 ** 8) // 2, 64, 5
    net = S._random_net(F, C, dev, seed=F + m + C)
    p0 = [p.detach().clone() for p in net.parameters()]
    x = torch.randn((m, F), device=dev, generator=torch.Generator(device=dev).manual_seed(F * 7 + m + C))
    ref_net = copy.deepcopy(net)
    tr = S._trainer(net)
    bf = tr.buffers(m)
    bf.x.copy_(x)
    tr.step_on_batch(bf, train=False)
    torch.cuda.synchronize()
    grads = [tr.gradient(i).clone() for i in range(8)]
    _check_step("myNet F=32896", tr.out[0].item(), grads, x, ref_net)
    ps = [p.clone().requires_grad_(True) for p in p0]
    for p, gr in zip(ps, grads):
        p.grad = gr.clone()
    torch.optim.RMSprop(ps, lr=1e-3, weight_decay=0.01).step()
    for p, want in zip(tr.params, ps):                           # (_check_against_autograd's bar)
        assert (p.detach() - want.detach()).abs().max().item() <= 1e-5 * want.detach().abs().max().item()


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_equals_eager_at_k8_width(dev):
    """An epoch on a 64-sequence store at F = 65 536 (192 pairs, batches of 16: twelve steps -- two of warm-up, four captured, one replay of
    four, two eager; run_epoch captures from eight full batches on -- dropout on) replayed from the captured graph equals the same epoch
    launched eagerly bit for bit."""
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    store, net0 = _store_and_net(dev, 64, F8, 5, seed=4)
    B = 16
    results = []
    for use_graph in (False, True):
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=11)
        gen = torch.Generator(device=dev); gen.manual_seed(77)
        total, nb = tr.run_epoch(store, B, use_graph=use_graph, generator=gen)
        torch.cuda.synchronize()
        assert nb == 12 and tr.ctl.tolist() == [12, store.n_pairs]
        if use_graph:
            assert len(tr._graphs) == 1, "the epoch did not go through a captured graph"
        results.append(([p.detach().clone() for p in tr.params], total.item()))
    assert np.isfinite(results[0][1]) and results[0][1] == results[1][1]
    for a, b in zip(results[0][0], results[1][0]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ end to end
def _args(**kw):
    a = {'sequence_file': os.path.join(DATA, "influenza_64.fas"), 'GT_file': None, 'n_clusters': 5, 'k': 8, 'model_size': 'linear',
         'n_mimics': 3, 'batch_sz': 32, 'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None,
         'n_epochs': 3, 'n_voters': 1}
    a.update(kw)
    return a


@pytest.mark.parametrize("size", ["linear", "small"])
def test_iid_model_trains_and_predicts_at_k8(dev, size):
    from idelucs_amd import models
    from idelucs_amd.fused_small import FusedSmallTrainer
    m = models.IID_model(_args(model_size=size, **({'small_step': 'native'} if size == "small" else {})))
    m.build_dataloader()
    m.begin_voter(0)
    assert m.net.n_input == (F8 if size == "linear" else (F8 + 2 ** 8) // 2)
    losses = [m.contrastive_training_epoch() for _ in range(3)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert (m._fused is not None) if size == "linear" else isinstance(m._small, FusedSmallTrainer)      # the native step forms, not autograd
    y, p, lat = m.predict()
    assert y.dtype == np.int64 and y.shape == (64,) and p.dtype == np.float64 and p.shape == (64,)
    assert lat.dtype == np.float64 and lat.shape == (64, 64) and np.all(np.isfinite(lat))
    probs = m.calculate_probs()
    assert probs.dtype == np.float64 and probs.shape == (64, 5)


def test_iid_model_refuses_k10(dev):
    from idelucs_amd import models
    with pytest.raises(ValueError, match=r"1\.\.9"):
        m = models.IID_model(_args(k=10))
        m.build_dataloader()


def test_augment_fasta_k8_compat_vs_reference(dev, tmp_path):
    """AugmentFasta(8 records, n_mimics = 3, k = 8, rng='compat') against the fixture from the reference, at the existing test's atol."""
    from idelucs_amd import utils as U
    from test_oracle_golden_large_k import influenza_8
    g = np.load(os.path.join(GOLDEN, "augment_k8.npz"))
    np.random.seed(0); random.seed(0)
    x = U.AugmentFasta(influenza_8(tmp_path), 3, k=8, rng="compat")
    assert x.dtype == np.float32 and list(x.shape) == g["shape"].tolist()
    np.testing.assert_allclose(x[:, :, g["cols"]], g["values"], rtol=0, atol=2e-6)
    # 65 536 entries within 2e-6 each
    np.testing.assert_allclose(x.astype(np.float64).sum(2), g["row_sums"], rtol=0, atol=2e-6 * F8)


@pytest.mark.parametrize("k", [8, 9])
@pytest.mark.parametrize("name", ["edge", "influenza_8"])
def test_fasta_entry_points_vs_golden(dev, tmp_path, name, k):
    """kmersFasta(reduce=False/True), cgrFasta and the scalar kmer_counts / cgr on top of a non-zero start, against the reference's rows."""
    import idelucs_amd as gpu
    from test_oracle_golden_large_k import large_k_rows, fixture_file
    g = np.load(os.path.join(GOLDEN, "large_k.npz"))
    fn = fixture_file(name, tmp_path)
    names, f = gpu.kmersFasta(fn, k=k)
    assert list(names) == g[f"{name}_names"].tolist() and f.dtype == np.float64 and np.array_equal(f, large_k_rows(g, name, k, "freq"))
    canon = large_k_rows(g, name, k, "canon", int(g[f"{name}_k{k}_canon_len"]))
    _, fr = gpu.kmersFasta(fn, k=k, reduce=True)
    assert np.array_equal(fr, canon / canon.sum(1, keepdims=True))
    _, cf = gpu.cgrFasta(fn, k=k)
    assert np.array_equal(cf, large_k_rows(g, name, k, "cgrfreq"))
    if k == 8:
        km, cg = large_k_rows(g, name, k, "kmer"), large_k_rows(g, name, k, "cgr")
        start = np.random.default_rng(1).integers(1, 9, 4 ** k).astype(np.int32)
        for i, (_, s) in enumerate(list(O.fasta_records(fn))[:3]):
            c = start.copy(); gpu.kmer_counts(bytearray(s), k, c)
            assert np.array_equal(c, start + km[i]), (name, i)
            c = start.copy(); gpu.cgr(bytearray(s), k, c)
            assert np.array_equal(c, start + cg[i]), (name, i)
    c1 = large_k_rows(g, name, k, "kmer1")[0].copy()
    out = gpu.kmer_rev_comp(c1, k)
    assert np.array_equal(out, canon[0]) and int(out.sum()) == int(g[f"{name}_k{k}_canon_sum"][0])


def test_cli_k8_writes_reference_outputs(tmp_path, monkeypatch, capsys):
    import pandas as pd
    from idelucs_amd.__main__ import main
    monkeypatch.chdir(tmp_path)
    out_dir = main(["--sequence_file", os.path.join(DATA, "influenza_64.fas"), "--k", "8", "--n_clusters", "5", "--n_epochs", "3", "--n_voters", "2",
                    "--batch_sz", "32"])
    capsys.readouterr()
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 64
    assert "'k': 8" in open(tmp_path / "ALL_RESULTS.tsv").read().splitlines()[-1]
