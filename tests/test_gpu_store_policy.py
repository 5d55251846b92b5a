"""The cache policy of the training step's bulk output stores (csrc/store_policy.h; IDELUCS_DEV=store_wt=<mask>) changes no bit: every site's kernel and
the whole step, with every store plain (mask 0), with the compiled-in default mask and with every site write-through (mask 15).  The environment is set
before each launcher call and before each trainer is built: the launchers read the mask at every launch, a captured graph keeps the mask it was captured with."""
import copy
import ctypes
import os

import pytest

pytestmark = pytest.mark.gpu

MASKS = (0, None, 15)                      # None: IDELUCS_DEV names no mask -- the compiled-in default


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _set_mask(monkeypatch, mask):
    """store_wt=<mask> beside whatever else IDELUCS_DEV carries; the library then reports that mask (the default for None)."""
    from idelucs_amd import _lib
    keep = [kv for kv in os.environ.get("IDELUCS_DEV", "").split(",") if kv and kv.split("=")[0] != "store_wt"]
    if mask is not None:
        keep.append("store_wt=%d" % mask)
    if keep:
        monkeypatch.setenv("IDELUCS_DEV", ",".join(keep))
    else:
        monkeypatch.delenv("IDELUCS_DEV", raising=False)
    got = int(_lib.lib.idl_store_wt_mask())
    assert 0 <= got <= 15 and (mask is None or got == mask), (mask, got)
    return got


def _same(runs):
    """Every run's tensors equal the first run's, bit for bit (compared as integers: a NaN left unwritten would be seen)."""
    import torch
    for r in runs[1:]:
        assert len(r) == len(runs[0])
        for i, (a, b) in enumerate(zip(runs[0], r)):
            assert a.shape == b.shape and a.dtype == b.dtype, i
            ai = a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a
            bi = b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b
            assert torch.equal(ai, bi), "tensor %d differs in %d places" % (i, (ai != bi).sum().item())


@pytest.mark.parametrize("F", [1024, 1028])
def test_the_batch_assembly_writes_the_same_rows_planes_and_flag(dev, monkeypatch, F):
    """gather_tile (the riders of idl_mid_fwd_gather, and the stand-alone idl_gather_pairs_at): 40 rows (a partial row group), a pair list that ends inside the
    batch (rows left untouched), one entry beyond the planes' range (clamped, flag raised).  F = 1024: lanes pair up for 16-byte plane stores;
    F = 1028: F / 4 is odd, a row's last lane has no partner and rows start 8 bytes off a 16-byte boundary -- the 8-byte stores remain."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    g = torch.Generator(device="cpu"); g.manual_seed(31 + F)
    n, B, C, H2, mm = 300, 20, 5, 64, 32
    feats = torch.randn(3, n, F, generator=g)
    perm = torch.randperm(2 * n, generator=g)
    first, cut = 64, 64 + 15                                                    # the batch starts at pair 64; the list ends 15 pairs later
    feats[0, int(perm[first + 3]) % n, 9] = 1e6                                 # (a "true" row of the batch: view 0)
    feats = feats.to(dev)
    mean = torch.randn(F, generator=g, dtype=torch.float64).to(dev); scale = (torch.rand(F, generator=g, dtype=torch.float64) + 0.5).to(dev)
    inv_scale = 1.0 / scale
    perm = perm.to(dev)
    base = torch.tensor([first], dtype=torch.int64, device=dev)
    a1 = (torch.randn(8, 512, mm, generator=g) * 0.1).to(dev); b1 = torch.zeros(512, device=dev)
    W2 = (torch.randn(H2, 512, generator=g) / 23).to(dev); b2 = torch.zeros(H2, device=dev)
    W3 = (torch.randn(C, H2, generator=g) / 8).to(dev); b3 = torch.zeros(C, device=dev)
    ctl = torch.zeros(2, dtype=torch.int64, device=dev)
    f = torch.empty(mm, H2, device=dev); inv = torch.empty(mm, device=dev); r2 = torch.empty(mm, H2, device=dev); z = torch.empty(mm, C, device=dev)
    runs = []
    for mask in MASKS:
        _set_mask(monkeypatch, mask)
        y = torch.full((2 * B, F), -7.0, device=dev); yh = torch.full((2 * B, F), 77, dtype=torch.int16, device=dev); yl = torch.full_like(yh, 78)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        nb = _lib.idl_next_batch_t(feats=_p(feats), n=n, f=F, view_stride=n * F, pair_idx=_p(perm), base=_p(base), base_add=0, n_pairs=cut, batch=B, mean=_p(mean),
                                   scale=_p(scale), inv_scale=_p(inv_scale), y=_p(y), y_hi=_p(yh), y_lo=_p(yl), overflow_flag=_p(flag), part=0, part_end=8, parts=8)
        _lib.check(L.idl_mid_fwd_gather(_p(a1.clone()), _p(b1), 1, _p(W2), _p(b2), _p(W3), _p(b3), mm, C, 1, ctypes.c_uint64(3), _p(ctl), _p(f), _p(inv), _p(r2), _p(z),
                                        nb, _stream()))
        alone = torch.full((2 * B, F), -7.0, device=dev)
        _lib.check(L.idl_gather_pairs_at(_p(feats), n, F, n * F, _p(perm), _p(base), B, _p(mean), _p(scale), _p(inv_scale), _p(alone), _stream()))
        torch.cuda.synchronize()
        runs.append((y, yh, yl, flag, alone))
    y, yh, yl, flag, alone = runs[0]
    assert flag.item() == 1 and bool((y[15:B] == -7.0).all()) and bool((y[B + 15:] == -7.0).all()) and bool((yh[15:B] == 77).all()) and bool((yl[B + 15:] == 78).all())
    assert torch.equal(y[:15], alone[:15]) and torch.equal(y[B:B + 15], alone[B:B + 15]) and not bool((y[:15] == -7.0).any())
    _same(runs)


@pytest.mark.parametrize("rows", [0, 1])
def test_layer_1_partial_sums_are_the_same(dev, monkeypatch, rows):
    """idl_l1_planes (part[8][n_out][m]) and idl_l1_planes_rows (part[8][m][n_out]) at the smallest shape they take."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    g = torch.Generator(device="cpu"); g.manual_seed(5)
    m, H, K = 128, 128, 1024
    assert L.idl_l1_planes_supported(m, H, K) == 1
    wh = (torch.randn(H, K, generator=g) * 0.1).half().view(torch.int16).to(dev); wl = (torch.randn(H, K, generator=g) * 1e-4).half().view(torch.int16).to(dev)
    xh = torch.randn(m, K, generator=g).half().view(torch.int16).to(dev); xl = (torch.randn(m, K, generator=g) * 1e-3).half().view(torch.int16).to(dev)
    fn = L.idl_l1_planes_rows if rows else L.idl_l1_planes
    runs = []
    for mask in MASKS:
        _set_mask(monkeypatch, mask)
        part = torch.full((int(L.idl_l1_planes_parts()), m, H) if rows else (int(L.idl_l1_planes_parts()), H, m), float("nan"), device=dev)
        _lib.check(fn(_p(wh), _p(wl), K, _p(xh), _p(xl), K, m, H, K, _p(part), _stream()))
        torch.cuda.synchronize()
        runs.append((part,))
    assert bool(torch.isfinite(runs[0][0]).all()) and runs[0][0].abs().max().item() > 0.0
    _same(runs)


def test_the_weight_gradient_launch_leaves_the_same_weights_and_planes(dev, monkeypatch):
    """idl_wgrad_rmsprop_xplanes: W, square_avg, the gradient, both planes of W and the flag."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    g = torch.Generator(device="cpu"); g.manual_seed(23)
    m, H, F = 256, 512, 1024
    assert L.idl_wgrad_xplanes_supported(m, H, F) == 1
    dy = (torch.randn(m, H, generator=g) * 1e-3).to(dev); x = torch.randn(m, F, generator=g).to(dev)
    W0 = (torch.randn(H, F, generator=g) * 0.02).to(dev); V0 = (torch.rand(H, F, generator=g) * 1e-6 + 1e-8).to(dev)
    hyper = torch.tensor([1e-3, 0.99, 1e-8, 0.01, 0.01], dtype=torch.float32, device=dev)

    def split(v, k):
        a = torch.empty(v.shape, dtype=torch.int16, device=dev); b = torch.empty_like(a); fl = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.idl_split_planes(_p(v), v.numel(), k, _p(a), _p(b), _p(fl), _stream()))
        return a, b

    xh, xl = split(x, int(L.idl_planes_exponent(0)))
    k = 9 - int(torch.frexp(dy.abs().max().cpu())[1].item())
    dyh, dyl = split(dy, k)
    runs = []
    for mask in MASKS:
        _set_mask(monkeypatch, mask)
        W, V, grad = W0.clone(), V0.clone(), torch.full((H, F), float("nan"), device=dev)
        wh = torch.full((H, F), 77, dtype=torch.int16, device=dev); wl = torch.full_like(wh, 78); flag = torch.zeros(1, dtype=torch.int32, device=dev)
        sc = torch.zeros(int(L.idl_dr1_scale_words()), dtype=torch.int32, device=dev); sc[0] = k
        _lib.check(L.idl_wgrad_rmsprop_xplanes(_p(dyh), _p(dyl), _p(sc), _p(xh), _p(xl), F, m, H, F, _p(grad), _p(W), _p(V), _p(hyper), _p(wh), _p(wl), _p(flag), _stream()))
        torch.cuda.synchronize()
        runs.append((W, V, grad, wh, wl, flag))
    W, V, grad, wh, wl, flag = runs[0]
    hi, lo = split(W, int(L.idl_planes_exponent(1)))
    assert torch.equal(hi, wh) and torch.equal(lo, wl) and flag.item() == 0 and not torch.equal(W, W0) and bool(torch.isfinite(grad).all())
    _same(runs)


def _store_and_net(dev, n, F=1024, C=20):
    import torch
    from idelucs_amd import utils as U, models
    from idelucs_amd.PytorchUtils import NetLinear
    g = torch.Generator(device=dev); g.manual_seed(11)
    P = 4
    base = torch.rand((1, n, F), device=dev, generator=g) + 0.5
    feats = base * (1.0 + 0.05 * torch.randn((P, n, F), device=dev, generator=g))
    feats = (feats / feats.sum(2, keepdim=True)).contiguous()
    mean, scale = U.col_stats(feats[0])
    store = U.FeatureStore(None, None, feats, mean, scale, 5 if F == 1024 else 6, False)
    torch.manual_seed(3)
    net = NetLinear(F, C).to(dev); net.apply(models.weights_init)
    return store, net


def test_the_default_step_trains_to_the_same_bits(dev, monkeypatch):
    """The lone voter's default step at k = 5's shape (F = 1024, 2 x 128 rows, 20 clusters, dropout on): nine batches -- two eager steps, a captured graph
    of two steps replayed three times, an eager step -- leave the same parameters, running averages, planes of W1, loss sum and counters."""
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    B = 128
    store, net0 = _store_and_net(dev, 3 * B)                                  # 3 mimics x 384 rows = 1 152 pairs = 9 batches
    assert store.n_pairs == 9 * B
    runs = []
    for mask in MASKS:
        _set_mask(monkeypatch, mask)
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=5)
        tr.begin_voter(0)
        assert tr._form(tr.buffers(2 * B), store) == "planes" and tr._sums_fwd, "not the default launch sequence"
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        total, nb = tr.run_epoch(store, B, use_graph=True, generator=gen)
        torch.cuda.synchronize()
        assert nb == 9 and getattr(tr, "n_captures", 0) == 1 and not tr.planes_overflowed()
        runs.append(tuple(p_.detach().clone() for p_ in tr.params) + tuple(v.clone() for v in tr.square_avg) + (tr._w1_planes[0].clone(), tr._w1_planes[1].clone(),
                                                                                                             tr.out.clone(), tr.ctl.clone(), total.clone().reshape(1)))
    assert bool(torch.isfinite(runs[0][-1]).all()) and runs[0][-2].tolist() == [9, 9 * B]
    _same(runs)


@pytest.mark.parametrize("F", [1024, 4096])
def test_two_voters_in_lockstep_train_to_the_same_bits(dev, monkeypatch, F):
    """The same for two voters whose launches are recorded and run once for both (BatchedLinearTrainer).  F = 1024: the shape above, where voters in lockstep
    take the fp32 products (the dW1 launch of the two-plane form wants a tile for 144 CUs or more) and the riders assemble fp32 rows; F = 4096: every launch
    of the two-plane step recorded -- the batched instances of the layer-1 and dW1 kernels."""
    import torch
    from idelucs_amd import fused
    from idelucs_amd.fused import BatchedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    monkeypatch.setitem(fused.VARIANTS, "lockstep_planes", "1")
    B = 128
    store, net0 = _store_and_net(dev, 3 * B, F=F)
    runs = []
    for mask in MASKS:
        _set_mask(monkeypatch, mask)
        nets = []
        for l in range(2):
            net = copy.deepcopy(net0)
            with torch.no_grad():
                for p_ in net.parameters():
                    p_.mul_(1.0 + 0.05 * l)
            nets.append(net)
        bt = BatchedLinearTrainer(nets, lr=1e-3, weight=0.25, lamb=2.8, seed=11)
        gens = []
        for l, tr in enumerate(bt.trainers):
            tr.begin_voter(l)
            gen = torch.Generator(device=dev); gen.manual_seed(100 + l)
            gens.append(gen)
        res = bt.run_epoch(store, B, gens, use_graph=True)
        torch.cuda.synchronize()
        assert bt._planes_step == (F == 4096) and len(bt._graphs) == 1 and not bt.planes_overflowed()
        out = []
        for (total, nb), tr in zip(res, bt.trainers):
            assert nb == 9
            out += [p_.detach().clone() for p_ in tr.params] + [v.clone() for v in tr.square_avg] + [tr.out.clone(), tr.ctl.clone(), total.clone().reshape(1)]
        runs.append(tuple(out))
    assert bool(torch.isfinite(runs[0][-1]).all())
    _same(runs)
