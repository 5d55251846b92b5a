"""The forward middle inside the launch that adds layer 1's K-slice partial sums (csrc/train_step.hip: sums_fwd_kernel; fused.VARIANTS['sums_fwd']): six
launches a step instead of seven, every result bit for bit what the two launches leave.
Reference: the step of idelucs/models.py:117-133 through Linear(F,512) .. Softmax of idelucs/PytorchUtils.py:38-50.

Shapes: the smallest the plane kernels take -- F = 1024, H = 512, m = 128 (one tile of the batch) and 384 (three: not a power of two), 2 / 20 / 48 output
units (one, two, three logit tiles).  The merged launch is part of the lone step only where the optimizer tail rides on the dW1 tiles, which needs a dW1 tile
for at least 144 CUs (fused._tile_per_cu: F >= 2304) and m >= 192: the twenty-step test therefore ALSO runs at F = 2560, m = 384, the smallest such shape, and
asserts there that the merged launch ran (at F = 1024 both settings take the seven launches)."""
import copy
import ctypes

import pytest

pytestmark = pytest.mark.gpu

H1, H2 = 512, 64


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


def _planes(v, which):
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    hi = torch.empty(v.shape, dtype=torch.int16, device=v.device)
    lo = torch.empty_like(hi)
    _lib.check(L.idl_split_planes(_p(v), v.numel(), int(L.idl_planes_exponent(which)), _p(hi), _p(lo), None, _stream()))
    return hi, lo


@pytest.mark.parametrize("n_out,m,K", [(512, 128, 1024), (512, 384, 1024), (128, 256, 1024)])
def test_partial_sums_with_a_row_contiguous_are_the_transposed_ones(dev, n_out, m, K):
    """idl_l1_planes_rows writes part[8][m][n_out]: slab for slab the transpose of idl_l1_planes' part[8][n_out][m] on the same operands, bit for bit (the
    swapped-role call is NOT: it adds the two low-plane products in the other order)."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    g = torch.Generator(device=dev); g.manual_seed(n_out + m)
    W = torch.randn((n_out, K), device=dev, generator=g) * 0.05
    x = torch.randn((m, K), device=dev, generator=g)
    wh, wl = _planes(W, 1)
    xh, xl = _planes(x, 0)
    parts = int(L.idl_l1_planes_parts())
    old = torch.full((parts, n_out, m), float("nan"), device=dev)
    new = torch.full((parts, m, n_out), float("nan"), device=dev)
    _lib.check(L.idl_l1_planes(_p(wh), _p(wl), K, _p(xh), _p(xl), K, m, n_out, K, _p(old), _stream()))
    _lib.check(L.idl_l1_planes_rows(_p(wh), _p(wl), K, _p(xh), _p(xl), K, m, n_out, K, _p(new), _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(old).all() and old.abs().max().item() > 0
    assert torch.equal(new.view(torch.int32), old.transpose(1, 2).contiguous().view(torch.int32))


def _small_store(dev, n, F, seed, views=2):
    import torch
    from idelucs_amd import utils as U
    g = torch.Generator(device=dev); g.manual_seed(seed)
    base = torch.rand((1, n, F), device=dev, generator=g) + 0.5
    feats = base * (1.0 + 0.05 * torch.randn((views, n, F), device=dev, generator=g))
    feats = (feats / feats.sum(2, keepdim=True)).contiguous()
    mean, scale = U.col_stats(feats[0])
    return U.FeatureStore(None, None, feats, mean, scale, 5, False)


@pytest.mark.parametrize("m", [128, 384])
@pytest.mark.parametrize("C", [2, 20, 48])
def test_merged_launch_leaves_what_the_two_launches_leave(dev, m, C):
    """On the same partial sums: idl_reduce_mid_fwd_gather_planes' r1, f, inv, r2, z (and the next batch's planes its riders assemble, and the step counter's
    copy) against idl_reduce_parts_rms + idl_mid_fwd_gather -- dropout on and off, riders on and off; bit for bit.  With dropout on, r1 is also what
    the unfused idl_relu_dropout_fwd (layer id 1) leaves on the summed, biased activations.  The partial sums are only read."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    F = 1024
    g = torch.Generator(device=dev); g.manual_seed(m + C)
    parts = int(L.idl_l1_planes_parts())
    part0 = torch.randn((parts, H1, m), device=dev, generator=g) * (0.5 + torch.rand((parts, 1, 1), device=dev, generator=g))
    rows0 = part0.transpose(1, 2).contiguous()                       # [8][m][512]
    b1 = torch.randn(H1, device=dev, generator=g) * 0.3
    W2 = torch.randn((H2, H1), device=dev, generator=g) * 0.06
    b2 = torch.randn(H2, device=dev, generator=g) * 0.1
    W3 = torch.randn((C, H2), device=dev, generator=g) * 0.3
    b3 = torch.randn(C, device=dev, generator=g) * 0.1
    st = _small_store(dev, 3 * m, F, seed=m)
    perm = torch.randperm(st.n_pairs, device=dev, generator=g)
    ctl = torch.tensor([(3 << 24) + 17, m // 2], dtype=torch.int64, device=dev)
    seed = 0x1234567887654321

    def outs():
        return [torch.full(s, float("nan"), device=dev) for s in ((m, H2), (m,), (m, H2), (m, C))]

    def next_batch(riders, xh, xl, flag):
        if not riders:
            return None
        return _lib.idl_next_batch_t(feats=_p(st.feats), n=st.n, f=st.f, view_stride=st.n * st.f, pair_idx=_p(perm), base=_p(ctl[1:]), base_add=m // 2,
                                     n_pairs=st.n_pairs, batch=m // 2, mean=_p(st.mean), scale=_p(st.scale), inv_scale=_p(st.inv_scale),
                                     y_hi=_p(xh), y_lo=_p(xl), overflow_flag=_p(flag), part=0, part_end=8, parts=8)

    for train in (0, 1):
        for riders in (0, 1):
            part = part0.clone()
            snap = torch.zeros(1, dtype=torch.int64, device=dev)
            f, inv, r2, z = outs()
            xh = torch.zeros((m, F), dtype=torch.int16, device=dev); xl = torch.zeros_like(xh)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(L.idl_reduce_parts_rms(_p(part), H1 * m, _p(ctl), _p(snap), None, _stream()))
            _lib.check(L.idl_mid_fwd_gather(_p(part), _p(b1), 1, _p(W2), _p(b2), _p(W3), _p(b3), m, C, train, seed, _p(ctl), _p(f), _p(inv), _p(r2),
                                            _p(z), next_batch(riders, xh, xl, flag), _stream()))
            torch.cuda.synchronize()
            want = (part[0].clone(), f, inv, r2, z, xh, xl, snap)
            assert all(torch.isfinite(t).all() for t in want[:5])
            src = rows0.clone()
            r1T = torch.full((H1, m), float("nan"), device=dev)
            snap_n = torch.zeros(1, dtype=torch.int64, device=dev)
            f_n, inv_n, r2_n, z_n = outs()
            xh_n = torch.zeros((m, F), dtype=torch.int16, device=dev); xl_n = torch.zeros_like(xh_n)
            _lib.check(L.idl_reduce_mid_fwd_gather_planes(_p(src), _p(ctl), _p(snap_n), _p(r1T), _p(b1), _p(W2), _p(b2), _p(W3), _p(b3), m, C, train,
                                                          seed, _p(f_n), _p(inv_n), _p(r2_n), _p(z_n), next_batch(riders, xh_n, xl_n, flag), _stream()))
            torch.cuda.synchronize()
            got = (r1T, f_n, inv_n, r2_n, z_n, xh_n, xl_n, snap_n)
            for name, a_, b_ in zip(("r1", "f", "inv", "r2", "z", "x_hi", "x_lo", "step snapshot"), got, want):
                assert torch.equal(a_, b_), (name, train, riders, (a_.double() - b_.double()).abs().max().item())
            assert torch.equal(src, rows0)
            assert snap_n.item() == ctl[0].item() and flag.item() == 0
            if train:
                assert (r1T == 0).float().mean().item() > 0.5 and (r1T > 0).any()
                # ... and the unfused kernel's: the sums in ascending slab order, the bias, then idl_relu_dropout_fwd on the flat [m][512] array
                acc = rows0[0].clone()
                for p_ in range(1, parts):
                    acc += rows0[p_]
                acc += b1
                _lib.check(L.idl_relu_dropout_fwd(_p(acc), acc.numel(), 1, seed, _p(ctl), 1, _stream()))
                torch.cuda.synchronize()
                assert torch.equal(r1T, acc.t()), (train, riders, (r1T.double() - acc.t().double()).abs().max().item())
            if riders:
                assert xh_n.ne(0).any()


def _run_twenty(dev, store, net0, B, sums_fwd, graph, cold, monkeypatch):
    import torch
    from idelucs_amd import fused
    monkeypatch.setitem(fused.VARIANTS, "sums_fwd", sums_fwd)
    monkeypatch.setitem(fused.VARIANTS, "test_cold", "1" if cold else "0")
    tr = fused.FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=11)
    tr.begin_voter(1)
    gen = torch.Generator(device=dev); gen.manual_seed(100)
    total, nb = tr.run_epoch(store, B, use_graph=graph, generator=gen)
    torch.cuda.synchronize()
    assert nb == 20 and (not graph or getattr(tr, "n_captures", 0) == 1)
    pb = getattr(tr.buffers(2 * B), "_planes", None)
    merged = pb is not None and pb["r1T"][0] is not None
    state = [p_.detach().clone() for p_ in tr.params] + [v.clone() for v in tr.square_avg] + [tr.out.clone(), tr.ctl.clone(), tr._dr1_scale.clone()]
    return state, merged


@pytest.mark.parametrize("F,m,C", [(1024, 128, 20), (1024, 384, 2), (2560, 384, 2), (2560, 384, 20), (2560, 384, 48)])
def test_twenty_steps_are_the_seven_launch_steps(dev, monkeypatch, F, m, C):
    """Twenty steps (an epoch of twenty full batches) from one state with sums_fwd = 0 and 1, eager and graph-replayed, with warm
    caches and under test_cold = 1: every parameter, running average, the loss sums and the counters are equal bit for bit."""
    import torch
    from idelucs_amd import models
    from idelucs_amd.PytorchUtils import NetLinear
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    B = m // 2
    store = _small_store(dev, 20 * B, F, seed=F + m + C)
    assert store.n_pairs == 20 * B
    torch.manual_seed(C)
    net0 = NetLinear(F, C).to(dev); net0.apply(models.weights_init)
    want, merged = _run_twenty(dev, store, net0, B, "0", False, False, monkeypatch)
    assert not merged
    assert all(torch.isfinite(t).all() for t in want[:13])
    for sums_fwd in ("0", "1"):
        for graph in (False, True):
            for cold in (False, True):
                if (sums_fwd, graph, cold) == ("0", False, False):
                    continue
                got, merged = _run_twenty(dev, store, net0, B, sums_fwd, graph, cold, monkeypatch)
                assert merged == (sums_fwd == "1" and F >= 2304 and m >= 192), (sums_fwd, F, m, merged)
                for i, (a_, b_) in enumerate(zip(got, want)):
                    assert torch.equal(a_, b_), (i, sums_fwd, graph, cold)
