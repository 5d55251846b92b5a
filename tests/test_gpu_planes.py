"""The two-fp16-plane form of the training step's layer-1 product (csrc/planes.h, csrc/l1_planes_device.h; IDELUCS_PLANES=1) against
float64 products, against the fp32 tiles it replaces, and against the default step.  Reference: Linear(F,512) of idelucs/PytorchUtils.py:38-45
inside the step of idelucs/models.py:117-133."""
import copy
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _split(v, which):
    """idl_split_planes of tensor v with the fixed exponent of its kind -> (hi, lo int16 tensors, exponent, flag)."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    k = int(L.idl_planes_exponent(which))
    hi = torch.empty(v.shape, dtype=torch.int16, device=v.device)
    lo = torch.empty_like(hi)
    flag = torch.zeros(1, dtype=torch.int32, device=v.device)
    _lib.check(L.idl_split_planes(_p(v), v.numel(), k, _p(hi), _p(lo), _p(flag), _stream()))
    return hi, lo, k, flag


def test_planes_carry_22_bits_and_flag_what_leaves_their_range(dev):
    import torch
    g = torch.Generator(device="cpu"); g.manual_seed(3)
    v = (torch.randn(512, 4096, generator=g) * torch.logspace(-6, 1.5, 4096)).to(dev)      # 1e-6 .. 30 in size
    hi, lo, k, flag = _split(v, 0)
    back = (hi.view(torch.float16).double() + lo.view(torch.float16).double()) * 2.0 ** -k
    err = (back - v.double()).abs()
    # 22 significand bits where the low plane is a normal fp16 number, fp16's subnormal spacing (2^-24) / 2^k below that
    assert bool((err <= torch.maximum(v.double().abs() * 2.0 ** -21, torch.tensor(2.0 ** (-25 - k), device=dev, dtype=torch.float64))).all())
    assert flag.item() == 0
    w = torch.full((8,), 1.0, device=dev); w[3] = 17.0                       # 17 * 2^12 > 65 000
    hi, lo, k, flag = _split(w, 1)
    assert flag.item() == 1
    back = (hi.view(torch.float16).float() + lo.view(torch.float16).float()) * 2.0 ** -k
    assert back[0].item() == 1.0 and abs(back[3].item() - 65000.0 / 4096) < 1e-3


@pytest.mark.parametrize("m,F", [(1024, 4096), (256, 1024), (128, 2048), (384, 1536)])
def test_layer1_product_from_planes_is_closer_to_float64_than_the_fp32_gemm(dev, m, F):
    """idl_l1_planes: the eight K-slice partial sums add up to W1 x^T within 5e-7 of its largest entry -- and no further from the float64
    product than torch's fp32 GEMM."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    g = torch.Generator(device="cpu"); g.manual_seed(m + F)
    H = 512
    W = ((torch.rand(H, F, generator=g) * 2 - 1) / F ** 0.5).to(dev)
    x = torch.randn(m, F, generator=g).to(dev)
    x[5, 7] = 300.0                                                            # an outlier of a standardised feature
    assert L.idl_l1_planes_supported(m, H, F) == 1 and L.idl_l1_planes_supported(m + 64, H, F) == 0 and L.idl_l1_planes_supported(m, H, 768) == 0
    wh, wl, kw, _ = _split(W, 1)
    xh, xl, kx, _ = _split(x, 0)
    P = int(L.idl_l1_planes_parts())
    part = torch.full((P, H, m), float("nan"), device=dev)
    _lib.check(L.idl_l1_planes(_p(wh), _p(wl), F, _p(xh), _p(xl), F, m, H, F, _p(part), _stream()))
    torch.cuda.synchronize()
    got = part.double().sum(0)
    ref = W.double() @ x.double().t()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item() / scale
    e_lib = ((W @ x.t()).double() - ref).abs().max().item() / scale
    assert err < 5e-7 and err <= e_lib, (err, e_lib)
    assert L.idl_l1_planes(_p(wh), _p(wl), F, _p(xh), _p(xl), F, m + 1, H, F, _p(part), _stream()) != 0


def test_producers_write_the_planes_of_what_they_write(dev):
    """The dW1 tiles' epilogue (idl_wgrad_rmsprop_planes) leaves W1 exactly as idl_wgrad_rmsprop does, with planes that are idl_split_planes of
    it; the batch-assembling workgroups of idl_mid_*_gather leave the batch idl_gather_pairs_at assembles, with its planes."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    g = torch.Generator(device="cpu"); g.manual_seed(21)
    m, H, F = 256, 512, 1024
    dy = (torch.randn(m, H, generator=g) * 1e-3).to(dev); x = torch.randn(m, F, generator=g).to(dev)
    W0 = ((torch.rand(H, F, generator=g) * 2 - 1) / F ** 0.5).to(dev); V0 = (torch.rand(H, F, generator=g) * 1e-6).to(dev)
    hyper = torch.tensor([1e-3, 0.99, 1e-8, 0.01, 0.01], device=dev)
    Wa, Va, Wb, Vb = W0.clone(), V0.clone(), W0.clone(), V0.clone()
    wh = torch.empty(H, F, dtype=torch.int16, device=dev); wl = torch.empty_like(wh); flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.idl_wgrad_rmsprop(_p(dy), _p(x), m, H, F, None, _p(Wa), _p(Va), _p(hyper), _stream()))
    _lib.check(L.idl_wgrad_rmsprop_planes(_p(dy), _p(x), m, H, F, None, _p(Wb), _p(Vb), _p(hyper), _p(wh), _p(wl), _p(flag), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(Wa, Wb) and torch.equal(Va, Vb) and not torch.equal(Wa, W0) and flag.item() == 0
    hi, lo, _, _ = _split(Wb, 1)
    assert torch.equal(hi, wh) and torch.equal(lo, wl)
    assert L.idl_wgrad_rmsprop_planes(_p(dy), _p(x), m, H, F, None, _p(Wb), _p(Vb), _p(hyper), None, _p(wl), _p(flag), _stream()) != 0
    # ---- the batch assembly
    n, B, C, H2 = 700, 128, 5, 64
    feats = torch.randn(3, n, F, generator=g).to(dev)                          # the true view + two mimics
    mean = torch.randn(F, generator=g, dtype=torch.float64).to(dev); scale = (torch.rand(F, generator=g, dtype=torch.float64) + 0.5).to(dev)
    inv_scale = 1.0 / scale
    perm = torch.randperm(2 * n, generator=g).to(dev)
    base = torch.tensor([64], dtype=torch.int64, device=dev)
    want = torch.empty(2 * B, F, device=dev)
    _lib.check(L.idl_gather_pairs_at(_p(feats), n, F, n * F, _p(perm), _p(base), B, _p(mean), _p(scale), _p(inv_scale), _p(want), _stream()))
    mm = 2 * B
    y = torch.zeros(mm, F, device=dev); yh = torch.zeros(mm, F, dtype=torch.int16, device=dev); yl = torch.zeros_like(yh)
    xflag = torch.zeros(1, dtype=torch.int32, device=dev)
    a1 = torch.randn(8, 512, mm, generator=g).to(dev) * 0.1
    b1 = torch.zeros(512, device=dev)
    W2 = (torch.randn(H2, 512, generator=g) / 23).to(dev); b2 = torch.zeros(H2, device=dev)
    W3 = (torch.randn(C, H2, generator=g) / 8).to(dev); b3 = torch.zeros(C, device=dev)
    ctl = torch.zeros(2, dtype=torch.int64, device=dev)
    f = torch.empty(mm, H2, device=dev); inv = torch.empty(mm, device=dev); r2 = torch.empty(mm, H2, device=dev); z = torch.empty(mm, C, device=dev)
    def next_batch(p0, p1, **over):        # shares [p0, p1) of 8 of the batch at *base, as fp32 rows and as planes
        fields = dict(feats=_p(feats), n=n, f=F, view_stride=n * F, pair_idx=_p(perm), base=_p(base), base_add=0, n_pairs=2 * n, batch=B, mean=_p(mean),
                      scale=_p(scale), inv_scale=_p(inv_scale), y=_p(y), y_hi=_p(yh), y_lo=_p(yl), overflow_flag=_p(xflag), part=p0, part_end=p1, parts=8)
        fields.update(over)
        return _lib.idl_next_batch_t(**fields)

    _lib.check(L.idl_mid_fwd_gather(_p(a1), _p(b1), 1, _p(W2), _p(b2), _p(W3), _p(b3), mm, C, 1, ctypes.c_uint64(3), _p(ctl), _p(f), _p(inv), _p(r2), _p(z),
                                    next_batch(0, 3), _stream()))
    G = torch.randn(1, mm, H2, generator=g).to(dev) * 1e-2; dP0 = torch.randn(C, C, generator=g).to(dev) * 1e-2
    dlg = torch.empty(mm, C, device=dev); dlat = torch.empty(mm, H2, device=dev); dr1 = torch.empty(mm, 512, device=dev)
    parts = int(L.idl_col_sum_parts())
    p1 = torch.empty(parts, 512, device=dev); p2 = torch.empty(parts, H2, device=dev); p3 = torch.empty(parts, C, device=dev); pw3 = torch.empty(parts, C, H2, device=dev)
    _lib.check(L.idl_mid_bwd_gather(_p(z), _p(r2), _p(f), _p(inv), _p(G), 1, _p(dP0), _p(W3), _p(W2), _p(a1), mm, C, 1, 1e-3, _p(dlg), _p(dlat),
                                    _p(dr1), _p(p1), _p(p2), _p(p3), _p(pw3), 1, None, None, None, None, None, next_batch(3, 8, overflow_flag=None), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(y, want) and xflag.item() == 0
    hi, lo, _, _ = _split(y, 0)
    assert torch.equal(hi, yh) and torch.equal(lo, yl)
    # ---- mid_bwd writes dr1 as planes (round 6): idl_split_planes of the fp32 dr1 with the exponent it finds in word [1] of the scale's words -- the
    # default when a voter begins, afterwards what the dW1 launch derived from the previous step's maxima; the exponent used is left in word [0], the
    # workgroups' largest |dr1| in words [4..]; a dr1 beyond the planes' range (or not finite) raises the flag, one inside the 128 x headroom does not
    KF = int(L.idl_planes_exponent(2))
    sc = torch.zeros(int(L.idl_dr1_scale_words()), dtype=torch.int32, device=dev); sc[1] = KF
    dh = torch.zeros(mm, 512, dtype=torch.int16, device=dev); dl = torch.zeros_like(dh); dflag = torch.zeros(1, dtype=torch.int32, device=dev)

    def bwd(G_, dP0_, planes):
        out = None if planes else torch.empty(mm, 512, device=dev)
        dr1_planes = (_p(dh), _p(dl), _p(sc)) if planes else (None, None, None)
        _lib.check(L.idl_mid_bwd_gather(_p(z), _p(r2), _p(f), _p(inv), _p(G_), 1, _p(dP0_), _p(W3), _p(W2), _p(a1), mm, C, 1, 1e-3, _p(dlg), _p(dlat),
                                        _p(out), _p(p1), _p(p2), _p(p3), _p(pw3), 1, *dr1_planes, _p(dflag), None, None, _stream()))
        torch.cuda.synchronize()
        return out

    def split_k(v, k):
        a = torch.empty(v.shape, dtype=torch.int16, device=dev); b = torch.empty_like(a); fl = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.idl_split_planes(_p(v), v.numel(), k, _p(a), _p(b), _p(fl), _stream()))
        return a, b

    def k_of(v):                                                               # 2^k max|v| in [2^8, 2^9)
        return 9 - int(np.frexp(v.abs().max().item())[1])

    ref1 = bwd(G, dP0, False)
    assert torch.equal(ref1, dr1)
    p1_ref = p1.clone()
    bwd(G, dP0, True)
    assert sc[0].item() == KF == 10 and dflag.item() == 0 and torch.equal(p1, p1_ref)      # (the bias gradient's partial sums come from the unrounded values)
    a_, b_ = split_k(ref1, KF)
    assert torch.equal(a_, dh) and torch.equal(b_, dl)
    assert sc[4:].view(torch.float32).max().item() == ref1.abs().max().item()
    k2 = k_of(ref1)
    sc[1] = k2                                                                 # (what the dW1 launch leaves: below)
    ref3 = bwd(G * 10, dP0 * 10, False)                                        # a gradient several times larger, inside the headroom
    bwd(G * 10, dP0 * 10, True)
    assert sc[0].item() == k2 and dflag.item() == 0 and 2.0 < (ref3.abs().max() / ref1.abs().max()).item() < 100.0
    a_, b_ = split_k(ref3, k2)
    assert torch.equal(a_, dh) and torch.equal(b_, dl)
    back = (dh.view(torch.float16).double() + dl.view(torch.float16).double()) * 2.0 ** -k2
    assert ((back - ref3.double()).abs().max() / ref3.double().abs().max()).item() < 1e-6
    ref4 = bwd(G * 1e5, dP0 * 1e5, False)                                      # far beyond what the exponent expects: clamped, and said so
    bwd(G * 1e5, dP0 * 1e5, True)
    assert ref4.abs().max().item() * 2.0 ** k2 > 65000.0 and dflag.item() == 1
    assert bool(torch.isfinite(dh.view(torch.float16).float()).all())
    dflag.zero_()
    Gn = G.clone(); Gn[0, 3, 5] = float("nan")
    bwd(Gn, dP0, True)
    assert dflag.item() == 1                                                   # a dr1 that is not finite raises the flag too
    # a column whose originals barely vary: the standardised entries leave the planes' range, are clamped there, and the flag says so
    scale2 = scale.clone(); scale2[7] = 1e-9
    inv2 = 1.0 / scale2
    _lib.check(L.idl_mid_fwd_gather(_p(a1), _p(b1), 1, _p(W2), _p(b2), _p(W3), _p(b3), mm, C, 1, ctypes.c_uint64(3), _p(ctl), _p(f), _p(inv), _p(r2), _p(z),
                                    next_batch(0, 8, scale=_p(scale2), inv_scale=_p(inv2), y=None), _stream()))
    torch.cuda.synchronize()
    assert xflag.item() == 1
    col = yh.view(torch.float16)[:, 7].float()
    assert bool(torch.isfinite(col).all()) and col.abs().max().item() <= 65000.0


@pytest.mark.parametrize("m,H,F", [(512, 128, 512), (1024, 512, 4096), (192, 64, 128)])
def test_weight_gradient_from_the_planes_matches_the_fp32_tiles(dev, m, H, F):
    """idl_wgrad_rmsprop_xplanes (csrc/wgrad_planes.hip): dW = dy^T x + RMSprop with BOTH operands read as planes -- the batch's, and dy's as mid_bwd
    writes them, whatever power of two within the headroom they were scaled by.  The gradient is within 1e-6 of the float64 product's largest entry and,
    at the scale mid_bwd chooses, no further from it than the fp32 tiles'; the update agrees with the fp32 tiles'; W's planes are idl_split_planes of the
    updated W; the exponent of the NEXT step's planes is derived from the producer's maxima."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    g = torch.Generator(device="cpu"); g.manual_seed(17 + m)
    dy = (torch.randn(m, H, generator=g) * 1e-3 * torch.rand(m, 1, generator=g) ** 3).to(dev)
    dy = dy * (torch.rand(m, H, generator=g).to(dev) > 0.5)
    x = torch.randn(m, F, generator=g).to(dev)
    ref = dy.double().t() @ x.double()
    scale = ref.abs().max().item()
    hyper = torch.tensor([1e-3, 0.99, 1e-8, 0.01, 0.01], dtype=torch.float32, device=dev)
    W0 = (torch.randn(H, F, generator=g) * 0.02).to(dev)
    V0 = (torch.rand(H, F, generator=g) * 1e-6 + 1e-8).to(dev)
    assert L.idl_wgrad_xplanes_supported(m, H, F) == 1 and L.idl_wgrad_xplanes_supported(160, H, F) == 0 and L.idl_wgrad_xplanes_supported(128, H, F) == 0
    xh, xl, _, _ = _split(x, 0)
    g32, gpl = torch.empty(H, F, device=dev), torch.empty(H, F, device=dev)
    W32, V32, Wpl, Vpl = W0.clone(), V0.clone(), W0.clone(), V0.clone()
    _lib.check(L.idl_wgrad_rmsprop(_p(dy), _p(x), m, H, F, _p(g32), _p(W32), _p(V32), _p(hyper), _stream()))
    torch.cuda.synchronize()
    e32 = (g32.double() - ref).abs().max().item() / scale
    wh = torch.empty(H, F, dtype=torch.int16, device=dev); wl = torch.empty_like(wh); flag = torch.zeros(1, dtype=torch.int32, device=dev)
    e_max = int(np.frexp(dy.abs().max().item())[1])
    for k in (9 - e_max, 15 - e_max, 3 - e_max):
        dyh = torch.empty(m, H, dtype=torch.int16, device=dev); dyl = torch.empty_like(dyh); f2 = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.idl_split_planes(_p(dy), dy.numel(), k, _p(dyh), _p(dyl), _p(f2), _stream()))
        sc = torch.zeros(int(L.idl_dr1_scale_words()), dtype=torch.int32, device=dev)
        sc[0] = k; sc[1] = -77
        sc[4:] = (dy.abs().max() * torch.rand(64, generator=g).to(dev)).view(torch.int32); sc[4 + 13] = dy.abs().max().view(torch.int32)
        Wpl.copy_(W0); Vpl.copy_(V0); gpl.fill_(float("nan"))
        _lib.check(L.idl_wgrad_rmsprop_xplanes(_p(dyh), _p(dyl), _p(sc), _p(xh), _p(xl), F, m, H, F, _p(gpl), _p(Wpl), _p(Vpl), _p(hyper), _p(wh), _p(wl), _p(flag), _stream()))
        torch.cuda.synchronize()
        e = (gpl.double() - ref).abs().max().item() / scale
        assert f2.item() == 0 and e < 1e-6 and (k != 9 - e_max or e <= e32), (k, e, e32)
        assert torch.allclose(Vpl, V32, rtol=1e-4, atol=0.0) and (Wpl - W32).abs().max().item() < 2e-6
        hi, lo, _, _ = _split(Wpl, 1)
        assert torch.equal(hi, wh) and torch.equal(lo, wl) and flag.item() == 0
        assert sc[0].item() == k and sc[1].item() == 9 - e_max             # the next step's exponent, from the maxima: 2^k max in [2^8, 2^9)
    # the gradient alone, W untouched; an all-zero gradient: the default exponent for the next step
    sc[4:] = 0
    Wpl.copy_(W0)
    _lib.check(L.idl_wgrad_rmsprop_xplanes(_p(dyh), _p(dyl), _p(sc), _p(xh), _p(xl), F, m, H, F, _p(gpl), None, None, None, None, None, None, _stream()))
    torch.cuda.synchronize()
    assert sc[1].item() == int(L.idl_planes_exponent(2)) and torch.equal(Wpl, W0) and (gpl.double() - ref).abs().max().item() / scale < 1e-6
    assert L.idl_wgrad_rmsprop_xplanes(_p(dyh), None, _p(sc), _p(xh), _p(xl), F, m, H, F, _p(gpl), None, None, None, None, None, None, _stream()) != 0


def _store_and_net(dev, n, seed=3, C=20):
    import test_gpu_encoder as E
    return E._cfg2_store_and_net(dev, n, seed=seed, C=C)


@pytest.mark.parametrize("reduce", ["launch", "tail_beside_the_sums", "fp32_wgrad"])
def test_step_on_planes_trains_like_the_default_step(dev, monkeypatch, reduce):
    """IDELUCS_PLANES=1: the default launch sequence with the layer-1 product from two-plane operands.  (1) One step from the same state on the
    same batch: the loss within 2e-6, dr1 and dW1 within 2e-5 of their largest entries but for the few elements whose ReLU flips (a
    pre-activation within a rounding of zero).  (2) Two epochs (graph replay, dropout on): the loss sums follow the default step's within
    2e-4 relative; W1's planes are idl_split_planes of W1 at the end; nothing left the planes' range."""
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    store, net0 = _store_and_net(dev, 4096, seed=6, C=20)
    B = 512
    one, sums = {}, {}
    # the default (the sums as a launch, the tail on the dW1 kernel's loader waves) and the measured variants kept as switches
    monkeypatch.setitem(__import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS, "planes_tail", "reduce" if reduce == "tail_beside_the_sums" else "wgrad")
    monkeypatch.setitem(__import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS, "planes_wgrad", "0" if reduce == "fp32_wgrad" else "1")
    for flag in ("0", "1"):
        monkeypatch.setenv("IDELUCS_PLANES", flag)
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=5)
        assert tr._planes == (flag == "1")
        tr._keep_w1_grad = True
        tr._perm = torch.randperm(store.n_pairs, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        bf = tr.buffers(2 * B)
        tr._gather(store, bf)
        tr._full_step(store, bf, pipelined=True)
        torch.cuda.synchronize()
        one[flag] = (tr.out[0].item(), tr.dr1_of(bf).clone(), tr.grads[0].clone(), tr.W1.detach().clone())
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=5)
        gen = torch.Generator(device=dev); gen.manual_seed(123)
        s = []
        for _ in range(2):
            total, nb = tr.run_epoch(store, B, use_graph=True, generator=gen)
            s.append(total.item())
        sums[flag] = s
        if flag == "1":
            assert tr._w1_planes is not None and not tr.planes_overflowed()
            assert getattr(tr, "n_captures", 0) == 1
    (l0, d0, g0, w0), (l1, d1, g1, w1) = one["0"], one["1"]
    assert abs(l1 - l0) <= 2e-6 * abs(l0), (l0, l1)
    off = ((d1 - d0).abs() > 2e-5 * d0.abs().max()).sum().item()
    assert off <= 64, off                                                     # (of 524 288)
    # dW1 = dr1^T x: a row of it (a hidden unit) inherits what its column of dr1 differs by -- the rows of the units WITHOUT a flipped element agree
    # within 2e-5 of the largest entry, and no more rows than flipped elements are beyond that (VERDICT r5 #2c: counted, not excused by a 1e-3 maximum)
    flipped = ((d1 - d0).abs() > 2e-5 * d0.abs().max()).any(0)                # [512] hidden units
    gdiff = (g1 - g0).abs().max(1).values / g0.abs().max()
    assert flipped.sum().item() <= off and (gdiff[~flipped] < 2e-5).all(), (flipped.sum().item(), off, gdiff[~flipped].max().item())
    assert (gdiff[flipped] < 5e-3).all() and ((g1 - g0).abs().mean() / g0.abs().max()).item() < 2e-6
    # (the second epoch: two fp32-grade implementations of a product part at the rate the step amplifies a rounding -- a gradient differing
    #  by 1e-6 flips ReLU / Dropout patterns a step later; measured 2.1e-4 here, 2e-4 .. 5e-4 over the epochs of tools/bench_planes.py)
    for a_, b_, tol in zip(sums["0"], sums["1"], (2e-4, 1e-3)):              # (first epoch: 7e-6 .. 8e-5 over the variants)
        assert np.isfinite(b_) and abs(b_ - a_) <= tol * abs(a_), (sums,)


def test_planes_follow_the_weights_through_an_epoch(dev, monkeypatch):
    """After an epoch of the two-plane form (replayed graphs + eager steps + the partial last batch on the fp32 path) and into the next one,
    W1's planes at the point the next layer-1 product reads them are idl_split_planes of W1."""
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    store, net0 = _store_and_net(dev, 4200, seed=4, C=20)                      # 12 600 pairs: 24 full batches of 512 + a partial one
    tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=2)
    gen = torch.Generator(device=dev); gen.manual_seed(5)
    tr.run_epoch(store, 512, use_graph=True, generator=gen)
    assert not tr._w1_planes_fresh                                            # (the partial batch updated W1 on the fp32 path)
    tr.run_epoch(store, 512, use_graph=True, generator=gen)
    bf = tr.buffers(1024)
    tr.ctl[1:2].zero_()                                                       # (the batch offset stands at the end of the pair list)
    tr._gather(store, bf)
    tr._prepare_planes(bf, bf._planes, 0)
    torch.cuda.synchronize()
    wh, wl, flag = tr._w1_planes
    hi, lo, _, _ = _split(tr.W1.detach(), 1)
    assert torch.equal(hi, wh) and torch.equal(lo, wl) and flag.item() == 0
    xh, xl, _, _ = _split(bf.xs[0], 0)
    assert torch.equal(xh, bf._planes["xh"][0]) and torch.equal(xl, bf._planes["xl"][0])


def test_a_weight_beyond_the_planes_range_is_reported(dev, monkeypatch):
    """|w| >= 15.8 does not fit W1's planes (scale 2^12): the entry is clamped in the layer-1 product, the flag is raised by whoever writes the
    planes (idl_split_planes before the first step, the dW1 tiles' epilogue afterwards) and IID_model raises where it next waits for the device."""
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    store, net0 = _store_and_net(dev, 1100, seed=4, C=20)
    tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=2)
    gen = torch.Generator(device=dev); gen.manual_seed(5)
    tr.run_epoch(store, 512, use_graph=False, generator=gen)
    assert not tr.planes_overflowed()
    with torch.no_grad():
        tr.W1[3, 5] = 20.0
    tr.run_epoch(store, 512, use_graph=False, generator=gen)
    assert tr.planes_overflowed()
    from idelucs_amd import models

    class _M:                      # (IID_model._check_planes on a stand-in: the method only looks at _fused)
        _fused = tr
    with pytest.raises(RuntimeError, match="IDELUCS_PLANES=0"):
        models.IID_model._check_planes(_M())


def test_step_on_planes_at_k5_shape(dev, monkeypatch):
    """The two-plane step at k = 5's shape (F = 1024: two 64-deep chunks a K slice, the shortest the layer-1 tiles take) and a batch of 2 x 128
    rows: an epoch's loss follows the fp32 form's, the planes follow the weights."""
    import torch
    from idelucs_amd import utils as U, models
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.fused import FusedLinearTrainer
    g = torch.Generator(device=dev); g.manual_seed(11)
    P, n, F, C, B = 4, 2100, 1024, 12, 128
    base = torch.rand((1, n, F), device=dev, generator=g) + 0.5
    feats = base * (1.0 + 0.05 * torch.randn((P, n, F), device=dev, generator=g))
    feats = (feats / feats.sum(2, keepdim=True)).contiguous()
    mean, scale = U.col_stats(feats[0])
    store = U.FeatureStore(None, None, feats, mean, scale, 5, False)
    torch.manual_seed(3)
    net0 = NetLinear(F, C).to(dev); net0.apply(models.weights_init)
    sums = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("IDELUCS_PLANES", flag)
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=5)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        total, nb = tr.run_epoch(store, B, use_graph=True, generator=gen)
        sums[flag] = total.item() / nb
        if flag == "1":
            bf = tr.buffers(2 * B)
            assert getattr(bf, "_planes", None) is not None and tr._w1_planes is not None and not tr.planes_overflowed()
    assert np.isfinite(sums["1"]) and abs(sums["1"] - sums["0"]) <= 1e-3 * abs(sums["0"]), sums


def test_step_on_planes_with_200_output_units(dev, monkeypatch):
    """The fine-grained mode's step (n_clusters > 48: separate backward kernels, the whole next batch assembled by the mid-forward launch,
    activations not transposed) in its two-plane form: one step from the same state has the fp32 form's loss within 2e-6 and dW1 within 1e-3 (max) /
    2e-6 (mean) of the largest entry; two epochs follow the fp32 form's losses; the step counter and batch offset move as they do there."""
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    store, net0 = _store_and_net(dev, 4096, seed=6, C=200)
    B = 512
    one, sums = {}, {}
    for flag in ("0", "1"):
        monkeypatch.setenv("IDELUCS_PLANES", flag)
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=5)
        tr._keep_w1_grad = True
        tr._perm = torch.randperm(store.n_pairs, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        bf = tr.buffers(2 * B)
        tr._gather(store, bf)
        tr._full_step(store, bf, pipelined=True)
        torch.cuda.synchronize()
        one[flag] = (tr.out[0].item(), tr.grads[0].clone(), tr.ctl.tolist())
        if flag == "1":
            assert getattr(bf, "_planes", None) is not None and not bf._planes["x32"][1] and tr._w1_planes is not None
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=5)
        gen = torch.Generator(device=dev); gen.manual_seed(123)
        s_ = []
        for _ in range(2):
            total, nb = tr.run_epoch(store, B, use_graph=True, generator=gen)
            s_.append(total.item())
        sums[flag] = s_
        if flag == "1":
            assert not tr.planes_overflowed()
    (l0, g0, c0), (l1, g1, c1) = one["0"], one["1"]
    assert c0 == c1 == [1, B]
    assert abs(l1 - l0) <= 2e-6 * abs(l0), (l0, l1)
    assert ((g1 - g0).abs().max() / g0.abs().max()).item() < 1e-3 and ((g1 - g0).abs().mean() / g0.abs().max()).item() < 2e-6
    # (the step losses of this mode change sign inside an epoch and their sum nearly cancels: the bound is per step, on losses of ~0.3)
    # (round 6: the two forms also differ in the order the IIC joint's 512-row sums are formed -- its tiles ride in InfoNCE pass 1 in the plane form --,
    #  a rounding the epoch amplifies like any other: 1.5e-4 a step measured in the first epoch)
    for a_, b_, tol in zip(sums["0"], sums["1"], (3e-4, 1e-3)):
        assert np.isfinite(b_) and abs(b_ - a_) <= tol * nb, (sums,)


@pytest.mark.parametrize("n,graph,lanes", [(1500, False, 3), (4200, False, 3), (4200, True, 3), (4200, True, 2), (4200, True, 4), (4200, False, 8)])
def test_lockstep_voters_on_planes_are_the_lone_voters(dev, monkeypatch, n, graph, lanes):
    """IDELUCS_LOCKSTEP_PLANES=1: the voters of a rank (2, 3, 4, 8: what 8 voters over 4 / 2 / 1 GPUs put on a rank) in lockstep with the six launches of the two-plane step recorded and run once for
    all of them (blockIdx.y = voter) -- the same kernel bodies on the same operands in the same order as three lone voters: an epoch
    (8 or 24 full batches + a partial one, dropout on), launch by launch or as a captured graph, leaves the same loss sums, parameters
    and counters."""
    import torch
    import test_gpu_encoder as E
    from idelucs_amd.fused import FusedLinearTrainer, BatchedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    monkeypatch.setitem(__import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS, "lockstep_planes", "1")
    bt = E._batched_like_single(dev, n, graph, copy, torch, FusedLinearTrainer, BatchedLinearTrainer, L=lanes)
    assert bt._planes_step and bt.L == lanes
    assert not any(t.planes_overflowed() for t in bt.trainers)


@pytest.mark.parametrize("form", ["planes", "planes_fp32_wgrad", "fp32", "planes_200_units"])
def test_cold_caches_leave_an_epoch_bit_identical(dev, monkeypatch, form):
    """The regression test of round 5's loader race (wgrad_planes_device.h: a copy of the dy ring's registers in front of their wait):
    IDELUCS_TEST_COLD=1 puts a 512 MB fill in front of every step's mid_fwd, so that the loads of the launches behind it come from HBM
    instead of a warm L2/MALL.  An epoch's loss sum and parameters are then what they are with warm caches, bit for bit, three times in
    a row -- a kernel that consumes a load before it has landed passes every warm test and fails this one."""
    import torch
    import test_gpu_encoder as E
    from idelucs_amd.fused import FusedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", "0" if form == "fp32" else "1")
    monkeypatch.setitem(__import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS, "planes_wgrad", "0" if form == "planes_fp32_wgrad" else "1")
    store, net0 = E._cfg2_store_and_net(dev, 4200, seed=4, C=200 if form == "planes_200_units" else 20)
    runs = []
    for cold in ("0", "1", "1", "1"):
        monkeypatch.setitem(__import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS, "test_cold", cold)
        tr = FusedLinearTrainer(copy.deepcopy(net0), lr=1e-3, weight=0.25, lamb=2.8, seed=11)
        assert tr._cold == (cold == "1")
        tr.begin_voter(0)
        gen = torch.Generator(device=dev); gen.manual_seed(100)
        total, nb = tr.run_epoch(store, 512, use_graph=False, generator=gen)
        runs.append((total.item(), [p_.detach().clone() for p_ in tr.params]))
    for total, params in runs[1:]:
        assert total == runs[0][0], [r[0] for r in runs]
        for a_, b_ in zip(params, runs[0][1]):
            assert torch.equal(a_, b_)


def test_cold_caches_leave_lockstep_voters_the_lone_voters(dev, monkeypatch):
    """The same with the eviction in front of each of the six batched launches of three voters in lockstep."""
    import torch
    import test_gpu_encoder as E
    from idelucs_amd.fused import FusedLinearTrainer, BatchedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    monkeypatch.setitem(__import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS, "lockstep_planes", "1")
    monkeypatch.setitem(__import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS, "test_cold", "1")
    bt = E._batched_like_single(dev, 4200, False, copy, torch, FusedLinearTrainer, BatchedLinearTrainer)
    assert bt._planes_step and bt.trainers[0]._cold


def test_plane_products_on_adversarial_operands(dev):
    """VERDICT r5 #2b: both plane products against float64 where a fixed power-of-two scale and fp16's subnormal floor could bite (tools/planes_adversarial.py
    has the cases: columns and rows spanning 1e-6 .. 30, near-cancelling sums, entries whose low plane is subnormal, outliers at the end of the planes'
    range, sparse operands).  The claim, as measured (profiles/r06_planes_adversarial.txt): relative to the float64 product's LARGEST entry a plane
    product of standardised operands is within 7e-7 on every case, and on long dense sums (the training step's shape) it is closer than the fp32
    arithmetic it replaces, whose error grows with the sum's length (2.4e-7 against 2.6e-6; dW1 4.5e-7 against 1.5e-6).  On sums carried by a few
    terms (outliers, sparse operands) fp32 accumulation is exact to 2^-24 and the planes are up to twice as far (4.9e-7 against 2.6e-7): "fp32-grade",
    not "better than fp32".  Outside the contract -- a batch that is ~1e-4 THROUGHOUT, which a standardised batch is not -- the fixed 2^3 leaves the
    low plane in fp16's subnormals: 2e-5 (the fp32 tiles 3e-6)."""
    import os
    import sys
    import math
    import torch
    from idelucs_amd import _lib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from planes_adversarial import cases
    L = _lib.lib
    g = torch.Generator(device="cpu"); g.manual_seed(11)
    m, H, F = 1024, 512, 4096
    h16 = lambda t: torch.empty(t.shape, dtype=torch.int16, device=dev)
    seen = {}
    for name, W, x, dy in cases(m, H, F, g):
        W, x, dy = W.to(dev).contiguous(), x.to(dev).contiguous(), dy.to(dev).contiguous()
        wh, wl, xh, xl, flag = h16(W), h16(W), h16(x), h16(x), torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.idl_split_planes(_p(W), W.numel(), L.idl_planes_exponent(1), _p(wh), _p(wl), _p(flag), _stream()))
        _lib.check(L.idl_split_planes(_p(x), x.numel(), L.idl_planes_exponent(0), _p(xh), _p(xl), _p(flag), _stream()))
        part = torch.empty(int(L.idl_l1_planes_parts()), H, m, device=dev)
        _lib.check(L.idl_l1_planes(_p(wh), _p(wl), F, _p(xh), _p(xl), F, m, H, F, _p(part), _stream()))
        ref = W.double() @ x.double().t()
        s1 = ref.abs().max().item()
        e_pl = (part.double().sum(0) - ref).abs().max().item() / s1
        e_lib = ((W @ x.t()).double() - ref).abs().max().item() / s1
        refg = dy.double().t() @ x.double()
        s2 = refg.abs().max().item()
        g32, gpl = torch.empty(H, F, device=dev), torch.empty(H, F, device=dev)
        _lib.check(L.idl_wgrad_rmsprop(_p(dy), _p(x), m, H, F, _p(g32), None, None, None, _stream()))
        kd = 9 - math.frexp(dy.abs().max().item())[1]
        dyh, dyl = h16(dy), h16(dy)
        _lib.check(L.idl_split_planes(_p(dy), dy.numel(), kd, _p(dyh), _p(dyl), _p(flag), _stream()))
        sc = torch.zeros(int(L.idl_dr1_scale_words()), dtype=torch.int32, device=dev); sc[0] = kd
        _lib.check(L.idl_wgrad_rmsprop_xplanes(_p(dyh), _p(dyl), _p(sc), _p(xh), _p(xl), F, m, H, F, _p(gpl), None, None, None, None, None, None, _stream()))
        torch.cuda.synchronize()
        e_g = (gpl.double() - refg).abs().max().item() / s2
        e_32 = (g32.double() - refg).abs().max().item() / s2
        seen[name] = (e_pl, e_lib, e_g, e_32)
        assert flag.item() == 0, name
        if name.startswith("near-cancelling"):               # (the largest entry is itself what cancellation left: every arithmetic is noise there -- no worse than fp32's)
            assert e_pl <= 2.0 * e_lib and e_g <= 3.0 * e_32, (name, seen[name])
        elif name.startswith("low plane subnormal"):         # OUTSIDE the step's contract (x is standardised: |x| ~ 1): a batch that is 1e-4 throughout leaves
            assert e_pl < 1e-4 and e_g < 1e-4, (name, seen[name])      # its low plane in fp16's subnormals under the fixed 2^3 -- 14 bits, the documented limit
        else:
            assert e_pl < 7e-7 and e_g < 7e-7, (name, seen[name])
    # the step's own regime (dense standardised operands, sums of 4096 / 1024 products): closer than the fp32 arithmetic
    e_pl, e_lib, e_g, e_32 = seen["plain"]
    assert e_pl <= e_lib and e_g <= e_32, seen["plain"]
    print({k: tuple(f"{v:.1e}" for v in t) for k, t in seen.items()})


def test_data_beyond_the_planes_range_falls_back_to_the_fp32_tiles(dev, monkeypatch, capsys):
    """a dataset the reference handles must not fail after a full training pass.  A standardised feature beyond +-8125 (here: a
    column whose scale is made tiny, as a k-mer absent from nearly every original gives) raises the planes' flag; training.train_voter then switches
    the process to the fp32 tiles and trains the voter again from its start -- the result is bit for bit the IDELUCS_PLANES=0 run's, and new trainers
    of the process take the fp32 form."""
    import os
    import torch
    from idelucs_amd import fused, models, training
    import test_gpu_encoder as E
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)

    def model(planes):
        monkeypatch.setenv("IDELUCS_PLANES", planes)
        m = models.IID_model({'sequence_file': os.path.join(E.DATA, "Influenza-A.fas"), 'GT_file': None, 'n_clusters': 5, 'k': 6,
                              'model_size': 'linear', 'n_mimics': 3, 'batch_sz': 512, 'optimizer': 'RMSprop', 'lambda': 2.8,
                              'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 2, 'n_voters': 1, 'seed': 3})
        m.build_dataloader()
        col = 77
        m.store.scale[col] = m.store.scale[col] * 1e-7                           # the column's standardised entries: ~1e7 standard deviations
        m.store.inv_scale[col] = 1.0 / m.store.scale[col]
        return m

    m1 = model("1")
    curve1, y1, p1, lat1 = training.train_voter(m1, 2, voter=0, n_voters=1, progress=False)
    assert "fp32 tiles" in capsys.readouterr().err
    assert fused._PLANES_DISABLED and not m1._fused._planes and not m1._fused.planes_overflowed()
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
    m0 = model("0")
    curve0, y0, p0, lat0 = training.train_voter(m0, 2, voter=0, n_voters=1, progress=False)
    assert curve1 == curve0 and np.array_equal(y1, y0) and np.array_equal(lat1, lat0)
    for a, b in zip(m1.net.parameters(), m0.net.parameters()):
        assert torch.equal(a, b)
    # without the fall-back (a caller driving the epochs itself): the exception names what happened
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
    m2 = model("1")
    m2.begin_voter(0)
    with pytest.raises(models.PlanesOverflow):
        m2.contrastive_training_epoch()
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
