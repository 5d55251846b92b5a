"""The MFMA product kernels element by element on exact operands (tests/tiles_ref.py): idl_l1_fwd, idl_wgrad_rmsprop(_planes), idl_l1_planes(_rows),
idl_wgrad_rmsprop_xplanes and idl_at_b against float64 products, BIT FOR BIT -- the operands are small integers, so every partial sum is exact in
fp32 and the order of the additions cannot show (test_tiles_reference.py checks that condition for every case run here).  A mismatch is a wrong
index, and the message names the element, its tile, its place in the tile and, for the K-sliced partial sums, the slice.

Every operand sits inside a larger buffer whose other bytes are NaN (rows in front of and behind it; the pad columns [n_in, ld) of a plane hold the fp16
NaN 0x7E00): one element read from outside an operand makes a whole row or column of the result NaN.  Every output sits between guard regions of a
sentinel.  The shapes are the edges *_supported admits (tiles_ref.SHAPES: the ring of wgrad_loop.inc exactly full, nc == STAGES, one tile, both tile
maps, the workload's width) and the leading dimensions the plane kernels accept but no other test passes.

The RMSprop epilogue (fused calls).  The gradient is exact, so the update is tested on its own against tiles_ref.rmsprop64 (float64).  The bars, from
the operation count, in units of u = 2^-24:
  V = alpha V + (1 - alpha) gi^2, gi = g + wd W: a correctly rounded fp32 replay (tiles_ref.rmsprop32) deviates by at most 4.1 u relative;
  W -= lr gi / (sqrt(V) + eps): that replay deviates by at most 0.5 ulp(W) (the last rounding) + 3.5 u of the step;
  the kernels use v_sqrt_f32 and v_rcp_f32 (wgrad_device.h: 1 ulp each, 2 u each on the step), and FMA contraction may move single roundings;
  so V within 8 u relative, W within 0.5 ulp(W) + 12 u |step|.  The start has |W| <= 1, W != 0 with the gradient's sign and V >= 0: g + wd W never cancels.
The largest deviation seen is printed in these units (MI355X: idl_wgrad_rmsprop V 3.52, W 3.69; idl_wgrad_rmsprop_xplanes V 3.47, W 4.01; the fp32 replay
on the CPU: 3.65 and 3.27)."""
import ctypes

import numpy as np
import pytest

import tiles_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
SENT16 = 0x5555
GUARD = 4096              # guard elements on either side of an output
PAD_ROWS = 8              # NaN rows in front of and behind an operand
HYPERS = ((1e-3, 0.99), (0.25, 0.9))      # (lr, alpha): a step far below an ulp of W, and one larger than W


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    L = _lib.lib
    assert (L.idl_planes_exponent(0), L.idl_planes_exponent(1), L.idl_l1_planes_parts()) == (R.X_EXP, R.W_EXP, R.KSPLIT)
    return torch.device("cuda:0")


def _L():
    from idelucs_amd import _lib
    return _lib, _lib.lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    import torch
    torch.cuda.synchronize()


def _framed(a, ld, dev):
    """Operand a [rows][cols] (fp32, or a plane's int16 image) with leading dimension ld inside a buffer that is NaN everywhere else: PAD_ROWS rows in
    front and behind, the pad columns -> (the buffer: keep it alive, pointer to a[0][0])."""
    import torch
    rows, cols = a.shape
    assert ld >= cols
    nan = np.float32("nan") if a.dtype == np.float32 else np.int16(R.NAN16)
    big = np.full((rows + 2 * PAD_ROWS, ld), nan, a.dtype)
    big[PAD_ROWS:PAD_ROWS + rows, :cols] = a
    t = torch.from_numpy(big).to(dev)
    return t, ctypes.c_void_p(t.data_ptr() + PAD_ROWS * ld * a.itemsize)


def _guarded(shape, dev, init=None, int16=False):
    """An output of `shape` between two guard regions, everything the sentinel (or `init` inside) -> (whole buffer, the output's view)."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT16 if int16 else SENTINEL, dtype=torch.int16 if int16 else torch.float32, device=dev)
    view = buf[GUARD:GUARD + n].view(*shape)
    if init is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(init)))
    return buf, view


def _intact(buf, view):
    s = SENTINEL if buf.is_floating_point() else SENT16
    n = view.numel()
    return bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + n:] == s).all())


def _untouched(*bufs):
    return all(bool((b == (SENTINEL if b.is_floating_point() else SENT16)).all()) for b in bufs)


def _same(view, want, kern, what):
    mm = R.first_mismatch(view.cpu().numpy(), want, R.TILES[kern])
    assert mm["count"] == 0, R.describe(mm, what)


def _split(W, dev):
    """idl_split_planes of W with W1's exponent -> (hi, lo, flag)"""
    import torch
    _lib, L = _L()
    Wc = W.contiguous()
    hi = torch.empty(Wc.shape, dtype=torch.int16, device=dev); lo = torch.empty_like(hi)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.idl_split_planes(_p(Wc), Wc.numel(), R.W_EXP, _p(hi), _p(lo), _p(flag), _stream()))
    _sync()
    return hi, lo, flag


def _check_update(W, V, g, W0, V0, hy, what, seen):
    dv, dw = R.epilogue_deviation(W.cpu().numpy(), V.cpu().numpy(), g, W0, V0, hy)
    seen[0], seen[1] = max(seen[0], dv), max(seen[1], dw)
    assert dv <= R.V_BAR and dw <= R.W_BAR, f"{what}: V off by {dv:.2f} x 2^-24 relative (bar {R.V_BAR}), W by 0.5 ulp + {dw:.2f} x 2^-24 |step| (bar {R.W_BAR})"


def _report(name, seen):
    print(f"\n  {name}: epilogue's largest deviation from float64: V {seen[0]:.2f} x 2^-24 relative, W 0.5 ulp + {seen[1]:.2f} x 2^-24 |step|")


# ---------------------------------------------------------------- idl_l1_fwd

@pytest.mark.parametrize("m,n_in", R.SHAPES["l1_fwd"])
def test_l1_fwd_is_the_float64_product(dev, m, n_in):
    """(32, 192): the smallest, nc == STAGES (prologue and epilogue only); (96, 192): n_rt = 3, the plain tile map; (128, 320): n_rt = 4, the smallest
    XCD-mapped grid, nc = 5 (leaves the unrolled loop in its middle); (256, 4096): the workload's width."""
    _lib, L = _L()
    assert L.idl_l1_fwd_supported(m, R.H1, n_in) == 1
    for case in R.CASES:
        o = R.operands("l1_fwd", (m, n_in), case)
        tw, pw = _framed(o["W"], n_in, dev)
        tx, px = _framed(o["x"], n_in, dev)
        buf, out = _guarded((R.H1, m), dev)
        _lib.check(L.idl_l1_fwd(pw, px, m, n_in, _p(out), _stream()))
        _sync()
        _same(out, R.reference("l1_fwd", (m, n_in), case), "l1_fwd", f"idl_l1_fwd m={m} n_in={n_in} {case} [hidden unit][batch row]")
        assert _intact(buf, out)


# ---------------------------------------------------------------- idl_wgrad_rmsprop, idl_wgrad_rmsprop_planes

@pytest.mark.parametrize("m,H,F", R.SHAPES["wgrad"])
def test_wgrad_is_the_float64_product_and_its_update_the_float64_update(dev, m, H, F, capsys):
    """(32, 64, 128): one tile, the register ring exactly full (the steady-state loop runs zero times); (64, 64, 128): one pass; (1024, 64, 128): a long
    contraction.  The gradient alone, then fused (with and without the gradient stored); at two shapes idl_wgrad_rmsprop_planes: the fused call's W and V
    bit for bit, planes that are idl_split_planes of that W."""
    import torch
    _lib, L = _L()
    assert L.idl_wgrad_supported(m, H, F) == 1
    seen = [0.0, 0.0]
    for case in R.CASES:
        o = R.operands("wgrad", (m, H, F), case)
        ref = R.reference("wgrad", (m, H, F), case)
        what = f"idl_wgrad_rmsprop m={m} n_out={H} n_in={F} {case}"
        td, pd = _framed(o["dy"], H, dev)
        tx, px = _framed(o["x"], F, dev)
        gbuf, g = _guarded((H, F), dev)
        _lib.check(L.idl_wgrad_rmsprop(pd, px, m, H, F, _p(g), None, None, None, _stream()))
        _sync()
        _same(g, ref, "wgrad", what + ", gradient only")
        assert _intact(gbuf, g)
        W0, V0 = R.rms_start(ref, ("wgrad", m, H, F, case))
        for i, (lr, alpha) in enumerate(HYPERS):
            hy = R.hyper(lr, alpha)
            hyper = torch.from_numpy(hy).to(dev)
            gbuf, g = _guarded((H, F), dev)
            wbuf, W = _guarded((H, F), dev, init=W0)
            vbuf, V = _guarded((H, F), dev, init=V0)
            _lib.check(L.idl_wgrad_rmsprop(pd, px, m, H, F, _p(g) if i == 0 else None, _p(W), _p(V), _p(hyper), _stream()))
            _sync()
            if i == 0:
                _same(g, ref, "wgrad", what + ", fused")
            else:
                assert _untouched(gbuf)
            assert _intact(gbuf, g) and _intact(wbuf, W) and _intact(vbuf, V)
            _check_update(W, V, ref, W0, V0, hy, what + f" lr={lr}", seen)
            if (m, H, F) in ((96, 128, 256), (32, 512, 4096)):
                w2buf, W2 = _guarded((H, F), dev, init=W0)
                v2buf, V2 = _guarded((H, F), dev, init=V0)
                hbuf, wh = _guarded((H, F), dev, int16=True)
                lbuf, wl = _guarded((H, F), dev, int16=True)
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                _lib.check(L.idl_wgrad_rmsprop_planes(pd, px, m, H, F, None, _p(W2), _p(V2), _p(hyper), _p(wh), _p(wl), _p(flag), _stream()))
                _sync()
                assert torch.equal(W2, W) and torch.equal(V2, V) and flag.item() == 0, what + " _planes"
                hi, lo, f2 = _split(W2, dev)
                assert torch.equal(hi, wh) and torch.equal(lo, wl) and f2.item() == 0, what + " _planes: W's planes"
                assert _intact(w2buf, W2) and _intact(v2buf, V2) and _intact(hbuf, wh) and _intact(lbuf, wl)
    with capsys.disabled():
        _report(f"idl_wgrad_rmsprop {m}x{H}x{F}", seen)


# ---------------------------------------------------------------- idl_l1_planes, idl_l1_planes_rows

LD_PAIRS = ((0, 0), (8, 0), (0, 1024), (1024, 8))            # (ld_w - K, ld_x - K)


@pytest.mark.parametrize("m,H,K", R.SHAPES["l1_planes"])
def test_l1_planes_slices_are_the_float64_slices_at_every_leading_dimension(dev, m, H, K):
    """(128, 128, 1024): the smallest, nc == STAGES; (128, 128, 1536): nc = 3; two batch tiles; four hidden-unit tiles; several both ways.  Each with the
    leading dimensions (K, K), (K + 8, K), (K, K + 1024), (K + 1024, K + 8), the pad columns NaN; each of the eight slices on its own; _rows the transposed
    slices; one call with the operands' roles swapped (the batch as "W1": the step of n_clusters > 48)."""
    import torch
    _lib, L = _L()
    assert L.idl_l1_planes_supported(m, H, K) == 1 and L.idl_l1_planes_supported(H, m, K) == 1
    for case in R.CASES:
        o = R.operands("l1_planes", (m, H, K), case)
        ref = R.reference("l1_planes", (m, H, K), case)
        refT = np.ascontiguousarray(ref.transpose(0, 2, 1))
        for dw, dx in LD_PAIRS:
            ldw, ldx = K + dw, K + dx
            what = f"m={m} n_out={H} K={K} ld_w={ldw} ld_x={ldx} {case}"
            (t0, pwh), (t1, pwl) = _framed(o["wh"], ldw, dev), _framed(o["wl"], ldw, dev)
            (t2, pxh), (t3, pxl) = _framed(o["xh"], ldx, dev), _framed(o["xl"], ldx, dev)
            buf, part = _guarded((R.KSPLIT, H, m), dev)
            rbuf, rows = _guarded((R.KSPLIT, m, H), dev)
            _lib.check(L.idl_l1_planes(pwh, pwl, ldw, pxh, pxl, ldx, m, H, K, _p(part), _stream()))
            _lib.check(L.idl_l1_planes_rows(pwh, pwl, ldw, pxh, pxl, ldx, m, H, K, _p(rows), _stream()))
            _sync()
            _same(part, ref, "l1_planes", "idl_l1_planes " + what + " [slice][hidden unit][batch row]")
            _same(rows, refT, "l1_planes", "idl_l1_planes_rows " + what + " [slice][batch row][hidden unit]")
            assert torch.equal(rows, part.transpose(1, 2)) and _intact(buf, part) and _intact(rbuf, rows)
            if (dw, dx) == LD_PAIRS[-1]:
                sbuf, swapped = _guarded((R.KSPLIT, m, H), dev)
                _lib.check(L.idl_l1_planes(pxh, pxl, ldx, pwh, pwl, ldw, H, m, K, _p(swapped), _stream()))
                _sync()
                _same(swapped, refT, "l1_planes", "idl_l1_planes, roles swapped, " + what + " [slice][batch row][hidden unit]")
                assert _intact(sbuf, swapped)


# ---------------------------------------------------------------- idl_wgrad_rmsprop_xplanes

@pytest.mark.parametrize("m,H,F", R.SHAPES["xplanes"])
def test_wgrad_xplanes_is_the_float64_product_at_every_leading_dimension_and_scale(dev, m, H, F, capsys):
    """(192, 64, 128): m / 64 == NS, the three stages filled once; (256, 64, 128): one chunk beyond; several tiles; the full hidden width.  ld_x in
    {n_in, n_in + 8, n_in + 1024} with NaN pad columns; exponents 0, 10, -3 in word 0 of dy's scale words; the gradient alone, then fused with W's planes
    against idl_split_planes.  (The address case: one exponent per leading dimension.)"""
    import torch
    _lib, L = _L()
    assert L.idl_wgrad_xplanes_supported(m, H, F) == 1
    words = int(L.idl_dr1_scale_words())
    seen = [0.0, 0.0]
    for case in R.CASES:
        o = R.operands("xplanes", (m, H, F), case)
        (t0, pdh), (t1, pdl) = _framed(o["dyh"], H, dev), _framed(o["dyl"], H, dev)
        for i, ldx in enumerate((F, F + 8, F + 1024)):
            (t2, pxh), (t3, pxl) = _framed(o["xh"], ldx, dev), _framed(o["xl"], ldx, dev)
            for k in (R.XPLANES_K if case == "dense" else (R.XPLANES_K[i],)):
                ref = R.reference("xplanes", (m, H, F), case, k)
                what = f"idl_wgrad_rmsprop_xplanes m={m} n_out={H} n_in={F} ld_x={ldx} k={k} {case}"
                sc = torch.zeros(words, dtype=torch.int32, device=dev); sc[0] = k; sc[1] = -77
                first = (m, H, F) == R.SHAPES["xplanes"][0] and case == "dense" and i == 0 and k == 0
                if first:                                     # the next step's exponent from the producer's maxima: 2^k' 5.0 in [2^8, 2^9)
                    mx = np.full(words - 4, 0.25, np.float32); mx[13] = 5.0
                    sc[4:] = torch.from_numpy(mx.view(np.int32)).to(dev)
                gbuf, g = _guarded((H, F), dev)
                _lib.check(L.idl_wgrad_rmsprop_xplanes(pdh, pdl, _p(sc), pxh, pxl, ldx, m, H, F, _p(g), None, None, None, None, None, None, _stream()))
                _sync()
                _same(g, ref, "xplanes", what + ", gradient only")
                assert _intact(gbuf, g) and sc[0].item() == k
                assert sc[1].item() == (9 - 3 if first else int(L.idl_planes_exponent(2)))
                W0, V0 = R.rms_start(ref, ("xplanes", m, H, F, case, k))
                lr, alpha = HYPERS[(i + R.XPLANES_K.index(k)) % 2]
                hy = R.hyper(lr, alpha)
                hyper = torch.from_numpy(hy).to(dev)
                g2buf, g2 = _guarded((H, F), dev)
                wbuf, W = _guarded((H, F), dev, init=W0)
                vbuf, V = _guarded((H, F), dev, init=V0)
                hbuf, wh = _guarded((H, F), dev, int16=True)
                lbuf, wl = _guarded((H, F), dev, int16=True)
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                _lib.check(L.idl_wgrad_rmsprop_xplanes(pdh, pdl, _p(sc), pxh, pxl, ldx, m, H, F, _p(g2), _p(W), _p(V), _p(hyper), _p(wh), _p(wl), _p(flag),
                                                       _stream()))
                _sync()
                _same(g2, ref, "xplanes", what + ", fused")
                _check_update(W, V, ref, W0, V0, hy, what + f" lr={lr}", seen)
                hi, lo, f2 = _split(W, dev)
                assert torch.equal(hi, wh) and torch.equal(lo, wl) and flag.item() == 0 and f2.item() == 0, what + ": W's planes"
                assert _intact(g2buf, g2) and _intact(wbuf, W) and _intact(vbuf, V) and _intact(hbuf, wh) and _intact(lbuf, wl)
    with capsys.disabled():
        _report(f"idl_wgrad_rmsprop_xplanes {m}x{H}x{F}", seen)


# ---------------------------------------------------------------- idl_at_b

@pytest.mark.parametrize("K", (1, 127, 128, 129, 511, 512, 513, 640))
def test_at_b_is_the_float64_product(dev, K):
    """K on either side of 128 and 512 (the blocks of the contraction dealt to the four waves) and (M, N) below, at and beyond a 16 x 16 tile; lda, ldb, ldo
    padded, the operands' pads NaN, the output's pad columns left at the sentinel."""
    _lib, L = _L()
    for (K_, M, N) in R.SHAPES["at_b"]:
        if K_ != K:
            continue
        lda, ldb, ldo = M + 3, N + 5, N + 7
        for case in R.CASES:
            o = R.operands("at_b", (K, M, N), case)
            ta, pa = _framed(o["A"], lda, dev)
            tb, pb = _framed(o["B"], ldb, dev)
            buf, out = _guarded((M, ldo), dev)
            _lib.check(L.idl_at_b(pa, lda, pb, ldb, K, M, N, _p(out), ldo, _stream()))
            _sync()
            _same(out[:, :N].contiguous(), R.reference("at_b", (K, M, N), case), "at_b", f"idl_at_b K={K} M={M} N={N} {case}")
            assert bool((out[:, N:] == SENTINEL).all()) and _intact(buf, out)


# ---------------------------------------------------------------- what *_supported refuses

def test_the_nearest_unsupported_shapes_are_refused_and_write_nothing(dev):
    import torch
    _lib, L = _L()
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
    i16 = lambda *shape: torch.zeros(*shape, dtype=torch.int16, device=dev)
    hyper = torch.from_numpy(R.hyper(1e-3, 0.99)).to(dev)
    # idl_l1_fwd: n_in = 128 (two chunks: fewer than the stages), m = 40
    W, x = f32(R.H1, 192), f32(64, 192)
    buf, out = _guarded((R.H1, 64), dev)
    for m, n_in in ((32, 128), (40, 192)):
        assert L.idl_l1_fwd_supported(m, R.H1, n_in) == 0
        assert L.idl_l1_fwd(_p(W), _p(x), m, n_in, _p(out), _stream()) != 0
    # idl_wgrad_rmsprop(_planes): m = 16 (half a ring), n_in = 64 (half a tile)
    dy, x = f32(32, 64), f32(32, 128)
    gbuf, g = _guarded((64, 128), dev); wbuf, Wt = _guarded((64, 128), dev); vbuf, V = _guarded((64, 128), dev)
    hbuf, wh = _guarded((64, 128), dev, int16=True); lbuf, wl = _guarded((64, 128), dev, int16=True)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for m, n_in in ((16, 128), (32, 64)):
        assert L.idl_wgrad_supported(m, 64, n_in) == 0
        assert L.idl_wgrad_rmsprop(_p(dy), _p(x), m, 64, n_in, _p(g), _p(Wt), _p(V), _p(hyper), _stream()) != 0
        assert L.idl_wgrad_rmsprop_planes(_p(dy), _p(x), m, 64, n_in, _p(g), _p(Wt), _p(V), _p(hyper), _p(wh), _p(wl), _p(flag), _stream()) != 0
    # idl_l1_planes(_rows): K = 512 (one chunk a slice), ld = K + 4 (not a multiple of 8), ld = K + 1032 (beyond K + 1024)
    K = 1024
    wp, xp = i16(128, K + 1032), i16(128, K + 1032)
    pbuf, part = _guarded((R.KSPLIT, 128, 128), dev)
    assert L.idl_l1_planes_supported(128, 128, 512) == 0
    for fn in (L.idl_l1_planes, L.idl_l1_planes_rows):
        assert fn(_p(wp), _p(wp), 512, _p(xp), _p(xp), 512, 128, 128, 512, _p(part), _stream()) != 0
        for ldw, ldx in ((K + 4, K), (K, K + 4), (K + 1032, K), (K, K + 1032)):
            assert fn(_p(wp), _p(wp), ldw, _p(xp), _p(xp), ldx, 128, 128, K, _p(part), _stream()) != 0
    # idl_wgrad_rmsprop_xplanes: m = 128 (two chunks: fewer than the stages); ld_x as above
    dyp, xq = i16(192, 64), i16(192, 128 + 1032)
    sc = torch.zeros(int(L.idl_dr1_scale_words()), dtype=torch.int32, device=dev); sc[1] = -77
    assert L.idl_wgrad_xplanes_supported(128, 64, 128) == 0
    for m, ldx in ((128, 128), (192, 128 + 4), (192, 128 + 1032)):
        assert L.idl_wgrad_rmsprop_xplanes(_p(dyp), _p(dyp), _p(sc), _p(xq), _p(xq), ldx, m, 64, 128, _p(g), _p(Wt), _p(V), _p(hyper), _p(wh), _p(wl), _p(flag),
                                           _stream()) != 0
    _sync()
    assert _untouched(buf, gbuf, wbuf, vbuf, hbuf, lbuf, pbuf) and flag.item() == 0 and sc[1].item() == -77
