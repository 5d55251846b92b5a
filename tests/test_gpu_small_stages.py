"""The five kernels of the small model's native step (csrc/small_step.hip), each launched alone through the C ABI and held, stage by
stage, to the float64 restatement in tests/small_ref.py (which tests/test_small_reference.py ties to torch autograd on the host).

STAGE ISOLATION.  Every reference value is formed in float64 from the float32 arrays the code under test read: the backward's da2 from
the dlogits and dh the kernel wrote, dr1 from its da2, the forward's a2 from its a1, and so on.  Signs of activations and masks are
then those the kernel saw, and each bar is one operation deep.

THE BARS.  A product is held to small_ref.product_bound ((K + 16) 2^-23 sum |a||b| + 2^-126, K the contraction length) and, with
operands drawn from -2..2, to the integer product bit for bit (every partial sum is then exact in float32, so a dropped, doubled or
misplaced term shows whatever the tolerance).  What is not a product is either restated in float32 bit for bit (layer 1's bias, ReLU
and Dropout in place; d2) or held to the product bound propagated to first order through the closed form and doubled; each
derivation stands beside its bar, with U = 2^-23 (one rounding is at most U / 2 of its result).  Every _hold() prints error / bar.

GUARD ROWS.  Every output has 16 rows (a vector: 1024 entries) of a sentinel behind it, which must survive the launch.

SHAPES are the smallest at which each tail exists: see the lists."""
import ctypes
import zlib

import numpy as np
import pytest

import small_ref as R
from small_ref import U, TINY, f64

pytestmark = pytest.mark.gpu

H1, H2, LAT = 400, 128, 64
GUARD = 16
SENTINEL = -7.0e11
SEED = 0x9E3779B97F4A7C15                        # a seed that needs all 64 bits
STEP = (3 << 24) + 5                             # a step counter with voter bits set (FusedSmallTrainer.begin_voter(3), 5 steps in)


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda")


def _gen(dev, *key):
    import torch
    return torch.Generator(device=dev).manual_seed(zlib.crc32(repr(key).encode()))


class _Guarded:
    """A float32 output of `shape` with the sentinel behind it; .t is the part the kernel may write."""

    def __init__(self, shape, dev, init=None):
        import torch
        shape = tuple(shape)
        extra = GUARD if len(shape) > 1 else 1024
        self.full = torch.full((shape[0] + extra,) + shape[1:], SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.full[:shape[0]]
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.full[self.t.shape[0]:] == SENTINEL).all())


def _hold(name, got, want, bar):
    """|got - want| <= bar elementwise; prints the worst error / bar (profiles/small_stages_bounds.txt collects these lines)."""
    got, want, bar = f64(got), np.asarray(want, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.all(np.isfinite(got)), name
    ratio = np.abs(got - want) / bar
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"RATIO {name} {worst:.4f}")
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    assert worst <= 1.0, (name, worst, at, got[at], want[at], bar[at])


def _ints(shape, dev, gen):
    import torch
    return torch.randint(-2, 3, shape, device=dev, generator=gen).float()


def _randn(shape, dev, gen, scale=1.0):
    import torch
    return torch.randn(shape, device=dev, generator=gen) * scale


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from idelucs_amd.fused import _stream as s
    return s()


def _masks(dev, m, step=STEP, seed=SEED):
    """The two keep masks of idl_small_dropout_masks as float32 0 / 1."""
    import torch
    from idelucs_amd import _lib
    m1, m2 = _Guarded((m, H1), dev), _Guarded((m, H2), dev)
    _lib.check(_lib.lib.idl_small_dropout_masks(seed, step, m, _p(m1.t), _p(m2.t), _stream()))
    torch.cuda.synchronize()
    assert m1.intact() and m2.intact()
    for mk in (m1.t, m2.t):
        assert bool(((mk == 0) | (mk == 1)).all())
    return m1.t.clone(), m2.t.clone()


# ================================================================================================ idl_small_l1_fwd
# fewer than eight 16-wide chunks (waves without a share), a chunk count that is no multiple of 8, a chunk that crosses F with
# F % 4 == 0 and != 0, m % 16 != 0, the widths of k = 4 .. 8 and of k = 8's canonical form
L1_SHAPES = [(1, 1), (2, 3), (16, 16), (17, 15), (18, 10), (31, 127), (33, 129), (48, 136), (62, 2080), (440, 512), (66, 32896)]


def _l1(dev, x, W1):
    import torch
    from idelucs_amd import _lib
    m, F = x.shape
    a1 = _Guarded((m, H1), dev)
    _lib.check(_lib.lib.idl_small_l1_fwd(_p(x), _p(W1), m, F, _p(a1.t), _stream()))
    torch.cuda.synchronize()
    assert a1.intact()
    return a1.t


@pytest.mark.parametrize("m,F", L1_SHAPES)
def test_l1_fwd_exact_on_small_integers(dev, m, F):
    """x, W1 in -2..2: |sum| <= 4 F < 2^24, every partial sum exact, the result is the integer product (float64 holds it exactly)."""
    g = _gen(dev, "l1i", m, F)
    x, W1 = _ints((m, F), dev, g), _ints((H1, F), dev, g)
    got = _l1(dev, x, W1)
    want = R.l1_fwd(x, W1)
    assert np.array_equal(want, np.rint(want)) and np.abs(want).max() < 2 ** 24
    assert np.array_equal(f64(got).astype(np.int64), want.astype(np.int64)) and np.array_equal(f64(got), want)


@pytest.mark.parametrize("m,F", L1_SHAPES)
def test_l1_fwd_random_within_the_product_bound(dev, m, F):
    import torch
    g = _gen(dev, "l1r", m, F)
    x, W1 = _randn((m, F), dev, g), _randn((H1, F), dev, g)
    got = _l1(dev, x, W1)
    want, bar = R.l1_fwd(x, W1), R.product_bound(x, W1.t())          # K = F
    _hold("l1_fwd a1'", got, want, bar)
    _hold("torch.mm l1", torch.mm(x, W1.t()), want, bar)              # (the bar is no tighter than a library product needs)


# ================================================================================================ idl_small_mid_fwd
MID_FWD_CASES = [(1, 1, 0), (2, 2, 1), (15, 5, 1), (16, 16, 0), (17, 17, 1), (34, 48, 1), (34, 49, 0), (440, 64, 1), (17, 65, 0),
                 (2, 200, 1), (34, 201, 1), (440, 256, 1), (16, 256, 0), (1, 49, 1), (15, 200, 0), (440, 5, 0)]


def test_mid_fwd_cases_cover_the_lists():
    assert {c[0] for c in MID_FWD_CASES} == {1, 2, 15, 16, 17, 34, 440}
    assert {c[1] for c in MID_FWD_CASES} == {1, 2, 5, 16, 17, 48, 49, 64, 65, 200, 201, 256}
    assert {c[2] for c in MID_FWD_CASES} == {0, 1}


@pytest.mark.parametrize("m,C,train", MID_FWD_CASES)
def test_mid_fwd_stage_by_stage(dev, m, C, train):
    import torch
    from idelucs_amd import _lib
    g = _gen(dev, "fwd", m, C, train)
    a1_pre = _randn((m, H1), dev, g)
    b1, W2, b2 = _randn((H1,), dev, g, 0.5), _randn((H2, H1), dev, g, 0.07), _randn((H2,), dev, g, 0.5)
    Wi, bi, Wc, bc = _randn((LAT, H2), dev, g, 0.1), _randn((LAT,), dev, g, 0.3), _randn((C, H2), dev, g, 0.3), _randn((C,), dev, g, 0.5)
    ctl = torch.tensor([STEP, 41], dtype=torch.int64, device=dev)
    masks = _masks(dev, m) if train else None
    a1 = _Guarded((m, H1), dev, init=a1_pre)
    a2, d2, f, inv, z = (_Guarded(s, dev) for s in ((m, H2), (m, H2), (m, LAT), (m,), (m, C)))
    _lib.check(_lib.lib.idl_small_mid_fwd(_p(a1.t), _p(b1), _p(W2), _p(b2), _p(Wi), _p(bi), _p(Wc), _p(bc), m, C, train, SEED, _p(ctl),
                                          _p(a2.t), _p(d2.t), _p(f.t), _p(inv.t), _p(z.t), _stream()))
    torch.cuda.synchronize()
    for o in (a1, a2, d2, f, inv, z):
        assert o.intact()
    assert ctl.tolist() == [STEP, 41]
    # ---- a1 = Dropout(ReLU(a1' + b1)) in place: float32, one add, one compare, one exact product with 0 / 1 / 2
    t = a1_pre + b1
    want_a1 = torch.where(t > 0, t * (2.0 * masks[0] if train else torch.ones_like(t)), torch.zeros_like(t))
    assert torch.equal(a1.t, want_a1)
    if train:
        assert bool((a1.t[masks[0] == 0] == 0).all())
    # ---- a2 = LeakyReLU(v), v = a1 W2^T + b2 (K = 400).  e_v = product bound + U (|a1 W2^T| + |b2|) for the added bias (U / 2 of the
    # sum would do).  LeakyReLU is 1-Lipschitz, so a v whose sign the error flips still lands within e_v; the slope 0.01f is 0.01 to
    # 2^-24 relative and its product rounds once: + 2 U |a2|.  Doubled.
    a1k = f64(a1.t)
    pre = a1k @ f64(W2).T
    v = pre + f64(b2)
    want_a2 = np.where(v > 0, v, R.SLOPE * v)
    e_v = R.product_bound(a1k, f64(W2).T) + U * (np.abs(pre) + np.abs(f64(b2)))
    _hold("mid_fwd a2", a2.t, want_a2, 2 * (e_v + 2 * U * np.abs(want_a2)))
    # ---- d2 = Dropout(a2): float32, an exact product with 0 / 1 / 2
    assert torch.equal(d2.t, a2.t * 2.0 * masks[1] if train else a2.t)
    # ---- h = a2 Wi^T + bi (K = 128), n = |h| over 64 entries, f = h / n, inv = 1 / n.  e_h as e_v.  n: d n = (h . d h) / n, and the
    # 64 squares, their sum (2 + 6 levels across the wave) and the root round 64 + 8 + 1 times at most, each U / 2 of n^2 or of n:
    # rel_n = (|h| . e_h) / n^2 + 40 U.  f = h / n: e_f = e_h / n + |f| (rel_n + U);  inv: inv (rel_n + U).  Doubled.
    a2k = f64(a2.t)
    pre = a2k @ f64(Wi).T
    h = pre + f64(bi)
    e_h = R.product_bound(a2k, f64(Wi).T) + U * (np.abs(pre) + np.abs(f64(bi)))
    n = np.sqrt((h * h).sum(1))
    assert n.min() > 1e-6                                 # (F.normalize's clamp at 1e-12 is out of reach of these inputs)
    rel_n = (np.abs(h) * e_h).sum(1) / n ** 2 + 40 * U
    _hold("mid_fwd f", f.t, h / n[:, None], 2 * (e_h / n[:, None] + np.abs(h / n[:, None]) * (rel_n[:, None] + U)) + TINY)
    _hold("mid_fwd inv", inv.t, 1.0 / n, 2 * (rel_n + U) / n)
    # ---- z = softmax(l), l = d2 Wc^T + bc (K = 128), from the kernel's d2.  e_l as e_v.  z_c = e_c / sum_j e_j with e_c = exp(l_c - max):
    # an error of l_c is a relative error of e_c; the subtraction rounds once and __expf is exp2 of a once-rounded argument:
    # (4 + |l_c - max|) U relative.  rel_c = e_l[c] + (4 + |l_c - max|) U.  The sum of C terms (4 a lane, 6 levels across the wave) has
    # the z-weighted mean of the rel_j plus 10 roundings, the quotient one more: e_z = z_c (rel_c + sum_j z_j rel_j + 12 U).  Doubled.
    d2k = f64(d2.t)
    pre = d2k @ f64(Wc).T
    lg = pre + f64(bc)
    e_l = R.product_bound(d2k, f64(Wc).T) + U * (np.abs(pre) + np.abs(f64(bc)))
    sh = lg - lg.max(1, keepdims=True)
    want_z = np.exp(sh) / np.exp(sh).sum(1, keepdims=True)
    rel = e_l + (4 + np.abs(sh)) * U
    _hold("mid_fwd z", z.t, want_z, 2 * want_z * (rel + (want_z * rel).sum(1, keepdims=True) + 12 * U) + TINY)


# ================================================================================================ idl_small_mid_bwd
# route: "lds" (dzs = NULL, C <= 48: dP0 and the partner rows of z in LDS), "dzs" (z dP0 given per row), "global" (dzs = NULL,
# C > 48: both read from global memory).  (route, m, C, g_parts, train, batch_advance, general dP0)
# The issue's clause that the LDS and the global route agree bit for bit at C <= 48 is not tested: with dzs = NULL the kernel picks
# the route from C alone, so the global one cannot be reached there without changing the kernel.
MID_BWD_CASES = [("lds", 2, 1, 1, 0, 0, False), ("lds", 6, 5, 2, 1, 7, False), ("lds", 18, 16, 16, 0, 0, False),
                 ("lds", 34, 17, 1, 1, 7, True), ("lds", 62, 48, 2, 1, 0, False), ("lds", 440, 48, 16, 0, 7, False),
                 ("dzs", 6, 5, 1, 1, 7, True), ("dzs", 18, 49, 1, 1, 0, False), ("dzs", 34, 130, 2, 0, 7, False),
                 ("dzs", 440, 200, 16, 1, 0, False),
                 ("global", 2, 49, 1, 0, 0, False), ("global", 6, 130, 2, 1, 7, True), ("global", 18, 201, 16, 1, 0, False),
                 ("global", 34, 256, 1, 0, 7, False), ("global", 62, 49, 16, 1, 7, False), ("global", 440, 130, 2, 1, 0, False),
                 ("global", 440, 256, 1, 1, 7, False), ("global", 18, 256, 2, 0, 0, True)]


def test_mid_bwd_cases_cover_the_lists():
    assert {c[1] for c in MID_BWD_CASES} == {2, 6, 18, 34, 62, 440}
    assert {c[2] for c in MID_BWD_CASES if c[0] == "global"} == {49, 130, 201, 256}
    assert {c[3] for c in MID_BWD_CASES} == {1, 2, 16} and {c[4] for c in MID_BWD_CASES} == {0, 1}
    assert {c[5] for c in MID_BWD_CASES} == {0, 7}
    for route in ("lds", "dzs", "global"):
        assert any(c[0] == route and c[6] for c in MID_BWD_CASES)
        assert all((c[2] <= 48) == (route == "lds") for c in MID_BWD_CASES if c[0] == route and route != "dzs")


@pytest.mark.parametrize("route,m,C,parts,train,adv,general", MID_BWD_CASES)
def test_mid_bwd_stage_by_stage(dev, route, m, C, parts, train, adv, general):
    import torch
    from idelucs_amd import _lib
    g = _gen(dev, "bwd", route, m, C, parts, train, adv)
    z = torch.softmax(_randn((m, C), dev, g, 2.0), dim=1)
    f = torch.nn.functional.normalize(_randn((m, LAT), dev, g), dim=1)
    inv = 0.2 + torch.rand((m,), device=dev, generator=g)
    G = _randn((parts, m, LAT), dev, g)
    dP0 = _randn((C, C), dev, g)
    if not general:
        dP0 = ((dP0 + dP0.t()) / 2).contiguous()              # symmetric, as in use
    dzs = _randn((m, C), dev, g) if route == "dzs" else None  # (any array: only "row partner(r) of dzs" is the kernel's business)
    a1 = torch.relu(_randn((m, H1), dev, g)) * (torch.rand((m, H1), device=dev, generator=g) < 0.5)
    a2 = _randn((m, H2), dev, g)
    a2 = torch.where(a2 > 0, a2, 0.01 * a2)
    a2[0, :4] = 0.0                                            # LeakyReLU'(0) = slope
    W2, Wi, Wc = _randn((H2, H1), dev, g, 0.07), _randn((LAT, H2), dev, g, 0.1), _randn((C, H2), dev, g, 0.3)
    nce_coef = float(np.float32(0.75 / (m * 0.85)))
    mask2 = _masks(dev, m)[1] if train else None
    ctl = torch.tensor([STEP, 100], dtype=torch.int64, device=dev)
    dlogits, dh, da2, dr1 = (_Guarded(s, dev) for s in ((m, C), (m, LAT), (m, H2), (m, H1)))
    _lib.check(_lib.lib.idl_small_mid_bwd(_p(z), _p(f), _p(inv), _p(G), parts, _p(None if route == "dzs" else dP0), _p(dzs), _p(a1), _p(a2),
                                          _p(W2), _p(Wi), _p(Wc), m, C, train, nce_coef, SEED, _p(ctl), adv,
                                          _p(dlogits.t), _p(dh.t), _p(da2.t), _p(dr1.t), _stream()))
    torch.cuda.synchronize()
    for o in (dlogits, dh, da2, dr1):
        assert o.intact()
    assert ctl.tolist() == [STEP, 100 + adv]                  # advanced exactly once, by one workgroup
    pr = R.partner(m)
    z6, f6, inv6 = f64(z), f64(f), f64(inv)
    want_dl, want_dh = R.bwd_rows(z, f, inv, G, dP0, nce_coef, dzs)
    # ---- dlogits = z (dz - dot), dz = z_partner dP0 (K = C; a row of dzs: exact), dot = sum_c dz_c z_c.  e_dz: the product bound.
    # dot: C products and a sum of 4 a lane and 6 levels: e_dot = sum_c z_c e_dz[c] + 12 U sum_c |dz_c z_c|.  The difference and the
    # product round once each: e = z_c (e_dz[c] + e_dot + U |dz_c - dot|) + U |dlogits|.  Doubled.
    dz = f64(dzs)[pr] if dzs is not None else z6[pr] @ f64(dP0)
    e_dz = np.zeros_like(dz) if dzs is not None else R.product_bound(z6[pr], f64(dP0))
    dot = (dz * z6).sum(1, keepdims=True)
    e_dot = (z6 * e_dz).sum(1, keepdims=True) + 12 * U * np.abs(dz * z6).sum(1, keepdims=True)
    _hold(f"mid_bwd dlogits ({route})", dlogits.t, want_dl, 2 * (z6 * (e_dz + e_dot + U * np.abs(dz - dot)) + U * np.abs(want_dl)) + TINY)
    # ---- dh = (df - f proj) inv, df = coef (gs - 2 f_partner), gs = the parts of G added in order, proj = sum_64 f df.
    # e_gs = (parts - 1) U sum_p |G_p|;  e_df = coef (e_gs + U |gs - 2 f_p|) + U |df|;  e_proj = sum |f| e_df + 8 U sum |f df|
    # (a product and 6 levels);  e = inv (e_df + |f| e_proj + U |f proj| + U |df - f proj|) + U |dh|.  Doubled.
    G6 = f64(G)
    gs = G6.sum(0)
    e_gs = (parts - 1) * U * np.abs(G6).sum(0)
    df = nce_coef * (gs - 2 * f6[pr])
    e_df = nce_coef * (e_gs + U * np.abs(gs - 2 * f6[pr])) + U * np.abs(df)
    proj = (f6 * df).sum(1, keepdims=True)
    e_proj = (np.abs(f6) * e_df).sum(1, keepdims=True) + 8 * U * np.abs(f6 * df).sum(1, keepdims=True)
    e_dh = inv6[:, None] * (e_df + np.abs(f6) * e_proj + U * np.abs(f6 * proj) + U * np.abs(df - f6 * proj)) + U * np.abs(want_dh)
    _hold("mid_bwd dh", dh.t, want_dh, 2 * e_dh + TINY)
    # ---- da2 = (k (dlogits Wc) + dh Wi) s from the kernel's dlogits and dh: k = 0 / 1 / 2 the classifier's mask, s = 1 or the slope
    # by the sign of a2 (an input).  e = s (k bound_C + bound_64 + U |sum|) + 2 U |da2| (the slope constant and its product).  Doubled.
    k2 = 2.0 * f64(mask2) if train else 1.0
    s2 = np.where(f64(a2) > 0, 1.0, R.SLOPE)
    want_da2 = R.bwd_da2(dlogits.t, dh.t, a2, Wi, Wc, mask2, bool(train))
    e_da2 = s2 * (k2 * R.product_bound(dlogits.t, Wc) + R.product_bound(dh.t, Wi) + U * np.abs(want_da2 / s2)) + 2 * U * np.abs(want_da2)
    _hold("mid_bwd da2", da2.t, want_da2, 2 * e_da2 + TINY)
    # ---- dr1 = k (da2 W2) where a1 > 0 (K = 128; k = 2 with dropout, exact), 0 elsewhere, from the kernel's da2.  Doubled.
    want_dr1 = R.bwd_dr1(da2.t, a1, W2, bool(train))
    _hold("mid_bwd dr1", dr1.t, want_dr1, 2 * (2.0 if train else 1.0) * R.product_bound(da2.t, W2))
    assert bool((dr1.t[a1 <= 0] == 0).all())


# ================================================================================================ idl_small_wgrad_rms(_momentum)
WGRAD_CASES = [(2, 1, 1), (6, 10, 5), (18, 63, 31), (30, 65, 33), (34, 136, 200), (66, 2080, 256), (250, 1, 256), (440, 10, 200),
               (1022, 63, 5), (1022, 2080, 1), (18, 136, 33), (2, 65, 31)]
HYPER = [1e-3, 0.99, 1e-8, 0.01, 1.0 - 0.99, 0.9]           # lr, alpha, eps, weight decay, 1 - alpha, momentum
JOBS = (("dr1", "x"), ("da2", "a1"), ("dh", "a2"), ("dlogits", "d2"))


def test_wgrad_cases_cover_the_lists():
    assert {c[0] for c in WGRAD_CASES} == {2, 6, 18, 30, 34, 66, 250, 440, 1022}
    assert {c[1] for c in WGRAD_CASES} == {1, 10, 63, 65, 136, 2080}
    assert {c[2] for c in WGRAD_CASES} == {1, 5, 31, 33, 200, 256}


class _Wgrad:
    """The operands and the state of idl_small_wgrad_rms / _momentum at one shape, every written tensor guarded."""

    def __init__(self, dev, m, F, C, mom, gen):
        import torch
        self.dev, self.m, self.F, self.C, self.mom, self.gen = dev, m, F, C, mom, gen
        self.shapes = [(H1, F), (H1,), (H2, H1), (H2,), (LAT, H2), (LAT,), (C, H2), (C,)]
        self.params = [_Guarded(s, dev, init=_randn(s, dev, gen, 0.1)) for s in self.shapes]
        self.sq, self.buf, self.grads = ([_Guarded(s, dev, init=torch.zeros(s, device=dev)) for s in self.shapes] for _ in range(3))
        self.hyper = torch.tensor(HYPER if mom else HYPER[:5], dtype=torch.float32, device=dev)
        self.ctl = torch.tensor([STEP, 17], dtype=torch.int64, device=dev)
        self.widths = dict(x=F, a1=H1, a2=H2, d2=H2, dr1=H1, da2=H2, dh=LAT, dlogits=C)

    def draw(self, ints=False):
        self.ops = {k: (_ints((self.m, w), self.dev, self.gen) if ints else _randn((self.m, w), self.dev, self.gen))
                    for k, w in self.widths.items()}

    def launch(self, loss_rows=None, w_nce=0.0, w_iic=0.0, out=None, gather=None, no_dW1=False):
        import torch
        from idelucs_amd import _lib
        arr = lambda ts: (ctypes.c_void_p * 8)(*[t.t.data_ptr() for t in ts])
        gp = arr(self.grads)
        if no_dW1:
            gp[0] = None
        o = self.ops
        tail = (_p(self.hyper), _p(self.ctl), _p(o["x"]), _p(o["dr1"]), _p(o["a1"]), _p(o["da2"]), _p(o["a2"]), _p(o["dh"]), _p(o["d2"]),
                _p(o["dlogits"]), self.m, self.F, self.C, _p(loss_rows), w_nce, w_iic, _p(out),
                gather, _stream())
        if self.mom:
            _lib.check(_lib.lib.idl_small_wgrad_rms_momentum(arr(self.params), gp, arr(self.sq), arr(self.buf), *tail))
        else:
            _lib.check(_lib.lib.idl_small_wgrad_rms(arr(self.params), gp, arr(self.sq), *tail))
        torch.cuda.synchronize()
        for t in self.params + self.sq + self.buf + self.grads:
            assert t.intact()

    def state(self):
        return [[t.t.clone() for t in ts] for ts in (self.params, self.sq, self.buf)]


@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("m,F,C", WGRAD_CASES)
def test_wgrad_exact_on_small_integers(dev, m, F, C, mom):
    """dy, xin in -2..2: |sum| <= 4 m < 2^24, so the four weight gradients and the four bias sums are the integer results exactly."""
    w = _Wgrad(dev, m, F, C, mom, _gen(dev, "wgi", m, F, C))
    w.draw(ints=True)
    w.launch()
    want = R.wgrads(*(w.ops[k] for k in ("x", "dr1", "a1", "da2", "a2", "dh", "d2", "dlogits")))
    for i, (got, wt) in enumerate(zip(w.grads, want)):
        assert np.array_equal(wt, np.rint(wt))
        bad = np.argwhere(f64(got.t).astype(np.int64) != wt.astype(np.int64))
        assert len(bad) == 0 and np.array_equal(f64(got.t), wt), (i, len(bad), bad[:4])
    assert w.ctl.tolist() == [STEP + 1, 17]


@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("m,F,C", WGRAD_CASES)
def test_wgrad_random_gradients_rmsprop_and_step_loss(dev, m, F, C, mom):
    """Two consecutive launches (the second on a non-zero running average and momentum buffer): the gradients within the product bound
    (K = m; a bias sum is a product with a column of ones), the update against small_ref.rmsprop fed the kernel's own gradient within
    small_ref.rmsprop_bound, and the step loss: out[2] = mean(loss_rows), out[0] = w_nce out[2] + w_iic out[3], out[1] += out[0],
    ctl[0] += 1."""
    import torch
    g = _gen(dev, "wgr", m, F, C)
    w = _Wgrad(dev, m, F, C, mom, g)
    out = _Guarded((4,), dev, init=torch.tensor([9.0, 3.5, 9.0, 0.75], device=dev))
    w_nce, w_iic = 0.75, 0.25
    for it in range(2):
        w.draw()
        loss_rows = torch.rand((m,), device=dev, generator=g) * 6
        p0, v0, b0 = w.state()
        out0 = out.t.clone()
        w.launch(loss_rows=loss_rows, w_nce=w_nce, w_iic=w_iic, out=out.t)
        assert out.intact() and w.ctl.tolist() == [STEP + it + 1, 17]
        ones = np.ones((m, 1))
        for i, (dy, xin) in enumerate(JOBS):
            dy, xin = w.ops[dy], w.ops[xin]
            want_w, bar_w = f64(dy).T @ f64(xin), R.product_bound(dy.t(), xin)
            _hold(f"wgrad dW[{i}]", w.grads[2 * i].t, want_w, bar_w)
            _hold(f"torch.mm dW[{i}]", torch.mm(dy.t(), xin), want_w, bar_w)
            _hold(f"wgrad db[{i}]", w.grads[2 * i + 1].t, f64(dy).sum(0), R.product_bound(dy.t(), ones)[:, 0])
        for i in range(8):
            fed = w.grads[i].t
            want = R.rmsprop(p0[i], v0[i], fed, w.hyper, b0[i] if mom else None)
            bars = R.rmsprop_bound(p0[i], v0[i], fed, w.hyper, b0[i] if mom else None)
            form = "rms_momentum" if mom else "rms"
            _hold(f"{form} parameter step {it}", w.params[i].t, want[0], bars[0])
            _hold(f"{form} running average step {it}", w.sq[i].t, want[1], bars[1])
            if mom:
                _hold(f"{form} momentum buffer step {it}", w.buf[i].t, want[2], bars[2])
            else:
                assert float(w.buf[i].t.abs().max()) == 0.0
        # ---- the step loss.  The mean: ceil(m / 64) terms a lane, 6 levels, one quotient, each U / 2 of a partial sum of positive
        # terms: (ceil(m / 64) + 7) U mean.  out[0] from the kernel's out[2]: two products and a sum, 3 U (|a| + |b|); out[1]: one sum.
        mean = f64(loss_rows).mean()
        _hold("wgrad out[2]", out.t[2:3], [mean], [((m + 63) // 64 + 7) * U * mean])
        a, b = np.float32(w_nce) * f64(out.t[2]), np.float32(w_iic) * f64(out0[3])
        _hold("wgrad out[0]", out.t[0:1], [a + b], [3 * U * (abs(a) + abs(b))])
        _hold("wgrad out[1]", out.t[1:2], [f64(out0[1]) + f64(out.t[0])], [U * abs(f64(out0[1]) + f64(out.t[0]))])
        assert float(out.t[3]) == 0.75


@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("m,F,C", [(18, 63, 31), (66, 2080, 256), (440, 10, 200)])
def test_wgrad_without_dW1_updates_the_same(dev, m, F, C, mom):
    """grads[0] = NULL, the form the trainer runs without keep_grads: W1's gradient is not written, every parameter, running average
    and momentum buffer is what the launch that writes it leaves, bit for bit."""
    import torch
    runs = []
    for no_dW1 in (False, True):
        w = _Wgrad(dev, m, F, C, mom, _gen(dev, "wgn", m, F, C))
        w.draw()
        w.launch(no_dW1=no_dW1)
        runs.append(w)
    a, b = runs
    assert float(b.grads[0].t.abs().max()) == 0.0 and float(a.grads[0].t.abs().max()) > 0.0
    for x, y in zip(sum(a.state(), []) + [t.t for t in a.grads[1:]], sum(b.state(), []) + [t.t for t in b.grads[1:]]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("gb,F,at", [(1, 136, 17), (9, 10, 17), (220, 136, 17), (9, 2080, 355), (220, 63, 0)])
def test_wgrad_riding_assembly_is_gather_pairs_at(dev, gb, F, at, mom):
    """The next batch the launch assembles into y_next is idl_gather_pairs_at's at the offset ctl[1], bit for bit, on a store of 120
    rows and 3 views (360 pairs); at = 355 with 9 pairs: the rows whose pair lies beyond the list are not written (gather_pairs_at
    has no such limit: the list handed to it is padded)."""
    import torch
    from idelucs_amd import _lib
    g = _gen(dev, "gth", gb, F, at)
    n, views = 120, 3
    n_pairs = n * views
    feats = torch.rand(((views + 1) * n, F), device=dev, generator=g)
    mean = feats[:n].double().mean(0)
    scale = feats[:n].double().std(0).clamp_min(1e-3)
    inv_scale = 1.0 / scale
    perm = torch.cat([torch.randperm(n_pairs, device=dev, generator=g), torch.zeros(256, dtype=torch.int64, device=dev)])
    w = _Wgrad(dev, 2 * gb, F, 5, mom, g)
    w.draw()
    w.ctl[1] = at
    y = _Guarded((2 * gb, F), dev)
    y.t.fill_(SENTINEL)
    w.launch(gather=_lib.idl_next_batch_t(feats=_p(feats), n=n, f=F, view_stride=n * F, pair_idx=_p(perm), base=_p(w.ctl[1:]), base_add=0, n_pairs=n_pairs,
                                          batch=gb, mean=_p(mean), scale=_p(scale), inv_scale=_p(inv_scale), y=_p(y.t), part=0, part_end=1, parts=1))
    assert y.intact() and w.ctl.tolist() == [STEP + 1, at]
    want = torch.empty((2 * gb, F), device=dev)
    _lib.check(_lib.lib.idl_gather_pairs_at(_p(feats), n, F, n * F, _p(perm), _p(w.ctl[1:]), gb, _p(mean), _p(scale), _p(inv_scale),
                                            _p(want), _stream()))
    torch.cuda.synchronize()
    live = (torch.arange(2 * gb, device=dev) % gb) + at < n_pairs
    assert int(live.sum()) == 2 * min(gb, n_pairs - at)
    assert torch.equal(y.t[live], want[live])
    assert bool((y.t[~live] == SENTINEL).all())
    assert bool(torch.isfinite(want[live]).all()) and float(want[live].abs().max()) > 0
