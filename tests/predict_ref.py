"""NetLinear's eval forward in float64, its a-priori error bar, a float32 replay of the kernels' arithmetic and the inputs the GPU test of
predict='native' runs (test_gpu_predict_native.py; checked on the CPU by test_predict_reference.py).  numpy only; imports nothing of the package.

The forward (reference idelucs/PytorchUtils.py:38-50 in eval mode: both Dropouts are the identity):
    a1 = x W1^T + b1;  r1 = max(a1, 0);  lat = r1 W2^T + b2;  r2 = max(lat, 0);  logit = r2 W3^T + b3;  z = softmax(logit)
    prob = max_c z;  unit = the lowest c with z_c = prob

The bar.  u = 2^-24 (fp32's unit roundoff), gamma_n = n u / (1 - n u): a sum of n terms, each a product or a summand rounded once, computed in ANY
order -- sequentially, in K slices, in an MFMA's accumulator, fused or not -- differs from the exact sum by at most gamma_n times the sum of the
terms' magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1).  Nothing here is fitted to a GPU's output.
  e1      = gamma_(F+1) (|W1| |x| + |b1|)                  F products and the bias: F + 1 terms.  ReLU is 1-Lipschitz: r1 is off by at most e1.
  e_lat   = |W2| e1 + gamma_513 (|W2| r1 + |b2|)           the inherited error through the exact map, plus 512 products and the bias of this layer
  e_logit = |W3| e_lat + gamma_65 (|W3| r2 + |b3|)         the same for Linear(64, C) (ReLU again passes e_lat on unchanged)
  z       : z_c = exp(l_c) / sum_j exp(l_j).  With every logit of the row off by at most e = max_c e_logit, numerator and denominator each move by a
            factor inside exp(+-e): |dz_c| <= z_c (exp(2 e) - 1).  The exponential, the sum of at most 256 terms below 1 and the division add a few
            roundings on a value that is at most 1: + 4 u.
(The products of the errors -- gamma times e1 -- are second order, 1e-7 of the bar, and left out as the bar above states.)
With exact operands (small integers whose partial sums all stay below 2^24: exact_ok) e1 = e_lat = 0 and lat has to be the float64 value bit for bit.
"""
import functools
import zlib

import numpy as np

H1, H2 = 512, 64
U = 2.0 ** -24
MARGIN_CAP = 0.02             # the share of rows the argmax test may skip (top-two margin below twice z's bar)

# ---- the cases of the GPU test
EXACT_C = (1, 5, 64, 65, 200, 256)
EXACT_MF = [(m, F) for F in (192, 256, 1024) for m in (32, 96)]                  # F = 192: layer 1's three-stage ring exactly full
EXACT_CASES = [(m, F, EXACT_C[(i + j) % 6]) for j in (0, 3) for i, (m, F) in enumerate(EXACT_MF)] + [(32, 65536, 5)]      # (m, F, C)
RANDOM_CASES = [(96, F, C, 1.0) for F in (256, 4096) for C in (5, 200)] + [(96, 256, 5, 10.0)]      # (m, F, C, scale of W3: 10 = large logits)
LARGE_LOGIT_CASE = RANDOM_CASES[-1]
ROWS_ALONE = (40, 256, 5)     # (rows, F, C) of the rows-alone test
TILE = 16                     # rows of a workgroup of idl_predict_mid


def gamma(n):
    return n * U / (1.0 - n * U)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------- inputs

@functools.lru_cache(maxsize=None)
def exact_operands(m, F, C):
    """Small integers all the way to the latent: x dense in [-7, 7]; W1 with 16 entries of +-1..3 per hidden unit at random k (|a1 + b1| <= 343: an
    element of a1 IS a signed sum of 16 named entries of x, and over the 512 units every 64-wide K chunk is read); b1, W2, b2 dense in [-7, 7]
    (|lat| < 1.3e6 < 2^24).  W3, b3: integers times 2^-16, logits of order 1 (not exact: z is held to the bar)."""
    rng = _rng("exact", m, F, C)
    ints = lambda shape: rng.integers(-7, 8, shape).astype(np.float32)
    W1 = np.zeros((H1, F), np.float32)
    cols = np.stack([rng.choice(F, 16, replace=False) for _ in range(H1)])
    vals = (rng.integers(1, 4, (H1, 16)) * rng.choice(np.array([-1, 1]), (H1, 16))).astype(np.float32)
    W1[np.arange(H1)[:, None], cols] = vals
    o = {"x": ints((m, F)), "W1": W1, "b1": ints(H1), "W2": ints((H2, H1)), "b2": ints(H2),
         "W3": (ints((C, H2)) * 2.0 ** -16).astype(np.float32), "b3": ints(C) * np.float32(0.125)}
    for a in o.values():
        a.setflags(write=False)
    return o


PLANT = 30.0                  # strength of the planted direction of random_operands


def class_of_unit(j, C):
    """The class that reads latent unit j in random_operands' W3 (one class a unit, spread over the whole range of C)."""
    c = j + 64 * (j % 3)
    return c if c < C else j


@functools.lru_cache(maxsize=None)
def random_operands(m, F, C, w3_scale=1.0):
    """Kaiming-normal W1, W2 (std sqrt(2 / fan_in), reference models.py:36-44), small normal biases (so that a lost bias shows), standard-normal rows.
    The bar is a worst-case one: through two dense layers it reaches 0.3 on a latent of size 1 at F = 4096, and with a dense Kaiming W3 on top the
    reference itself cannot name the largest z of most rows (the cap of the argmax test).  So every row carries, besides its standard-normal entries, a
    planted direction PLANT W1^T max(W2[j], 0) that lifts ONE latent unit j = row mod min(C, 64) to about 2 PLANT, and W3 is 0.02 of a Kaiming matrix
    plus 0.2 at [class_of_unit(j), j]: the row's class is class_of_unit(j), by a margin far outside the bar.  w3_scale multiplies W3 (10: logits
    beyond 100, where exp overflows fp32 unless the row's largest logit is subtracted)."""
    rng = _rng("random", m, F, C, w3_scale)
    n = lambda shape, std: (rng.standard_normal(shape) * std).astype(np.float32)
    W1, W2 = n((H1, F), np.sqrt(2.0 / F)), n((H2, H1), np.sqrt(2.0 / H1))
    units = np.arange(m) % min(C, H2)
    x = n((m, F), 1.0) + np.float32(PLANT) * (np.maximum(W2[units], 0) @ W1)
    W3 = 0.02 * n((C, H2), np.sqrt(2.0 / H2))
    for j in range(min(C, H2)):
        W3[class_of_unit(j, C), j] += 0.2
    o = {"x": x.astype(np.float32), "W1": W1, "b1": n(H1, 0.5), "W2": W2, "b2": n(H2, 0.5), "W3": (W3 * w3_scale).astype(np.float32), "b3": n(C, 0.5)}
    for a in o.values():
        a.setflags(write=False)
    return o


# ---------------------------------------------------------------- float64

def forward64(x, W1, b1, W2, b2, W3, b3):
    """-> dict(a1, r1, lat, r2, logit, z, prob, unit), float64 (unit int64: np.argmax takes the lowest index among equals)."""
    f = lambda a: np.asarray(a, np.float64)
    a1 = f(x) @ f(W1).T + f(b1)
    r1 = np.maximum(a1, 0.0)
    lat = r1 @ f(W2).T + f(b2)
    r2 = np.maximum(lat, 0.0)
    logit = r2 @ f(W3).T + f(b3)
    e = np.exp(logit - logit.max(1, keepdims=True))
    z = e / e.sum(1, keepdims=True)
    return {"a1": a1, "r1": r1, "lat": lat, "r2": r2, "logit": logit, "z": z, "prob": z.max(1), "unit": np.argmax(z, 1).astype(np.int64)}


def bars(x, W1, b1, W2, b2, W3, b3, ref=None):
    """The a-priori bars of the module docstring -> dict(lat [m, 64], logit [m, C], z [m, C])."""
    f = lambda a: np.abs(np.asarray(a, np.float64))
    r = forward64(x, W1, b1, W2, b2, W3, b3) if ref is None else ref
    F = np.shape(x)[1]
    e1 = gamma(F + 1) * (f(x) @ f(W1).T + f(b1))
    e_lat = e1 @ f(W2).T + gamma(H1 + 1) * (r["r1"] @ f(W2).T + f(b2))
    e_logit = e_lat @ f(W3).T + gamma(H2 + 1) * (r["r2"] @ f(W3).T + f(b3))
    e_z = r["z"] * np.expm1(2.0 * e_logit.max(1, keepdims=True)) + 4.0 * U
    return {"lat": e_lat, "logit": e_logit, "z": e_z}


@functools.lru_cache(maxsize=None)
def reference(kind, case):
    """(float64 forward, bars) of exact_operands(*case) / random_operands(*case); computed once, shared, read-only."""
    o = (exact_operands if kind == "exact" else random_operands)(*case)
    r = forward64(**o)
    b = bars(**o, ref=r)
    for a in list(r.values()) + list(b.values()):
        a.setflags(write=False)
    return r, b


def margin_rows(z, z_bar):
    """bool [m]: rows whose top-two margin in z is below twice the row's largest bar -- where a result inside the bar may name another unit."""
    if z.shape[1] < 2:
        return np.zeros(z.shape[0], bool)
    top = np.sort(z, 1)[:, -2:]
    return (top[:, 1] - top[:, 0]) < 2.0 * z_bar.max(1)


def exact_ok(x, W1, b1, W2, b2, **_):
    """Every partial sum on the way to lat is an integer below 2^24 in any order: integer operands, sum of the terms' magnitudes < 2^24 at both layers."""
    f = lambda a: np.abs(np.asarray(a, np.float32))
    if not all(np.array_equal(a, np.rint(a)) for a in (x, W1, b1, W2, b2)):
        return False
    s1 = f(x) @ f(W1).T + f(b1)                 # (integers below 2^24: exact in float32 whatever BLAS does)
    if not s1.max() < 2.0 ** 24:
        return False
    s2 = s1.astype(np.float64) @ np.abs(np.asarray(W2, np.float64)).T + np.abs(np.asarray(b2, np.float64))
    return bool(s2.max() < 2.0 ** 24)


# ---------------------------------------------------------------- the kernels' arithmetic in float32

def replay32(x, W1, b1, W2, b2, W3, b3, drop_l1_chunk=None, drop_b1=False, drop_l2_slice=None, subtract_max=True):
    """idl_l1_fwd + idl_predict_mid in float32 numpy: layer 1 in K chunks of 64 added in ascending order; the bias and ReLU; lat = b2 + the 16 K
    slices of 32 in ascending order; ReLU; logits; softmax with the row's largest logit subtracted.  The keywords BREAK it (a chunk or slice left
    out, the bias left out, no subtraction): what the bar has to catch.  -> dict(lat, z, prob, unit)"""
    f = lambda a: np.asarray(a, np.float32)
    x, W1, b1, W2, b2, W3, b3 = (f(a) for a in (x, W1, b1, W2, b2, W3, b3))
    m, F = x.shape
    a1 = np.zeros((m, H1), np.float32)
    for c in range(F // 64):
        if c != drop_l1_chunk:
            a1 = a1 + x[:, 64 * c:64 * c + 64] @ W1[:, 64 * c:64 * c + 64].T
    r1 = np.maximum(a1 if drop_b1 else a1 + b1, np.float32(0))
    lat = np.broadcast_to(b2, (m, H2)).astype(np.float32)
    for w in range(16):
        if w != drop_l2_slice:
            lat = lat + r1[:, 32 * w:32 * w + 32] @ W2[:, 32 * w:32 * w + 32].T
    logit = np.maximum(lat, np.float32(0)) @ W3.T + b3
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(logit - logit.max(1, keepdims=True)) if subtract_max else np.exp(logit)
        z = e / e.sum(1, keepdims=True, dtype=np.float32)
    assert lat.dtype == z.dtype == np.float32
    return {"lat": lat, "z": z, "prob": z.max(1), "unit": np.argmax(z, 1).astype(np.int64)}


def over_bar(got, want, bar):
    """Largest |got - want| / bar; a value that is not a number counts as infinitely far.  (bar > 0 everywhere: the 4 u, or a bias.)"""
    d = np.abs(np.asarray(got, np.float64) - want)
    d[~np.isfinite(d)] = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0.0, 0.0, d / bar)
    return float(q.max())


# ---------------------------------------------------------------- reporting

def first_mismatch(got, want):
    """got (fp32) against want (float64, exactly representable in fp32) by bit pattern, [rows][cols] -> None, or a message naming the row, the
    column and the tile (16 rows a workgroup)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    w32 = want.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want), "the reference is not an fp32 number"
    bad = np.ascontiguousarray(got).view(np.int32) != np.ascontiguousarray(w32).view(np.int32)
    if not bad.any():
        return None
    r, c = (int(i) for i in np.argwhere(bad)[0])
    return f"{int(bad.sum())} elements differ; first at row {r}, column {c} (tile {r // TILE}, row {r % TILE} of the tile): got {float(got[r, c])!r}, want {float(w32[r, c])!r}"
