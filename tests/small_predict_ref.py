"""myNet's eval forward in float64, its a-priori error bars, a float32 replay of the kernels' arithmetic and the inputs the GPU test of
small_predict='native' runs (test_gpu_small_predict_native.py; checked on the CPU by test_small_predict_reference.py).  numpy only; imports
predict_ref for what it shares (gamma, the margin rule and its cap, over_bar, first_mismatch) and nothing of the package.

The forward (reference idelucs/PytorchUtils.py:13-22 in eval mode: both Dropouts are the identity):
    a1 = x W1^T + b1;  r1 = max(a1, 0);  p2 = r1 W2^T + b2;  a2 = p2 if p2 > 0 else 0.01 p2;  lat = a2 Wi^T + bi  (raw)
    logit = a2 Wc^T + bc;  z = softmax(logit);  prob = max_c z;  unit = the lowest c with z_c = prob

The bars.  u = 2^-24, gamma_n = n u / (1 - n u): a sum of n terms, each a product or a summand rounded once, computed in ANY order differs from the
exact sum by at most gamma_n times the sum of the terms' magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1).
  e1      = gamma_(F+1) (|W1| |x| + |b1|)                  F products and the bias.  ReLU is 1-Lipschitz: r1 is off by at most e1.
  e_p2    = |W2| e1 + gamma_401 (|W2| r1 + |b2|)           the inherited error through the exact map, plus 400 products and the bias
  e_a2    = e_p2 + gamma_2 |a2|                            LeakyReLU is 1-Lipschitz; on the negative side the slope is fl32(0.01), off 0.01 by less than
                                                           u relatively, and the product is rounded once: two roundings of a value |a2|
  e_lat   = |Wi| e_a2 + gamma_129 (|Wi| |a2| + |bi|)       Linear(128, 64)
  e_logit = |Wc| e_a2 + gamma_129 (|Wc| |a2| + |bc|)       Linear(128, C)
  z       : every logit of the row off by at most e = max_c e_logit: |dz_c| <= z_c (exp(2 e) - 1), + 4 u for the exponential, the sum of at most
            256 terms below 1 and the division on a value that is at most 1 (as predict_ref.bars).
Nothing here is fitted to a GPU's output.  With exact operands (small integers, every partial sum below 2^24) and p2 >= 0 everything up to lat is
exact and lat has to be the float64 value bit for bit.
"""
import functools
import zlib

import numpy as np

from predict_ref import MARGIN_CAP, U, first_mismatch, gamma, margin_rows, over_bar  # noqa: F401  (re-exported to the tests)

H1, H2, LAT = 400, 128, 64
SLOPE = 0.01
NAMES = ("W1", "b1", "W2", "b2", "Wi", "bi", "Wc", "bc")
STAGE = 32                    # k of one LDS stage of idl_small_predict_l1
TILE = 16                     # rows of a workgroup of idl_small_predict_mid


def n_features(k):
    """Rows of model_size='small' (reference models.py:59-66)."""
    return (4 ** k + 4 ** (k // 2)) // 2 if k % 2 == 0 else (4 ** k) // 2


WIDEST_F = n_features(9)      # the widest row the small model builds at today (k = 9)

# ---- the cases of the GPU test: F' = 136 (k = 4) and 2080 (k = 6) end in a partly filled stage / 16-wide half; m = 1, 15, 17 are ragged tiles
EXACT_C = (1, 5, 16, 17, 64, 65, 200, 256)
EXACT_CASES = [(m, F, EXACT_C[(6 * i + j) % 8]) for i, F in enumerate((32, 136, 512, 2080)) for j, m in enumerate((1, 15, 16, 17, 33, 96))] \
    + [(16, WIDEST_F, 5)]                                                           # (m, F, C)
NEGATIVE_CASES = [(33, 136, 5), (17, 2080, 65)]                                     # exact operands with negative pre-activations of layer 2
RANDOM_CASES = [(96, F, C, 1.0) for F in (136, 2080) for C in (5, 200)] + [(96, 136, 5, 10.0)]      # (m, F, C, scale of Wc: 10 = large logits)
LARGE_LOGIT_CASE = RANDOM_CASES[-1]
ROWS_ALONE = [(40, 136, 5), (40, 2080, 200)]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _frozen(o):
    for a in o.values():
        a.setflags(write=False)
    return o


# ---------------------------------------------------------------- inputs

@functools.lru_cache(maxsize=None)
def exact_operands(m, F, C, negative=False):
    """Small integers all the way to the latent.  x dense in [-7, 7]; W1 with min(F, 16) entries of +-1..3 per hidden unit at random k (over the
    400 units every stage of F is read); b1 in [-7, 7].
    negative = False: W2 in {0, 1} and b2 in [0, 7], so p2 >= 0 and a2 = p2; Wi dense in [-3, 3], bi in [-7, 7]: lat is an integer below 2^24.
    negative = True: W2 in [-3, 3] and b2 in [-7, 7] (p2 of both signs, integers); Wi one-hot -- latent unit j reads a2[:, 2 j + 1] with weight 1 --
    so lat = fl32(fl32(a2) + bi) with a2 = p2 or fl32(fl32(0.01) p2): negative_latent32.
    Wc, bc: integers times 2^-16 / 2^-3, logits of order 1 (not exact: z is held to the bar)."""
    rng = _rng("small exact", m, F, C, negative)
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    nz = min(F, 16)
    W1 = np.zeros((H1, F), np.float32)
    cols = np.stack([rng.choice(F, nz, replace=False) for _ in range(H1)])
    vals = (rng.integers(1, 4, (H1, nz)) * rng.choice(np.array([-1, 1]), (H1, nz))).astype(np.float32)
    W1[np.arange(H1)[:, None], cols] = vals
    if negative:
        W2, b2 = ints(-3, 3, (H2, H1)), ints(-7, 7, H2)
        Wi = np.zeros((LAT, H2), np.float32)
        Wi[np.arange(LAT), 2 * np.arange(LAT) + 1] = 1.0
    else:
        W2, b2, Wi = ints(0, 1, (H2, H1)), ints(0, 7, H2), ints(-3, 3, (LAT, H2))
    return _frozen({"x": ints(-7, 7, (m, F)), "W1": W1, "b1": ints(-7, 7, H1), "W2": W2, "b2": b2, "Wi": Wi, "bi": ints(-7, 7, LAT),
                    "Wc": (ints(-7, 7, (C, H2)) * 2.0 ** -16).astype(np.float32), "bc": ints(-7, 7, C) * np.float32(0.125)})


def negative_latent32(o):
    """The latent of exact_operands(negative=True) as float32 arithmetic gives it in any order: p2 is an exact integer, the slope product and the
    bias add are one rounding each."""
    p2 = forward64(**o)["p2"].astype(np.float32)
    a2 = np.where(p2 > 0, p2, np.float32(SLOPE) * p2).astype(np.float32)
    return (a2[:, 1::2] + o["bi"]).astype(np.float32)


PLANT = 30.0                  # strength of the planted direction of random_operands


def class_of_unit(j, C):
    """The class that reads unit j of a2 in random_operands' Wc (one class a unit, spread over the whole range of C)."""
    c = j + 128 * (j % 2)
    return c if c < C else j


@functools.lru_cache(maxsize=None)
def random_operands(m, F, C, wc_scale=1.0):
    """Kaiming-normal W1, W2, Wi (std sqrt(2 / fan_in), reference models.py:36-44), small normal biases (so that a lost bias shows), standard-normal
    rows.  As predict_ref.random_operands: the bars are worst-case ones, and with a dense Kaiming classifier on top the reference itself could not
    name the largest z of many rows.  So every row carries a planted direction PLANT W1^T max(W2[j], 0) that lifts ONE unit j = row mod min(C, 128)
    of a2, and Wc is 0.02 of a Kaiming matrix plus 0.2 at [class_of_unit(j), j].  wc_scale multiplies Wc (10: logits beyond 100)."""
    rng = _rng("small random", m, F, C, wc_scale)
    n = lambda shape, std: (rng.standard_normal(shape) * std).astype(np.float32)
    W1, W2, Wi = n((H1, F), np.sqrt(2.0 / F)), n((H2, H1), np.sqrt(2.0 / H1)), n((LAT, H2), np.sqrt(2.0 / H2))
    units = np.arange(m) % min(C, H2)
    x = n((m, F), 1.0) + np.float32(PLANT) * (np.maximum(W2[units], 0) @ W1)
    Wc = 0.02 * n((C, H2), np.sqrt(2.0 / H2))
    for j in range(min(C, H2)):
        Wc[class_of_unit(j, C), j] += 0.2
    return _frozen({"x": x.astype(np.float32), "W1": W1, "b1": n(H1, 0.5), "W2": W2, "b2": n(H2, 0.5), "Wi": Wi, "bi": n(LAT, 0.5),
                    "Wc": (Wc * wc_scale).astype(np.float32), "bc": n(C, 0.5)})


# ---------------------------------------------------------------- float64

def forward64(x, W1, b1, W2, b2, Wi, bi, Wc, bc):
    """-> dict(a1, r1, p2, a2, lat, logit, z, prob, unit), float64 (unit int64: np.argmax takes the lowest index among equals)."""
    f = lambda a: np.asarray(a, np.float64)
    a1 = f(x) @ f(W1).T + f(b1)
    r1 = np.maximum(a1, 0.0)
    p2 = r1 @ f(W2).T + f(b2)
    a2 = np.where(p2 > 0, p2, SLOPE * p2)
    lat = a2 @ f(Wi).T + f(bi)
    logit = a2 @ f(Wc).T + f(bc)
    e = np.exp(logit - logit.max(1, keepdims=True))
    z = e / e.sum(1, keepdims=True)
    return {"a1": a1, "r1": r1, "p2": p2, "a2": a2, "lat": lat, "logit": logit, "z": z, "prob": z.max(1), "unit": np.argmax(z, 1).astype(np.int64)}


def bars(x, W1, b1, W2, b2, Wi, bi, Wc, bc, ref=None):
    """The a-priori bars of the module docstring -> dict(lat [m, 64], logit [m, C], z [m, C])."""
    f = lambda a: np.abs(np.asarray(a, np.float64))
    r = forward64(x, W1, b1, W2, b2, Wi, bi, Wc, bc) if ref is None else ref
    F = np.shape(x)[1]
    e1 = gamma(F + 1) * (f(x) @ f(W1).T + f(b1))
    e_p2 = e1 @ f(W2).T + gamma(H1 + 1) * (r["r1"] @ f(W2).T + f(b2))
    e_a2 = e_p2 + gamma(2) * f(r["a2"])
    e_lat = e_a2 @ f(Wi).T + gamma(H2 + 1) * (f(r["a2"]) @ f(Wi).T + f(bi))
    e_logit = e_a2 @ f(Wc).T + gamma(H2 + 1) * (f(r["a2"]) @ f(Wc).T + f(bc))
    e_z = r["z"] * np.expm1(2.0 * e_logit.max(1, keepdims=True)) + 4.0 * U
    return {"lat": e_lat, "logit": e_logit, "z": e_z}


@functools.lru_cache(maxsize=None)
def reference(kind, case):
    """(float64 forward, bars) of exact_operands(*case) / exact_operands(*case, negative=True) / random_operands(*case); computed once, shared,
    read-only."""
    o = {"exact": exact_operands, "negative": lambda *c: exact_operands(*c, negative=True), "random": random_operands}[kind](*case)
    r = forward64(**o)
    b = bars(**o, ref=r)
    for a in list(r.values()) + list(b.values()):
        a.setflags(write=False)
    return r, b


def exact_ok(x, W1, b1, W2, b2, Wi, bi, **_):
    """Every partial sum on the way to lat is an integer below 2^24 in any order: integer operands, sum of the terms' magnitudes < 2^24 at layers 1
    and 2, and -- where p2 >= 0 throughout, so that a2 is that integer -- at the instance head."""
    f = lambda a: np.abs(np.asarray(a, np.float64))
    if not all(np.array_equal(a, np.rint(a)) for a in (x, W1, b1, W2, b2, Wi, bi)):
        return False
    s1 = f(x) @ f(W1).T + f(b1)
    s2 = s1 @ f(W2).T + f(b2)
    if not (s1.max() < 2.0 ** 24 and s2.max() < 2.0 ** 24):
        return False
    p2 = forward64(x, W1, b1, W2, b2, Wi, bi, np.zeros((1, H2)), np.zeros(1))["p2"]
    if (p2 < 0).any():
        return True                       # (the latent is then negative_latent32's, not an integer)
    return bool((s2 @ f(Wi).T + f(bi)).max() < 2.0 ** 24)


# ---------------------------------------------------------------- the kernels' arithmetic in float32

def replay32(x, W1, b1, W2, b2, Wi, bi, Wc, bc, drop_l1_stage=None, drop_b1=False, drop_b2=False, drop_bi=False, drop_l2_chunk=None, relu2=False,
             slope=SLOPE, dropout1=1.0, dropout2=1.0, top_highest=False):
    """idl_small_predict_l1 + idl_small_predict_mid in float32 numpy: layer 1 in K stages of 32 added in ascending order (a stage that crosses F'
    is shorter: its missing entries are zeros); the bias and ReLU; p2 = the 25 K chunks of 16 in ascending order, then b2; LeakyReLU; the two heads;
    softmax with the row's largest logit subtracted; the lowest class among equal z.  The keywords BREAK it: a stage or chunk left out, a bias left
    out, ReLU or another slope in LeakyReLU's place, a Dropout's training factor left in (dropout1: on r1; dropout2: on the classifier's input), the
    highest class on a tie.  -> dict(lat, z, prob, unit)"""
    f = lambda a: np.asarray(a, np.float32)
    x, W1, b1, W2, b2, Wi, bi, Wc, bc = (f(a) for a in (x, W1, b1, W2, b2, Wi, bi, Wc, bc))
    m, F = x.shape
    a1 = np.zeros((m, H1), np.float32)
    for c in range((F + STAGE - 1) // STAGE):
        if c != drop_l1_stage:
            a1 = a1 + x[:, STAGE * c:STAGE * c + STAGE] @ W1[:, STAGE * c:STAGE * c + STAGE].T
    r1 = np.maximum(a1 if drop_b1 else a1 + b1, np.float32(0)) * np.float32(dropout1)
    p2 = np.zeros((m, H2), np.float32)
    for c in range(H1 // 16):
        if c != drop_l2_chunk:
            p2 = p2 + r1[:, 16 * c:16 * c + 16] @ W2[:, 16 * c:16 * c + 16].T
    if not drop_b2:
        p2 = p2 + b2
    a2 = np.where(p2 > 0, p2, (np.float32(0) if relu2 else np.float32(slope)) * p2).astype(np.float32)
    lat = a2 @ Wi.T if drop_bi else a2 @ Wi.T + bi
    logit = (a2 * np.float32(dropout2)) @ Wc.T + bc
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(logit - logit.max(1, keepdims=True))
        z = e / e.sum(1, keepdims=True, dtype=np.float32)
    assert lat.dtype == z.dtype == np.float32
    C = z.shape[1]
    unit = (C - 1 - np.argmax(z[:, ::-1], 1)) if top_highest else np.argmax(z, 1)
    return {"lat": lat, "z": z, "prob": z.max(1), "unit": unit.astype(np.int64)}
