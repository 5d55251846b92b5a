"""An exact reference for the scaler kernels (csrc/scaler.hip, csrc/scaler_device.h) and the error bounds their statistics must meet.
numpy and the standard library only.

The reference.  exact_stats gives a column's mean and population variance in np.longdouble (64-bit significand): the mean is math.fsum
of the float64 values (the correctly rounded sum) divided by n, plus the residual sum(x - mean) / n taken in longdouble; the variance is
the corrected two-pass form sum(d d) / n - (sum(d) / n)^2 with d = x - mean in longdouble.  Its own error is a few 2^-64 relative to the
quantities the bounds below are stated in: four decimal orders below the bounds.  Where longdouble is no wider than float64 the same
quantities are formed with fractions.Fraction.

The bounds.  The kernels sum t = x - x0 and t^2 per column, x0 = row 0 of the matrix (so t is exact up to one rounding, and exact where
the column's values are near each other), in float64: inside a row block sequentially, at most rpb = rows_per_block(n) terms; the
finishing kernel adds the blocks = stat_row_blocks(n) partial sums in 16 groups of at most ceil(blocks / 16) terms and then the 16 groups.
With EPS = 2^-53 every sum therefore carries at most

    gamma = (rpb + ceil(blocks / 16) + 16 + 4) * EPS

relative to the sum of the magnitudes of its terms (the 4: the rounding of t, of t t, and two to spare).  Writing t1 = sum t, t2 = sum t^2:
  * a2 sums non-negative terms: |a2 - t2| <= gamma t2;
  * |a1 - t1| <= gamma sum|t|, and (sum|t|)^2 / n <= t2 (Cauchy-Schwarz), so the error of a1^2 / n is at most 2 gamma t2 to first order;
  * var = (a2 - a1^2 / n) / n is therefore off by at most 3 gamma t2 / n, and t2 / n = var + (x0 - mean)^2 = var * kappa with

        kappa = 1 + (x0 - mean)^2 / var        (<= n + 1: one row cannot be further from the mean than sqrt(n var))

    -- the shift is row 0, not the mean, so the variance formula does cancel when row 0 is an outlier, by the factor kappa;
  * scale = sqrt(var):    |scale - exact| / exact <= 1.5 gamma kappa + 4 EPS      (4 EPS: the two divisions, the subtraction, the root)
  * mean = x0 + a1 / n:   |mean - exact| <= gamma mean_r|x_r - x0| + 4 EPS |exact| (4 EPS: the division and the final addition)
A fused multiply-add in a2 += t t (the device contracts it) removes a rounding: it only tightens these.  The bounds are derived, not
measured; tests/test_scaler_reference.py checks that the algorithm itself (stats_ref.stats_whole, the non-FMA replay) meets them.
"""
import fractions
import math

import numpy as np

from stats_ref import rows_per_block, stat_row_blocks

EPS = 2.0 ** -53                        # unit roundoff of float64
SK_EPS = 2.220446049250313e-16          # np.finfo(float64).eps: sklearn's _handle_zeros_in_scale compares with 10 of these
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)


def _exact_stats_fraction(x):
    n, f = x.shape
    mean, var = np.empty(f, np.longdouble), np.empty(f, np.longdouble)
    for j in range(f):
        col = [fractions.Fraction(float(v)) for v in x[:, j]]
        m = sum(col) / n
        v = sum((c - m) ** 2 for c in col) / n
        # (a Fraction -> float conversion is correctly rounded; a second term carries the next 53 bits)
        mean[j] = np.longdouble(float(m)) + np.longdouble(float(m - fractions.Fraction(float(m))))
        var[j] = np.longdouble(float(v)) + np.longdouble(float(v - fractions.Fraction(float(v))))
    return mean, var


def exact_stats(x):
    """[n, f] float32 or float64 -> (mean [f], population variance [f]) as np.longdouble"""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    x64 = x.astype(np.float64)                                            # exact for float32
    n, f = x64.shape
    if not LONGDOUBLE_OK:
        return _exact_stats_fraction(x64)
    m0 = np.array([math.fsum(x64[:, j]) for j in range(f)], np.float64).astype(np.longdouble) / n
    d = x64.astype(np.longdouble) - m0
    r = d.sum(axis=0) / n
    var = (d * d).sum(axis=0) / n - r * r
    return m0 + r, np.maximum(var, np.longdouble(0))


def scale_of(var):
    """sqrt with sklearn's rule (_handle_zeros_in_scale): a scale below 10 float64 epsilons becomes 1"""
    s = np.sqrt(np.asarray(var, np.longdouble))
    s[s < 10 * SK_EPS] = 1
    return s


def freq_rows(counts):
    """the float64 frequency rows of int32 counts: IEEE division (correctly rounded) by the row's int64 total"""
    counts = np.asarray(counts)
    return counts.astype(np.float64) / counts.sum(1, dtype=np.int64)[:, None].astype(np.float64)


def transform_f32(x32, mean, scale):
    """StandardScaler.transform in place on a float32 array with float64 statistics (oracle.scaler_transform): each of the two operations
    in float64, rounded to float32"""
    x32 = np.asarray(x32)
    assert x32.dtype == np.float32
    mean, scale = np.asarray(mean, np.float64), np.asarray(scale, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        t = (x32.astype(np.float64) - mean).astype(np.float32)
        return (t.astype(np.float64) / scale).astype(np.float32)


def transform_f64(x64, mean, scale):
    """the same on a float64 array, rounded once to float32 afterwards"""
    x64 = np.asarray(x64)
    assert x64.dtype == np.float64
    mean, scale = np.asarray(mean, np.float64), np.asarray(scale, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return ((x64 - mean) / scale).astype(np.float32)


def gamma(n):
    blocks, rpb = stat_row_blocks(n), rows_per_block(n)
    return (rpb + -(-blocks // 16) + 16 + 4) * EPS


def bounds(x, n=None, stats=None):
    """-> (kappa [f], relative bound on the scale [f], absolute bound on the mean [f]) for the one-pass statistics of x [n, f]
    (longdouble; derivation in the module docstring).  stats: exact_stats(x) where the caller has it."""
    x = np.asarray(x)
    n = x.shape[0] if n is None else n
    assert n == x.shape[0]
    mean, var = exact_stats(x) if stats is None else stats
    xl = x.astype(np.float64).astype(np.longdouble)
    off = xl[0] - mean
    kappa = np.ones_like(var)
    nz = var > 0
    kappa[nz] = 1 + off[nz] * off[nz] / var[nz]
    g = np.longdouble(gamma(n))
    tol_scale = 1.5 * g * kappa + 4 * EPS
    tol_mean = g * np.abs(xl - xl[0]).mean(axis=0) + 4 * EPS * np.abs(mean)
    return kappa, tol_scale, tol_mean


def error_ratios(x, mean, scale):
    """error / bound of a route's float64 (mean, scale) on x: -> (ratio of the mean [f], ratio of the scale [f]).  A column whose bound and
    error are both 0 gives 0; a column whose error is not 0 where the bound is gives inf."""
    m_ref, v_ref = exact_stats(x)
    s_ref = scale_of(v_ref)
    _, tol_s, tol_m = bounds(x, stats=(m_ref, v_ref))
    e_m = np.abs(np.asarray(mean, np.float64).astype(np.longdouble) - m_ref)
    e_s = np.abs(np.asarray(scale, np.float64).astype(np.longdouble) - s_ref) / s_ref
    with np.errstate(divide="ignore", invalid="ignore"):
        r_m = np.where(e_m == 0, 0, e_m / tol_m)
        r_s = np.where(e_s == 0, 0, e_s / tol_s)
    return r_m.astype(np.float64), r_s.astype(np.float64)


def families(n, dtype, rng):
    """the column families of the statistics tests that fit dtype: name -> column [n] (u = uniform [0, 1))"""
    dtype = np.dtype(dtype)
    f32 = dtype == np.float32

    def u():
        return rng.random(n)

    def with_row(col, r, v):
        col = np.array(col, np.float64)
        col[r] = v
        return col
    fam = {
        "benign": u() * 1e-3,
        "const": np.full(n, 0.25),
        "zero": np.zeros(n),
        "third_row0": with_row(np.full(n, 1.0 / 3.0), 0, 0.5),
        "third_last": with_row(np.full(n, 1.0 / 3.0), n - 1, 0.5),
        "spike": with_row(np.zeros(n), n // 2, 1.0),
        "near_one": 1.0 + (1e-4 if f32 else 1e-7) * u(),
        "freq_like": with_row(2.4e-4 + 1e-4 * (u() - 0.5), 0, 0.5),
        "alternating": np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + u()),
        "huge": u() * (1e18 if f32 else 1e30),
        "tiny": u() * (1e-18 if f32 else 1e-30),
    }
    if f32:
        fam["subnormal"] = u() * 1e-40                       # (float32's smallest normal is 1.18e-38)
    return {k: v.astype(dtype) for k, v in fam.items()}


def family_matrix(n, f, dtype, seed):
    """[n, f] of dtype whose column j is of family j % (number of families), every column with draws of its own
    -> (matrix, the f family names)"""
    rng = np.random.default_rng(seed)
    cols, names = [], []
    while len(cols) < f:
        for k, v in families(n, dtype, rng).items():
            cols.append(v)
            names.append(k)
    return np.ascontiguousarray(np.stack(cols[:f], axis=1)), names[:f]
