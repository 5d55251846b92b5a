"""CPU tests of tests/scaler_ref.py: the exact reference against rational arithmetic and sklearn, and the derived bounds against the
algorithm's own numpy replay (stats_ref.stats_whole, without the device's FMA) -- the check that the bounds the GPU tests assert are
bounds the algorithm meets."""
import fractions

import numpy as np
import pytest

import scaler_ref as S
import stats_ref as R

NS = [1, 2, 5, 257, 4097, 65537]


def _awkward():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((7, 5)) * np.array([1.0, 1e-30, 1e30, 1e-3, 1.0])
    x[:, 0] = 1.0 + rng.integers(0, 64, 7) * 2.0 ** -52            # values one rounding apart
    x[:, 3] = [1.0 / 3.0, 0.1, 0.2, 0.3, 1e-17, -0.1, 2.0 / 3.0]
    x[:, 4] = 1e16 + rng.integers(0, 9, 7) * 2.0                    # a mean far above the spread
    return x


def test_exact_stats_equal_rational_arithmetic():
    x = _awkward()
    n = x.shape[0]
    for stats in (S.exact_stats, S._exact_stats_fraction):
        mean, var = stats(x)
        assert mean.dtype == var.dtype == np.longdouble
        for j in range(x.shape[1]):
            col = [fractions.Fraction(float(v)) for v in x[:, j]]
            m = sum(col) / n
            v = sum((c - m) ** 2 for c in col) / n
            spread = sum(abs(c - m) for c in col) / n
            # the mean to 2^-60 of the spread (or of itself), the variance to 2^-58 relative: longdouble sums of 7 terms
            em = abs(fractions.Fraction(float(mean[j])) + fractions.Fraction(float(mean[j] - np.longdouble(float(mean[j])))) - m)
            ev = abs(fractions.Fraction(float(var[j])) + fractions.Fraction(float(var[j] - np.longdouble(float(var[j])))) - v)
            assert em <= fractions.Fraction(2) ** -60 * max(spread, abs(m)), (stats.__name__, j)
            assert ev <= fractions.Fraction(2) ** -58 * v, (stats.__name__, j)


def test_exact_stats_agree_with_sklearn():
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(4)
    for dtype in (np.float32, np.float64):
        x = (rng.random((300, 16)) * 1e-3).astype(dtype)
        x[:, 0] = 0.25
        sk = StandardScaler().fit(x.astype(np.float64))
        mean, var = S.exact_stats(x)
        np.testing.assert_allclose(mean.astype(np.float64), sk.mean_, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S.scale_of(var).astype(np.float64), sk.scale_, rtol=1e-12, atol=0)
        assert S.scale_of(var)[0] == 1.0


def test_transforms_are_the_oracles():
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    x32, _ = S.family_matrix(33, 12, np.float32, 6)
    x64, _ = S.family_matrix(33, 11, np.float64, 7)
    for x, fn in ((x32, S.transform_f32), (x64, S.transform_f64)):
        mean = rng.standard_normal(x.shape[1]) * 1e-3
        scale = rng.random(x.shape[1]) + 1e-3
        assert np.array_equal(fn(x, mean, scale).view(np.int32), O.scaler_transform(x, mean, scale).astype(np.float32).view(np.int32))
    c = rng.integers(1, 1000, (5, 8)).astype(np.int32)
    assert np.array_equal(S.freq_rows(c), c / c.sum(1, keepdims=True))


@pytest.mark.parametrize("n", NS)
def test_replay_meets_the_bounds(n, capsys):
    """stats_ref.stats_whole stays inside bounds() for every family and both dtypes; kappa <= n + 1"""
    for dtype in (np.float32, np.float64):
        x, names = S.family_matrix(n, 12, dtype, 100 + n)
        assert set(names) == set(S.families(n, dtype, np.random.default_rng(0)))
        kappa, _, _ = S.bounds(x, n)
        assert (kappa >= 1).all() and (kappa <= n + 1).all(), dict(zip(names, kappa))
        mean, scale = R.stats_whole(x)
        r_m, r_s = S.error_ratios(x, mean, scale)
        with capsys.disabled():
            print(f"\n  replay {np.dtype(dtype).name} n={n}: largest error / bound: mean {r_m.max():.3g} ({names[int(r_m.argmax())]}), "
                  f"scale {r_s.max():.3g} ({names[int(r_s.argmax())]}), largest kappa {float(kappa.max()):.6g}")
        assert (r_m <= 1).all(), dict(zip(names, r_m))
        assert (r_s <= 1).all(), dict(zip(names, r_s))
        for j, name in enumerate(names):
            if name in ("const", "zero") or n == 1:
                assert mean[j] == x[0, j] and scale[j] == 1.0
