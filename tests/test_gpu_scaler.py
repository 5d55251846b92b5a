"""GPU tests of the scaler kernels (csrc/scaler.hip, csrc/scaler_device.h) against an exact reference (tests/scaler_ref.py): the statistics
column by column inside bounds derived from the algorithm (scaler_ref's docstring), the quotients and the transforms bit for bit.

Largest observed error / bound per dtype and row count (every width and column family of test_col_stats_against_the_exact_reference on
the MI355X; "replay" is stats_ref.stats_whole, the numpy replay without FMA, on 12 columns in tests/test_scaler_reference.py).  A ratio
above 1 is a failure of the kernel (or of the derivation), never a reason to widen a bound.

                      idl_col_stats (MI355X)    replay (numpy)
    dtype        n      mean     scale         mean     scale
    float32      1         0         0            0         0
    float32      2         0         0            0         0
    float32      3     0.167    0.0332
    float32      4         0    0.0215
    float32      5       0.2    0.0276       0.0479    0.0105
    float32    255     0.247    0.0524
    float32    256         0    0.0462
    float32    257     0.241    0.0476        0.145    0.0232
    float32   4097     0.249    0.0431        0.119    0.0153
    float32  65537     0.191    0.0354        0.176    0.0318
    float64      1         0         0            0         0
    float64      2      0.25    0.0136         0.25   0.00793
    float64      3     0.167     0.042
    float64      4      0.25    0.0362
    float64      5       0.2    0.0397          0.1    0.0202
    float64    255     0.249    0.0242
    float64    256     0.248     0.025
    float64    257     0.247    0.0728        0.208    0.0728
    float64   4097     0.248    0.0132        0.239   0.00857
    float64  65537     0.128    0.0101        0.203    0.0101
    (the mean's 0.25: half an ulp of the mean against the 4 EPS |mean| of its bound.  The other routes, largest over their cases: probe
    columns 6e-5 / 7e-5, idl_counts_stats 0.13 / 0.05, idl_counts_stream_* 0.32 / 0.08, idl_col_stats_stream 0.25 / 0.04, threshold 0.25 / 0.)
"""
import math

import numpy as np
import pytest

import scaler_ref as S
import stats_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                # guard words on either side of a guarded buffer
FILL = -12345
INT_MAX = 2 ** 31 - 1
RATIOS = {}               # (route, dtype name, n) -> [largest mean ratio, largest scale ratio]


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    print("\nlargest error / bound   route dtype n: mean scale")
    for (route, dtype, n), (rm, rs) in sorted(RATIOS.items()):
        print(f"    {route:<14} {dtype:<8} {n:>6}: {rm:8.3g} {rs:8.3g}")


def _dev():
    import torch
    return torch.device("cuda")


def _up(x, misalign=False):
    """a numpy array on the device; misalign: as a view that starts one element into its buffer"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x))
    if not misalign:
        return t.to(_dev())
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=_dev())
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.data_ptr() % 32 != 0
    return v


def _guarded(n, dtype, fill=FILL):
    import torch
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=_dev())
    return buf, buf[GUARD:GUARD + n]


def _untouched(buf):
    return bool((buf == FILL).all())


def _intact(buf, n):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n:] == FILL).all())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _check_stats(x, mean, scale, names, key):
    """the exact-reference bounds on a route's (mean, scale) device tensors for the host matrix x; the bitwise cases"""
    mean, scale = mean.cpu().numpy(), scale.cpu().numpy()
    n = x.shape[0]
    r_m, r_s = S.error_ratios(x, mean, scale)
    best = RATIOS.setdefault(key, [0.0, 0.0])
    best[0], best[1] = max(best[0], float(r_m.max())), max(best[1], float(r_s.max()))
    jm, js = int(r_m.argmax()), int(r_s.argmax())
    print(f"{key} f={x.shape[1]}: error / bound: mean {r_m[jm]:.3g} (column {jm} {names[jm]}), scale {r_s[js]:.3g} (column {js} {names[js]})")
    assert (r_m <= 1).all(), (key, x.shape, jm, names[jm], r_m[jm])
    assert (r_s <= 1).all(), (key, x.shape, js, names[js], r_s[js])
    for j, name in enumerate(names):
        if name in ("const", "zero") or n == 1:
            assert mean[j] == x[0, j] and scale[j] == 1.0, (key, x.shape, j, name, mean[j], scale[j])
    return mean, scale


# ------------------------------------------------------------------------------------------------ a. idl_col_stats
WIDTHS = [(12, False), (68, False), (1028, False), (10, False), (260, False), (12, True)]      # (f, misaligned): V = 4, 4, 4, 1, 1, 1
ROWS = [1, 2, 3, 4, 5, 255, 256, 257, 4097, 65537]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_col_stats_against_the_exact_reference(dtype, n):
    """idl_col_stats, both dtypes: 16-byte / 32-byte row reads (f = 12; 68: a second finishing workgroup; 1028: a second column block) and
    scalar ones (f = 10; 260: a second column block; 12 from a misaligned pointer); row counts around the unroll by 4 (1..5), around one
    row block (255..257), with 17 row blocks (4097: the finishing kernel's second trip) and with 256 blocks of 257 rows (65537)"""
    from idelucs_amd import utils as U
    for f, misalign in WIDTHS:
        if n > 4097 and f > 12:
            continue
        x, names = S.family_matrix(n, f, dtype, 1000 * f + n)
        mean, scale = U.col_stats(_up(x, misalign))
        _check_stats(x, mean, scale, names, ("col_stats", np.dtype(dtype).name, n))


# ------------------------------------------------------------------------------------------------ b. every row once
def _probe_rows(n):
    blocks, rpb = R.stat_row_blocks(n), R.rows_per_block(n)
    rows = {0, n - 1}
    for b in (0, 1, 15, 16, blocks - 1):
        rows |= {b * rpb, min((b + 1) * rpb, n) - 1}
    return sorted(rows)


@pytest.mark.parametrize("n", [4097, 65537])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_row_is_dropped_or_counted_twice(dtype, n):
    """columns that are zero but for a 1.0 at one probe row (the first and last row of the first, second, 16th, 17th and last row block;
    each probe in all four lanes of a 16-byte read): mean 1 / n and variance (1 / n)(1 - 1 / n).  A row missed leaves scale 1, a row
    taken twice misses the bound by ~1e13."""
    from idelucs_amd import utils as U
    assert R.stat_row_blocks(n) >= 17
    probes = _probe_rows(n)
    f = 4 * len(probes)
    x = np.zeros((n, f), dtype)
    for i, r in enumerate(probes):
        x[r, 4 * i:4 * i + 4] = 1.0
    mean, scale = U.col_stats(_up(x))
    names = [f"probe row {r}" for r in probes for _ in range(4)]
    mean, scale = _check_stats(x, mean, scale, names, ("probes", np.dtype(dtype).name, n))
    want = math.sqrt((1.0 / n) * (1.0 - 1.0 / n))
    assert (np.abs(scale / want - 1) < 1e-8).all() and (np.abs(mean - 1.0 / n) < 1e-15).all()


# ------------------------------------------------------------------------------------------------ c. the scale threshold
@pytest.mark.parametrize("n", [2, 256, 512])
def test_scale_threshold_is_exact(n):
    """float64, half the rows 1.0 and half 1 + k 2^-52: every intermediate of the kernel is exact (n is a power of two), the variance is
    (k 2^-53)^2.  k = 19 is below sklearn's 10 eps = 20 * 2^-53 (scale 1), k = 20 is equal to it (kept: the rule is "less than"), k = 21
    above.  Columns: the halves one after the other / interleaved, and either value in row 0; f = 4 (32-byte reads) and f = 5."""
    from idelucs_amd import utils as U
    u = 2.0 ** -52
    r = np.arange(n)
    high = np.stack([r >= n // 2, r % 2 == 1, r < n // 2, r % 2 == 0, r >= n // 2], axis=1)
    assert 10 * S.SK_EPS == 20 * 2.0 ** -53
    for k in (19, 20, 21):
        for f in (4, 5):
            x = np.where(high[:, :f], 1.0 + k * u, 1.0)
            mean, scale = U.col_stats(_up(x))
            mean, scale = _check_stats(x, mean, scale, [f"k={k}"] * f, ("threshold", "float64", n))
            want = 1.0 if k == 19 else k * 2.0 ** -53
            assert (scale == want).all(), (n, k, f, scale, want)
            if k % 2 == 0:
                assert (mean == 1.0 + k * 2.0 ** -53).all(), (n, k, f, mean)


# ------------------------------------------------------------------------------------------------ d. the streamed forms
def _cuts(n):
    """one row at a time for 20 rows; 7, 8 and 9 rows (SLAB_ROWS = 8); a chunk inside one row block; one over three row blocks; the rest"""
    rpb = R.rows_per_block(n)
    out, lo = [], 0
    for length in [1] * 20 + [7, 8, 9, rpb // 4, 2 * rpb]:
        out.append((lo, lo + length))
        lo += length
    inside, three = out[-2], out[-1]
    assert inside[0] // rpb == (inside[1] - 1) // rpb and inside[0] % rpb != 0
    assert (three[1] - 1) // rpb - three[0] // rpb == 2
    assert lo < n
    return out + [(lo, n)]


def _counts(n, f, rng, shift=0):
    """synthetic int32 counts [n, f], the row's type by (row + shift) % 4: k-mer-like counts (pseudocount 1); all ones; a total of exactly
    2^31 - 1 (one huge entry, ones elsewhere); a total that is a power of two"""
    c = rng.integers(1, 60, (n, f)).astype(np.int64)
    c[:, 0] += rng.integers(0, 70000, n)
    kind = (np.arange(n) + shift) % 4
    col = rng.integers(0, f, n)
    for r in range(n):
        if kind[r] == 1:
            c[r] = 1
        elif kind[r] == 2:
            c[r] = 1
            c[r, col[r]] = INT_MAX - (f - 1)
        elif kind[r] == 3:
            t = int(c[r].sum())
            c[r, col[r]] += (1 << (t - 1).bit_length()) - t
    assert (c.sum(1) <= INT_MAX).all()
    return c.astype(np.int32)


STREAM_SHAPES = [(4097, 1028), (65537, 8)]


@pytest.mark.parametrize("n,f", STREAM_SHAPES)
def test_col_stats_stream_cut_anywhere(n, f):
    """idl_col_stats_stream over one reused chunk buffer, the workspace NaN before the first chunk: idl_col_stats' float32 statistics bit
    for bit, and inside the exact-reference bounds"""
    import torch
    from idelucs_amd import _lib, utils as U
    L = _lib.lib
    x, names = S.family_matrix(n, f, np.float32, 7 * n + f)
    cuts = _cuts(n)
    buf = torch.empty((max(hi - lo for lo, hi in cuts), f), dtype=torch.float32, device=_dev())
    ws_bytes = int(L.idl_col_stats_stream_workspace(n, f))
    assert ws_bytes == (2 * R.stat_row_blocks(n) + 1) * f * 8
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=_dev())
    sp = U._stream_ptr()
    for lo, hi in cuts:
        buf[:hi - lo].copy_(torch.from_numpy(x[lo:hi]))
        _lib.check(L.idl_col_stats_stream(U._ptr(buf), lo, hi - lo, n, f, U._ptr(ws), sp))
    mean_buf, mean = _guarded(f, torch.float64)
    scale_buf, scale = _guarded(f, torch.float64)
    _lib.check(L.idl_col_stats_stream_finish(n, f, U._ptr(ws), U._ptr(mean), U._ptr(scale), sp))
    m_whole, s_whole = U.col_stats(_up(x))
    assert torch.equal(mean, m_whole) and torch.equal(scale, s_whole)
    assert _intact(mean_buf, f) and _intact(scale_buf, f)
    _check_stats(x, mean, scale, names, ("rows_stream", "float32", n))


@pytest.mark.parametrize("n,f", STREAM_SHAPES)
def test_counts_stream_cut_anywhere(n, f):
    """idl_row_totals_i32 + idl_counts_stream_stats per chunk (one reused buffer, NaN workspace) + idl_counts_stream_finish: idl_col_stats
    of the float64 frequency rows bit for bit, and inside the exact-reference bounds"""
    import torch
    from idelucs_amd import _lib, utils as U
    L = _lib.lib
    counts = _counts(n, f, np.random.default_rng(n + f))
    freq = S.freq_rows(counts)
    cuts = _cuts(n)
    buf = torch.empty((max(hi - lo for lo, hi in cuts), f), dtype=torch.int32, device=_dev())
    ws = torch.full((int(L.idl_counts_stream_workspace(n, f)) // 8,), float("nan"), dtype=torch.float64, device=_dev())
    tot_buf, tot = _guarded(n, torch.int32)
    sp = U._stream_ptr()
    for lo, hi in cuts:
        buf[:hi - lo].copy_(torch.from_numpy(counts[lo:hi]))
        _lib.check(L.idl_row_totals_i32(U._ptr(buf), hi - lo, f, U._ptr(tot[lo:hi]), sp))
        _lib.check(L.idl_counts_stream_stats(U._ptr(buf), U._ptr(tot[lo:hi]), lo, hi - lo, n, f, U._ptr(ws), sp))
    mean = torch.empty(f, dtype=torch.float64, device=_dev())
    scale = torch.empty(f, dtype=torch.float64, device=_dev())
    _lib.check(L.idl_counts_stream_finish(n, f, U._ptr(ws), U._ptr(mean), U._ptr(scale), sp))
    assert np.array_equal(tot.cpu().numpy(), counts.sum(1, dtype=np.int64)) and _intact(tot_buf, n)
    m_whole, s_whole = U.col_stats(_up(freq))
    assert torch.equal(mean, m_whole) and torch.equal(scale, s_whole)
    _check_stats(freq, mean, scale, [f"column {j}" for j in range(f)], ("counts_stream", "float64", n))


# ------------------------------------------------------------------------------------------------ e. the counts routes
def _counts_stats(counts):
    """idl_counts_stats on host counts -> (mean, scale, totals) device tensors"""
    import torch
    from idelucs_amd import _lib, utils as U
    n, f = counts.shape
    dc = _up(counts)
    mean = torch.empty(f, dtype=torch.float64, device=_dev())
    scale = torch.empty(f, dtype=torch.float64, device=_dev())
    tot_buf, tot = _guarded(n, torch.int32)
    ws = torch.full((int(_lib.lib.idl_counts_stats_workspace(n, f)) // 8,), float("nan"), dtype=torch.float64, device=_dev())
    _lib.check(_lib.lib.idl_counts_stats(U._ptr(dc), n, f, U._ptr(mean), U._ptr(scale), U._ptr(tot), U._ptr(ws), U._stream_ptr()))
    assert _intact(tot_buf, n)
    return mean, scale, tot


@pytest.mark.parametrize("f", [256, 768, 1024, 4096, 16384])
def test_counts_stats_on_synthetic_counts(f):
    """idl_counts_stats with one wave, three waves, 256 and 1024 threads, and four column groups a thread; 1..5 and 9 rows (the four-row
    trips and their remainders), 257 (two row blocks) and, at f = 256, 4097 (the finishing kernel's second trip): the row totals, the
    statistics of idl_col_stats on the float64 frequency rows bit for bit, and the exact-reference bounds"""
    import torch
    from idelucs_amd import utils as U
    for n in [1, 2, 3, 4, 5, 9, 257] + ([4097] if f == 256 else []):
        counts = _counts(n, f, np.random.default_rng(f + n), shift=n)
        freq = S.freq_rows(counts)
        mean, scale, tot = _counts_stats(counts)
        assert np.array_equal(tot.cpu().numpy(), counts.sum(1, dtype=np.int64)), (f, n)
        m_whole, s_whole = U.col_stats(_up(freq))
        assert torch.equal(mean, m_whole) and torch.equal(scale, s_whole), (f, n)
        _check_stats(freq, mean, scale, [f"column {j}" for j in range(f)], ("counts_stats", "float64", n))


def test_counts_stats_refusals_write_nothing():
    """widths no workgroup shape fits (f / 4 = 34: no multiple of 64; f = 8192: two column groups) and a counts pointer 4 bytes off a
    16-byte boundary: IDL_ERR_ARG before anything is launched"""
    import torch
    from idelucs_amd import _lib, utils as U
    L = _lib.lib
    sp = U._stream_ptr()
    for f, off in ((136, 0), (8192, 0), (256, 1)):
        n = 5
        counts = torch.ones(n * f + 4, dtype=torch.int32, device=_dev())[off:off + n * f]
        bufs = [_guarded(f, torch.float64)[0], _guarded(f, torch.float64)[0], _guarded(n, torch.int32)[0],
                _guarded(int(L.idl_counts_stats_workspace(n, f)) // 8, torch.float64)[0]]
        mean, scale, tot, ws = (b[GUARD:] for b in bufs)
        rc = L.idl_counts_stats(U._ptr(counts), n, f, U._ptr(mean), U._ptr(scale), U._ptr(tot), U._ptr(ws), sp)
        torch.cuda.synchronize()
        assert rc == _lib.IDL_ERR_ARG, (f, off, rc)
        assert all(_untouched(b) for b in bufs), (f, off)


@pytest.mark.parametrize("f", [4, 8, 256, 4096, 4100, 16384])
def test_row_totals(f):
    """idl_row_totals_i32: a wave a row (f / 4 <= 1024: f = 4 and 8 leave lanes idle, 256 is one remainder trip, 4096 four unrolled trips)
    and a workgroup a row (4100: one unrolled trip and a remainder trip of one lane; 16384: four unrolled trips); 1, 3, 4 and 5 rows
    (four rows a workgroup on the wave path); a row whose total is exactly 2^31 - 1"""
    import torch
    from idelucs_amd import _lib, utils as U
    for rows in (1, 3, 4, 5):
        counts = _counts(rows, f, np.random.default_rng(f + rows), shift=2 if rows == 1 else 0)
        assert (counts.sum(1, dtype=np.int64) == INT_MAX).any()
        tot_buf, tot = _guarded(rows, torch.int32)
        dc = _up(counts)
        _lib.check(_lib.lib.idl_row_totals_i32(U._ptr(dc), rows, f, U._ptr(tot), U._stream_ptr()))
        assert np.array_equal(tot.cpu().numpy(), counts.sum(1, dtype=np.int64)), (f, rows)
        assert _intact(tot_buf, rows)


# ------------------------------------------------------------------------------------------------ f. count_freq at float64 resolution
def _next_prime(x):
    while any(x % d == 0 for d in range(2, math.isqrt(x) + 1)):
        x += 1
    return x


def _totals():
    kmer = [4 ** k + length - k + 1 for k, length in ((4, 1500), (6, 10000), (6, 70000), (7, 150000))]      # 4^k pseudocounts + the windows
    primes = [_next_prime(2 ** 20 - 40), _next_prime(2 ** 20 + 1), _next_prime(2 ** 30 - 40), _next_prime(2 ** 30 + 1)]
    return [3, 7, 2 ** 24 - 1, INT_MAX] + primes + kmer + [2 ** 10, 2 ** 20, 2 ** 30]


def _composition(total, f, rng):
    """f non-negative integers that add up to total"""
    cuts = np.sort(rng.integers(0, total + 1, f - 1))
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int32)


def test_count_freq_is_the_correctly_rounded_quotient():
    """With one row the mean is the shift x0 = count_freq(c, T) itself, in float64: it must be numpy's c / T (IEEE division) bit for bit.
    Through idl_counts_stats the total is the row's own (two rows a total: T - 1 and 1 among zeros; a random composition of T); through
    idl_counts_stream_stats the totals array is set by hand, so any c in 0..T goes with any T (0, 1, T - 1, T and random values)."""
    import torch
    from idelucs_amd import _lib, utils as U
    L = _lib.lib
    f = 256
    rng = np.random.default_rng(17)
    sp = U._stream_ptr()
    bad = []
    for total in _totals():
        edge = np.zeros(f, np.int32)
        edge[:2] = [total - 1, 1]
        for row in (edge, _composition(total, f, rng)):
            assert int(row.sum(dtype=np.int64)) == total
            mean, scale, tot = _counts_stats(row[None, :])
            got = mean.cpu().numpy()
            assert int(tot[0]) == total and bool((scale == 1.0).all())
            want = row.astype(np.float64) / float(total)
            bad += [("counts_stats", total, int(c)) for c in row[_bits(got) != _bits(want)]]
        row = rng.integers(0, total + 1, f).astype(np.int32)
        row[:4] = [0, 1, total - 1, total]
        ws = torch.full((int(L.idl_counts_stream_workspace(1, f)) // 8,), float("nan"), dtype=torch.float64, device=_dev())
        mean = torch.empty(f, dtype=torch.float64, device=_dev())
        scale = torch.empty(f, dtype=torch.float64, device=_dev())
        d_row, d_total = _up(row), _up(np.array([total], np.int32))
        _lib.check(L.idl_counts_stream_stats(U._ptr(d_row), U._ptr(d_total), 0, 1, 1, f, U._ptr(ws), sp))
        _lib.check(L.idl_counts_stream_finish(1, f, U._ptr(ws), U._ptr(mean), U._ptr(scale), sp))
        want = row.astype(np.float64) / float(total)
        bad += [("counts_stream", total, int(c)) for c in row[_bits(mean.cpu().numpy()) != _bits(want)]]
        assert bool((scale == 1.0).all())
    assert not bad, bad[:20]


# ------------------------------------------------------------------------------------------------ g. the transforms, bit for bit
def _transform_case(n, f, dtype, seed):
    """a family matrix with the exact reference's statistics rounded to float64 (a constant column: x == mean and scale == 1), and two
    columns set by hand whose quotients leave float32's normal range: +-1e30 (1 + u) / 1e-10 -> +-inf, +-1e-30 (1 + u) / 1e10 -> subnormal"""
    x, names = S.family_matrix(n, f, dtype, seed)
    m, v = S.exact_stats(x)
    mean, scale = m.astype(np.float64), S.scale_of(v).astype(np.float64)
    j_const, j_over, j_sub = names.index("const"), names.index("alternating"), names.index("benign")
    assert mean[j_const] == 0.25 and scale[j_const] == 1.0 and (x[:, j_const] == mean[j_const]).all()
    alt = x[:, j_over].astype(np.float64)
    x[:, j_over], mean[j_over], scale[j_over] = (alt * 1e30).astype(dtype), 0.0, 1e-10
    x[:, j_sub], mean[j_sub], scale[j_sub] = (alt * 1e-30).astype(dtype), 0.0, 1e10
    want = (S.transform_f32 if np.dtype(dtype) == np.float32 else S.transform_f64)(x, mean, scale)
    assert np.isinf(want[:, j_over]).all() and (want[:, j_over] > 0).any() and (want[:, j_over] < 0).any()
    assert ((np.abs(want[:, j_sub]) < 1.1754944e-38) & (want[:, j_sub] != 0)).all()
    assert np.isfinite(np.delete(want, j_over, axis=1)).all()
    return x, mean, scale, want


@pytest.mark.parametrize("dtype,f,misalign", [(np.float32, 1028, False), (np.float32, 10, False), (np.float32, 12, True),
                                              (np.float64, 12, False), (np.float64, 10, False)])
def test_standardise_bit_for_bit(dtype, f, misalign):
    """idl_standardise: float32 by 16-byte vectors (f = 1028), float32 scalar (f = 10, and f = 12 from a misaligned pointer), float64"""
    import torch
    from idelucs_amd import utils as U
    n = 37
    x, mean, scale, want = _transform_case(n, f, dtype, 50 + f)
    y_buf, y = _guarded(n * f, torch.float32)
    U.standardise(_up(x, misalign), _up(mean), _up(scale), out=y.view(n, f))
    got = y.cpu().numpy().reshape(n, f)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:10]
    assert _intact(y_buf, n * f)


def test_standardise_grid_stride_wraps():
    """float32, f = 4096, one row more than cus * 8 * 256 16-byte elements: the vector kernel's grid-stride loop takes a second trip"""
    import torch
    from idelucs_amd import utils as U
    f = 4096
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 8 * 256 * 4 // f + 1
    assert n * f // 4 > cus * 8 * 256
    rng = np.random.default_rng(23)
    x = (rng.random((n, f)) * 1e-3).astype(np.float32)
    mean, scale = 5e-4 + 1e-5 * rng.standard_normal(f), 2.9e-4 * (1 + rng.random(f))
    scale[::7] = 1.0
    y_buf, y = _guarded(n * f, torch.float32)
    U.standardise(_up(x), _up(mean), _up(scale), out=y.view(n, f))
    assert np.array_equal(_bits(y.cpu().numpy().reshape(n, f)), _bits(S.transform_f32(x, mean, scale)))
    assert _intact(y_buf, n * f)


def test_counts_standardise_on_a_row_shard():
    """idl_counts_standardise on rows 3..7 of synthetic counts (all four row types) with their totals: StandardScaler.transform of the
    float64 frequency rows, one rounding to float32"""
    import torch
    from idelucs_amd import _lib, utils as U
    n, f, lo, hi = 9, 1024, 3, 8
    counts = _counts(n, f, np.random.default_rng(31))
    freq = S.freq_rows(counts)
    m, v = S.exact_stats(freq)
    mean, scale = m.astype(np.float64), S.scale_of(v).astype(np.float64)
    dc, dt, d_mean, d_scale = _up(counts), _up(counts.sum(1, dtype=np.int64).astype(np.int32)), _up(mean), _up(scale)
    y_buf, y = _guarded((hi - lo) * f, torch.float32)
    _lib.check(_lib.lib.idl_counts_standardise(U._ptr(dc[lo:hi]), U._ptr(dt[lo:hi]), hi - lo, f, U._ptr(d_mean), U._ptr(d_scale), U._ptr(y), U._stream_ptr()))
    want = S.transform_f64(freq[lo:hi], mean, scale)
    assert np.array_equal(_bits(y.cpu().numpy().reshape(hi - lo, f)), _bits(want))
    assert _intact(y_buf, (hi - lo) * f)


@pytest.mark.parametrize("f", [1028, 10])
@pytest.mark.parametrize("with_inv", [False, True])
def test_gather_pairs_bit_for_bit(f, with_inv):
    """idl_gather_pairs_at, divide and reciprocal form, tiled (f = 1028) and row by row (f = 10), for batches around GATHER_ROWS = 8, two
    mimic views, pairs on the first and last row of each view, with and without a device-side offset into the pair list: transform_f32 of
    the gathered rows.  With f % 4 != 0 an inv_scale is ignored (the divide form): it is all NaN here.
    The reciprocal form's domain is finite features without -0.0f (std_f32_rcp gives +0 where the division gives -0 for that input, and
    NaN for an infinite one; the vectoriser produces neither), so the features here hold neither."""
    import torch
    from idelucs_amd import _lib, utils as U
    n, views = 33, 3
    feats = np.stack([S.family_matrix(n, f, np.float32, 70 + f + v)[0] for v in range(views)])
    assert np.isfinite(feats).all() and not np.signbit(feats[feats == 0]).any()
    m, v = S.exact_stats(feats[0])
    mean, scale = m.astype(np.float64), S.scale_of(v).astype(np.float64)
    inv = (1.0 / scale) if f % 4 == 0 else np.full(f, np.nan)
    rng = np.random.default_rng(f)
    idx = np.concatenate([[0, n - 1, n, 2 * n - 1], rng.integers(0, (views - 1) * n, 8)]).astype(np.int64)
    d_feats, d_idx, d_mean, d_scale, d_inv = _up(feats), _up(idx), _up(mean), _up(scale), _up(inv)
    d_base = _up(np.array([3], np.int64))
    for batch in (1, 7, 8, 9):
        for base in (0, 3):
            y_buf, y = _guarded(2 * batch * f, torch.float32)
            _lib.check(_lib.lib.idl_gather_pairs_at(U._ptr(d_feats), n, f, n * f, U._ptr(d_idx), U._ptr(d_base) if base else None, batch,
                                                    U._ptr(d_mean), U._ptr(d_scale), U._ptr(d_inv) if with_inv else None, U._ptr(y),
                                                    U._stream_ptr()))
            pair = idx[base:base + batch]
            rows = np.concatenate([feats[0][pair % n], feats[1 + pair // n, pair % n]])
            got = y.cpu().numpy().reshape(2 * batch, f)
            assert np.array_equal(_bits(got), _bits(S.transform_f32(rows, mean, scale))), (f, with_inv, batch, base)
            assert _intact(y_buf, 2 * batch * f)


def test_gather_pairs_refuses_misaligned_features():
    import torch
    from idelucs_amd import _lib, utils as U
    n, f = 5, 1028
    feats = _up(np.zeros((2, n, f), np.float32), misalign=True)
    stats, idx = _up(np.ones(f)), _up(np.zeros(1, np.int64))
    y_buf, y = _guarded(2 * f, torch.float32)
    rc = _lib.lib.idl_gather_pairs_at(U._ptr(feats), n, f, n * f, U._ptr(idx), None, 1, U._ptr(stats), U._ptr(stats), None, U._ptr(y), U._stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.IDL_ERR_ARG and _untouched(y_buf)
