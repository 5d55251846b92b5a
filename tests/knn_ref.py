"""float64 reference, the specification of both stages and the test inputs for the core-distance kernels of csrc/knn.hip
(idl_knn_window, idl_knn_select).  Plain numpy: nothing here imports the package under test -- the one number the reference shares
with it, the rounding constant GRAM_ERR, is an argument (the tests pass posthoc.KNN_GRAM_ERR, and the kernel's own copy is tied to it
by comparing the `delta` the kernel writes with delta_ref).  Used by tests/test_knn_reference.py (the reference against itself and
against mst_ref, no GPU) and tests/test_gpu_knn_stages.py (the kernels, column by column).

THE CHAIN OF CLAIMS (csrc/knn.hip, head comment).  A row a of a wave centred on the point m = centre_of(row), a column b:
  1. idl_knn_window's value of |a - b|^2 is off by at most GRAM_ERR (|a - m|^2 + |b - m|^2); a column that can come out under `hi`
     has |b - m| <= |a - m| + sqrt(hi), so delta / 2, delta = delta_ref(...), bounds the error of every such column;
  2. hence: a column whose true value lies in [lo + delta/2, hi - delta/2) is kept, exactly once; one at or above hi + delta/2 or
     below lo - delta/2 is not; cnt_lo lies between the counts of the columns truly below lo -+ delta/2; cand_cnt is the number of
     columns that came out inside the window, whether or not the slot (cap) could hold them;
  3. idl_knn_select picks v, the (k - cnt_lo)-th smallest kept value (clamped into [lo, hi]); v is within delta/2 of the true k-th,
     so with v - delta > lo and v + delta < hi every candidate for the k-th is among the kept values within v -+ delta: their
     float64 distances (difference vector, sklearn's order) and the rank inside that band give the k-th exactly.
must_succeed() turns 3 around: the rows for which the claims OBLIGE status 0, from float64 values alone.  select_spec() restates
the selection on given slots, whatever put them there."""
import functools

import numpy as np

from mst_ref import _columns, _sq_dist_to  # noqa: F401  (the same arithmetic, row by row: tests/test_knn_reference.py compares)

F32 = np.float32
ROWS_WAVE = 64                # rows of a wave: they share a centre
BAND_CAP = 1024               # members idl_knn_select's exact band can hold
NOTHING_BELOW = -1.0e30       # the caller's `lo` where the lower rank does not exist


def f32(a):
    """The nearest float32, as float64 (what the device holds exactly)."""
    return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def true_d2(x, rows=None, block=256):
    """[len(rows), n] float64 squared distances from the difference vector: t = a_c - b_c, acc += t * t coordinate by coordinate,
    product and sum each rounded (sklearn's EuclideanDistance; mst_ref._sq_dist_to's operations on a block of rows at a time)."""
    xt = _columns(x)
    n = xt.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = np.empty((len(rows), n))
    for b0 in range(0, len(rows), block):
        r = rows[b0:b0 + block]
        acc = np.zeros((len(r), n))
        for col in xt:
            t = col[r][:, None] - col[None, :]
            acc += t * t
        out[b0:b0 + block] = acc
    return out


def d2_to(x, row, idx):
    """true_d2's value of (row, j) for the columns j in idx."""
    x = np.asarray(x, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    acc = np.zeros(len(idx))
    for c in range(x.shape[1]):
        t = x[row, c] - x[idx, c]
        acc += t * t
    return acc


def centre_of(row, row0, last):
    """The row a row's wave centres on in a launch over [row0, last]: row0 + 256 blk + 64 wv, clamped to last."""
    rel = np.asarray(row, dtype=np.int64) - row0
    return np.minimum(row0 + rel // ROWS_WAVE * ROWS_WAVE, last)


def delta_ref(x, hi, row0, rows, gram_err):
    """[rows] float64: the `delta` idl_knn_window must write for the rows row0 .. row0 + rows - 1 given their `hi`."""
    x = np.asarray(x, dtype=np.float64)
    r = row0 + np.arange(rows)
    diff = x[r] - x[centre_of(r, row0, row0 + rows - 1)]
    sqa = (diff * diff).sum(1)
    reach = np.sqrt(sqa) + np.sqrt(np.maximum(np.asarray(hi, dtype=np.float64), 0.0))
    return 2.0 * gram_err * (sqa + 1.001 * reach * reach)


def kth_d2(d2, k):
    """The k-th smallest (1-based) of every row of d2."""
    return np.partition(d2, k - 1, axis=1)[:, k - 1]


def must_succeed(d2, k, lo, hi, delta, cap):
    """[rows] bool: the rows idl_knn_select is OBLIGED to finish with status 0 (module docstring, 3).  d2 [rows, n]: true values;
    lo, hi, delta per row.  The selected v lies within delta/2 of the k-th, so v -+ delta stays inside (lo, hi) when the k-th is
    1.5 delta away from both ends; the band v -+ delta holds computed values, each within delta/2 of the truth: true values within
    2 delta of the k-th; the slot holds what came out inside the window: true values within delta/2 of it."""
    lo, hi, delta = (np.asarray(a, dtype=np.float64) for a in (lo, hi, delta))
    kth = kth_d2(d2, k)
    band = (np.abs(d2 - kth[:, None]) <= 2.0 * delta[:, None]).sum(1)
    slot = ((d2 >= (lo - delta / 2)[:, None]) & (d2 < (hi + delta / 2)[:, None])).sum(1)
    return (kth - 1.5 * delta > lo) & (kth + 1.5 * delta < hi) & (band <= BAND_CAP) & (slot <= cap)


def rank_window(d2, k, w):
    """(lo, hi) float32 per row: the float32 roundings of the true values at ranks k - w and k + w (1-based); NOTHING_BELOW where
    the lower rank does not exist."""
    srt = np.sort(d2, axis=1)
    hi = srt[:, k + w - 1].astype(F32)
    lo = srt[:, k - w - 1].astype(F32) if k - w >= 1 else np.full(len(d2), NOTHING_BELOW, dtype=F32)
    return lo, hi


def select_spec(x, row, k, lo, hi, delta, cnt_lo, cand_cnt, cap, cand_d2, cand_idx):
    """(status, core or None): what idl_knn_select must answer for one row's slot, restated: the kept values clamped into [lo, hi]
    (a NaN counts as lo) and sorted, the (k - cnt_lo)-th of them = v; the edge test; the band v -+ delta on the values as kept; the
    float64 distances of its members and the rank inside it.  float32 where the kernel compares float32 values."""
    lo, hi, delta = F32(lo), F32(hi), F32(delta)
    if cand_cnt > cap:
        return 2, None
    want = int(k) - int(cnt_lo)
    if want < 1 or want > cand_cnt:
        return 1, None
    d2 = np.asarray(cand_d2[:cand_cnt], dtype=F32)
    ix = np.asarray(cand_idx[:cand_cnt], dtype=np.int64)
    v = np.sort(np.minimum(np.fmax(d2, lo), hi))[want - 1]
    under, over = F32(v - delta), F32(v + delta)
    if not under > lo or not over < hi:
        return 3, None
    below = d2 < under
    band = ~below & (d2 <= over)
    nb = int(band.sum())
    if nb > BAND_CAP:
        return 4, None
    target = want - 1 - int(below.sum())
    if target < 0 or target >= nb:
        return 3, None
    return 0, float(np.sqrt(np.sort(d2_to(x, row, ix[band]))[target]))


SENT_F, SENT_I = -7.0, -77          # what the tests fill every output buffer with before a launch


def check_window(out, d2, lo, hi, dref, cap, what):
    """THE assertions on a window pass (module docstring, 1 and 2), for every row of the launch.  out: cnt_lo, cand_cnt, delta [rows],
    cand_d2, cand_idx [rows, cap] as the pass left them in buffers filled with SENT_F / SENT_I; d2 [rows, n] true values; lo, hi as
    given to the pass; dref = delta_ref(...).  Prints and returns the largest |kept value - true| / (dref / 2)."""
    rows, n = d2.shape
    lo, hi, dref = (np.asarray(a, dtype=np.float64) for a in (lo, hi, dref))
    cnt_lo, cnt = out["cnt_lo"].astype(np.int64), out["cand_cnt"].astype(np.int64)
    val, idx = out["cand_d2"].astype(np.float64).reshape(rows, cap), out["cand_idx"].astype(np.int64).reshape(rows, cap)
    assert np.allclose(out["delta"].astype(np.float64), dref, rtol=1e-5, atol=0.0), f"{what}: delta is not the specified bound"
    assert (cnt >= 0).all() and (cnt_lo >= 0).all(), f"{what}: a count was not written"
    used = np.arange(cap)[None, :] < np.minimum(cnt, cap)[:, None]
    assert (out["cand_d2"].reshape(rows, cap)[~used] == F32(SENT_F)).all() and (idx[~used] == SENT_I).all(), \
        f"{what}: a slot past a row's count was written"
    assert ((idx >= 0) & (idx < n))[used].all(), f"{what}: a kept index outside [0, n)"
    ri = np.broadcast_to(np.arange(rows)[:, None], (rows, cap))
    kept = np.zeros((rows, n), dtype=bool)
    kept[ri[used], idx[used]] = True
    assert (kept.sum(1) == np.minimum(cnt, cap)).all(), f"{what}: a column kept twice in a row"
    half = (dref / 2)[:, None]
    err = np.abs(val - np.take_along_axis(d2, np.where(used, idx, 0), axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(used, np.where(half > 0.0, err / half, np.where(err > 0.0, np.inf, 0.0)), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: largest |kept value - true| / (delta / 2) = {worst:.3g}; kept per row <= {int(cnt.max())}")
    assert not (used & ~(err <= half)).any(), f"{what}: a kept value is further than delta / 2 from the true squared distance (worst ratio {worst:.3g})"
    inner = (d2 >= lo[:, None] + half) & (d2 < hi[:, None] - half)
    outer = (d2 >= lo[:, None] - half) & (d2 < hi[:, None] + half)
    assert not (kept & ~outer).any(), f"{what}: a column truly outside the window was kept"
    fits = cnt <= cap
    assert not (inner & ~kept)[fits].any(), f"{what}: a column truly inside the window was not kept"
    assert (inner.sum(1) <= cnt).all() and (cnt <= outer.sum(1)).all(), f"{what}: cand_cnt is not the number of columns in the window"
    assert ((d2 < lo[:, None] - half).sum(1) <= cnt_lo).all() and (cnt_lo <= (d2 < lo[:, None] + half).sum(1)).all(), \
        f"{what}: cnt_lo is not the number of columns below the window"
    return worst


# ------------------------------------------------------------------------------------------------ inputs
def blobs(n, seed, noise=20, spread=(0.3, 0.9), offset=0.0):
    """tests/test_gpu_knn.py's _blobs: seven Gaussian blobs of 64 coordinates, the first n // noise rows uniform background."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(7, 64)) * 2.5 + offset
    truth = rng.integers(0, 7, n)
    x = centres[truth] + rng.normal(size=(n, 64)) * rng.uniform(*spread, size=(7,))[truth][:, None]
    if noise:
        x[: n // noise] = rng.uniform(-8, 8, size=(n // noise, 64)) + offset
    return f32(x)


def _tight(n, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(6, 64)) * 30.0
    x = centres[rng.integers(0, 6, n)] + rng.normal(size=(n, 64)) * 0.05
    x[: n // 50] = rng.uniform(-60, 60, size=(n // 50, 64))
    return f32(x)


def _duplicates(n, seed):
    x = blobs(n, seed, noise=0)
    x[n // 2:] = x[np.random.default_rng(seed + 1).integers(0, 40, n - n // 2)]
    return x


def spatial_order(x, pivots=16, seed=0):
    """The rows grouped by their nearest of `pivots` of them (a stable sort of the group number): neighbours in memory are
    neighbours in space, as posthoc._spatial_order arranges it -- WITHOUT its padding to whole waves: a wave may straddle groups."""
    x = np.asarray(x, dtype=np.float64)
    rng = np.random.default_rng(seed)
    xc = x - x.mean(0)
    p = xc[rng.choice(len(x), min(pivots, len(x)), replace=False)]
    group = ((p * p).sum(1)[None, :] - 2.0 * (xc @ p.T)).argmin(1)
    return np.argsort(group, kind="stable")


DATASETS = ("blobs", "offset", "tight", "duplicates")
BENIGN = ("blobs", "offset")             # must_succeed has to cover 90 % of their rows, in both orders
ORDERS = ("spatial", "shuffled")
KW = ((2, 16), (21, 16), (200, 24))      # (k, w): the window spans the true ranks k - w .. k + w


def window_cap(w):
    return -(-4 * (2 * w + 1) // 256) * 256


@functools.lru_cache(maxsize=None)
def dataset(name, order, n=1500):
    """x [n, 64] float64 holding float32 values, read-only.  shuffled: a wave's centre is a cluster distance away from its rows."""
    seed = 40 + DATASETS.index(name)
    if name in ("blobs", "offset"):
        x = blobs(n, seed, offset=4.0e4 if name == "offset" else 0.0)
    elif name == "tight":
        x = _tight(n, seed)
    else:
        x = _duplicates(n, seed)
    perm = spatial_order(x) if order == "spatial" else np.random.default_rng(seed + 100).permutation(n)
    x = np.ascontiguousarray(x[perm])
    assert np.array_equal(f32(x), x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, order, n=1500):
    """(x, true_d2(x)) of a dataset, computed once and read-only."""
    x = dataset(name, order, n)
    d2 = true_d2(x)
    d2.setflags(write=False)
    return x, d2


FAMILIES = ("stagnation", "same_sign", "cancelling", "far_column")
BIG_AT = (0, 15, 16, 47, 63)             # the kernel permutes the k order per 16-lane group: first / last of a group, first / last of all


def _block(m, pts):
    """One wave's rows: m first, then the points, m repeated up to 64 rows."""
    assert len(pts) < ROWS_WAVE
    return np.concatenate([m[None, :], pts, np.repeat(m[None, :], ROWS_WAVE - 1 - len(pts), axis=0)])


@functools.lru_cache(maxsize=None)
def constructed(family):
    """dict(x [128, 64], far [128] bool, near_hi): two waves, each with its centre m at its first row, the other rows m + e, the
    columns m +- e' (every point is row and column), built so that float32 holds every coordinate AND every e = point - m exactly:
      stagnation  one coordinate of e is +-1, at BIG_AT; the other 63 are +-2^-12 (1 - t 2^-10), t = 1 .. 3: their squares lie just
                  under half an ulp of 1, so a float32 sum that has taken in the large term first loses every one of them
      same_sign   the entries of e are a permutation of 1 + j 2^-12, j = 0 .. 63: against m + e' 64 positive products, against
                  m - e' 64 negative ones, none of which float32 holds
      cancelling  every point is m + e + t_i, |e| = 8 and |t_i - t_j| about 7e-3: the norms exceed the distances a thousandfold
      far_column  rows m + e, |e| = 1, near columns m +- e', far columns m + 10^4 f, |f| = 1 (far[j]); near_hi: the `hi` of a near
                  row, twice the largest squared distance between near points (the far columns must come out above it)
    The second wave has another m (multiples of 0.5 up to 1.5 in size, as the first: about 11 away)."""
    rng = np.random.default_rng([31, FAMILIES.index(family)])
    blocks, far = [], []
    for b in range(2):
        m = rng.integers(-3, 4, size=64) * 0.5
        is_far = np.zeros(ROWS_WAVE, dtype=bool)
        if family == "stagnation":
            es = []
            for p in BIG_AT:
                for _ in range(6):
                    e = rng.choice([-1.0, 1.0], 64) * 2.0 ** -12 * (1.0 - rng.integers(1, 4, 64) * 2.0 ** -10)
                    e[p] = rng.choice([-1.0, 1.0])
                    es.append(e)
            es = np.asarray(es)
            pts = np.concatenate([m + es, m - es[rng.permutation(len(es))]])
        elif family == "same_sign":
            es = np.asarray([1.0 + rng.permutation(64) * 2.0 ** -12 for _ in range(31)])
            pts = np.concatenate([m + es, m - es[rng.permutation(len(es))]])
        elif family == "cancelling":
            e = rng.choice([-1.0, 1.0], 64)
            pts = m + e + rng.integers(-8, 9, size=(63, 64)) * 2.0 ** -13
        else:
            near = rng.choice([-1.0, 1.0], size=(43, 64)) * 2.0 ** -3
            farp = rng.choice([-1.0, 1.0], size=(20, 64)) * 1250.0
            pts = np.concatenate([m + near, m + farp])
            is_far[1 + len(near):1 + len(near) + len(farp)] = True
        blocks.append(_block(m, pts))
        far.append(is_far)
    x = np.concatenate(blocks)
    assert np.array_equal(f32(x), x), "the construction does not fit float32"
    for b in range(2):
        e = x[64 * b:64 * b + 64] - x[64 * b]
        assert np.array_equal(f32(e), e)
    x.setflags(write=False)
    return dict(x=x, far=np.concatenate(far), near_hi=8.0 if family == "far_column" else None)


# ------------------------------------------------------------------------------------------------ hand-made slots for the selection
def ulps_above(base, i):
    """The float32 i ulps above the positive float32 `base`."""
    return (np.asarray(base, dtype=F32).view(np.int32) + np.asarray(i, dtype=np.int32)).view(F32)


def radix_passes(lo, hi):
    """The 8-bit passes idl_knn_select walks for a window: the bytes of the span of its order-preserving keys."""
    def key(f):
        b = int(np.asarray(f, dtype=F32).view(np.uint32))
        return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)
    span = key(hi) - key(lo)
    return max(1, (span.bit_length() + 7) // 8)


@functools.lru_cache(maxsize=None)
def hand_made_slots():
    """One launch of idl_knn_select over rows row0 .. of 300 real points, every row's slot written by hand so that one branch of the
    selection is reached: dict(x, row0, k, cap, names, intended [rows] status, passes [rows], lo, hi, delta, cnt_lo, cand_cnt [rows],
    cand_d2, cand_idx [rows, cap]).  k is the launch's; a row's rank among its kept values is k - cnt_lo.  Unless given, the kept
    indices are random columns: what the slot claims about them need not be true, the specification (select_spec) is a function of
    the slot.  (A negative rank inside the band cannot be reached from any slot: every kept value under v - delta is keyed under v,
    so fewer than k - cnt_lo of them exist.  Past the band is reached by a NaN, which is keyed as lo and belongs to no band.)"""
    rng = np.random.default_rng(77)
    n, k, cap, row0 = 300, 100, 1280, 5
    x = blobs(n, seed=11)
    tenths = (40.0 + 0.1 * np.arange(1, 10)).astype(F32)
    cases = []

    def add(name, status, vals, lo, hi, delta, want, idx=None, cand_cnt=None):
        vals = np.asarray(vals, dtype=F32)
        idx = rng.integers(0, n, len(vals)) if idx is None else np.asarray(idx)
        cases.append(dict(name=name, status=status, vals=vals, idx=idx, lo=F32(lo), hi=F32(hi), delta=F32(delta), cnt_lo=k - want,
                          cand_cnt=len(vals) if cand_cnt is None else cand_cnt))

    add("rank 0", 1, tenths, 40, 41, 1e-3, 0)
    add("rank count + 1", 1, tenths, 40, 41, 1e-3, 10)
    add("nothing kept", 1, [], 40, 41, 1e-3, 1)
    add("slot overflowed", 2, np.linspace(40.1, 40.9, cap), 40, 41, 1e-3, 5, cand_cnt=cap + 5)
    add("selected within delta of lo", 3, np.r_[F32(40.0005), tenths], 40, 41, 1e-3, 1)
    add("selected within delta of hi", 3, np.r_[tenths, F32(40.9995)], 40, 41, 1e-3, 10)
    add("rank past the band (NaN)", 3, [np.nan, np.nan, 40.5], 40, 41, 1e-3, 3)
    add("band of 1100", 4, np.full(1100, 40.5), 40, 41, 1e-3, 500)
    add("band of exactly 1024", 0, np.r_[np.linspace(40.1, 40.2, 30), np.full(1024, 40.5), np.linspace(40.8, 40.9, 20)], 40, 41, 1e-3, 430)
    below_lo = np.nextafter(F32(40), F32(0))
    add("one ulp below lo and at hi, 3 passes", 0, np.r_[below_lo, tenths[:8], F32(41)], 40, 41, 1e-3, 4)
    add("one ulp below lo and at hi, 4 passes", 0, np.r_[below_lo, tenths[:8], F32(4000)], 40, 4000, 1e-3, 4)
    add("one ulp below lo and at hi, 2 passes", 0, np.r_[below_lo, ulps_above(40, 1000 * np.arange(1, 9)), ulps_above(40, 50000)],
        40, ulps_above(40, 50000), 2.0 ** -16, 4)
    add("lo = -1e30", 0, tenths, NOTHING_BELOW, 42, 1e-3, 3)
    add("lo = hi", 3, [40, 40], 40, 40, 1e-3, 1)
    add("1 pass", 0, ulps_above(40, 20 * np.arange(1, 10)), 40, ulps_above(40, 200), 2.0 ** -16, 3)
    add("2 passes", 0, ulps_above(40, 1000 * np.arange(1, 41)), 40, ulps_above(40, 50000), 2.0 ** -16, 17)
    add("3 passes", 0, ulps_above(40, 20000 * np.arange(1, 41)), 40, ulps_above(40, 2 ** 20), 2.0 ** -16, 23)
    add("4 passes", 0, np.geomspace(2.0, 900.0, 30), 1, 1000, 1e-4, 11)
    shared = np.r_[np.linspace(40.01, 40.2, 20).astype(F32), ulps_above(40, 128000 + np.arange(300) % 250)]
    add("300 values in one bin of the last pass", 0, shared, 40, 41, 2.0 ** -20, 20 + 137)
    add("two equal values at the rank", 0, shared, 40, 41, 2.0 ** -20, 20 + 21)
    add("five equal values at the rank", 0, np.r_[F32(40.1), F32(40.2), np.full(5, 40.3), F32(40.6), F32(40.7)], 40, 41, 1e-3, 5)
    add("one kept value", 0, [40.5], 40, 41, 1e-3, 1)
    for _ in range(3):                                           # true slots: the definition's k-th must come out
        t = d2_to(x, row0 + len(cases), np.arange(n)).astype(F32)
        srt = np.sort(t)
        lo, hi = srt[79], srt[119]
        inside = np.nonzero((t >= lo) & (t < hi))[0]
        add("a true window", 0, t[inside], lo, hi, (hi - lo) / 100, k - int((t < lo).sum()), idx=inside)
    rows = len(cases)
    out = dict(x=x, row0=row0, k=k, cap=cap, names=[c["name"] for c in cases], intended=np.array([c["status"] for c in cases]),
               passes=np.array([radix_passes(c["lo"], c["hi"]) for c in cases]))
    for f, dt in (("lo", F32), ("hi", F32), ("delta", F32), ("cnt_lo", np.int32), ("cand_cnt", np.int32)):
        out[f] = np.array([c[f] for c in cases], dtype=dt)
    out["cand_d2"], out["cand_idx"] = np.zeros((rows, cap), dtype=F32), np.zeros((rows, cap), dtype=np.int32)
    for i, c in enumerate(cases):
        out["cand_d2"][i, :len(c["vals"])], out["cand_idx"][i, :len(c["vals"])] = c["vals"], c["idx"]
    return out


def hand_made_expected(h):
    """[(status, core or None)] of hand_made_slots() by select_spec."""
    return [select_spec(h["x"], h["row0"] + i, h["k"], h["lo"][i], h["hi"][i], h["delta"][i], h["cnt_lo"][i], h["cand_cnt"][i], h["cap"],
                        h["cand_d2"][i], h["cand_idx"][i]) for i in range(len(h["names"]))]
