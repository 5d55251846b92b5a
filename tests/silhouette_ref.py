"""float64 reference, a-priori rounding bound and test inputs for the silhouette paths of idelucs_amd.posthoc (idl_silhouette_sums in
csrc/knn.hip through _silhouette_one_pass, and the GEMM form).  Plain numpy / scipy / sklearn: nothing here imports the package
under test.  Used by tests/test_silhouette_bound.py (a float32 numpy replay of the kernel's arithmetic, no GPU) and
tests/test_gpu_silhouette.py (the kernel itself); both go through check_within.

THE BOUND.  u = 2^-24 (fp32 unit roundoff).  A row i of a wave centred on the point c and a column j; a = x_i - c, b = x_j - c,
A = |a|^2, B = |b|^2, d = |x_i - x_j|.  The kernel computes d2 = (sqa + sqc) - 2 acc, clamps at 0, takes v_sqrt_f32 and adds up.
Its error in d2 is at most E = gamma u (A + B), gamma from the operation count:

    4    the coordinate subtractions x - c: every coordinate of a and of b carries a relative error u, so the difference vector
         a - b is off by at most u (|a| + |b|) in length, and its square by 2 d u (|a| + |b|) <= 2 u (|a| + |b|)^2 <= 4 u (A + B)
   18    the two squared norms: per lane a chain of 16 fma (one rounding each, the products are exact inside an fma), then the two
         shuffle adds: 18 roundings of sums of non-negative terms, so |sqa - A| <= 18 u A and |sqc - B| <= 18 u B
   64    the 64-term dot product on the matrix cores (16 v_mfma_f32_16x16x4f32 steps of 4 terms), at most 64 roundings whatever
         the order inside the instruction: |acc - a.b| <= 64 u sum |a_k b_k| <= 64 u |a| |b|, twice that <= 64 u (A + B)
    3    the final combine: sqa + sqc is one rounding of a value A + B; 2 acc is exact; the subtraction is one rounding of a
         value that is d^2 <= 2 (A + B) up to the errors above
   --
   89    first order in u; GAMMA_KERNEL = 90 takes in the second-order terms (89^2 u = 5e-4 of the total; 90 / 89 = 1.011).

From d2 to d: |sqrt(d^2 + e) - d| <= min(sqrt(|e|), |e| / d), and v_sqrt_f32 is accurate to 1 ulp = 2 u relative, so
|delta d| <= min(sqrt(E), E / d) + 2 u d; the row's own diagonal is set to 0 exactly and the weight (0 or 1) multiplies exactly.
S[i, c] adds the cluster's columns in one fp32 register per column lane, one add per 16-column tile, then four shuffle adds:
(tiles_of_c + 4) u S[i, c] on top of the sum of the columns' bounds.

The GEMM form (posthoc._silhouette_gemm_blocks) centres on the global mean; its squared norms are a rounded product and a D-term
sum each (D + 1 roundings), its dot product D roundings, and -2 x.y + |x|^2 + |y|^2 two roundings of values <= 2 (A + B):
gamma = 4 + (D + 1) + D + 4 = 2 D + 9 (137 for the 64 coordinates of the latent).  The accumulation term is kept as above.
"""
import functools

import numpy as np

U = 2.0 ** -24
GAMMA_KERNEL = 90.0
REF_SLACK = 1e-9          # sklearn's own silhouette_samples takes float64 Gram-form distances: 1e-16 of the squared norms (<= 6e6 here) over the distance


def gamma_gemm(d):
    return 2.0 * d + 9.0


def _dist(a, b):
    """float64 distances [len(a), len(b)], each from the difference vector (scipy's C loop: s += (u_k - v_k)^2, sqrt)."""
    from scipy.spatial.distance import cdist
    return cdist(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64), metric="euclidean")


def kernel_centres(n):
    """centre_of_row for idl_silhouette_sums: the first row of the row's 64-row wave.  (The tail waves of the last workgroup centre
    on row n - 1; they hold no row.)"""
    return (np.arange(n) // 64) * 64


def _core(x, w, col_cluster, K, centre_xyz, centre_sel, gamma, acc_len, rows=None, want_dmin=False, block=512):
    """(S, bound, dmin) [len(rows), K] for the rows `rows` (default all): the float64 sums, their allowed error, and (want_dmin) the
    smallest distance that went into each sum.  centre_xyz [m, D]: the centres; centre_sel [len(rows)]: which of them each of `rows` uses;
    acc_len [K]: roundings of the running sum of each cluster."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n = len(x)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    onehot = np.zeros((n, K))
    onehot[np.arange(n), col_cluster] = w
    b2_all = _dist(centre_xyz, x) ** 2                              # [m, n] |x_j - c|^2
    S = np.empty((len(rows), K)); bound = np.empty((len(rows), K))
    dmin = np.full((len(rows), K), np.inf) if want_dmin else None
    members = [np.nonzero((col_cluster == c) & (w > 0))[0] for c in range(K)] if want_dmin else None
    for lo in range(0, len(rows), block):
        r = rows[lo:lo + block]
        k = np.arange(len(r))
        d = _dist(x[r], x)
        d[k, r] = 0.0
        ci = centre_sel[lo:lo + block]
        A = b2_all[ci, r]
        E = gamma * U * (A[:, None] + b2_all[ci])
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = np.where(d > 0.0, np.minimum(np.sqrt(E), E / d), np.sqrt(E))
        delta += 2.0 * U * d
        delta[k, r] = 0.0
        S[lo:lo + block] = d @ onehot
        bound[lo:lo + block] = delta @ onehot + acc_len[None, :] * U * S[lo:lo + block]
        if want_dmin:
            d[k, r] = np.inf
            for c in range(K):
                if len(members[c]):
                    dmin[lo:lo + block, c] = d[:, members[c]].min(1)
    return S, bound, dmin


def sums_ref_and_bound(x, w, tile_cluster, K, centre_of_row, rows=None, gamma=GAMMA_KERNEL, want_dmin=False):
    """ref_sums, sums_bound and the smallest single distance inside every sum, from one pass over the pairs."""
    tile_cluster = np.asarray(tile_cluster, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    centre_of_row = np.asarray(centre_of_row)
    uniq, inv = np.unique(centre_of_row if rows is None else centre_of_row[np.asarray(rows)], return_inverse=True)
    acc_len = np.bincount(tile_cluster, minlength=K).astype(np.float64) + 4.0          # ceil(rows_of_c / 16) + 4
    return _core(x, w, np.repeat(tile_cluster, 16), K, x[uniq], inv, gamma, acc_len, rows=rows, want_dmin=want_dmin)


def ref_sums(x, w, tile_cluster, K, rows=None):
    """S[i, c] = sum_j w[j] |x_i - x_j| over the rows j of cluster c (tile_cluster[t]: the cluster of rows 16 t .. 16 t + 15)."""
    return sums_ref_and_bound(x, w, tile_cluster, K, kernel_centres(len(x)), rows=rows)[0]


def sums_bound(x, w, tile_cluster, K, centre_of_row, rows=None, gamma=GAMMA_KERNEL):
    """The error the kernel's arithmetic is allowed in S[i, c] (module docstring)."""
    return sums_ref_and_bound(x, w, tile_cluster, K, centre_of_row, rows=rows, gamma=gamma)[1]


def ref_samples(x, labels):
    from sklearn.metrics import silhouette_samples
    return silhouette_samples(np.asarray(x, dtype=np.float64), labels)


def layout(x, lab, K, pad=64, order=None, last_pad=None, fill="copy", rng=None):
    """The points cluster by cluster as idl_silhouette_sums takes them: the clusters in `order` (default: ascending id, what
    posthoc._silhouette_one_pass does, with pad = 64), the points of a cluster in their given order (a stable sort), every cluster
    padded to a multiple of `pad` rows (the last one of `last_pad`) of weight 0.  fill "copy": the padding repeats the cluster's
    first point; "far": unrelated points around 1e3.  lab: ids 0 .. K - 1 (an id may be unused: it gets no tile).
    -> dict(x [npad, D] float64, w [npad], tile_cluster [npad / 16] int32, pos [n]: the row of every given point)."""
    x = np.asarray(x, dtype=np.float64)
    lab = np.asarray(lab)
    order = [c for c in range(K) if (lab == c).any()] if order is None else list(order)
    xs, ws, tc, pos = [], [], [], np.empty(len(x), dtype=np.int64)
    at = 0
    for k, c in enumerate(order):
        idx = np.nonzero(lab == c)[0]
        p = last_pad if (last_pad is not None and k == len(order) - 1) else pad
        rows = -(-len(idx) // p) * p
        blk = np.repeat(x[idx[:1]], rows, axis=0)
        if fill == "far":
            blk = (1.0e3 + 10.0 * rng.standard_normal(blk.shape)).astype(np.float32).astype(np.float64)
        blk[:len(idx)] = x[idx]
        wk = np.zeros(rows); wk[:len(idx)] = 1.0
        pos[idx] = at + np.arange(len(idx))
        xs.append(blk); ws.append(wk); tc += [c] * (rows // 16)
        at += rows
    return dict(x=np.concatenate(xs), w=np.concatenate(ws), tile_cluster=np.asarray(tc, dtype=np.int32), pos=pos, K=K)


def samples_from_sums(S, own, counts):
    """silhouette of every point from its per-cluster sums (float64): (b - a) / max(a, b), 0 for a singleton."""
    n_own = counts[own]
    k = np.arange(len(own))
    a = S[k, own] / np.maximum(n_own - 1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(counts[None, :] > 0, S / counts[None, :], np.inf)
    means[k, own] = np.inf
    b = means.min(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (b - a) / np.maximum(a, b)
    return np.where(n_own > 1.0, np.nan_to_num(s), 0.0)


def propagate(S, bound, own, counts):
    """The error of s = (b - a) / max(a, b) allowed by `bound` on the sums.  a = S_own / (n_own - 1) moves by da = bound_own /
    (n_own - 1).  b = min_c m_c, m_c = S_c / n_c with its own bound e_c = bound_c / n_c: min is 1-Lipschitz, so whichever cluster
    attains the computed minimum, it lies between min_c (m_c - e_c) and m_c* + e_c* (c* the true nearest cluster) -- b moves by at
    most db = max(e_c*, b - min_c (m_c - e_c)), which a far cluster's large e_c does not enter.  Both partial derivatives of s are at most 1 / max(a, b) in size, and on the segment between the true and
    the computed (a, b) that maximum is at least max(a, b) - max(da, db): |ds| <= (da + db) / (max(a, b) - max(da, db)), and never
    more than 2, the width of [-1, 1].  Singletons score an exact 0 on both sides."""
    n_own = counts[own]
    k = np.arange(len(own))
    a = S[k, own] / np.maximum(n_own - 1.0, 1.0)
    da = bound[k, own] / np.maximum(n_own - 1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(counts[None, :] > 0, S / counts[None, :], np.inf)
        dmeans = np.where(counts[None, :] > 0, bound / counts[None, :], 0.0)
    means[k, own] = np.inf
    dmeans[k, own] = 0.0
    b, near = means.min(1), means.argmin(1)
    db = np.maximum(dmeans[k, near], b - (means - dmeans).min(1))
    room = np.maximum(a, b) - np.maximum(da, db)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(room > 0.0, (da + db) / room, 2.0)
    return np.where(n_own > 1.0, np.minimum(ds, 2.0) + REF_SLACK, 0.0)


def samples_bound(x, labels, path="kernel"):
    """The error allowed in every point's silhouette (the caller's point order) on the path the library takes: "kernel"
    (posthoc._silhouette_one_pass: clusters in ascending label order, padded to whole 64-row waves with copies of their first point,
    every wave centred on its first row) or "gemm" (centred on the global mean)."""
    x = np.asarray(x, dtype=np.float64)
    uniq, lab = np.unique(np.asarray(labels), return_inverse=True)
    K = len(uniq)
    counts = np.bincount(lab, minlength=K).astype(np.float64)
    if path == "kernel":
        lay = layout(x, lab, K, pad=64)
        S, bound, _ = sums_ref_and_bound(lay["x"], lay["w"], lay["tile_cluster"], K, kernel_centres(len(lay["x"])), rows=lay["pos"])
    else:
        acc_len = np.ceil(counts / 16.0) + 4.0
        S, bound, _ = _core(x, np.ones(len(x)), lab, K, x.mean(0, keepdims=True), np.zeros(len(x), dtype=np.int64), gamma_gemm(x.shape[1]), acc_len)
    return propagate(S, bound, lab, counts)


def check_within(got, want, bound, what):
    """THE assertion of both test modules: every element of `got` within `bound` of `want`.  Prints and returns (largest error
    over its bound, largest error)."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err > 0.0, np.inf, 0.0))
    bad = ~(err <= bound)
    worst = float(np.nanmax(ratio)) if not np.isnan(err).all() else float("nan")
    print(f"{what}: largest error / bound {worst:.3g}, largest error {float(np.nanmax(err)):.3g} (bound there {float(bound.flat[np.nanargmax(err)]):.3g})")
    if bad.any():
        at = np.argwhere(bad)[:5]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside their bound; first at {at.tolist()}: got "
                             f"{[float(got[tuple(i)]) for i in at]}, want {[float(want[tuple(i)]) for i in at]}, bound {[float(bound[tuple(i)]) for i in at]}")
    return worst, float(err.max())


# ------------------------------------------------------------------------------------------------ inputs
def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)          # what the device holds exactly


def _sizes(n, k, small=8):
    """k unequal cluster sizes adding up to n, the smallest `small`: few enough points that ONE un-zeroed diagonal entry (the Gram
    form leaves about 1e-3 of the row's distance to its centre there) is several times the bound of the row's own sum, which
    grows with the number of columns in it (tests/test_silhouette_bound.py, the "keep_diagonal" mistake)."""
    share = np.arange(2, k + 1, dtype=np.float64)
    s = np.floor((n - small) * share / share.sum()).astype(int)
    s[-1] += n - small - s.sum()
    return [small] + s.tolist()


def _blobs(rng, sizes, scale, spread, d=64):
    lab = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    centres = rng.standard_normal((len(sizes), d)) * scale
    return centres, lab, centres[lab] + rng.standard_normal((len(lab), d)) * spread


SAMPLE_CASES = ("blobs", "tight", "offset", "copies", "k2", "singletons", "sizes_63_64_65", "cut", "halo")
BENIGN = ("blobs", "tight", "offset", "k2", "singletons", "sizes_63_64_65", "cut")      # no zero distances, no wide cluster


@functools.lru_cache(maxsize=None)
def sample_case(name, n=3000, d=64):
    """(x [n, d] float64 holding float32 values, labels [n]) of one regime."""
    rng = np.random.default_rng([17, SAMPLE_CASES.index(name), n, d])
    if name in ("blobs", "offset"):
        _, lab, x = _blobs(rng, _sizes(n, 6), 2.0, 1.0, d)
        x = x + (300.0 if name == "offset" else 0.0)
    elif name == "tight":
        _, lab, x = _blobs(rng, _sizes(n, 6), 40.0, 0.02, d)
    elif name == "copies":                                        # the second half repeats the first, every tenth copy under another label
        _, lab, x = _blobs(rng, _sizes(n // 2, 6), 2.0, 1.0, d)
        lab2 = lab.copy()
        lab2[::10] = (lab2[::10] + 1) % 6
        x, lab = np.concatenate([x, x]), np.concatenate([lab, lab2])
    elif name == "k2":
        _, lab, x = _blobs(rng, [8, n - 8], 2.0, 1.0, d)
    elif name == "singletons":
        _, lab, x = _blobs(rng, _sizes(n, 6), 2.0, 1.0, d)
        lab[[3, 500, 501, 1777, n - 1]] = [9, 11, 12, 20, 21]
    elif name == "sizes_63_64_65":
        _, lab, x = _blobs(rng, [63, 64, 65] + _sizes(n - 192, 3), 2.0, 1.0, d)
    elif name == "cut":                                           # every tight blob under two labels
        _, blob, x = _blobs(rng, _sizes(n, 6, small=16), 40.0, 0.02, d)
        lab = 2 * blob + rng.integers(0, 2, n)
    elif name == "halo":                                          # a third of the points just outside their tight blob, labelled -1 together
        centres, lab, x = _blobs(rng, _sizes(n, 6), 40.0, 0.02, d)
        out = rng.random(n) < 1.0 / 3.0
        direction = rng.standard_normal((n, d))
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        x[out] = (centres[lab] + direction * rng.uniform(0.25, 0.5, (n, 1)))[out]
        lab = np.where(out, -1, lab)
    x, lab = _f32(x), np.asarray(lab, dtype=np.int64)
    x.setflags(write=False); lab.setflags(write=False)
    return x, lab


@functools.lru_cache(maxsize=None)
def sample_reference(name, n=3000, d=64, path="kernel"):
    """(sklearn's per-point values, their mean, the per-point bound) of sample_case(name, n, d), computed once."""
    x, lab = sample_case(name, n, d)
    want = ref_samples(x, lab)
    bound = samples_bound(x, lab, path)
    for a in (want, bound):
        a.setflags(write=False)
    return want, float(want.mean()), bound


STRADDLE_SIZES = (64, 65, 63, 17, 16, 15, 1, 33, 20)             # 23 tiles of 16 rows; rows 0, 64, ... 320 are points, not padding
STRADDLE_IDS = (0, 1, 2, 4, 5, 6, 7, 8, 9)                        # of 10 cluster ids: id 3 owns no tile


@functools.lru_cache(maxsize=None)
def direct_case(name):
    """A call of idl_silhouette_sums as the C ABI allows it: layout() dict."""
    rng = np.random.default_rng([23, ("straddle", "straddle_far", "straddle_dups", "one", "many", "long").index(name)])
    if name.startswith("straddle"):
        # n = 16 * 23, clusters padded to 16 rows only: two workgroups, the second partly used, an odd tile count, waves that straddle clusters
        rng = np.random.default_rng([23, 0])                      # the three variants share their points
        lab = np.repeat(STRADDLE_IDS, STRADDLE_SIZES)
        centres = rng.standard_normal((10, 64)) * 2.0
        x = _f32(centres[lab] + rng.standard_normal((len(lab), 64)))
        if name == "straddle_dups":                               # exact duplicates inside a cluster and across clusters
            first = np.concatenate([[0], np.cumsum(STRADDLE_SIZES)[:-1]])
            x[first[0] + 5] = x[first[0] + 3]
            x[first[1] + 64] = x[first[1] + 2]
            x[first[1] + 2 + 1] = x[first[0] + 7]
            x[first[7] + 1] = x[first[2] + 9]
            x[first[6]] = x[first[5] + 4]                         # the singleton is a copy of a point of another cluster
        lay = layout(x, lab, 10, pad=16, order=STRADDLE_IDS, fill="far" if name == "straddle_far" else "copy", rng=np.random.default_rng(5))
        assert len(lay["x"]) == 16 * 23 and (lay["w"][::64] == 1.0).all()
    elif name == "one":                                           # n = 16, one cluster
        lay = layout(_f32(rng.standard_normal((11, 64))), np.zeros(11, dtype=int), 1, pad=16)
    elif name == "many":                                          # 300 clusters of 3 .. 40 points
        sizes = 3 + np.floor(37.999 * rng.random(300) ** 3).astype(int)
        lab = np.repeat(np.arange(300), sizes)
        centres = rng.standard_normal((300, 64)) * 2.0
        lay = layout(_f32(centres[lab] + rng.standard_normal((len(lab), 64))), lab, 300, pad=16)
    elif name == "long":                                          # accumulation length: 6 250 tiles in one running sum
        lab = np.repeat([0, 1], [100000, 500])
        centres = rng.standard_normal((2, 64)) * 2.0
        lay = layout(_f32(centres[lab] + rng.standard_normal((len(lab), 64))), lab, 2, pad=16)
    for a in lay.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return lay
