"""A float64 numpy restatement of the embedding behind --plot (idelucs_amd/csrc/embed.hip, posthoc.umap_embedding_device;
DESIGN.md section 7): the exact kNN graph, UMAP's calibration with 64 fixed bisection rounds, the fuzzy union, Philox4x32-10, one
Jacobi epoch of optimize_layout_euclidean, a full run, and a float32 replay of the epoch (the same formulae on float32 arrays).
tests/test_umap_reference.py pins this file to sklearn / scipy and to its own mutations; tests/test_gpu_embedding.py holds the
kernels to it.  Nothing here imports the package."""
import functools

import numpy as np

A_UMAP, B_UMAP = 1.5769434603, 0.8950608779       # the constants umap-learn prints for min_dist = 0.1, spread = 1
SEEDS = (42, 1, 2, 3, 4)


# ---------------------------------------------------------------- inputs
def blobs(n, n_blobs, rng_seed, d=64, spread=1.0, offset=0.0):
    """n points in d dimensions around n_blobs centres N(0, 1) per coordinate, labels uniform -> (float32 points, labels)."""
    rng = np.random.default_rng(rng_seed)
    centres = rng.normal(size=(n_blobs, d))
    labels = rng.integers(0, n_blobs, size=n)
    x = centres[labels] + spread * rng.normal(size=(n, d)) + offset
    return x.astype(np.float32), labels


def blobs600():
    """The issue's input: 600 points, 8 blobs, numpy.random.default_rng(3)."""
    return blobs(600, 8, 3)


def doubled400():
    """400 points of the same eight blobs (the same generator), each twice."""
    x, lab = blobs(400, 8, 3)
    return np.concatenate([x, x]), np.concatenate([lab, lab])


# ---------------------------------------------------------------- section 1: the exact kNN graph
def knn_graph(x, k):
    """(idx int32 [N, k], dist float64 [N, k]) of the points rounded to float32: per row the k nearest INCLUDING the point itself, by
    (distance, index); distances by the sequential coordinate loop t = a - b; d += t * t in float64, then sqrt."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, dim = x.shape
    idx = np.empty((n, k), dtype=np.int32)
    dist = np.empty((n, k), dtype=np.float64)
    cols = np.arange(n)
    for i in range(n):
        acc = np.zeros(n)
        for c in range(dim):
            t = x[i, c] - x[:, c]
            acc += t * t
        dv = np.sqrt(acc)
        order = np.lexsort((cols, dv))[:k]
        idx[i], dist[i] = order, dv[order]
    return idx, dist


# ---------------------------------------------------------------- section 2: calibration, union, curve
def smooth_knn(idx, dist):
    """(rho, sigma, w): rho = smallest strictly positive distance of the row (0 if none); sigma by UMAP's bisection, ALWAYS 64 rounds;
    the floor; w_ij = exp(-max(0, d_ij - rho_i) / sigma_i), 0 for j = i."""
    n, k = dist.shape
    target = np.log2(float(k))
    rho = np.zeros(n)
    sigma = np.zeros(n)
    mean_all = dist.mean()
    for i in range(n):
        d = dist[i]
        pos = d[d > 0.0]
        r = pos.min() if len(pos) else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            psum = 0.0
            for j in range(1, k):
                psum += np.exp(-max(0.0, d[j] - r) / mid)
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        floor = 1e-3 * (d.mean() if r > 0.0 else mean_all)
        rho[i], sigma[i] = r, max(mid, floor)
    w = np.exp(-np.maximum(0.0, dist - rho[:, None]) / sigma[:, None])
    w[idx == np.arange(n)[:, None]] = 0.0
    return rho, sigma, w


def fuzzy_union(idx, w, n_epochs):
    """P = A + A^T - A o A^T pruned below max(P) / n_epochs -> (indptr int64, indices int32, P float64), CSR with sorted columns and
    both directions of every edge."""
    import scipy.sparse as sp
    n, k = w.shape
    a = sp.csr_matrix((w.reshape(-1), (np.repeat(np.arange(n), k), idx.reshape(-1).astype(np.int64))), shape=(n, n))
    a.eliminate_zeros()
    t = a.T.tocsr()
    p = (a + t - a.multiply(t)).tocsr()
    p.data[p.data < p.data.max() / float(n_epochs)] = 0.0
    p.eliminate_zeros()
    p.sort_indices()
    return p.indptr.astype(np.int64), p.indices.astype(np.int32), p.data.astype(np.float64)


def ab_params(min_dist=0.1, spread=1.0):
    from scipy.optimize import curve_fit
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    params, _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(params[0]), float(params[1])


# ---------------------------------------------------------------- Philox4x32-10 (csrc/philox_device.h)
def philox(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays of output words for arrays (or scalars) of counter words and a scalar key."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0 & m32, p1 & m32, n2 & m32, p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def draws(seed, entries, epoch, n_draws, n):
    """[len(entries), n_draws] drawn vertices: draw p is word p % 4 of the group p / 4 of counter (entry low, entry high, epoch, group),
    key (seed low, seed high); the vertex is (word * n) >> 32."""
    entries = np.asarray(entries, dtype=np.uint64)
    out = np.empty((len(entries), n_draws), dtype=np.int64)
    for g in range((n_draws + 3) // 4):
        words = philox(entries, entries >> np.uint64(32), epoch, g, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        for wd in range(4):
            if 4 * g + wd < n_draws:
                out[:, 4 * g + wd] = (words[wd].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)
    return out


def jitter(n, seed, scale=1e-4):
    """float32 [n, 2]: scale * (2 u - 1), u = (word >> 8) * 2^-24 of counter (vertex low, vertex high, 0, 0xffffffff)."""
    v = np.arange(n, dtype=np.uint64)
    words = philox(v, v >> np.uint64(32), 0, 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = np.stack([(words[c] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) for c in (0, 1)], 1)
    return np.float32(scale) * (np.float32(2.0) * u - np.float32(1.0))


# ---------------------------------------------------------------- section 3: the layout
def pca_start(x, seed):
    """First two principal components (float64 covariance, eigh, each component's largest-magnitude entry positive), largest
    |coordinate| 10, float32, plus the jitter."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    xc = x - x.mean(0)
    evals, evecs = np.linalg.eigh(xc.T @ xc / max(len(x) - 1, 1))
    v = evecs[:, [-1, -2]]
    top = v[np.abs(v).argmax(0), np.arange(2)]
    v = v * np.where(top < 0, -1.0, 1.0)[None, :]
    y = xc @ v
    y = (y * (10.0 / np.abs(y).max())).astype(np.float32)
    return y + jitter(len(x), seed)


def schedule_start(p):
    """(eps, next, next_neg) float64 per directed entry: eps = max(P) / P_e, next = eps, next_neg = eps / 5."""
    eps = p.max() / p
    return eps, eps.copy(), eps / 5.0


def _scatter(acc, rows, vals):
    """acc[rows] += vals, in acc's own precision (float32: one addition after the other, as written)."""
    if acc.dtype == np.float64:
        for c in (0, 1):
            acc[:, c] += np.bincount(rows, vals[:, c], minlength=len(acc))
    else:
        np.add.at(acc, rows, vals)


def epoch(y, indptr, indices, eps, nxt, nneg, ep, n_epochs, a, b, seed, dtype=np.float64,
          drop_entry=None, attraction_count=2, skip_draws_of=None, alpha_epoch=None):
    """One Jacobi sweep, epoch number `ep` (1 ..), in `dtype` (float64: the reference; float32: the replay of the kernel's arithmetic).
    -> (new positions [N, 2] in dtype, next, next_neg, info) with info = {"terms": sum of |terms| per vertex and coordinate, "fired":
    entries that fired, "n_neg": their draw counts, "drawn": [fired, max n_neg] drawn vertices (-1 beyond an entry's count)}.
    The keyword arguments are the mutations of tests/test_umap_reference.py: one fired entry dropped, the attraction counted
    attraction_count times, the draws of one entry skipped, alpha taken from another epoch."""
    f = dtype
    y = np.asarray(y).astype(f)
    n = len(y)
    a_, b_ = f(a), f(b)
    owner = np.repeat(np.arange(n), np.diff(indptr))
    fired = np.nonzero(nxt <= float(ep))[0]
    esn = eps[fired] / 5.0
    n_neg = np.floor((float(ep) - nneg[fired]) / esn).astype(np.int64)
    nxt2, nneg2 = nxt.copy(), nneg.copy()
    nxt2[fired] = nxt[fired] + eps[fired]
    nneg2[fired] = nneg[fired] + n_neg.astype(np.float64) * esn
    acc = np.zeros((n, 2), dtype=f)
    terms = np.zeros((n, 2), dtype=f)
    live = np.ones(len(fired), dtype=bool)
    if drop_entry is not None:
        live &= fired != drop_entry
    # attraction
    j, kk = owner[fired], indices[fired]
    diff = y[j] - y[kk]
    d2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        pb = np.power(d2, b_)
        c = (f(-2.0) * a_ * b_ * (pb / d2)) / (a_ * pb + f(1.0))
    c = np.where(d2 > 0, c, f(0.0)).astype(f)
    g = (f(attraction_count) * np.clip(c[:, None] * diff, f(-4.0), f(4.0))).astype(f)
    _scatter(acc, j[live], g[live])
    _scatter(terms, j[live], np.abs(g[live]))
    # repulsion
    m = int(n_neg.max()) if len(fired) else 0
    drawn = np.full((len(fired), max(m, 0)), -1, dtype=np.int64)
    if m > 0:
        dv = draws(seed, fired, ep, m, n)
        for p_ in range(m):
            use = live & (n_neg > p_)
            drawn[n_neg > p_, p_] = dv[n_neg > p_, p_]
            if skip_draws_of is not None:
                use &= fired != skip_draws_of
            s = dv[:, p_]
            use &= s != j
            diff = y[j] - y[s]
            d2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                pb = np.power(d2, b_)
                c = (f(2.0) * b_) / ((f(0.001) + d2) * (a_ * pb + f(1.0)))
            g = np.where((d2 > 0)[:, None], np.clip(c[:, None] * diff, f(-4.0), f(4.0)), f(4.0)).astype(f)
            _scatter(acc, j[use], g[use])
            _scatter(terms, j[use], np.abs(g[use]))
    alpha = f(1.0 - ((ep if alpha_epoch is None else alpha_epoch) - 1) / float(n_epochs))
    out = (y + alpha * acc).astype(f)
    return out, nxt2, nneg2, {"terms": terms.astype(np.float64), "fired": fired, "n_neg": n_neg, "drawn": drawn}


def run(y0, indptr, indices, p, n_epochs, a, b, seed, last_epoch=None, dtype=np.float64):
    """Epochs 1 .. last_epoch (default n_epochs) from y0 -> (positions, (eps, next, next_neg))."""
    eps, nxt, nneg = schedule_start(p)
    y = np.asarray(y0).astype(dtype)
    for ep in range(1, (n_epochs if last_epoch is None else last_epoch) + 1):
        y, nxt, nneg, _ = epoch(y, indptr, indices, eps, nxt, nneg, ep, n_epochs, a, b, seed, dtype=dtype)
    return y, (eps, nxt, nneg)


def deviation(y_test, y_ref, info, y_before):
    """Per vertex: |y_test - y_ref| relative to sum |terms| + |y|, the larger of the two coordinates -> float64 [N]."""
    scale = info["terms"] + np.abs(np.asarray(y_before, dtype=np.float64))
    return (np.abs(np.asarray(y_test, dtype=np.float64) - np.asarray(y_ref, dtype=np.float64)) / scale).max(1)


# ---------------------------------------------------------------- shared, computed once
@functools.lru_cache(maxsize=None)
def graph(name, k=15, n_epochs=500):
    """(x, labels, idx, dist, (indptr, indices, P)) of a named input: "blobs600" | "doubled400"."""
    x, lab = {"blobs600": blobs600, "doubled400": doubled400}[name]()
    idx, dist = knn_graph(x, k)
    _, _, w = smooth_knn(idx, dist)
    return x, lab, idx, dist, fuzzy_union(idx, w, n_epochs)


@functools.lru_cache(maxsize=None)
def embedding(name, seed, n_epochs=500):
    """The float64 reference's full run on a named input."""
    x, _, _, _, (indptr, indices, p) = graph(name, n_epochs=n_epochs)
    a, b = ab_params()
    return run(pca_start(x, seed), indptr, indices, p, n_epochs, a, b, seed)[0]


@functools.lru_cache(maxsize=None)
def state_before(name, seed, ep, n_epochs=500):
    """(positions float32, eps, next, next_neg) the float64 reference holds at the start of epoch `ep` (positions rounded to float32:
    what a kernel can be fed)."""
    x, _, _, _, (indptr, indices, p) = graph(name, n_epochs=n_epochs)
    a, b = ab_params()
    y, (eps, nxt, nneg) = run(pca_start(x, seed), indptr, indices, p, n_epochs, a, b, seed, last_epoch=ep - 1)
    return y.astype(np.float32), eps, nxt, nneg


def pca2(x):
    x = np.asarray(x, dtype=np.float64)
    xc = x - x.mean(0)
    _, evecs = np.linalg.eigh(xc.T @ xc)
    return xc @ evecs[:, [-1, -2]]


def purity(y, labels, k=15):
    """Share of the k nearest neighbours in the plane (the point excluded) that carry the point's label, mean over the points."""
    from sklearn.neighbors import NearestNeighbors
    nb = NearestNeighbors(n_neighbors=k + 1).fit(y).kneighbors(y, return_distance=False)[:, 1:]
    return float((labels[nb] == labels[:, None]).mean())
