"""tests/umap_ref.py -- the float64 restatement the embedding kernels are held to (tests/test_gpu_embedding.py) -- pinned itself:
its kNN graph to sklearn's brute-force neighbours, its curve constants to the ones umap-learn prints, its union to symmetry bit for
bit, its full run to a quality the plot needs (trustworthiness above PCA's, pure neighbourhoods), and its epoch to mutations: an
epoch with one fired entry dropped, the attraction counted once, one entry's draws skipped, or the previous epoch's alpha must
move some vertex by more than the bar the GPU epoch is allowed (4 x the float32 replay's own deviation)."""
import functools

import numpy as np
import pytest

import umap_ref as R

EPOCH = 10                      # the epoch the mutations are applied to (its state comes from nine reference epochs)


@functools.lru_cache(maxsize=None)
def _small(name):
    if name == "blobs":
        return R.blobs(300, 4, 11)[0]
    x = R.blobs(200, 4, 12)[0]
    return np.concatenate([x, x[:100]])          # duplicates: ties, also across the k-th place


@pytest.mark.parametrize("name", ["blobs", "duplicates"])
def test_knn_graph_is_sklearns(name):
    from sklearn.neighbors import NearestNeighbors
    x = _small(name)
    idx16, dist16 = R.knn_graph(x, 16)            # (one more: whether the k-th place is tied with what follows it)
    idx, dist = idx16[:, :15], dist16[:, :15]
    i15, d15 = R.knn_graph(x[:40], 15)
    i16, d16 = R.knn_graph(x[:40], 16)
    assert np.array_equal(i15, i16[:, :15]) and np.array_equal(d15, d16[:, :15])       # a prefix of the longer list
    sd, si = NearestNeighbors(n_neighbors=15, algorithm="brute").fit(x.astype(np.float64)).kneighbors(x.astype(np.float64))
    scale = dist[:, -1:]
    # 1e-6 relative, element by element; the zeros (the point itself, its exact copies) come out of sklearn's Gram form as ~1e-7:
    # those alone are taken relative to the row's largest distance
    assert np.all(np.abs(dist - sd) <= 1e-6 * np.where(dist > 0, dist, scale))
    assert np.all(np.diff(dist, axis=1) >= 0)
    gap = np.diff(dist16, axis=1) > 1e-6 * scale
    clear = np.concatenate([gap[:, :1], gap[:, 1:] & gap[:, :-1]], 1)      # both neighbouring distances apart
    clear[:, 0] = False                           # (rank 0 is the point or one of its copies: distance 0 either way)
    assert clear.sum() > 0.5 * clear.size or name == "duplicates"
    assert np.array_equal(idx[clear], si[clear])
    ties = dist[:, 1:] == dist[:, :-1]
    assert np.all(idx[:, 1:][ties] > idx[:, :-1][ties])          # ties by ascending index
    assert np.all(idx[np.arange(len(x)), (idx == np.arange(len(x))[:, None]).argmax(1)] == np.arange(len(x)))   # itself included


def test_curve_constants_are_umap_learns():
    a, b = R.ab_params()
    assert abs(a - R.A_UMAP) < 1e-6 and abs(b - R.B_UMAP) < 1e-6


@pytest.mark.parametrize("name", ["blobs600", "doubled400"])
def test_union_is_symmetric_bit_for_bit(name):
    import scipy.sparse as sp
    x, _, idx, dist, (indptr, indices, p) = R.graph(name)
    n = len(x)
    m = sp.csr_matrix((p, indices, indptr), shape=(n, n))
    t = m.T.tocsr(); t.sort_indices()
    assert np.array_equal(t.indptr, m.indptr) and np.array_equal(t.indices, m.indices)
    assert np.array_equal(t.data.view(np.uint64), m.data.view(np.uint64))
    assert p.min() >= p.max() / 500.0 and not np.any(indices == np.repeat(np.arange(n), np.diff(indptr)))


def test_calibration_reaches_the_target():
    _, _, idx, dist, _ = R.graph("blobs600")
    rho, sigma, w = R.smooth_knn(idx[:50], dist[:50])
    psum = np.exp(-np.maximum(0.0, dist[:50, 1:] - rho[:, None]) / sigma[:, None]).sum(1)
    assert np.all(np.abs(psum - np.log2(15.0)) < 1e-12 * 15)
    assert np.all(w[:, 0] == 0.0) and np.all(w[:, 1] == 1.0)


def test_philox_known_answer():
    """Random123's known-answer vectors of Philox4x32-10."""
    assert [int(v) for v in R.philox(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in R.philox(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(v) for v in R.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("seed", R.SEEDS)
def test_full_run_quality(seed):
    from sklearn.manifold import trustworthiness
    x, lab, _, _, _ = R.graph("blobs600")
    y = R.embedding("blobs600", seed)
    assert np.all(np.isfinite(y)) and np.abs(y).max() < 20.0
    t, t_pca = trustworthiness(x, y, n_neighbors=15), trustworthiness(x, R.pca2(x), n_neighbors=15)
    print(f"seed {seed}: trustworthiness {t:.4f}, PCA-2 {t_pca:.4f}")
    assert t > t_pca
    assert R.purity(y, lab) == 1.0


def _epoch_case(seed):
    _, _, _, _, (indptr, indices, p) = R.graph("blobs600")
    a, b = R.ab_params()
    y0, eps, nxt, nneg = R.state_before("blobs600", seed, EPOCH)
    args = (y0, indptr, indices, eps, nxt, nneg, EPOCH, 500, a, b, seed)
    y64, _, _, info = R.epoch(*args)
    y32 = R.epoch(*args, dtype=np.float32)[0]
    bar = 4.0 * R.deviation(y32, y64, info, y0).max()
    return args, y64, info, bar


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("mutation", ["entry_dropped", "attraction_once", "draws_skipped", "previous_alpha"])
def test_mutations_exceed_the_epoch_bar(seed, mutation):
    args, y64, info, bar = _epoch_case(seed)
    assert 0.0 < bar < 1e-5
    fired, n_neg = info["fired"], info["n_neg"]
    kw = {"entry_dropped": dict(drop_entry=int(fired[len(fired) // 2])),
          "attraction_once": dict(attraction_count=1),
          "draws_skipped": dict(skip_draws_of=int(fired[n_neg > 0][len(fired) // 3])),
          "previous_alpha": dict(alpha_epoch=EPOCH - 1)}[mutation]
    y_mut = R.epoch(*args, **kw)[0]
    moved = R.deviation(y_mut, y64, info, args[0]).max()
    print(f"seed {seed}, {mutation}: moved {moved:.3e}, bar {bar:.3e}")
    assert moved > bar
