"""tests/ensemble_ref.py checked without a GPU: the vote-table form of the 'ensemble' assignment rule equals the dense squared distances
of posthoc.label_features' centred one-hot rows to the cluster means; re-assigning the votes of a converged sklearn KMeans returns its
labels; a missing vote, an empty cluster and a record on its centre behave as the rule says."""
import numpy as np
import pytest

import ensemble_ref as E

SHAPES = [(949, 3, 5, 5), (3000, 5, 20, 20)]          # (N, V, C, K)


@pytest.mark.parametrize("n,v,c,k", SHAPES + [(400, 4, 7, 3)])
def test_table_form_is_the_dense_form(n, v, c, k):
    rng = np.random.default_rng(n)
    votes = E.synthetic_votes(n, v, c, seed=n + 1, noise=0.3)
    y = rng.integers(0, k, n)
    p = rng.integers(-1, c, size=(v, 200))                        # new records, some votes missing
    counts, cnt = E.tables(votes, y, k, c)
    for q in (votes, p):
        got, want = E.sq_dists(q, counts, cnt), E.dense_sq_dists(q, votes, y, k, c)
        err = np.abs(got - want).max()
        print(f"(N, V, C, K) = {(n, v, c, k)}: largest |table form - dense form| = {err:.3g}")
        assert err <= 1e-12


@pytest.mark.parametrize("n,v,c,k", SHAPES)
def test_reassigning_a_converged_kmeans_returns_its_labels(n, v, c, k):
    from sklearn.cluster import KMeans
    votes = E.synthetic_votes(n, v, c, seed=11 * n)
    x = E.one_hot(votes, c)
    centred = x - x.sum(axis=0) / n
    km = KMeans(n_clusters=k, init="k-means++", n_init=10, tol=0.0, random_state=0).fit(centred)     # tol = 0: Lloyd runs until no label moves
    y = km.labels_
    counts, cnt = E.tables(votes, y, k, c)
    label, conf, d2 = E.assign(votes, counts, cnt)
    print(f"(N, V, C, K) = {(n, v, c, k)}: records re-assigned elsewhere = {int((label != y).sum())}, smallest margin = {E.margin(d2).min():.3g}")
    assert np.array_equal(label, y)
    assert np.abs(np.sqrt(d2) - km.transform(centred)).max() <= 1e-9
    assert ((conf > 0) & (conf <= 1)).all()


def test_a_missing_vote_contributes_its_voters_squares():
    votes = E.synthetic_votes(300, 3, 4, seed=5)
    y = np.random.default_rng(6).integers(0, 4, 300)
    counts, cnt = E.tables(votes, y, 4)
    a = counts / cnt[:, None, None]
    p = votes[:, :50].copy()
    full = E.sq_dists(p, counts, cnt)
    p[1] = -1
    cut = E.sq_dists(p, counts, cnt)
    voted = votes[1, :50]
    want = full - (1.0 - 2.0 * a[:, 1, :].T[voted])                # voter 1's term leaves; sum_c a[k, 1, c]^2 stays in the first sum
    assert np.abs(cut - want).max() <= 1e-12
    none = E.sq_dists(np.full((3, 1), -1), counts, cnt)[0]
    assert np.abs(none - (a * a).sum(axis=(1, 2))).max() <= 1e-15


def test_an_empty_cluster_is_never_chosen():
    votes = E.synthetic_votes(500, 3, 6, seed=8)
    y = np.random.default_rng(9).integers(0, 5, 500)
    y[y == 2] = 4                                                   # cluster 2 of 0 .. 5 has no record; 5 never had one
    counts, cnt = E.tables(votes, y, 6)
    assert cnt[2] == 0 and cnt[5] == 0
    p = np.random.default_rng(10).integers(-1, 6, size=(3, 400))
    label, conf, d2 = E.assign(p, counts, cnt)
    assert np.isinf(d2[:, [2, 5]]).all() and not np.isin(label, [2, 5]).any()
    assert np.isfinite(conf).all() and np.abs(E.dense_sq_dists(p, votes, y, 6)[:, [0, 1, 3, 4]] - d2[:, [0, 1, 3, 4]]).max() <= 1e-12


def test_confidence_is_one_on_a_centre():
    votes = np.array([[0, 0, 0, 1, 1, 2], [1, 1, 1, 0, 0, 2]])     # cluster 0: three identical records; cluster 1: two; cluster 2: one
    y = np.array([0, 0, 0, 1, 1, 2])
    counts, cnt = E.tables(votes, y, 3)
    label, conf, d2 = E.assign(votes, counts, cnt)
    assert np.array_equal(label, y)
    assert (d2[np.arange(6), y] == 0.0).all() and (conf == 1.0).all()
    label, conf, d2 = E.assign(np.array([[0], [0]]), counts, cnt)   # between the centres: a proper confidence
    assert 0.0 < conf[0] < 1.0 and abs(conf[0] - (1.0 / d2[0]).max() / (1.0 / d2[0]).sum()) <= 1e-15
    tie = E.assign(np.array([[-1], [-1]]), counts, cnt)             # no vote at all: every centre equally far -> the lowest k
    assert tie[0][0] == 0
