"""float64 reference of the 'ensemble' assignment rule of idelucs_amd/ensemble.py (FittedEnsemble.assign, n_clusters > 0).  Plain
numpy: nothing here imports the package under test.  Used by tests/test_ensemble_reference.py (no GPU) and tests/test_gpu_assign.py.

THE RULE.  votes [V, N] in [0, C): the voters' relabelled votes on the training file; y [N] in [0, K): the run's final labels (k-means
on the centred one-hot vote rows, posthoc.label_features).  counts[k, v, c] = records with label k whose voter v voted c, cnt[k] =
records with label k, a = counts / cnt.  A new record with votes p [V] (-1: no vote) is at squared distance
    d2[k] = sum_{v, c} a[k, v, c]^2 + sum_{v: p_v >= 0} (1 - 2 a[k, v, p_v])
from cluster k's mean -- the squared Euclidean distance between its centred one-hot row and the mean of cluster k's centred rows; the
centring cancels.  cnt[k] == 0: +inf.  Label: argmin, lowest k on ties.  Confidence: (1 / d2)[k*] / sum_k (1 / d2)[k], 1.0 where
d2[k*] == 0."""
import numpy as np


def tables(votes, y, n_clusters, n_classes=None):
    votes, y = np.asarray(votes, dtype=np.int64), np.asarray(y, dtype=np.int64)
    n_classes = n_clusters if n_classes is None else n_classes
    counts = np.zeros((n_clusters, votes.shape[0], n_classes), dtype=np.int64)
    for k in range(n_clusters):
        for v in range(votes.shape[0]):
            counts[k, v] = np.bincount(votes[v][y == k], minlength=n_classes)
    return counts, np.bincount(y, minlength=n_clusters).astype(np.int64)


def sq_dists(p, counts, cnt):
    """[M, K] float64 by the table form; p [V, M]."""
    p = np.asarray(p, dtype=np.int64)
    cnt = np.asarray(cnt, dtype=np.float64)
    a = np.asarray(counts, dtype=np.float64) / np.maximum(cnt, 1.0)[:, None, None]
    d2 = np.tile((a * a).sum(axis=(1, 2))[None, :], (p.shape[1], 1))
    for v in range(p.shape[0]):
        valid = p[v] >= 0
        d2[valid] += 1.0 - 2.0 * a[:, v, :].T[p[v][valid]]
    d2 = np.maximum(d2, 0.0)
    d2[:, cnt == 0] = np.inf
    return d2


def one_hot(p, n_classes):
    """[M, V * C]: posthoc.label_features' rows before centring; a voter without a vote (-1) leaves its block zero."""
    p = np.asarray(p, dtype=np.int64)
    v, m = p.shape
    x = np.zeros((m, v * n_classes))
    for i in range(v):
        valid = p[i] >= 0
        x[np.nonzero(valid)[0], i * n_classes + p[i][valid]] = 1.0
    return x


def dense_sq_dists(p, votes, y, n_clusters, n_classes=None):
    """[M, K] float64 by the dense form: label_features' centred one-hot rows (centred with the TRAINING rows' mean) against the means of
    the training rows of every cluster.  An empty cluster: +inf."""
    n_classes = n_clusters if n_classes is None else n_classes
    train = one_hot(votes, n_classes)
    mu = train.sum(axis=0) / len(train)
    train = train - mu
    x = one_hot(p, n_classes) - mu
    y = np.asarray(y)
    out = np.full((len(x), n_clusters), np.inf)
    for k in range(n_clusters):
        if (y == k).any():
            c = train[y == k].mean(axis=0)
            out[:, k] = ((x - c) ** 2).sum(axis=1)
    return out


def assign(p, counts, cnt):
    """(label int64 [M], confidence float64 [M], d2 [M, K])."""
    d2 = sq_dists(p, counts, cnt)
    label = d2.argmin(axis=1)                       # the first minimum: the lowest k
    best = d2[np.arange(len(d2)), label]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / d2
        conf = np.where(best == 0.0, 1.0, (1.0 / best) / w.sum(axis=1))
    return label.astype(np.int64), conf, d2


def margin(d2):
    """Second-best minus best squared distance per record."""
    s = np.sort(d2, axis=1)
    return s[:, 1] - s[:, 0] if d2.shape[1] > 1 else np.full(len(d2), np.inf)


def synthetic_votes(n, n_voters, n_classes, seed, noise=0.15):
    """Votes with structure: a hidden class per record, every voter names it through its own permutation and errs with probability noise."""
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, n_classes, n)
    votes = np.empty((n_voters, n), dtype=np.int64)
    for v in range(n_voters):
        perm = rng.permutation(n_classes)
        wrong = rng.random(n) < noise
        votes[v] = np.where(wrong, rng.integers(0, n_classes, n), perm[truth])
    return votes
