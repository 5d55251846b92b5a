"""tests/nn_ref.py checked without a GPU: its distances are knn_ref.true_d2's bit for bit, equal distances go to the lowest index,
and self-exclusion gives a point's nearest OTHER point."""
import numpy as np

import knn_ref
import nn_ref


def test_nearest_is_true_d2_and_argmin():
    x = knn_ref.blobs(300, seed=5)
    d2 = knn_ref.true_d2(x)
    assert np.array_equal(nn_ref.sq_dists(x, x), d2), "nn_ref's distances are not knn_ref.true_d2's bit for bit"
    idx, val = nn_ref.nearest(x[:120], x)
    assert idx.dtype == np.int32 and val.dtype == np.float64
    assert np.array_equal(idx, d2[:120].argmin(1)) and np.array_equal(val, d2[:120].min(1))
    assert np.array_equal(idx, np.arange(120)) and not val.any()        # a row's own copy: distance exactly 0
    q = knn_ref.blobs(50, seed=6)
    idx, val = nn_ref.nearest(q, x)
    both = knn_ref.true_d2(np.concatenate([q, x]), rows=np.arange(50))[:, 50:]
    assert np.array_equal(idx, both.argmin(1)) and np.array_equal(val, both.min(1))


def test_ties_go_to_the_lowest_index():
    x = knn_ref.blobs(200, seed=7, noise=0)
    x[150:] = x[10:60]                                                   # rows 150 .. 199 are copies of rows 10 .. 59
    idx, val = nn_ref.nearest(x[150:], x)
    assert np.array_equal(idx, np.arange(10, 60)) and not val.any()
    idx, val = nn_ref.nearest(x[10:60], x[::-1])                         # reversed corpus: the copy now comes first
    assert np.array_equal(idx, np.arange(49, -1, -1)) and not val.any()


def test_self_exclusion():
    x = knn_ref.blobs(200, seed=8)
    x[199] = x[3]
    d2 = knn_ref.true_d2(x)
    np.fill_diagonal(d2, np.inf)
    idx, val = nn_ref.nearest(x, x, self0=0)
    assert (idx != np.arange(200)).all()
    assert np.array_equal(idx, d2.argmin(1)) and np.array_equal(val, d2.min(1))
    assert idx[3] == 199 and idx[199] == 3 and val[3] == 0.0 and val[199] == 0.0
    idx, val = nn_ref.nearest(x[40:90], x, self0=40)                     # a row range of the corpus as the query set
    assert np.array_equal(idx, d2[40:90].argmin(1)) and np.array_equal(val, d2[40:90].min(1))
