"""float64 reference and specification of idl_nn_rows (csrc/nn_rows.hip): the exact nearest corpus row of every query.  Plain numpy:
nothing here imports the package under test.  Used by tests/test_nn_reference.py (the reference against knn_ref.true_d2, no GPU) and
tests/test_gpu_nn_rows.py (the kernel: indices equal, distances bit-equal).

THE CONTRACT.  q [m, 64], x [n, 64] hold float32 values.  D(i, j) = sum over c = 0 .. 63, ascending, of t * t with
t = (double)q[i, c] - (double)x[j, c]; the product and the sum are each rounded (no fused multiply-add).  self0 >= 0 leaves out
j == self0 + i.  The answer for i is the j that minimises (D(i, j), j) lexicographically, and that D."""
import numpy as np


def sq_dists(q, x, block=512):
    """[m, n] float64: D of the contract.  An explicit loop over the coordinates -- np.sum adds pairwise, which is another rounding."""
    q = np.asarray(q, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((len(q), len(x)))
    for b0 in range(0, len(q), block):
        qb = q[b0:b0 + block]
        acc = np.zeros((len(qb), len(x)))
        for c in range(q.shape[1]):
            t = qb[:, c][:, None] - x[:, c][None, :]
            acc += t * t
        out[b0:b0 + block] = acc
    return out


def nearest(q, x, self0=-1):
    """(idx int32 [m], d2 float64 [m]) of the contract.  np.argmin returns the first minimum: the lowest index among equal distances."""
    d = sq_dists(q, x)
    if self0 >= 0:
        assert len(x) >= 2
        i = np.arange(len(d))
        d[i, self0 + i] = np.inf
    idx = d.argmin(axis=1)
    return idx.astype(np.int32), d[np.arange(len(d)), idx]
