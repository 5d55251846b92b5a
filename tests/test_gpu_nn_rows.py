"""idl_nn_rows (csrc/nn_rows.hip) straight through the C ABI against tests/nn_ref.nearest -- float64 from the difference vector,
equal distances to the lowest index; tests/test_nn_reference.py checks that reference without a GPU.  For every case the indices
must be equal and the squared distances bit-equal, and both outputs are exactly m elements between two guards of sentinel values.

Shapes: more than one chunk of 64 corpus rows and less than one tile of 256 queries (70 x 1000); n = 1; m = 1; a ragged tile and a
ragged chunk (65 x 257, 300 x 257: two query tiles); exact duplicates; self-exclusion; coordinates around 300, where the float32 Gram
form cancels; and the first case again on a corpus long enough for the sliced path (idl_nn_rows_slices > 1), whose added rows are far
away: identical outputs."""
import ctypes

import numpy as np
import pytest

import knn_ref
import nn_ref

pytestmark = pytest.mark.gpu

GUARD = 1024
SENT_I, SENT_D = -77, -7.0


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _run(dev, q, x, self0=-1):
    """idl_nn_rows on float32 copies of q and x -> (idx, d2) as numpy arrays, the guards around both outputs checked."""
    import torch
    from idelucs_amd import _lib
    q = np.ascontiguousarray(q, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    m, n = len(q), len(x)
    qt, xt = torch.from_numpy(q).to(dev), torch.from_numpy(x).to(dev)
    idx = torch.full((m + 2 * GUARD,), SENT_I, dtype=torch.int32, device=dev)
    d2 = torch.full((m + 2 * GUARD,), SENT_D, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib.idl_nn_rows(ctypes.c_void_p(qt.data_ptr()), m, ctypes.c_void_p(xt.data_ptr()), n, 64, self0,
                                    ctypes.c_void_p(idx.data_ptr() + 4 * GUARD), ctypes.c_void_p(d2.data_ptr() + 8 * GUARD),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    for a, s, name in ((idx, SENT_I, "idx"), (d2, SENT_D, "d2")):
        assert (a[:GUARD] == s).all(), f"{name}: written in front of the buffer"
        assert (a[GUARD + m:] == s).all(), f"{name}: written behind the buffer"
    return idx[GUARD:GUARD + m].copy(), d2[GUARD:GUARD + m].copy()


def _check(dev, q, x, self0=-1, what=""):
    from idelucs_amd import _lib
    got_i, got_d = _run(dev, q, x, self0)
    want_i, want_d = nn_ref.nearest(q, x, self0)
    print(f"{what}: m = {len(q)}, n = {len(x)}, slices = {_lib.lib.idl_nn_rows_slices(len(q), len(x))}, "
          f"indices differing = {int((got_i != want_i).sum())}, distances differing = {int((got_d != want_d).sum())}")
    assert np.array_equal(got_i, want_i), f"{what}: a neighbour is not the reference's"
    assert np.array_equal(got_d.view(np.int64), want_d.view(np.int64)), f"{what}: a squared distance is not bit-equal to the reference's"
    return got_i, got_d


@pytest.fixture(scope="module")
def blobs():
    x = knn_ref.blobs(1000, seed=21)
    q = knn_ref.blobs(70, seed=22)
    x.setflags(write=False)
    q.setflags(write=False)
    return q, x


def test_blobs(dev, blobs):
    _check(dev, *blobs, what="blobs")


def test_one_corpus_row(dev, blobs):
    idx, _ = _check(dev, blobs[0], blobs[1][5:6], what="n = 1")
    assert not idx.any()


def test_one_query(dev, blobs):
    _check(dev, blobs[0][3:4], blobs[1], what="m = 1")


@pytest.mark.parametrize("m", [65, 300])
def test_ragged_tiles(dev, m):
    _check(dev, knn_ref.blobs(m, seed=23), knn_ref.blobs(257, seed=24), what="ragged")


def test_duplicates_and_copies(dev):
    x = knn_ref.blobs(500, seed=25, noise=0).copy()
    x[300:] = x[np.random.default_rng(3).integers(0, 40, 200)]          # exact duplicates, the first of each below row 40
    q = np.concatenate([x[450:], x[:30], x[200:230]])                    # queries that are copies of corpus rows
    idx, d2 = _check(dev, q, x, what="duplicates")
    assert not d2.any(), "a copy of a corpus row is not at distance exactly 0"
    assert (idx[:50] < 40).all() and np.array_equal(idx[50:80], np.arange(30)), "a duplicate did not go to its lowest index"


def test_self_exclusion(dev):
    x = knn_ref.blobs(400, seed=26).copy()
    x[399] = x[7]
    idx, d2 = _check(dev, x, x, self0=0, what="self0 = 0")
    assert (idx != np.arange(400)).all()
    assert idx[7] == 399 and idx[399] == 7 and d2[7] == 0.0 and d2[399] == 0.0
    _check(dev, x[100:170], x, self0=100, what="self0 = 100")


def test_offset_coordinates(dev):
    x = knn_ref.blobs(600, seed=27, offset=300.0)
    q = np.concatenate([knn_ref.blobs(40, seed=28, offset=300.0), x[100:130]])
    idx, d2 = _check(dev, q, x, what="offset 300")
    assert np.array_equal(idx[40:], np.arange(100, 130)) and not d2[40:].any()


def test_sliced_corpus_gives_the_same(dev, blobs):
    from idelucs_amd import _lib
    q, x = blobs
    far = knn_ref.blobs(4000, seed=29, offset=500.0)
    big = np.concatenate([x, far])
    assert _lib.lib.idl_nn_rows_slices(len(q), len(x)) == 1 and _lib.lib.idl_nn_rows_slices(len(q), len(big)) > 1
    one = _run(dev, q, x)
    cut = _check(dev, q, big, what="sliced")
    assert np.array_equal(one[0], cut[0]) and np.array_equal(one[1].view(np.int64), cut[1].view(np.int64))
    # neighbours in every slice: the corpus shuffled, so that the merge decides between slices; a duplicated row in two slices
    perm = np.random.default_rng(4).permutation(len(big))
    mixed = big[perm].copy()
    mixed[4900] = mixed[30]
    qq = np.concatenate([q, mixed[30:31]])
    idx, d2 = _check(dev, qq, mixed, what="sliced, shuffled")
    assert idx[-1] == 30 and d2[-1] == 0.0
    _check(dev, mixed[:300], mixed, self0=0, what="sliced, self0 = 0")
