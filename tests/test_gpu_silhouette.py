"""The silhouette on the GPU, element by element: idl_silhouette_sums (silhouette_sums_kernel, csrc/knn.hip) against float64 sums of
difference-vector distances, and posthoc.silhouette_samples_device against sklearn.metrics.silhouette_samples -- every sum and every
point inside the a-priori rounding bound of tests/silhouette_ref.py (derived from the kernel's operation count; checked against a
float32 replay and five planted mistakes in tests/test_silhouette_bound.py), where the score's mean over thousands of points hides
a wrong row, a wrong wave or a wrong flush.

1. Straight through the C ABI, at shapes posthoc._silhouette_one_pass never produces (it pads every cluster to 64 rows): n any
   multiple of 16, an odd tile count, waves that straddle clusters, a last workgroup with idle waves, one cluster, 300 clusters,
   a cluster id without tiles, padding that is not a copy of anything, exact duplicates, a running sum over 6 250 tiles.  Every
   call writes into a buffer with a sentinel-filled guard on both sides.
2. Through silhouette_samples_device, nine regimes on the one-pass path and the GEMM path's two entry conditions.

Every test prints, per regime, the largest error over its bound and the largest error (pytest -s); DESIGN.md section 7 keeps the table."""
import ctypes

import numpy as np
import pytest

import silhouette_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD_ROWS = 256              # a whole workgroup's rows on either side of the sums


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def kernel_sums(dev, lay):
    """idl_silhouette_sums on a layout() dict -> sums [n, K] (numpy float32); asserts that nothing outside them was written."""
    import torch
    from idelucs_amd import _lib
    n, K = len(lay["x"]), lay["K"]
    assert n % 16 == 0 and len(lay["tile_cluster"]) == n // 16 and 0 <= lay["tile_cluster"].min() and lay["tile_cluster"].max() < K
    x = torch.from_numpy(np.ascontiguousarray(lay["x"], dtype=np.float32)).to(dev)
    w = torch.from_numpy(np.ascontiguousarray(lay["w"], dtype=np.float32)).to(dev)
    tc = torch.from_numpy(np.ascontiguousarray(lay["tile_cluster"], dtype=np.int32)).to(dev)
    buf = torch.full(((n + 2 * GUARD_ROWS) * K,), SENTINEL, dtype=torch.float32, device=dev)
    vp = ctypes.c_void_p
    _lib.check(_lib.lib.idl_silhouette_sums(vp(x.data_ptr()), vp(w.data_ptr()), vp(tc.data_ptr()), n, 64, K,
                                            vp(buf.data_ptr() + 4 * GUARD_ROWS * K), vp(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize(dev)
    out = buf.cpu().numpy()
    assert (out[:GUARD_ROWS * K] == SENTINEL).all(), "written in front of the sums"
    assert (out[(GUARD_ROWS + n) * K:] == SENTINEL).all(), "written behind the sums (a tail wave of the last workgroup?)"
    return out[GUARD_ROWS * K:(GUARD_ROWS + n) * K].reshape(n, K)


def check_sums(got, lay, what, rows=None):
    """Every written element of `got` (the rows `rows`, default all) against the float64 sums within the bound; the columns of
    cluster ids without tiles still hold the sentinel."""
    n, K = len(lay["x"]), lay["K"]
    S, bound, _ = R.sums_ref_and_bound(lay["x"], lay["w"], lay["tile_cluster"], K, R.kernel_centres(n), rows=rows)
    cols = np.isin(np.arange(K), lay["tile_cluster"])
    got = got if rows is None else got[rows]
    assert (got[:, ~cols] == SENTINEL).all(), "a cluster id without tiles was written"
    return R.check_within(got[:, cols], S[:, cols], bound[:, cols], what)


# ------------------------------------------------------------------------------------------------ 1. the C ABI
def test_odd_tile_count_and_straddling_waves(dev):
    """n = 16 * 23, clusters of 1, 15, 16, 17, 63, 64, 65 (and 33, 20) points padded to 16 rows: two workgroups, the second with
    48 of its 256 rows missing and two idle waves, the double-buffered loop's odd tail, waves whose rows and whose column tiles
    belong to several clusters, and cluster id 3 of 10 without a tile (its column is not written)."""
    lay = R.direct_case("straddle")
    assert len(lay["x"]) == 16 * 23 and not (lay["tile_cluster"] == 3).any()
    check_sums(kernel_sums(dev, lay), lay, "sums, 23 tiles")


def test_one_tile_one_cluster(dev):
    """n = 16, n_clusters = 1: one wave with 16 rows, three tail waves that centre on the last row and write nothing."""
    lay = R.direct_case("one")
    assert len(lay["x"]) == 16 and lay["K"] == 1
    check_sums(kernel_sums(dev, lay), lay, "sums, one tile")


def test_three_hundred_small_clusters(dev):
    """300 clusters of 3 to 40 points (what the fine-grained mode produces): a flush every one to three tiles."""
    lay = R.direct_case("many")
    assert lay["K"] == 300 and len(np.unique(lay["tile_cluster"])) == 300
    check_sums(kernel_sums(dev, lay), lay, "sums, 300 clusters")


def test_padding_rows_count_for_nothing(dev):
    """Padding rows that are points of their own (coordinates around 1e3, weight 0) instead of copies of a cluster member: inside
    the bound, and the rows that hold points get the SAME BITS either way -- no wave centres on a padding row here, so nothing but
    the weight-0 columns differs between the two calls."""
    far, copy = R.direct_case("straddle_far"), R.direct_case("straddle")
    assert np.array_equal(far["w"], copy["w"]) and (far["w"][::64] == 1.0).all()
    real = far["w"] > 0
    assert np.array_equal(far["x"][real], copy["x"][real]) and np.abs(far["x"][~real]).min() > 900.0
    got_far, got_copy = kernel_sums(dev, far), kernel_sums(dev, copy)
    check_sums(got_far, far, "sums, padding far away")
    assert np.array_equal(got_far[real].view(np.int32), got_copy[real].view(np.int32))


def test_exact_duplicates(dev):
    """Points that are exact copies of others, inside a cluster and across clusters (a singleton among them): distance 0 off the
    diagonal, where the Gram form leaves sqrt(rounding) and only the row's own column is zeroed."""
    lay = R.direct_case("straddle_dups")
    check_sums(kernel_sums(dev, lay), lay, "sums, duplicates")


def test_long_running_sum(dev):
    """One cluster of 100 000 points beside one of 500: 6 250 adds into each lane's running sum.  64 rows (both clusters, the
    partly used last wave, padding) against the float64 sums of those rows."""
    lay = R.direct_case("long")
    n = len(lay["x"])
    assert n == 100000 + 512
    rows = np.unique(np.concatenate([np.random.default_rng(1).integers(0, n, 52), [0, 63, 64, 99999, 100000, 100499, 100500, n - 1],
                                     np.arange(100480, 100484)]))
    assert len(rows) == 64
    check_sums(kernel_sums(dev, lay), lay, "sums, 100 000-point cluster", rows=rows)


# ------------------------------------------------------------------------------------------------ 2. per point, through the library
def check_samples(name, n, d, path, block=4096):
    from idelucs_amd import posthoc
    x, lab = R.sample_case(name, n, d)
    want, want_score, bound = R.sample_reference(name, n, d, path)
    got = posthoc.silhouette_samples_device(x.copy(), lab.copy(), block=block)
    score = posthoc.silhouette_score_device(x.copy(), lab.copy(), block=block)
    assert got.dtype == np.float64 and got.shape == (n,)
    print(f"{name} n={n} d={d} {path}: score {score:.9f}, sklearn {want_score:.9f}, difference {abs(score - want_score):.3g}")
    R.check_within(got, want, bound, f"{name} n={n} d={d} {path}, per point")
    assert abs(got.mean() - score) < 1e-12                       # the same values, added up in another order
    assert abs(score - want_score) < 2e-5, (score, want_score)


@pytest.mark.parametrize("name", R.SAMPLE_CASES)
def test_samples_one_pass(dev, monkeypatch, name):
    """3 000 points through the one-pass kernel (its threshold lowered to 0), every point against sklearn within the bound, the
    score within 2e-5."""
    from idelucs_amd import posthoc
    monkeypatch.setattr(posthoc, "SILHOUETTE_ONE_PASS_MIN", 0)
    monkeypatch.setitem(posthoc.OPTIONS, "silhouette", "")
    check_samples(name, 3000, 64, "kernel")


def test_samples_at_the_one_pass_threshold(dev, monkeypatch):
    """The module's own threshold: 4 096 points take the kernel, 4 095 the GEMM form (in row blocks of 1 000, the last one short)."""
    from idelucs_amd import posthoc
    monkeypatch.setitem(posthoc.OPTIONS, "silhouette", "")
    assert posthoc.SILHOUETTE_ONE_PASS_MIN == 4096
    check_samples("blobs", 4096, 64, "kernel")
    check_samples("blobs", 4095, 64, "gemm", block=1000)


def test_samples_gemm_with_40_coordinates(dev, monkeypatch):
    """Data that are not 64 wide take the GEMM form whatever their size."""
    from idelucs_amd import posthoc
    monkeypatch.setattr(posthoc, "SILHOUETTE_ONE_PASS_MIN", 0)
    monkeypatch.setitem(posthoc.OPTIONS, "silhouette", "")
    check_samples("blobs", 3000, 40, "gemm")


def test_samples_keep_the_callers_order(dev, monkeypatch):
    """Un-permuting: labels given as arbitrary values in arbitrary order; a singleton scores an exact 0 at its own position."""
    from idelucs_amd import posthoc
    monkeypatch.setattr(posthoc, "SILHOUETTE_ONE_PASS_MIN", 0)
    x, lab = R.sample_case("singletons")
    got = posthoc.silhouette_samples_device(x.copy(), lab.copy())
    assert (got[[3, 500, 501, 1777, 2999]] == 0.0).all() and (got != 0.0).sum() == 2995
