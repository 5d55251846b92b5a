"""The a-priori rounding bound of tests/silhouette_ref.py, checked without a GPU: a float32 numpy replay of silhouette_sums_kernel's
arithmetic (csrc/knn.hip: coordinates centred on the first row of every 64-row wave, 16-step fma chains and two adds for the squared
norms, a float32 dot product, (sqa + sqc) - 2 acc clamped at 0, square root, weight, exact zeros on the diagonal, one running sum
per column lane and cluster, four pairwise adds at the flush) goes through check_within -- the assertion tests/test_gpu_silhouette.py
applies to the kernel.  The faithful replay must pass on every input; five replays with one mistake each, the kind that touches a
handful of rows, must fail on every benign input.  That they fail is arranged, not hoped for: a benign input asserts -- on the
reference alone -- that the bound of every sum is below a quarter of the smallest distance inside it, so one distance left out,
misplaced or added moves a sum by three bounds at least."""
import functools

import numpy as np
import pytest

import silhouette_ref as R

F32 = np.float32


def _sq_norm(v):
    """|v|^2 per row as the kernel forms it: the lane that holds coordinates 16 q .. 16 q + 15 runs a 16-step fma chain (emulated:
    the product of two float32 is exact in float64, the sum is rounded once to float32), then the four lanes add up pairwise."""
    part = np.zeros((v.shape[0], 4), dtype=F32)
    v4 = v.reshape(v.shape[0], 4, 16).astype(np.float64)
    for s in range(16):
        part = (part.astype(np.float64) + v4[:, :, s] * v4[:, :, s]).astype(F32)
    return (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])


def replay_distances(x):
    """(d [n, n] float32 with the diagonal zeroed, the diagonal as the Gram form left it) in the kernel's arithmetic."""
    x32 = np.asarray(x).astype(F32)
    n = len(x32)
    d = np.empty((n, n), dtype=F32)
    for r0 in range(0, n, 64):
        a, b = x32[r0:r0 + 64] - x32[r0], x32 - x32[r0]
        acc = a @ b.T
        d2 = (_sq_norm(a)[:, None] + _sq_norm(b)[None, :]) - F32(2.0) * acc
        d[r0:r0 + 64] = np.sqrt(np.maximum(d2, F32(0.0)))
    raw = d.diagonal().copy()
    np.fill_diagonal(d, 0.0)
    return d, raw


def replay_sums(d, raw, w, tile_cluster, K, mutation=None):
    """The kernel's epilogue on replay_distances' output: sums [n, K] float32 (zero where no flush wrote).  mutation, one mistake:
      ("drop_column", j)     column j left out
      ("late_flush", j)      column j added to the cluster after its own
      ("keep_diagonal", t)   the rows of tile t keep the Gram form's value of their own diagonal
      ("pad_weight", p)      the padding row p counted with weight 1
      ("skip_last_tile",)    the last tile never processed (what a double-buffered loop without its odd tail does)"""
    kind = mutation[0] if mutation else None
    n = d.shape[0]
    w = np.asarray(w).astype(F32).copy()
    ntile = n // 16 - (1 if kind == "skip_last_tile" else 0)
    if kind in ("drop_column", "late_flush"):
        w[mutation[1]] = 0.0
    if kind == "pad_weight":
        assert w[mutation[1]] == 0.0
        w[mutation[1]] = 1.0
    sums = np.zeros((n, K), dtype=F32)
    tot = np.zeros((n, 16), dtype=F32)

    def flush(c):
        v = tot.copy()
        for _ in range(4):
            v = v[:, 0::2] + v[:, 1::2]
        sums[:, c] = v[:, 0]
        tot[:] = 0.0

    cur = tile_cluster[0]
    for t in range(ntile):
        if tile_cluster[t] != cur:
            flush(cur)
            cur = tile_cluster[t]
        blk = d[:, 16 * t:16 * t + 16]
        if kind == "keep_diagonal" and t == mutation[1]:
            blk = blk.copy()
            blk[16 * t + np.arange(16), np.arange(16)] = raw[16 * t:16 * t + 16]
        tot += blk * w[None, 16 * t:16 * t + 16]
    flush(cur)
    if kind == "late_flush":
        j = mutation[1]
        later = [c for c in tile_cluster[j // 16:] if c != tile_cluster[j // 16]]
        sums[:, later[0]] += d[:, j]
    return sums


def _odd_tail(lay_args):
    """The wrapper's layout with the last cluster padded to 16 rows only and chosen so that the tile count is odd and the last tile
    holds points: every wave but the last keeps its rows and its centre."""
    x, lab, K = lay_args
    counts = np.bincount(lab, minlength=K)
    odd = [c for c in range(K) if counts[c] and (-(-counts[c] // 16)) % 2 == 1]
    assert odd, "no cluster with an odd number of tiles"
    order = [c for c in range(K) if counts[c] and c != odd[-1]] + [odd[-1]]
    return R.layout(x, lab, K, pad=64, order=order, last_pad=16)


@functools.lru_cache(maxsize=None)
def _prepared(name, variant):
    """(layout, S, bound, dmin, d, raw) of one input: float64 reference and float32 replay distances, computed once."""
    if name in R.SAMPLE_CASES:
        x, labels = R.sample_case(name)
        uniq, lab = np.unique(labels, return_inverse=True)
        lay = R.layout(x, lab, len(uniq), pad=64) if variant == "wrapper" else _odd_tail((x, lab, len(uniq)))
    else:
        lay = R.direct_case(name)
    n = len(lay["x"])
    S, bound, dmin = R.sums_ref_and_bound(lay["x"], lay["w"], lay["tile_cluster"], lay["K"], R.kernel_centres(n), want_dmin=True)
    d, raw = replay_distances(lay["x"])
    return lay, S, bound, dmin, d, raw


def _written(lay):
    return np.isin(np.arange(lay["K"]), lay["tile_cluster"])


@pytest.mark.parametrize("name", R.SAMPLE_CASES + ("straddle", "straddle_far", "straddle_dups", "one"))
def test_faithful_replay_is_inside_the_bound(name):
    """Every input of the GPU tests with at most 3 000 points, in the layout the GPU tests run it in: each sum of the faithful
    replay within its bound -- the inputs and gamma are sound."""
    lay, S, bound, _, d, raw = _prepared(name, "wrapper")
    assert len(lay["x"]) <= 3000 + 64 * lay["K"]
    got = replay_sums(d, raw, lay["w"], lay["tile_cluster"], lay["K"])
    cols = _written(lay)
    R.check_within(got[:, cols], S[:, cols], bound[:, cols], f"replay {name}")
    assert (got[:, ~cols] == 0.0).all()
    if name in R.SAMPLE_CASES:                                    # and through to the per-point values
        x, labels = R.sample_case(name)
        _, lab = np.unique(labels, return_inverse=True)
        counts = np.bincount(lab).astype(np.float64)
        want, _, sbound = R.sample_reference(name)
        worst, _ = R.check_within(R.samples_from_sums(got[lay["pos"]].astype(np.float64), lab, counts), want, sbound, f"replay {name}, per point")


MUTATION_CASES = tuple((n, "tail") for n in R.BENIGN) + (("straddle", "wrapper"),)


@pytest.mark.parametrize("name,variant", MUTATION_CASES)
def test_mutated_replays_are_outside_the_bound(name, variant):
    """On every benign input (laid out with an odd tile count, so that all five mistakes can happen) the faithful replay passes and
    each mutated one fails the same assertion."""
    lay, S, bound, dmin, d, raw = _prepared(name, variant)
    w, tc, K = lay["w"], lay["tile_cluster"], lay["K"]
    n = len(w)
    assert (n // 16) % 2 == 1 and w[-16:].any()
    cols = _written(lay)
    # benign: every sum's bound below a quarter of the smallest distance in it (on the reference alone)
    # (the rows that hold points: a padding row is a copy, at distance 0 of its original, and nothing reads its sums)
    real = w > 0
    assert (bound[real][:, cols] < 0.25 * dmin[real][:, cols]).all(), float((bound[real][:, cols] / dmin[real][:, cols]).max())

    def check(mutation):
        got = replay_sums(d, raw, w, tc, K, mutation)
        R.check_within(got[:, cols], S[:, cols], bound[:, cols], f"replay {name} {mutation}")

    check(None)
    col_cluster = np.repeat(tc, 16)
    sizes = np.bincount(col_cluster, weights=w, minlength=K)
    big = int(tc[0])                                              # a cluster that is not the last in memory
    j = int(np.nonzero((col_cluster == big) & (w > 0))[0][-1])
    pads = np.nonzero((w == 0) & (sizes[col_cluster] >= 2))[0]
    # the tile whose un-zeroed diagonal shows most: |raw| against the bound of the row's own sum
    with np.errstate(divide="ignore", invalid="ignore"):
        show = np.where(w > 0, raw / bound[np.arange(n), col_cluster], 0.0)
    show = np.nan_to_num(show, posinf=np.finfo(np.float64).max).reshape(-1, 16).max(1)
    for mutation in (("drop_column", j), ("late_flush", j), ("keep_diagonal", int(show.argmax())), ("pad_weight", int(pads[0])), ("skip_last_tile",)):
        with pytest.raises(AssertionError, match="outside their bound"):
            check(mutation)


def test_check_within_rejects_nan_and_accepts_exact_zero():
    R.check_within(np.zeros(3), np.zeros(3), np.zeros(3), "zeros")
    with pytest.raises(AssertionError):
        R.check_within(np.array([0.0, np.nan]), np.zeros(2), np.ones(2), "nan")
    with pytest.raises(AssertionError):
        R.check_within(np.array([1e-30]), np.zeros(1), np.zeros(1), "zero bound")


def test_gemm_form_on_the_host_is_inside_its_bound():
    """posthoc's GEMM form runs on any torch device: on the host, every point of silhouette_samples_device against sklearn within
    the GEMM bound (float32 products in whatever order the host BLAS takes them), in the caller's order, and the score is their mean."""
    from idelucs_amd import posthoc
    x, lab = R.sample_case("blobs", 3000, 40)
    want, want_score, bound = R.sample_reference("blobs", 3000, 40, "gemm")
    got = posthoc.silhouette_samples_device(x.copy(), lab.copy(), device="cpu", block=1000)
    score = posthoc.silhouette_score_device(x.copy(), lab.copy(), device="cpu", block=1000)
    assert got.dtype == np.float64 and got.shape == (3000,)
    R.check_within(got, want, bound, "GEMM form on the host, per point")
    assert abs(got.mean() - score) < 1e-12 and abs(score - want_score) < 2e-5
