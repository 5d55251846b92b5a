"""tests/knn_ref.py checked without a GPU: its float64 distances are mst_ref's (and so sklearn's) bit for bit; a float32 numpy
replay of knn_window_kernel's arithmetic (csrc/knn.hip: coordinates centred on the wave's first row, float32 squared norms, a
float32 dot product, t2 = sqc - 2 acc compared with lo - sqa and hi - sqa, kept as t2 + sqa) goes through check_window -- the
assertions tests/test_gpu_knn_stages.py applies to the kernel -- and passes on every dataset, order and (k, w), while replays with
one planted mistake each fail; must_succeed covers the benign datasets (the condition test 4 of the GPU module stands on); and
select_spec on slots filled from the replay gives the k-th distance of the definition for every row must_succeed names."""
import numpy as np
import pytest

import knn_ref as R
from mst_ref import _columns, _sq_dist_to, core_by_definition

GRAM_ERR = 144.0 * 2.0 ** -23          # posthoc.KNN_GRAM_ERR (the GPU module takes it from there; this one needs no built library)
F32 = np.float32


def replay_window(x, lo, hi, row0, rows, cap, mutation=None):
    """knn_window_kernel in numpy float32 -> check_window's `out`.  mutation: "no_centring" (bv = raw instead of raw - mv, av alike),
    "le_and_keep" (a column AT lo counted below and kept as well), "drop_last_tile" (the columns of the last 16-column tile never
    seen), "recount" (cand_cnt stops at cap)."""
    x32 = np.asarray(x).astype(F32)
    n = len(x32)
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    out = dict(cnt_lo=np.full(rows, R.SENT_I, np.int32), cand_cnt=np.full(rows, R.SENT_I, np.int32), delta=np.full(rows, R.SENT_F, F32),
               cand_d2=np.full((rows, cap), R.SENT_F, F32), cand_idx=np.full((rows, cap), R.SENT_I, np.int32))
    ncol = (n - 1) // 16 * 16 if mutation == "drop_last_tile" else n
    for w0 in range(0, rows, 64):
        r = row0 + np.arange(w0, min(w0 + 64, rows))
        m = x32[row0 + w0] * F32(0.0 if mutation == "no_centring" else 1.0)
        a, b = x32[r] - m, x32[:ncol] - m
        sqa, sqc = (a * a).sum(1, dtype=F32), (b * b).sum(1, dtype=F32)
        t2 = sqc[None, :] - F32(2.0) * (a @ b.T)
        lo_m, hi_m = (lo[r - row0] - sqa)[:, None], (hi[r - row0] - sqa)[:, None]
        below = t2 <= lo_m if mutation == "le_and_keep" else t2 < lo_m
        inside = (t2 >= lo_m) & (t2 < hi_m)
        reach = np.sqrt(sqa) + np.sqrt(np.maximum(hi[r - row0], F32(0.0)))
        out["delta"][r - row0] = F32(2.0) * F32(GRAM_ERR) * (sqa + F32(1.001) * reach * reach)
        out["cnt_lo"][r - row0] = below.sum(1)
        for i, rl in enumerate(r - row0):
            j = np.nonzero(inside[i])[0]
            out["cand_cnt"][rl] = min(len(j), cap) if mutation == "recount" else len(j)
            j = j[:cap]
            out["cand_d2"][rl, :len(j)] = t2[i, j] + sqa[i]
            out["cand_idx"][rl, :len(j)] = j
    return out


def _case(name, order, k, w):
    x, d2 = R.reference(name, order)
    lo, hi = R.rank_window(d2, k, w)
    return x, d2, lo, hi, R.delta_ref(x, hi, 0, len(x), GRAM_ERR), R.window_cap(w)


def test_true_d2_is_mst_refs_row_by_row():
    x = R.dataset("blobs", "shuffled")
    rows = np.array([0, 1, 63, 64, 700, 1499])
    got = R.true_d2(x, rows, block=4)
    xt = _columns(x)
    for i, r in enumerate(rows):
        assert np.array_equal(got[i], _sq_dist_to(xt, r))
        assert np.array_equal(R.d2_to(x, r, np.arange(len(x))), got[i])
    assert np.array_equal(np.sqrt(R.kth_d2(got, 21)), core_by_definition(x, 21, rows))


def test_centre_of_is_the_first_row_of_the_wave_inside_the_launch():
    assert R.centre_of(np.array([192, 255, 256, 447, 448, 491]), 192, 491).tolist() == [192, 192, 256, 384, 448, 448]
    assert R.centre_of(np.array([0, 63, 64, 999]), 0, 999).tolist() == [0, 0, 64, 960]
    assert int(R.centre_of(999, 999, 999)) == 999 and int(R.centre_of(300, 256, 256 + 40)) == 256


@pytest.mark.parametrize("name", R.DATASETS)
@pytest.mark.parametrize("order", R.ORDERS)
def test_replay_passes_the_window_assertions_and_must_succeed_covers_the_benign_sets(name, order):
    for k, w in R.KW:
        x, d2, lo, hi, dref, cap = _case(name, order, k, w)
        out = replay_window(x, lo, hi, 0, len(x), cap)
        worst = R.check_window(out, d2, lo, hi, dref, cap, f"replay {name}/{order} k={k} w={w}")
        assert worst < 0.25, "random data was expected far inside the bound"
        ms = R.must_succeed(d2, k, lo, hi, dref, cap)
        print(f"must_succeed {name}/{order} k={k} w={w}: {ms.mean():.3f}")
        if name in R.BENIGN:
            assert ms.mean() >= 0.9
        # the selection restated, on the replay's slots: the definition's k-th wherever it is obliged to answer
        kth = np.sqrt(R.kth_d2(d2, k))
        for r in np.nonzero(ms)[0][::37]:
            st, core = R.select_spec(x, r, k, lo[r], hi[r], out["delta"][r], out["cnt_lo"][r], out["cand_cnt"][r], cap,
                                     out["cand_d2"][r], out["cand_idx"][r])
            assert st == 0 and core == kth[r]


@pytest.mark.parametrize("mutation", ["no_centring", "le_and_keep", "drop_last_tile", "recount"])
def test_replays_with_a_planted_mistake_fail(mutation):
    """no_centring needs norms far above the distances (offset); recount a full slot.  le_and_keep shows only where a column's
    computed value IS lo -- lo is the rounded true value of one of the row's columns, so this happens in a few rows of every
    case -- and only in the selection: both counts stay inside their bounds, but together they count that column twice, the rank
    among the kept columns is one short, and status 0 comes with the (k - 1)-th distance."""
    name, order, k, w = {"no_centring": ("offset", "spatial", 21, 16), "le_and_keep": ("blobs", "spatial", 21, 16),
                         "drop_last_tile": ("blobs", "spatial", 200, 24), "recount": ("blobs", "spatial", 200, 24)}[mutation]
    x, d2, lo, hi, dref, cap = _case(name, order, k, w)
    if mutation == "recount":
        cap = 8
    out = replay_window(x, lo, hi, 0, len(x), cap, mutation)
    if mutation != "le_and_keep":
        with pytest.raises(AssertionError):
            R.check_window(out, d2, lo, hi, dref, cap, mutation)
        return
    R.check_window(out, d2, lo, hi, dref, cap, mutation)
    kth = np.sqrt(R.kth_d2(d2, k))
    wrong = 0
    for r in np.nonzero(R.must_succeed(d2, k, lo, hi, dref, cap))[0]:
        st, core = R.select_spec(x, r, k, lo[r], hi[r], out["delta"][r], out["cnt_lo"][r], out["cand_cnt"][r], cap, out["cand_d2"][r], out["cand_idx"][r])
        wrong += st != 0 or core != kth[r]
    print(f"{wrong} rows answer wrongly")
    assert wrong > 0


@pytest.mark.parametrize("family", R.FAMILIES)
def test_constructed_operands_are_what_they_claim(family):
    c = R.constructed(family)
    x = c["x"]
    assert x.shape == (128, 64) and c["far"].sum() == (40 if family == "far_column" else 0)
    e = x[:64] - x[0]
    if family == "stagnation":
        big = np.abs(e) == 1.0
        rows = big.any(1)
        assert rows.sum() == 60 and set(np.nonzero(big)[1]) == set(R.BIG_AT)
        small = np.abs(e[rows])[~big[rows]].astype(np.float64) ** 2
        assert (small < 2.0 ** -24).all() and (small > 0.99 * 2.0 ** -24).all()
        assert (F32(1.0) + small.astype(F32) == F32(1.0)).all()
    elif family == "same_sign":
        assert (np.sort(np.abs(e[1:63]), axis=1) == 1.0 + np.arange(64) * 2.0 ** -12).all()
    elif family == "cancelling":
        d = np.sqrt(R.true_d2(x[:64])[1:, 1:])
        assert np.allclose(np.linalg.norm(e[1:], axis=1), 8.0, rtol=1e-3) and 500 < 8.0 / d[d > 0].mean() < 2000
    else:
        assert np.allclose(np.linalg.norm(e[c["far"][:64]], axis=1), 1.0e4) and np.allclose(np.linalg.norm(e[1:44], axis=1), 1.0)
        assert R.true_d2(x[1:44]).max() <= c["near_hi"] / 2


def test_hand_made_slots_reach_the_branches_they_name():
    h = R.hand_made_slots()
    exp = R.hand_made_expected(h)
    for name, want, (st, core) in zip(h["names"], h["intended"], exp):
        assert st == want, (name, st, want)
    assert set(h["intended"]) == {0, 1, 2, 3, 4}
    by_name = dict(zip(h["names"], h["passes"]))
    assert [by_name[f"{p} pass" + ("es" if p > 1 else "")] for p in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert by_name["lo = -1e30"] == 4 and by_name["lo = hi"] == 1 and by_name["one ulp below lo and at hi, 2 passes"] == 2
    assert by_name["one ulp below lo and at hi, 3 passes"] == 3 and by_name["one ulp below lo and at hi, 4 passes"] == 4
    # the true windows answer with the definition's k-th
    x, row0, k = h["x"], h["row0"], h["k"]
    for i, name in enumerate(h["names"]):
        if name == "a true window":
            assert exp[i][1] == core_by_definition(x, k, [row0 + i])[0]
    # the selection restated differently where the band is a single value: the float64 distance of the rank's own column
    i = h["names"].index("3 passes")
    order = np.argsort(h["cand_d2"][i, :h["cand_cnt"][i]], kind="stable")
    j = h["cand_idx"][i, order[k - h["cnt_lo"][i] - 1]]
    assert exp[i][1] == float(np.sqrt(R.d2_to(x, row0 + i, [j])[0]))
