"""The core-distance kernels of csrc/knn.hip stage by stage: idl_knn_window and idl_knn_select straight through the C ABI, with
windows the TEST chooses (true ranks, not posthoc's sampled bracket), against float64 distances from the difference vector and
the specification restated in tests/knn_ref.py (its module docstring has the chain of claims; tests/test_knn_reference.py checks
the reference, a float32 replay of the window pass and four planted mistakes without a GPU).

  1. the window pass column by column: `delta`, every kept (value, index), every column that must / must not be kept, cnt_lo,
     cand_cnt -- four datasets in a spatial and a shuffled order, three (k, w);
  2. sizes that are no multiple of the 16-column tile, the 64-row wave or the 256-row workgroup, shards (row0, rows) of a launch,
     a slot that overflows; every output buffer is exactly as long as the ABI says, between two guards of sentinel values;
  3. the rounding bound on operands constructed against it;
  4. the selection after the real window pass: status 0 means the k-th distance bit for bit, and the rows the claims oblige to
     status 0 get it;
  5. the selection on hand-made slots, every branch reached deliberately.

Every test prints what it measured (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest

import knn_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 1024                      # sentinel elements on either side of every output buffer
STATUSES = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _gram_err():
    from idelucs_amd import posthoc
    return posthoc.KNN_GRAM_ERR


class _Out:
    """A device buffer of exactly `size` elements between two guards, everything filled with `fill`."""

    def __init__(self, dev, size, dtype, fill):
        import torch
        self.size, self.fill = size, fill
        self.buf = torch.full((size + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def get(self, what):
        a = self.buf.cpu().numpy()
        fill = a.dtype.type(self.fill)
        assert (a[:GUARD] == fill).all(), f"{what}: written in front of the buffer"
        assert (a[GUARD + self.size:] == fill).all(), f"{what}: written behind the buffer"
        return a[GUARD:GUARD + self.size].copy()


def _in(dev, a, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    return t, ctypes.c_void_p(t.data_ptr())


def run_window(dev, x, lo, hi, row0, rows, cap):
    """idl_knn_window over the rows row0 .. row0 + rows - 1 -> check_window's `out` (numpy)."""
    import torch
    from idelucs_amd import _lib
    n = len(x)
    assert len(lo) == rows and len(hi) == rows and 0 <= row0 and row0 + rows <= n
    xd, xp = _in(dev, x, F32)
    lod, lop = _in(dev, lo, F32)
    hid, hip = _in(dev, hi, F32)
    o = dict(cnt_lo=_Out(dev, rows, torch.int32, R.SENT_I), cand_cnt=_Out(dev, rows, torch.int32, R.SENT_I),
             delta=_Out(dev, rows, torch.float32, R.SENT_F), cand_d2=_Out(dev, rows * cap, torch.float32, R.SENT_F),
             cand_idx=_Out(dev, rows * cap, torch.int32, R.SENT_I))
    _lib.check(_lib.lib.idl_knn_window(xp, n, 64, lop, hip, row0, rows, o["cnt_lo"].ptr, o["cand_cnt"].ptr, o["delta"].ptr,
                                       o["cand_d2"].ptr, o["cand_idx"].ptr, cap, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize(dev)
    out = {name: b.get(name) for name, b in o.items()}
    out["cand_d2"], out["cand_idx"] = out["cand_d2"].reshape(rows, cap), out["cand_idx"].reshape(rows, cap)
    return out


def run_select(dev, x, lo, hi, delta, row0, rows, k, cnt_lo, cand_cnt, cand_d2, cand_idx, cap):
    """idl_knn_select on the given slots -> (core [n] float64, SENT_F where not written; status [rows])."""
    import torch
    from idelucs_amd import _lib
    n = len(x)
    keep = [_in(dev, x, F32), _in(dev, lo, F32), _in(dev, hi, F32), _in(dev, delta, F32), _in(dev, cnt_lo, np.int32),
            _in(dev, cand_cnt, np.int32), _in(dev, np.reshape(cand_d2, -1), F32), _in(dev, np.reshape(cand_idx, -1), np.int32)]
    assert all(len(t) == rows for t, _ in keep[1:6]) and len(keep[6][0]) == rows * cap and len(keep[7][0]) == rows * cap
    xp, lop, hip, dp, clp, ccp, d2p, ixp = (p for _, p in keep)
    core, status = _Out(dev, n, torch.float64, R.SENT_F), _Out(dev, rows, torch.int32, R.SENT_I)
    _lib.check(_lib.lib.idl_knn_select(xp, n, 64, lop, hip, dp, row0, rows, k, clp, ccp, d2p, ixp, cap, core.ptr, status.ptr,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize(dev)
    core, status = core.get("core"), status.get("status")
    assert (core[:row0] == R.SENT_F).all() and (core[row0 + rows:] == R.SENT_F).all(), "core written outside the launch's rows"
    return core, status


def check_select(core, status, d2, k, row0, must):
    """Test 4's assertions: d2 [rows, n] true values of the launch's rows, must = must_succeed(...)."""
    rows = len(d2)
    assert np.isin(status, STATUSES).all(), f"a status outside {STATUSES}: {np.unique(status).tolist()}"
    done = status == 0
    want = np.sqrt(R.kth_d2(d2, k))
    mine = core[row0:row0 + rows]
    assert np.array_equal(mine[done], want[done]), \
        f"status 0 with another value than the k-th distance in {int((mine[done] != want[done]).sum())} rows"
    assert (mine[~done] == R.SENT_F).all(), "a flagged row's core distance was written"
    assert done[must].all(), f"{int((~done[must]).sum())} rows flagged {np.unique(status[must & ~done]).tolist()} that the bound obliges to status 0"
    print(f"status counts {np.bincount(status, minlength=5).tolist()}, obliged {int(must.sum())} of {rows}")


def window_and_select(dev, x, d2, lo, hi, row0, rows, k, cap, what):
    """Both stages over one launch with all assertions of tests 1 and 4 -> (out, core, status)."""
    dref = R.delta_ref(x, hi, row0, rows, _gram_err())
    must = R.must_succeed(d2, k, lo, hi, dref, cap)                # from the reference alone, before anything runs on the GPU
    out = run_window(dev, x, lo, hi, row0, rows, cap)
    R.check_window(out, d2, lo, hi, dref, cap, what)
    core, status = run_select(dev, x, lo, hi, out["delta"], row0, rows, k, out["cnt_lo"], out["cand_cnt"], out["cand_d2"], out["cand_idx"], cap)
    check_select(core, status, d2, k, row0, must)
    return out, core, status


# ------------------------------------------------------------------------------------------------ 1. the window pass, column by column
CASES = [(name, order, k, w) for name in R.DATASETS for order in R.ORDERS for k, w in R.KW]
_window_out = {}


def _window_case(dev, name, order, k, w):
    """(x, d2, lo, hi, dref, cap, out) of a case; the pass runs once for tests 1 and 4."""
    x, d2 = R.reference(name, order)
    lo, hi = R.rank_window(d2, k, w)
    cap = R.window_cap(w)
    key = (name, order, k, w)
    if key not in _window_out:
        _window_out[key] = run_window(dev, x, lo, hi, 0, len(x), cap)
    return x, d2, lo, hi, R.delta_ref(x, hi, 0, len(x), _gram_err()), cap, _window_out[key]


@pytest.mark.parametrize("name,order,k,w", CASES)
def test_window_pass_column_by_column(dev, name, order, k, w):
    """n = 1500 (six workgroups, the last with 220 rows, 93.75 column tiles); lo / hi the float32 roundings of the true squared
    distances at ranks k - w and k + w (k = 2: no lower rank, lo = -1e30); cap = 256.  In the shuffled order a wave's centre lies a
    cluster distance from its rows: the bound grows and must still hold.  duplicates: lo = hi = 0 on the copies' rows."""
    x, d2, lo, hi, dref, cap, out = _window_case(dev, name, order, k, w)
    R.check_window(out, d2, lo, hi, dref, cap, f"{name}/{order} k={k} w={w}")


# ------------------------------------------------------------------------------------------------ 2. sizes, shards, canaries, overflow
@functools.lru_cache(maxsize=None)
def _sized(n):
    x = R.blobs(n, seed=7)
    d2 = R.true_d2(x)
    for a in (x, d2):
        a.setflags(write=False)
    return x, d2


def _window_or_everything(d2_rows, d2_max, k, w):
    """rank_window where the ranks exist; else nothing below and twice the largest true value above."""
    n = d2_rows.shape[1]
    if k + w <= n:
        lo, hi = R.rank_window(d2_rows, k, w)
    else:
        lo, hi = np.full(len(d2_rows), R.NOTHING_BELOW, dtype=F32), np.full(len(d2_rows), 2.0 * d2_max, dtype=F32)
    return lo, hi


@pytest.mark.parametrize("n", [1, 15, 17, 255, 257, 1000])
def test_sizes_off_the_tile_the_wave_and_the_workgroup(dev, n):
    """k = min(2, n), w = 16; n < 18: everything under twice the largest distance is kept (n = 1: hi = 0, nothing is)."""
    x, d2 = _sized(n)
    k = min(2, n)
    lo, hi = _window_or_everything(d2, d2.max(), k, 16)
    out, _, status = window_and_select(dev, x, d2, lo, hi, 0, n, k, 256, f"n={n}")
    if n < 18:
        assert (out["cand_cnt"] == (n if n > 1 else 0)).all() and (out["cnt_lo"] == 0).all()
        assert (status == (0 if n > 1 else 1)).all()


@pytest.mark.parametrize("row0,rows", [(0, 1000), (192, 300), (256, 1), (999, 1), (700, 300)])
def test_shards_of_a_launch(dev, row0, rows):
    """n = 1000, k = 21, w = 16: lo, hi and every output addressed by row - row0, the waves centred from row0 on (192 + 64 i: not the
    rows a launch from 0 centres on), a launch of one row, the last row alone, the last 300."""
    x, d2 = _sized(1000)
    d2r = d2[row0:row0 + rows]
    lo, hi = R.rank_window(d2r, 21, 16)
    window_and_select(dev, x, d2r, lo, hi, row0, rows, 21, 256, f"rows {row0}..{row0 + rows - 1}")


def test_slot_overflow_is_counted_not_written(dev):
    """cap = 8 under a window of 50 columns: cand_cnt reports them all, the first 8 slots hold columns of the window, the next row's
    slots and the guards are intact (check_window, run_window), and the selection answers 2."""
    x, d2 = _sized(1000)
    row0, rows, cap = 192, 300, 8
    d2r = d2[row0:row0 + rows]
    _, hi = R.rank_window(d2r, 26, 25)                            # hi at rank 51: 50 columns truly below it
    lo = np.full(rows, R.NOTHING_BELOW, dtype=F32)
    dref = R.delta_ref(x, hi, row0, rows, _gram_err())
    out = run_window(dev, x, lo, hi, row0, rows, cap)
    R.check_window(out, d2r, lo, hi, dref, cap, "cap 8")
    assert (out["cand_cnt"] > cap).all() and (np.abs(out["cand_cnt"] - 50) <= 1).all()
    core, status = run_select(dev, x, lo, hi, out["delta"], row0, rows, 26, out["cnt_lo"], out["cand_cnt"], out["cand_d2"], out["cand_idx"], cap)
    assert (status == 2).all() and (core == R.SENT_F).all()


# ------------------------------------------------------------------------------------------------ 3. the bound on constructed operands
@pytest.mark.parametrize("family", R.FAMILIES)
def test_rounding_bound_on_constructed_operands(dev, family):
    """Operands built against the bound (knn_ref.constructed): lo = -1e30, hi 1 % above the row's largest true value (far_column: 8 on
    the near rows, so that the far columns, 10^8 away, must come out above it: not kept, not counted).  The assertion is
    |kept value - true| <= delta_ref / 2.  Measured on an MI355X, largest |error| / (delta_ref / 2), and (not asserted) the largest
    |error| / (GRAM_ERR (|a - m|^2 + |b - m|^2)), the kernel comment's sharper claim:
        stagnation   0.0099   0.27
        same_sign    0.0060   0.030
        cancelling   0.0089   0.021
        far_column   0.0124   0.047
    A record, not a threshold: the test prints both figures and asserts the first to be at most 1."""
    c = R.constructed(family)
    x, n = c["x"], len(c["x"])
    d2 = R.true_d2(x)
    lo = np.full(n, R.NOTHING_BELOW, dtype=F32)
    hi = (1.01 * d2.max(1) + 2.0 ** -10).astype(F32)
    centre = R.centre_of(np.arange(n), 0, n - 1)
    near_row = np.zeros(n, dtype=bool)
    if family == "far_column":
        near_row = ~c["far"]
        hi[near_row] = c["near_hi"]
    dref = R.delta_ref(x, hi, 0, n, _gram_err())
    out = run_window(dev, x, lo, hi, 0, n, 128)
    worst = R.check_window(out, d2, lo, hi, dref, 128, family)
    used = np.arange(128)[None, :] < out["cand_cnt"][:, None]
    idx = np.where(used, out["cand_idx"], 0)
    err = np.abs(out["cand_d2"].astype(np.float64) - np.take_along_axis(d2, idx, axis=1))
    sq = ((x[:, None, :] - x[None, ::64, :]) ** 2).sum(2)           # [n, 2]: |x_j - m|^2 for both centres
    pair = _gram_err() * (sq[np.arange(n), centre // 64][:, None] + sq[idx, (centre // 64)[:, None]])
    with np.errstate(divide="ignore", invalid="ignore"):
        sharp = np.where(used & (err > 0), err / pair, 0.0)
    print(f"BOUND {family}: |err| / (delta_ref / 2) = {worst:.4f}; |err| / (GRAM_ERR (|a - m|^2 + |b - m|^2)) = {float(sharp.max()):.4f}")
    assert worst <= 1.0
    if family == "far_column":
        assert near_row.sum() == 88 and (out["cnt_lo"] == 0).all()
        kept_far = used & c["far"][idx]
        assert not kept_far[near_row].any(), "a column 10^4 |a - m| away came out under hi"
        assert (out["cand_cnt"][near_row] >= 44).all()             # m and the 43 near points of the row's own wave, at most 4 apart
    else:
        assert (out["cand_cnt"] == n).all(), "hi was to keep every constructed column"


# ------------------------------------------------------------------------------------------------ 4. select after the real window pass
@pytest.mark.parametrize("name,order,k,w", CASES)
def test_select_after_the_window_pass(dev, name, order, k, w):
    """Status 0 means the k-th distance of the definition, bit for bit; a row the claims oblige to status 0 (must_succeed, from float64
    alone) gets it.  blobs and offset: at least 90 % of the rows are obliged, in both orders (asserted on the reference before the
    launch); tight and duplicates have no minimum -- shuffled tight clusters legitimately fail the edge test, the copies' k-th sits
    on the window's end -- and are held to the soundness of status 0."""
    x, d2, lo, hi, dref, cap, out = _window_case(dev, name, order, k, w)
    must = R.must_succeed(d2, k, lo, hi, dref, cap)
    if name in R.BENIGN:
        assert must.mean() >= 0.9, f"only {must.mean():.3f} of the rows are obliged: widen w"
    core, status = run_select(dev, x, lo, hi, out["delta"], 0, len(x), k, out["cnt_lo"], out["cand_cnt"], out["cand_d2"], out["cand_idx"], cap)
    check_select(core, status, d2, k, 0, must)


# ------------------------------------------------------------------------------------------------ 5. select on hand-made slots
def test_select_on_hand_made_slots(dev):
    """knn_ref.hand_made_slots(): one launch from row 5 of 300 points, a row per branch -- rank 0 and count + 1, an empty and an
    overflowed slot, a selection within delta of either end, a NaN (a rank past the band), bands of 1100 and of exactly 1024, a kept
    value one ulp below lo with one at hi under brackets of 2, 3 and 4 radix passes (unclamped, the first is keyed as the largest
    and every rank shifts), lo = -1e30, lo = hi, brackets of 1 to 4 passes, 300 values in one bin of the last pass, ties at the rank
    settled by the band's exact values, one kept value, three true windows.  Status AND value are select_spec's, and the status is the
    one the row was built for; a flagged row leaves its core distance alone."""
    h = R.hand_made_slots()
    exp = R.hand_made_expected(h)
    rows = len(exp)
    core, status = run_select(dev, h["x"], h["lo"], h["hi"], h["delta"], h["row0"], rows, h["k"], h["cnt_lo"], h["cand_cnt"],
                              h["cand_d2"], h["cand_idx"], h["cap"])
    bad = []
    for i, (name, (st, val)) in enumerate(zip(h["names"], exp)):
        got = core[h["row0"] + i]
        print(f"{name}: {h['passes'][i]} passes, status {status[i]} (specified {st}), core {got!r} (specified {val!r})")
        assert st == h["intended"][i]
        if status[i] != st or got != (R.SENT_F if val is None else val):
            bad.append(name)
    assert not bad, f"rows that differ from the specification: {bad}"
