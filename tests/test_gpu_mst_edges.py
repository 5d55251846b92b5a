"""Prim's minimum spanning tree on the device (csrc/mst.hip: idl_mst_prim, idl_mst_prim_local) against sklearn's own loop, edge for
edge: nodes, order and float64 weights, bit for bit, through posthoc.hdbscan_device -- the permutation, `orig`, `start`, the
float32-or-float64 choice and the code tables are part of what is compared.  The reference is tests/mst_ref.py (pinned to
sklearn's mst_from_data_matrix on the host by tests/test_mst_reference.py); both sides start from the same core distances
(mst_ref.core_by_definition), so the comparison is of the tree alone.  The inputs tie (lattices, grids, duplicates, equal points),
sit around one 256-thread workgroup, and have 1 to 256 features in float32 and float64: mst_ref.datasets().

Not covered here: idl_mst_prim_lazy (refuses n < 65536; test_gpu_knn.py::test_lazy_prim_builds_the_same_tree compares it with the
filtered scan pinned here) and the strided tail behind the look-ahead (n > 2^20)."""
import functools

import numpy as np
import pytest

import mst_ref

pytestmark = pytest.mark.gpu

FIELDS = ("current_node", "next_node", "distance")
PIVOTS = {"grid-k14": 3, "size-n1027": 3}       # groups of _spatial_order in the filtered runs: 6 unless 6 leave the filter too little to do (below)
IN_RUN_MIN = 0.5                               # share of the points whose group is their 256-position run's first point's (n >= 1024)


def _filterable(name):
    d = mst_ref.dataset(name)[1].shape[1]
    return d % 4 == 0 and d <= 64


@functools.lru_cache(maxsize=None)
def _reference_labels(name):
    """(labels, probabilities, None) of sklearn's tree code on the reference edges, or (None, None, the exception it raises)."""
    try:
        return mst_ref.labels_from_edges(mst_ref.reference(name)[1], mst_ref.dataset(name)[2]) + (None,)
    except Exception as err:      # noqa: BLE001 -- whatever sklearn says of a degenerate tree, the device path must say too
        return None, None, err


def _check(name, stats_path):
    """Run hdbscan_device on the dataset from the reference core distances; compare edges, then labels."""
    from idelucs_amd import posthoc
    _, x, k = mst_ref.dataset(name)
    core, edges = mst_ref.reference(name)
    stats, result, raised = {}, None, None
    try:
        result = posthoc.hdbscan_device(x.copy(), k, core=core.copy(), stats=stats)
    except Exception as err:      # noqa: BLE001 -- sklearn's tree code on a degenerate tree: the edges are in `stats` by then
        if "mst_edges" not in stats:
            raise
        raised = err
    assert stats["mst_path"] == stats_path
    assert ("mst_groups" in stats) == (stats_path != "plain")
    got = stats["mst_edges"]
    assert len(got) == len(x) - 1
    for field, ref in zip(FIELDS, edges):
        same = got[field] == ref
        if not same.all():
            i = int(np.argmin(same))
            lo, hi = max(i - 2, 0), i + 3
            pytest.fail(f"{name} ({stats_path}): {field} differs at {int((~same).sum())} of {len(ref)} edges, first at {i}: device "
                        f"{[(int(a), int(b), float(c)) for a, b, c in got[lo:hi]]}, sklearn "
                        f"{list(zip(edges[0][lo:hi].tolist(), edges[1][lo:hi].tolist(), edges[2][lo:hi].tolist()))}")
    labels, prob, ref_raised = _reference_labels(name)
    if ref_raised is not None or raised is not None:
        assert type(raised) is type(ref_raised), (raised, ref_raised)
    else:
        assert np.array_equal(result[0], labels) and np.array_equal(result[1], prob)
    return stats


@pytest.mark.parametrize("name", mst_ref.dataset_names())
def test_plain_prim_is_sklearns_edge_for_edge(name):
    """idl_mst_prim: prim_step_kernel<float, false, true> (64 float32 features), <float, false, false> (another width) and
    <double, false, false> (values float32 does not hold)."""
    _check(name, "plain")


@pytest.mark.parametrize("name", [n for n in mst_ref.dataset_names() if _filterable(n)])
def test_filtered_prim_is_sklearns_edge_for_edge(name, monkeypatch):
    """idl_mst_prim_local, the 8-bit lower bound in front of the exact distances: <float, true, true>, <float, true, false>,
    <double, true, false>.  With the default 256 pivots a small input leaves the filter idle -- it acts on a point only when the
    point shares its group with the first point of its 256-position run (the kernel's in_run) -- so the order is cut into 6
    groups (PIVOTS: fewer where 6 miss the share), and from 1024 points on at least half of the points must be such."""
    import torch
    from idelucs_amd import posthoc
    _, x, _ = mst_ref.dataset(name)
    pivots = PIVOTS.get(name, 6)
    spatial_order = posthoc._spatial_order
    monkeypatch.setattr(posthoc, "MST_FILTER_MIN", 0)
    monkeypatch.setattr(posthoc, "_spatial_order", lambda x64, pivots_=pivots, seed=0: spatial_order(x64, pivots=pivots_, seed=seed))
    n = len(x)
    _, gid = posthoc._spatial_order(torch.from_numpy(x.copy()).cuda())
    gid = gid.cpu().numpy()
    p = np.arange(n)
    share = float(np.mean(gid == gid[p - p % 256]))
    print(f"{name}: n = {n}, {pivots} pivots, {int(gid[-1]) + 1} groups, in-run share {share:.3f}")
    if n >= 1024:
        assert share >= IN_RUN_MIN
    stats = _check(name, "local")
    assert stats["mst_groups"] == int(gid[-1]) + 1


@pytest.mark.parametrize("name", [n for n in mst_ref.dataset_names() if n.split("-")[0] in ("lattice", "lattice12", "duplicates", "grid")])
def test_matrix_core_distances_on_ties(name, monkeypatch):
    """Whole bands of equal distances sit at rank k on these inputs: the Gram form only FINDS the neighbours around that rank
    (_core_distances_rows, its re-ranking window `pad`); the value must still be the definition's, bit for bit."""
    import torch
    from idelucs_amd import posthoc
    _, x, k = mst_ref.dataset(name)
    n = len(x)
    rows = np.arange(n) if n <= 513 else np.sort(np.random.default_rng(1).choice(n, 256, replace=False))
    monkeypatch.setitem(posthoc.OPTIONS, "knn", "matrix")
    dev = torch.device("cuda")
    got = posthoc.core_distances_device(torch.from_numpy(x.copy()).to(dev), k, dev).cpu().numpy()
    ref = mst_ref.reference(name)[0][rows]
    bad = np.nonzero(got[rows] != ref)[0]
    assert bad.size == 0, f"{name}: {bad.size} of {len(rows)} rows differ, first row {rows[bad[0]]}: {got[rows][bad[0]]!r} against {ref[bad[0]]!r}"


class _Recorder:
    """libidelucs_hip with every call noted: (name, return value)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            rc = fn(*args)
            self.calls.append((name, rc))
            return rc
        return call


@pytest.mark.parametrize("case", ["one point", "k above n", "nan", "257 features"])
def test_hdbscan_device_refuses_what_it_cannot_do(case, monkeypatch):
    """One point, more neighbours than points and a NaN coordinate are ValueErrors before the library is entered at all; 257
    features get as far as idl_mst_prim, whose argument check (prim_run: the first thing it does) answers IDL_ERR_ARG -- no Prim
    kernel was launched in any of them, and the device is as usable afterwards as before."""
    import torch
    from idelucs_amd import _lib, posthoc
    rng = np.random.default_rng(0)
    x, k, core = rng.normal(size=(40, 8)), 5, None
    if case == "one point":
        x = x[:1]
    elif case == "k above n":
        k = 41
    elif case == "nan":
        x[17, 3] = np.nan
    else:
        x = rng.normal(size=(40, 257))
        core = mst_ref.core_by_definition(x, k)               # (so that nothing but Prim is asked of the library)
    rec = _Recorder(_lib.lib)
    monkeypatch.setattr(_lib, "lib", rec)
    with pytest.raises(ValueError) as info:
        posthoc.hdbscan_device(x, k, core=core)
    calls = [c for c in rec.calls if c[0] != "idl_last_error"]
    if case == "257 features":
        assert [c[0] for c in calls] == ["idl_mst_prim_workspace", "idl_mst_prim"] and calls[1][1] == _lib.IDL_ERR_ARG
        assert "features" in str(info.value)
    else:
        assert calls == []
    monkeypatch.undo()
    torch.cuda.synchronize()
    name = "size-n3"
    stats = {}
    posthoc.hdbscan_device(mst_ref.dataset(name)[1].copy(), 3, core=mst_ref.reference(name)[0].copy(), stats=stats)
    assert all(np.array_equal(stats["mst_edges"][f], ref) for f, ref in zip(FIELDS, mst_ref.reference(name)[1]))
