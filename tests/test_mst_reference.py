"""tests/mst_ref.py against sklearn itself, on the host: the reference the GPU tests (test_gpu_mst_edges.py) hold Prim's kernels to
is sklearn's mst_from_data_matrix edge for edge -- nodes, order, float64 weights -- on every test input, and the inputs built for
their ties do tie."""
import numpy as np
import pytest

import mst_ref


@pytest.mark.parametrize("name", mst_ref.dataset_names())
def test_prim_reference_is_sklearns(name):
    try:
        from sklearn.cluster._hdbscan._linkage import mst_from_data_matrix  # noqa: F401
    except ImportError as err:
        pytest.skip(f"this scikit-learn has no private mst_from_data_matrix ({err})")
    _, x, _ = mst_ref.dataset(name)
    core, edges = mst_ref.reference(name)
    theirs = mst_ref.sklearn_prim(x, core)
    for field, a, b in zip(("current_node", "next_node", "distance"), edges, theirs):
        assert a.dtype == b.dtype and np.array_equal(a, b), field


@pytest.mark.parametrize("name", [n for n in mst_ref.dataset_names() if n.split("-")[0] in mst_ref.TIE_HEAVY])
def test_tie_heavy_inputs_tie(name):
    _, edges = mst_ref.reference(name)
    share = mst_ref.tied_share(edges[2])
    print(name, "share of tied weights", share)
    assert share > 0.4


def test_datasets_are_what_they_claim():
    items = mst_ref.datasets()
    assert len({name for name, _, _ in items}) == len(items)
    assert {name.split("-")[0] for name, _, _ in items} >= set(mst_ref.TIE_HEAVY)
    for name, x, k in items:
        n, d = x.shape
        assert x.dtype == np.float64 and 2 <= n <= 3072 and 2 <= k <= n and np.all(np.isfinite(x)), name
        f32_exact = np.array_equal(x.astype(np.float32).astype(np.float64), x)
        assert f32_exact != name.startswith("width-f64"), name
    assert {x.shape[0] for name, x, _ in items if name.startswith("size-")} == {2, 3, 255, 256, 257, 1027}
    assert {x.shape[1] for name, x, _ in items if name.startswith("width-f64")} == {1, 3, 16, 40, 65, 256}
    x = mst_ref.dataset("lattice12-k2")[1]
    assert len(np.unique(x, axis=0)) == 1536                   # every point twice
    x = mst_ref.dataset("duplicates-k2")[1]
    assert len(np.unique(x[len(x) // 2:], axis=0)) <= 40


def test_core_by_definition_on_a_case_done_by_hand():
    """0, 3, 4 and 10 on a line: the distances of each point, sorted, are its row."""
    x = np.array([[0.0], [3.0], [4.0], [10.0]])
    assert np.array_equal(mst_ref.core_by_definition(x, 2), [3.0, 1.0, 1.0, 6.0])
    assert np.array_equal(mst_ref.core_by_definition(x, 3, rows=[0, 3]), [4.0, 7.0])
    # k = 2, cores 3 1 1 6.  From 0: 3, 4, 10 -> node 1.  From 1: max(1, 1, 1) = 1 < 4 and max(1, 6, 7) = 7 < 10 -> node 2.  From 2: 6 < 7
    cur, nxt, w = mst_ref.prim_reference(x, mst_ref.core_by_definition(x, 2))
    assert cur.tolist() == [0, 1, 2] and nxt.tolist() == [1, 2, 3] and w.tolist() == [3.0, 1.0, 6.0]


def test_prim_reference_tie_rule_on_a_case_done_by_hand():
    """The unit square, k = 2: every core distance is 1.  From corner 0 its two neighbours tie at 1 and the FIRST is taken; from
    there corner 3 falls to 1 (source 1); corner 2 (source 0) precedes it; from 2, corner 3 is offered 1 again -- not smaller, so
    its source stays 1."""
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    core = mst_ref.core_by_definition(x, 2)
    assert core.tolist() == [1.0] * 4
    cur, nxt, w = mst_ref.prim_reference(x, core)
    assert cur.tolist() == [0, 0, 1] and nxt.tolist() == [1, 2, 3] and w.tolist() == [1.0] * 3
