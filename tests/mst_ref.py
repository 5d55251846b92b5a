"""float64 reference and test inputs for Prim's minimum spanning tree of the mutual-reachability graph (csrc/mst.hip: idl_mst_prim,
idl_mst_prim_local, reached through idelucs_amd.posthoc.hdbscan_device).  Plain numpy / sklearn: nothing here imports the package
under test.  Used by tests/test_mst_reference.py (prim_reference against sklearn's own mst_from_data_matrix, no GPU) and
tests/test_gpu_mst_edges.py (the kernels against prim_reference, bit for bit).

THE LOOP.  sklearn/cluster/_hdbscan/_linkage.pyx, mst_from_data_matrix (1.7): current = 0; n - 1 times: mark current in the tree;
for every j outside it, ascending: mrd = max(core[current], core[j], dist(current, j)); ONLY when mrd < min_reach[j] are
min_reach[j] and source[j] replaced; the next node is the first j with the smallest min_reach (strict <), its edge
(source[j], j, min_reach[j]).  dist is EuclideanDistance64: d += t * t over the coordinates in their order, product and sum each
rounded, one sqrt.  Nothing is compared with a tolerance anywhere: the arithmetic is restated operation for operation.

THE INPUTS (datasets()) are chosen for what a kernel can get wrong without the labels of well-separated blobs noticing: weights
that tie (lattices, integer grids, exact duplicates, all points equal, k = n) so that the order of the edges and the source of
each is decided by the tie rule alone; sizes just around one 256-thread workgroup; feature counts that are no multiple of
anything; float64 values float32 does not hold; tight far-apart clusters, the regime the 8-bit filter was built for."""
import functools

import numpy as np


def _columns(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).T)


def _sq_dist_to(xt, r):
    """sum_c (x[r, c] - x[:, c])^2 for every point, the sum taken coordinate by coordinate in float64 (sklearn's EuclideanDistance:
    _dist_metrics.pyx.tp rdist loop).  xt: the points feature-major."""
    acc = np.zeros(xt.shape[1])
    for col in xt:
        t = col[r] - col
        acc += t * t
    return acc


def core_by_definition(x, k, rows=None, sq_rows=None):
    """sqrt of the k-th smallest of sum_c (a_c - b_c)^2, the row itself included, for the rows `rows` (default: all).
    sq_rows: a dict that keeps every row of squared distances formed here (reference() hands them on to prim_reference)."""
    xt = _columns(x)
    rows = np.arange(xt.shape[1]) if rows is None else np.asarray(rows)
    out = np.empty(len(rows))
    for i, r in enumerate(rows):
        acc = _sq_dist_to(xt, r)
        if sq_rows is not None:
            sq_rows[int(r)] = acc
        out[i] = np.sqrt(np.partition(acc, k - 1)[k - 1])
    return out


def prim_reference(x, core, sq_rows=None):
    """(current_node, next_node, distance), n - 1 each: sklearn's loop (module docstring) in numpy float64.
    sq_rows: rows of squared distances core_by_definition has formed already (the same function of the same values)."""
    xt = _columns(x)
    core = np.asarray(core, dtype=np.float64)
    n = xt.shape[1]
    in_tree = np.zeros(n, dtype=bool)
    min_reach = np.full(n, np.inf)
    source = np.ones(n, dtype=np.int64)
    cur_nodes, next_nodes, weights = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1)
    cur = 0
    for i in range(n - 1):
        in_tree[cur] = True
        mrd = np.maximum(np.maximum(core[cur], core), np.sqrt(sq_rows.pop(cur) if sq_rows and cur in sq_rows else _sq_dist_to(xt, cur)))
        lower = ~in_tree & (mrd < min_reach)
        min_reach[lower] = mrd[lower]
        source[lower] = cur
        j = int(np.argmin(np.where(in_tree, np.inf, min_reach)))          # the first of the smallest
        cur_nodes[i], next_nodes[i], weights[i] = source[j], j, min_reach[j]
        cur = j
    return cur_nodes, next_nodes, weights


def sklearn_prim(x, core):
    """The same three arrays from sklearn's own (private) function; ImportError when this sklearn does not have it."""
    from sklearn.cluster._hdbscan._linkage import mst_from_data_matrix
    from sklearn.metrics import DistanceMetric
    mst = mst_from_data_matrix(np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(core, dtype=np.float64),
                               DistanceMetric.get_metric("euclidean"), 1.0)
    return mst["current_node"].copy(), mst["next_node"].copy(), mst["distance"].copy()


def labels_from_edges(edges, k):
    """What hdbscan_device does with its edges: sklearn's single-linkage and condensed-tree code with HDBSCAN's defaults."""
    from sklearn.cluster._hdbscan._linkage import MST_edge_dtype, make_single_linkage
    from sklearn.cluster._hdbscan._tree import tree_to_labels
    mst = np.empty(len(edges[0]), dtype=MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = edges
    mst = mst[np.argsort(mst["distance"])]
    return tree_to_labels(make_single_linkage(mst), max(int(k), 2), "eom", False, 0.0, None)


def tied_share(weights):
    """Share of the weights that some other edge has too."""
    _, inverse, counts = np.unique(weights, return_inverse=True, return_counts=True)
    return float(np.mean(counts[inverse] > 1))


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _lattice():
    x = np.zeros((256, 64))
    x[:, :4] = np.stack(np.meshgrid(*[np.arange(4.0)] * 4, indexing="ij"), -1).reshape(256, 4)
    return x


def _lattice_copies():
    rng = np.random.default_rng(11)
    base = _lattice()
    parts = []
    for c in range(12):
        part = base[rng.permutation(256)].copy()
        part[:, 4] += 9.0 * (c // 2)                           # 6 integer offsets, each used twice: clusters 9 apart, every point twice
        parts.append(part)
    return np.concatenate(parts)[rng.permutation(3072)]


def _duplicates():
    rng = np.random.default_rng(3)
    n = 1500
    centres = rng.normal(size=(7, 64)) * 2.5
    truth = rng.integers(0, 7, n)
    x = _f32(centres[truth] + rng.normal(size=(n, 64)) * rng.uniform(0.3, 0.9, size=(7,))[truth][:, None])
    x[n // 2:] = x[rng.integers(0, 40, n - n // 2)]
    return x


def _tight():
    rng = np.random.default_rng(9)
    centres = rng.normal(size=(6, 64)) * 30.0
    return _f32(centres[rng.integers(0, 6, 3000)] + rng.normal(size=(3000, 64)) * 0.05)


def _gauss(n, d, seed, f32):
    """Three loose groups (so that the tree has structure) of values that float32 holds (f32) or does not."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(3, d))[rng.integers(0, 3, n)] * 2.0 + rng.normal(size=(n, d)) * 0.5
    x = _f32(x) if f32 else x + 1.0 / 3.0
    assert f32 == bool(np.array_equal(_f32(x), x))
    return x


TIE_HEAVY = ("lattice", "lattice12", "duplicates", "grid", "equal")       # families (the part of a name before "-")


@functools.lru_cache(maxsize=None)
def _datasets():
    out = []
    for k in (2, 9):
        out.append((f"lattice-k{k}", _lattice(), k))
    for k in (2, 7):
        out.append((f"lattice12-k{k}", _lattice_copies(), k))
    for k in (2, 16):
        out.append((f"duplicates-k{k}", _duplicates(), k))
    out.append(("grid-k14", np.random.default_rng(5).integers(0, 3, size=(1300, 64)).astype(np.float64), 14))
    out.append(("equal-k5", np.full((513, 64), 1.5), 5))
    out.append(("tight-k31", _tight(), 31))
    for n in (2, 3, 255, 256, 257, 1027):
        out.append((f"size-n{n}", _gauss(n, 64, 100 + n, True), min(5, n)))
    for d in (1, 3, 16, 40, 65, 256):
        out.append((f"width-f64-d{d}", _gauss(600, d, 200 + d, False), 6))
    out.append(("width-f32-d16", _gauss(600, 16, 216, True), 6))
    out.append(("kn-n700", _gauss(700, 64, 300, True), 700))
    for _, x, _ in out:
        x.setflags(write=False)
    return tuple(out)


def datasets():
    """(name, x float64 [n, d], k) with fixed seeds, n <= 3072; the arrays are shared and read-only."""
    return _datasets()


def dataset(name):
    return next(item for item in _datasets() if item[0] == name)


def dataset_names():
    return [item[0] for item in _datasets()]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(core, (current_node, next_node, distance)) of a dataset, computed once."""
    _, x, k = dataset(name)
    sq_rows = {}
    core = core_by_definition(x, k, sq_rows=sq_rows)
    edges = prim_reference(x, core, sq_rows=sq_rows)
    for a in (core,) + edges:
        a.setflags(write=False)
    return core, edges
