"""The embedding behind --plot on the device (csrc/knn.hip idl_knn_graph, csrc/embed.hip, posthoc.umap_embedding_device) against
tests/umap_ref.py, stage by stage: the kNN graph bit for bit, the calibration to 1e-12, one layout epoch per vertex inside 4 x the
float32 replay's own deviation from the float64 epoch with the schedule decisions exact, the draws equal to numpy's Philox; then
what only a full run can show: the same bits twice, and a picture as good as the float64 reference's."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import umap_ref as R
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

K = 15


@functools.lru_cache(maxsize=None)
def _points(name):
    if name == "n300":
        return R.blobs(300, 4, 11)[0]
    if name == "n1003":
        return R.blobs(1003, 6, 12)[0]
    if name == "far300":
        return R.blobs(300, 4, 13, offset=300.0)[0]
    if name == "dup4099":
        x = R.blobs(4099, 12, 14)[0]
        rng = np.random.default_rng(15)
        order = rng.permutation(4099)
        copies, rest = order[:4099 // 3], order[4099 // 3:]
        x[copies] = x[rng.choice(rest, size=len(copies))]
        return x
    if name == "copies60":                       # one point 60 times: more ties than the matrix route's first shortlist (k + 32) holds
        x = R.blobs(300, 4, 11)[0].copy()
        x[100:160] = x[5]
        return x
    if name == "copies600":                      # one point 600 times: more than a row of the window route can keep (KNN_GRAPH_CAP)
        x = R.blobs(1003, 6, 12)[0].copy()
        x[np.random.default_rng(17).permutation(1003)[:600]] = x[7]
        return x
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref_graph(name, k):
    return R.knn_graph(_points(name), k)


def _same_graph(got, want, what):
    for g, w, field in zip(got, want, ("idx", "dist")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, field, g.dtype, g.shape)
        same = g == w
        if not same.all():
            i = int(np.argmin(same.all(1)))
            pytest.fail(f"{what}: {field} differs in {int((~same.all(1)).sum())} of {len(w)} rows, first row {i}: device {got[0][i].tolist()} "
                        f"{got[1][i].tolist()}, reference {want[0][i].tolist()} {want[1][i].tolist()}")


# ---------------------------------------------------------------- the kNN graph
@pytest.mark.parametrize("route", ["matrix", "window"])
@pytest.mark.parametrize("name,k", [("n300", K), ("n1003", K), ("dup4099", K), ("n300", 2), ("n300", 64), ("far300", K), ("copies60", K), ("copies600", K)])
def test_knn_graph_bit_for_bit(name, k, route, monkeypatch):
    from idelucs_amd import posthoc
    monkeypatch.setitem(posthoc.OPTIONS, "knn", route)
    stats = {}
    got = posthoc.knn_graph_device(_points(name), k, stats=stats)
    assert stats["graph_path"] == route
    if route == "window":
        print(name, k, {s: stats.get(s) for s in ("graph_cap", "graph_missed", "graph_status_counts", "graph_kept_max", "matrix_widened")})
        if name == "copies600":
            # a row whose k nearest include the copied point keeps all its copies, more than KNN_GRAPH_CAP columns (status 2), and goes
            # through the matrix route: the copies' own rows and whatever rows reach the clump; every other row is idl_knn_graph's
            clump = np.all(_points(name) == _points(name)[7], axis=1)
            reach = int(clump[_ref_graph(name, k)[0]].any(1).sum())
            assert clump.sum() > posthoc.KNN_GRAPH_CAP and reach >= clump.sum()
            assert stats["graph_status_counts"] == [1003 - reach, 0, reach, 0, 0, 0]
        else:
            # hi's margin covers the pass's delta by construction (status 3 cannot occur), the k-th distance is exact (nor 5), and no row
            # of these inputs keeps more than KNN_GRAPH_CAP columns: idl_knn_graph does every row
            assert stats["graph_missed"] == 0 and stats["graph_kept_max"] <= posthoc.KNN_GRAPH_CAP
    elif name in ("copies60", "copies600"):
        assert stats["matrix_widened"] >= 60, "the first shortlist cannot have been closed for the copies' rows"
    _same_graph(got, _ref_graph(name, k), f"{name} k={k} {route}")


def test_knn_graph_default_route_and_dtypes():
    from idelucs_amd import posthoc
    stats = {}
    idx, dist = posthoc.knn_graph_device(_points("n300").astype(np.float64), K, stats=stats)
    assert stats["graph_path"] == "matrix" and idx.dtype == np.int32 and dist.dtype == np.float64
    _same_graph((idx, dist), _ref_graph("n300", K), "default route")


@pytest.mark.parametrize("route", ["matrix", "window"])
def test_knn_graph_writes_inside_its_outputs(route):
    import torch
    from idelucs_amd import posthoc
    x = _points("n300")
    dev = torch.device("cuda", torch.cuda.current_device())
    n, g = len(x), 4096
    ibuf = torch.full((n * K + 2 * g,), -77, dtype=torch.int32, device=dev)
    dbuf = torch.full((n * K + 2 * g,), -77.0, dtype=torch.float64, device=dev)
    idx, dist = ibuf[g:g + n * K].view(n, K), dbuf[g:g + n * K].view(n, K)
    x64 = torch.from_numpy(x).to(dev).double()
    if route == "window":
        core = torch.from_numpy(_ref_graph("n300", K)[1][:, -1].copy()).to(dev)
        todo = posthoc._knn_graph_window(x64, K, core, dev, idx, dist)
        posthoc._knn_graph_rows(x64, todo, K, dev, idx, dist)
    else:
        posthoc._knn_graph_rows(x64, None, K, dev, idx, dist)
    _same_graph((idx.cpu().numpy(), dist.cpu().numpy()), _ref_graph("n300", K), route)
    for buf in (ibuf, dbuf):
        assert bool((buf[:g] == -77).all()) and bool((buf[g + n * K:] == -77).all()), "a guard word was overwritten"


def test_knn_graph_refuses_on_the_host(monkeypatch):
    from idelucs_amd import posthoc
    x = _points("n300")
    for k in (1, 0, 301):
        with pytest.raises(ValueError):
            posthoc.knn_graph_device(x, k)
    monkeypatch.setitem(posthoc.OPTIONS, "knn", "window")
    with pytest.raises(ValueError):
        posthoc.knn_graph_device(x[:, :32], K)
    with pytest.raises(ValueError):
        posthoc.knn_graph_device(x, 301)
    with pytest.raises(ValueError):
        posthoc.knn_graph_device(x, 1)


# ---------------------------------------------------------------- calibration and union
def _crafted_rows():
    """blobs600's graph with two rows replaced: row 0 has no positive distance, row 1 has all 14 neighbours at one distance."""
    _, _, idx, dist, _ = R.graph("blobs600")
    idx, dist = idx.copy(), dist.copy()
    dist[0] = 0.0
    dist[1, 1:] = 7.25
    return idx, dist


@pytest.mark.parametrize("case", ["blobs600", "crafted", "n17", "doubled400"])
def test_calibration_matches_the_reference(case):
    from idelucs_amd import posthoc
    if case == "crafted":
        idx, dist = _crafted_rows()
    elif case == "n17":
        idx, dist = R.knn_graph(R.blobs(17, 2, 16)[0], K)
    else:
        idx, dist = R.graph(case)[2:4]
    rho, sigma, w = (t.cpu().numpy() for t in posthoc.umap_smooth_knn_device(idx, dist))
    rho_r, sigma_r, w_r = R.smooth_knn(idx, dist)
    assert np.array_equal(rho, rho_r)
    assert np.all(np.abs(sigma - sigma_r) <= 1e-12 * sigma_r), np.abs(sigma / sigma_r - 1).max()
    assert np.all(np.abs(w - w_r) <= 1e-12 * w_r), np.abs(w - w_r).max()
    if case == "crafted":
        assert rho[0] == 0.0 and abs(sigma[0] / (1e-3 * dist.mean()) - 1.0) < 1e-12                 # no positive distance: the floor of all rows' mean
        assert rho[1] == 7.25 and abs(sigma[1] / (1e-3 * dist[1].mean()) - 1.0) < 1e-12 and np.all(w[1, 1:] == 1.0)   # sigma lands on the row's floor


@pytest.mark.parametrize("case", ["blobs600", "n17", "doubled400"])
def test_union_matches_the_reference(case):
    import torch
    from idelucs_amd import posthoc
    idx, dist = R.knn_graph(R.blobs(17, 2, 16)[0], K) if case == "n17" else R.graph(case)[2:4]
    dev = torch.device("cuda", torch.cuda.current_device())
    idx_t = torch.from_numpy(idx).to(dev)
    w = posthoc.umap_smooth_knn_device(idx_t, dist)[2]
    indptr, indices, p = (t.cpu().numpy() for t in posthoc.umap_fuzzy_union_device(idx_t, w, 500))
    indptr_r, indices_r, p_r = R.fuzzy_union(idx, R.smooth_knn(idx, dist)[2], 500)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32
    assert np.array_equal(indptr, indptr_r) and np.array_equal(indices, indices_r)
    assert np.all(np.abs(p - p_r) <= 1e-12 * p_r)
    import scipy.sparse as sp
    m = sp.csr_matrix((p, indices, indptr), shape=(len(idx), len(idx)))
    t = m.T.tocsr(); t.sort_indices()
    assert np.array_equal(t.data.view(np.uint64), m.data.view(np.uint64)), "P_jk and P_kj are not the same bits"


# ---------------------------------------------------------------- the start
@pytest.mark.parametrize("n", [17, 600, 100003])
def test_jitter_is_the_restatements(n):
    import torch
    from idelucs_amd import _lib
    for seed in (42, (7 << 32) | 3):
        y = torch.zeros((n + 8, 2), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib.idl_umap_jitter(ctypes.c_void_p(y.data_ptr()), n, 1e-4, seed, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = y.cpu().numpy()
        want = R.jitter(n, seed)
        assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)) and np.all(got[n:] == 0.0)
        assert np.abs(want).max() <= 1e-4 and (n < 600 or np.abs(want).max() > 0.9e-4)
    base = np.random.default_rng(1).normal(size=(n, 2)).astype(np.float32) * 10
    y = torch.from_numpy(base).cuda()
    _lib.check(_lib.lib.idl_umap_jitter(ctypes.c_void_p(y.data_ptr()), n, 1e-4, 42, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(y.cpu().numpy(), base + R.jitter(n, 42))


@pytest.mark.parametrize("name", ["blobs600", "doubled400"])
def test_pca_start_is_the_restatements(name):
    """Two float64 covariances and eigensolvers agree to ~1e-13; rounded to float32 at a largest |coordinate| of 10 that is the same
    number or, at a rounding boundary, its neighbour (one ulp at 10 is 9.5e-7): 1e-6 of the scale."""
    import torch
    from idelucs_amd import posthoc
    x = R.graph(name)[0]
    for seed in (42, 1):
        got = posthoc.umap_pca_start_device(torch.from_numpy(x).cuda().double(), seed).cpu().numpy()
        want = R.pca_start(x, seed)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-6 * 10.0, np.abs(got - want).max()
        assert abs(np.abs(got).max() - 10.0) < 2e-4


# ---------------------------------------------------------------- one epoch
def _csr(case):
    """(n, indptr, indices, p) of the layout cases: blobs600's union; the same with vertex 7 cut out (degree 0); a 17-point graph."""
    if case == "n17":
        idx, dist = R.knn_graph(R.blobs(17, 2, 16)[0], K)
        return (17,) + R.fuzzy_union(idx, R.smooth_knn(idx, dist)[2], 500)
    indptr, indices, p = R.graph("blobs600")[4]
    if case == "degree0":
        owner = np.repeat(np.arange(600), np.diff(indptr))
        keep = (owner != 7) & (indices != 7)
        indices, p, owner = indices[keep], p[keep], owner[keep]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=600))]).astype(np.int64)
        assert indptr[8] == indptr[7]
    return (600, indptr, indices, p)


def _device_epoch(y0, indptr, indices, p, nxt, nneg, ep, a, b, seed):
    import torch
    from idelucs_amd import posthoc
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    y, (eps, nxt2, nneg2) = posthoc.umap_layout_device(t(y0), t(indptr), t(indices), t(p), 500, a, b, seed, first_epoch=ep, last_epoch=ep,
                                                       state=(t(nxt), t(nneg)))
    return y.cpu().numpy(), eps.cpu().numpy(), nxt2.cpu().numpy(), nneg2.cpu().numpy()


@pytest.mark.parametrize("case,ep", [("blobs600", 1), ("blobs600", 2), ("blobs600", 250), ("degree0", 1), ("degree0", 2), ("n17", 1), ("n17", 2)])
def test_one_epoch_against_float64(case, ep):
    seed = 42
    a, b = R.ab_params()
    n, indptr, indices, p = _csr(case)
    assert case != "blobs600" or np.diff(indptr).max() > 8, "no row longer than the lane group"
    if case == "blobs600":
        y0, eps, nxt, nneg = R.state_before("blobs600", seed, ep)
    else:
        y0 = R.pca_start(R.blobs(n, 2, 16)[0] if case == "n17" else R.graph("blobs600")[0], seed)
        y0, (eps, nxt, nneg) = R.run(y0, indptr, indices, p, 500, a, b, seed, last_epoch=ep - 1)
        y0 = y0.astype(np.float32)
    args = (y0, indptr, indices, eps, nxt, nneg, ep, 500, a, b, seed)
    y64, nxt_r, nneg_r, info = R.epoch(*args)
    y32 = R.epoch(*args, dtype=np.float32)[0]
    y_gpu, eps_g, nxt_g, nneg_g = _device_epoch(y0, indptr, indices, p, nxt, nneg, ep, a, b, seed)
    assert np.array_equal(eps_g, eps)
    assert np.array_equal(nxt_g, nxt_r) and np.array_equal(nneg_g, nneg_r), "the schedule decisions differ"
    replay, gpu = R.deviation(y32, y64, info, y0), R.deviation(y_gpu, y64, info, y0)
    print(f"{case} epoch {ep}: {len(info['fired'])} entries fired, float32 replay deviates by {replay.max():.3e}, the GPU by {gpu.max():.3e} "
          f"(bar {4 * replay.max():.3e})")
    assert len(info["fired"]) > 0 and replay.max() > 0
    assert np.all(gpu <= 4.0 * replay.max()), int(np.argmax(gpu))
    if case == "degree0":
        assert np.array_equal(y_gpu[7], y0[7])


@pytest.mark.parametrize("n,entry0", [(600, 0), (17, 12190), (1000000, (1 << 32) + 5), ((1 << 31) - 1, 21999990)])
def test_draws_are_numpy_philox(n, entry0):
    import torch
    from idelucs_amd import _lib
    count, n_draws, ep = 300, 9, 250
    for seed in (42, (7 << 32) | 3):
        out = torch.full((count * n_draws + 64,), -5, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib.idl_umap_draws(seed, entry0, count, ep, n_draws, n, ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = out.cpu().numpy()
        assert np.all(got[count * n_draws:] == -5)
        want = R.draws(seed, np.arange(entry0, entry0 + count), ep, n_draws, n)
        assert np.array_equal(got[:count * n_draws].reshape(count, n_draws), want)
        assert want.min() >= 0 and want.max() < n


# ---------------------------------------------------------------- full runs
@functools.lru_cache(maxsize=None)
def _gpu_embedding(name, seed):
    from idelucs_amd import posthoc
    return posthoc.umap_embedding_device(R.graph(name)[0], n_neighbors=K, n_epochs=500, seed=seed)


def test_same_seed_same_bits():
    from idelucs_amd import posthoc
    x = R.graph("blobs600")[0]
    first = _gpu_embedding("blobs600", 42)
    again = posthoc.umap_embedding_device(x, n_neighbors=K, n_epochs=500, seed=42)
    assert first.shape == (600, 2) and first.dtype == np.float64
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))
    assert not np.array_equal(first, _gpu_embedding("blobs600", 1))


@pytest.mark.parametrize("name", ["blobs600", "doubled400"])
def test_quality_of_the_full_run(name):
    from sklearn.manifold import trustworthiness
    x, lab = R.graph(name)[:2]
    t_pca = trustworthiness(x, R.pca2(x), n_neighbors=K)
    t_gpu, t_ref = [], []
    for seed in R.SEEDS:
        y = _gpu_embedding(name, seed)
        assert np.all(np.isfinite(y))
        t_gpu.append(trustworthiness(x, y, n_neighbors=K))
        t_ref.append(trustworthiness(x, R.embedding(name, seed), n_neighbors=K))
        assert t_gpu[-1] > t_pca, (seed, t_gpu[-1], t_pca)
        assert R.purity(y, lab) == 1.0, (seed, R.purity(y, lab))
    print(f"{name}: trustworthiness GPU {np.round(t_gpu, 4).tolist()}, float64 reference {np.round(t_ref, 4).tolist()}, PCA-2 {t_pca:.4f}; "
          f"largest |coordinate| {max(np.abs(_gpu_embedding(name, s)).max() for s in R.SEEDS):.2f}")
    assert np.mean(t_gpu) >= np.mean(t_ref) - 3.0 * (max(t_ref) - min(t_ref))


def test_too_few_points_is_a_value_error():
    from idelucs_amd import posthoc
    with pytest.raises(ValueError):
        posthoc.umap_embedding_device(R.blobs(15, 2, 1)[0], n_neighbors=15)
    assert posthoc.umap_embedding_device(R.blobs(17, 2, 16)[0], n_neighbors=15, n_epochs=20).shape == (17, 2)


# ---------------------------------------------------------------- the CLI
CHILD = r"""
import os, sys, types
import numpy as np
mode = sys.argv[1]
if mode == "absent":
    sys.modules["umap"] = None                    # `import umap` raises ImportError
else:
    stub = types.ModuleType("umap")
    class UMAP:
        def __init__(self, **kw):
            self.kw = kw
        def fit_transform(self, latent):
            open("umap_stub_called.txt", "w").write(repr(self.kw) + " " + repr(np.asarray(latent).shape))
            return np.random.default_rng(0).normal(size=(len(latent), 2))
    stub.UMAP = UMAP
    sys.modules["umap"] = stub
from idelucs_amd import posthoc
calls = []
inner = posthoc.umap_embedding_device
posthoc.umap_embedding_device = lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1]
from idelucs_amd.__main__ import main
out = main(sys.argv[2:])
open("embedding_calls.txt", "w").write(str(len(calls)))
print("OUT_DIR", out)
"""


@pytest.mark.parametrize("mode", ["absent", "stub"])
def test_cli_writes_the_picture(tmp_path, mode):
    import subprocess
    from PIL import Image
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-c", CHILD, mode, "--sequence_file", os.path.join(DATA, "Influenza-A.fas"), "--GT_file", os.path.join(DATA, "Influenza-A_GT.tsv"),
           "--plot", "True", "--n_clusters", "5", "--n_epochs", "2", "--n_voters", "1", "--batch_sz", "256"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = [d for d in (tmp_path / "Results" / "Influenza-A").iterdir()]
    assert len(res) == 1
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg", "contingency_matrix.tsv", "contingency_matrix.jpg", "learned_representation.jpg"):
        assert (res[0] / f).exists(), f
    assert "skipping the plot" not in r.stdout
    img = np.asarray(Image.open(res[0] / "learned_representation.jpg").convert("L"), dtype=np.float64)
    assert img.shape[0] >= 400 and img.shape[1] >= 400 and img.std() > 5.0 and (img < 128).mean() > 0.002, "an empty picture"
    assert (tmp_path / "embedding_calls.txt").read_text() == ("1" if mode == "absent" else "0")
    assert (tmp_path / "umap_stub_called.txt").exists() == (mode == "stub")
    if mode == "stub":
        assert "random_state" in (tmp_path / "umap_stub_called.txt").read_text() and "(949, 64)" in (tmp_path / "umap_stub_called.txt").read_text()
