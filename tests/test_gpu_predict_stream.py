"""GPU tests of the streamed predict inputs: the chunked statistics kernels against the materialised float64 route (bit for bit, wherever
the chunks are cut), utils.predict_feature_chunks against utils.predict_features, and IID_model's streamed predict (memory, values,
routing, row shards)."""
import copy
import functools
import os

import numpy as np
import pytest

import stats_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                # guard words on either side of every output buffer
FILL = -12345


def _sequences(n, seed, kind="random"):
    """'random': 50..3000 bases, skewed composition, every fifth record with a run of N, record 3 = 70 000 x A (one large count);
    'sparse': every record 500 bases of A / C only -- equal row totals, and the k-mers with a G or T never occur (constant columns)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    for i in range(n):
        if kind == "sparse":
            s = rng.choice(acgt[:2], size=500)
        elif i == 3:
            s = np.full(70000, ord("A"), np.uint8)
        else:
            L = int(rng.integers(50, 3001))
            s = rng.choice(acgt, size=L, p=[0.4, 0.1, 0.2, 0.3])
            if i % 5 == 0:
                s[L // 2: L // 2 + 1 + L // 20] = ord("N")
        recs.append(b">r%d\n" % i + s.tobytes() + b"\n")
    return b"".join(recs)


@functools.lru_cache(maxsize=None)
def _fasta(n, seed, kind):
    import atexit
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="idl_stream_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, f"{kind}_{n}_{seed}.fas")
    with open(path, "wb") as h:
        h.write(_sequences(n, seed, kind))
    return path


@functools.lru_cache(maxsize=2)
def _reference(k, n, kind):
    """the materialised route, once per case: int32 counts, float64 rows -> idl_col_stats -> idl_standardise"""
    import torch
    from idelucs_amd import _lib, utils as U
    ff = U.FastaFile(_fasta(n, 10 * k + n, kind), check=True)
    din = U._DeviceInput(ff, torch.device("cuda"))
    counts = U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_COUNTS_I32)[0]
    f64 = U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_FREQ_F64)[0]
    mean, scale = U.col_stats(f64)
    want = U.standardise(f64, mean, scale)
    del f64
    ff.close()
    return counts, counts.long().sum(1).int(), mean, scale, want


def _guarded(n, dtype, dev):
    import torch
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n:] == FILL).all())


CASES = [(8, 600, "random", 1), (8, 600, "random", 64), (8, 600, "random", 600), (8, 600, "random", 1000),
         (8, 600, "sparse", 64), (9, 300, "random", 150), (9, 300, "random", 37), (4, 1000, "random", 333), (4, 1000, "random", 7)]


@pytest.mark.parametrize("k,n,kind,chunk", CASES)
def test_chunked_kernels_equal_the_float64_route(k, n, kind, chunk):
    """idl_row_totals_i32 + idl_counts_stream_stats per chunk + idl_counts_stream_finish give idl_col_stats' mean and scale of the float64
    rows bit for bit, and idl_counts_standardise per chunk gives idl_standardise's rows, for chunks of any length (64 straddles the
    row-block boundary at row 200 of 600; 1000 exceeds the matrix); nothing is written outside the output buffers."""
    import torch
    from idelucs_amd import _lib, utils as U
    L = _lib.lib
    counts, tot_want, mean_want, scale_want, want = _reference(k, n, kind)
    dev = counts.device
    f = counts.shape[1]
    assert f == 4 ** k and counts.shape[0] == n
    if kind == "sparse":
        assert int((scale_want == 1.0).sum()) >= f // 2           # the constant columns: scale 1
    else:
        assert int(counts[3, 0]) > 60000
    ws_bytes = int(L.idl_counts_stream_workspace(n, f))
    assert ws_bytes == (2 * R.stat_row_blocks(n) + 1) * f * 8
    ws_buf, ws = _guarded(ws_bytes // 8, torch.float64, dev)
    tot_buf, tot = _guarded(n, torch.int32, dev)
    mean_buf, mean = _guarded(f, torch.float64, dev)
    scale_buf, scale = _guarded(f, torch.float64, dev)
    cr = min(chunk, n)
    y_buf, y = _guarded(cr * f, torch.float32, dev)
    sp = U._stream_ptr()
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        _lib.check(L.idl_row_totals_i32(U._ptr(counts[lo:hi]), hi - lo, f, U._ptr(tot[lo:hi]), sp))
        _lib.check(L.idl_counts_stream_stats(U._ptr(counts[lo:hi]), U._ptr(tot[lo:hi]), lo, hi - lo, n, f, U._ptr(ws), sp))
    _lib.check(L.idl_counts_stream_finish(n, f, U._ptr(ws), U._ptr(mean), U._ptr(scale), sp))
    assert torch.equal(tot, tot_want)
    assert torch.equal(mean, mean_want), (mean - mean_want).abs().max().item()
    assert torch.equal(scale, scale_want), (scale - scale_want).abs().max().item()
    same = torch.ones((), dtype=torch.bool, device=dev)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        y.fill_(FILL)
        _lib.check(L.idl_counts_standardise(U._ptr(counts[lo:hi]), U._ptr(tot[lo:hi]), hi - lo, f, U._ptr(mean), U._ptr(scale), U._ptr(y), sp))
        m = (hi - lo) * f
        same &= (y[:m].view(torch.int32) == want[lo:hi].reshape(-1).view(torch.int32)).all() & (y[m:] == FILL).all()
    assert bool(same)
    for buf, size in ((ws_buf, ws_bytes // 8), (tot_buf, n), (mean_buf, f), (scale_buf, f), (y_buf, cr * f)):
        assert _intact(buf, size)
    # a chunk outside the matrix is refused before anything is launched
    assert L.idl_counts_stream_stats(U._ptr(counts), U._ptr(tot), n - 1, 2, n, f, U._ptr(ws), sp) == _lib.IDL_ERR_ARG
    assert L.idl_row_totals_i32(U._ptr(counts), 1, f + 2, U._ptr(tot), sp) == _lib.IDL_ERR_ARG


@pytest.mark.parametrize("k,reduce", [(6, False), (8, False), (6, True), (8, True)])
def test_predict_feature_chunks_equal_predict_features(k, reduce):
    """the generator's chunks, put together, are utils.predict_features' float32 matrix bit for bit: all rows, an empty range, a range
    that begins and ends inside chunks; plain and canonical rows"""
    import torch
    from idelucs_amd import utils as U
    n = 600
    path = _fasta(n, 5, "random")
    want = U.predict_features(path, k=k, reduce=reduce, with_names=False)[2]
    f = want.shape[1]

    def gather(**kw):
        parts, at = [], None
        for lo, hi, x in U.predict_feature_chunks(path, k=k, reduce=reduce, **kw):
            assert x.dtype == torch.float32 and tuple(x.shape) == (hi - lo, f) and (at is None or lo == at)
            parts.append((lo, hi, x.clone()))                    # (x is the generator's one buffer)
            at = hi
        return parts
    for chunk_rows in (None, 64, 37):
        parts = gather(chunk_rows=chunk_rows)
        assert parts[0][0] == 0 and parts[-1][1] == n
        assert len(parts) == (1 if chunk_rows is None else -(-n // chunk_rows))
        assert torch.equal(torch.cat([p[2] for p in parts]), want), (k, reduce, chunk_rows)
    assert gather(rows=(123, 123), chunk_rows=64) == []
    parts = gather(rows=(100, 333), chunk_rows=64)
    assert [(p[0], p[1]) for p in parts] == [(100, 128), (128, 192), (192, 256), (256, 320), (320, 333)]      # the whole file's cuts
    assert torch.equal(torch.cat([p[2] for p in parts]), want[100:333])
    for lo, hi, buf, at in U.predict_feature_chunks(path, k=k, reduce=reduce, rows=(100, 333), chunk_rows=64, padded=True):
        assert tuple(buf.shape) == (64, f) and at == lo % 64 and torch.equal(buf[at:at + hi - lo], want[lo:hi])
        assert bool(torch.isfinite(buf).all())
    with pytest.raises(ValueError):
        gather(rows=(10, n + 1))


# ------------------------------------------------------------------------------------------------ the model
N_MODEL, K_MODEL, CHUNK_MODEL, CLUSTERS = 600, 8, 32, 5


class _Recorder:
    """libidelucs_hip with the name of every call noted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


NEW_ENTRIES = {"idl_row_totals_i32", "idl_counts_stream_workspace", "idl_counts_stream_stats", "idl_counts_stream_finish"}


@pytest.fixture(scope="module")
def model_case():
    """a k = 8 NetLinear on 600 sequences, its predict inputs (the bit-identical ones of the test above) and the float64 CPU forward of
    its weights on them: computed once, read by the tests below"""
    import torch
    import idelucs_amd
    from idelucs_amd import utils as U
    path = _fasta(N_MODEL, 5, "random")
    model = idelucs_amd.IID_model({'sequence_file': path, 'GT_file': None, 'n_clusters': CLUSTERS, 'k': K_MODEL, 'model_size': 'linear',
                                   'n_mimics': 3, 'batch_sz': 64, 'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25,
                                   'scheduler': None, 'n_epochs': 1, 'n_voters': 1, 'predict_chunk_rows': CHUNK_MODEL})
    model.build_dataloader()
    x = U.predict_features(path, k=K_MODEL, with_names=False)[2]
    net64 = copy.deepcopy(model.net).double().cpu().eval()
    with torch.no_grad():
        probs64, latent64 = net64(x.double().cpu())
    del x
    return model, probs64.numpy(), latent64.numpy()


def _streamed(model, monkeypatch, rows=None):
    from idelucs_amd import utils as U
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "1")
    return model._predict_outputs(rows)


def test_streamed_predict_values(model_case, monkeypatch):
    """latent and probabilities of the streamed route against the float64 forward: its largest error is at most twice the resident
    route's on the same case (both are fp32 GEMMs; the kernel may differ with the row count), and the labels agree wherever float64
    separates the two best clusters by more than 1e-3"""
    from idelucs_amd import utils as U
    model, probs64, latent64 = model_case
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "0")
    o_res, l_res = (t.double().cpu().numpy() for t in model._predict_outputs())
    o_str, l_str = (t.double().cpu().numpy() for t in _streamed(model, monkeypatch))
    assert o_str.shape == (N_MODEL, CLUSTERS) and l_str.shape == (N_MODEL, 64)
    err = {name: (np.abs(l - latent64).max(), np.abs(o - probs64).max()) for name, (o, l) in (("resident", (o_res, l_res)), ("streamed", (o_str, l_str)))}
    print(f"largest |error| against float64 (latent, probabilities): resident {err['resident'][0]:.3e} {err['resident'][1]:.3e}, "
          f"streamed {err['streamed'][0]:.3e} {err['streamed'][1]:.3e}; |latent| up to {np.abs(latent64).max():.3e}")
    top2 = np.sort(probs64, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-3
    print(f"rows whose float64 top-two gap exceeds 1e-3: {int(clear.sum())} of {N_MODEL}")
    assert clear.mean() >= 0.9
    assert np.array_equal(o_str.argmax(1)[clear], probs64.argmax(1)[clear])
    assert err["streamed"][0] <= 2 * err["resident"][0] and err["streamed"][1] <= 2 * err["resident"][1], err
    # predict() and calculate_probs() are the same outputs
    y, p, lat = model.predict()
    assert np.array_equal(y, o_str.argmax(1)) and np.array_equal(lat, l_str) and np.array_equal(p, o_str.max(1))
    assert np.array_equal(model.calculate_probs(), o_str)


def test_streamed_predict_memory(model_case, monkeypatch):
    """predict on the streamed route allocates a chunk's buffers, the statistics and the outputs -- not the matrix"""
    import torch
    from idelucs_amd import utils as U
    model, _, _ = model_case
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "1")
    n, f = N_MODEL, 4 ** K_MODEL
    with torch.no_grad():          # (what the first GEMM of a process allocates for good -- the BLAS workspace -- is not predict's)
        model.net.eval()
        model.net(torch.zeros((CHUNK_MODEL, f), device=model.device))
    ff = U.FastaFile(model.sequence_file, check=True)
    packed = int(((ff.lengths + 63) // 64).sum()) * 24
    ff.close()
    allowed = (CHUNK_MODEL * f * 4 + CHUNK_MODEL * f * 4 + 2 * R.stat_row_blocks(n) * f * 8 + n * 4 + packed
               + 2 * n * (CLUSTERS + 64) * 4)
    assert 12 * n * f >= 4 * allowed                   # materialising the rows cannot meet the bound
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    model.predict()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"streamed predict: peak {peak / 2 ** 20:.2f} MiB above the level before, bound {1.25 * allowed / 2 ** 20:.2f} MiB, "
          f"materialised rows {12 * n * f / 2 ** 20:.0f} MiB")
    assert peak <= 1.25 * allowed


def test_predict_routing(model_case, monkeypatch):
    """beyond PREDICT_CACHE_BYTES the streamed route is taken and nothing is cached; with the default line this model calls no new entry"""
    from idelucs_amd import models, utils as U
    model, _, _ = model_case
    assert U.OPTIONS["predict_stream"] == ""
    rec = _Recorder(U._L)
    monkeypatch.setattr(U, "_L", rec)
    model._shared.clear()
    out_default = model._predict_outputs()[1]
    assert not NEW_ENTRIES & set(rec.calls) and "idl_col_stats" in rec.calls
    assert model._shared.get("predict_inputs") is not None
    model._shared.clear()
    del rec.calls[:]
    monkeypatch.setattr(models, "PREDICT_CACHE_BYTES", N_MODEL * 4 ** K_MODEL * 4 - 1)
    out_streamed = model._predict_outputs()[1]
    assert NEW_ENTRIES <= set(rec.calls) and "idl_col_stats" not in rec.calls and "idl_standardise" not in rec.calls
    assert rec.calls.count("idl_counts_standardise") == -(-N_MODEL // CHUNK_MODEL)
    assert model._shared.get("predict_inputs") is None
    assert out_streamed.shape == out_default.shape
    del rec.calls[:]
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "0")              # the dev key overrides the size
    model._predict_outputs()
    assert not NEW_ENTRIES & set(rec.calls)


def test_streamed_latent_shard(model_case, monkeypatch):
    import torch
    model, _, _ = model_case
    full = _streamed(model, monkeypatch)[1].float()
    for lo, hi in ((0, 600), (17, 403), (590, 600), (64, 96)):
        assert torch.equal(model.predict_latent_shard(lo, hi), full[lo:hi]), (lo, hi)
    assert model.predict_latent_shard(5, 5).shape == (0, 64)
    assert tuple(model._predict_outputs((7, 7))[1].shape) == (0, 64)
