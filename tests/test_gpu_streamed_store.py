"""GPU tests of the streamed feature store: a batch vectorised straight from the packed bases (idl_vectorise_pairs_at) against
FeatureStore.gather_pairs on the resident store, the chunked scaler fit (idl_col_stats_stream*) against idl_col_stats, both bit for bit;
utils.StreamedFeatureStore against the resident store; IID_model trained on either store (the same loss curves and parameters); the peak
memory of a streamed run; the CLI with --store streamed."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
GUARD = 4096              # guard floats on either side of y
INFLUENZA = os.path.join(DATA, "Influenza-A.fas")


def _tmpdir():
    import atexit
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="idl_sstore_")
    atexit.register(shutil.rmtree, d, True)
    return d


def _write(path, seqs):
    with open(path, "wb") as h:
        for i, s in enumerate(seqs):
            h.write(b">r%d\n" % i + s.tobytes() + b"\n")
    return path


def _random_seqs(rng, lengths):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return [rng.choice(acgt, size=int(L), p=[0.35, 0.15, 0.2, 0.3]) for L in lengths]


SHORT, WITH_N, LONG = 37, 38, 39      # records of the 40-record file: 3 bases (< k), runs of N, 25 000 bases


@functools.lru_cache(maxsize=None)
def _file40():
    """37 sequences of 40 .. 3 000 bases, one shorter than any k, one with runs of N, one of 25 000 bases (beyond the slice kernel's
    20 480-base staging chunk and the histogram kernel's 10 240)."""
    rng = np.random.default_rng(40)
    seqs = _random_seqs(rng, np.linspace(40, 3000, 37).astype(int))
    seqs.append(np.frombuffer(b"ACG", np.uint8).copy())
    s = _random_seqs(rng, [1500])[0]
    s[100:140] = ord("N"); s[700:703] = ord("N"); s[1490:] = ord("N")
    seqs.append(s)
    seqs.append(_random_seqs(rng, [25000])[0])
    return _write(os.path.join(_tmpdir(), "file40.fas"), seqs)


@functools.lru_cache(maxsize=None)
def _file6():
    rng = np.random.default_rng(6)
    return _write(os.path.join(_tmpdir(), "file6.fas"), _random_seqs(rng, [60, 333, 1000, 2500, 21000, 700]))


@functools.lru_cache(maxsize=2)
def _both_stores(path, k, n_mimics=3, seed=5):
    """The resident store by the project's existing code (idl_vectorise_ranges / idl_vectorise, idl_col_stats) and a streamed store over the
    SAME device input, edits and scaler -- so a difference in a batch is the new kernel's."""
    import torch
    from idelucs_amd import _lib, utils as U
    dev = torch.device("cuda")
    ff = U.FastaFile(path, check=True)
    din = U._DeviceInput(ff, dev)
    tfs = U.mimic_transforms(n_mimics)
    edits, eo = U._philox_edits(din, [t.spec() for t in tfs], seed)
    feats = U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_FREQ_F32, len(tfs), edits, eo)
    mean, scale = U.col_stats(feats[0])
    res = U.FeatureStore(ff.names, ff.lengths, feats, mean, scale, k, False)
    stre = U.StreamedFeatureStore(ff.names, ff.lengths, din, edits, U._edit_ranges(eo, len(tfs) * din.n), mean, scale, k, len(tfs))
    ff.close()
    return res, stre


def _guarded_y(rows, f, dev):
    import torch
    buf = torch.full((rows * f + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + rows * f].view(rows, f)


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _entry(st, pair_idx, base, base_add, batch, n_pairs, y, inv_scale=True):
    from idelucs_amd import _lib, utils as U
    d = st.din
    _lib.check(_lib.lib.idl_vectorise_pairs_at(U._ptr(d.codes), U._ptr(d.mask), U._ptr(d.slot_off), U._ptr(d.lengths), st.n, st.k, _lib.MODE_KMER,
                                               _lib.INIT_ONE, st.n_views, U._ptr(st.edits), U._ptr(st.edit_ranges), st.max_len, U._ptr(st.mean),
                                               U._ptr(st.scale), U._ptr(st.inv_scale) if inv_scale else None, U._ptr(pair_idx), U._ptr(base), base_add,
                                               batch, n_pairs, U._ptr(y), U._stream_ptr()))


@pytest.mark.parametrize("k", [4, 6, 7, 8])
def test_batch_from_the_packed_bases_has_the_resident_stores_bits(k):
    """16 pairs -- a sequence twice, every view, pair 0, pair n_pairs - 1, the record shorter than k, the one with runs of N, the one of
    25 000 bases -- with base = NULL (either standardisation), with a device base of 5 into a longer list, and with a window that runs past
    n_pairs (those rows keep the sentinel); nothing is written outside y."""
    import torch
    res, st = _both_stores(_file40(), k)
    dev, n, f, P = res.feats.device, res.n, res.f, res.n_pairs
    assert n == 40 and P == 120 and f == 4 ** k and st.max_len == 25000
    assert not torch.equal(res.feats[0], res.feats[1])                  # the views are mutated
    pairs = [0, P - 1, SHORT, n + SHORT, 2 * n + WITH_N, WITH_N, LONG, n + LONG, 2 * n + LONG, 5, n + 5, 2 * n + 5, 5, 17, n + 30, 2 * n + 36]
    idx = torch.tensor(pairs, dtype=torch.int64, device=dev)
    want = res.gather_pairs(idx)
    assert bool(torch.isfinite(want).all())
    for inv in (True, False):
        buf, y = _guarded_y(32, f, dev)
        _entry(st, idx, None, 0, 16, 16, y, inv_scale=inv)
        assert torch.equal(y, want), (k, inv)
        assert _intact(buf, 32 * f)
    assert torch.equal(st.gather_pairs(idx), want)
    # the batch as the two-plane step's fp16 planes, with and without the fp32 rows: the planes idl_split_planes makes of the resident batch
    from idelucs_amd import _lib, utils as U
    wh, wl = torch.empty((32, f), dtype=torch.int16, device=dev), torch.empty((32, f), dtype=torch.int16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib.idl_split_planes(U._ptr(want), want.numel(), int(_lib.lib.idl_planes_exponent(0)), U._ptr(wh), U._ptr(wl), U._ptr(flag), U._stream_ptr()))
    for with_y in (True, False):
        buf, y = _guarded_y(32, f, dev)
        hi, lo = torch.full((32, f), 0x5555, dtype=torch.int16, device=dev), torch.full((32, f), 0x5555, dtype=torch.int16, device=dev)
        got_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        st.pairs_at(idx, None, 0, 16, 16, y if with_y else None, planes=(hi, lo), flag=got_flag)
        assert torch.equal(hi, wh) and torch.equal(lo, wl) and int(got_flag) == int(flag), (k, with_y)
        assert (torch.equal(y, want) if with_y else bool((y == SENTINEL).all())) and _intact(buf, 32 * f)
    # a device base of 5 into the whole (shuffled) pair list
    perm = torch.randperm(P, device=dev, generator=torch.Generator(device=dev).manual_seed(k))
    base = torch.tensor([5], dtype=torch.int64, device=dev)
    buf, y = _guarded_y(32, f, dev)
    _entry(st, perm, base, 0, 16, P, y)
    assert torch.equal(y, res.gather_pairs(perm[5:21])) and _intact(buf, 32 * f)
    buf, y = _guarded_y(32, f, dev)
    _entry(st, perm, base, 3, 16, P, y)                                 # base_add on top of it
    assert torch.equal(y, res.gather_pairs(perm[8:24])) and _intact(buf, 32 * f)
    # the window [5, 21) of a 16-entry list: places 16 .. 20 lie beyond n_pairs, rows 11 .. 15 and 27 .. 31 are left alone
    buf, y = _guarded_y(32, f, dev)
    _entry(st, idx, base, 0, 16, 16, y)
    w = res.gather_pairs(idx[5:16])
    assert torch.equal(y[:11], w[:11]) and torch.equal(y[16:27], w[11:])
    assert bool((y[11:16] == SENTINEL).all()) and bool((y[27:] == SENTINEL).all()) and _intact(buf, 32 * f)


def test_batch_at_k9():
    import torch
    res, st = _both_stores(_file6(), 9)
    dev = res.feats.device
    assert res.n == 6 and res.f == 4 ** 9
    idx = torch.tensor([4, 6 + 4, 17, 0], dtype=torch.int64, device=dev)       # the 21 000-base record twice (two staged chunks), pair n_pairs - 1, pair 0
    buf, y = _guarded_y(8, res.f, dev)
    _entry(st, idx, None, 0, 4, 4, y)
    assert torch.equal(y, res.gather_pairs(idx)) and _intact(buf, 8 * res.f)


def _cuts(n):
    out, lo = [], 0
    for size in (1, 7, 64, 333):
        if lo < n:
            out.append((lo, min(lo + size, n)))
            lo = min(lo + size, n)
    if lo < n:
        out.append((lo, n))
    return out


@pytest.mark.parametrize("n,f", [(1000, 4096), (37, 65536)])
def test_chunked_scaler_fit_is_col_stats_wherever_the_cuts_fall(n, f):
    import torch
    from idelucs_amd import _lib, utils as U
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.rand((n, f), device=dev, generator=g) * torch.rand((1, f), device=dev, generator=g) * 1e-3
    x[:, 5] = 0.25                                          # a constant column
    x[:, 9] = 0.0
    mean_want, scale_want = U.col_stats(x)
    assert float(scale_want[5]) == 1.0 and float(scale_want[9]) == 1.0 and float(mean_want[5]) == 0.25
    L = _lib.lib
    for cuts in (_cuts(n), [(0, n)], [(lo, min(lo + 3, n)) for lo in range(0, n, 3)] if n < 100 else [(0, 500), (500, n)]):
        ws = torch.full((int(L.idl_col_stats_stream_workspace(n, f)) // 8,), float("nan"), dtype=torch.float64, device=dev)
        chunk = torch.empty((max(b - a for a, b in cuts), f), dtype=torch.float32, device=dev)       # ONE buffer, as the store's fit has
        for a, b in cuts:
            chunk[:b - a].copy_(x[a:b])
            _lib.check(L.idl_col_stats_stream(U._ptr(chunk), a, b - a, n, f, U._ptr(ws), U._stream_ptr()))
        mean = torch.empty(f, dtype=torch.float64, device=dev)
        scale = torch.empty(f, dtype=torch.float64, device=dev)
        _lib.check(L.idl_col_stats_stream_finish(n, f, U._ptr(ws), U._ptr(mean), U._ptr(scale), U._stream_ptr()))
        assert torch.equal(mean, mean_want) and torch.equal(scale, scale_want), cuts[:3]


@functools.lru_cache(maxsize=None)
def _influenza_stores():
    from idelucs_amd import utils as U
    res = U.build_feature_store(INFLUENZA, 3, k=6, rng="philox", seed=0)
    st = U.build_feature_store(INFLUENZA, 3, k=6, rng="philox", seed=0, resident=False, chunk_rows=100)
    return res, st


def test_streamed_store_equals_the_resident_store():
    import torch
    from idelucs_amd import utils as U
    res, st = _influenza_stores()
    assert isinstance(st, U.StreamedFeatureStore) and not hasattr(st, "feats") and not st.resident and res.resident
    assert (st.n, st.f, st.n_views, st.n_pairs, st.k) == (res.n, res.f, res.n_views, res.n_pairs, res.k) == (949, 4096, 4, 2847, 6)
    assert list(st.names) == list(res.names) and np.array_equal(st.lengths, res.lengths)
    assert torch.equal(st.mean, res.mean) and torch.equal(st.scale, res.scale) and torch.equal(st.inv_scale, res.inv_scale)
    dev = res.feats.device
    la = iter(U.DeviceBatchLoader(res, 64, generator=torch.Generator(device=dev).manual_seed(1)))
    lb = iter(U.DeviceBatchLoader(st, 64, generator=torch.Generator(device=dev).manual_seed(1)))
    for _ in range(3):
        a, b = next(la), next(lb)
        assert torch.equal(a["true"], b["true"]) and torch.equal(a["modified"], b["modified"])
    with pytest.raises(ValueError, match="rng='philox'"):
        U.build_feature_store(INFLUENZA, 3, k=6, rng="compat", resident=False)


ARGS = {'sequence_file': INFLUENZA, 'GT_file': None, 'n_clusters': 5, 'k': 6, 'model_size': 'linear', 'n_mimics': 3, 'batch_sz': 64,
        'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 3, 'n_voters': 1, 'seed': 0}


def _train(store, epochs=3, **extra):
    import torch
    import idelucs_amd
    model = idelucs_amd.IID_model({**ARGS, **({'store': store} if store else {}), **extra})
    model.build_dataloader()
    model.begin_voter(0)
    curve = [model.contrastive_training_epoch() for _ in range(epochs)]
    torch.cuda.synchronize()
    return model, curve


def test_native_step_on_the_streamed_store_is_the_resident_run(monkeypatch):
    """IDELUCS_PLANES=0: the fp32 tiles on either store -- 44 full batches an epoch (graph capture and replay included) and the partial last
    batch: the same loss curve and the same parameters, bit for bit; predict too."""
    import torch
    monkeypatch.setenv("IDELUCS_PLANES", "0")
    ma, ca = _train(None)
    mb, cb = _train('streamed')
    assert mb._fused is not None and getattr(mb._fused, "n_captures", 0) == 1 and not mb.store.resident
    assert ca == cb and all(np.isfinite(ca)), (ca, cb)
    for (name, pa), pb in zip(ma.net.named_parameters(), mb.net.parameters()):
        assert torch.equal(pa, pb), name
    assert torch.equal(ma._fused.square_avg[0], mb._fused.square_avg[0])
    ya, pa, la = ma.predict()
    yb, pb, lb = mb.predict()
    assert np.array_equal(ya, yb) and np.array_equal(la, lb)


def test_default_step_form_on_the_streamed_store_is_the_resident_run(monkeypatch):
    """The planes on (the default), 2 x 128 rows a batch -- the smallest the two-plane form takes: both stores run that form, the streamed
    store's added launch writing the next batch's planes itself, and the runs are the same bit for bit (graph replay and the partial last
    batch included)."""
    import torch
    from idelucs_amd import fused
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    assert fused.planes_default()
    ma, ca = _train(None, batch_sz=128)
    mb, cb = _train('streamed', batch_sz=128)
    for mdl in (ma, mb):
        assert mdl._fused._form(mdl._fused.buffers(256), mdl.store) == "planes" and not mdl._fused.planes_overflowed()
    assert getattr(mb._fused, "n_captures", 0) == 1
    assert ca == cb and all(np.isfinite(ca)), (ca, cb)
    for (name, pa), pb in zip(ma.net.named_parameters(), mb.net.parameters()):
        assert torch.equal(pa, pb), name


def test_autograd_configurations_train_on_the_streamed_store():
    """DeviceBatchLoader's gather is the store's: SGD through autograd takes the same batches from either store."""
    ma, ca = _train(None, epochs=1, optimizer='SGD')
    mb, cb = _train('streamed', epochs=1, optimizer='SGD')
    assert ca == cb and np.isfinite(ca[0])


def test_streamed_run_stays_below_half_the_resident_feature_buffer():
    """4 096 x 2 kbp, k = 6, 3 mimics: the resident feats alone are 4 x 4096 x 4096 x 4 B = 268 MB.  Build + one epoch + predict of a streamed
    run, fit / predict chunk 256 rows, peak below half of that above the level before."""
    import torch
    import idelucs_amd
    rng = np.random.default_rng(4096)
    path = _write(os.path.join(_tmpdir(), "syn4096.fas"), _random_seqs(rng, [2000] * 4096))
    model = idelucs_amd.IID_model({**ARGS, 'sequence_file': path, 'store': 'streamed', 'predict_chunk_rows': 256, 'n_epochs': 1})
    with torch.no_grad():                               # the GEMM library's workspace belongs to the process, not to the run
        model.net.eval()
        model.net(torch.zeros((256, 4096), device=model.device))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    model.build_dataloader()
    model.begin_voter(0)
    loss = model.contrastive_training_epoch()
    y, p, lat = model.predict()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"streamed run: peak {peak / 1e6:.1f} MB above the level before (resident feats alone: {4 * 4096 * 4096 * 4 / 1e6:.0f} MB)")
    assert np.isfinite(loss) and y.shape == (4096,) and lat.shape == (4096, 64)
    assert peak < 4 * 4096 * 4096 * 4 // 2, peak


def test_cli_with_a_streamed_store(tmp_path, monkeypatch):
    """test_cli_surface's ensemble run (Influenza-A, k = 6, 5 clusters, 5 voters, batch 512) at 10 epochs with --store streamed: the same
    output files, the ensemble ACC accepted as that test accepts its runs (within 0.03 of the reference's worst 5-voter ensemble and of
    the reference's mean, tests/golden/anchor_seeds.json)."""
    import pandas as pd
    from idelucs_amd.__main__ import main
    ref = [r["acc_ensemble"] for r in json.load(open(os.path.join(GOLDEN, "anchor_seeds.json")))["voters5"]]
    monkeypatch.chdir(tmp_path)
    out_dir = main(["--sequence_file", INFLUENZA, "--GT_file", os.path.join(DATA, "Influenza-A_GT.tsv"), "--n_clusters", "5", "--n_epochs", "10",
                    "--n_voters", "5", "--batch_sz", "512", "--k", "6", "--store", "streamed"])
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg", "contingency_matrix.jpg", "contingency_matrix.tsv"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    assert os.path.exists(tmp_path / "ALL_RESULTS.tsv") and "'store': 'streamed'" in open(tmp_path / "ALL_RESULTS.tsv").read()
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 949
    m = pd.read_csv(os.path.join(out_dir, "metrics.tsv"), sep="\t", index_col=0)
    assert {"ACC", "ARI", "NMI", "Silhouette-Score", "Davies-Boulding"} <= set(m.index)
    accs = [float(m.loc["ACC", "Value"])]
    print("5-voter ensemble ACC, streamed store, 10 epochs", np.round(accs, 4), "| reference ensembles", np.round(ref, 4))
    assert len(ref) >= 10 and min(accs) >= min(ref) - 0.03 and abs(np.mean(accs) - np.mean(ref)) <= 0.03, (accs, np.mean(ref))
