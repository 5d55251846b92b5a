"""predict='native' on the GPU: idl_l1_fwd followed by idl_predict_mid (csrc/predict.hip) against tests/predict_ref.py, against the training
step's own middle launch, row by row on its own, and up through IID_model, a saved ensemble's assign and the CLI.

  exact      small-integer operands: lat is the float64 value BIT FOR BIT (every partial sum is exact, so a mismatch is a wrong index: the message
             names row, column and tile); operands in NaN-framed buffers, outputs between sentinel guards;
  random     Kaiming weights, standard-normal rows (with predict_ref's planted direction): lat and z within the a-priori bars of predict_ref
             (operation counts; nothing fitted), prob == max z, unit == the reference's outside the margin set (at most 2 % of the rows);
  training   z and max(lat, 0) bit-equal to idl_mid_fwd_gather(train = 0, a1_transposed = 1);
  rows       a row's outputs do not depend on the batch, its place in it, or the other rows;
  model      IID_model(predict='native'): types, shards, routes and chunk sizes agree bit for bit;  assign: a fine-mode run returns its training
             labels and probabilities bit for bit at another chunk size;  CLI: --predict native end to end.
Every test prints what it measured (pytest -s).  Seen on MI355X, as shares of the bars: exact cases z <= 1.4e-5; random cases lat <= 5.3e-4,
z <= 4.3e-4, no row in the margin set; Influenza-A (k = 4, 2 epochs) lat 9.2e-4, z 7.4e-5; every bit-for-bit comparison with 0 entries differing."""
import ctypes
import os

import numpy as np
import pytest

import predict_ref as R
from conftest import DATA

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
SENT32 = -777
GUARD = 4096              # guard elements on either side of an output
PAD_ROWS = 8              # NaN rows in front of and behind an operand
FASTA = os.path.join(DATA, "Influenza-A.fas")
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _L():
    from idelucs_amd import _lib
    return _lib, _lib.lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _framed(a, dev):
    """Operand a (fp32 vector or matrix) inside a buffer that is NaN everywhere else: PAD_ROWS rows of its width in front and behind ->
    (the buffer: keep it alive, pointer to the operand's first element)."""
    import torch
    a2 = np.atleast_2d(np.asarray(a, np.float32))
    rows, ld = a2.shape
    big = np.full((rows + 2 * PAD_ROWS, ld), np.float32("nan"), np.float32)
    big[PAD_ROWS:PAD_ROWS + rows] = a2
    t = torch.from_numpy(big).to(dev)
    return t, ctypes.c_void_p(t.data_ptr() + PAD_ROWS * ld * 4)


def _guarded(shape, dev, int32=False):
    """An output of `shape` between two guard regions, everything the sentinel -> (whole buffer, the output's view)."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT32 if int32 else SENTINEL, dtype=torch.int32 if int32 else torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _intact(buf, view):
    s = SENTINEL if buf.is_floating_point() else SENT32
    return bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + view.numel():] == s).all())


def _untouched(buf):
    return bool((buf == (SENTINEL if buf.is_floating_point() else SENT32)).all())


def _launch(o, dev, want_z=True):
    """idl_l1_fwd + idl_predict_mid on framed operands and guarded outputs -> dict(lat, z, prob, unit, a1_t: device tensors; intact: every guard (and
    with want_z = False the whole z buffer) still holds its sentinel)."""
    import torch
    _lib, L = _L()
    m, F = o["x"].shape
    C = o["W3"].shape[0]
    assert L.idl_l1_fwd_supported(m, R.H1, F) == 1
    keep, ptr = {}, {}
    for name in ("x",) + NAMES:
        keep[name], ptr[name] = _framed(o[name], dev)
    bufs = {"a1_t": _guarded((R.H1, m), dev), "lat": _guarded((m, R.H2), dev), "z": _guarded((m, C), dev), "prob": _guarded((m,), dev),
            "unit": _guarded((m,), dev, int32=True)}
    _lib.check(L.idl_l1_fwd(ptr["W1"], ptr["x"], m, F, _p(bufs["a1_t"][1]), _stream()))
    _lib.check(L.idl_predict_mid(_p(bufs["a1_t"][1]), ptr["b1"], ptr["W2"], ptr["b2"], ptr["W3"], ptr["b3"], m, C, _p(bufs["lat"][1]),
                                 _p(bufs["z"][1]) if want_z else None, _p(bufs["prob"][1]), _p(bufs["unit"][1]), _stream()))
    torch.cuda.synchronize()
    out = {name: view for name, (_, view) in bufs.items()}
    out["intact"] = all(_intact(*bufs[name]) for name in bufs if want_z or name != "z") and (want_z or _untouched(bufs["z"][0]))
    return out


def _check_top(out):
    """prob is the largest z of its row, bit for bit, and unit the lowest index that attains it."""
    import torch
    z = out["z"]
    assert torch.equal(out["prob"], z.max(1)[0])
    C = z.shape[1]
    index = torch.arange(C, device=z.device, dtype=torch.int32)[None, :].expand_as(z)
    first = torch.where(z == out["prob"][:, None], index, torch.full_like(index, C)).min(1)[0]
    assert torch.equal(out["unit"], first)


# ---------------------------------------------------------------- 1. exact operands

@pytest.mark.parametrize("m,F,C", R.EXACT_CASES, ids=str)
def test_exact_operands_give_the_float64_latent_bit_for_bit(dev, m, F, C):
    """F = 192: layer 1's ring exactly full; 65 536: the widest row idl_l1_fwd is asked for (k = 8); C = 64 | 65: the last lane of a class slot and the
    first of the next; 256: every slot full; m = 96: six workgroups."""
    o = R.exact_operands(m, F, C)
    r, b = R.reference("exact", (m, F, C))
    out = _launch(o, dev)
    assert out["intact"], "a guard region around an output was written"
    msg = R.first_mismatch(out["lat"].cpu().numpy(), r["lat"])
    assert msg is None, f"idl_l1_fwd + idl_predict_mid m={m} F={F} C={C}, lat: {msg}"
    over = R.over_bar(out["z"].cpu().numpy(), r["z"], b["z"])
    print(f"\n  exact m={m} F={F} C={C}: lat equal; z's largest error over its bar {over:.3g}")
    assert over <= 1.0
    _check_top(out)
    skip = R.margin_rows(r["z"], b["z"])
    assert np.array_equal(out["unit"].cpu().numpy()[~skip], r["unit"][~skip])


# ---------------------------------------------------------------- 2. random operands

@pytest.mark.parametrize("m,F,C,w3", R.RANDOM_CASES, ids=str)
def test_random_operands_stay_within_the_a_priori_bars(dev, m, F, C, w3):
    """The bars are predict_ref's (operation counts; worst case, so a correct kernel sits far inside them: at most 5.3e-4 of lat's and 4.3e-4 of z's on
    MI355X, where a lost K chunk, bias or K slice is beyond 1: test_predict_reference.py).  The last case has logits beyond 100: exp overflows there
    unless the row's largest logit is subtracted."""
    import torch
    o = R.random_operands(m, F, C, w3)
    r, b = R.reference("random", (m, F, C, w3))
    out = _launch(o, dev)
    assert out["intact"], "a guard region around an output was written"
    over_lat = R.over_bar(out["lat"].cpu().numpy(), r["lat"], b["lat"])
    over_z = R.over_bar(out["z"].cpu().numpy(), r["z"], b["z"])
    skip = R.margin_rows(r["z"], b["z"])
    print(f"\n  random m={m} F={F} C={C} W3 x {w3}: largest error over its bar: lat {over_lat:.3g}, z {over_z:.3g}; rows skipped by the argmax check: "
          f"{int(skip.sum())} of {m}")
    assert over_lat <= 1.0 and over_z <= 1.0
    _check_top(out)
    assert skip.mean() <= R.MARGIN_CAP
    assert np.array_equal(out["unit"].cpu().numpy()[~skip], r["unit"][~skip])
    # z = NULL: nothing is written to z, the other outputs have the same bits
    bare = _launch(o, dev, want_z=False)
    assert bare["intact"], "z = NULL: the z buffer or a guard region was written"
    for name in ("lat", "prob", "unit"):
        assert torch.equal(bare[name], out[name]), name


# ---------------------------------------------------------------- 3. against the training step's middle launch

@pytest.mark.parametrize("m", [32, 96])
@pytest.mark.parametrize("C", [5, 200])
def test_z_and_relu_of_lat_are_the_training_kernels_bits(dev, m, C):
    import torch
    _lib, L = _L()
    o = R.random_operands(96, 256, C, 1.0)
    o = dict(o, x=o["x"][:m])
    out = _launch(o, dev)
    w = {name: torch.from_numpy(np.array(o[name])).to(dev) for name in NAMES}
    a1 = out["a1_t"].clone()
    ctl = torch.zeros(4, dtype=torch.int64, device=dev)
    f, r2 = torch.empty((m, 64), device=dev), torch.empty((m, 64), device=dev)
    inv, z = torch.empty(m, device=dev), torch.empty((m, C), device=dev)
    _lib.check(L.idl_mid_fwd_gather(_p(a1), _p(w["b1"]), 1, _p(w["W2"]), _p(w["b2"]), _p(w["W3"]), _p(w["b3"]), m, C, 0, ctypes.c_uint64(3), _p(ctl),
                                    _p(f), _p(inv), _p(r2), _p(z), None, _stream()))
    torch.cuda.synchronize()
    print(f"\n  m={m} C={C}: z differing from idl_mid_fwd_gather's in {int((z != out['z']).sum())} entries, max(lat, 0) from its r2 in "
          f"{int((r2 != out['lat'].clamp_min(0)).sum())}")
    assert torch.equal(z, out["z"])
    assert torch.equal(r2, out["lat"].clamp_min(0))
    assert (r2 > 0).any() and (out["lat"] < 0).any()


# ---------------------------------------------------------------- 4. rows alone

def test_a_rows_outputs_depend_on_that_row_alone(dev):
    import torch
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.predict_native import NativeLinearPredictor
    n, F, C = R.ROWS_ALONE
    o = R.random_operands(n, F, C, 1.0)
    # a. first in a batch of 64, zero rows behind them
    xa = np.zeros((64, F), np.float32)
    xa[:n] = o["x"]
    a = _launch(dict(o, x=xa), dev)
    # b. permuted inside a batch of 96 whose other rows are NaN
    place = np.random.default_rng(7).permutation(96)[:n]
    xb = np.full((96, F), np.float32("nan"), np.float32)
    xb[place] = o["x"]
    b = _launch(dict(o, x=xb), dev)
    # c. through the predictor, n = 40 (one padded block)
    net = NetLinear(F, C).to(dev)
    with torch.no_grad():
        for p, name in zip((net.layers[0].weight, net.layers[0].bias, net.layers[3].weight, net.layers[3].bias, net.classifier[2].weight,
                            net.classifier[2].bias), NAMES):
            p.copy_(torch.from_numpy(np.array(o[name])))
    pred = NativeLinearPredictor(net)
    x = torch.from_numpy(np.array(o["x"])).to(dev)
    lat, prob, unit, z = pred.forward(x, want_z=True)
    c = {"lat": lat, "prob": prob, "unit": unit, "z": z}
    assert lat.shape == (n, 64) and z.shape == (n, C) and prob.shape == unit.shape == (n,) and unit.dtype == torch.int32
    sel = torch.from_numpy(place).to(dev)
    for name in ("lat", "z", "prob", "unit"):
        assert torch.equal(a[name][:n], c[name]), f"{name}: first in a batch of 64 against the predictor"
        assert torch.equal(b[name][sel], c[name]), f"{name}: scattered among NaN rows against the predictor"
    assert bool(torch.isfinite(lat).all()) and len(set(unit.tolist())) == C
    # without z the predictor returns None for it and the same bits otherwise; its scratch is reused; the weights are read in place
    lat2, prob2, unit2, z2 = pred.forward(x)
    assert z2 is None and torch.equal(lat2, lat) and torch.equal(prob2, prob) and torch.equal(unit2, unit)
    scratch = pred._a1_t.data_ptr()
    pred.forward(x[:7])
    assert pred._a1_t.data_ptr() == scratch
    with torch.no_grad():
        net.layers[3].bias.add_(1.0)
    moved = pred.forward(x)[0]
    assert not torch.equal(moved, lat) and float((moved - lat - 1.0).abs().max()) < 1e-3
    assert pred.forward(x[:0])[0].shape == (0, 64)


# ---------------------------------------------------------------- 5. model level

def _model(predict, chunk_rows=None):
    import idelucs_amd
    args = {'sequence_file': FASTA, 'GT_file': None, 'n_clusters': 5, 'k': 4, 'model_size': 'linear', 'n_mimics': 3, 'batch_sz': 256,
            'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 2, 'n_voters': 1,
            'predict_chunk_rows': chunk_rows}
    if predict is not None:
        args['predict'] = predict
    return idelucs_amd.IID_model(args)


@pytest.fixture(scope="module")
def trained(dev):
    model = _model('native', 64)
    model.build_dataloader()
    model.begin_voter(0)
    for _ in range(2):
        model.contrastive_training_epoch()
    return model


def test_model_predict_is_typed_as_before_and_agrees_with_itself(dev, trained, monkeypatch):
    import torch
    from idelucs_amd import utils as U
    model = trained
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "0")
    y, p, lat = model.predict()
    assert (y.dtype, p.dtype, lat.dtype) == (np.int64, np.float64, np.float64) and y.shape == p.shape == (949,) and lat.shape == (949, 64)
    probs = model.calculate_probs()
    assert probs.dtype == np.float64 and probs.shape == (949, 5)
    assert np.array_equal(y, probs.argmax(1)) and np.array_equal(p, probs.max(1))
    full = torch.from_numpy(lat).float().to(dev)
    assert np.array_equal(full.double().cpu().numpy(), lat)          # float32 values, widened

    def shards(what):
        for lo, hi in ((0, 949), (1, 34), (500, 949), (37, 37)):
            got = model.predict_latent_shard(lo, hi)
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (hi - lo, 64)
            assert torch.equal(got, full[lo:hi]), f"{what}: rows [{lo}, {hi}) differ from the full latent"

    shards("resident route")
    # the streamed route (IDELUCS_DEV predict_stream=1; utils.OPTIONS holds the key once the package is imported), at two chunk sizes
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "1")
    for chunk in (64, 160):
        monkeypatch.setattr(model, "predict_chunk_rows", chunk)
        y2, p2, lat2 = model.predict()
        assert np.array_equal(y2, y) and np.array_equal(p2, p) and np.array_equal(lat2, lat), f"streamed route, chunk {chunk}"
        assert np.array_equal(model.calculate_probs(), probs)
        shards(f"streamed route, chunk {chunk}")
    # ... and within the bar of the float64 forward of the model's own weights on its own inputs
    x = U.predict_features(FASTA, k=4, device=dev, with_names=False)[2]
    net = model.net
    w = [t.detach().cpu().numpy() for t in (net.layers[0].weight, net.layers[0].bias, net.layers[3].weight, net.layers[3].bias,
                                            net.classifier[2].weight, net.classifier[2].bias)]
    r = R.forward64(x.cpu().numpy(), *w)
    b = R.bars(x.cpu().numpy(), *w, ref=r)
    over_lat, over_z = R.over_bar(lat, r["lat"], b["lat"]), R.over_bar(probs, r["z"], b["z"])
    print(f"\n  Influenza-A, k = 4, 2 epochs: largest error over its bar: lat {over_lat:.3g}, z {over_z:.3g}")
    assert over_lat <= 1.0 and over_z <= 1.0


def test_without_the_key_the_model_takes_todays_path(dev, monkeypatch):
    from idelucs_amd import predict_native
    model = _model(None)
    assert model._native_predict is False

    def refuse(*a, **k):
        raise AssertionError("the native predictor was built without predict='native'")

    monkeypatch.setattr(predict_native, "NativeLinearPredictor", refuse)
    model.build_dataloader()
    y, p, lat = model.predict()
    assert model._predictor is None and y.shape == (949,) and lat.shape == (949, 64)
    out = model._predict_outputs()
    assert len(out) == 2 and tuple(out[0].shape) == (949, 5) and tuple(out[1].shape) == (949, 64)
    lane = _model('native').lane()
    assert lane._native_predict is True                     # the lanes of training.train_voters inherit the key


# ---------------------------------------------------------------- 6. assign, 7. the CLI

def _cli(tmp, argv):
    from idelucs_amd.__main__ import main
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        return main(argv)
    finally:
        os.chdir(cwd)


def _records(path):
    recs = []
    with open(path) as fh:
        for line in fh:
            if line.startswith(">"):
                recs.append([line])
            elif recs:
                recs[-1].append(line)
    return ["".join(r) if r[-1].endswith("\n") else "".join(r) + "\n" for r in recs]


def test_a_fine_mode_run_gets_its_own_labels_back_bit_for_bit(dev, tmp_path):
    import pandas as pd
    import torch
    from idelucs_amd.ensemble import FittedEnsemble
    out_dir = _cli(str(tmp_path), ["--sequence_file", FASTA, "--k", "4", "--batch_sz", "256", "--n_epochs", "2", "--n_clusters", "0", "--n_voters", "2",
                                   "--predict", "native", "--save_model", str(tmp_path / "model")])
    t = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", float_precision="round_trip")
    y_run, p_run = t["assignment"].to_numpy().astype(np.int64), t["confidence_score"].to_numpy().astype(np.float64)
    ens = FittedEnsemble.load(str(tmp_path / "model"))
    assert ens.mode == "fine" and ens.version == 1 and ens.n_units == 200
    labels, prob = ens.labels.numpy(), ens.prob.numpy()
    assert np.array_equal(labels, y_run) and np.array_equal(prob, p_run)
    # the latent again, at another chunk size than the run's predict used (its default: one chunk for 949 rows of 256)
    for chunk in (100, 37):
        _, units, lat = ens.voter_outputs(FASTA, dev, chunk_rows=chunk, predict='native')
        assert torch.equal(lat.cpu(), ens.latent), f"chunk_rows={chunk}: {int((lat.cpu() != ens.latent).any(1).sum())} rows of the latent differ from the run's"
    # every record finds itself (or a lower-index record with exactly its latent) at distance 0
    _, first, inv = np.unique(ens.latent.numpy(), axis=0, return_index=True, return_inverse=True)
    first = first[np.asarray(inv).reshape(-1)]
    dup = first != np.arange(949)
    names, y, conf = ens.assign(FASTA, dev, predict='native')
    print(f"\n  fine mode: clusters {len(set(labels.tolist()) - {0})}, exact-duplicate latents {int(dup.sum())}; labels differing from the run's "
          f"{int((y != labels[first]).sum())}, probabilities {int((conf != prob[first]).sum())}")
    assert list(names) == list(t["sequence_id"].astype(str))
    assert np.array_equal(y, labels[first]) and np.array_equal(conf, prob[first])
    assert np.array_equal(y[~dup], y_run[~dup]) and np.array_equal(conf[~dup], p_run[~dup])
    # every third record in reverse order
    recs = _records(FASTA)
    rows = np.arange(0, 949, 3)[::-1].copy()
    path_b = str(tmp_path / "subset_B.fas")
    with open(path_b, "w") as fh:
        fh.write("".join(recs[i] for i in rows))
    names_b, y_b, conf_b = ens.assign(path_b, dev, predict='native')
    assert list(names_b) == [names[i] for i in rows]
    assert np.array_equal(y_b, labels[first][rows]) and np.array_equal(conf_b, prob[first][rows])
    # the CLI takes the flag beside --assign
    out_b = _cli(str(tmp_path), ["--assign", path_b, "--model", str(tmp_path / "model"), "--predict", "native"])
    tb = pd.read_csv(os.path.join(out_b, "assignments.tsv"), sep="\t", float_precision="round_trip")
    assert np.array_equal(tb["assignment"].to_numpy().astype(np.int64), y_b) and np.array_equal(tb["confidence_score"].to_numpy().astype(np.float64), conf_b)


def test_cli_end_to_end_with_native_predict(dev, tmp_path):
    import pandas as pd
    out_dir = _cli(str(tmp_path), ["--sequence_file", FASTA, "--GT_file", os.path.join(DATA, "Influenza-A_GT.tsv"), "--n_clusters", "5", "--n_epochs", "2",
                                   "--n_voters", "2", "--batch_sz", "512", "--k", "4", "--predict", "native"])
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg", "contingency_matrix.jpg", "contingency_matrix.tsv"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 949
    table = pd.read_csv(tmp_path / "ALL_RESULTS.tsv", sep="\t")
    assert len(table) == 1 and "'predict': 'native'" in table["Parameters"][0]
