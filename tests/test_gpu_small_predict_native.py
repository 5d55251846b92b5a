"""small_predict='native' on the GPU: layer 1 (idl_small_predict_l1, and idl_small_l1_fwd for as long as both are in the tree) followed by
idl_small_predict_mid (csrc/small_predict.hip) against tests/small_predict_ref.py, row by row on its own, and up through IID_model, a saved
ensemble's assign and the CLI.

  exact      small-integer operands: lat is the float64 value BIT FOR BIT (every partial sum is exact, so a mismatch is a wrong index: the message
             names row, column and tile); with negative pre-activations of layer 2 and a one-hot instance head, lat = fl32(fl32(0.01) v) + bi;
             operands in NaN-framed buffers, outputs between sentinel guards;
  random     Kaiming weights, standard-normal rows (with the planted direction): lat and z within the a-priori bars (operation counts; nothing
             fitted), prob == z[unit] bitwise, unit == the reference's outside the margin set (at most 2 % of the rows), lowest class on planted ties;
  rows       a row's outputs do not depend on m, its place, or the other rows (NaN / inf rows included); z = NULL writes nothing;
  model      IID_model(small_predict='native'): types, shards, routes and chunk sizes agree bit for bit; the torch path of the same weights within
             the bars;  assign: a fine-mode run returns its training labels and probabilities bit for bit;  CLI: --small_predict native end to end.
Every test prints what it measured (pytest -s).  Seen on MI355X, as shares of the bars, on either layer-1 launch: random cases lat <= 1.7e-4,
z <= 1.3e-3, no row in the margin set; Influenza-A (2 epochs) lat 5.3e-4 and z 1.9e-4 at k = 4, 5.6e-5 and 1.6e-5 at k = 6, the torch path's latent
within 2.4e-4 of two bars; every bit-for-bit comparison with 0 entries differing; the fine-mode run had no two records with the same latent."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import small_predict_ref as R
from conftest import DATA

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
SENT32 = -777
GUARD = 4096              # guard elements on either side of an output
PAD_ROWS = 8              # NaN rows in front of and behind an operand
FASTA = os.path.join(DATA, "Influenza-A.fas")
ROUTES = ("idl_small_predict_l1", "idl_small_l1_fwd")


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _framed(a, dev):
    """Operand a (fp32 vector or matrix) inside a buffer that is NaN everywhere else: PAD_ROWS rows of its width in front and behind ->
    (the buffer: keep it alive, pointer to the operand's first element; 16-byte aligned for every width that is a multiple of 4 or every vector)."""
    import torch
    a2 = np.atleast_2d(np.asarray(a, np.float32))
    rows, ld = a2.shape
    pad = PAD_ROWS if ld % 4 == 0 else 4 * PAD_ROWS          # (PAD_ROWS * ld * 4 bytes in front: a multiple of 16 either way)
    big = np.full((rows + 2 * pad, ld), np.float32("nan"), np.float32)
    big[pad:pad + rows] = a2
    t = torch.from_numpy(big).to(dev)
    return t, ctypes.c_void_p(t.data_ptr() + pad * ld * 4)


def _guarded(shape, dev, int32=False):
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT32 if int32 else SENTINEL, dtype=torch.int32 if int32 else torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _intact(buf, view):
    s = SENTINEL if buf.is_floating_point() else SENT32
    return bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + view.numel():] == s).all())


def _untouched(buf):
    return bool((buf == (SENTINEL if buf.is_floating_point() else SENT32)).all())


def _launch(o, dev, route=ROUTES[0], want_z=True):
    """Layer 1 by `route` + idl_small_predict_mid on framed operands and guarded outputs -> dict(lat, z, prob, unit, a1: device tensors; intact:
    every guard (and with want_z = False the whole z buffer) still holds its sentinel)."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    m, F = o["x"].shape
    C = o["Wc"].shape[0]
    keep, ptr = {}, {}
    for name in ("x",) + R.NAMES:
        keep[name], ptr[name] = _framed(o[name], dev)
    bufs = {"a1": _guarded((m, R.H1), dev), "lat": _guarded((m, R.LAT), dev), "z": _guarded((m, C), dev), "prob": _guarded((m,), dev),
            "unit": _guarded((m,), dev, int32=True)}
    _lib.check(getattr(L, route)(ptr["x"], ptr["W1"], m, F, _p(bufs["a1"][1]), _stream()))
    _lib.check(L.idl_small_predict_mid(_p(bufs["a1"][1]), *(ptr[name] for name in R.NAMES[1:]), m, C, _p(bufs["lat"][1]),
                                       _p(bufs["z"][1]) if want_z else None, _p(bufs["prob"][1]), _p(bufs["unit"][1]), _stream()))
    torch.cuda.synchronize()
    out = {name: view for name, (_, view) in bufs.items()}
    out["intact"] = all(_intact(*bufs[name]) for name in bufs if want_z or name != "z") and (want_z or _untouched(bufs["z"][0]))
    return out


def _check_top(out):
    """prob is z[unit] and the largest z of its row, bit for bit, and unit the lowest class that attains it."""
    import torch
    z = out["z"]
    assert torch.equal(out["prob"], z.max(1)[0])
    assert torch.equal(out["prob"], z.gather(1, out["unit"].long()[:, None])[:, 0])
    C = z.shape[1]
    index = torch.arange(C, device=z.device, dtype=torch.int32)[None, :].expand_as(z)
    first = torch.where(z == out["prob"][:, None], index, torch.full_like(index, C)).min(1)[0]
    assert torch.equal(out["unit"], first)


# ---------------------------------------------------------------- 1. exact operands

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("m,F,C", R.EXACT_CASES, ids=str)
def test_exact_operands_give_the_float64_latent_bit_for_bit(dev, m, F, C, route):
    """F' = 136 and 2080: the tail stages; m = 1, 15, 17, 33: ragged tiles; C = 16 | 17 and 64 | 65: a logits tile and a lane group; 131 072: k = 9."""
    o = R.exact_operands(m, F, C)
    r, b = R.reference("exact", (m, F, C))
    out = _launch(o, dev, route)
    assert out["intact"], "a guard region around an output was written"
    msg = R.first_mismatch(out["lat"].cpu().numpy(), r["lat"])
    assert msg is None, f"{route} + idl_small_predict_mid m={m} F={F} C={C}, lat: {msg}"
    over = R.over_bar(out["z"].cpu().numpy(), r["z"], b["z"])
    print(f"\n  exact m={m} F={F} C={C} ({route}): lat equal; z's largest error over its bar {over:.3g}")
    assert over <= 1.0
    _check_top(out)
    skip = R.margin_rows(r["z"], b["z"])
    assert np.array_equal(out["unit"].cpu().numpy()[~skip], r["unit"][~skip])


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("m,F,C", R.NEGATIVE_CASES, ids=str)
def test_negative_pre_activations_take_the_slope_once(dev, m, F, C, route):
    o = R.exact_operands(m, F, C, negative=True)
    want = R.negative_latent32(o)
    out = _launch(o, dev, route)
    assert out["intact"]
    got = out["lat"].cpu().numpy()
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{int(bad.sum())} entries of lat differ from fl32(fl32(0.01) v) + bi; first at {tuple(np.argwhere(bad)[0])}"
    _check_top(out)


# ---------------------------------------------------------------- 2. random operands

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("m,F,C,wc", R.RANDOM_CASES, ids=str)
def test_random_operands_stay_within_the_a_priori_bars(dev, m, F, C, wc, route):
    import torch
    o = R.random_operands(m, F, C, wc)
    r, b = R.reference("random", (m, F, C, wc))
    out = _launch(o, dev, route)
    assert out["intact"], "a guard region around an output was written"
    over_lat = R.over_bar(out["lat"].cpu().numpy(), r["lat"], b["lat"])
    over_z = R.over_bar(out["z"].cpu().numpy(), r["z"], b["z"])
    skip = R.margin_rows(r["z"], b["z"])
    print(f"\n  random m={m} F={F} C={C} Wc x {wc} ({route}): largest error over its bar: lat {over_lat:.3g}, z {over_z:.3g}; rows skipped by the "
          f"argmax check: {int(skip.sum())} of {m}")
    assert over_lat <= 1.0 and over_z <= 1.0
    _check_top(out)
    assert skip.mean() <= R.MARGIN_CAP
    assert np.array_equal(out["unit"].cpu().numpy()[~skip], r["unit"][~skip])
    bare = _launch(o, dev, route, want_z=False)
    assert bare["intact"], "z = NULL: the z buffer or a guard region was written"
    for name in ("lat", "prob", "unit"):
        assert torch.equal(bare[name], out[name]), name


def test_the_lowest_class_wins_a_planted_tie(dev):
    o = R.random_operands(*R.RANDOM_CASES[1])                      # C = 200
    Wc = np.array(o["Wc"]); bc = np.array(o["bc"])
    twins = [(4, 5), (2, 70), (129, 199)]                          # neighbouring lanes, two slots of different lanes, the last class
    for lo, hi in twins:
        Wc[hi], bc[hi] = Wc[lo], bc[lo]
    tied = dict(o, Wc=Wc, bc=bc)
    r = R.forward64(**tied)
    out = _launch(tied, dev)
    _check_top(out)
    unit = out["unit"].cpu().numpy()
    for lo, hi in twins:
        assert bool((out["z"][:, lo] == out["z"][:, hi]).all()) and hi not in unit
    assert sum(int(((unit == lo) & (r["unit"] == lo)).sum()) for lo, _ in twins) > 0, "no row's largest z sits on a planted tie"


def test_z_has_the_bits_of_the_training_steps_eval_middle(dev):
    """idl_small_mid_fwd(train = 0) runs the same stages on the same tiles: z equal bit for bit (its f is the latent normalised: not compared)."""
    import torch
    from idelucs_amd import _lib
    m, F, C, wc = R.RANDOM_CASES[1]
    o = R.random_operands(m, F, C, wc)
    out = _launch(o, dev)
    w = {name: torch.from_numpy(np.array(o[name])).to(dev) for name in R.NAMES}
    a1 = out["a1"].clone()
    ctl = torch.zeros(4, dtype=torch.int64, device=dev)
    a2, d2 = torch.empty((m, R.H2), device=dev), torch.empty((m, R.H2), device=dev)
    f, inv, z = torch.empty((m, R.LAT), device=dev), torch.empty(m, device=dev), torch.empty((m, C), device=dev)
    _lib.check(_lib.lib.idl_small_mid_fwd(_p(a1), *(_p(w[name]) for name in R.NAMES[1:]), m, C, 0, ctypes.c_uint64(3), _p(ctl), _p(a2), _p(d2), _p(f),
                                          _p(inv), _p(z), _stream()))
    torch.cuda.synchronize()
    print(f"\n  z differing from idl_small_mid_fwd(train = 0)'s in {int((z != out['z']).sum())} entries")
    assert torch.equal(z, out["z"])


# ---------------------------------------------------------------- 3. rows alone

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n,F,C", R.ROWS_ALONE, ids=str)
def test_a_rows_outputs_depend_on_that_row_alone(dev, n, F, C, route):
    import torch
    o = R.random_operands(n, F, C, 1.0)
    full = _launch(o, dev, route)
    assert full["intact"] and bool(torch.isfinite(full["lat"]).all())
    names = ("lat", "z", "prob", "unit")
    # a. alone: m = 1
    for i in (0, 15, 16, 39):
        one = _launch(dict(o, x=o["x"][i:i + 1]), dev, route)
        assert one["intact"]
        for name in names:
            assert torch.equal(one[name][0], full[name][i]), f"{name}: row {i} alone (m = 1) against the block of {n}"
    # b. at another place, in a block of 150 (two workgroups of layer 1) whose other rows are NaN, +inf and -inf
    place = np.random.default_rng(7).permutation(150)[:n]
    xb = np.full((150, F), np.float32("nan"), np.float32)
    xb[1::3] = np.float32("inf")
    xb[2::3] = -np.float32("inf")
    xb[place] = o["x"]
    b = _launch(dict(o, x=xb), dev, route)
    assert b["intact"]
    sel = torch.from_numpy(place).to(dev)
    for name in names:
        assert torch.equal(b[name][sel], full[name]), f"{name}: scattered among NaN / inf rows against the block of {n}"
    # c. z = NULL
    bare = _launch(o, dev, route, want_z=False)
    assert bare["intact"], "z = NULL: the z buffer or a guard region was written"
    for name in ("lat", "prob", "unit"):
        assert torch.equal(bare[name], full[name]), name


def test_the_predictor_blocks_and_reads_the_weights_in_place(dev, monkeypatch):
    import torch
    from idelucs_amd import predict_native as P
    from idelucs_amd.PytorchUtils import myNet
    n, F, C = R.ROWS_ALONE[0]
    o = R.random_operands(n, F, C, 1.0)
    full = _launch(o, dev)
    net = myNet(F, C).to(dev)
    pars = (net.layers[0].weight, net.layers[0].bias, net.layers[3].weight, net.layers[3].bias, net.instance.weight, net.instance.bias,
            net.classifier[1].weight, net.classifier[1].bias)
    with torch.no_grad():
        for p, name in zip(pars, R.NAMES):
            p.copy_(torch.from_numpy(np.array(o[name])))
    pred = P.NativeSmallPredictor(net)
    x = torch.from_numpy(np.array(o["x"])).to(dev)
    lat, prob, unit, z = pred.forward(x, want_z=True)
    assert lat.shape == (n, 64) and z.shape == (n, C) and prob.shape == unit.shape == (n,) and unit.dtype == torch.int32
    for name, got in (("lat", lat), ("z", z), ("prob", prob), ("unit", unit)):
        assert torch.equal(got, full[name]), name
    lat2, prob2, unit2, z2 = pred.forward(x)
    assert z2 is None and torch.equal(lat2, lat) and torch.equal(prob2, prob) and torch.equal(unit2, unit)
    scratch = pred._a1.data_ptr()
    pred.forward(x[:7])
    assert pred._a1.data_ptr() == scratch
    monkeypatch.setattr(P, "MAX_BLOCK_ROWS", 17)                   # three blocks: 17, 17, 6 rows
    lat3, prob3, unit3, z3 = pred.forward(x, want_z=True)
    assert torch.equal(lat3, lat) and torch.equal(z3, z) and torch.equal(prob3, prob) and torch.equal(unit3, unit)
    with torch.no_grad():
        net.instance.bias.add_(1.0)
    moved = pred.forward(x)[0]
    assert not torch.equal(moved, lat) and float((moved - lat - 1.0).abs().max()) < 1e-3
    assert pred.forward(x[:0])[0].shape == (0, 64)


# ---------------------------------------------------------------- 4. model level

def _model(k, small_predict, chunk_rows=None, **more):
    import idelucs_amd
    args = {'sequence_file': FASTA, 'GT_file': None, 'n_clusters': 5, 'k': k, 'model_size': 'small', 'n_mimics': 3, 'batch_sz': 256,
            'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 2, 'n_voters': 1,
            'predict_chunk_rows': chunk_rows}
    if small_predict is not None:
        args['small_predict'] = small_predict
    args.update(more)
    return idelucs_amd.IID_model(args)


def _weights(net):
    return [t.detach().cpu().numpy() for t in (net.layers[0].weight, net.layers[0].bias, net.layers[3].weight, net.layers[3].bias, net.instance.weight,
                                               net.instance.bias, net.classifier[1].weight, net.classifier[1].bias)]


@pytest.mark.parametrize("k,step", [(4, "native"), (6, None)], ids=["k4-small_step-native", "k6-autograd"])
def test_model_predict_is_typed_as_before_and_agrees_with_itself(dev, monkeypatch, k, step):
    import torch
    from idelucs_amd import utils as U
    model = _model(k, 'native', 64, **({'small_step': step} if step else {}))
    model.build_dataloader()
    model.begin_voter(0)
    for _ in range(2):
        model.contrastive_training_epoch()
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "0")
    y, p, lat = model.predict()
    assert (y.dtype, p.dtype, lat.dtype) == (np.int64, np.float64, np.float64) and y.shape == p.shape == (949,) and lat.shape == (949, 64)
    probs = model.calculate_probs()
    assert probs.dtype == np.float64 and probs.shape == (949, 5)
    assert np.array_equal(y, probs.argmax(1)) and np.array_equal(p, probs.max(1))
    full = torch.from_numpy(lat).float().to(dev)
    assert np.array_equal(full.double().cpu().numpy(), lat)          # float32 values, widened

    def shards(what):
        for lo, hi in ((0, 949), (0, 311), (311, 700), (700, 949), (37, 37)):
            got = model.predict_latent_shard(lo, hi)
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (hi - lo, 64)
            assert torch.equal(got, full[lo:hi]), f"{what}: rows [{lo}, {hi}) differ from the full latent"

    shards("resident route")
    monkeypatch.setitem(U.OPTIONS, "predict_stream", "1")
    for chunk in (64, 160):
        monkeypatch.setattr(model, "predict_chunk_rows", chunk)
        y2, p2, lat2 = model.predict()
        assert np.array_equal(y2, y) and np.array_equal(p2, p) and np.array_equal(lat2, lat), f"streamed route, chunk {chunk}"
        assert np.array_equal(model.calculate_probs(), probs)
        shards(f"streamed route, chunk {chunk}")
    # within the bars of the float64 forward of the model's own weights on its own inputs; the torch path of the same weights likewise, so the two
    # are at most two bars apart; argmax equal outside the margin rows
    x = U.predict_features(FASTA, k=k, reduce=True, device=dev, with_names=False)[2]
    w = _weights(model.net)
    r = R.forward64(x.cpu().numpy(), *w)
    b = R.bars(x.cpu().numpy(), *w, ref=r)
    over_lat, over_z = R.over_bar(lat, r["lat"], b["lat"]), R.over_bar(probs, r["z"], b["z"])
    with torch.no_grad():
        model.net.eval()
        z_t, lat_t = model.net(x)
    apart = R.over_bar(lat_t.double().cpu().numpy(), lat, 2.0 * b["lat"])
    skip = R.margin_rows(r["z"], b["z"])
    y_t = torch.max(z_t, 1)[1].cpu().numpy()
    print(f"\n  Influenza-A, small, k = {k}, 2 epochs: largest error over its bar: lat {over_lat:.3g}, z {over_z:.3g}; the torch path's latent over "
          f"two bars: {apart:.3g}; rows in the margin set {int(skip.sum())}, argmax differing outside it {int((y_t != y)[~skip].sum())}")
    assert over_lat <= 1.0 and over_z <= 1.0 and apart <= 1.0
    assert np.array_equal(y_t[~skip], y[~skip]) and np.array_equal(y[~skip], r["unit"][~skip])


def test_without_the_key_the_model_takes_todays_path(dev, monkeypatch):
    from idelucs_amd import predict_native

    def refuse(*a, **k):
        raise AssertionError("a native predictor was built without its key")

    monkeypatch.setattr(predict_native, "NativeLinearPredictor", refuse)
    monkeypatch.setattr(predict_native, "NativeSmallPredictor", refuse)
    for value in (None, 'torch'):
        model = _model(4, value)
        assert model._native_predict is False and model._small_native_predict is False
    model.build_dataloader()
    model.begin_voter(0)
    model.contrastive_training_epoch()
    y, p, lat = model.predict()
    assert model._predictor is None and y.shape == (949,) and lat.shape == (949, 64)
    out = model._predict_outputs()
    assert len(out) == 2 and tuple(out[0].shape) == (949, 5) and tuple(out[1].shape) == (949, 64)
    lane = _model(4, 'native').lane()
    assert lane._small_native_predict is True and lane._native_predict is True          # the lanes of training.train_voters inherit the key


# ---------------------------------------------------------------- 5. assign, the CLI

def _cli(tmp, argv):
    from idelucs_amd.__main__ import main
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        return main(argv)
    finally:
        os.chdir(cwd)


def test_a_fine_mode_run_gets_its_own_labels_back_bit_for_bit(dev, tmp_path):
    import pandas as pd
    import torch
    from idelucs_amd.ensemble import FittedEnsemble
    out_dir = _cli(str(tmp_path), ["--sequence_file", FASTA, "--k", "4", "--batch_sz", "256", "--n_epochs", "2", "--n_clusters", "0", "--n_voters", "2",
                                   "--model_size", "small", "--small_predict", "native", "--save_model", str(tmp_path / "model")])
    t = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", float_precision="round_trip")
    y_run, p_run = t["assignment"].to_numpy().astype(np.int64), t["confidence_score"].to_numpy().astype(np.float64)
    ens = FittedEnsemble.load(str(tmp_path / "model"))
    assert ens.mode == "fine" and ens.version == 1 and ens.n_units == 200 and ens.model_size == "small"
    payload = torch.load(os.path.join(str(tmp_path / "model"), "ensemble.pt"), map_location="cpu", weights_only=True)
    assert not any("predict" in key for key in payload)                       # the file has no new field
    for chunk in (100, 37):
        _, units, lat = ens.voter_outputs(FASTA, dev, chunk_rows=chunk, small_predict='native')
        assert torch.equal(lat.cpu(), ens.latent), f"chunk_rows={chunk}: {int((lat.cpu() != ens.latent).any(1).sum())} rows of the latent differ from the run's"
    # every record finds itself (or a lower-index record with exactly its latent) at distance 0
    _, first, inv = np.unique(ens.latent.numpy(), axis=0, return_index=True, return_inverse=True)
    first = first[np.asarray(inv).reshape(-1)]
    dup = first != np.arange(949)
    # (the same records under another file name: ./Results/<stem>/<time stamp to the second> of the run above may still be this second's)
    again = str(tmp_path / "the_same_records.fas")
    shutil.copyfile(FASTA, again)
    out_b = _cli(str(tmp_path), ["--assign", again, "--model", str(tmp_path / "model"), "--small_predict", "native"])
    tb = pd.read_csv(os.path.join(out_b, "assignments.tsv"), sep="\t", float_precision="round_trip")
    y, conf = tb["assignment"].to_numpy().astype(np.int64), tb["confidence_score"].to_numpy().astype(np.float64)
    print(f"\n  fine mode, small: clusters {len(set(y_run.tolist()) - {0})}, exact-duplicate latents {int(dup.sum())}; labels differing from the run's "
          f"{int((y != y_run).sum())}, probabilities {int((conf != p_run).sum())}")
    assert list(tb["sequence_id"].astype(str)) == list(t["sequence_id"].astype(str))
    assert np.array_equal(y, y_run[first]) and np.array_equal(conf, p_run[first])
    assert np.array_equal(y[~dup], y_run[~dup]) and np.array_equal(conf[~dup], p_run[~dup])


def test_cli_end_to_end_with_native_small_predict(dev, tmp_path):
    import pandas as pd
    common = ["--sequence_file", FASTA, "--GT_file", os.path.join(DATA, "Influenza-A_GT.tsv"), "--n_clusters", "5", "--n_epochs", "2", "--n_voters", "2",
              "--batch_sz", "512", "--k", "4", "--model_size", "small"]
    out_dir = _cli(str(tmp_path), common + ["--small_predict", "native"])
    for f in ("assignments.tsv", "metrics.tsv", "training_plots.jpg", "contingency_matrix.jpg", "contingency_matrix.tsv"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    df = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", index_col=0)
    assert list(df.columns) == ["sequence_id", "assignment", "confidence_score"] and len(df) == 949
    table = pd.read_csv(tmp_path / "ALL_RESULTS.tsv", sep="\t")
    assert len(table) == 1 and "'small_predict': 'native'" in table["Parameters"][0]
    plain = tmp_path / "plain"
    plain.mkdir()
    _cli(str(plain), common)
    table = pd.read_csv(plain / "ALL_RESULTS.tsv", sep="\t")
    assert len(table) == 1 and "predict" not in table["Parameters"][0]
