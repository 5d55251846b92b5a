"""A trained ensemble kept and applied (idelucs_amd/ensemble.py; --save_model / --assign) on Influenza-A (949 records), k = 6, batch 256,
a handful of epochs.

  scaler       utils.predict_scaler gives the statistics behind predict_features -- checked through the rows: with stats=... the chunked
               inputs of the training file are predict_features' rows, torch.equal; a file B (every third record, in reverse order) under
               the SAVED statistics gives the corresponding training rows, torch.equal -- which fails when the scaler is refitted on B;
  'ensemble'   5 clusters, 3 voters through the CLI with --save_model: assign(training file) returns the run's labels wherever the float64
               margin (second-best minus best squared distance, tests/ensemble_ref.py on the run's votes) exceeds 1e-3 -- the run's own
               k-means works in float32 on distances of order V, rounding about 6e-5 -- with at most 1 % of the records left out; the
               confidence is ensemble_ref's to 1e-9; the saved voters' outputs on the training file are the run's own votes;
  'fine'       --n_clusters 0, 2 voters: assign(training file) gives every record its training label and probability exactly (nearest =
               itself or a lower-index exact duplicate at distance 0); assign(B) gives the labels of B's records;
  round trip   save -> load -> assign equals assign before saving;  CLI: --assign ... --model ... writes those labels.

The references (ensemble_ref, nn_ref) import nothing from the package.  Every test prints what it measured (pytest -s)."""
import os

import numpy as np
import pytest

import ensemble_ref as E
import nn_ref
from conftest import DATA

pytestmark = pytest.mark.gpu

FASTA = os.path.join(DATA, "Influenza-A.fas")
K = 6
COMMON = ["--sequence_file", FASTA, "--k", str(K), "--batch_sz", "256", "--n_epochs", "4"]


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _records(path):
    recs, cur = [], None
    with open(path) as fh:
        for line in fh:
            if line.startswith(">"):
                cur = [line]
                recs.append(cur)
            elif cur is not None:
                cur.append(line)
    return ["".join(r) if r[-1].endswith("\n") else "".join(r) + "\n" for r in recs]


@pytest.fixture(scope="module")
def file_b(tmp_path_factory):
    """(path of B, the training row of every record of B): every third record of the training file, in reverse order."""
    recs = _records(FASTA)
    assert len(recs) == 949
    rows = np.arange(0, len(recs), 3)[::-1].copy()
    path = str(tmp_path_factory.mktemp("b") / "subset_B.fas")
    with open(path, "w") as fh:
        fh.write("".join(recs[i] for i in rows))
    return path, rows


def _rows_of(path, dev, stats, chunk_rows=None):
    """(names, the chunked predict inputs of a file under the given statistics, gathered)."""
    import torch
    from idelucs_amd import ensemble, utils
    din, ff = ensemble._open_input(path, dev)
    try:
        out = [x.clone() for _, _, x in utils.feature_chunks_of_input(din, K, False, None, chunk_rows, stats=stats)]
        torch.cuda.synchronize()
    finally:
        ff.close()
    return ff.names, torch.cat(out)


def _scaler(path, dev, chunk_rows=None):
    from idelucs_amd import ensemble
    mean, scale = ensemble.scaler_of_file(path, K, "linear", dev, chunk_rows)
    return mean.to(dev), scale.to(dev)


@pytest.fixture(scope="module")
def training_rows(dev):
    from idelucs_amd import utils
    names, _, rows = utils.predict_features(FASTA, k=K, device=dev)
    return list(names), rows.clone()


@pytest.mark.parametrize("chunk_rows", [None, 256])
def test_scaler_is_predict_features(dev, training_rows, chunk_rows):
    import torch
    names, want = training_rows
    stats = _scaler(FASTA, dev, chunk_rows)
    assert stats[0].dtype == stats[1].dtype == torch.float64 and stats[0].shape == stats[1].shape == (4 ** K,)
    got_names, got = _rows_of(FASTA, dev, stats, chunk_rows)
    assert list(got_names) == names and got.dtype == torch.float32
    print(f"chunk_rows = {chunk_rows}: rows differing from predict_features = {int((got != want).any(1).sum())} of {len(want)}")
    assert torch.equal(got, want)
    assert torch.equal(_rows_of(FASTA, dev, None, chunk_rows)[1], want)          # without stats: what it did before


def test_new_rows_take_the_saved_statistics(dev, training_rows, file_b):
    import torch
    names, want = training_rows
    path, rows = file_b
    stats = _scaler(FASTA, dev)
    got_names, got = _rows_of(path, dev, stats, 100)
    assert list(got_names) == [names[i] for i in rows]
    sel = want[torch.from_numpy(rows).to(dev)]
    print(f"B: {len(rows)} records, rows differing from the training rows = {int((got != sel).any(1).sum())}")
    assert torch.equal(got, sel)
    refit = _rows_of(path, dev, None)[1]                                         # B's own statistics: other rows
    assert not torch.equal(refit, sel)


def _cli(tmp, extra, votes=None):
    """python -m idelucs_amd in this process, in a directory of its own -> the run's output directory."""
    from idelucs_amd.__main__ import main
    cwd, old = os.getcwd(), os.environ.get("IDELUCS_DUMP_VOTES")
    os.chdir(tmp)
    if votes is not None:
        os.environ["IDELUCS_DUMP_VOTES"] = votes
    try:
        return main(extra)
    finally:
        os.chdir(cwd)
        if votes is not None:
            if old is None:
                del os.environ["IDELUCS_DUMP_VOTES"]
            else:
                os.environ["IDELUCS_DUMP_VOTES"] = old


def _table(out_dir):
    import pandas as pd
    t = pd.read_csv(os.path.join(out_dir, "assignments.tsv"), sep="\t", float_precision="round_trip")   # (the default parser may be an ulp off)
    return list(t["sequence_id"].astype(str)), t["assignment"].to_numpy().astype(np.int64), t["confidence_score"].to_numpy().astype(np.float64)


@pytest.fixture(scope="module")
def ensemble_run(dev, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ens")
    votes = str(tmp / "votes.npy")
    out_dir = _cli(str(tmp), COMMON + ["--n_clusters", "5", "--n_voters", "3", "--save_model", str(tmp / "model")], votes)
    assert os.path.exists(tmp / "model" / "ensemble.pt")
    return dict(tmp=tmp, model=str(tmp / "model"), votes=np.load(votes), table=_table(out_dir))


@pytest.fixture(scope="module")
def fine_run(dev, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fine")
    out_dir = _cli(str(tmp), COMMON + ["--n_clusters", "0", "--n_voters", "2", "--save_model", str(tmp / "model")])
    return dict(tmp=tmp, model=str(tmp / "model"), table=_table(out_dir))


def test_ensemble_mode_returns_the_runs_labels(dev, ensemble_run):
    import torch
    from idelucs_amd.ensemble import FittedEnsemble
    ens = FittedEnsemble.load(ensemble_run["model"])
    votes = ensemble_run["votes"]
    names_run, y_run, _ = ensemble_run["table"]
    assert ens.mode == "ensemble" and len(ens.states) == 3 and tuple(ens.counts.shape) == (5, 3, 5) and votes.shape == (3, 949)
    # the saved voters on the training file: the run's own votes (the same function on bit-equal inputs at the same shape)
    _, units, _ = ens.voter_outputs(FASTA, dev)
    p = torch.gather(ens.unit_maps.to(dev).long(), 1, units).cpu().numpy()
    print(f"votes differing from the run's: {int((p != votes).sum())} of {votes.size}")
    assert np.array_equal(p, votes)
    # the saved tables are the run's votes against its final labels
    counts, cnt = E.tables(votes, y_run, 5)
    assert np.array_equal(ens.counts.numpy(), counts) and np.array_equal(ens.cnt.numpy(), cnt)
    want_y, want_conf, d2 = E.assign(votes, counts, cnt)
    keep = E.margin(d2) > 1e-3
    names, y, conf = ens.assign(FASTA, dev)
    assert list(names) == names_run and y.dtype == np.int64 and conf.dtype == np.float64
    left_out = 1.0 - keep.mean()
    print(f"records left out (margin <= 1e-3): {left_out:.4%}; labels differing from the run's among the rest: {int((y[keep] != y_run[keep]).sum())}; "
          f"from the reference's: {int((y != want_y).sum())}; largest |confidence - reference| = {np.abs(conf - want_conf).max():.3g}")
    assert left_out <= 0.01
    assert np.array_equal(y[keep], y_run[keep])
    assert np.array_equal(y[keep], want_y[keep])
    assert np.abs(conf - want_conf).max() <= 1e-9


def _first_copy(lat):
    """For every row the lowest index of a row with exactly its coordinates."""
    _, first, inv = np.unique(lat, axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inv).reshape(-1)]


def test_fine_mode_gives_training_records_their_own(dev, fine_run, file_b):
    from idelucs_amd.ensemble import FittedEnsemble
    ens = FittedEnsemble.load(fine_run["model"])
    names_run, y_run, p_run = fine_run["table"]
    lat, labels, prob = ens.latent.numpy(), ens.labels.numpy(), ens.prob.numpy()
    assert ens.mode == "fine" and len(ens.states) == 1 and lat.shape == (949, 64) and ens.n_units == 200
    print(f"saved against the run's table: labels differing = {int((labels != y_run).sum())}, probabilities differing = {int((prob != p_run).sum())}, "
          f"largest difference = {np.abs(prob - p_run).max():.3g}")
    assert np.array_equal(labels, y_run) and np.array_equal(prob, p_run)          # what the run wrote
    # spacing: every training point's distance to its nearest other one, against the float64 reference
    want_sp = np.sqrt(nn_ref.nearest(lat, lat, self0=0)[1])
    assert np.array_equal(ens.spacing.numpy(), want_sp)
    first = _first_copy(lat)
    dup = first != np.arange(len(lat))
    agree = bool((labels[dup] == labels[first[dup]]).all())
    print(f"clusters: {len(set(labels.tolist()) - {0})}, unclustered records: {int((labels == 0).sum())}, exact-duplicate latents: {int(dup.sum())}, "
          f"carrying their first copy's label: {agree}")
    names, y, conf = ens.assign(FASTA, dev)
    assert list(names) == names_run
    print(f"training file: labels differing = {int((y != labels[first]).sum())}, probabilities differing = {int((conf != prob[first]).sum())}")
    assert np.array_equal(y, labels[first]) and np.array_equal(conf, prob[first])
    if agree:
        assert np.array_equal(y, y_run)
    path, rows = file_b
    names_b, y_b, conf_b = ens.assign(path, dev)
    assert list(names_b) == [names_run[i] for i in rows]
    print(f"B: labels differing from its records' = {int((y_b != labels[first][rows]).sum())} of {len(rows)}")
    assert np.array_equal(y_b, labels[first][rows])
    assert ((conf_b >= 0) & (conf_b <= prob.max())).all()


@pytest.mark.parametrize("mode", ["ensemble", "fine"])
def test_round_trip_and_cli(dev, mode, ensemble_run, fine_run, file_b, tmp_path):
    from idelucs_amd.ensemble import FittedEnsemble
    run = ensemble_run if mode == "ensemble" else fine_run
    path, rows = file_b
    ens = FittedEnsemble.load(run["model"])
    before = ens.assign(path, dev)
    ens.save(str(tmp_path / "again"))
    after = FittedEnsemble.load(str(tmp_path / "again")).assign(path, dev)
    assert list(before[0]) == list(after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    out_dir = _cli(str(tmp_path), ["--assign", path, "--model", run["model"]])
    assert os.path.dirname(out_dir) == os.path.join(str(tmp_path), "Results", "subset_B")
    names, y, conf = _table(out_dir)
    assert names == list(before[0]) and np.array_equal(y, before[1]) and np.array_equal(conf, before[2])
    assert not os.path.exists(os.path.join(str(tmp_path), "ALL_RESULTS.tsv"))
