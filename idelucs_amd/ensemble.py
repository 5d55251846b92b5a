"""idelucs_amd.ensemble -- what a training run learns, kept: FittedEnsemble holds the voters' weights, the predict scaler of the training
file and the ensemble's vote tables (or, in the fine-grained mode, the last voter's training latent with HDBSCAN's labels), writes them to
one file and assigns the sequences of ANOTHER file to the run's clusters without training again.

The reference has no counterpart: idelucs/__main__.py trains, writes assignments.tsv and ends.  Two rules make the assignment:

  mode 'ensemble' (n_clusters > 0).  The run's final labels are k-means on the centred one-hot vote rows (posthoc.label_features); a
      k-means centre is its cluster's mean, so the centres are the vote tables counts[K, V, C] / cnt[K] and a new record's squared
      distance to centre k is, with a = counts / cnt and p_v its (relabelled) vote,
          d2[k] = sum_{v, c} a[k, v, c]^2 + sum_{v: p_v >= 0} (1 - 2 a[k, v, p_v])
      -- the centring cancels.  Label: argmin, lowest k on ties; confidence: the reference's (1 / d2)[k*] / sum_k (1 / d2)[k].
  mode 'fine' (n_clusters == 0).  HDBSCAN is not parametric; a new record takes the label of its nearest training latent
      (idl_nn_rows: float64 distances from the difference vector, ties to the lowest index, so a training sequence finds itself at
      distance exactly 0) and that point's probability scaled by min(1, spacing / distance) -- the rule fine_grained_clusters(mode="approx")
      applies to its unsampled points.
"""
import os

import numpy as np
import torch

from . import _lib
from . import utils
from .PytorchUtils import NetLinear, myNet

FORMAT_VERSION = 1
FILE_NAME = "ensemble.pt"
_L = _lib.lib


def check_scope(k, model_size):
    """What a saved ensemble supports, refused with a message before any work: one rank, and a (k, model_size) whose rows
    utils.feature_chunks_of_input can form."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("saving or applying an ensemble needs one rank (WORLD_SIZE is %s): the voters' weights live on the ranks that trained them"
                         % os.environ["WORLD_SIZE"])
    if model_size not in ("linear", "small"):
        raise ValueError("Invalid Model Type")
    if not isinstance(k, int) or not 1 <= k <= _lib.MAX_K or not utils.stream_route_ok(k, model_size == "small"):
        raise ValueError(f"k={k} with model_size={model_size!r} gives rows the chunked predict inputs cannot form (their length must be a "
                         "multiple of 4): an ensemble of this shape cannot be saved or applied")


def model_path(directory):
    return os.path.join(directory, FILE_NAME)


def check_not_saved(directory):
    """save() does not overwrite: the CLI asks before it trains."""
    if os.path.exists(model_path(directory)):
        raise FileExistsError(f"{model_path(directory)} exists: a saved ensemble is not overwritten (choose another directory)")


def nn_rows(q, x, self0=-1):
    """idl_nn_rows: q [m, 64], x [n, 64] float32 device tensors -> (idx int32 [m], d2 float64 [m]): every query's exact nearest corpus row
    (float64 from the difference vector, equal distances to the lowest index); self0 >= 0: q is x[self0 : self0 + m] and a row is not its own
    neighbour."""
    if not (q.is_cuda and x.is_cuda and q.dtype == x.dtype == torch.float32 and q.dim() == x.dim() == 2 and q.shape[1] == x.shape[1]):
        raise ValueError("nn_rows takes two float32 device matrices of the same width")
    q, x = q.contiguous(), x.contiguous()
    m, n = q.shape[0], x.shape[0]
    idx = torch.empty(m, dtype=torch.int32, device=q.device)
    d2 = torch.empty(m, dtype=torch.float64, device=q.device)
    _lib.check(_L.idl_nn_rows(utils._ptr(q), m, utils._ptr(x), n, q.shape[1], int(self0), utils._ptr(idx), utils._ptr(d2), utils._stream_ptr()))
    return idx, d2


def unit_map(y_raw, n_units):
    """int32 [n_units]: output unit -> its label after posthoc.relabel_first_occurrence (reference __main__.py:129-139) on the training
    file; -1 for a unit that never won there."""
    from .posthoc import relabel_first_occurrence
    y_raw = np.asarray(y_raw).astype(np.int64)
    out = np.full(n_units, -1, dtype=np.int32)
    out[y_raw] = relabel_first_occurrence(y_raw)
    return out


def vote_tables(votes, y_pred, n_clusters):
    """(counts int64 [K, V, C], cnt int64 [K]) of the gathered votes [V, N] and the final labels [N]: counts[k, v, c] = the training
    records with final label k whose voter v voted c."""
    votes = np.asarray(votes).astype(np.int64)
    y = np.asarray(y_pred).astype(np.int64)
    v, n = votes.shape
    counts = np.zeros((n_clusters, v, n_clusters), dtype=np.int64)
    for i in range(v):
        np.add.at(counts, (y, i, votes[i]), 1)
    return counts, np.bincount(y, minlength=n_clusters).astype(np.int64)


def votes_to_clusters(p, counts, cnt):
    """The 'ensemble' rule on a chunk: p int64 [V, M] (-1 = no vote), counts [K, V, C], cnt [K] on p's device -> (label int64 [M],
    confidence float64 [M], d2 float64 [M, K]).  float64 throughout.  A cluster without training records is at distance +inf; where the
    best distance is 0 the confidence is 1.0 (the reference's inf / inf is NaN there)."""
    k, v, c = counts.shape
    cn = cnt.to(torch.float64)
    a = counts.to(torch.float64) / cn.clamp_min(1.0)[:, None, None]
    d2 = (a * a).sum((1, 2))[None, :].repeat(p.shape[1], 1)
    for i in range(v):
        valid = p[i] >= 0
        g = a[:, i, :].t()[p[i].clamp_min(0)]                            # [M, K]: a[k, i, p_i]
        d2 += torch.where(valid[:, None], 1.0 - 2.0 * g, torch.zeros_like(g))
    d2 = d2.clamp_min_(0.0)
    d2[:, cn == 0] = float("inf")
    best, label = torch.min(d2, 1)                                        # (the first minimum: the lowest k on ties)
    w = 1.0 / d2
    conf = torch.where(best == 0.0, torch.ones_like(best), (1.0 / best) / w.sum(1))
    return label, conf, d2


def _open_input(sequence_file, dev):
    """The packed bases of a file on the device, through the reader predict_feature_chunks uses -> (device input, FastaFile to close)."""
    din = None
    if utils.OPTIONS["one_pass"] != "0":
        din = utils._OnePassInput.create(sequence_file, dev)
        if din is not None:
            ff = din.ff
            din.fill()
    if din is None:
        ff = utils.FastaFile(sequence_file, check=True)
        din = utils._DeviceInput(ff, dev)
    return din, ff


def scaler_of_file(sequence_file, k, model_size, device=None, chunk_rows=None):
    """utils.predict_scaler of a file -> (mean, scale) float64 [F] on the host."""
    dev = utils._device(device)
    din, ff = _open_input(sequence_file, dev)
    try:
        mean, scale = utils.predict_scaler(din, k, model_size == "small", chunk_rows)
        return mean.cpu(), scale.cpu()
    finally:
        ff.close()


def _cpu_state(net):
    return {name: t.detach().to("cpu", copy=True) for name, t in net.state_dict().items()}


class VoterCapture:
    """The on_voter hook of training.train_voters: keeps the state_dict of every voter (or of `only`) on the host."""

    def __init__(self, only=None):
        self.only, self.states = only, {}

    def __call__(self, voter, net):
        if self.only is None or voter == self.only:
            self.states[int(voter)] = _cpu_state(net)           # (a voter trained again after a PlanesOverflow replaces its first attempt)


class FittedEnsemble:
    """A trained ensemble: format version, k, model_size, n_units (the networks' output width), mode ('ensemble' or 'fine'), the predict
    scaler (mean, scale: float64 [F]), the voters' state_dicts; mode 'ensemble': unit_maps int32 [V, n_units], counts int64 [K, V, C],
    cnt int64 [K]; mode 'fine' (the last voter only): latent float32 [N, 64], labels int64 [N] (HDBSCAN's + 1), prob float64 [N],
    spacing float64 [N] (every training point's distance to its nearest other one).  All tensors on the host."""

    TENSORS = ("mean", "scale", "unit_maps", "counts", "cnt", "latent", "labels", "prob", "spacing")

    def __init__(self, k, model_size, n_units, mode, mean, scale, states, unit_maps=None, counts=None, cnt=None, latent=None, labels=None,
                 prob=None, spacing=None, version=FORMAT_VERSION):
        if version != FORMAT_VERSION:
            raise ValueError(f"a saved ensemble of format version {version}: this package reads version {FORMAT_VERSION}")
        check_scope(k, model_size)
        if mode not in ("ensemble", "fine"):
            raise ValueError(f"mode must be 'ensemble' or 'fine', not {mode!r}")
        self.version, self.k, self.model_size, self.n_units, self.mode = int(version), int(k), model_size, int(n_units), mode
        self.mean, self.scale = mean, scale
        self.states = list(states)
        self.unit_maps, self.counts, self.cnt = unit_maps, counts, cnt
        self.latent, self.labels, self.prob, self.spacing = latent, labels, prob, spacing
        f = self.n_features
        if tuple(mean.shape) != (f,) or tuple(scale.shape) != (f,) or mean.dtype != torch.float64 or scale.dtype != torch.float64:
            raise ValueError(f"the predict scaler must be two float64 [{f}] tensors")
        if mode == "ensemble":
            v = len(self.states)
            if v < 1 or unit_maps is None or counts is None or cnt is None or tuple(unit_maps.shape) != (v, self.n_units) \
                    or counts.dim() != 3 or counts.shape[1] != v or tuple(cnt.shape) != (counts.shape[0],):
                raise ValueError("mode 'ensemble' needs unit_maps [V, n_units], counts [K, V, C] and cnt [K] for its V voters")
        else:
            if len(self.states) != 1 or latent is None or labels is None or prob is None or spacing is None or latent.dim() != 2 \
                    or latent.shape[1] != 64 or latent.dtype != torch.float32 or not len(latent) == len(labels) == len(prob) == len(spacing):
                raise ValueError("mode 'fine' needs the last voter alone, its latent float32 [N, 64] and labels, prob, spacing [N]")

    @property
    def reduce(self):
        return self.model_size == "small"

    @property
    def n_features(self):
        k = self.k
        if self.model_size == "linear":
            return 4 ** k
        return (4 ** k + 4 ** (k // 2)) // 2 if k % 2 == 0 else (4 ** k) // 2

    # ------------------------------------------------------------------ from a run
    @classmethod
    def from_votes(cls, sequence_file, k, model_size, states, raw_votes, votes, y_pred, n_clusters, device=None):
        """mode 'ensemble'.  states / raw_votes: per voter, in voter order, the state_dict and the network's own argmax on the training
        file; votes [V, N]: the relabelled votes the run's ensemble was computed from; y_pred [N]: its final labels."""
        check_scope(k, model_size)
        mean, scale = scaler_of_file(sequence_file, k, model_size, device)
        maps = np.stack([unit_map(raw, n_clusters) for raw in raw_votes])
        votes = np.asarray(votes)
        for v, raw in enumerate(raw_votes):
            if not np.array_equal(maps[v][np.asarray(raw).astype(np.int64)], votes[v]):
                raise ValueError(f"voter {v}: the gathered votes are not its outputs relabelled in order of first occurrence")
        counts, cnt = vote_tables(votes, y_pred, n_clusters)
        return cls(k, model_size, n_clusters, "ensemble", mean, scale, states, unit_maps=torch.from_numpy(maps),
                   counts=torch.from_numpy(counts), cnt=torch.from_numpy(cnt))

    @classmethod
    def from_latent(cls, sequence_file, k, model_size, state, latent, labels, prob, device=None):
        """mode 'fine'.  state: the last voter's state_dict; latent [N, 64]: its predict's latent on the training file (float32 values, as
        predict returns them widened); labels / prob: fine_grained_clusters' (HDBSCAN's labels + 1, probabilities)."""
        check_scope(k, model_size)
        dev = utils._device(device)
        mean, scale = scaler_of_file(sequence_file, k, model_size, dev)
        lat64 = np.asarray(latent)
        lat = torch.from_numpy(np.ascontiguousarray(lat64, dtype=np.float32))
        if not np.array_equal(lat.numpy().astype(lat64.dtype), lat64):
            raise ValueError("the latent does not hold float32 values")
        if len(lat) >= 2:
            spacing = nn_rows(lat.to(dev), lat.to(dev), self0=0)[1].sqrt_().cpu()
        else:
            spacing = torch.full((len(lat),), float("inf"), dtype=torch.float64)
        n_units = int(state[[name for name in state if name.startswith("classifier") and name.endswith("weight")][-1]].shape[0])
        return cls(k, model_size, n_units, "fine", mean, scale, [state], latent=lat,
                   labels=torch.from_numpy(np.asarray(labels).astype(np.int64)), prob=torch.from_numpy(np.asarray(prob).astype(np.float64)),
                   spacing=spacing)

    # ------------------------------------------------------------------ disk
    def _payload(self):
        d = {"format_version": self.version, "k": self.k, "model_size": self.model_size, "n_units": self.n_units, "mode": self.mode,
             "voters": [{name: t.detach().cpu().contiguous() for name, t in s.items()} for s in self.states]}
        for name in self.TENSORS:
            t = getattr(self, name)
            d[name] = None if t is None else t.detach().cpu().contiguous()
        return d

    def save(self, directory):
        """Write directory/ensemble.pt (tensors and plain Python values only: torch.load(..., weights_only=True) reads it) -> its path.
        An existing file is not overwritten."""
        os.makedirs(directory, exist_ok=True)
        check_not_saved(directory)
        path = model_path(directory)
        with open(path, "xb") as fh:
            torch.save(self._payload(), fh)
        return path

    @classmethod
    def load(cls, directory):
        d = torch.load(model_path(directory), map_location="cpu", weights_only=True)
        version = d.get("format_version") if isinstance(d, dict) else None
        if version != FORMAT_VERSION:
            raise ValueError(f"{model_path(directory)} holds format version {version!r}: this package reads version {FORMAT_VERSION}")
        return cls(d["k"], d["model_size"], d["n_units"], d["mode"], d["mean"], d["scale"], d["voters"],
                   **{name: d[name] for name in cls.TENSORS[2:]}, version=version)

    # ------------------------------------------------------------------ assignment
    def _networks(self, dev):
        nets = []
        for state in self.states:
            net = (NetLinear if self.model_size == "linear" else myNet)(self.n_features, self.n_units)
            net.load_state_dict(state)
            nets.append(net.to(dev).eval())
        return nets

    def _predict_mode(self, predict):
        """predict=None or 'torch': the voters run as nn.Modules; 'native': through predict_native.NativeLinearPredictor -- linear models
        of the shapes IID_model._predict_mode accepts; anything else raises ValueError."""
        from .models import IID_model
        return IID_model._predict_mode({'predict': predict, 'model_size': self.model_size, 'k': self.k, 'n_clusters': self.n_units})

    def _small_predict_mode(self, small_predict, predict=None):
        """small_predict=None or 'torch': as _predict_mode decides; 'native': through predict_native.NativeSmallPredictor -- small models of the
        shapes IID_model._small_predict_mode accepts; anything else raises ValueError."""
        from .models import IID_model
        return IID_model._small_predict_mode({'small_predict': small_predict, 'predict': predict, 'model_size': self.model_size, 'k': self.k,
                                              'n_clusters': self.n_units})

    def voter_outputs(self, sequence_file, device=None, chunk_rows=None, predict=None, small_predict=None):
        """The saved voters' eval forward on a file's rows, standardised with the TRAINING file's statistics, a chunk at a time (there is
        no [M, F] matrix) -> (names, units int64 [V, M] on the device: every voter's argmax, latent float32 [M, 64] on the device: the
        last voter's).  predict: the mode the run predicted with ('native': a row's outputs are the training run's bit for bit whatever
        chunk_rows is, and no library product is involved).  small_predict: the same for model_size='small'."""
        native = self._predict_mode(predict) == 'native'
        small_native = self._small_predict_mode(small_predict, predict) == 'native'
        native = native or small_native
        _lib.require_gpu()
        dev = utils._device(device)
        if not native:
            from . import gemm_tuning
            gemm_tuning.maybe_enable(0)             # the products run on the solutions a training run's predict runs on (nothing is tuned)
        stats = (self.mean.to(dev), self.scale.to(dev))
        nets = self._networks(dev)
        if native:
            from . import predict_native
            predictors = [(predict_native.NativeSmallPredictor if small_native else predict_native.NativeLinearPredictor)(net) for net in nets]
        din, ff = _open_input(sequence_file, dev)
        try:
            m = din.n
            units = torch.empty((len(nets), m), dtype=torch.int64, device=dev)
            latent = torch.empty((m, 64), dtype=torch.float32, device=dev)
            with torch.no_grad():
                for lo, hi, x in utils.feature_chunks_of_input(din, self.k, self.reduce, None, chunk_rows, stats=stats):
                    for v, net in enumerate(nets):
                        if native:
                            lat, _, unit, _ = predictors[v].forward(x)
                            units[v, lo:hi] = unit
                        else:
                            out, lat = net(x)
                            units[v, lo:hi] = torch.max(out, 1)[1]         # (as IID_model.predict)
                    latent[lo:hi] = lat
            torch.cuda.current_stream().synchronize()                      # (the reader's arenas are reused by the next file)
        finally:
            ff.close()
        return ff.names, units, latent

    def assign(self, sequence_file, device=None, predict=None, small_predict=None):
        """The sequences of a file -> (names, y_pred int64 [M], confidence float64 [M]) in the clusters of the training run.
        mode 'ensemble': every voter's argmax through its unit map (a unit that never won on the training file: no vote), then
        votes_to_clusters -- confidence 1.0 where the record sits on its centre (the reference's inf / inf is NaN there).
        mode 'fine': labels[nn], prob[nn] * min(1, spacing[nn] / dist) with nn the nearest training latent (dist == 0: the factor is 1),
        so a sequence of the training file gets its training label and probability.
        predict / small_predict: as voter_outputs -- assign with the mode the run predicted with."""
        names, units, latent = self.voter_outputs(sequence_file, device, predict=predict, small_predict=small_predict)
        dev = units.device
        if self.mode == "ensemble":
            maps = self.unit_maps.to(dev).long()
            p = torch.gather(maps, 1, units)
            y, conf, _ = votes_to_clusters(p, self.counts.to(dev), self.cnt.to(dev))
        else:
            nn, d2 = nn_rows(latent, self.latent.to(dev))
            if latent.shape[0] and int(nn.min()) < 0:
                raise ValueError("a sequence's latent is not finite: it has no nearest training point")
            nn = nn.long()
            dist = d2.sqrt()
            factor = torch.where(dist == 0.0, torch.ones_like(dist), (self.spacing.to(dev)[nn] / dist).clamp_max(1.0))
            y, conf = self.labels.to(dev)[nn], self.prob.to(dev)[nn] * factor
        return names, y.cpu().numpy().astype(np.int64), conf.double().cpu().numpy()
