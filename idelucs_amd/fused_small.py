"""idelucs_amd.fused_small -- the explicit training step of model_size='small' (myNet + RMSprop) on this library's own kernels,
replayed as a HIP graph.  Opt-in: IID_model(args) with args['small_step'] = 'native' (CLI: --small_step native).

One full-batch step of reference idelucs/models.py:117-133 is at most 8 launches (csrc/small_step.hip has the design):
    idl_small_l1_fwd  ->  idl_small_mid_fwd  ->  InfoNCE / IIC (2 launches; 4 for n_clusters > 48)  ->  idl_small_mid_bwd
                      ->  idl_small_wgrad_rms (every gradient with RMSprop in its epilogue, step loss, step counter, next batch)
Batches are assembled from the HBM feature store into two x buffers that alternate: the last launch of step t writes the batch of
step t + 1 into the buffer step t does not read, at the device-resident offset ctl[1].  An epoch replays one captured graph of an
even number of steps (one stream, no forked branches); the steps that do not fill a replay and the partial last batch run eagerly
(the partial batch: the same kernels, and for an m that is not a multiple of 32 one library product for S = f f^T).

The parameters are the nn.Parameters of model.net (state_dict / predict / weights_init unchanged); RMSprop state lives here.
FusedSmallTrainer(..., momentum=mu) is the momentum form: torch's RMSprop with a momentum_buffer, which is what the Triangle
scheduler's CyclicLR makes of the reference's optimizer (models.py:87-88, 99); its last launch is idl_small_wgrad_rms_momentum and
set_momentum() follows the scheduler beside set_lr().  FusedSmallOptTrainer (below) is the step with torch's SGD or Adam
(models.py:89-92): the same five launches and idl_small_wgrad_opt as the last one.
"""
import ctypes

import torch

from . import _lib
from ._lib import lib as _L
from .fused import TEMPERATURE, _launch, _p, _stream, launch_losses
from .fused_opt import KIND_ADAM, KIND_SGD, _OptimizerState  # (KIND_* stay names of this module)

H1, H2, LAT = 400, 128, 64  # myNet's widths (reference PytorchUtils.py:12-18)
MAX_C = 256
STEPS_PER_GRAPH = 16


class _SmallBuffers:
    """Activations / gradients of one batch shape (m = 2*B rows)."""

    def __init__(self, m, F, C, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.m = m
        self.xs = [torch.zeros((m, F), **f32), torch.zeros((m, F), **f32)]     # this step's batch / the next one being assembled
        self.x = self.xs[0]
        self.a1 = torch.empty((m, H1), **f32)
        self.a2 = torch.empty((m, H2), **f32)
        self.d2 = torch.empty((m, H2), **f32)
        self.f = torch.empty((m, LAT), **f32)
        self.inv = torch.empty((m,), **f32)
        self.z = torch.empty((m, C), **f32)
        self.lse = torch.empty((m,), **f32)
        self.loss_rows = torch.empty((m,), **f32)
        self.nce_ws_bytes = int(_L.idl_nce_fused_workspace(m))          # -1: m not taken by the fused InfoNCE kernels
        self.nce_fused = self.nce_ws_bytes > 0
        parts = int(_L.idl_nce_fused_parts()) if self.nce_fused else 1
        self.G = torch.empty((parts, m, LAT), **f32)
        self.nce_ws = torch.empty(max(self.nce_ws_bytes, 4) // 4, **f32)
        self.S = None if self.nce_fused else torch.empty((m, m), **f32)
        self.P0 = torch.empty((C, C), **f32)
        self.iic_scratch = torch.empty((C * C + 2 * C + 8,), **f32)
        self.dzs = torch.empty((m, C), **f32) if 48 < C <= 200 else None
        self.dlogits = torch.empty((m, C), **f32)
        self.dh = torch.empty((m, LAT), **f32)
        self.da2 = torch.empty((m, H2), **f32)
        self.dr1 = torch.empty((m, H1), **f32)


class FusedSmallTrainer:
    def __init__(self, net, lr, weight, lamb, weight_decay=0.01, alpha=0.99, eps=1e-8, seed=0, momentum=None):
        """momentum: None -> the momentum-free step; a number -> the momentum form (momentum_buffer per tensor, set_momentum())."""
        self._init_network(net, weight, lamb, seed)
        self.square_avg = [torch.zeros_like(p) for p in self.params]
        self.with_momentum = momentum is not None
        self.momentum_buffer = [torch.zeros_like(p) for p in self.params] if self.with_momentum else []
        self.hyper = torch.tensor([lr, alpha, eps, weight_decay, 1.0 - alpha] + ([float(momentum)] if self.with_momentum else []),
                                  dtype=torch.float32, device=self.dev)
        n = len(self.params)
        self._vp = (ctypes.c_void_p * n)(*[v.data_ptr() for v in self.square_avg])
        self._mp = (ctypes.c_void_p * n)(*[v.data_ptr() for v in self.momentum_buffer]) if self.with_momentum else None

    def _init_network(self, net, weight, lamb, seed):
        """Everything of the trainer that does not depend on the optimizer: the parameters, the gradients, the counters, the buffers."""
        lin1, lin2, lini, linc = net.layers[0], net.layers[3], net.instance, net.classifier[1]
        self.net = net
        self.params = [lin1.weight, lin1.bias, lin2.weight, lin2.bias, lini.weight, lini.bias, linc.weight, linc.bias]
        self.dev = lin1.weight.device
        self.F, self.C = lin1.in_features, linc.out_features
        if (lin1.out_features, lin2.in_features, lin2.out_features, lini.in_features, lini.out_features, linc.in_features) != (H1, H1, H2, H2, LAT, H2) \
                or self.C > MAX_C:
            raise ValueError(f"FusedSmallTrainer needs myNet (400 -> 128 -> 64 / C) and n_clusters <= {MAX_C}")
        self.grads = [torch.zeros_like(p) for p in self.params]
        self.weight, self.lamb, self.seed = float(weight), float(lamb), int(seed) & (2 ** 64 - 1)
        self.ctl = torch.zeros(2, dtype=torch.int64, device=self.dev)        # [step counter, batch offset]
        self.out = torch.zeros(4, dtype=torch.float32, device=self.dev)      # [step loss, running sum, nce, iic]
        self._bufs = {}
        self._graphs = {}
        self._perm = None
        self._pp = (ctypes.c_void_p * len(self.params))(*[p.data_ptr() for p in self.params])
        self.keep_grads = False         # True: the step also writes dW1 to grads[0] (tests; the small tensors' gradients are always kept)

    def _gp(self):
        return (ctypes.c_void_p * len(self.grads))(*[None if (i == 0 and not self.keep_grads) else g.data_ptr()
                                                     for i, g in enumerate(self.grads)])

    def begin_voter(self, voter, keep_state=False):
        """Dropout stream of voter v: the Philox counter word the kernels take from ctl[0] starts at v << 24 (as FusedLinearTrainer's),
        so voter v draws the same masks wherever it trains.  keep_state: the previous voter's RMSprop running averages stay
        (IDELUCS_VOTER_STATE=carry, models.IID_model)."""
        self.ctl[0:1].fill_((int(voter) & 0xFF) << 24)
        if keep_state:
            return
        for v in self.square_avg + self.momentum_buffer:
            v.zero_()

    def set_lr(self, lr):
        self.hyper[0:1].fill_(float(lr))

    def set_momentum(self, momentum):
        if not self.with_momentum:
            raise ValueError("this FusedSmallTrainer was built without a momentum buffer (momentum=None)")
        self.hyper[5:6].fill_(float(momentum))

    def gradient(self, i):
        """Gradient of parameter i of the last step (i = 0, dW1: only when keep_grads was set before that step)."""
        return self.grads[i]

    def buffers(self, m):
        if m not in self._bufs:
            self._bufs[m] = _SmallBuffers(m, self.F, self.C, self.dev)
        return self._bufs[m]

    def dropout_masks(self, step, m):
        """(mask after layer 1 [m, 400], classifier mask [m, 128]) as bool tensors: what a training step whose counter ctl[0] is
        `step` draws (tests)."""
        m1 = torch.empty((m, H1), dtype=torch.float32, device=self.dev)
        m2 = torch.empty((m, H2), dtype=torch.float32, device=self.dev)
        _lib.check(_L.idl_small_dropout_masks(self.seed, int(step), m, _p(m1), _p(m2), _stream()))
        return m1 > 0.5, m2 > 0.5

    # ------------------------------------------------------------------ one step on a filled buffer
    @torch.no_grad()
    def step_on_batch(self, bf, train=True, xi=0, next_from=None):
        """Forward, backward and RMSprop update for the [m, F] batch in bf.xs[xi] (rows [0, m/2) "true", [m/2, m) "modified").
        Only enqueues work on the current stream.  next_from = a FeatureStore: the step advances the batch offset ctl[1] by m/2 and
        its last launch assembles the next batch into bf.xs[1 - xi]."""
        m, C, F, tr = bf.m, self.C, self.F, 1 if train else 0
        x = bf.xs[xi]
        chk = _lib.check
        W1, b1, W2, b2, Wi, bi, Wc, bc = self.params
        chk(_L.idl_small_l1_fwd(_p(x), _p(W1), m, F, _p(bf.a1), _stream()))
        chk(_L.idl_small_mid_fwd(_p(bf.a1), _p(b1), _p(W2), _p(b2), _p(Wi), _p(bi), _p(Wc), _p(bc), m, C, tr, self.seed, _p(self.ctl),
                                 _p(bf.a2), _p(bf.d2), _p(bf.f), _p(bf.inv), _p(bf.z), _stream()))
        # ---- the losses: the existing InfoNCE / IIC launches on f and z (with the fused InfoNCE kernels, 48 < C <= 200: the IIC core's
        # rows, then z dP0 for every row)
        dz = bf.nce_fused and 48 < C <= 200
        launch_losses(_launch, bf, self.lamb, self.weight, self.out, dz=dz)
        dP0, dzs = (None, bf.dzs) if dz else (bf.P0, None)
        nce_coef = (1.0 - self.weight) / (m * TEMPERATURE)
        adv = m // 2 if next_from is not None else 0
        chk(_L.idl_small_mid_bwd(_p(bf.z), _p(bf.f), _p(bf.inv), _p(bf.G), bf.G.shape[0], _p(dP0), _p(dzs), _p(bf.a1), _p(bf.a2),
                                 _p(W2), _p(Wi), _p(Wc), m, C, tr, nce_coef, self.seed, _p(self.ctl), adv,
                                 _p(bf.dlogits), _p(bf.dh), _p(bf.da2), _p(bf.dr1), _stream()))
        st = next_from
        # the whole next batch as fp32 rows, at the offset ctl[1] that the middle backward advanced
        nb = None if st is None else _lib.idl_next_batch_t(
            feats=_p(st.feats), n=st.n, f=st.f, view_stride=st.n * st.f, pair_idx=_p(self._perm), base=_p(self.ctl[1:]), base_add=0, n_pairs=st.n_pairs,
            batch=m // 2, mean=_p(st.mean), scale=_p(st.scale), inv_scale=_p(st.inv_scale), y=_p(bf.xs[1 - xi]), part=0, part_end=1, parts=1)
        self._last_launch((_p(x), _p(bf.dr1), _p(bf.a1), _p(bf.da2), _p(bf.a2), _p(bf.dh), _p(bf.d2), _p(bf.dlogits), m, F, C,
                           _p(bf.loss_rows), 1.0 - self.weight, self.weight, _p(self.out), nb, _stream()))

    def _last_launch(self, tail):
        """The step's last launch: every gradient with the optimizer's update in its epilogue, the step loss, the step counter, the next batch.
        tail: the arguments every form of it takes from `x` on."""
        if self.with_momentum:
            _lib.check(_L.idl_small_wgrad_rms_momentum(self._pp, self._gp(), self._vp, self._mp, _p(self.hyper), _p(self.ctl), *tail))
        else:
            _lib.check(_L.idl_small_wgrad_rms(self._pp, self._gp(), self._vp, _p(self.hyper), _p(self.ctl), *tail))

    def _graph_key_extra(self):
        """What a captured graph bakes in besides the store's addresses and the batch shape (a tuple; nothing here)."""
        return ()

    def _gather(self, store, bf, b):
        _lib.check(_L.idl_gather_pairs_at(_p(store.feats), store.n, store.f, store.n * store.f, _p(self._perm), _p(self.ctl[1:]),
                                          b, _p(store.mean), _p(store.scale), _p(store.inv_scale), _p(bf.xs[0]), _stream()))

    # ------------------------------------------------------------------ one epoch over the store
    @torch.no_grad()
    def run_epoch(self, store, batch_sz, generator=None, use_graph=True):
        """One pass over a fresh permutation of the N*n_mimics pairs (models.py:117-133) -> (device scalar sum of the step losses,
        number of batches)."""
        if store.f != self.F:
            raise ValueError(f"the feature store has {store.f} features a row, the network {self.F}")
        n_pairs = store.n_pairs
        if self._perm is None or self._perm.numel() != n_pairs:
            self._perm = torch.empty(n_pairs, dtype=torch.int64, device=self.dev)
            self._graphs.clear()
        torch.randperm(n_pairs, device=self.dev, generator=generator, out=self._perm)
        self.ctl[1:2].zero_()
        self.out[1:2].zero_()
        n_full, rem = divmod(n_pairs, batch_sz)
        if n_full:
            bf = self.buffers(2 * batch_sz)
            self._gather(store, bf, batch_sz)         # batch 0; every later one is assembled by the step before it
            done = 0
            per = min(STEPS_PER_GRAPH, n_full // 2 * 2)
            if use_graph and per >= 2:
                # every address the captured launches bake in is part of the key (a store refitted in place keeps its graph)
                base = (2 * batch_sz, store.feats.data_ptr(), store.mean.data_ptr(), store.scale.data_ptr(), store.inv_scale.data_ptr(),
                       self._perm.data_ptr(), store.n, store.f, store.n_pairs, per, self.keep_grads)
                key = base + self._graph_key_extra()
                g = self._graphs.get(key)
                if g is None:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for i in range(per):
                            self.step_on_batch(bf, xi=i % 2, next_from=store)
                    self._graphs = {k_: v for k_, v in self._graphs.items() if k_[:len(base)] == base}      # one store at a time
                    self._graphs[key] = g
                for _ in range(n_full // per):
                    g.replay()
                done = n_full // per * per
            for i in range(done, n_full):
                self.step_on_batch(bf, xi=i % 2, next_from=store)
        if rem:
            bf = self.buffers(2 * rem)
            self._gather(store, bf, rem)
            self.step_on_batch(bf)
        return self.out[1], n_full + (1 if rem else 0)


class FusedSmallOptTrainer(_OptimizerState, FusedSmallTrainer):
    """The step of FusedSmallTrainer with torch.optim.SGD or torch.optim.Adam (reference models.py:89-92) in its last launch,
    idl_small_wgrad_opt.  Opt-in: IID_model(args) with args['small_opt_step'] = 'native' (CLI: --small_opt_step native).  Nothing in the
    five launches in front of it knows which optimizer follows; buffers, dropout streams, dropout_masks(), keep_grads, partial batches and
    the epoch loop are inherited.  SGD keeps momentum_buffer per tensor, Adam exp_avg and exp_avg_sq plus its step count in two words that
    swap roles from step to step (fused_opt._OptimizerState, which FusedLinearOptTrainer shares).  The hyperparameters are copied from
    the torch optimizer's group before every epoch (sync_hyper): the schedulers keep acting on that object, CyclicLR on momentum / beta1
    as well as the rate."""

    def __init__(self, net, optimizer, weight, lamb, seed=0):
        """optimizer: the torch.optim.SGD / torch.optim.Adam object whose first group holds the hyperparameters (its state is not used)."""
        self._init_network(net, weight, lamb, seed)
        self._init_optimizer(optimizer, kinds=(KIND_SGD, KIND_ADAM), state2_kinds=(KIND_ADAM,))

    def begin_voter(self, voter, keep_state=False):
        """Dropout stream of voter v as FusedSmallTrainer.begin_voter sets it.  keep_state: the previous voter's optimizer state stays
        (IDELUCS_VOTER_STATE=carry); the step count is part of it."""
        self.ctl[0:1].fill_((int(voter) & 0xFF) << 24)
        if not keep_state:
            self._reset_state()

    def _last_launch(self, tail):
        _lib.check(_L.idl_small_wgrad_opt(self._opt_state(), self._pp, self._gp(), _p(self.ctl), *tail))
        self._step_taken()

    def _graph_key_extra(self):
        """The role of the two step words: an epoch with an odd number of steps flips it, and a captured graph bakes their addresses."""
        return (self._tpar,)
