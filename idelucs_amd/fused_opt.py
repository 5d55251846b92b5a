"""idelucs_amd.fused_opt -- the explicit training step of NetLinear with torch.optim.SGD or torch.optim.Adam (reference
idelucs/models.py:89-92) on this library's own kernels, replayed as a HIP graph.  Opt-in: IID_model(args) with
args['linear_step'] = 'native' (CLI: --linear_step native).  Also torch.optim.RMSprop WITH the momentum buffer that the Triangle
scheduler's CyclicLR gives it (models.py:87-88, 99): args['rmsprop_momentum'] = 'follow' (CLI: --rmsprop_momentum follow).

Nothing in the forward or backward of the fp32 step forms of fused.FusedLinearTrainer knows which optimizer follows, so a step here is
those launches with the gradient-only dW1 tiles and ONE new last launch (csrc/opt_step.hip):
    n_clusters <= 48     idl_l1_fwd -> idl_mid_fwd_gather -> InfoNCE + IIC -> idl_mid_bwd_gather -> idl_wgrad_rmsprop (gradient only)
                         -> idl_opt_step_gather_wgrad (dW2 tiles, SGD / Adam on every tensor, step loss, counters)
    anything else        the general form's forward and backward (_LinearStepParts._general_fwd_bwd: library products for odd shapes and n_clusters > 48; at
                         48 < n_clusters <= 200 the IIC core writes z dP0 itself), dW1 on the tiles where they apply, the same last launch
The next batch rides in the two middle launches where it does for RMSprop.  SGD keeps momentum_buffer per tensor, RMSprop square_avg and
momentum_buffer, Adam exp_avg and exp_avg_sq plus its step count in two words that swap roles from step to step (the launch reads one and writes the other).  The
hyperparameters are copied from the torch optimizer's group before every epoch (sync_hyper): the schedulers keep acting on that
object, CyclicLR on momentum / beta1 as well as the rate.
"""
import ctypes

import torch

from . import _lib
from ._lib import lib as _L
from .fused import STEPS_PER_GRAPH, _LinearStepParts, _launch, _mm_now, _p, _stream

KIND_SGD, KIND_ADAM, KIND_RMSPROP = 1, 2, 3
_OPTIMIZERS = ((KIND_SGD, "SGD"), (KIND_ADAM, "Adam"), (KIND_RMSPROP, "RMSprop"))      # a kind and its class in torch.optim


class _OptimizerState:
    """What a native step keeps for the torch optimizer whose update its last launch applies (FusedLinearOptTrainer here,
    fused_small.FusedSmallOptTrainer): the kind, one or two state tensors per parameter, the hyperparameters as a device double[5] and the
    step count in two words that swap roles from step to step (the launch reads one and writes the other)."""

    def _init_optimizer(self, optimizer, kinds, state2_kinds):
        """kinds: the optimizers this trainer takes; state2_kinds: those of them whose update keeps a second state tensor.  After
        _init_network (self.params, self.dev)."""
        who = type(self).__name__
        self.kind = next((k for k, name in _OPTIMIZERS if k in kinds and isinstance(optimizer, getattr(torch.optim, name))), None)
        if self.kind is None:
            names = [f"torch.optim.{name}" for k, name in _OPTIMIZERS if k in kinds]
            raise ValueError(f"{who} needs a {', '.join(names[:-1])} or {names[-1]} object")
        grp = optimizer.param_groups[0]
        if self.kind == KIND_RMSPROP and (grp.get('centered') or grp.get('maximize')):
            raise ValueError(f"{who}: centered and maximize are not supported with RMSprop")
        if grp.get('nesterov') or grp.get('dampening') or grp.get('amsgrad') or grp.get('maximize'):
            raise ValueError(f"{who}: nesterov, dampening, amsgrad and maximize are not supported")
        self.optimizer = optimizer
        self.state1 = [torch.zeros_like(p) for p in self.params]             # SGD: momentum_buffer; Adam: exp_avg; RMSprop: square_avg
        self.state2 = [torch.zeros_like(p) for p in self.params] if self.kind in state2_kinds else []      # Adam: exp_avg_sq; RMSprop: momentum_buffer
        self.hyper64 = torch.zeros(5, dtype=torch.float64, device=self.dev)      # [lr, momentum | beta1, beta2 | alpha, eps, weight_decay]
        self._hyper_host = [None] * 5
        self.steps = torch.zeros(2, dtype=torch.int64, device=self.dev)          # the optimizer's step count: steps[_tpar] is current
        self._tpar = 0
        n = len(self.params)
        self._s1p = (ctypes.c_void_p * n)(*[v.data_ptr() for v in self.state1])
        self._s2p = (ctypes.c_void_p * n)(*[v.data_ptr() for v in self.state2]) if self.state2 else None
        self.sync_hyper()

    def state_tensors(self):
        return list(self.state1) + list(self.state2)

    def step_count(self):
        """The optimizer's step count (waits for the device)."""
        return int(self.steps[self._tpar].item())

    def _reset_state(self):
        """A new voter that does not carry the previous one's state: zero states, step count 0."""
        for v in self.state_tensors():
            v.zero_()
        self.steps.zero_()
        self._tpar = 0

    def sync_hyper(self):
        """Copy the torch optimizer's current group to the device (before every epoch: the schedulers act on that object)."""
        grp = self.optimizer.param_groups[0]
        if self.kind == KIND_SGD:
            vals = [grp['lr'], grp['momentum'], 0.0, 0.0, grp['weight_decay']]
        elif self.kind == KIND_RMSPROP:
            vals = [grp['lr'], grp['momentum'], grp['alpha'], grp['eps'], grp['weight_decay']]
        else:
            vals = [grp['lr'], grp['betas'][0], grp['betas'][1], grp['eps'], grp['weight_decay']]
        for i, v in enumerate(vals):
            v = float(v)
            if v != self._hyper_host[i]:
                self.hyper64[i:i + 1].fill_(v)    # (fill_ on a view: no host-to-device copy from pageable memory, FusedLinearTrainer.begin_voter)
                self._hyper_host[i] = v

    def _opt_state(self):
        """The idl_opt_state_t of the next last launch: it reads the step count from steps[_tpar] and writes the other word; _step_taken() after it
        swaps their roles."""
        return _lib.idl_opt_state_t(self.kind, self._s1p, self._s2p, _p(self.hyper64), _p(self.steps[self._tpar:]), _p(self.steps[1 - self._tpar:]))

    def _step_taken(self):
        self._tpar ^= 1


class FusedLinearOptTrainer(_OptimizerState, _LinearStepParts):
    def __init__(self, net, optimizer, weight, lamb, seed=0):
        """optimizer: the torch.optim.SGD / torch.optim.Adam / torch.optim.RMSprop object whose first group holds the hyperparameters (its state is not used)."""
        self._init_network(net, weight, lamb, seed)     # (gradients as FusedLinearTrainer keeps them)
        self._init_optimizer(optimizer, kinds=(KIND_SGD, KIND_ADAM, KIND_RMSPROP), state2_kinds=(KIND_ADAM, KIND_RMSPROP))

    def begin_voter(self, voter, keep_state=False):
        """Dropout stream of voter v as FusedLinearTrainer.begin_voter sets it (ctl[0] starts at v << 24: voter v draws what it draws under
        RMSprop).  keep_state: the previous voter's optimizer state stays (IDELUCS_VOTER_STATE=carry); the step count is part of it."""
        self.ctl[0:1].fill_((int(voter) & 0xFF) << 24)
        if not keep_state:
            self._reset_state()

    def layer1_output(self, bf):
        """Layer 1's ReLU (+ Dropout) output of the last step on bf as an [m, 512] tensor (tests): the step forms whose layer-1 product is
        W1 x^T keep it transposed."""
        return bf.r1.view(self.H1, bf.m).t() if getattr(bf, "_r1_transposed", False) else bf.r1

    # ------------------------------------------------------------------ one step on a filled bf.xs[xi]
    def _opt(self, bf, r1, transposed, advance, st=None):
        """The step's last launch: dW2 = dlat^T r1 tiles + the optimizer on every tensor + step loss + counters (+ with st, the next batch from
        that store into bf.x: the whole batch, at the offset ctl[1] itself)."""
        nb = None if st is None else self._next_batch(st, bf.m, y=bf.x, base_add=0)
        _launch(_L.idl_opt_step_gather_wgrad, self._tail(bf, advance=advance, **self._wg(bf, r1, transposed)), self._opt_state(), nb, _stream())
        self._step_taken()

    def _dw1(self, bf, x):
        m, H1, F = bf.m, self.H1, self.F
        if _L.idl_wgrad_supported(m, H1, F):      # the dW1 tiles, gradient only
            _launch(_L.idl_wgrad_rmsprop, _p(bf.dr1), _p(x), m, H1, F, _p(self.grads[0]), None, None, None, _stream())
        else:
            torch.mm(bf.dr1.t(), x, out=self.grads[0])

    @torch.no_grad()
    def step_on_batch(self, bf, train=True, batch_advance=0, next_from=None, xi=0, defer_tail=False):
        """Forward, backward and the optimizer's update for the [m, F] batch in bf.xs[xi]; arguments as FusedLinearTrainer.step_on_batch
        (defer_tail, which _full_step passes on, has no meaning here: the step ends with its own last launch)."""
        tr, st = 1 if train else 0, next_from
        m, C, H1, F = bf.m, self.C, self.H1, self.F
        early = self._early(bf, st)                                 # the middle launches assemble the next batch into bf.xs[1 - xi]
        if not early:
            xi = 0                                                  # (otherwise the last launch does, into bf.x)
        both = early and C <= 48
        x, r1 = bf.xs[xi], bf.r1
        bf._r1_transposed = both
        if both and _L.idl_l1_fwd_supported(m, H1, F) and _L.idl_wgrad_supported(m, H1, F):
            _launch(_L.idl_l1_fwd, _p(self.W1), _p(x), m, F, _p(r1.view(H1, m)), _stream())
            self._tiles_middle(_launch, bf, tr, st, xi, r1)
        else:
            # (48 < n_clusters <= 200 with the fused InfoNCE kernels: the joint rides in InfoNCE pass 1 and the IIC core writes z dP0 -- two
            #  launches and one library product fewer than joint + core + z dP0 as a GEMM, which FusedLinearTrainer._step_general still runs)
            self._general_fwd_bwd(bf, tr, batch_advance, st, xi, k=_launch, mm=_mm_now, dz=bf.nce_fused and 48 < C <= 200, dw2=False)
        # ---- dW1, then the optimizer (dW2 inside its launch)
        self._dw1(bf, x)
        if early:
            self._opt(bf, r1, int(both), m // 2)
        elif st is not None:        # the offset moved mid-step: the last launch assembles the next batch into bf.x
            self._opt(bf, r1, 0, 0, st=st)
        else:
            self._opt(bf, r1, 0, batch_advance)

    # ------------------------------------------------------------------ one epoch over the store
    @torch.no_grad()
    def run_epoch(self, store, batch_sz, use_graph=True, generator=None):
        """One pass over a fresh permutation of the N*n_mimics pairs (models.py:117-133) -> (device scalar sum of the step losses,
        number of batches).  Full batches replay a captured graph of an even number of steps; what does not fill a replay and the partial
        last batch run eagerly."""
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
            self._gather(store, bf)             # batch 0; every later one is assembled by the step before it
            done = 0
            if use_graph and n_full >= 4:
                per = min(STEPS_PER_GRAPH, (n_full - 2) // 2 * 2)
                # every address the captured launches bake in is part of the key, and so is the role of the two step words
                base = (2 * batch_sz, store.feats.data_ptr(), store.mean.data_ptr(), store.scale.data_ptr(), store.inv_scale.data_ptr(),
                        self._perm.data_ptr(), store.n, store.f, store.n_pairs, per)
                key = base + (self._tpar,)
                g = self._graphs.get(key)
                if g is None:
                    for i in range(2):           # (two real steps first: whatever a library product sets up lazily happens outside the capture)
                        self._full_step(store, bf, pipelined=True, xi=i)
                    done = 2
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for i in range(per):
                            self._full_step(store, bf, pipelined=True, xi=i % 2)
                    self._graphs = {k_: v for k_, v in self._graphs.items() if k_[:-1] == base}      # one store at a time
                    self._graphs[key] = g
                    self.n_captures = getattr(self, "n_captures", 0) + 1
                reps = (n_full - done) // per
                for _ in range(reps):
                    g.replay()
                done += reps * per
            for i in range(done, n_full):
                self._full_step(store, bf, pipelined=True, xi=i % 2)
        if rem:
            self._full_step(store, self.buffers(2 * rem))
        return self.out[1], n_full + (1 if rem else 0)
