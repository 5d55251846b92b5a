"""idelucs_amd.fused -- the explicit, fused optimizer step for the default configuration
(NetLinear encoder + RMSprop), replayed as a HIP graph.

One step of reference idelucs/models.py:117-133 takes one of five launch sequences (FusedLinearTrainer._form picks it once per step):
    planes       (default, n_clusters <= 48) the two big products on the fp16 matrix cores from two-plane operands:
                 idl_l1_planes_rows -> idl_reduce_mid_fwd_gather_planes (the partial sums and the forward middle in one launch) -> idl_nce_fused_iic_z
                 -> idl_mid_bwd_gather -> idl_wgrad_xplanes_rms (dW1 with RMSprop in the tiles' epilogue, the optimizer's tail on their loader
                 waves); recorded, or with another ending: idl_l1_planes -> idl_reduce_parts_rms -> idl_mid_fwd_gather -> ...
    planes_rows  the same for n_clusters > 48 (the fine-grained mode's 200 output units: joint + IIC core with z dP0, dW3 on idl_at_b)
    tiles        IDELUCS_PLANES=0 (or shapes the planes do not take): own fp32 tiles, idl_l1_fwd -> idl_mid_fwd_gather -> InfoNCE + IIC ->
                 idl_mid_bwd_gather -> idl_wgrad_rmsprop; the optimizer's tail rides in the NEXT step's layer-1 launch (idl_l1_fwd_rms)
    record_planes, record_planes_rows (48 < n_clusters <= 200)  the SAME bodies (_step_planes, _step_planes_rows) issued through the recorder
                 for BatchedLinearTrainer: every launch recorded instead of performed, no step state kept
    general      everything else on library GEMMs + the unfused kernels: a lockstep step on batched fp32 GEMMs, n_clusters > 48 in fp32,
                 partial batches and the shapes the own tiles do not take
(DESIGN.md 4.4 has the table of what each launch carries).  Batches are assembled from the HBM feature store at a device-resident
offset that the step advances, the next batch by spare workgroups of the middle launches into the other of two x buffers, so an
epoch is replays of one captured single-stream graph of several steps with no host work between.

The parameters remain the nn.Parameters of model.net (state_dict / predict / weights_init unchanged).
RMSprop state lives here; begin_voter() clears it (every voter is an independent run, models.IID_model.begin_voter).

BatchedLinearTrainer steps several voters of one ensemble in lockstep: the layer-1 product becomes a batched GEMM and each of
the other kernels ONE launch with the voter index in its grid (recorded launches, idl_plan_*; in the two-plane form all six
launches, at 48 < n_clusters <= 200 all eight), so the latency-bound launches are paid once per step of the whole batch of voters
instead of once per voter.
"""
import ctypes
import os
import sys

import torch

from . import _lib
from ._lib import lib as _L

EPS = sys.float_info.epsilon
TEMPERATURE = 0.85          # hard-coded at the reference call site, models.py:128


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_PLANES_DISABLED = False


def planes_default():
    """Whether a new trainer takes the two-plane step form: IDELUCS_PLANES (default on) unless a run of this process already left the planes' range
    (disable_planes: training.train_voter's fall-back)."""
    return os.environ.get("IDELUCS_PLANES", "1") != "0" and not _PLANES_DISABLED


# Launch-sequence variants kept because tests or the training policy compare them with the default form (each was measured and not adopted:
# DESIGN, History).  They are NOT environment switches: a test sets an entry with monkeypatch.setitem(fused.VARIANTS, ...) before it builds a trainer.
VARIANTS = {
    "test_cold": "0",        # 1: a 512 MB fill in front of the hand-scheduled launches (tests/test_gpu_planes.py::test_cold_caches_*)
    "lockstep_planes": "1",  # 0: a rank's voters in lockstep on batched fp32 library GEMMs
    "planes_wgrad": "1",     # 0: dW1 on the fp32 tiles (writing W1's planes) beside the two-plane layer 1
    "planes_tail": "wgrad",  # reduce: the optimizer tail beside the next step's partial sums instead of on the dW1 tiles' loader waves
    "sums_fwd": "1",         # 0: the lone step's forward middle as a launch of its own behind the partial sums (seven launches a step instead of six)
    "fused": "1",            # 0: models.IID_model trains NetLinear + RMSprop through torch autograd instead of the fused explicit step
}
VARIANTS.update({k: v for k, v in _lib.DEV.items() if k in VARIANTS})
STEPS_PER_GRAPH = 16         # steps a replayed graph carries (between two replays the GPU idles ~9 us)
GATHER_SPLIT = 4             # eighths of the next batch's tiles the mid-forward launch assembles (the rest: mid-backward) at n_clusters <= 48
PLANES_MAX_ROWS = 60_000_000  # feature-store rows the two-plane form's batch assembly takes


def _v(name):
    return VARIANTS[name]


def disable_planes():
    """From here on every trainer of this process runs the fp32 tiles (the data left the fp16 planes' range once: it will again)."""
    global _PLANES_DISABLED
    _PLANES_DISABLED = True


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# idl_mid_bwd_gather's dr1_hi, dr1_lo, dr1_scale, dr1_overflow_flag and z_dP0 when dr1 is the fp32 tensor alone and the kernel forms z dP0 itself
_DR1_FP32 = (None,) * 5


def _tile_per_cu(H1, F, cus):
    """Whether the dW1 launch has a tile per CU and one CU for each block of the optimizer's tail on its loader waves (idl_wgrad_xplanes_rms)."""
    return 144 <= (H1 // 64) * (F // 128) <= cus


def rows_shape_applies(m, H1, F, cus):
    """Whether a batch shape takes the two-plane step of n_clusters > 48 (FusedLinearTrainer._step_planes_rows, lone or recorded): the layer-1
    tiles with the operands' roles swapped, dW1 from the batch's planes, a dW1 tile per CU with one for each block of the tail on its loader waves."""
    return bool(_L.idl_l1_planes_supported(H1, m, F)) and bool(_L.idl_wgrad_xplanes_supported(m, H1, F)) and _tile_per_cu(H1, F, cus)


def rows_lockstep_applies(m, H1, F, C, n_rows, cus):
    """Whether the voters of a NetLinear(F, C) trained on full batches of m rows can run in lockstep at 48 < C <= 200 (the form 'record_planes_rows' of
    a trainer built now): decided from the shape and the process's settings alone, before any trainer exists (training.can_batch)."""
    return (48 < C <= 200 and planes_default() and _v("lockstep_planes") != "0" and _v("planes_wgrad") != "0" and _v("planes_tail") != "reduce"
            and m % 16 == 0 and F % 4 == 0 and n_rows < PLANES_MAX_ROWS and _L.idl_nce_fused_workspace(m) > 0 and rows_shape_applies(m, H1, F, cus))


def _resident(st):
    """Whether st keeps its rows in HBM (utils.FeatureStore, or any object with its fields) -- else a utils.StreamedFeatureStore."""
    return getattr(st, "resident", True)


def _addresses(st):
    """Every address a launch on st bakes in: part of a captured graph's key."""
    if hasattr(st, "addresses"):
        return st.addresses()
    return tuple(t.data_ptr() for t in (st.feats, st.mean, st.scale, st.inv_scale))


def _launch(fn, *args):
    """One kernel launch, performed now (the launcher of launch_losses outside a recording)."""
    _lib.check(fn(*args))


def _mm_now(a, b, out):
    """One library product, performed now (beside _launch what FusedLinearTrainer._mm / _k are while nothing is recorded)."""
    torch.mm(a, b, out=out)


def launch_losses(k, bf, lamb, weight, out, dz=False):
    """InfoNCE on bf.f and IIC on bf.z of one step (FusedLinearTrainer and fused_small.FusedSmallTrainer), each kernel through the
    launcher k(fn, *args).  dz: the IIC core writes z dP0 to bf.dzs (idl_iic_core_dz) instead of dP0 to bf.P0, for a middle backward
    that takes it per row."""
    m, C = bf.m, bf.P0.shape[0]
    if bf.nce_fused and C <= 48:
        # the IIC workgroup of InfoNCE pass 1 forms the joint z1^T z2 itself (MFMA tiles) before the core
        k(_L.idl_nce_fused_iic_z, _p(bf.f), m, TEMPERATURE, _p(bf.lse), _p(bf.loss_rows), _p(bf.G), _p(bf.nce_ws), _p(bf.z), _p(bf.P0), C,
          lamb, EPS, weight, _p(bf.iic_scratch), _p(out), _stream())
    elif bf.nce_fused and dz:
        # the joint's 16 x 16 tiles ride in InfoNCE pass 1 as spare workgroups; then the IIC core's first launch and z dP0 with the
        # gradient's shift in its epilogue (no shift launch, no library GEMM)
        k(_L.idl_nce_fused_joint, _p(bf.f), m, TEMPERATURE, _p(bf.lse), _p(bf.loss_rows), _p(bf.G), _p(bf.nce_ws), _p(bf.z), _p(bf.P0), C, _stream())
        k(_L.idl_iic_core_dz, _p(bf.P0), C, lamb, EPS, weight, _p(bf.iic_scratch), _p(out), _p(bf.z), m, _p(bf.dzs), _stream())
    else:
        k(_L.idl_iic_joint, _p(bf.z), m, C, _p(bf.P0), _stream())       # (a library GEMM here: 118 us untuned at C = 200)
        if dz:
            k(_L.idl_iic_core_dz, _p(bf.P0), C, lamb, EPS, weight, _p(bf.iic_scratch), _p(out), _p(bf.z), m, _p(bf.dzs), _stream())
        else:
            k(_L.idl_iic_core, _p(bf.P0), C, lamb, EPS, weight, _p(bf.iic_scratch), _p(out), _stream())
        if bf.nce_fused:       # S = f f^T, lse, E + E^T and (E + E^T) f in two MFMA kernels, S never written
            k(_L.idl_nce_fused, _p(bf.f), m, TEMPERATURE, _p(bf.lse), _p(bf.loss_rows), _p(bf.G), _p(bf.nce_ws), _stream())
        else:                  # (m not a multiple of 32, or above the fused kernels' 2048 rows)
            torch.mm(bf.f, bf.f.t(), out=bf.S)
            k(_L.idl_nce_rows, _p(bf.S), m, TEMPERATURE, _p(bf.lse), _p(bf.loss_rows), _stream())
            torch.mm(bf.S, bf.f, out=bf.G[0])                            # (E + E^T) f


class _Buffers:
    """Activations / gradients of one batch shape (m = 2*B rows)."""

    def __init__(self, m, F, H1, H2, C, dev, shared=None):
        """shared: {'xs0', 'xs1', 'r1', 'dr1'} = this voter's slices of a BatchedLinearTrainer's stacked GEMM operands."""
        f32 = dict(dtype=torch.float32, device=dev)
        sh = shared or {}
        self.m = m
        # the batch of this step / the next one being assembled
        self.xs = [sh['xs0'] if 'xs0' in sh else torch.empty((m, F), **f32), sh['xs1'] if 'xs1' in sh else torch.empty((m, F), **f32)]
        self.x = self.xs[0]
        self.r1 = sh['r1'] if 'r1' in sh else torch.empty((m, H1), **f32)        # Linear1 output, then ReLU+Dropout in place
        self.r1T = self.r1.view(H1, m)                # the same memory as the transposed image [H1, m] (one of the two is in use)
        # tail-in-layer-1 (FusedLinearTrainer's tiles form): the layer-1 launch of step t + 1 writes its activations while riders of the
        # same launch still read step t's (dW2 = dlat^T r1), so the steps alternate between two images; made on first use
        self._r1_other = None
        self._H1 = H1
        self.lat = torch.empty((m, H2), **f32)
        self._dims = (m, H2, dev)
        self.f = torch.empty((m, H2), **f32)
        self.inv = torch.empty((m,), **f32)
        self.r2 = torch.empty((m, H2), **f32)
        self.z = torch.empty((m, C), **f32)
        self.nce_ws_bytes = _L.idl_nce_fused_workspace(m)            # -1: shape not supported by the fused InfoNCE kernels
        self.nce_fused = self.nce_ws_bytes > 0
        self.S = torch.empty((1, 1) if self.nce_fused else (m, m), **f32)
        self.lse = torch.empty((m,), **f32)
        self.loss_rows = torch.empty((m,), **f32)
        self.nce_parts = _L.idl_nce_fused_parts()
        self.G = torch.empty((self.nce_parts if self.nce_fused else 1, m, H2), **f32)
        self.nce_ws = torch.empty(max(self.nce_ws_bytes, 4) // 4, **f32)
        self.P0 = torch.empty((C, C), **f32)
        self.iic_scratch = torch.empty((C * C + 2 * C,), **f32)
        self.dlogits = torch.empty((m, C), **f32)
        self.dzs = torch.empty((m, C), **f32) if C > 48 else None       # z dP0 (fine-grained mode)
        self.dlat = torch.empty((m, H2), **f32)
        self.dr1 = sh['dr1'] if 'dr1' in sh else torch.empty((m, H1), **f32)


def _r1_of(bf, xi):
    """The layer-1 activation image of a step of parity xi ([m, H1]; the transposed image is the same memory)."""
    if xi == 0:
        return bf.r1
    if bf._r1_other is None:
        bf._r1_other = torch.empty_like(bf.r1)
    return bf._r1_other


def _r1T_of(pb, bf, xi):
    """The transposed activations [H1, m] of a step of parity xi whose sums launch carries the forward middle (VARIANTS['sums_fwd']), made on first use."""
    if pb["r1T"][xi] is None:
        pb["r1T"][xi] = torch.empty((bf._H1, bf.m), dtype=torch.float32, device=bf.f.device)
    return pb["r1T"][xi]


def _planes_of(bf, F):
    """Buffers of the two-plane step form (FusedLinearTrainer._planes), made on first use: the two batches' fp16 planes and the
    two images of idl_l1_planes' K-slice partial sums [8][H1][m] (slab 0 of an image becomes the step's transposed activations)."""
    if getattr(bf, "_planes", None) is None:
        m, H2, dev = bf._dims
        h16 = dict(dtype=torch.int16, device=dev)
        bf._planes = {"xh": [torch.empty((m, F), **h16) for _ in range(2)], "xl": [torch.empty((m, F), **h16) for _ in range(2)],
                      "part": [torch.empty((int(_L.idl_l1_planes_parts()), bf._H1, m), dtype=torch.float32, device=dev) for _ in range(2)],
                      "dh": torch.empty((m, bf._H1), **h16), "dl": torch.empty((m, bf._H1), **h16),      # dr1 as planes (mid_bwd -> the dW1 tiles)
                      "r1T": [None, None],              # sums_fwd: a parity's activations [H1, m] (its partial sums stay as they are)
                      "valid": [False, False],          # valid[i]: xh[i] / xl[i] hold the planes of the batch in bf.xs[i]
                      "x32": [True, True]}              # x32[i]: bf.xs[i] itself holds that batch (False: it was assembled as planes only)
    return bf._planes


class _Recorder:
    """step_on_batch in record mode: the big products are skipped (the batched trainer runs them as batched GEMMs) and every
    kernel launch is recorded as a plan (idl_plan_begin / idl_plan_end) instead of being performed."""

    def __init__(self):
        self.plans = []          # uint8 host tensors [PLAN_BYTES], in launch order
        self.mms = 0

    def launch(self, fn, *args):
        blob = torch.zeros(int(_L.idl_plan_bytes()), dtype=torch.uint8)
        _lib.check(_L.idl_plan_begin(ctypes.c_void_p(blob.data_ptr())))
        rc = fn(*args)
        end = _L.idl_plan_end()
        _lib.check(rc)
        _lib.check(end)
        self.plans.append(blob)


class _LinearStepParts:
    """What every explicit NetLinear step shares whichever optimizer ends it (FusedLinearTrainer; fused_opt.FusedLinearOptTrainer): the
    buffers of a batch shape, the argument lists of the optimizer-free launches, the prologue gather and the two ways a step is issued.
    _init_network provides the network's tensors and shapes, grads / parts, weight, ctl and the launches' pointer arrays; a user adds its
    optimizer's state and step_on_batch."""

    _cold, _cold_buf = False, None       # (FusedLinearTrainer's test hook: a fill in front of the hand-scheduled launches)

    def _init_network(self, net, weight, lamb, seed, grad_w1=None, shared_buffers=None):
        """The part of __init__ that knows no optimizer.  grad_w1 / shared_buffers: a BatchedLinearTrainer's stacked dW1 slice and buffer views."""
        lin1, lin2, lin3 = net.layers[0], net.layers[3], net.classifier[2]
        self.net = net
        self.W1, self.b1, self.W2, self.b2, self.W3, self.b3 = lin1.weight, lin1.bias, lin2.weight, lin2.bias, lin3.weight, lin3.bias
        self.params = [self.W1, self.b1, self.W2, self.b2, self.W3, self.b3]
        self.dev = self.W1.device
        self.F, self.H1, self.H2, self.C = lin1.in_features, lin1.out_features, lin2.out_features, lin3.out_features
        if self.H1 != 512 or self.H2 != 64 or self.C > 256 or lin2.in_features != self.H1 or lin3.in_features != 64:
            raise ValueError(f"{type(self).__name__} needs NetLinear (hidden 512, latent 64) and n_clusters <= 256")
        # bias gradients are kept as COL_PARTS stacked partial column sums, added up inside the optimizer's launch
        self.parts = [1 if p.dim() == 2 else _L.idl_col_sum_parts() for p in self.params]
        # the last layer's weight gradient (C x 64) is produced as partials by the middle-backward launch when C <= 48
        if self.C <= 48:
            self.parts[4] = _L.idl_col_sum_parts()
        self.grads = [torch.zeros((q,) + tuple(p.shape), dtype=p.dtype, device=p.device) if q > 1 else torch.zeros_like(p)
                      for p, q in zip(self.params, self.parts)]
        if grad_w1 is not None:                  # this voter's slice of a BatchedLinearTrainer's stacked dW1
            assert tuple(grad_w1.shape) == tuple(self.W1.shape) and grad_w1.is_contiguous()
            self.grads[0] = grad_w1
        self.weight, self.lamb, self.seed = float(weight), float(lamb), int(seed) & (2 ** 64 - 1)
        self.ctl = torch.zeros(2, dtype=torch.int64, device=self.dev)        # [dropout step counter, batch offset]
        self.out = torch.zeros(4, dtype=torch.float32, device=self.dev)      # [step loss, running sum, nce, iic]
        self._bufs, self._graphs, self._perm = {}, {}, None
        self._shared_buffers = shared_buffers    # {m: {...}} views handed to _Buffers
        n = len(self.params)
        self._pp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in self.params])
        self._gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in self.grads])
        self._sz = (ctypes.c_int64 * n)(*[p.numel() for p in self.params])
        self._parts = (ctypes.c_int32 * n)(*self.parts)

    def gradient(self, i):
        """Gradient of parameter i as a tensor of the parameter's shape (sums the stacked partials)."""
        return self.grads[i].sum(0) if self.parts[i] > 1 else self.grads[i]

    def buffers(self, m):
        if m not in self._bufs:
            self._bufs[m] = _Buffers(m, self.F, self.H1, self.H2, self.C, self.dev, shared=(self._shared_buffers or {}).get(m))
        return self._bufs[m]

    def _next_batch(self, st, m, *, y=None, planes=(None, None), flag=None, part=0, part_end=8, parts=8, base_add=None):
        """The next batch's assembly by a launch (idl_next_batch_t): the store, the pair list and the offset -- ctl[1], which a middle launch
        reads before the step has advanced it (base_add: m // 2 rows on) --, the destination y and / or the two planes with their overflow flag,
        and the share [part, part_end) of `parts` this launch takes.
        A streamed store (utils.StreamedFeatureStore) has no rows to copy: the batch -- fp32, planes, or both, as asked for here -- is vectorised by ONE
        launch of its own (idl_vectorise_pairs_at / _planes_at), issued here, in front of the launch that would have carried share 0, so it reads the
        offset where that launch would have; the step's launches get no assembly at all (None: NULL)."""
        if not _resident(st):
            if self._rec_active():
                raise RuntimeError("a streamed feature store assembles the batches of a lone voter's step: its launch cannot be recorded for a lockstep batch")
            if part == 0:
                st.pairs_at(self._perm, self.ctl[1:], m // 2 if base_add is None else base_add, m // 2, st.n_pairs, y, planes, flag)
            return None
        return _lib.idl_next_batch_t(_p(st.feats), st.n, st.f, st.n * st.f, _p(self._perm), _p(self.ctl[1:]), m // 2 if base_add is None else base_add,
                                     st.n_pairs, m // 2, _p(st.mean), _p(st.scale), _p(st.inv_scale), _p(y), _p(planes[0]), _p(planes[1]), _p(flag),
                                     part, part_end, parts)

    _vp, hyper = None, None              # RMSprop's running averages and float hyperparameters (FusedLinearTrainer); another optimizer travels as idl_opt_state_t

    def _tail(self, bf, *, skip=-1, advance=0, **wg):
        """The optimizer's tail of the step on bf (idl_opt_tail_t): every tensor's RMSprop but tensor `skip`'s (0: W1, which dW1 tiles update), the
        step loss, the batch offset's advance, and the in-launch dW2 tiles where the caller adds them (**self._wg(...))."""
        return _lib.idl_opt_tail_t(count=len(self.params), params=self._pp, grads=self._gp, grad_parts=self._parts, square_avg=self._vp, sizes=self._sz,
                                   hyper=_p(self.hyper), ctl=_p(self.ctl), loss_rows=_p(bf.loss_rows), loss_m=bf.m, w_nce=1.0 - self.weight,
                                   w_iic=self.weight, out=_p(self.out), skip_index=skip, batch_advance=advance, **(wg or {"wg_index": -1}))

    def _wg(self, bf, r1, transposed):
        """The dW2 = dlat^T r1 tiles of an optimizer launch: idl_opt_tail_t's wg_* fields."""
        return dict(wg_index=2, wg_dy=_p(bf.dlat), wg_x=_p(r1), wg_x_transposed=transposed, wg_m=bf.m, wg_n_out=self.H2, wg_n_in=self.H1,
                    wg_grad=_p(self.grads[2]))

    def _mid_fwd_tensors(self, bf, tr):
        """The forward middle's weights, shape and dropout seed, and its outputs (the step counter goes between the two)."""
        return (_p(self.W2), _p(self.b2), _p(self.W3), _p(self.b3), bf.m, self.C, tr, self.seed), (_p(bf.f), _p(bf.inv), _p(bf.r2), _p(bf.z))

    def _mid_fwd_args(self, bf, tr):
        head, outs = self._mid_fwd_tensors(bf, tr)
        return (*head, _p(self.ctl), *outs)

    def _mid_bwd_args(self, bf, tr, r1, gW3):
        _, gb1, _, gb2, _, gb3 = self.grads
        m = bf.m
        return (_p(bf.z), _p(bf.r2), _p(bf.f), _p(bf.inv), _p(bf.G), bf.G.shape[0], _p(bf.P0), _p(self.W3), _p(self.W2), _p(r1), m, self.C, tr,
                (1.0 - self.weight) / (m * TEMPERATURE), _p(bf.dlogits), _p(bf.dlat), _p(bf.dr1), _p(gb1), _p(gb2), _p(gb3), _p(gW3))

    def _evict(self):
        if self._cold_buf is None:
            self._cold_buf = torch.empty(128 << 20, dtype=torch.float32, device=self.dev)
        self._cold_buf.fill_(1.0)

    def _tiles_middle(self, k, bf, tr, st, xi, r1):
        """The middle of a step at n_clusters <= 48 on fp32 operands, behind the layer-1 product W1 x^T in r1 ([H1, m]; mid_fwd adds the bias):
        mid_fwd + its share of the next batch (into bf.xs[1 - xi]), InfoNCE + IIC, mid_bwd + the rest of the next batch -- each through the
        launcher k."""
        m = bf.m
        y = bf.xs[1 - xi]
        k(_L.idl_mid_fwd_gather, _p(r1), _p(self.b1), 1, *self._mid_fwd_args(bf, tr), self._next_batch(st, m, y=y, part_end=GATHER_SPLIT), _stream())
        launch_losses(k, bf, self.lamb, self.weight, self.out)
        k(_L.idl_mid_bwd_gather, *self._mid_bwd_args(bf, tr, r1, self.grads[4]), 1, *_DR1_FP32, self._next_batch(st, m, y=y, part=GATHER_SPLIT), _stream())

    def _early(self, bf, st):
        """Whether the middle launches of a general step on bf assemble the next batch from st (else the step's last launch does, or nobody)."""
        return st is not None and bf.m % 16 == 0 and self.F % 4 == 0

    def _general_fwd_bwd(self, bf, tr, batch_advance, st, xi, *, k, mm, dz, dw2):
        """Forward and backward of the general step form on the batch in bf.xs[xi]: library products and the unfused kernels where a shape
        needs them.  An early step (_early): the middle launches assemble the next batch into bf.xs[1 - xi]
        (n_clusters <= 48: both of them, _tiles_middle; else the forward alone); otherwise the backward's last launch advances the batch offset
        by batch_advance and the caller's optimizer launch assembles the batch.  What the two callers do differently is an argument:
          k, mm  the launcher and the layer-1 product W1 x^T of an early step at n_clusters <= 48: FusedLinearTrainer's _k (in an early step;
                 else _launch) and _mm, both recordable; fused_opt's _launch / _mm_now
          dz     the IIC core writes z dP0 (launch_losses): fused_opt.FusedLinearOptTrainer.step_on_batch passes nce_fused and
                 48 < n_clusters <= 200, FusedLinearTrainer._step_general never -- it runs joint + core and, beyond 64 output units, z dP0
                 as a library product.  (The two have drifted apart; which one RMSprop should take is a measurement, not a refactor.)
          dw2    dW2 = dlat^T r1 as a library product here (FusedLinearTrainer when st is None: its idl_rmsprop_step has no dW2 tiles); else
                 it is left to the caller's last launch
        On return dr1 and every gradient but dW1 (and dW2 unless dw2) are written: dW1 and the optimizer are the caller's ending."""
        m, C, H1 = bf.m, self.C, self.H1
        early = self._early(bf, st)
        both = early and C <= 48
        x, r1 = bf.xs[xi], bf.r1
        _, gb1, gW2, gb2, gW3, gb3 = self.grads
        adv_ctl, adv = (_p(self.ctl), batch_advance) if (st is not None and not early) else (None, 0)
        # ---- forward
        if both:    # a1^T = W1 x^T: the orientation hipBLASLt runs this product fastest in; mid_fwd adds the bias
            mm(self.W1, x.t(), r1.view(H1, m))
        else:
            torch.addmm(self.b1, x, self.W1.t(), out=r1)
        if self._cold:
            self._evict()
        if both:
            self._tiles_middle(k, bf, tr, st, xi, r1)
            return
        if early:       # (n_clusters > 48: ALL of the next batch's tiles ride in the mid-forward launch)
            k(_L.idl_mid_fwd_gather, _p(r1), None, 0, *self._mid_fwd_args(bf, tr), self._next_batch(st, m, y=bf.xs[1 - xi]), _stream())
        elif m % 16 == 0:   # ReLU/Dropout + Linear(512,64) + head in one MFMA kernel
            k(_L.idl_mid_fwd, _p(r1), *self._mid_fwd_args(bf, tr), _stream())
        else:
            k(_L.idl_relu_dropout_fwd, _p(r1), r1.numel(), tr, self.seed, _p(self.ctl), 1, _stream())
            torch.addmm(self.b2, r1, self.W2.t(), out=bf.lat)
            k(_L.idl_head_fwd, _p(bf.lat), _p(self.W3), _p(self.b3), m, C, tr, self.seed, _p(self.ctl), _p(bf.f), _p(bf.inv), _p(bf.r2), _p(bf.z),
              _stream())
        launch_losses(k, bf, self.lamb, self.weight, self.out, dz=dz)
        # ---- backward
        if C <= 48:     # head backward + dr1 = dlat W2 (MFMA) + ReLU/Dropout backward + every bias gradient + dW3 in one launch
            k(_L.idl_mid_bwd, *self._mid_bwd_args(bf, tr, r1, gW3), adv_ctl, adv, _stream())
            if dw2:
                torch.mm(bf.dlat.t(), r1, out=gW2)
            return
        # (at n_clusters = 200 the per-row C x C products want all 256 CUs: separate kernels)
        head = (_p(bf.z), _p(bf.r2), _p(bf.f), _p(bf.inv), _p(bf.G), bf.G.shape[0])
        rest = (_p(self.W3), m, C, tr, (1.0 - self.weight) / (m * TEMPERATURE), _p(bf.dlogits), _p(bf.dlat), _stream())
        if dz or C > 64:    # z_partner dP0 for all rows from the IIC core, or as one GEMM, instead of 40 000 FMAs per row inside the kernel
            if not dz:
                torch.mm(bf.z, bf.P0, out=bf.dzs)
            k(_L.idl_head_bwd_dz, *head, _p(bf.dzs), *rest)
        else:
            k(_L.idl_head_bwd, *head, _p(bf.P0), *rest)
        torch.mm(bf.dlogits.t(), bf.r2, out=gW3)
        if dw2:
            torch.mm(bf.dlat.t(), r1, out=gW2)
        torch.mm(bf.dlat, self.W2, out=bf.dr1)
        # (one launch for the three bias gradients + the ReLU/Dropout backward of layer 1)
        k(_L.idl_bias_grads, _p(bf.dr1), _p(r1), H1, _p(gb1), _p(bf.dlat), self.H2, _p(gb2), _p(bf.dlogits), C, _p(gb3),
          m, tr, adv_ctl, adv, None, None, _stream())

    def _rec_active(self):
        return getattr(self, "_rec", None) is not None

    def _gather(self, store, bf):
        b = bf.m // 2
        if not _resident(store):      # the same entry as the steps' added launch
            store.pairs_at(self._perm, self.ctl[1:], 0, b, store.n_pairs, bf.x)
        else:
            _lib.check(_L.idl_gather_pairs_at(_p(store.feats), store.n, store.f, store.n * store.f, _p(self._perm), _p(self.ctl[1:]),
                                              b, _p(store.mean), _p(store.scale), _p(store.inv_scale), _p(bf.x), _stream()))
        if getattr(bf, "_planes", None) is not None:
            bf._planes["valid"][0] = False
            bf._planes["x32"][0] = True

    def _full_step(self, store, bf, train=True, pipelined=False, xi=0, defer_tail=False):
        """pipelined: bf.xs[xi] already holds this batch (assembled by the previous step, or by the prologue gather);
        this step assembles the next one (into bf.xs[1 - xi] when the middle launches do it, else into bf.x).
        defer_tail (run_epoch's steps): the step's optimizer tail may wait for the next step's first launch (flush_tail)."""
        if pipelined:
            # (a step that is not early assembles the next batch into bf.x in its last launch: every such step runs on bf.xs[0])
            self.step_on_batch(bf, train=train, batch_advance=bf.m // 2, next_from=store, xi=xi if self._early(bf, store) else 0, defer_tail=defer_tail)
        else:
            self._gather(store, bf)
            self.step_on_batch(bf, train=train, batch_advance=bf.m // 2)


class FusedLinearTrainer(_LinearStepParts):
    def __init__(self, net, lr, weight, lamb, weight_decay=0.01, alpha=0.99, eps=1e-8, seed=0, grad_w1=None, shared_buffers=None):
        self._init_network(net, weight, lamb, seed, grad_w1, shared_buffers)
        self._rec = None                         # a _Recorder while a BatchedLinearTrainer records this voter's launches
        self.square_avg = [torch.zeros_like(p) for p in self.params]
        self.hyper = torch.tensor([lr, alpha, eps, weight_decay, 1.0 - alpha], dtype=torch.float32, device=self.dev)
        # TEST HOOK (IDELUCS_DEV=test_cold=1; tests/test_gpu_planes.py): a 512 MB fill in front of the step's middle and of each plane kernel, so that every load of
        # the hand-scheduled kernels comes from HBM instead of a warm L2/MALL -- a load consumed before its wait is right when it landed
        # early and wrong when it did not (DESIGN.md History, round 5), and only cold caches show that
        self._cold = _v("test_cold") == "1"
        # Round 5, default (IDELUCS_PLANES=0: the fp32 tiles below; csrc/planes.h): the two big products on the fp16 matrix cores from operands kept
        # as two fp16 planes (22 significand bits a factor, three products, fp32 accumulators: closer to a float64 product than an fp32 GEMM) --
        # the batch's planes written by the workgroups that assemble it, W1's by the epilogue of the dW1 tiles that update it.  A step
        # 100.6 us against 111.0 at cfg2 (tools/bench_planes.py).  Needs a single voter's pipelined step,
        # m % 128 == 0 and F % 512 == 0; any other step runs the fp32 tiles.
        self._planes = planes_default()
        # ... and the same for a rank's voters in lockstep (BatchedLinearTrainer; IDELUCS_DEV=lockstep_planes=0: their products as batched fp32
        # library GEMMs instead): the six launches of the two-plane step recorded per voter and run once for all of them, blockIdx.y = voter
        # -- the lone voters' steps bit for bit (tests/test_gpu_planes.py), 47.5 / 45.4 / 43.6 ms a voter-epoch in batches of 2 / 4 / 8
        # against 54.2 alone (fp32 GEMMs: 58.9 / 54.8 / 52.6); at 48 < n_clusters <= 200 the eight launches of _step_planes_rows the same way
        # (recorded: 58.1 / 53.9 / 51.4 ms at 200 output units against 74.6 alone, tools/bench_lockstep_rows.py)
        self._planes_lockstep = _v("lockstep_planes") != "0"
        # ... and dW1 from the batch's planes too (csrc/wgrad_planes.hip); the assembling workgroups then write the planes ONLY
        self._planes_wgrad = _v("planes_wgrad") != "0"
        # ... whose loader waves run the step's optimizer tail under the tiles' epilogue (IDELUCS_DEV=planes_tail=reduce: the tail beside the
        # next step's partial sums instead, 9.4 us for that launch against 4.7)
        self._planes_tail_wgrad = _v("planes_tail") != "reduce"
        # ... and the forward middle inside the launch that adds the partial sums (lone voter, tail on the dW1 tiles: _step_planes)
        self._sums_fwd = _v("sums_fwd") == "1"
        self._cus = torch.cuda.get_device_properties(self.dev).multi_processor_count if self.dev.type == "cuda" else 0
        self._ctl_snap = torch.zeros(1, dtype=torch.int64, device=self.dev)       # the step counter as the step's reduce launch saw it (idl_wgrad_xplanes_rms)
        self._w1_planes = None                   # (W1 hi, W1 lo, overflow flag)
        # the words of dr1's scale (csrc/planes.h): [0] the exponent mid_bwd gave this step's planes, [1] the next step's (the dW1 launch derives it), [4..] maxima
        self._dr1_scale = torch.zeros(int(_L.idl_dr1_scale_words()), dtype=torch.int32, device=self.dev)
        self._dr1_scale[1:2].fill_(int(_L.idl_planes_exponent(2)))
        self._w1_planes_fresh = False
        self._keep_w1_grad = False               # tests: the dW1 tiles also write dW1 to grads[0]
        # Round 5, tail-in-layer-1 (the tiles form): the layer-1 product on this package's own tiles (idl_l1_fwd: no library build decides
        # its speed) and the optimizer's TAIL -- the dW2 tiles, the small tensors, step loss, step counter: 5.8 us behind the dW1 tiles
        # of the optimizer launch, where they cannot become resident beside a tile -- riding in the layer-1 launch of the NEXT step
        # (idl_l1_fwd_rms), where they have 30 us of slack.  A step then ends with the dW1 tiles alone; its tail is pending until the
        # next step's first launch, or flush_tail().
        self._pending = None                     # (buffers, parity) of the step whose tail has not run yet
        n = len(self.params)
        self._vp = (ctypes.c_void_p * n)(*[v.data_ptr() for v in self.square_avg])

    def begin_voter(self, voter, keep_state=False):
        """Dropout stream of voter v: the Philox counter word the kernels take from ctl[0] (its low 32 bits) starts at
        v << 24, so voters never share masks whichever rank runs them (16.7 M optimizer steps per voter, 256 voters).
        keep_state: the previous voter's RMSprop running averages stay (IDELUCS_VOTER_STATE=carry, models.IID_model)."""
        # (fill_ on a view, here and below: `tensor[i] = python_scalar` is a host-to-device copy from pageable memory, which holds the
        #  host until everything queued on the stream has run -- the vectoriser, when a voter begins right behind the store's build)
        self.ctl[0:1].fill_((int(voter) & 0xFF) << 24)
        self._dr1_scale[1:2].fill_(int(_L.idl_planes_exponent(2)))       # (a voter's first step does not inherit the last voter's gradient range)
        if keep_state:
            return
        for v in self.square_avg:               # a voter starts with fresh optimizer state (models.IID_model.begin_voter)
            v.zero_()

    def set_lr(self, lr):
        self.hyper[0:1].fill_(float(lr))

    def _k(self, fn, *args):
        """One kernel launch of the step: performed, or recorded while a BatchedLinearTrainer is recording."""
        if self._rec is not None:
            self._rec.launch(fn, *args)
        else:
            _lib.check(fn(*args))

    def _mm(self, a, b, out):
        if self._rec is not None:
            self._rec.mms += 1                   # the batched trainer runs the big products as batched GEMMs
        else:
            torch.mm(a, b, out=out)

    # ------------------------------------------------------------------ one step on a filled bf.x
    def _form(self, bf, st):
        """The launch sequence of a step on bf with next_from = st (module docstring): 'record_planes', 'record_planes_rows', 'planes',
        'planes_rows', 'tiles' or 'general'."""
        m, H1, F = bf.m, self.H1, self.F
        if st is None or m % 16 != 0 or F % 4 != 0:      # only a pipelined step's middle launches assemble the next batch
            return "general"
        planes = self._planes and st.n < PLANES_MAX_ROWS
        xplanes = bool(_L.idl_wgrad_xplanes_supported(m, H1, F))
        if self._rec is not None:
            if (self.C <= 48 and planes and self._planes_lockstep and bf.nce_fused and bool(_L.idl_l1_planes_supported(m, H1, F)) and xplanes
                    and _tile_per_cu(H1, F, self._cus)):
                return "record_planes"
            if (48 < self.C <= 200 and planes and self._planes_lockstep and self._planes_wgrad and self._planes_tail_wgrad and bf.nce_fused
                    and rows_shape_applies(m, H1, F, self._cus)):
                return "record_planes_rows"
            return "general"
        if self._shared_buffers:
            return "general"
        if self.C <= 48:
            if not (_L.idl_l1_fwd_supported(m, H1, F) and _L.idl_wgrad_supported(m, H1, F)):
                return "general"
            return "planes" if planes and bool(_L.idl_l1_planes_supported(m, H1, F)) else "tiles"
        if planes and self._planes_wgrad and self._planes_tail_wgrad and rows_shape_applies(m, H1, F, self._cus):
            return "planes_rows"
        return "general"

    @torch.no_grad()
    def step_on_batch(self, bf, train=True, batch_advance=0, next_from=None, xi=0, defer_tail=False):
        """Forward, backward and RMSprop update for the [m, F] batch in bf.xs[xi] (rows [0,m/2) "true", [m/2,m) "modified").
        Only enqueues work on the current stream.  next_from = a FeatureStore: the step advances the batch offset and also
        assembles the NEXT batch (into bf.xs[1 - xi] where its middle launches do it, else into bf.x).  defer_tail: a step of the
        planes / tiles forms may leave its optimizer tail pending for the next step's first launch (flush_tail)."""
        tr, st = 1 if train else 0, next_from
        form = self._form(bf, st)
        if form not in ("planes", "tiles", "record_planes", "record_planes_rows"):
            self.flush_tail()                   # (a step of another form: whatever is pending goes first; a recording touches nothing pending)
        if form in ("planes", "record_planes"):
            self._step_planes(bf, tr, st, xi, defer_tail)
        elif form in ("planes_rows", "record_planes_rows"):
            self._step_planes_rows(bf, tr, st, xi)
        elif form == "tiles":
            self._step_tiles(bf, tr, st, xi, defer_tail)
        else:
            self._step_general(bf, tr, batch_advance, st, xi)

    def _gw1(self):
        return _p(self.grads[0]) if self._keep_w1_grad else None

    def _reduce(self, part, m):
        """The sum of idl_l1_planes' eight K-slice partial sums, with no optimizer tail beside it."""
        self._k(_L.idl_reduce_parts_rms, _p(part), self.H1 * m, _p(self.ctl), _p(self._ctl_snap), None, _stream())

    def _check_x32(self, bf, xi):
        if getattr(bf, "_planes", None) is not None and not bf._planes["x32"][xi]:
            raise RuntimeError("the batch in this buffer was assembled as planes only: a step of another form cannot read it")

    def _fp32_step(self, bf, xi):
        """A step that updates W1 without its planes and assembles the next batch without them."""
        self._check_x32(bf, xi)
        self._w1_planes_fresh = False
        if getattr(bf, "_planes", None) is not None:
            bf._planes["valid"][1 - xi] = False

    def _leave_tail_pending(self, bf, xi, r1, defer_tail):
        """The dW1 tiles ended the step: the rest of the optimizer is pending for the next step's first launch."""
        self._pending = (bf, xi, r1)
        if not defer_tail:
            self.flush_tail()

    def _planes_operands(self, bf, pb, xi):
        """W1's planes and the overflow flag for a two-plane step on bf.xs[xi].  A lone step makes the planes it lacks (_prepare_planes); a
        recording performs nothing and only allocates them: BatchedLinearTrainer.run_epoch splits W1 and batch 0 after it has recorded."""
        if self._rec is not None:
            return self._w1_planes_of()
        self._prepare_planes(bf, pb, xi)
        return self._w1_planes

    def _step_planes(self, bf, tr, st, xi, defer_tail):
        """n_clusters <= 48, the two big products from two-plane operands: a1^T = W1 x^T as eight K-slice partial sums on the fp16 matrix
        cores, ONE launch that adds them up on every CU (beside the previous step's pending tail, if any), mid_fwd (its spare workgroups
        assemble the first half of the next batch AND its planes), InfoNCE + IIC, mid_bwd (the other half; dr1 as planes), the dW1 tiles.
        The lone step with the tail on the dW1 tiles (the default) has the sums and mid_fwd in ONE launch (VARIANTS['sums_fwd']): six launches.
        Lone, or recorded for BatchedLinearTrainer (self._rec: every launch through self._k becomes a record): a recording performs nothing
        and keeps no step state, and it is always the six launches with the tail on the dW1 tiles -- _form's recording branch asks for that
        shape and does not consult planes_wgrad / planes_tail, which choose among the lone step's endings only."""
        m, H1, F = bf.m, self.H1, self.F
        rec = self._rec is not None
        cold = self._cold and not rec           # (the fill is work: BatchedLinearTrainer._step evicts in front of the batched launches itself)
        pb = _planes_of(bf, F)
        xplanes, wide = bool(_L.idl_wgrad_xplanes_supported(m, H1, F)), _tile_per_cu(H1, F, self._cus)
        # (the lone-only endings below are unreachable while recording only as long as _form's recording branch asks for this shape)
        assert not rec or (xplanes and wide), "a recorded two-plane step ends with the tail on the dW1 tiles: _form must not record another shape"
        plw = xplanes and (rec or self._planes_wgrad)                   # dW1 from the batch's planes: both operands by LDS-DMA
        tail_on_wgrad = plw and wide and (rec or self._planes_tail_wgrad)
        if not plw:
            self._check_x32(bf, xi)
        part, x = pb["part"][xi], bf.xs[xi]
        # the sums launch carries the forward middle (six launches): the lone step with the tail on the dW1 tiles and no tail pending from another ending
        merged = self._sums_fwd and tail_on_wgrad and not rec and self._pending is None
        r1 = _r1T_of(pb, bf, xi) if merged else part[0]      # [H1, m]: (else) slab 0 of the partial sums, where mid_fwd leaves the activations
        if not rec:
            bf._l1_src = "r1T" if merged else "part"
        wh, wl, flag = self._planes_operands(bf, pb, xi)
        if cold:
            self._evict()
        self._k(_L.idl_l1_planes_rows if merged else _L.idl_l1_planes, _p(wh), _p(wl), F, _p(pb["xh"][xi]), _p(pb["xl"][xi]), F, m, H1, F, _p(part), _stream())
        nxt = dict(y=None if plw else bf.xs[1 - xi], planes=(pb["xh"][1 - xi], pb["xl"][1 - xi]), flag=flag)
        if merged:          # part[8][m][512] -> sums, ReLU / Dropout (r1), lat, head, softmax by workgroups of whole rows; the riders as in mid_fwd
            if cold:
                self._evict()
            head, outs = self._mid_fwd_tensors(bf, tr)
            _launch(_L.idl_reduce_mid_fwd_gather_planes, _p(part), _p(self.ctl), _p(self._ctl_snap), _p(r1), _p(self.b1), *head, *outs,
                    self._next_batch(st, m, part_end=GATHER_SPLIT, **nxt), _stream())
        else:
            if self._pending is not None and not rec:       # (a recording looks at no pending tail: a lockstep voter never leaves one)
                self._tail_launch(*self._pending, red=(part, H1 * m))
            else:
                self._reduce(part, m)
            if cold:
                self._evict()
            self._k(_L.idl_mid_fwd_gather, _p(part), _p(self.b1), 1, *self._mid_fwd_args(bf, tr), self._next_batch(st, m, part_end=GATHER_SPLIT, **nxt), _stream())
        launch_losses(self._k, bf, self.lamb, self.weight, self.out)
        self._k(_L.idl_mid_bwd_gather, *self._mid_bwd_args(bf, tr, r1, self.grads[4]), 1, *self._dr1_planes_args(pb, plw, flag),
                self._next_batch(st, m, part=GATHER_SPLIT, **nxt), _stream())
        if not rec:     # a recording assembled nothing: run_epoch records both parities between _gather (which clears valid[0]) and the split of
            #             batch 0, so a recording at parity 1 that set valid[0] would let the first step run on stale planes
            pb["valid"][1 - xi] = True
            pb["x32"][1 - xi] = not plw
        w1 = (None if rec else self._gw1(), _p(self.W1), _p(self.square_avg[0]))       # (a recorded dW1 launch never writes dW1 out)
        if tail_on_wgrad:
            # ... and THIS step's optimizer tail is run by the tiles' loader waves under the tiles' epilogue: nothing is pending
            if cold:
                self._evict()
            self._k(_L.idl_wgrad_xplanes_rms, *self._dy_planes_args(pb), _p(pb["xh"][xi]), _p(pb["xl"][xi]), F, m, H1, F, *w1, _p(wh), _p(wl), _p(flag),
                    self._tail(bf, skip=0, advance=m // 2, **self._wg(bf, r1, 1)), _stream())
            return
        if plw:
            _launch(_L.idl_wgrad_rmsprop_xplanes, *self._dy_planes_args(pb), _p(pb["xh"][xi]), _p(pb["xl"][xi]), F, m, H1, F, *w1, _p(self.hyper),
                    _p(wh), _p(wl), _p(flag), _stream())
        else:       # dW1 on the fp32 tiles; their epilogue writes the updated W1's planes for the next layer-1 product
            _launch(_L.idl_wgrad_rmsprop_planes, _p(bf.dr1), _p(x), m, H1, F, *w1, _p(self.hyper), _p(wh), _p(wl), _p(flag), _stream())
        self._leave_tail_pending(bf, xi, r1, defer_tail)

    def _step_planes_rows(self, bf, tr, st, xi):
        """n_clusters > 48 (the fine-grained mode's 200 output units), the two big products from two-plane operands: the layer-1 tiles with
        the operands' roles swapped give part[8][m][512] (activations NOT transposed), mid_fwd assembles the whole next batch as planes
        only, the IIC core writes z dP0, ONE launch for the rest of the middle backward (softmax / Linear(64,C) / normalise backward per
        row, dr1 = dlat W2 as planes for the dW1 tiles, every bias gradient), dW3 on idl_at_b, and the dW1 tiles with the whole
        optimizer tail on their loader waves end the step.  Lone, or recorded for BatchedLinearTrainer at 48 < n_clusters <= 200 (eight
        records, ten kernels): a recording performs nothing and keeps no step state (_step_planes)."""
        m, C, H1, F = bf.m, self.C, self.H1, self.F
        rec = self._rec is not None
        cold = self._cold and not rec
        pb = _planes_of(bf, F)
        part = pb["part"][xi]
        r1 = part.view(-1, m, H1)[0]            # [m, H1]: slab 0 of part[8][m][512]
        if not rec:
            bf._l1_src = "part_rows"
        wh, wl, flag = self._planes_operands(bf, pb, xi)
        if cold:
            self._evict()
        self._k(_L.idl_l1_planes, _p(pb["xh"][xi]), _p(pb["xl"][xi]), F, _p(wh), _p(wl), F, H1, m, F, _p(part), _stream())
        self._reduce(part, m)
        if cold:
            self._evict()
        nxt = dict(planes=(pb["xh"][1 - xi], pb["xl"][1 - xi]), flag=flag)
        # (the bias of Linear(F,512) is added here)
        self._k(_L.idl_mid_fwd_gather, _p(r1), _p(self.b1), 0, *self._mid_fwd_args(bf, tr), self._next_batch(st, m, part_end=GATHER_SPLIT, **nxt), _stream())
        # the core writes z dP0 up to 200 output units, a library product beyond them (lone only: _form records no wider head, and a
        # recording takes no library product)
        dz = rec or 48 < C <= 200
        launch_losses(self._k, bf, self.lamb, self.weight, self.out, dz=dz)
        if not dz:
            torch.mm(bf.z, bf.P0, out=bf.dzs)
        self._k(_L.idl_mid_bwd_gather, *self._mid_bwd_args(bf, tr, r1, None), 0, *self._dr1_planes_args(pb, True, flag, bf.dzs),
                self._next_batch(st, m, part=GATHER_SPLIT, **nxt), _stream())
        if not rec:     # (a recording assembled nothing: _step_planes)
            pb["valid"][1 - xi] = True
            pb["x32"][1 - xi] = False
        self._k(_L.idl_at_b, _p(bf.dlogits), C, _p(bf.r2), self.H2, m, C, self.H2, _p(self.grads[4]), self.H2, _stream())      # dW3 = dlogits^T r2
        if cold:
            self._evict()
        self._k(_L.idl_wgrad_xplanes_rms, *self._dy_planes_args(pb), _p(pb["xh"][xi]), _p(pb["xl"][xi]), F, m, H1, F, None if rec else self._gw1(),
                _p(self.W1), _p(self.square_avg[0]), _p(wh), _p(wl), _p(flag), self._tail(bf, skip=0, advance=m // 2, **self._wg(bf, r1, 0)), _stream())

    def _step_tiles(self, bf, tr, st, xi, defer_tail):
        """n_clusters <= 48 on the fp32 tiles: a1^T = W1 x^T on own tiles (the previous step's optimizer tail rides in the same launch),
        mid_fwd + its share of the next batch, InfoNCE + IIC, mid_bwd + the rest of the next batch, the dW1 tiles with RMSprop."""
        m, H1, F = bf.m, self.H1, self.F
        self._fp32_step(bf, xi)
        x, r1 = bf.xs[xi], _r1_of(bf, xi)
        bf._l1_src = "r1_of"
        if self._pending is not None:
            self._tail_launch(*self._pending, l1=(x, m, r1.view(H1, m)))
        else:
            _launch(_L.idl_l1_fwd, _p(self.W1), _p(x), m, F, _p(r1.view(H1, m)), _stream())
        if self._cold:
            self._evict()
        self._tiles_middle(_launch, bf, tr, st, xi, r1)
        _launch(_L.idl_wgrad_rmsprop, _p(bf.dr1), _p(x), m, H1, F, self._gw1(), _p(self.W1), _p(self.square_avg[0]), _p(self.hyper), _stream())
        self._leave_tail_pending(bf, xi, r1, defer_tail)

    def _step_general(self, bf, tr, batch_advance, st, xi):
        """Library GEMMs and the unfused kernels where a shape needs them (_general_fwd_bwd), then dW1 and RMSprop.  A pipelined step with
        m % 16 == 0 has the next batch assembled by its middle launches (n_clusters <= 48: both, the launches recordable for
        BatchedLinearTrainer; else the forward alone); any other pipelined step assembles it into bf.x in its optimizer launch."""
        m, H1, F = bf.m, self.H1, self.F
        early = self._early(bf, st)
        both = early and self.C <= 48
        k = self._k if early else _launch
        self._fp32_step(bf, xi)
        x, r1 = bf.xs[xi], bf.r1
        if self._rec is None:
            bf._l1_src = "r1_t" if both else "r1"
        self._general_fwd_bwd(bf, tr, batch_advance, st, xi, k=k, mm=self._mm, dz=False, dw2=st is None)
        # ---- dW1 on own MFMA tiles with RMSprop in their epilogue: at the head of the optimizer launch of a pipelined step, else a
        # launch of its own (a recorded step takes the tiles only inside its optimizer launch); dW1 as a GEMM where the tiles do not apply
        w1_tiles = bool(_L.idl_wgrad_supported(m, H1, F))
        skip = -1                               # the tensor the optimizer launch leaves out: W1 (0) once tiles have updated it
        if w1_tiles and not early and self._rec is None:
            _launch(_L.idl_wgrad_rmsprop, _p(bf.dr1), _p(x), m, H1, F, self._gw1(), _p(self.W1), _p(self.square_avg[0]), _p(self.hyper), _stream())
            skip = 0
        elif not (w1_tiles and early):
            self._mm(bf.dr1.t(), x, self.grads[0])
        # ---- RMSprop (and advance the device-side step counter / batch offset)
        if w1_tiles and early:
            k(_L.idl_wgrad_rmsprop_step, _p(bf.dr1), _p(x), m, H1, F, self._gw1(), self._tail(bf, skip=0, advance=m // 2, **self._wg(bf, r1, int(both))), _stream())
        elif early:     # no batch assembly here; the offset moves on at the end of the step
            k(_L.idl_rmsprop_step, self._tail(bf, skip=skip, advance=m // 2, **self._wg(bf, r1, int(both))), None, _stream())
        elif st is not None:    # the whole next batch into bf.x, at the offset the middle of the step has advanced
            _launch(_L.idl_rmsprop_step, self._tail(bf, skip=skip, **self._wg(bf, r1, 0)), self._next_batch(st, m, y=bf.x, base_add=0), _stream())
        else:
            _launch(_L.idl_rmsprop_step, self._tail(bf, skip=skip, advance=batch_advance), None, _stream())

    def _w1_planes_of(self):
        """W1's planes and the planes' overflow flag, made on first use."""
        if self._w1_planes is None:
            self._w1_planes = (torch.empty(self.W1.shape, dtype=torch.int16, device=self.dev), torch.empty(self.W1.shape, dtype=torch.int16, device=self.dev),
                               torch.zeros(1, dtype=torch.int32, device=self.dev))
        return self._w1_planes

    def _dr1_planes_args(self, pb, on, flag, dzs=None):
        """idl_mid_bwd_gather's arguments behind act1_transposed: dr1's planes and the words of their scale (or none of them: dr1 in fp32), the
        overflow flag they raise (the word the next batch's planes raise too) and z dP0 as an input (the step of n_clusters > 48)."""
        pb["dr1_as_planes"] = bool(on)
        return ((_p(pb["dh"]), _p(pb["dl"]), _p(self._dr1_scale)) if on else (None, None, None)) + (_p(flag), _p(dzs))

    def dr1_of(self, bf):
        """dr1 of the last step on these buffers as an fp32 tensor (tests): the step's own tensor, or -- where mid_bwd wrote it as planes only --
        the planes put back together."""
        pb = getattr(bf, "_planes", None)
        if pb is None or not pb.get("dr1_as_planes", False):
            return bf.dr1
        return ((pb["dh"].view(torch.float16).double() + pb["dl"].view(torch.float16).double()) * 2.0 ** -int(self._dr1_scale[0].item())).float()

    def layer1_output(self, bf, xi=0):
        """Layer 1's ReLU (+ Dropout) output of the last step on bf, run at parity xi, as an [m, 512] tensor (tests; no launch): the general
        form's bf.r1 (transposed where the product was W1 x^T), the tiles form's image of that parity, slab 0 of the parity's partial sums
        (transposed at n_clusters <= 48), or the transposed activations of a sums launch that carried the forward middle."""
        src = getattr(bf, "_l1_src", None)
        if src is None:
            raise RuntimeError("no step has run on these buffers")
        if src == "r1":
            return bf.r1
        if src == "r1_t":
            return bf.r1T.t()
        if src == "r1_of":
            return _r1_of(bf, xi).view(self.H1, bf.m).t()
        pb = bf._planes
        if src == "r1T":
            return _r1T_of(pb, bf, xi).t()
        return pb["part"][xi].view(-1, bf.m, self.H1)[0] if src == "part_rows" else pb["part"][xi][0].t()

    def _dy_planes_args(self, pb):
        return (_p(pb["dh"]), _p(pb["dl"]), _p(self._dr1_scale))

    def _tail_launch(self, bf, xi, r1, l1=None, red=None):
        """The optimizer's tail of the step that ran on (bf, xi) with the activations r1: dW2 tiles + RMSprop on every tensor but W1 + step
        loss + step counter -- behind the layer-1 tiles of the next step (l1 = (x, m, r1T) of THAT step), beside the workgroups that add up the next
        step's layer-1 partial sums (red), or as a launch of its own."""
        tail = self._tail(bf, skip=0, advance=bf.m // 2, **self._wg(bf, r1, 1))       # (without W1: the tiles' own launch updated it)
        if red is not None:       # beside the workgroups that add up the next step's layer-1 partial sums (red = (part, elements of a slab))
            part, slab = red
            _launch(_L.idl_reduce_parts_rms, _p(part), slab, None, None, tail, _stream())
        elif l1 is not None:
            x, m1, r1T = l1
            _launch(_L.idl_l1_fwd_rms, _p(self.W1), _p(x), m1, self.F, _p(r1T), tail, _stream())
        else:
            _launch(_L.idl_rmsprop_step, tail, None, _stream())
        self._pending = None

    def flush_tail(self):
        """Run the pending optimizer tail now (end of an epoch, before a step of another form, before anybody looks at the small
        tensors); a no-op when nothing is pending."""
        if self._pending is not None:
            bf, xi, r1 = self._pending
            self._tail_launch(bf, xi, r1)

    def _prepare_planes(self, bf, pb, xi):
        """Before a step of the two-plane form: W1's planes (made once; afterwards the dW1 tiles' epilogue keeps them) and the planes of the
        batch in bf.xs[xi] unless the step that assembled it wrote them."""
        wh, wl, flag = self._w1_planes_of()
        if not self._w1_planes_fresh:
            _lib.check(_L.idl_split_planes(_p(self.W1), self.W1.numel(), int(_L.idl_planes_exponent(1)), _p(wh), _p(wl), _p(flag), _stream()))
            self._w1_planes_fresh = True
        if not pb["valid"][xi]:
            x = bf.xs[xi]
            _lib.check(_L.idl_split_planes(_p(x), x.numel(), int(_L.idl_planes_exponent(0)), _p(pb["xh"][xi]), _p(pb["xl"][xi]), _p(flag), _stream()))
            pb["valid"][xi] = True

    def planes_overflowed(self):
        """Whether an entry of W1 (|w| >= 15.8) or of a standardised batch (|x| > 8 125: a mimic's feature thousands of the originals' standard
        deviations out) ever left its planes' range (waits for the device).  Such an entry was clamped in the two big products: the run
        should be repeated with IDELUCS_PLANES=0."""
        return self._w1_planes is not None and bool(self._w1_planes[2].item())

    def drop_planes(self):
        """Leave the two-plane step form for good (an operand left the planes' range): the fp32 tiles from the next step on, the flag cleared, the
        captured graphs (they hold the plane launches) dropped.  The caller restarts its voter: what was trained on clamped operands is not kept."""
        self.flush_tail()
        self._planes = False
        self._planes_lockstep = False
        self._graphs.clear()
        self._w1_planes_fresh = False
        if self._w1_planes is not None:
            self._w1_planes[2].zero_()
        for bf in self._bufs.values():
            if getattr(bf, "_planes", None) is not None:
                bf._planes["valid"] = [False, False]
                bf._planes["x32"] = [True, True]
                bf._planes["dr1_as_planes"] = False

    # ------------------------------------------------------------------ one epoch over the store
    @torch.no_grad()
    def run_epoch(self, store, batch_sz, use_graph=True, generator=None):
        """One pass over a fresh permutation of the N*n_mimics pairs (models.py:117-133).
        Returns the device scalar sum of the per-step losses and the number of batches."""
        n_pairs = store.n_pairs
        if self._perm is None or self._perm.numel() != n_pairs:
            self._perm = torch.empty(n_pairs, dtype=torch.int64, device=self.dev)
            self._graphs.clear()
        # (the permutation on a stream of its own beside the vectoriser was measured: the epoch 67.2-67.4 ms against 64.8-65.0 on the
        #  main stream, T_e2e 76.8-79.2 against 76.1-76.3 -- the step graphs wait for the other stream's event)
        torch.randperm(n_pairs, device=self.dev, generator=generator, out=self._perm)
        self._w1_planes_fresh = False           # (whoever set the weights since the last epoch -- a voter's initialisation -- did not write planes)
        self.ctl[1:2].zero_()
        self.out[1:2].zero_()
        n_full, rem = divmod(n_pairs, batch_sz)
        if n_full:
            bf = self.buffers(2 * batch_sz)
            self._gather(store, bf)             # prologue: batch 0; every later batch is assembled by the previous step
            if self._planes and bool(_L.idl_l1_planes_supported(bf.m, self.H1, self.F)):
                self._prepare_planes(bf, _planes_of(bf, self.F), 0)      # (a replayed graph starts from valid planes)
            # steps per graph replay: an even number when two x buffers alternate.  Between two replays the GPU idles ~9 us
            # (profiles/r02_f: kernel trace), so a replay carries several steps
            per = STEPS_PER_GRAPH
            while per > 2 and n_full < 2 + 2 * per:      # short epochs: the capture itself runs 2 + per real steps
                per = max(2, per // 4 * 2)
            # every address the captured launches bake in is part of the key (a store refitted in place keeps its graph)
            # (a streamed store: its packed bases, offsets, lengths, edits and edit ranges in place of feats)
            key = (2 * batch_sz, *_addresses(store), self._perm.data_ptr(), store.n, store.f, store.n_views, per)
            if use_graph and n_full >= 8:
                g = self._graphs.get(key)
                if g is None:
                    g = self._capture(store, bf, per)
                    self._graphs = {key: g}             # one store at a time: drop graphs of older stores
                    n_done = 2 + per                     # the warm-up + capture already ran real steps (an even number when per == 2)
                else:
                    n_done = 0
                for _ in range((n_full - n_done) // per):
                    g.replay()
                for i in range((n_full - n_done) % per):
                    self._full_step(store, bf, pipelined=True, xi=i % 2, defer_tail=True)
            else:
                for i in range(n_full):
                    self._full_step(store, bf, pipelined=True, xi=i % 2, defer_tail=True)
        self.flush_tail()                       # (the last eager step's tail; a replayed graph ends with its own)
        if rem:
            self._full_step(store, self.buffers(2 * rem))
        return self.out[1], n_full + (1 if rem else 0)

    @torch.no_grad()
    def _capture(self, store, bf, per):
        """Warm up on a side stream (2 real steps), then capture the next `per` real steps into a HIP graph.
        Every launch is a genuine optimizer step on the next batch, so nothing is wasted or repeated."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for i in range(2):
                self._full_step(store, bf, pipelined=True, xi=i % 2, defer_tail=True)
            self.flush_tail()
        torch.cuda.current_stream().wait_stream(s)
        # (tail-in-layer-1: a replay is self-contained -- its first step has nothing pending in front of it, its last step's tail is
        #  a launch of its own at the end of the graph: one more launch per `per` steps, and a replay never applies a tail twice)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(per):
                self._full_step(store, bf, pipelined=True, xi=i % 2, defer_tail=True)
            self.flush_tail()
        g.replay()          # capture does not execute: run the captured step(s) once
        self.n_captures = getattr(self, "n_captures", 0) + 1
        return g


class BatchedLinearTrainer:
    """Several voters of one ensemble trained in lockstep on one GPU (each on its own network, permutation, dropout stream and
    optimizer state -- the same independent runs as one after the other; only the rounding of the batched GEMMs may differ
    from the single-voter ones).

    The step of voter l is the launch sequence of FusedLinearTrainer.step_on_batch; here each of its launches is issued ONCE for
    all voters: the two big products as batched GEMMs over stacked operands ([L, 512, F] weights, [L, m, F] batches), the five
    kernels as recorded launches (idl_plan_*: every voter's launch is recorded through the ordinary launcher, the records
    live on the device, the kernels take the voter index from blockIdx.x / .y / .z); in the two-plane forms every launch of the
    step is a recorded one (six at n_clusters <= 48, eight at 48 < n_clusters <= 200) and the voters' steps are the lone voters'
    bit for bit.  n_clusters <= 48 takes either form; 48 < n_clusters <= 200 has the two-plane form only (rows_lockstep_applies:
    training.can_batch asks before it builds one), and beyond 200 output units voters train one after the other."""

    def __init__(self, nets, lr, weight, lamb, seed=0):
        if nets[0].classifier[2].out_features > 200:
            raise ValueError("BatchedLinearTrainer needs n_clusters <= 200 (beyond 48: on the two-plane step form, fused.rows_lockstep_applies)")
        self.L = L = len(nets)
        lin1 = [n.layers[0] for n in nets]
        self.dev = dev = lin1[0].weight.device
        H1, F = lin1[0].weight.shape
        f32 = dict(dtype=torch.float32, device=dev)
        # stacked GEMM operands; every voter's parameters / gradients / buffers are views of them
        self.W1s = torch.empty((L, H1, F), **f32)
        self.gW1s = torch.zeros((L, H1, F), **f32)
        for l, lin in enumerate(lin1):
            self.W1s[l].copy_(lin.weight.data)
            lin.weight.data = self.W1s[l]
        self._stacks = {}
        self._H1, self._F = H1, F
        self.trainers = []
        for l, net in enumerate(nets):
            self.trainers.append(FusedLinearTrainer(net, lr, weight, lamb, seed=seed, grad_w1=self.gW1s[l], shared_buffers=_SharedViews(self, l)))
        self._programs = {}
        self._graphs = {}
        self._w1_in_launch = False
        self._planes_step = False

    def planes_overflowed(self):
        """Whether any voter's operands left the planes' range (FusedLinearTrainer.planes_overflowed): every lane's flag in ONE read (waits for the device)."""
        flags = [t._w1_planes[2] for t in self.trainers if t._w1_planes is not None]
        return bool(flags) and bool(torch.cat(flags).any().item())

    def drop_planes(self):
        """After the voters' trainers left the two-plane form (FusedLinearTrainer.drop_planes): the recorded programs and captured graphs hold its launches."""
        self._programs = {}
        self._graphs.clear()
        self._planes_step = False

    def stack(self, m):
        """Stacked GEMM operands of batch shape m: XS[2][L, m, F], R1 [L, m, 512] (its transposed image [L, 512, m] is the layer-1
        product's output), DR1 [L, m, 512]."""
        if m not in self._stacks:
            f32 = dict(dtype=torch.float32, device=self.dev)
            self._stacks[m] = dict(xs=[torch.empty((self.L, m, self._F), **f32), torch.empty((self.L, m, self._F), **f32)],
                                   r1=torch.empty((self.L, m, self._H1), **f32), dr1=torch.empty((self.L, m, self._H1), **f32))
        return self._stacks[m]

    # ------------------------------------------------------------------ recording
    def _program(self, store, m):
        """The recorded launches of one pipelined step for the two x-buffer parities: [(host records [L, B], device records)] x 4."""
        key = (m, store.feats.data_ptr(), store.mean.data_ptr(), store.scale.data_ptr(), store.inv_scale.data_ptr(), store.n, store.f,
               store.n_views) + tuple(t._perm.data_ptr() for t in self.trainers)
        prog = self._programs.get(key)
        if prog is None:
            prog = []
            for xi in (0, 1):
                recs = []
                for t in self.trainers:
                    t._rec = _Recorder()
                    try:
                        t.step_on_batch(t.buffers(m), train=True, batch_advance=m // 2, next_from=store, xi=xi)
                    finally:
                        rec, t._rec = t._rec, None
                    # the two-plane step: six recorded launches (eight at 48 < n_clusters <= 200), no library GEMM; the fp32 form: 4 kernel launches +
                    # the two big products as batched GEMMs (dW1 on own tiles at the head of the optimizer launch is a recorded launch instead: one GEMM)
                    if (len(rec.plans), rec.mms) not in ((4, 2), (4, 1), (6, 0), (8, 0)):
                        raise RuntimeError("the recorded step is not the default launch sequence")
                    self._planes_step = rec.mms == 0
                    self._w1_in_launch = rec.mms == 1
                    recs.append(rec.plans)
                ops = []
                for k in range(len(recs[0])):
                    host = torch.stack([recs[l][k] for l in range(self.L)]).contiguous()
                    ops.append((host, host.to(self.dev)))
                prog.append(ops)
            self._programs = {key: prog}
            self._graphs.clear()
        return prog

    def _step(self, prog, st, xi):
        """One optimizer step of every voter on the batches in XS[xi] (assembling the next ones into XS[1 - xi])."""
        L = self.L
        ops = prog[xi]
        if self._planes_step:
            # l1, reduce, mid_fwd, InfoNCE passes, (IIC core + z dP0,) mid_bwd, (dW3,) dW1 + RMSprop + tail: every voter's, one launch each
            for k in range(len(ops)):
                if self.trainers[0]._cold:
                    self.trainers[0]._evict()
                _lib.check(_L.idl_plan_launch(ctypes.c_void_p(ops[k][0].data_ptr()), _p(ops[k][1]), L, _stream()))
            return
        k0 = 0
        r1T = st['r1'].view(L, self._H1, -1)
        torch.bmm(self.W1s, st['xs'][xi].transpose(1, 2), out=r1T)                        # a1^T = W1 x^T per voter
        for k in (k0, k0 + 1, k0 + 2):                                                   # mid_fwd, InfoNCE passes, mid_bwd
            _lib.check(_L.idl_plan_launch(ctypes.c_void_p(ops[k][0].data_ptr()), _p(ops[k][1]), L, _stream()))
        if not self._w1_in_launch:
            torch.bmm(st['dr1'].transpose(1, 2), st['xs'][xi], out=self.gW1s)            # dW1 = dr1^T x per voter
        _lib.check(_L.idl_plan_launch(ctypes.c_void_p(ops[k0 + 3][0].data_ptr()), _p(ops[k0 + 3][1]), L, _stream()))

    # ------------------------------------------------------------------ one epoch of every voter
    @torch.no_grad()
    def run_epoch(self, store, batch_sz, generators, use_graph=True):
        """One pass of every voter over its own fresh permutation -> [(device scalar sum of step losses, n_batches)] per voter."""
        n_pairs = store.n_pairs
        for t, g in zip(self.trainers, generators):
            if t._perm is None or t._perm.numel() != n_pairs:
                t._perm = torch.empty(n_pairs, dtype=torch.int64, device=self.dev)
            torch.randperm(n_pairs, device=self.dev, generator=g, out=t._perm)
            t.ctl[1:2].zero_()
            t.out[1:2].zero_()
        n_full, rem = divmod(n_pairs, batch_sz)
        m = 2 * batch_sz
        if n_full and m % 32 == 0:
            st = self.stack(m)
            for t in self.trainers:
                t._gather(store, t.buffers(m))            # prologue: batch 0 of every voter
            prog = self._program(store, m)
            if self._planes_step:                         # W1's planes (the weights were set since the last epoch) and those of every voter's batch 0
                for t in self.trainers:
                    t._w1_planes_fresh = False
                    bf = t.buffers(m)
                    t._prepare_planes(bf, _planes_of(bf, t.F), 0)
            per = STEPS_PER_GRAPH
            while per > 2 and n_full < 2 + 2 * per:
                per = max(2, per // 4 * 2)
            done = 0
            if use_graph and n_full >= 8:
                g = self._graphs.get((m, per))
                if g is None:
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        for i in range(2):
                            self._step(prog, st, i % 2)
                    torch.cuda.current_stream().wait_stream(s)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for i in range(per):
                            self._step(prog, st, i % 2)
                    g.replay()
                    self._graphs[(m, per)] = g
                    done = 2 + per
                for _ in range((n_full - done) // per):
                    g.replay()
                done += (n_full - done) // per * per
            for i in range(n_full - done):
                self._step(prog, st, i % 2)
        elif n_full:
            for t in self.trainers:
                for i in range(n_full):
                    t._full_step(store, t.buffers(m), pipelined=True, xi=i % 2)
        if rem:                                           # the partial last batch: voter by voter, the single-voter kernels
            for t in self.trainers:
                t._full_step(store, t.buffers(2 * rem))
        return [(t.out[1], n_full + (1 if rem else 0)) for t in self.trainers]


class _SharedViews:
    """{m: views} handed to a voter's _Buffers: its slices of the batched trainer's stacked GEMM operands (full batches only)."""

    def __init__(self, owner, l):
        self._owner, self._l = owner, l

    def get(self, m, default=None):
        if m % 32 != 0 or m < 64:
            return default
        st = self._owner.stack(m)
        l = self._l
        return dict(xs0=st['xs'][0][l], xs1=st['xs'][1][l], r1=st['r1'][l], dr1=st['dr1'][l])
