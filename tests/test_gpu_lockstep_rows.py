"""Lockstep training of a rank's voters at 48 < n_clusters <= 200 (the fine-grained mode's 200 output units): the eight launches of the
two-plane step of FusedLinearTrainer._step_planes_rows, the body the lone voters run, recorded per voter and run once for all voters
(BatchedLinearTrainer); and the six of _step_planes at n_clusters <= 48 held to the same bits.  The batched
kernels are the lone kernels' bodies on a voter's record, so everything here is compared with torch.equal, never within a tolerance.  Reference: the step of
idelucs/models.py:117-133, one voter after the other (idelucs/__main__.py:100-123)."""
import copy
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _variants():
    return __import__("idelucs_amd.fused", fromlist=["VARIANTS"]).VARIANTS


def _lockstep_is_lone(dev, monkeypatch, n, graph, lanes, C=200):
    """An epoch of `lanes` voters (weights scaled apart, dropout on, a generator each) alone and in lockstep: every parameter, every RMSprop running
    average, the loss sum and ctl are the same bits.  The form and the records per parity follow from C: planes_rows and eight beyond 48 output
    units, planes and six up to them.  -> the batched trainer."""
    import torch
    import test_gpu_encoder as E
    from idelucs_amd.fused import FusedLinearTrainer, BatchedLinearTrainer
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    monkeypatch.setitem(_variants(), "lockstep_planes", "1")
    store, net0 = E._cfg2_store_and_net(dev, n, seed=4, C=C)
    B = 512
    form, records = ("planes_rows", 8) if C > 48 else ("planes", 6)
    nets_a, nets_b = [], []
    for l in range(lanes):
        net = copy.deepcopy(net0)
        with torch.no_grad():
            for p_ in net.parameters():                       # different voters: different weights
                p_.mul_(1.0 + 0.05 * l)
        nets_a.append(net)
        nets_b.append(copy.deepcopy(net))
    single = []
    for l, net in enumerate(nets_a):
        tr = FusedLinearTrainer(net, lr=1e-3, weight=0.25, lamb=2.8, seed=11)
        tr.begin_voter(l)
        assert tr._form(tr.buffers(2 * B), store) == form
        gen = torch.Generator(device=dev); gen.manual_seed(100 + l)
        total, nb = tr.run_epoch(store, B, use_graph=graph, generator=gen)
        torch.cuda.synchronize()
        assert not tr.planes_overflowed()
        single.append((total.clone(), nb, [p_.detach().clone() for p_ in tr.params], [v.clone() for v in tr.square_avg], tr.ctl.clone()))
        del tr
    bt = BatchedLinearTrainer(nets_b, lr=1e-3, weight=0.25, lamb=2.8, seed=11)
    gens = []
    for l, tr in enumerate(bt.trainers):
        tr.begin_voter(l)
        g = torch.Generator(device=dev); g.manual_seed(100 + l)
        gens.append(g)
    res = bt.run_epoch(store, B, gens, use_graph=graph)
    torch.cuda.synchronize()
    # the feature was exercised: the recorded two-plane step, eight (six) records per parity, nothing left the planes' range, one captured graph
    assert bt._planes_step and bt.L == lanes
    prog = next(iter(bt._programs.values()))
    assert [len(ops) for ops in prog] == [records, records]
    assert not any(t.planes_overflowed() for t in bt.trainers) and not bt.planes_overflowed()
    assert len(bt._graphs) == (1 if graph else 0)
    for l, ((total, nb), tr) in enumerate(zip(res, bt.trainers)):
        want_total, want_nb, want_params, want_avg, want_ctl = single[l]
        print(f"voter {l}: loss sum {total.item()!r} (alone {want_total.item()!r}), ctl {tr.ctl.tolist()} (alone {want_ctl.tolist()})")
        assert nb == want_nb and torch.equal(tr.ctl, want_ctl)
        assert torch.equal(total, want_total), (l, total.item(), want_total.item())
        for i, (a, b) in enumerate(zip(tr.params, want_params)):
            assert torch.equal(a.detach(), b), (l, "parameter", i, (a.detach() - b).abs().max().item())
        for i, (a, b) in enumerate(zip(tr.square_avg, want_avg)):
            assert torch.equal(a, b), (l, "running average", i, (a - b).abs().max().item())
        assert nets_b[l].layers[0].weight.data_ptr() == bt.W1s[l].data_ptr()          # the network's parameter IS the stacked slice
    assert not torch.equal(bt.trainers[0].params[2], bt.trainers[1].params[2])       # voters are different runs
    if graph:       # a second epoch replays the same graph
        g_before = next(iter(bt._graphs.values()))
        bt.run_epoch(store, B, gens)
        torch.cuda.synchronize()
        assert len(bt._graphs) == 1 and next(iter(bt._graphs.values())) is g_before
        assert all(torch.isfinite(p_).all() for t in bt.trainers for p_ in t.params)
    return bt, store


@pytest.mark.parametrize("n,graph,lanes", [(1500, False, 3), (4200, True, 2), (4200, True, 3), (4200, True, 5), (4200, False, 8)])
def test_lockstep_voters_at_200_units_are_the_lone_voters(dev, monkeypatch, n, graph, lanes):
    """2, 3, 5, 8 voters of NetLinear(4096, 200) in lockstep, the eight launches of the step recorded and run once for all of them: an epoch (8 or
    24 full batches of 512 + a partial one, dropout on), launch by launch or as a captured graph, leaves the lone voters' bits in every parameter,
    every RMSprop running average, the loss sum and the counters."""
    _lockstep_is_lone(dev, monkeypatch, n, graph, lanes)


@pytest.mark.parametrize("n,graph,lanes,C", [(1500, False, 3, 20), (4200, True, 2, 20)])
def test_lockstep_voters_at_20_units_are_the_lone_voters(dev, monkeypatch, n, graph, lanes, C):
    """The same at n_clusters <= 48: the six launches of _step_planes recorded and run once for all voters leave the lone voters' bits (the lone
    step and the recorded one are one body, so what tests/test_gpu_encoder.py holds within a tolerance for both lockstep forms is held exactly here)."""
    _lockstep_is_lone(dev, monkeypatch, n, graph, lanes, C=C)


def test_cold_caches_leave_lockstep_voters_at_200_units_the_lone_voters(dev, monkeypatch):
    """The same with a 512 MB fill in front of each of the eight batched launches (test_cold=1): three voters are the lone voters (whose hand-scheduled
    launches are evicted in front of, too).  Once, not in a loop."""
    monkeypatch.setitem(_variants(), "test_cold", "1")
    bt, _ = _lockstep_is_lone(dev, monkeypatch, 4200, False, 3)
    assert bt._planes_step and bt.trainers[0]._cold


# ------------------------------------------------------------------------------------------------ each new record alone
def _record(fn, *args):
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    blob = torch.zeros(int(L.idl_plan_bytes()), dtype=torch.uint8)
    _lib.check(L.idl_plan_begin(ctypes.c_void_p(blob.data_ptr())))
    rc = fn(*args)
    end = L.idl_plan_end()
    _lib.check(rc)
    _lib.check(end)
    return blob


def _recorded_equals_launched(dev, fn, make, args_of, outputs, voters=3):
    """make(v) -> {name: tensor} of voter v; args_of(bufs) -> the launcher's arguments.  The voters' launches recorded and run by ONE idl_plan_launch
    write into every tensor named in `outputs` what `voters` ordinary launches write into copies."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    rec = [make(v) for v in range(voters)]
    ref = [{k: (t.clone() if t is not None else None) for k, t in b.items()} for b in rec]
    for b in ref:
        _lib.check(fn(*args_of(b)))
    blobs = [_record(fn, *args_of(b)) for b in rec]
    torch.cuda.synchronize()
    for b, r in zip(rec, ref):              # recording launched nothing
        assert not torch.equal(b[outputs[0]], r[outputs[0]]), outputs[0]
    host = torch.stack(blobs).contiguous()
    devp = host.to(dev)
    _lib.check(L.idl_plan_launch(ctypes.c_void_p(host.data_ptr()), _p(devp), voters, _stream()))
    torch.cuda.synchronize()
    for v, (b, r) in enumerate(zip(rec, ref)):
        for k in outputs:
            # (bit patterns: a buffer may hold NaN fill where the kernel writes nothing)
            assert torch.equal(b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k],
                               r[k].view(torch.int32) if r[k].dtype == torch.float32 else r[k]), (v, k)
    assert not torch.equal(rec[0][outputs[0]], rec[1][outputs[0]])        # the voters are different problems


def _gen(seed):
    import torch
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    return g


@pytest.mark.parametrize("C", [49, 130, 200])
def test_recorded_infonce_with_the_joint_equals_three_launches(dev, C):
    """idl_nce_fused_joint recorded (the joint's 16 x 16 tiles ride in pass 1 as spare workgroups; C = 130: ragged tile edges)."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    m = 1024

    def make(v):
        g = _gen(1000 * C + v)
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        return dict(f=torch.nn.functional.normalize(torch.randn(m, 64, generator=g), dim=1).to(dev),
                    z=torch.softmax(torch.randn(m, C, generator=g) * 2.0, 1).to(dev),
                    lse=nan(m), rows=nan(m), G=nan(int(L.idl_nce_fused_parts()), m, 64), ws=nan(int(L.idl_nce_fused_workspace(m)) // 4), P0=nan(C, C))

    args_of = lambda b: (_p(b["f"]), m, 0.85, _p(b["lse"]), _p(b["rows"]), _p(b["G"]), _p(b["ws"]), _p(b["z"]), _p(b["P0"]), C, _stream())
    _recorded_equals_launched(dev, L.idl_nce_fused_joint, make, args_of, ["P0", "lse", "rows", "G", "ws"])


@pytest.mark.parametrize("C", [49, 200])
def test_recorded_iic_core_dz_equals_three_launches(dev, C):
    """idl_iic_core_dz recorded: one record, two launches (the rows launch with the joint in dynamic LDS -- 160.8 KB at C = 200 --, then the z dP0 tiles)."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    m = 1024

    def make(v):
        g = _gen(77 * C + v)
        z = torch.softmax(torch.randn(m, C, generator=g) * 2.0, 1).to(dev)
        return dict(z=z, P0=(z[:m // 2].t() @ z[m // 2:]).contiguous(), scratch=torch.zeros(C * C + 2 * C, device=dev),
                    out=torch.zeros(4, device=dev), dzs=torch.full((m, C), float("nan"), device=dev))

    args_of = lambda b: (_p(b["P0"]), C, 2.8, 2.2e-16, 0.25, _p(b["scratch"]), _p(b["out"]), _p(b["z"]), m, _p(b["dzs"]), _stream())
    _recorded_equals_launched(dev, L.idl_iic_core_dz, make, args_of, ["dzs", "scratch", "out"])


@pytest.mark.parametrize("C", [49, 200])
def test_recorded_mid_bwd_beyond_48_classes_equals_three_launches(dev, C):
    """idl_mid_bwd_gather recorded at C > 48 (the BIG body: W3 in dynamic LDS, dr1 as planes, z dP0 given), its spare workgroups assembling the
    second half of the next batch as planes: mid_bwd_big_batched_kernel against mid_bwd_kernel<true, true>.  Another form beyond 48 classes is refused."""
    import torch
    import test_gpu_encoder as E
    from idelucs_amd import _lib
    L = _lib.lib
    m, H1, H2, F = 1024, 512, 64, 4096
    store, _ = E._cfg2_store_and_net(dev, 600, seed=9, C=C)
    parts, cp = int(L.idl_nce_fused_parts()), int(L.idl_col_sum_parts())

    def make(v):
        g = _gen(31 * C + v)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)
        i16 = lambda *s: torch.zeros(s, dtype=torch.int16, device=dev)
        f = torch.nn.functional.normalize(r(m, H2), dim=1)
        scale = torch.zeros(int(L.idl_dr1_scale_words()), dtype=torch.int32, device=dev)
        scale[1] = int(L.idl_planes_exponent(2))
        return dict(z=torch.softmax(r(m, C) * 2.0, 1), r2=torch.relu(r(m, H2)), f=f, inv=torch.rand(m, generator=g).to(dev) + 0.5, G=r(parts, m, H2) * 0.1,
                    P0=r(C, C) * 1e-3, W3=r(C, H2) * 0.1, W2=r(H2, H1) * 0.05, act1=torch.relu(r(m, H1)), dzs=r(m, C) * 1e-3,
                    dlogits=torch.zeros(m, C, device=dev), dlat=torch.zeros(m, H2, device=dev), gb1=torch.zeros(cp, H1, device=dev),
                    gb2=torch.zeros(cp, H2, device=dev), gb3=torch.zeros(cp, C, device=dev), dh=i16(m, H1), dl=i16(m, H1), scale=scale,
                    flag=torch.zeros(1, dtype=torch.int32, device=dev), yh=i16(m, F), yl=i16(m, F),
                    perm=torch.randperm(store.n_pairs, generator=g).to(dev), base=torch.zeros(1, dtype=torch.int64, device=dev))

    def args_of(b, dr1_planes=True):
        nxt = _lib.idl_next_batch_t(feats=_p(store.feats), n=store.n, f=store.f, view_stride=store.n * store.f, pair_idx=_p(b["perm"]), base=_p(b["base"]),
                                    base_add=m // 2, n_pairs=store.n_pairs, batch=m // 2, mean=_p(store.mean), scale=_p(store.scale),
                                    inv_scale=_p(store.inv_scale), y_hi=_p(b["yh"]), y_lo=_p(b["yl"]), overflow_flag=_p(b["flag"]), part=4, part_end=8, parts=8)
        dr1 = (None, _p(b["dh"]), _p(b["dl"]), _p(b["scale"])) if dr1_planes else (_p(b["act1"].new_empty(m, H1)), None, None, None)
        return (_p(b["z"]), _p(b["r2"]), _p(b["f"]), _p(b["inv"]), _p(b["G"]), parts, _p(b["P0"]), _p(b["W3"]), _p(b["W2"]), _p(b["act1"]), m, C, 1,
                0.75 / (m * 0.85), _p(b["dlogits"]), _p(b["dlat"]), dr1[0], _p(b["gb1"]), _p(b["gb2"]), _p(b["gb3"]), None, 0,
                *dr1[1:], _p(b["flag"]), _p(b["dzs"]), nxt, _stream())

    _recorded_equals_launched(dev, L.idl_mid_bwd_gather, make, args_of, ["dlogits", "dlat", "dh", "dl", "scale", "gb1", "gb2", "gb3", "yh", "yl", "flag"])
    blob = torch.zeros(int(L.idl_plan_bytes()), dtype=torch.uint8)          # dr1 in fp32 beyond 48 classes: not a recordable form
    _lib.check(L.idl_plan_begin(ctypes.c_void_p(blob.data_ptr())))
    rc = L.idl_mid_bwd_gather(*args_of(make(0), dr1_planes=False))
    L.idl_plan_end()
    assert rc != 0 and "beyond 48 classes" in _lib.last_error()


@pytest.mark.parametrize("C", [49, 130, 200])
def test_recorded_at_b_equals_three_launches(dev, C):
    """idl_at_b recorded (dW3 = dlogits^T r2): a 2-D tile grid per voter, the voter in blockIdx.z."""
    import torch
    from idelucs_amd import _lib
    L = _lib.lib
    K, N = 1024, 64

    def make(v):
        g = _gen(5 * C + v)
        return dict(A=torch.randn(K, C, generator=g).to(dev), B=torch.randn(K, N, generator=g).to(dev), out=torch.full((C, N), float("nan"), device=dev))

    args_of = lambda b: (_p(b["A"]), C, _p(b["B"]), N, K, C, N, _p(b["out"]), N, _stream())
    _recorded_equals_launched(dev, L.idl_at_b, make, args_of, ["out"])


# ------------------------------------------------------------------------------------------------ launch budget
def test_a_lockstep_step_of_four_voters_is_ten_launches(dev, monkeypatch):
    """torch.profiler over four lockstep steps of 4 voters at C = 200: 10 kernel launches a step (the lone voters' would be 40), every one a batched
    kernel of this package, none a library GEMM (Cijk_*), none an unbatched one."""
    import torch
    import test_gpu_encoder as E
    from torch.profiler import profile, ProfilerActivity
    from idelucs_amd.fused import BatchedLinearTrainer, _planes_of
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    monkeypatch.setitem(_variants(), "lockstep_planes", "1")
    store, net0 = E._cfg2_store_and_net(dev, 1100, seed=8, C=200)           # 6 full batches + a partial one
    B, lanes = 512, 4
    bt = BatchedLinearTrainer([copy.deepcopy(net0) for _ in range(lanes)], lr=1e-3, weight=0.25, lamb=2.8, seed=3)
    gens = []
    for l, tr in enumerate(bt.trainers):
        tr.begin_voter(l)
        gens.append(torch.Generator(device=dev).manual_seed(1 + l))
    bt.run_epoch(store, B, gens, use_graph=False)                           # warm-up: allocations, the recorded program
    torch.cuda.synchronize()
    assert bt._planes_step
    m = 2 * B
    for tr in bt.trainers:                                                  # run_epoch's prologue
        tr.ctl[1:2].zero_()
        bf = tr.buffers(m)
        tr._gather(store, bf)
        tr._w1_planes_fresh = False
        tr._prepare_planes(bf, _planes_of(bf, tr.F), 0)
    prog, st = bt._program(store, m), bt.stack(m)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(4):
            bt._step(prog, st, i % 2)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not names:
        pytest.skip("the profiler reported no device kernels on this box")
    print(sorted(set(names)))
    assert len(names) == 4 * 10, (len(names), sorted(set(names)))
    assert not any("Cijk" in n for n in names)
    batched = ["l1_planes_batched_kernel", "reduce_batched_kernel", "mid_fwd_batched_kernel", "nce_pass1_batched_kernel", "nce_pass2_batched_kernel",
               "iic_core_rows_batched_kernel", "iic_dz_batched_kernel", "mid_bwd_big_batched_kernel", "at_b_batched_kernel", "wgrad_xplanes_rms_batched_kernel"]
    for k in batched:
        assert sum(k in n for n in names) == 4, (k, sorted(set(names)))
    for k in ("l1_planes_kernel", "reduce_rms_kernel", "mid_fwd_kernel", "nce_pass1_kernel", "nce_pass2_kernel", "iic_core_rows_kernel", "iic_dz_kernel",
              "mid_bwd_kernel", "mid_bwd_batched_kernel", "at_b_kernel", "wgrad_dplanes_rms_kernel"):
        assert not any(k in n for n in names), (k, sorted(set(names)))


# ------------------------------------------------------------------------------------------------ through training.train_voters
def _influenza(monkeypatch, planes="1", **kw):
    import test_gpu_encoder as E
    from idelucs_amd import training
    monkeypatch.setenv("IDELUCS_PLANES", planes)
    args = E._args(**{**dict(k=6, n_clusters=200, batch_sz=512, n_epochs=3, n_voters=3, seed=3), **kw})
    return training.prepare_model(args), args


def test_train_voters_in_lockstep_at_200_units_equals_one_after_the_other(dev, monkeypatch):
    """training.train_voters on Influenza-A (k = 6, n_clusters = 200, batch 512, 3 voters, 3 epochs) with lanes = 3 and with lanes = 1: the same loss
    curves, y_pred and latent per voter; the batched trainer is built in the first run only.  IDELUCS_PLANES=0 and n_clusters = 201: can_batch is
    false up front and the run completes one voter after the other."""
    import torch
    from idelucs_amd import fused, training
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
    built = []
    real = fused.BatchedLinearTrainer

    class Spy(real):
        def __init__(self, *a, **k):
            built.append(len(a[0]))
            super().__init__(*a, **k)

    monkeypatch.setattr(fused, "BatchedLinearTrainer", Spy)
    model, args = _influenza(monkeypatch)
    assert training.can_batch(model) and training.lockstep_rows_applies(model)
    lock = training.train_voters(model, [0, 1, 2], 3, 3, lanes=3, progress=False)
    assert built == [3]
    y_last = model.predict()[0]
    assert np.array_equal(y_last, lock[2][1])                     # the caller's model holds the last voter's weights
    model1, _ = _influenza(monkeypatch)
    seq = training.train_voters(model1, [0, 1, 2], 3, 3, lanes=1, progress=False)
    assert built == [3] and not fused._PLANES_DISABLED
    assert training.can_batch(model)
    for v in (0, 1, 2):
        print(f"voter {v}: curve {lock[v][0]} (one after the other {seq[v][0]})")
        assert lock[v][0] == seq[v][0] and all(np.isfinite(lock[v][0]))
        assert np.array_equal(lock[v][1], seq[v][1]) and np.array_equal(lock[v][2], seq[v][2]) and np.array_equal(lock[v][3], seq[v][3])
    assert not np.array_equal(lock[0][3], lock[1][3])
    for planes, kw in (("0", {}), ("1", dict(n_clusters=201))):
        other, _ = _influenza(monkeypatch, planes, **kw)
        assert not training.can_batch(other)
        out = training.train_voters(other, [0, 1], 1, 2, lanes=2, progress=False)
        assert built == [3] and sorted(out) == [0, 1] and all(np.isfinite(out[v][0]).all() for v in out)
    # ... and the other settings that keep voters one after the other, decided before any trainer exists
    monkeypatch.setenv("IDELUCS_PLANES", "1")
    monkeypatch.setitem(_variants(), "lockstep_planes", "0")
    assert not training.can_batch(model)
    monkeypatch.setitem(_variants(), "lockstep_planes", "1")
    model.schedule = "Plateau"
    assert not training.can_batch(model)


# ------------------------------------------------------------------------------------------------ overflow fall-back in lockstep
@pytest.mark.parametrize("C", [5, 200])
def test_data_beyond_the_planes_range_falls_back_in_lockstep(dev, monkeypatch, capsys, C):
    """ADVICE (low, training.py): a lockstep batch whose data leaves the planes' range (the scaled column of
    test_gpu_planes.test_data_beyond_the_planes_range_falls_back_to_the_fp32_tiles) is noticed after its FIRST epoch -- one read of the lanes' flags --
    and trained again: at n_clusters = 5 in lockstep on the fp32 form, at 200 (no recordable fp32 form) one voter after the other on the fp32 tiles.
    Either way the result is the IDELUCS_PLANES=0 run bit for bit, and stderr names the fall-back."""
    import torch
    import test_gpu_encoder as E
    from idelucs_amd import fused, models, training
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
    epochs = []
    real_epoch = fused.BatchedLinearTrainer.run_epoch

    def counting(self, *a, **k):
        epochs.append(self._planes_step or None)
        return real_epoch(self, *a, **k)

    monkeypatch.setattr(fused.BatchedLinearTrainer, "run_epoch", counting)

    def model(planes):
        monkeypatch.setenv("IDELUCS_PLANES", planes)
        m = models.IID_model({'sequence_file': os.path.join(E.DATA, "Influenza-A.fas"), 'GT_file': None, 'n_clusters': C, 'k': 6,
                              'model_size': 'linear', 'n_mimics': 3, 'batch_sz': 512, 'optimizer': 'RMSprop', 'lambda': 2.8,
                              'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 3, 'n_voters': 2, 'seed': 3})
        m.build_dataloader()
        col = 77
        m.store.scale[col] = m.store.scale[col] * 1e-7                           # the column's standardised entries: ~1e7 standard deviations
        m.store.inv_scale[col] = 1.0 / m.store.scale[col]
        return m

    m1 = model("1")
    assert training.can_batch(m1)
    got = training.train_voters(m1, [0, 1], 3, 2, lanes=2, progress=False)
    err = capsys.readouterr().err
    assert "fp32 tiles" in err and "again from the start" in err
    assert fused._PLANES_DISABLED
    # one epoch in lockstep on the planes before the flag was read; then the retrain: three lockstep epochs on the fp32 form (n_clusters = 5), or none
    print("lockstep epochs:", len(epochs))
    assert len(epochs) == (1 + 3 if C <= 48 else 1), epochs
    n_first = len(epochs)
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
    m0 = model("0")
    assert training.can_batch(m0) == (C <= 48)
    want = training.train_voters(m0, [0, 1], 3, 2, lanes=2, progress=False)
    assert len(epochs) - n_first == (3 if C <= 48 else 0)
    for v in (0, 1):
        assert got[v][0] == want[v][0] and np.array_equal(got[v][1], want[v][1]) and np.array_equal(got[v][2], want[v][2]) and np.array_equal(got[v][3], want[v][3])
    for a, b in zip(m1.net.parameters(), m0.net.parameters()):
        assert torch.equal(a, b)
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
