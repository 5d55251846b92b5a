"""The loss kernels on saturated, degenerate inputs: the regimes in which training ends (dead output units, classes that never co-occur, a
one-hot head, a collapsed encoder), where cells and marginals of the IIC joint fall below EPS and the reference REPLACES them by the constant EPS
(reference LossFunctions.py:32-38: no gradient through a replaced cell or a replaced marginal).  Every other tensor that reaches a loss kernel in
this suite is random: each cell of its joint is ~1/C^2, eleven orders of magnitude above EPS, and not one of the kernels' `if (!(x < eps))` gates is taken.

1. regime_logits: the four input regimes, seeded, built on the host (tests/golden/make_golden_degenerate.py writes the same logits into the fixture that
   pins idelucs_amd.LossFunctions.IID_loss -- the float64 reference of sections 2 and 4 -- to the reference where cells are replaced).
2. the IIC stage through every dispatch of fused.launch_losses against float64 autograd of the reference formula on the joint.
3. InfoNCE on degenerate latents (a collapsed encoder, exact duplicates, two antipodal clusters) through the same dispatches.
4. one whole step per step form with a saturated head against float64 autograd.

Replaced-cell and replaced-marginal branches reached, per kernel body (every regime at every shape listed):
    iic_core_small (in InfoNCE pass 1: idl_nce_fused_iic_z)   (m, C) = (32, 5), (128, 20), (96, 48)
    iic_core_small (idl_iic_core, C <= 48)                    (14, 5), (72, 48)
    iic_core_rows_multi + iic_core_shift (idl_iic_core)       (112, 49), (72, 200)
    iic_core_rows (idl_iic_core, C > 200)                     (80, 256)
    iic_core_rows_multi + iic_dz_body (idl_iic_core_dz)       (96, 49), (256, 130), (256, 200), (112, 130); recorded, two voters in one launch: (256, 200)
"dead", "onehot" and "collapsed" replace cells and marginals; "disjoint" replaces cells whose two marginals are not replaced (and marginals, of its dead columns)."""
import copy
import ctypes
import functools
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = sys.float_info.epsilon
LAMB, W_IIC, T = 2.8, 0.25, 0.85
REGIMES = ("dead", "disjoint", "onehot", "collapsed")


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ 1. the input regimes
def regime_logits(name, B, C, seed=0):
    """fp32 logits a[2B, C] (numpy; rows b and b + B are a pair) of one regime; z = softmax(a) in fp32.  live = max(3, C // 4) classes stay in use.
      dead       randn * 2; columns live: pushed down by 60 (z ~ e^-60: a normal fp32 number far below EPS), the last max(1, C // 8) by a further 140
                 (an exact 0 in fp32): replaced cells AND replaced marginals
      disjoint   as dead without the 140; the first half of the pairs pushed down by 50 on the live columns live//2:live, the other half on :live//2:
                 live classes that never co-occur -- replaced cells whose two marginals are NOT replaced
      onehot     every pair one-hot (+200 / -200) on the same random class out of 0..C-2: exact 0 and 1, one class never used
      collapsed  every row one-hot on class C // 2: the joint is a single 1"""
    rng = np.random.default_rng([seed, B, C, REGIMES.index(name)])
    live = max(3, C // 4)
    if name in ("dead", "disjoint"):
        a = (rng.standard_normal((2 * B, C)) * 2.0).astype(np.float32)
        a[:, live:] -= 60.0
        if name == "dead":
            a[:, C - max(1, C // 8):] -= 140.0
        else:
            h = B // 2
            first, second = np.r_[0:h, B:B + h], np.r_[h:B, B + h:2 * B]
            a[np.ix_(first, np.arange(live // 2, live))] -= 50.0
            a[np.ix_(second, np.arange(0, live // 2))] -= 50.0
        return a
    a = np.full((2 * B, C), -200.0, np.float32)
    cls = rng.integers(0, C - 1, size=B) if name == "onehot" else np.full(B, C // 2)
    a[np.arange(B), cls] = 200.0
    a[np.arange(B) + B, cls] = 200.0
    return a


def regime_z(name, B, C):
    import torch
    return torch.softmax(torch.from_numpy(regime_logits(name, B, C)), dim=1)


@functools.lru_cache(maxsize=None)
def iic_reference(name, m, C):
    """float64, on the host, once per (regime, shape): the reference formula on P0 = z1^T z2 (z: the fp32 softmax cast to double) with torch.where, as
    test_gpu_encoder.py::test_iic_core_large_joint_vs_torch writes it -> (z fp32, loss, w_iic dIIC/dP0, w_iic dIIC/dz = cat(z2 dP0^T, z1 dP0)), all on the host.
    Asserts that no cell and no marginal of the float64 joint lies within a factor 1000 of EPS (there fp32 and float64 could take different branches)
    and that the regime reaches the branches it is there for."""
    import torch
    B = m // 2
    z = regime_z(name, B, C)
    z1, z2 = z[:B].double(), z[B:].double()
    P0 = (z1.t() @ z2).requires_grad_(True)
    P = (P0 + P0.t()) / 2.0
    P = P / P.sum()
    pi = P.sum(1, keepdim=True).expand(C, C); pj = P.sum(0, keepdim=True).expand(C, C)
    v = torch.cat([P.detach().flatten(), pi[:, 0].detach(), pj[0].detach()])
    assert not bool(((v > EPS / 1e3) & (v < EPS * 1e3)).any()), (name, m, C, "a cell or marginal within 1000 x of EPS")
    cell, marg = (P < EPS).detach(), (pi[:, 0] < EPS).detach()
    assert bool(cell.any()), (name, m, C, "no replaced cell")
    if name == "disjoint":
        assert bool((cell & ~marg[:, None] & ~marg[None, :]).any()), (name, m, C, "no replaced cell between two live marginals")
    else:
        assert bool(marg.any()), (name, m, C, "no replaced marginal")
    e = torch.full_like(P, EPS)
    Pc = torch.where(P < EPS, e, P); pic = torch.where(pi < EPS, e, pi); pjc = torch.where(pj < EPS, e, pj)
    loss = -(Pc * (torch.log(Pc) - LAMB * torch.log(pjc) - LAMB * torch.log(pic))).sum()
    loss.backward()
    dP0 = W_IIC * P0.grad
    dzs = torch.cat([z2 @ dP0.t(), z1 @ dP0])
    return z, float(loss.item()), dP0, dzs


def _unit_rows(m, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(m, 64, generator=g), dim=1)


def _nan(*shape, dev):
    import torch
    return torch.full(shape, float("nan"), device=dev)


DISPATCH = {  # (fused InfoNCE, C <= 48, dz) -> the launches of fused.launch_losses
    (True, True): ["idl_nce_fused_iic_z"],
    (True, False, True): ["idl_nce_fused_joint", "idl_iic_core_dz"],
    (True, False, False): ["idl_iic_joint", "idl_iic_core", "idl_nce_fused"],
    (False, False, True): ["idl_iic_joint", "idl_iic_core_dz", "idl_nce_rows"],
    (False, False, False): ["idl_iic_joint", "idl_iic_core", "idl_nce_rows"],
    (False, True): ["idl_iic_joint", "idl_iic_core", "idl_nce_rows"],
}


def _launch_losses(dev, z, f, dz, fused_nce):
    """fused.launch_losses (the dispatch the trainers use) on z and f in a fresh fused._Buffers whose every output and scratch buffer is NaN, twice:
    the launches are the expected ones, the second call leaves the first call's bits.  -> (buffers, out)."""
    import torch
    from idelucs_amd import fused
    m, C = z.shape
    bf = fused._Buffers(m, 4, 4, 64, C, dev)
    assert bf.nce_fused == fused_nce, (m, bf.nce_fused)
    for name in ("P0", "dzs", "lse", "loss_rows", "G", "S", "iic_scratch", "nce_ws"):
        if getattr(bf, name) is not None:
            getattr(bf, name).fill_(float("nan"))
    bf.z.copy_(z); bf.f.copy_(f)
    names = []

    def k(fn, *args):
        names.append(fn.__name__)
        fused._launch(fn, *args)

    first = None
    for _ in range(2):
        out = _nan(4, dev=dev)
        del names[:]
        fused.launch_losses(k, bf, LAMB, W_IIC, out, dz=dz)
        torch.cuda.synchronize()
        key = (fused_nce, True) if C <= 48 else (fused_nce, False, dz)
        assert names == DISPATCH[key], names
        got = [t.clone() for t in (out[3:], bf.dzs if (dz and C > 48) else bf.P0, bf.lse, bf.loss_rows, bf.G)]
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert torch.equal(_bits(a), _bits(b)), "a second call on the same scratch gave other bits"
    return bf, out


# ------------------------------------------------------------------------------------------------ 2. the IIC stage, every dispatch
def _dz_of(dzs):
    """w_iic dIIC/dz as the middle backward reads it from idl_iic_core_dz's output: the kernel writes z dP0 for every row, and row r of the batch takes its
    PARTNER's row of that product (dIIC/dz1 = z2 dP0^T, dIIC/dz2 = z1 dP0; csrc/train_step.hip, head_bwd_kernel / mid_bwd: `dzs[prow * C + c]`)."""
    return dzs.roll(dzs.shape[0] // 2, 0)


def _check_iic(name, out, got, loss, want):
    """The bars of test_iic_core_large_joint_vs_torch: loss 1e-4 relative (collapsed, whose loss is ~ -1e-9: 1e-6 absolute -- 1e-4 of a loss of
    log C size, rounded down); gradient rtol 2e-3, atol 2e-4 max|want|; everything finite.  (fp32 arithmetic alone needs 3.6e-7 max|want|; a gate
    taken the wrong way costs more than 3 max|want|.)"""
    import torch
    iic = out[3].item()
    wmax = want.abs().max().item()
    err = (got.double().cpu() - want).abs().max().item()
    print(f"{name}: IIC {iic!r} (float64 {loss!r}), max gradient error {err / wmax:.2e} of max|want| = {wmax:.3e}")
    assert np.isfinite(iic) and bool(torch.isfinite(got).all())
    assert abs(iic - loss) <= (1e-6 if name == "collapsed" else 1e-4 * abs(loss)), (iic, loss)
    assert wmax > 0
    assert torch.allclose(got.double().cpu(), want, rtol=2e-3, atol=2e-4 * wmax), (err, wmax)


IIC_CASES = [  # m, C, dz, fused InfoNCE
    (32, 5, False, True), (128, 20, False, True), (96, 48, False, True),            # idl_nce_fused_iic_z: the core rides in InfoNCE pass 1
    (96, 49, True, True), (256, 130, True, True), (256, 200, True, True),           # idl_nce_fused_joint + idl_iic_core_dz
    (112, 49, False, False), (72, 200, False, False), (80, 256, False, False),      # idl_iic_joint + idl_iic_core (C > 200: rows in registers)
    (14, 5, False, False), (72, 48, False, False),                                  # idl_iic_joint + idl_iic_core, C <= 48
    (112, 130, True, False),                                                        # idl_iic_joint + idl_iic_core_dz
]


@pytest.mark.parametrize("name", REGIMES)
@pytest.mark.parametrize("m,C,dz,fused_nce", IIC_CASES)
def test_iic_stage_on_degenerate_joints_vs_float64(dev, m, C, dz, fused_nce, name):
    """C = 48 / 49: the LDS / rows split; 130: ragged 16-wide tiles; 200: the 160 KB dynamic-LDS joint; 256: the register-rows limit; m % 32 != 0:
    the fused InfoNCE kernels are off and the joint is idl_iic_joint's."""
    z, loss, dP0, dzs = iic_reference(name, m, C)
    bf, out = _launch_losses(dev, z.to(dev), _unit_rows(m, m + C).to(dev), dz, fused_nce)
    _check_iic(name, out, _dz_of(bf.dzs) if dz else bf.P0, loss, dzs if dz else dP0)


def test_recorded_iic_core_dz_on_degenerate_joints(dev):
    """Two voters, "dead" and "onehot", at C = 200 (m = 256): idl_iic_core_dz recorded per voter and run by ONE idl_plan_launch (voter in blockIdx.y)
    leaves the bits of the two lone launches, which are the float64 reference's values."""
    import torch
    from idelucs_amd import _lib
    import test_gpu_lockstep_rows as LR
    L = _lib.lib
    m, C = 256, 200
    refs = [iic_reference(name, m, C) for name in ("dead", "onehot")]

    def make(v):
        z = refs[v][0].to(dev)
        P0 = _nan(C, C, dev=dev)
        _lib.check(L.idl_iic_joint(_p(z), m, C, _p(P0), _stream()))
        return dict(z=z, P0=P0, scratch=_nan(C * C + 2 * C, dev=dev), out=_nan(4, dev=dev), dzs=_nan(m, C, dev=dev))

    args_of = lambda b: (_p(b["P0"]), C, LAMB, EPS, W_IIC, _p(b["scratch"]), _p(b["out"]), _p(b["z"]), m, _p(b["dzs"]), _stream())
    lone, rec = [make(v) for v in range(2)], [make(v) for v in range(2)]
    for b in lone:
        _lib.check(L.idl_iic_core_dz(*args_of(b)))
    blobs = [LR._record(L.idl_iic_core_dz, *args_of(b)) for b in rec]
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b["dzs"]).all()) for b in rec)             # recording launched nothing
    host = torch.stack(blobs).contiguous()
    devp = host.to(dev)
    _lib.check(L.idl_plan_launch(ctypes.c_void_p(host.data_ptr()), _p(devp), 2, _stream()))
    torch.cuda.synchronize()
    for v, name in enumerate(("dead", "onehot")):
        assert torch.equal(_bits(rec[v]["dzs"]), _bits(lone[v]["dzs"])) and torch.equal(_bits(rec[v]["out"][3:]), _bits(lone[v]["out"][3:])), name
        _check_iic(name, rec[v]["out"], _dz_of(rec[v]["dzs"]), refs[v][1], refs[v][3])
    assert not torch.equal(rec[0]["dzs"], rec[1]["dzs"])


# ------------------------------------------------------------------------------------------------ 3. InfoNCE on degenerate latents
LATENTS = ("collapsed", "duplicates", "antipodal")
DUPLICATE_ROWS_EQUAL = {32: True, 72: True, 512: False}      # m -> loss_rows[b] == loss_rows[b + B] bit for bit on "duplicates" (measured: see the test)


@functools.lru_cache(maxsize=None)
def nce_reference(name, m):
    """Unit rows f[m, 64] (fp32, host) and the float64 reference as test_gpu_encoder.py::test_fused_infonce_kernels_vs_torch writes it
    -> (f, lse, loss rows, (E + E^T) f).
      collapsed   one direction + 1e-3 randn, renormalised (a collapsed encoder: every similarity ~ 1)
      duplicates  f[b + B] = f[b] exactly, and eight rows (1..4 and their partners) are exact copies of row 0
      antipodal   two clusters +-u (a pair on the same side), noise 1e-2"""
    import torch
    B = m // 2
    g = torch.Generator().manual_seed(1000 * LATENTS.index(name) + m)
    u = torch.nn.functional.normalize(torch.randn(1, 64, generator=g), dim=1)
    if name == "collapsed":
        h = u + 1e-3 * torch.randn(m, 64, generator=g)
    elif name == "duplicates":
        h = torch.randn(B, 64, generator=g)
        h[1:5] = h[0]
        h = torch.cat([h, h])
    else:
        sign = (torch.randint(0, 2, (B, 1), generator=g) * 2 - 1).float()
        h = torch.cat([sign, sign]) * u + 1e-2 * torch.randn(m, 64, generator=g)
    f = torch.nn.functional.normalize(h, dim=1).contiguous()
    if name == "duplicates":
        assert torch.equal(f[:B], f[B:]) and all(torch.equal(f[i], f[0]) for i in (1, 2, 3, 4, B + 1, B + 4))
    fd = f.double()
    S = (fd @ fd.t()) / T
    eye = torch.eye(m, dtype=torch.bool)
    lse = torch.logsumexp(S.masked_fill(eye, float("-inf")), dim=1)
    r = torch.arange(m)
    rows = lse - S[r, (r + B) % m]
    E = torch.exp(S - lse[:, None]).masked_fill(eye, 0.0)
    return f, lse, rows, (E + E.t()) @ fd


@pytest.mark.parametrize("name", LATENTS)
@pytest.mark.parametrize("m,C,dz", [(32, 5, False), (32, 49, True), (32, 49, False), (512, 5, False), (512, 49, True), (512, 49, False), (72, 5, False)])
def test_infonce_on_degenerate_latents_vs_float64(dev, m, C, dz, name):
    """The three fused forms (pass 1 carrying the IIC core, carrying the joint's tiles, alone) at m = 32 and 512 and idl_nce_rows at m = 72, with the
    bars of test_fused_infonce_kernels_vs_torch on lse, the loss rows and (E + E^T) f; everything finite.
    duplicates: rows b and b + B see the same similarities, but their sums skip the diagonal at different places.  Measured on the kernels of the
    commit before this module: loss_rows[b] == loss_rows[b + B] bit for bit at m = 32 (all three fused forms) and at m = 72 (idl_nce_rows), and NOT at
    m = 512 (the fused kernels split a row's columns over several workgroups there and add the parts up in another order for the two rows: they differ
    in the last bits, both within 1.4e-6 of float64).  Asserted where it held (DUPLICATE_ROWS_EQUAL), printed everywhere."""
    import torch
    f, lse, rows, G = nce_reference(name, m)
    z = torch.softmax(torch.randn(m, C, generator=torch.Generator().manual_seed(m + C)) * 2, dim=1)
    bf, _ = _launch_losses(dev, z.to(dev), f.to(dev), dz, m % 32 == 0)
    got_G = bf.G.sum(0)
    for t in (bf.lse, bf.loss_rows, got_G):
        assert bool(torch.isfinite(t).all())
    print(f"{name} m={m}: max errors lse {(bf.lse.cpu() - lse).abs().max().item():.2e}, rows {(bf.loss_rows.cpu() - rows).abs().max().item():.2e}, "
          f"G {(got_G.cpu() - G).abs().max().item():.2e}")
    np.testing.assert_allclose(bf.lse.cpu().numpy(), lse.float().numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(bf.loss_rows.cpu().numpy(), rows.float().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got_G.cpu().numpy(), G.float().numpy(), rtol=1e-4, atol=2e-6)
    if name == "duplicates":
        same = torch.equal(bf.loss_rows[:m // 2], bf.loss_rows[m // 2:])
        print(f"duplicates m={m} C={C} dz={dz}: loss_rows[b] == loss_rows[b + B] bit for bit: {same}")
        if DUPLICATE_ROWS_EQUAL[m]:
            assert same


# ------------------------------------------------------------------------------------------------ 4. whole steps with a saturated head
SHARP_K = 256      # see test_step_with_a_saturated_head_vs_float64


def _head(net):
    import torch.nn as nn
    return [mod for mod in net.classifier if isinstance(mod, nn.Linear)][0]


def saturate_head(net, head, k=SHARP_K):
    """dead: the bias of three quarters of the output units -60, of the last max(1, C // 8) of them -200; sharp: W3 and b3 times k."""
    import torch
    lin = _head(net)
    C = lin.out_features
    with torch.no_grad():
        if head == "dead":
            lin.bias[C - (3 * C) // 4:] = -60.0
            lin.bias[C - max(1, C // 8):] = -200.0
        else:
            lin.weight.mul_(k); lin.bias.mul_(k)


def autograd_step(net, x, dtype):
    """The reference step (models.py:117-133), dropout off, on a copy of net in `dtype`, through idelucs_amd.LossFunctions.IID_loss (pinned to the reference
    on replaced cells by tests/test_oracle_degenerate.py) and info_nce_loss written out without its cast to float32 -> (loss, {name: gradient})."""
    import torch
    from idelucs_amd.LossFunctions import IID_loss
    ref = copy.deepcopy(net).to(dtype).eval()
    z, h = ref(x.to(dtype))
    b = x.shape[0] // 2
    f = torch.nn.functional.normalize(h, dim=1)
    s = (f @ f.t()) / T
    r = torch.arange(2 * b, device=s.device)
    pos = s[r, (r + b) % (2 * b)]
    s = s.masked_fill(r.unsqueeze(0) == r.unsqueeze(1), float("-inf"))
    loss = (1.0 - W_IIC) * (torch.logsumexp(s, dim=1) - pos).mean() + W_IIC * IID_loss(z[:b], z[b:], lamb=LAMB)
    loss.backward()
    return float(loss.item()), {n: p.grad.detach().double() for n, p in ref.named_parameters()}


STEP_FORMS = [("linear", 20, "1"), ("linear", 200, "1"), ("linear", 20, "0"), ("linear", 200, "0"), ("small", 5, None), ("small", 200, None),
              ("SGD", 20, None), ("Adam", 20, None)]


def step_case(dev, monkeypatch, kind, C, planes, head, k=SHARP_K):
    """A trainer of one step form on a network whose head is saturated, and its batch -> (trainer, run, the network before the step, x)."""
    import torch
    if kind == "linear":          # FusedLinearTrainer's default dispatch at m = 256, F = 4096: planes / planes_rows (IDELUCS_PLANES=0: tiles / general)
        import test_gpu_encoder as E
        from idelucs_amd.fused import FusedLinearTrainer
        monkeypatch.setenv("IDELUCS_PLANES", planes)
        store, net = E._cfg2_store_and_net(dev, 300, seed=6, C=C)
        saturate_head(net, head, k)
        tr = FusedLinearTrainer(net, lr=1e-3, weight=W_IIC, lamb=LAMB, seed=5)
        tr._keep_w1_grad = True
        tr._perm = torch.randperm(store.n_pairs, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
        tr.ctl[1] = 0; tr.out[1] = 0.0
        bf = tr.buffers(256)
        want_form = {("1", 20): "planes", ("1", 200): "planes_rows", ("0", 20): "tiles", ("0", 200): "general"}[(planes, C)]
        assert bf.nce_fused and tr._form(bf, store) == want_form, "not the launch sequence this case is about"
        tr._gather(store, bf)
        x = bf.xs[0].clone()
        run = lambda: tr._full_step(store, bf, train=False, pipelined=True, xi=0)
    elif kind == "small":         # FusedSmallTrainer at F = 136, m = 64
        import test_gpu_small_step as SS
        net = SS._random_net(136, C, dev, seed=136 + C)
        saturate_head(net, head, k)
        tr = SS._trainer(net)
        x = torch.randn((64, 136), device=dev, generator=torch.Generator(device=dev).manual_seed(7 + C))
        bf = tr.buffers(64)
        bf.x.copy_(x)
        run = lambda: tr.step_on_batch(bf, train=False)
    else:                         # FusedLinearOptTrainer (SGD / Adam) at F = 256, m = 64: a pipelined step, the form an epoch's full batches take
        import test_gpu_linear_opt_step as LO
        net = LO._random_net(256, C, dev, seed=256 + C)
        saturate_head(net, head, k)
        st = LO._store(256, dev)
        tr = LO._trainer(net, kind)
        tr._perm = torch.randperm(st.n_pairs, device=dev)
        x = torch.randn((64, 256), device=dev, generator=torch.Generator(device=dev).manual_seed(11 + C))
        bf = tr.buffers(64)
        bf.xs[0].copy_(x)
        run = lambda: tr.step_on_batch(bf, train=False, batch_advance=32, next_from=st, xi=0)
    return tr, run, copy.deepcopy(net), x


def worst_gradient_error(got, want):
    """max over the parameters of max|got - want| / max|want|."""
    return max((got[n].double() - want[n]).abs().max().item() / want[n].abs().max().item() for n in want)


@pytest.mark.parametrize("head", ["dead", "sharp"])
@pytest.mark.parametrize("kind,C,planes", STEP_FORMS)
def test_step_with_a_saturated_head_vs_float64(dev, monkeypatch, kind, C, planes, head):
    """One step, dropout off, of every step form on a network whose head is saturated -- softmax forward and backward, the normalisation and the IIC
    stage meet with z at (nearly) exact 0 / 1 -- against float64 autograd: the loss 2e-4 relative, every gradient within 2e-3 of its tensor's largest
    entry (the bars of test_gpu_encoder.py::test_default_fused_step_at_cfg2_shape_vs_autograd, test_gpu_small_step.py and
    test_gpu_linear_opt_step.py), everything finite, the planes' overflow flag not raised.
    sharp: W3 and b3 times SHARP_K = 256, the largest power of two at which fp32 torch autograd of the same step (the worst of its gradients, as a
    fraction of that tensor's largest entry) stays within half that gradient bar, 1e-3, against float64 on every form.  Measured on an MI355X,
    fp32 autograd alone at k = 128 / 256 / 512 / 1024 (this test prints the figure at SHARP_K):
        FusedLinearTrainer C = 20    2.1e-5 / 6.2e-5 / 1.5e-4 / 3.1e-4        C = 200    6.4e-5 / 8.6e-5 / 3.2e-4 / 9.5e-4
        FusedSmallTrainer  C = 5     7.8e-5 / 1.7e-4 / 3.3e-2 / 1.0           C = 200    3.3e-5 / 1.1e-4 / 2.9e-4 / 6.7e-4
        FusedLinearOptTrainer C = 20 7.9e-5 / 1.9e-4 / 1.3e-2 / 1.0
    (at k = 512 the head of 5 and 20 units rounds z to exact 0 / 1 in fp32 where float64 still has a gradient); the steps themselves are
    within 2.7e-4 at k = 256.  With the "dead" head fp32 autograd alone is within 4.5e-6 on every form.
    No banding condition on the joint is needed at step level: a cell that fp32 and float64 place on different sides of EPS has P ~ EPS, its term moves
    dP0 by at most EPS x (|log EPS| ~ 35) x w / s, and dlogits by no more."""
    import torch
    tr, run, net0, x = step_case(dev, monkeypatch, kind, C, planes, head)
    run()
    torch.cuda.synchronize()
    loss, want = autograd_step(net0, x, torch.float64)
    _, alone = autograd_step(net0, x, torch.float32)
    names = {id(p): n for n, p in tr.net.named_parameters()}
    got = {names[id(p)]: tr.gradient(i) for i, p in enumerate(tr.params)}
    have = tr.out[0].item()
    print(f"{kind} C={C} planes={planes} {head}: loss {have!r} (float64 {loss!r}); fp32 autograd alone: {worst_gradient_error(alone, want):.2e} of max|want|")
    assert np.isfinite(have) and abs(have - loss) <= 2e-4 * abs(loss), (have, loss)
    assert bool(torch.isfinite(tr.out).all())
    for n, w in want.items():
        assert bool(torch.isfinite(got[n]).all()), n
        err, wmax = (got[n].double() - w).abs().max().item(), w.abs().max().item()
        print(f"  {n}: max gradient error {err / wmax:.2e} of the gradient's max {wmax:.3e}")
        assert err <= 2e-3 * wmax + 1e-12, (n, err, wmax)
    assert all(bool(torch.isfinite(p).all()) for p in tr.params)
    if kind == "linear":
        assert not tr.planes_overflowed()
