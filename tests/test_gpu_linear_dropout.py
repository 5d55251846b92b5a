"""GPU tests of the default trainer (idelucs_amd/fused.py: NetLinear + RMSprop) under dropout and on partial batches, against the host
restatement of the masks and the float64 step of tests/linear_dropout_ref.py (held to a scalar Philox and to fp32 autograd by
tests/test_linear_dropout_reference.py):
  a. the unfused kernels draw the restated masks bit for bit;
  b. three consecutive pipelined steps with dropout on, of every launch sequence FusedLinearTrainer._form picks between;
  c. the partial last batch of an epoch (one non-pipelined step) over a ragged grid of shapes, dropout on and off."""
import copy

import pytest

import linear_dropout_ref as R

pytestmark = pytest.mark.gpu

NAMES = ["layers.0.weight", "layers.0.bias", "layers.3.weight", "layers.3.bias", "classifier.2.weight", "classifier.2.bias"]
SEED, VOTER = 5, 3
WORD0 = VOTER << 24
BIG_SEED = (7 << 32) + 11


@pytest.fixture(scope="module")
def dev():
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda")


# ================================================================================================ a. the kernels draw the restated masks
@pytest.mark.parametrize("seed", [SEED, BIG_SEED])
@pytest.mark.parametrize("word", [0, (3 << 24) + 1, 0xFFFFFFFF])
@pytest.mark.parametrize("m", [2, 18, 200])
def test_unfused_kernels_draw_the_restated_masks(dev, m, word, seed):
    import torch
    from idelucs_amd import _lib
    from idelucs_amd.fused import _p, _stream
    L = _lib.lib
    mask1, mask2 = (torch.from_numpy(a).to(dev) for a in R.masks(seed, word, m))
    ctl = torch.tensor([word, 0], dtype=torch.int64, device=dev)
    a1 = torch.ones((m, 512), device=dev)
    _lib.check(L.idl_relu_dropout_fwd(_p(a1), a1.numel(), 1, seed, _p(ctl), 1, _stream()))
    lat = torch.ones((m, 64), device=dev)
    C = 5
    W3, b3 = torch.zeros((C, 64), device=dev), torch.zeros(C, device=dev)
    f, inv, r2, z = torch.empty((m, 64), device=dev), torch.empty(m, device=dev), torch.full((m, 64), -1.0, device=dev), torch.empty((m, C), device=dev)
    _lib.check(L.idl_head_fwd(_p(lat), _p(W3), _p(b3), m, C, 1, seed, _p(ctl), _p(f), _p(inv), _p(r2), _p(z), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(a1, 2.0 * mask1.float()), f"layer 1: {int((a1 != 2.0 * mask1.float()).sum())} of {a1.numel()} entries"
    assert torch.equal(r2, 2.0 * mask2.float()), f"the latent: {int((r2 != 2.0 * mask2.float()).sum())} of {r2.numel()} entries"
    assert ctl.tolist() == [word, 0]                      # (the kernels read the step word; only a step's last launch advances it)


# ================================================================================================ what b and c share
_STORES = {}


def _store(dev, F, n=400, seed=3):
    """test_gpu_encoder._cfg2_store_and_net's feature store at F columns: 4 views x n frequency-like rows, the mimic views perturbed copies."""
    import torch
    from idelucs_amd import utils as U
    if F not in _STORES:
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        base = torch.rand((1, n, F), device=dev, generator=g) + 0.5
        feats = base * (1.0 + 0.05 * torch.randn((4, n, F), device=dev, generator=g))
        feats = (feats / feats.sum(2, keepdim=True)).contiguous()
        mean, scale = U.col_stats(feats[0])
        _STORES[F] = U.FeatureStore(None, None, feats, mean, scale, 6, False)
    return _STORES[F]


def _net(dev, F, C, seed):
    """NetLinear(F, C) after weights_init, the biases 0.1 randn (weights_init leaves them at a constant: every bias term matters)."""
    import torch
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.models import weights_init
    torch.manual_seed(seed)
    net = NetLinear(F, C)
    net.apply(weights_init)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape))
    return net.to(dev)


def _trainer(dev, net, store, perm_seed=9):
    import torch
    from idelucs_amd.fused import FusedLinearTrainer
    tr = FusedLinearTrainer(net, lr=1e-3, weight=0.25, lamb=2.8, seed=SEED)
    tr.begin_voter(VOTER)
    tr._keep_w1_grad = True                              # the dW1 tiles also write dW1 out (the timed step never does)
    gen = torch.Generator(device=dev)
    gen.manual_seed(perm_seed)
    tr._perm = torch.randperm(store.n_pairs, device=dev, generator=gen)
    tr.ctl[1:2].zero_()
    tr.out[1:2].zero_()
    return tr


def _shadow(tr):
    import torch
    params = [p.detach().clone().requires_grad_(True) for p in tr.params]
    return params, torch.optim.RMSprop(params, lr=1e-3, weight_decay=0.01)


def _check_step(dev, tr, bf, xi, before, x, word, train, shadow, label):
    """One finished step of tr on the batch x from the parameters `before`: loss and the six gradients against float64 on the restated masks
    of step word `word` (the branches the trainer took, which _same_branch holds to (pre > 0) & mask), then RMSprop on the trainer's own
    gradients against torch.optim's."""
    import torch
    m = bf.m
    mk = tuple(torch.from_numpy(a).to(dev) for a in R.masks(SEED, word, m)) if train else None
    kept = (tr.layer1_output(bf, xi) > 0, bf.r2 > 0)
    assert tuple(kept[0].shape) == (m, 512)
    print(f"{label}:")
    loss_ref, grads_ref = R._autograd_step(before, x, kept, masks=mk)
    _, grads32, _ = R.fp32_autograd_step(before, x, mk)
    got = tr.out[0].item()
    print(f"  loss {got:.7f} float64 {loss_ref:.7f} (off by {abs(got - loss_ref) / abs(loss_ref):.1e})")
    assert torch.isfinite(tr.out).all() and abs(got - loss_ref) <= 2e-4 * abs(loss_ref), (label, got, loss_ref)
    worst = [0.0, 0.0]
    for i, n_ in enumerate(NAMES):
        have, want = tr.gradient(i), grads_ref[i]
        top = want.abs().max().item()
        assert top > 0 and bool(torch.isfinite(have).all()), (label, n_)
        err, err32 = (have - want).abs().max().item() / top, (grads32[i] - want).abs().max().item() / top
        worst = [max(worst[0], err), max(worst[1], err32)]
        print(f"  {n_}: gradient error {err:.2e} of the gradient's max (fp32 autograd, its own branches: {err32:.2e})")
        assert err <= 2e-3, (label, n_, err)
    print(f"  worst gradient error {worst[0]:.2e}; fp32 autograd's own {worst[1]:.2e}")
    sparams, sopt = shadow
    for p, i in zip(sparams, range(6)):
        p.grad = tr.gradient(i).clone()
    sopt.step()
    for n_, p, want in zip(NAMES, tr.params, sparams):
        p, want = p.detach(), want.detach()
        assert bool(torch.isfinite(p).all()), (label, n_)
        bad = (p - want).abs() > 1e-5 * want.abs().max().item()
        # a first RMSprop step is lr * g / (0.1 |g| + eps), the sign of g: where the bias partials are summed in another order a near-zero
        # gradient may flip (test_default_fused_step_at_cfg2_shape_vs_autograd); a weight never
        assert bad.float().mean().item() <= (2e-3 if p.dim() == 1 else 0.0), (label, n_, int(bad.sum()), (p - want).abs().max().item() / want.abs().max().item())
    with torch.no_grad():                                # the next step's shadow starts where the trainer stands; its running averages stay
        for p, q in zip(sparams, tr.params):
            p.copy_(q)
    assert not tr.planes_overflowed()


# ================================================================================================ b. every form, three pipelined steps
# (id, the form, early (general only), IDELUCS_PLANES, VARIANTS entries, m, F, C).  The rows at F = 1024 and below are the smallest shapes each
# form takes; there the dW1 launch has fewer than 144 tiles, so a planes step ends with a dW1 launch and a tail of its own whatever the
# ending's variants say.  The rows at F = 2560 (160 tiles on 256 CUs) are the default six launches -- the forward middle inside the sums
# launch, the tail on the dW1 tiles' loader waves -- and the variants that really take another ending.  The tiles form's small shape is
# F = 256: its dW1 tiles need F % 128 == 0, so F = 192 is refused.
FORM_CASES = [
    ("planes-256-1024-20", "planes", None, "1", {}, 256, 1024, 20),
    ("planes-128-1024-5", "planes", None, "1", {}, 128, 1024, 5),
    ("planes-sums_fwd0-256-1024-20", "planes", None, "1", {"sums_fwd": "0"}, 256, 1024, 20),
    ("planes-tail_reduce-256-1024-20", "planes", None, "1", {"planes_tail": "reduce"}, 256, 1024, 20),
    ("planes-wgrad0-256-1024-48", "planes", None, "1", {"planes_wgrad": "0"}, 256, 1024, 48),
    ("planes-256-2560-20", "planes", None, "1", {}, 256, 2560, 20),
    ("planes-sums_fwd0-256-2560-20", "planes", None, "1", {"sums_fwd": "0"}, 256, 2560, 20),
    ("planes-tail_reduce-256-2560-48", "planes", None, "1", {"planes_tail": "reduce"}, 256, 2560, 48),
    ("planes_rows-256-2560-49", "planes_rows", None, "1", {}, 256, 2560, 49),
    ("planes_rows-256-2560-200", "planes_rows", None, "1", {}, 256, 2560, 200),
    ("tiles-256-1024-20", "tiles", None, "0", {}, 256, 1024, 20),
    ("tiles-32-256-5", "tiles", None, "0", {}, 32, 256, 5),
    ("general-early-48-128-20", "general", True, "1", {}, 48, 128, 20),
    ("general-early-256-1024-64", "general", True, "0", {}, 256, 1024, 64),
    ("general-early-256-1024-200", "general", True, "0", {}, 256, 1024, 200),
    ("general-late-200-256-20", "general", False, "1", {}, 200, 256, 20),
    ("general-late-200-256-200", "general", False, "1", {}, 200, 256, 200),
    ("general-late-64-10-5", "general", False, "1", {}, 64, 10, 5),
]


def test_form_cases_cover_every_form():
    forms = {(c[1], c[2]) for c in FORM_CASES}
    assert forms == {("planes", None), ("planes_rows", None), ("tiles", None), ("general", True), ("general", False)}
    gen = [c for c in FORM_CASES if c[1] == "general"]
    assert any(c[2] and c[7] <= 48 for c in gen) and any(c[2] and 48 < c[7] <= 64 for c in gen) and any(c[2] and c[7] > 64 for c in gen)
    assert any(not c[2] and c[5] % 16 != 0 for c in gen) and any(not c[2] and c[6] % 4 != 0 for c in gen)
    assert any(not c[2] and c[7] <= 48 for c in gen) and any(not c[2] and c[7] > 64 for c in gen)
    assert {k for c in FORM_CASES for k in c[4]} == {"sums_fwd", "planes_tail", "planes_wgrad"}
    assert all(c[5] <= 256 and c[6] <= 2560 for c in FORM_CASES)      # nothing at the workload's size


def _next_batch_is(tr, bf, xi, want, late):
    """The batch the step assembled is `want`, bit for bit: in bf.x (the step's last launch assembled it), in the other x buffer, or -- a
    plane form that wrote the planes only -- within the planes' reconstruction bound (test_default_fused_step_at_cfg2_shape_vs_autograd)."""
    import torch
    from idelucs_amd import _lib
    pb = getattr(bf, "_planes", None)
    if late:
        assert torch.equal(bf.x, want)
    elif pb is not None and not pb["x32"][1 - xi]:
        k = int(_lib.lib.idl_planes_exponent(0))
        back = (pb["xh"][1 - xi].view(torch.float16).double() + pb["xl"][1 - xi].view(torch.float16).double()) * 2.0 ** -k
        err = (back - want.double()).abs()
        assert pb["valid"][1 - xi] and bool((err <= torch.clamp(want.double().abs() * 2.0 ** -21, min=2.0 ** (-25 - k))).all())
    else:
        assert torch.equal(bf.xs[1 - xi], want)


@pytest.mark.parametrize("form,early,planes,variants,m,F,C", [c[1:] for c in FORM_CASES], ids=[c[0] for c in FORM_CASES])
def test_three_pipelined_dropout_steps_of_every_form_vs_float64(dev, monkeypatch, form, early, planes, variants, m, F, C):
    import torch
    from idelucs_amd import fused
    monkeypatch.setenv("IDELUCS_PLANES", planes)
    monkeypatch.setattr(fused, "_PLANES_DISABLED", False)
    for k_, v in variants.items():
        monkeypatch.setitem(fused.VARIANTS, k_, v)
    store, net = _store(dev, F), _net(dev, F, C, seed=F + m + C)
    tr = _trainer(dev, net, store)
    B = m // 2
    bf = tr.buffers(m)
    assert tr._form(bf, store) == form, (tr._form(bf, store), form)
    if form == "general":
        assert tr._early(bf, store) == early
    tr._gather(store, bf)                                # prologue: batch 0 into bf.xs[0]
    shadow = _shadow(tr)
    for k in range(3):
        before = copy.deepcopy(net)
        tr._full_step(store, bf, train=True, pipelined=True, xi=k % 2)
        torch.cuda.synchronize()
        x = store.gather_pairs(tr._perm[k * B:(k + 1) * B])
        _check_step(dev, tr, bf, k % 2, before, x, WORD0 + k, True, shadow, f"{form} m={m} F={F} C={C} step {k}")
        assert tr.ctl.tolist() == [WORD0 + k + 1, (k + 1) * B]
        _next_batch_is(tr, bf, k % 2, store.gather_pairs(tr._perm[(k + 1) * B:(k + 2) * B]), late=form == "general" and not early)


# ================================================================================================ c. the partial last batch
def _branches(m, C, F):
    """The branches of a non-pipelined general step (FusedLinearTrainer._step_general with no store) at this shape."""
    return {"unfused forward" if m % 16 else "idl_mid_fwd", "unfused InfoNCE" if m % 32 else "fused InfoNCE",
            "idl_mid_bwd" if C <= 48 else ("idl_head_bwd" if C <= 64 else "idl_head_bwd_dz"),
            "dW1 tiles" if (m % 32 == 0 and F >= 128 and F % 128 == 0) else "dW1 library product"}


def test_ragged_grid_meets_every_branch():
    assert R.RAGGED_GRID == [(m, C, R.RAGGED_F[(i + j) % 3]) for i, m in enumerate(R.RAGGED_M) for j, C in enumerate(R.RAGGED_C)]
    assert R.RAGGED_M == [2, 18, 34, 48, 96, 200, 440] and R.RAGGED_C == [5, 48, 49, 64, 65, 200, 256] and R.RAGGED_F == [10, 136, 256]
    met = set().union(*(_branches(*c) for c in R.RAGGED_GRID))
    assert met == {"unfused forward", "idl_mid_fwd", "unfused InfoNCE", "fused InfoNCE", "idl_mid_bwd", "idl_head_bwd", "idl_head_bwd_dz",
                   "dW1 tiles", "dW1 library product"}
    # each backward with each forward, and the dW1 tiles (m = 96, F = 256) behind the one-launch backward and behind the separate kernels
    for bwd in ("idl_mid_bwd", "idl_head_bwd", "idl_head_bwd_dz"):
        for fwd in ("unfused forward", "idl_mid_fwd"):
            assert any({bwd, fwd} <= _branches(*c) for c in R.RAGGED_GRID), (bwd, fwd)
    for bwd in ("idl_mid_bwd", "idl_head_bwd_dz"):
        assert any({bwd, "dW1 tiles"} <= _branches(*c) for c in R.RAGGED_GRID), bwd


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("m,C,F", R.RAGGED_GRID)
def test_partial_last_batch_step_vs_float64(dev, m, C, F, train):
    """What run_epoch does with the pairs a last full batch leaves over: one non-pipelined step on buffers of their own."""
    import torch
    from idelucs_amd import _lib
    store, net = _store(dev, F), _net(dev, F, C, seed=1000 * m + C)
    tr = _trainer(dev, net, store, perm_seed=m + C)
    bf = tr.buffers(m)
    assert tr._form(bf, None) == "general"
    assert bf.nce_fused == (m % 32 == 0) and bool(_lib.lib.idl_wgrad_supported(m, 512, F)) == ("dW1 tiles" in _branches(m, C, F))
    before, shadow = copy.deepcopy(net), _shadow(tr)
    tr._full_step(store, bf, train=train)
    torch.cuda.synchronize()
    x = store.gather_pairs(tr._perm[:m // 2])
    assert torch.equal(bf.x, x)
    _check_step(dev, tr, bf, 0, before, x, WORD0, train, shadow, f"partial batch m={m} C={C} F={F} train={train}")
    assert tr.ctl.tolist() == [WORD0 + 1, m // 2]
