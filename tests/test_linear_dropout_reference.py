"""Host tests of tests/linear_dropout_ref.py, what tests/test_gpu_linear_dropout.py holds the default trainer's kernels to: the restated
dropout masks against a scalar Philox, their properties, and the float64 step against plain fp32 autograd on every shape of the ragged
grid -- the reference's own error, well inside the bars the GPU tests apply."""
import numpy as np
import pytest

import linear_dropout_ref as R

M32 = 0xFFFFFFFF
BIG_SEED = (7 << 32) + 11


def _philox_int(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on Python ints: counter c[4], key k[2] -> four output words."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def _keep1(seed, word, row, col):
    e = row * 512 + col
    g = e >> 2
    return bool(_philox_int([g & M32, 1, word, g >> 32], [seed & M32, seed >> 32])[e & 3] >> 31)


def _keep2(seed, word, row, col):
    out = _philox_int([row, 2, word, 0], [seed & M32, seed >> 32])
    return bool((out[0 if col < 32 else 1] >> (col & 31)) & 1)


def test_scalar_philox_reproduces_the_known_answers():
    """Random123's kat_vectors for philox4x32-10: the scalar the masks are checked with is itself the published generator."""
    assert _philox_int([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox_int([M32] * 4, [M32, M32]) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _philox_int([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("seed,word", [(5, 0), (5, (3 << 24) + 1), (BIG_SEED, M32), (BIG_SEED, (255 << 24) + 7)])
def test_vectorised_masks_equal_a_scalar_philox(seed, word):
    """A handful of (row, col) of both layers: the corners of a group of four, of a row, of the 32-bit halves of the latent's words, rows
    on both sides of 2^16 (2^23 groups) and of 2^25 (the group index's high word becomes 1)."""
    rows = [0, 1, 17, 199, 65535, 65536, 65537, 3 * 65536 + 5, (1 << 25) - 1, 1 << 25, (1 << 25) + 3]
    m1, m2 = R.layer1_rows(seed, word, rows), R.latent_rows(seed, word, rows)
    assert m1.shape == (len(rows), 512) and m2.shape == (len(rows), 64) and m1.dtype == bool and m2.dtype == bool
    for i, row in enumerate(rows):
        for col in (0, 1, 2, 3, 4, 255, 256, 509, 510, 511):
            assert m1[i, col] == _keep1(seed, word, row, col), (row, col)
        for col in (0, 1, 30, 31, 32, 33, 62, 63):
            assert m2[i, col] == _keep2(seed, word, row, col), (row, col)
    a1, a2 = R.masks(seed, word, 18)
    assert np.array_equal(a1, R.layer1_rows(seed, word, range(18))) and np.array_equal(a2, R.latent_rows(seed, word, range(18)))
    assert np.array_equal(a1[:2], m1[:2]) and np.array_equal(a2[17], m2[2])


def test_mask_rows_do_not_depend_on_the_batch_size():
    big1, big2 = R.masks(5, (3 << 24) + 2, 440)
    for m in (2, 18, 200):
        m1, m2 = R.masks(5, (3 << 24) + 2, m)
        assert m1.shape == (m, 512) and m2.shape == (m, 64)
        assert np.array_equal(m1, big1[:m]) and np.array_equal(m2, big2[:m])


def test_masks_of_another_step_voter_layer_or_seed_are_independent():
    seed, word, m = 5, (3 << 24) + 1, 440
    m1, m2 = R.masks(seed, word, m)
    others = {"step": R.masks(seed, word + 1, m), "voter": R.masks(seed, (4 << 24) + 1, m), "seed": R.masks(seed + 1, word, m),
              "seed's high word": R.masks(seed + (1 << 32), word, m)}
    for name, (o1, o2) in others.items():
        for a, b, layer in ((m1, o1, 1), (m2, o2, 2)):
            d = float((a != b).mean())
            print(f"another {name}, layer {layer}: {d:.4f} of the entries differ")
            assert 0.45 <= d <= 0.55, (name, layer, d)
    d = float((m1[:, :64] != m2).mean())                 # the two layers of one step
    print(f"the two layers: {d:.4f} of the entries differ")
    assert 0.45 <= d <= 0.55, d


@pytest.mark.parametrize("seed", [5, BIG_SEED])
def test_keep_rate_is_a_half(seed):
    m1, m2 = R.masks(seed, 3 << 24, 440)
    # (mask2 has 440 x 64 entries: the same interval over seven steps' worth, 197 120 entries, three standard deviations of which are 3.4e-3)
    m2 = np.concatenate([m2] + [R.masks(seed, (3 << 24) + k, 440)[1] for k in range(1, 7)])
    for name, mk in (("layer 1", m1), ("the latent", m2)):
        print(f"{name}: keep rate {mk.mean():.4f} over {mk.size} entries")
        assert 0.49 <= mk.mean() <= 0.51, (name, mk.mean())
    assert 0.49 <= m1.mean() <= 0.51 and m1.shape == (440, 512)


# ---------------------------------------------------------------------------------------------- the float64 step against fp32 autograd
def net_and_batch(F, C, m, seed):
    """NetLinear(F, C) after weights_init with biases 0.1 randn (weights_init leaves them constant: every bias term matters), and a batch
    of m / 2 pairs: standard normal rows and their perturbed copies."""
    import torch
    from idelucs_amd.PytorchUtils import NetLinear
    from idelucs_amd.models import weights_init
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = NetLinear(F, C)
    net.apply(weights_init)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    a = torch.randn((m // 2, F), generator=g)
    return net, torch.cat([a, a + 0.3 * torch.randn((m // 2, F), generator=g)])


def test_ragged_grid_covers_the_lists():
    assert len(R.RAGGED_GRID) == 49 and len(set(R.RAGGED_GRID)) == 49
    assert {c[0] for c in R.RAGGED_GRID} == set(R.RAGGED_M) and {c[1] for c in R.RAGGED_GRID} == set(R.RAGGED_C)
    for m in R.RAGGED_M:
        assert {c[2] for c in R.RAGGED_GRID if c[0] == m} == set(R.RAGGED_F)
    for C in R.RAGGED_C:
        assert {c[2] for c in R.RAGGED_GRID if c[1] == C} == set(R.RAGGED_F)


# A case whose two loss terms cancel (0.75 InfoNCE + 0.25 IIC = 3.8e-4 at seed 96 048 with dropout on, where fp32's absolute error of 1e-7 is
# 2.8e-4 of it) measures the cancellation, not the step: it takes another seed.
_OTHER_SEED = {(96, 48, 256): 7}


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("m,C,F", R.RAGGED_GRID)
def test_float64_step_and_fp32_autograd_agree_inside_the_bars(m, C, F, train):
    """The step on the masks of voter 3's first step, seed 5 (what the GPU test of the partial batch draws): fp32 autograd and the float64
    reference agree to 5e-5 of the loss and 2e-4 of each gradient's largest entry -- a quarter and a tenth of the bars the kernels are
    held to --, no unit lies on different sides of a ReLU kink, every gradient is non-zero and the loss is finite."""
    import torch
    net, x = net_and_batch(F, C, m, seed=_OTHER_SEED.get((m, C, F), 1000 * m + C))
    mk = tuple(torch.from_numpy(a) for a in R.masks(5, 3 << 24, m)) if train else None
    loss32, g32, kept = R.fp32_autograd_step(net, x, mk)
    loss64, g64 = R._autograd_step(net, x, kept, mk)
    with torch.no_grad():                                # the float64 forward's own branches: the same sets, not merely close to them
        pre1 = torch.nn.functional.linear(x.double(), net.layers[0].weight.double(), net.layers[0].bias.double())
        want1 = (pre1 > 0) & mk[0] if train else pre1 > 0
        h = torch.nn.functional.linear(pre1 * want1 * (2.0 if train else 1.0), net.layers[3].weight.double(), net.layers[3].bias.double())
        want2 = (h > 0) & mk[1] if train else h > 0
    assert torch.equal(want1, kept[0]) and torch.equal(want2, kept[1]), "a unit on different sides of a kink: another seed for this case"
    assert np.isfinite(loss64) and np.isfinite(loss32)
    print(f"m={m} C={C} F={F} train={train}: loss {loss64:.7f}, fp32 off by {abs(loss32 - loss64) / abs(loss64):.1e}")
    assert abs(loss32 - loss64) <= 5e-5 * abs(loss64), (loss32, loss64)
    for i, (a, b) in enumerate(zip(g32, g64)):
        top = b.abs().max().item()
        assert top > 0 and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), i
        err = (a - b).abs().max().item() / top
        assert err <= 2e-4, (i, err)
