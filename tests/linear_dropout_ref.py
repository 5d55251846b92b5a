"""Host references of the NetLinear step under dropout (idelucs_amd/fused.py, fused_opt.py): the two dropout masks of
csrc/mid_fwd_device.h restated in numpy on umap_ref.philox (held to Random123's known answers by test_umap_reference.py), the step
(models.py:117-133) written out in float64 and in fp32 autograd on given masks, and the ragged grid of partial-batch shapes the host
and the GPU tests share."""
import copy

import numpy as np

from umap_ref import philox

H1, H2 = 512, 64


# ---------------------------------------------------------------------------------------------- the masks
def layer1_rows(seed, word, rows):
    """Layer 1's keep mask of the given rows -> [len(rows), 512] bool.  Flat row-major element e = row * 512 + col, group g = e >> 2:
    counter (g, 1, word, g >> 32), key (seed low, seed high); the element is kept when bit 31 of output word e & 3 is set."""
    rows = np.asarray(rows, dtype=np.uint64)
    g = (rows[:, None] * np.uint64(H1 // 4) + np.arange(H1 // 4, dtype=np.uint64)[None, :]).reshape(-1)
    words = philox(g & np.uint64(0xFFFFFFFF), 1, int(word) & 0xFFFFFFFF, g >> np.uint64(32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return (np.stack(words, axis=1) >> np.uint32(31)).astype(bool).reshape(len(rows), H1)


def latent_rows(seed, word, rows):
    """The latent's keep mask of the given rows -> [len(rows), 64] bool.  Counter (row, 2, word, 0): column c is kept when bit c & 31 of
    output word x (c < 32) or y (c >= 32) is set."""
    rows = np.asarray(rows, dtype=np.uint64)
    x, y, _, _ = philox(rows & np.uint64(0xFFFFFFFF), 2, int(word) & 0xFFFFFFFF, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    bits = np.arange(32, dtype=np.uint32)[None, :]
    return np.concatenate([(x[:, None] >> bits) & np.uint32(1), (y[:, None] >> bits) & np.uint32(1)], axis=1).astype(bool)


def masks(seed, word, m):
    """The keep masks of one step on m rows -> (mask1 [m, 512] bool, mask2 [m, 64] bool); kept units are doubled.  seed: the trainer's
    64-bit seed; word: the low 32 bits of ctl[0], (voter & 0xFF) << 24 plus the steps taken since begin_voter."""
    rows = np.arange(m)
    return layer1_rows(seed, word, rows), latent_rows(seed, word, rows)


# ---------------------------------------------------------------------------------------------- the partial-batch grid
RAGGED_M = [2, 18, 34, 48, 96, 200, 440]
RAGGED_C = [5, 48, 49, 64, 65, 200, 256]
RAGGED_F = [10, 136, 256]
# every m with every C; the width alternates so that every m and every C meets every width (7 is no multiple of 3)
RAGGED_GRID = [(m, C, RAGGED_F[(i + j) % 3]) for i, m in enumerate(RAGGED_M) for j, C in enumerate(RAGGED_C)]


# ---------------------------------------------------------------------------------------------- the step
def _same_branch(want, have, pre, bound, name):
    """The units the float64 forward keeps (want) and the ones the trainer kept (have) are the same set, but for units whose float64
    pre-activation lies within fp32 rounding of zero: |pre| <= 1e-5 x sum |x_k| |w_k| (some 170 fp32 epsilons of the dot product's
    terms), and no more than 1e-4 of all units."""
    mism = want != have
    n = int(mism.sum().item())
    print(f"  {name}: {n} of {mism.numel()} units at a ReLU kink" + (f" (|pre| / bound <= {float((pre.abs()[mism] / bound[mism]).max()):.1e})" if n else ""))
    if n:
        assert bool((pre.abs()[mism] <= 1e-5 * bound[mism]).all()), (name, n, float((pre.abs()[mism] / bound[mism]).max()))
        assert n <= 1e-4 * mism.numel(), (name, n)


def _autograd_step(net, x, kept, masks=None):
    """The reference step (models.py:117-133) written out on a float64 copy of net: dropout off, or the given keep masks x 2 in place of
    nn.Dropout.  -> (loss, [6 gradients as float32]).
    kept = (layer 1's output > 0 [m, 512], the classifier's masked latent > 0 [m, 64]) of the trainer's step on the same parameters: ReLU
    has no derivative at 0, and a unit whose pre-activation is zero to fp32 rounding falls on either side of it in two correct forwards --
    its whole contribution to the weight gradients (one sample's outer product: 1e-2 of dW1's largest entry at F = 256) then differs, which
    says nothing about either step.  The reference therefore differentiates the branch the trainer took, after checking (_same_branch) that
    the two forwards chose differently at such units only."""
    import torch
    import torch.nn.functional as Fn
    from idelucs_amd.LossFunctions import IID_loss
    ref = copy.deepcopy(net).double()
    x = x.double()
    l1, l2, l3 = ref.layers[0], ref.layers[3], ref.classifier[2]
    ps = [l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias]
    scale = 2.0 if masks is not None else 1.0
    with torch.no_grad():
        pre1 = Fn.linear(x, l1.weight, l1.bias)
        want1 = (pre1 > 0) & masks[0] if masks is not None else pre1 > 0
        _same_branch(want1, kept[0], pre1, Fn.linear(x.abs(), l1.weight.abs(), l1.bias.abs()), "layer 1")
    a1 = Fn.linear(x, l1.weight, l1.bias) * kept[0].double() * scale
    h = Fn.linear(a1, l2.weight, l2.bias)
    with torch.no_grad():
        want2 = (h > 0) & masks[1] if masks is not None else h > 0
        _same_branch(want2, kept[1], h, Fn.linear(a1.abs(), l2.weight.abs(), l2.bias.abs()), "the latent")
    r2 = h * kept[1].double() * scale
    z = torch.softmax(Fn.linear(r2, l3.weight, l3.bias), dim=1)
    b = x.shape[0] // 2
    f = Fn.normalize(h, dim=1)                          # info_nce_loss (LossFunctions.py:65-98) without its cast to float32
    s = (f @ f.t()) / 0.85
    r = torch.arange(2 * b, device=s.device)
    pos = s[r, (r + b) % (2 * b)]
    s = s.masked_fill(r.unsqueeze(0) == r.unsqueeze(1), float("-inf"))
    nce = (torch.logsumexp(s, dim=1) - pos).mean()
    loss = 0.75 * nce + 0.25 * IID_loss(z[:b], z[b:], lamb=2.8)
    loss.backward()
    return float(loss.item()), [p.grad.detach().float().clone() for p in ps]


def fp32_autograd_step(net, x, masks=None):
    """The same step as plain fp32 torch autograd on a copy of net, the library's own relu, losses and branches: what a correct fp32
    implementation that is none of this package's kernels gives.  -> (loss, [6 gradients], kept as _autograd_step takes it)."""
    import torch
    import torch.nn.functional as Fn
    from idelucs_amd.LossFunctions import IID_loss, info_nce_loss
    ref = copy.deepcopy(net).float()
    x = x.float()
    l1, l2, l3 = ref.layers[0], ref.layers[3], ref.classifier[2]
    ps = [l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias]
    a1 = torch.relu(Fn.linear(x, l1.weight, l1.bias))
    if masks is not None:
        a1 = a1 * masks[0].float() * 2.0
    h = Fn.linear(a1, l2.weight, l2.bias)
    r2 = torch.relu(h)
    if masks is not None:
        r2 = r2 * masks[1].float() * 2.0
    z = torch.softmax(Fn.linear(r2, l3.weight, l3.bias), dim=1)
    b = x.shape[0] // 2
    loss = 0.75 * info_nce_loss(h[:b], h[b:], 0.85) + 0.25 * IID_loss(z[:b], z[b:], lamb=2.8)
    loss.backward()
    return float(loss.item()), [p.grad.detach().clone() for p in ps], (a1.detach() > 0, r2.detach() > 0)
