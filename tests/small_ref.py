"""float64 restatement of the native step of model_size='small' (csrc/small_step.hip), one function per stage, each taking the arrays
its kernel takes.  Plain numpy: nothing here imports the package under test.  Used by tests/test_small_reference.py (the stages
composed around a float64 InfoNCE / IIC reproduce torch autograd's gradients of myNet, no GPU) and tests/test_gpu_small_stages.py
(each kernel alone against its stage, from the float32 arrays that kernel read).

myNet (reference PytorchUtils.py:6-31): a1 = Dropout(ReLU(x W1^T + b1)) [m, 400]; a2 = LeakyReLU(a1 W2^T + b2) [m, 128];
h = a2 Wi^T + bi [m, 64]; z = Softmax(Dropout(a2) Wc^T + bc) [m, C].  Rows [0, m/2) are the "true" halves of the pairs, row r's
partner is (r + m/2) mod m.  Dropout(0.5) is a keep mask times 2.

Also here: the rounding bars the GPU tests hold the kernels to (product_bound, rmsprop_bound), so that the derivation stands next to
the arithmetic it is about."""
import numpy as np

SLOPE = 0.01            # nn.LeakyReLU() default
U = 2.0 ** -23          # the spacing of float32 at 1 (twice its unit roundoff)
TINY = 2.0 ** -126


def f64(a):
    """Any array-like (a torch tensor on any device included) as a float64 numpy array, exactly."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def partner(m):
    r = np.arange(m)
    return (r + m // 2) % m


# ------------------------------------------------------------------------------------------------ the stages
def l1_fwd(x, W1):
    """idl_small_l1_fwd: a1' = x W1^T (the bias is mid_fwd's)."""
    return f64(x) @ f64(W1).T


def mid_fwd(a1_pre, b1, W2, b2, Wi, bi, Wc, bc, masks=None):
    """idl_small_mid_fwd.  masks: None (eval) or the two keep masks ([m, 400], [m, 128]).  -> a1, a2, d2, f, inv, z."""
    a1 = np.maximum(f64(a1_pre) + f64(b1), 0.0)
    if masks is not None:
        a1 = a1 * (2.0 * f64(masks[0]))
    v = a1 @ f64(W2).T + f64(b2)
    a2 = np.where(v > 0.0, v, SLOPE * v)
    d2 = a2 * (2.0 * f64(masks[1])) if masks is not None else a2
    h = a2 @ f64(Wi).T + f64(bi)
    nrm = np.maximum(np.sqrt((h * h).sum(1)), 1e-12)          # F.normalize's clamp (LossFunctions.py:79)
    f, inv = h / nrm[:, None], 1.0 / nrm
    lg = d2 @ f64(Wc).T + f64(bc)
    e = np.exp(lg - lg.max(1, keepdims=True))
    return a1, a2, d2, f, inv, e / e.sum(1, keepdims=True)


def bwd_rows(z, f, inv, G_parts, dP0, nce_coef, dzs=None):
    """The per-row part of idl_small_mid_bwd: dlogits = softmax backward of the IIC gradient (row r: z_partner(r) dP0, or row
    partner(r) of dzs = z dP0 when dzs is given), dh = normalise backward of nce_coef (sum of G's parts - 2 f_partner)."""
    z, f, inv = f64(z), f64(f), f64(inv)
    m = z.shape[0]
    pr = partner(m)
    dz = f64(dzs)[pr] if dzs is not None else z[pr] @ f64(dP0)
    dlogits = z * (dz - (dz * z).sum(1, keepdims=True))
    G = f64(G_parts)
    G = G.reshape(-1, m, G.shape[-1]).sum(0)
    df = float(nce_coef) * (G - 2.0 * f[pr])
    dh = (df - f * (f * df).sum(1, keepdims=True)) * inv[:, None]
    return dlogits, dh


def bwd_da2(dlogits, dh, a2, Wi, Wc, mask2=None, train=False):
    """da2 = (Dropout'(dlogits Wc) + dh Wi) LeakyReLU'(a2): the classifier's keep mask x 2 (train), the sign of the forward's a2."""
    dd2 = f64(dlogits) @ f64(Wc)
    if train:
        dd2 = dd2 * (2.0 * f64(mask2))
    return (dd2 + f64(dh) @ f64(Wi)) * np.where(f64(a2) > 0.0, 1.0, SLOPE)


def bwd_dr1(da2, a1, W2, train=False):
    """dr1 = (da2 W2) ReLU'/Dropout': a positive a1 is an active and (train) a kept one, x 2."""
    return (f64(da2) @ f64(W2)) * np.where(f64(a1) > 0.0, 2.0 if train else 1.0, 0.0)


def mid_bwd(z, f, inv, G_parts, dP0, a1, a2, W2, Wi, Wc, nce_coef, mask2=None, train=False, dzs=None):
    """idl_small_mid_bwd, after the comment above it in include/idelucs_hip.h: the three parts above in a row (dP0 may be None when dzs
    is given).  -> dlogits, dh, da2, dr1."""
    dlogits, dh = bwd_rows(z, f, inv, G_parts, dP0, nce_coef, dzs)
    da2 = bwd_da2(dlogits, dh, a2, Wi, Wc, mask2, train)
    return dlogits, dh, da2, bwd_dr1(da2, a1, W2, train)


def wgrads(x, dr1, a1, da2, a2, dh, d2, dlogits):
    """The eight gradients of idl_small_wgrad_rms in myNet's parameter order: dW = dy^T xin, db = column sums of dy."""
    out = []
    for dy, xin in ((dr1, x), (da2, a1), (dh, a2), (dlogits, d2)):
        dy = f64(dy)
        out += [dy.T @ f64(xin), dy.sum(0)]
    return out


def rmsprop(p, v, g, hyper, buf=None):
    """torch.optim.RMSprop's update (weight decay, no centring), hyper = [lr, alpha, eps, weight_decay, 1 - alpha(, momentum)]:
    g' = g + wd p; v = alpha v + (1 - alpha) g'^2; without buf: p -= lr g' / (sqrt(v) + eps) -> (p, v); with the momentum buffer:
    buf = mu buf + g' / (sqrt(v) + eps); p -= lr buf -> (p, v, buf)."""
    p, v, g, h = f64(p), f64(v), f64(g), f64(hyper)
    gi = g + h[3] * p
    v = v * h[1] + h[4] * gi * gi
    r = gi / (np.sqrt(v) + h[2])
    if buf is None:
        return p - h[0] * r, v
    buf = f64(buf) * h[5] + r
    return p - h[0] * buf, v, buf


# ------------------------------------------------------------------------------------------------ the bars
def product_bound(A, B, K=None):
    """Elementwise bar of a float32 product A B ([n, K] x [K, p]): (K + 16) 2^-23 sum_k |a_k| |b_k| + 2^-126.  A running float32 sum of
    K exact-or-once-rounded products is off by at most (K - 1 + 1) u sum |a_k b_k| to first order, u = 2^-24; the bar takes one bit
    more than that (2^-23) for the matrix core's internal rounding and the tree of the eight-wave reduction, and 16 for the small K."""
    A, B = np.abs(f64(A)), np.abs(f64(B))
    K = A.shape[1] if K is None else K
    return (K + 16) * U * (A @ B) + TINY


def rmsprop_bound(p, v, g, hyper, buf=None):
    """Bars (first order, then doubled) of one float32 RMSprop update as rmsprop() states it, one rounding (2^-23 of the result: twice the
    half-ulp, which also covers a division or a square root that is not correctly rounded) per operation:
        g' = g + wd p              e_g = U (|g| + |wd p|)                       (two roundings, or one if contracted)
        v' = alpha v + ca g'^2     e_v = 2 ca |g'| e_g + 3 U (|alpha v| + ca g'^2)
        s = sqrt(v'),  d = s + eps e_d = min(e_v / 2s, sqrt(e_v)) + U s + U d   (|sqrt a - sqrt b| <= sqrt |a - b|)
        r = g' / d                 e_r = e_g / d + |r| e_d / d + U |r|
        p' = p - lr r              e_p = lr e_r + U |lr r| + U |p'|
        buf' = mu buf + r          e_b = e_r + U (|mu buf| + |buf'|);  p' = p - lr buf': e_p = lr e_b + U |lr buf'| + U |p'|
    -> (bar of p, bar of v[, bar of buf])."""
    p, v, g, h = f64(p), f64(v), f64(g), f64(hyper)
    gi = g + h[3] * p
    e_g = U * (np.abs(g) + np.abs(h[3] * p))
    v1 = v * h[1] + h[4] * gi * gi
    e_v = 2 * h[4] * np.abs(gi) * e_g + 3 * U * (np.abs(h[1] * v) + h[4] * gi * gi)
    s = np.sqrt(v1)
    d = s + h[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s = np.where(s > 0, np.minimum(e_v / (2 * np.where(s > 0, s, 1.0)), np.sqrt(e_v)), np.sqrt(e_v))
    e_d = e_s + U * s + U * d
    r = gi / d
    e_r = e_g / d + np.abs(r) * e_d / d + U * np.abs(r)
    if buf is None:
        p1 = p - h[0] * r
        return 2 * (h[0] * e_r + U * np.abs(h[0] * r) + U * np.abs(p1)) + TINY, 2 * e_v + TINY
    b1 = f64(buf) * h[5] + r
    e_b = e_r + U * (np.abs(h[5] * f64(buf)) + np.abs(b1))
    p1 = p - h[0] * b1
    return 2 * (h[0] * e_b + U * np.abs(h[0] * b1) + U * np.abs(p1)) + TINY, 2 * e_v + TINY, 2 * e_b + TINY
