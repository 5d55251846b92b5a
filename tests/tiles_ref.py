"""Exact operands and float64 references for the MFMA product kernels (csrc/l1_device.h, wgrad_device.h, l1_planes_device.h,
wgrad_planes_device.h, at_b_tile.inc).  numpy only; imports nothing of the package.

With operands that are small integers every product and every partial sum of a contraction is an integer below 2^24: exactly representable
in fp32 (and in an MFMA's fp32 accumulator), whatever the order of the additions.  A kernel's output element then has to be the float64
product's value bit for bit, and a wrong index -- a swizzle slip, a chunk lost, a pad column read, a plane product that should be absent --
is an exact mismatch at a named element.  exact_ok() is that condition on the inputs; the shapes and cases the GPU test runs are listed HERE so
that the CPU test (test_tiles_reference.py) checks it for every one of them.

Contracts (as the kernels' headers state them):
  idl_l1_fwd                  a1^T = W1 x^T                                   [512][m]
  idl_wgrad_rmsprop           grad = dy^T x                                   [n_out][n_in]
  idl_l1_planes               part[s] = 2^-(W_EXP + X_EXP) sum_{k in slice s} (w0 x0 + w0 x1 + w1 x0)     [8][n_out][m]; _rows: [8][m][n_out]
  idl_wgrad_rmsprop_xplanes   grad = 2^-(k + X_EXP) sum_m (dy0 x0 + dy0 x1 + dy1 x0), k = word 0 of the scale words
  idl_at_b                    out = A^T B                                     [M][N]
  RMSprop epilogue            gi = g + wd p;  v = alpha v + (1 - alpha) gi^2;  p -= lr gi / (sqrt(v) + eps)
"""
import functools
import zlib

import numpy as np

W_EXP, X_EXP = 12, 3          # csrc/planes.h (the GPU test asserts idl_planes_exponent agrees)
KSPLIT = 8                    # K slices of idl_l1_planes
H1 = 512                      # idl_l1_fwd's hidden width
NAN16 = 0x7E00                # an fp16 NaN as int16 bits: what the pad columns and surrounding rows of a plane hold
LIM = 7                       # operand entries are integers in [-LIM, LIM]

TILES = {"l1_fwd": (64, 32), "wgrad": (64, 128), "l1_planes": (128, 128), "xplanes": (64, 128), "at_b": (16, 16)}      # a workgroup's tile of the output

SHAPES = {
    "l1_fwd": [(32, 192), (32, 256), (96, 192), (128, 320), (256, 4096)],                                     # (m, n_in)
    "wgrad": [(32, 64, 128), (64, 64, 128), (96, 128, 256), (1024, 64, 128), (32, 512, 4096)],                # (m, n_out, n_in)
    "l1_planes": [(128, 128, 1024), (128, 128, 1536), (256, 128, 1024), (128, 512, 1024), (384, 256, 2048)],  # (m, n_out, K)
    "xplanes": [(192, 64, 128), (256, 64, 128), (192, 128, 256), (192, 512, 1024)],                           # (m, n_out, n_in)
    "at_b": [(K, M, N) for K in (1, 127, 128, 129, 511, 512, 513, 640) for (M, N) in ((1, 1), (17, 70), (16, 16), (200, 64))],
}
CASES = ("dense", "address")
XPLANES_K = (0, 10, -3)       # exponents in word 0 of dy's scale words


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------- operand generators

def ints(rng, shape, lim=LIM, p_zero=1.0 / 3.0):
    """dense integers in [-lim, lim] \\ {0} as float32, about p_zero of them replaced by zero"""
    v = rng.integers(1, lim + 1, shape) * rng.choice(np.array([-1, 1]), shape)
    v[rng.random(shape) < p_zero] = 0
    return v.astype(np.float32)


def f16_bits(a):
    """integers (|a| <= 2048, or multiples of a power of two beyond) -> their fp16 images as int16"""
    h = np.asarray(a, np.float64).astype(np.float16)
    assert np.array_equal(h.astype(np.float64), np.asarray(a, np.float64))
    return h.view(np.int16)


def f16_vals(bits):
    return np.asarray(bits, np.int16).view(np.float16).astype(np.float64)


def int_planes(rng, shape):
    """(hi, lo) int16 images of two fp16 planes of small integers; lo is non-zero in two thirds of the entries"""
    return f16_bits(ints(rng, shape)), f16_bits(ints(rng, shape))


def one_per_row(rng, rows, K):
    """[rows][K] with a single 1 per row at a pseudo-random k -> (matrix float32, k of each row)"""
    k = rng.integers(0, K, rows)
    a = np.zeros((rows, K), np.float32)
    a[np.arange(rows), k] = 1.0
    return a, k


@functools.lru_cache(maxsize=None)
def operands(kernel, shape, case):
    """The operands of (kernel, shape, case): a dict of numpy arrays, fp32 matrices or int16 plane images, the same on every call.
    case "dense": integers in [-7, 7], a third of them zero (in both planes of a plane operand).
    case "address": the weight-side operand has a single 1 per output row (in each plane: at different places), the other operand holds a code of
    its own position -- an output element IS an entry (plane kernels: a sum of three) of the other operand."""
    rng = _rng(kernel, shape, case)
    if kernel == "l1_fwd":
        m, K = shape
        if case == "dense":
            return {"W": ints(rng, (H1, K)), "x": ints(rng, (m, K))}
        W, k = one_per_row(rng, H1, K)
        return {"W": W, "x": (np.arange(m)[:, None] * K + np.arange(K)[None, :]).astype(np.float32), "k": k}       # out[h][r] = r K + k_h
    if kernel == "wgrad":
        m, H, F = shape
        if case == "dense":
            return {"dy": ints(rng, (m, H)), "x": ints(rng, (m, F))}
        dyT, k = one_per_row(rng, H, m)
        return {"dy": np.ascontiguousarray(dyT.T), "x": (np.arange(m)[:, None] * F + np.arange(F)[None, :]).astype(np.float32), "k": k}    # grad[h][f] = m_h F + f
    if kernel == "at_b":
        K, M, N = shape
        if case == "dense":
            return {"A": ints(rng, (K, M)), "B": ints(rng, (K, N))}
        AT, k = one_per_row(rng, M, K)
        return {"A": np.ascontiguousarray(AT.T), "B": (np.arange(K)[:, None] * N + np.arange(N)[None, :]).astype(np.float32), "k": k}      # out[i][j] = k_i N + j
    if kernel == "l1_planes":
        m, H, K = shape
        if case == "dense":
            wh, wl = int_planes(rng, (H, K))
            xh, xl = int_planes(rng, (m, K))
            return {"wh": wh, "wl": wl, "xh": xh, "xl": xl}
        w0, k = one_per_row(rng, H, K)
        k1 = (k + K // 2) % K                                  # the low plane's 1 sits in another K slice
        w1 = np.zeros_like(w0); w1[np.arange(H), k1] = 1.0
        x0 = np.broadcast_to(np.arange(K)[None, :], (m, K))                         # k itself (K <= 2048: exact in fp16)
        x1 = np.broadcast_to(2048 * (np.arange(m) % 8 + 1)[:, None], (m, K))        # 2048 (r % 8 + 1)
        # slice of k_h: 2^-15 (k_h + 2048 (r % 8 + 1)); slice of k1_h: 2^-15 k1_h; the other six: 0
        return {"wh": f16_bits(w0), "wl": f16_bits(w1), "xh": f16_bits(x0), "xl": f16_bits(x1), "k": k, "k1": k1}
    if kernel == "xplanes":
        m, H, F = shape
        if case == "dense":
            dyh, dyl = int_planes(rng, (m, H))
            xh, xl = int_planes(rng, (m, F))
            return {"dyh": dyh, "dyl": dyl, "xh": xh, "xl": xl}
        d0T, k = one_per_row(rng, H, m)
        k1 = (k + m // 2) % m
        d1T = np.zeros_like(d0T); d1T[np.arange(H), k1] = 1.0
        x0 = np.arange(m)[:, None] + 256 * (np.arange(F) % 8)[None, :]              # m + 256 (f % 8) < 2048
        x1 = np.broadcast_to(2048 * ((np.arange(F) >> 3) % 8 + 1)[None, :], (m, F))
        # grad[h][f] 2^(k + 3) = x0[m_h][f] + x1[m_h][f] + x0[m1_h][f]
        return {"dyh": f16_bits(d0T.T), "dyl": f16_bits(d1T.T), "xh": f16_bits(x0), "xl": f16_bits(x1), "k": k, "k1": k1}
    raise KeyError(kernel)


# ---------------------------------------------------------------- float64 references

def ref_l1_fwd(W, x):
    return np.asarray(W, np.float64) @ np.asarray(x, np.float64).T


def ref_wgrad(dy, x):
    return np.asarray(dy, np.float64).T @ np.asarray(x, np.float64)


def ref_at_b(A, B):
    return np.asarray(A, np.float64).T @ np.asarray(B, np.float64)


def ref_l1_planes(wh, wl, xh, xl, rows=False):
    """part[KSPLIT][n_out][m] (rows: [KSPLIT][m][n_out]); no w1 x1 term"""
    w0, w1, x0, x1 = f16_vals(wh), f16_vals(wl), f16_vals(xh), f16_vals(xl)
    K = w0.shape[1]
    kr = K // KSPLIT
    out = np.empty((KSPLIT, w0.shape[0], x0.shape[0]), np.float64)
    for s in range(KSPLIT):
        sl = slice(s * kr, (s + 1) * kr)
        out[s] = (w0[:, sl] @ (x0[:, sl] + x1[:, sl]).T + w1[:, sl] @ x0[:, sl].T) * 2.0 ** -(W_EXP + X_EXP)
    return np.ascontiguousarray(out.transpose(0, 2, 1)) if rows else out


def ref_full_planes_product(wh, wl, xh, xl):
    """(w0 + w1)(x0 + x1)^T 2^-(W_EXP + X_EXP) over the whole K: what a product WITH the w1 x1 term would give"""
    return (f16_vals(wh) + f16_vals(wl)) @ (f16_vals(xh) + f16_vals(xl)).T * 2.0 ** -(W_EXP + X_EXP)


def ref_xplanes(dyh, dyl, xh, xl, k):
    d0, d1, x0, x1 = f16_vals(dyh), f16_vals(dyl), f16_vals(xh), f16_vals(xl)
    return (d0.T @ (x0 + x1) + d1.T @ x0) * 2.0 ** -(k + X_EXP)


@functools.lru_cache(maxsize=None)
def reference(kernel, shape, case, k=0):
    """The float64 reference of (kernel, shape, case); computed once, shared, read-only."""
    o = operands(kernel, shape, case)
    if kernel == "l1_fwd":
        r = ref_l1_fwd(o["W"], o["x"])
    elif kernel == "wgrad":
        r = ref_wgrad(o["dy"], o["x"])
    elif kernel == "at_b":
        r = ref_at_b(o["A"], o["B"])
    elif kernel == "l1_planes":
        r = ref_l1_planes(o["wh"], o["wl"], o["xh"], o["xl"])
    elif kernel == "xplanes":
        r = ref_xplanes(o["dyh"], o["dyl"], o["xh"], o["xl"], k)
    else:
        raise KeyError(kernel)
    r.setflags(write=False)
    return r


def terms(kernel, o, k=0):
    """The contraction as a list of (A [R][K], B [K][C]) float64 pairs and a power-of-two scale: out = scale sum_pairs A B."""
    f = lambda a: np.asarray(a, np.float64)
    if kernel == "l1_fwd":
        return [(f(o["W"]), f(o["x"]).T)], 1.0
    if kernel == "wgrad":
        return [(f(o["dy"]).T, f(o["x"]))], 1.0
    if kernel == "at_b":
        return [(f(o["A"]).T, f(o["B"]))], 1.0
    if kernel == "l1_planes":
        w0, w1, x0, x1 = f16_vals(o["wh"]), f16_vals(o["wl"]), f16_vals(o["xh"]), f16_vals(o["xl"])
        return [(w0, x0.T), (w0, x1.T), (w1, x0.T)], 2.0 ** -(W_EXP + X_EXP)
    if kernel == "xplanes":
        d0, d1, x0, x1 = f16_vals(o["dyh"]), f16_vals(o["dyl"]), f16_vals(o["xh"]), f16_vals(o["xl"])
        return [(d0.T, x0), (d0.T, x1), (d1.T, x0)], 2.0 ** -(k + X_EXP)
    raise KeyError(kernel)


def exact_ok(pairs, scale=1.0):
    """The condition under which a sum of products is the same fp32 bits in ANY order: every term is an integer multiple of one power-of-two quantum
    (here: integer operands, unit = scale) and, for every output element, sum |term| / unit < 2^24 -- so every partial sum of every subset is an
    integer below 2^24 times the unit; the scale is a power of two that keeps the result a normal fp32 number.  A condition on the inputs."""
    total = 0.0
    for A, B in pairs:
        if not (np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B))):
            return False
        total = total + np.abs(A) @ np.abs(B)
    m, e = np.frexp(scale)
    return bool(m == 0.5 and -100 < e < 100 and total.max() < 2.0 ** 24)


# ---------------------------------------------------------------- the RMSprop epilogue

def hyper(lr, alpha, eps=1e-8, wd=0.01):
    """[lr, alpha, eps, weight_decay, 1 - alpha] as the fp32 words the kernels read"""
    a = np.float32(alpha)
    return np.array([lr, a, eps, wd, np.float32(1.0) - a], np.float32)


def rmsprop64(g, W, V, hy):
    """The update of wgrad_device.h in float64 from an exact gradient -> (W', V', step), step = lr gi / (sqrt(v) + eps)"""
    lr, alpha, eps, wd, oma = (float(h) for h in hy)
    g, W, V = np.asarray(g, np.float64), np.asarray(W, np.float64), np.asarray(V, np.float64)
    gi = g + wd * W
    v = alpha * V + oma * gi * gi
    step = lr * gi / (np.sqrt(v) + eps)
    return W - step, v, step


def rmsprop32(g, W, V, hy):
    """The same update with every operation a correctly rounded fp32 one (numpy: no FMA, IEEE sqrt and division), in torch.optim.RMSprop's order"""
    lr, alpha, eps, wd, oma = (np.float32(h) for h in hy)
    g, W, V = np.asarray(g, np.float32), np.asarray(W, np.float32), np.asarray(V, np.float32)
    gi = g + wd * W
    v = V * alpha + (oma * gi) * gi
    step = lr * (gi / (np.sqrt(v) + eps))
    out = W - step
    assert out.dtype == v.dtype == np.float32
    return out, v


V_BAR, W_BAR = 8.0, 12.0      # in units of 2^-24: V relative; W: (|dW| - 0.5 ulp(W)) / |step|


def epilogue_deviation(W_got, V_got, g, W0, V0, hy):
    """Largest deviation of an fp32 update from rmsprop64 in the units of the bars: (V: |dV| / (2^-24 V), W: (|dW| - 0.5 ulp(W)) / (2^-24 |step|)).
    ulp(W) is the spacing of fp32 where the result lies (the larger of the two values' binades)."""
    Wr, Vr, step = rmsprop64(g, W0, V0, hy)
    u = 2.0 ** -24
    dv = np.abs(np.asarray(V_got, np.float64) - Vr) / (u * Vr)
    ulp = np.spacing(np.maximum(np.abs(np.asarray(W_got, np.float32)), np.abs(Wr).astype(np.float32))).astype(np.float64)
    dw = (np.abs(np.asarray(W_got, np.float64) - Wr) - 0.5 * ulp) / (u * np.abs(step))
    return float(dv.max()), float(dw.max())


def rms_start(g, seed):
    """W0 with 1/64 <= |W0| <= 1 carrying the gradient's sign (g + wd W never cancels, gi != 0), V0 >= 0 (a quarter of it exactly 0)"""
    rng = _rng("rms", seed)
    g = np.asarray(g, np.float64)
    sign = np.where(g != 0, np.sign(g), rng.choice(np.array([-1.0, 1.0]), g.shape))
    W0 = (sign * (1.0 / 64 + (1 - 1.0 / 64) * rng.random(g.shape))).astype(np.float32)
    V0 = (rng.random(g.shape) * np.maximum(g * g, 1e-4) * 4).astype(np.float32)
    V0[rng.random(g.shape) < 0.25] = 0.0
    return W0, V0


# ---------------------------------------------------------------- reporting

def first_mismatch(got, want, tile):
    """got (fp32) against want (float64, exactly representable in fp32) by BIT PATTERN.  2-D [rows][cols] or 3-D [slice][rows][cols]; tile = (th, tw).
    -> dict(count, index, slice, tile, in_tile, got, want); count == 0 and the rest None when they agree."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(want), (got.dtype, got.shape, np.shape(want))
    w32 = np.asarray(want, np.float64).astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want), "the reference is not an fp32 number"
    bad = np.ascontiguousarray(got).view(np.int32) != np.ascontiguousarray(w32).view(np.int32)
    count = int(bad.sum())
    if count == 0:
        return {"count": 0, "index": None, "slice": None, "tile": None, "in_tile": None, "got": None, "want": None}
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    r, c = idx[-2], idx[-1]
    return {"count": count, "index": idx, "slice": idx[0] if got.ndim == 3 else None, "tile": (r // tile[0], c // tile[1]),
            "in_tile": (r % tile[0], c % tile[1]), "got": float(got[idx]), "want": float(w32[idx])}


def describe(mm, what=""):
    if mm["count"] == 0:
        return f"{what}: equal"
    s = f"{what}: {mm['count']} elements differ; first at {mm['index']}"
    if mm["slice"] is not None:
        s += f" (K slice {mm['slice']})"
    return s + f", tile {mm['tile']}, in-tile position {mm['in_tile']}: got {mm['got']!r}, want {mm['want']!r}"
