"""idelucs_amd.predict_native -- NetLinear's eval forward on this package's own launches (predict='native').

nn.Linear runs on hipBLASLt, whose choice of solution -- and with it the summation order of every output -- depends on the product's shape,
on the library version and on whether online tuning ran.  Here a row's outputs are a function of that row and of the weights alone:

    idl_l1_fwd       a1^T = W1 x^T on fp32 MFMA tiles (csrc/l1_fwd.hip); an element's summation order depends on F alone
    idl_predict_mid  bias, ReLU, lat = r1 W2^T + b2, ReLU, logits, softmax, its largest value and where (csrc/predict.hip)

so a row shard, another chunk size, the streamed route or a later process with the same weights reproduce a row bit for bit.
Reference: idelucs/PytorchUtils.py:38-50 in eval mode, as called at idelucs/models.py:158-170.

model_size='small' (myNet, idelucs/PytorchUtils.py:13-22 in eval mode; small_predict='native') has the same on csrc/small_predict.hip:

    idl_small_predict_l1   a1 = x W1^T, 128 rows a workgroup with the operands' K stages shared through LDS; the order depends on F' alone
    idl_small_predict_mid  bias, ReLU, a2 = LeakyReLU(r1 W2^T + b2), lat = a2 Wi^T + bi, logits, softmax, its largest value and where
"""
import torch

from . import _lib
from .utils import _ptr as _p, _stream_ptr as _stream

_L = _lib.lib
H1, H2 = 512, 64
MAX_BLOCK_ROWS = 32768          # rows of one launch pair (a1_t scratch: 64 MB); a multiple of 32


def supported(F, C):
    """The shapes the two launches take: idl_l1_fwd's F (F % 64 == 0, F >= 192) and idl_predict_mid's 1 <= C <= 256."""
    return F % 64 == 0 and F >= 192 and 1 <= C <= 256


def block_rows(F):
    """Rows of a full block: the largest multiple of 32 up to MAX_BLOCK_ROWS with m * F < 2^29 (idl_l1_fwd_supported)."""
    return min(MAX_BLOCK_ROWS, ((1 << 29) - 1) // F // 32 * 32)


class NativeLinearPredictor:
    """The eval forward of a NetLinear on the device.  The parameters are read in place at every call (no copy): a forward after a training step
    sees the weights that step wrote."""

    def __init__(self, net):
        lin1, lin2, lin3 = net.layers[0], net.layers[3], net.classifier[2]
        self.params = (lin1.weight, lin1.bias, lin2.weight, lin2.bias, lin3.weight, lin3.bias)
        self.F, self.C = int(lin1.weight.shape[1]), int(lin3.weight.shape[0])
        if tuple(lin1.weight.shape) != (H1, self.F) or tuple(lin2.weight.shape) != (H2, H1) or tuple(lin3.weight.shape) != (self.C, H2):
            raise ValueError("NativeLinearPredictor takes a NetLinear: Linear(F, 512), Linear(512, 64), Linear(64, C)")
        if not supported(self.F, self.C):
            raise ValueError(f"predict='native' supports F % 64 == 0, F >= 192 and n_clusters in 1..256 (got F={self.F}, n_clusters={self.C})")
        self._a1_t = None           # [512 * rows of the largest block so far], reused between calls
        self._pad = None            # the last block of a call, zero-padded to a multiple of 32 rows

    def _weights(self):
        for t in self.params:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("predict='native' needs contiguous float32 parameters on the device")
        return [_p(t) for t in self.params]

    def _scratch(self, m, dev):
        if self._a1_t is None or self._a1_t.numel() < H1 * m or self._a1_t.device != dev:
            self._a1_t = torch.empty(H1 * m, dtype=torch.float32, device=dev)
        return self._a1_t

    def _block(self, w, x, m, lat, z, prob, unit):
        """x [m, F] (m % 32 == 0) -> the m rows of lat, z (or None), prob, unit."""
        a1_t = self._scratch(m, x.device)
        _lib.check(_L.idl_l1_fwd(w[0], _p(x), m, self.F, _p(a1_t), _stream()))
        _lib.check(_L.idl_predict_mid(_p(a1_t), w[1], w[2], w[3], w[4], w[5], m, self.C, _p(lat), _p(z), _p(prob), _p(unit), _stream()))

    def forward(self, x, want_z=False):
        """x [n, F] float32 on the device, any n -> (lat float32 [n, 64], prob float32 [n], unit int32 [n], z float32 [n, C] or None)."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.F):
            raise ValueError(f"predict='native' takes a float32 device matrix [n, {self.F}]")
        x = x.contiguous()
        n, dev = x.shape[0], x.device
        w = self._weights()
        lat = torch.empty((n, H2), dtype=torch.float32, device=dev)
        prob = torch.empty(n, dtype=torch.float32, device=dev)
        unit = torch.empty(n, dtype=torch.int32, device=dev)
        z = torch.empty((n, self.C), dtype=torch.float32, device=dev) if want_z else None
        blk = block_rows(self.F)
        for lo in range(0, n, blk):
            r = min(blk, n - lo)
            if r % 32 == 0:
                self._block(w, x[lo:lo + r], r, lat[lo:], z[lo:] if want_z else None, prob[lo:], unit[lo:])
                continue
            # the ragged end: its rows in a zero-padded buffer, the pad rows' outputs dropped
            m = (r + 31) // 32 * 32
            if self._pad is None or self._pad.shape[0] < m or self._pad.device != dev:
                self._pad = torch.zeros((m, self.F), dtype=torch.float32, device=dev)
            pad = self._pad[:m]
            pad[:r].copy_(x[lo:lo + r])
            pad[r:].zero_()
            o_lat = torch.empty((m, H2), dtype=torch.float32, device=dev)
            o_prob = torch.empty(m, dtype=torch.float32, device=dev)
            o_unit = torch.empty(m, dtype=torch.int32, device=dev)
            o_z = torch.empty((m, self.C), dtype=torch.float32, device=dev) if want_z else None
            self._block(w, pad, m, o_lat, o_z, o_prob, o_unit)
            lat[lo:].copy_(o_lat[:r])
            prob[lo:].copy_(o_prob[:r])
            unit[lo:].copy_(o_unit[:r])
            if want_z:
                z[lo:].copy_(o_z[:r])
        return lat, prob, unit, z


# ---------------------------------------------------------------- model_size='small'
SH1, SH2, SLAT = 400, 128, 64


def small_supported(F, C):
    """The shapes the two launches of small_predict.hip take: whole float4s of a row (F % 4 == 0, F >= 4: every canonical row of k >= 2) and
    1 <= C <= 256."""
    return F % 4 == 0 and F >= 4 and 1 <= C <= 256


def small_block_rows(F):
    """Rows of a full block: at most MAX_BLOCK_ROWS with m * F < 2^29 (the launches take any m: no rounding to a tile)."""
    return max(1, min(MAX_BLOCK_ROWS, ((1 << 29) - 1) // F))


class NativeSmallPredictor:
    """The eval forward of a myNet on the device, with NativeLinearPredictor's interface.  The parameters are read in place at every call."""

    def __init__(self, net):
        lin1, lin2, lin_i, lin_c = net.layers[0], net.layers[3], net.instance, net.classifier[1]
        self.params = (lin1.weight, lin1.bias, lin2.weight, lin2.bias, lin_i.weight, lin_i.bias, lin_c.weight, lin_c.bias)
        self.F, self.C = int(lin1.weight.shape[1]), int(lin_c.weight.shape[0])
        if tuple(lin1.weight.shape) != (SH1, self.F) or tuple(lin2.weight.shape) != (SH2, SH1) or tuple(lin_i.weight.shape) != (SLAT, SH2) \
                or tuple(lin_c.weight.shape) != (self.C, SH2):
            raise ValueError("NativeSmallPredictor takes a myNet: Linear(F, 400), Linear(400, 128), heads Linear(128, 64) and Linear(128, C)")
        if not small_supported(self.F, self.C):
            raise ValueError(f"small_predict='native' supports F % 4 == 0, F >= 4 and n_clusters in 1..256 (got F={self.F}, n_clusters={self.C})")
        self._a1 = None             # [rows of the largest block so far * 400], reused between calls

    def _weights(self):
        for t in self.params:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("small_predict='native' needs contiguous float32 parameters on the device")
        return [_p(t) for t in self.params]

    def _scratch(self, m, dev):
        if self._a1 is None or self._a1.numel() < SH1 * m or self._a1.device != dev:
            self._a1 = torch.empty(SH1 * m, dtype=torch.float32, device=dev)
        return self._a1

    def forward(self, x, want_z=False):
        """x [n, F] float32 on the device, any n -> (lat float32 [n, 64], prob float32 [n], unit int32 [n], z float32 [n, C] or None)."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.F):
            raise ValueError(f"small_predict='native' takes a float32 device matrix [n, {self.F}]")
        x = x.contiguous()
        n, dev = x.shape[0], x.device
        w = self._weights()
        lat = torch.empty((n, SLAT), dtype=torch.float32, device=dev)
        prob = torch.empty(n, dtype=torch.float32, device=dev)
        unit = torch.empty(n, dtype=torch.int32, device=dev)
        z = torch.empty((n, self.C), dtype=torch.float32, device=dev) if want_z else None
        blk = small_block_rows(self.F)
        for lo in range(0, n, blk):
            r = min(blk, n - lo)
            a1 = self._scratch(r, dev)
            _lib.check(_L.idl_small_predict_l1(_p(x[lo:]), w[0], r, self.F, _p(a1), _stream()))
            _lib.check(_L.idl_small_predict_mid(_p(a1), *w[1:], r, self.C, _p(lat[lo:]), _p(z[lo:]) if want_z else None, _p(prob[lo:]), _p(unit[lo:]),
                                                _stream()))
        return lat, prob, unit, z
