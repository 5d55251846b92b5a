"""numpy float64 replay of the scaler's one-pass statistics (csrc/scaler.hip): per-column sums of t = x - x0 and t^2, x0 = row 0, taken in
ascending row order inside the fixed row blocks of the WHOLE matrix, then the finishing combine.  Two forms of the sums: over the whole
matrix (col_shifted_sums_kernel / counts_stats_kernel) and over chunks of rows cut anywhere (counts_slab_stats_kernel: a chunk that begins
inside a row block continues from the partial stored for it)."""
import numpy as np

EPS = 2.220446049250313e-16


def stat_row_blocks(n):
    return min(max((n + 255) // 256, 1), 256)


def rows_per_block(n):
    b = stat_row_blocks(n)
    return (n + b - 1) // b


def shifted_sums_whole(x):
    """-> (x0 [f], partial1 [blocks, f], partial2 [blocks, f]): every row block from its first row to its last"""
    x = np.asarray(x, np.float64)
    n, f = x.shape
    blocks, rpb = stat_row_blocks(n), rows_per_block(n)
    p1, p2 = np.zeros((blocks, f)), np.zeros((blocks, f))
    x0 = x[0].copy()
    for b in range(blocks):
        a1, a2 = np.zeros(f), np.zeros(f)
        for r in range(b * rpb, min((b + 1) * rpb, n)):
            t = x[r] - x0
            a1 = a1 + t
            a2 = a2 + t * t
        p1[b], p2[b] = a1, a2
    return x0, p1, p2


class ChunkedSums:
    """The same sums from chunks of rows given in ascending order without gaps (the workspace of idl_counts_stream_stats)."""

    def __init__(self, n, f):
        self.n, self.f = n, f
        self.blocks, self.rpb = stat_row_blocks(n), rows_per_block(n)
        self.p1 = np.full((self.blocks, f), np.nan)          # (never read before written: a block's first row zeroes)
        self.p2 = np.full((self.blocks, f), np.nan)
        self.x0 = None
        self.next_row = 0

    def add(self, rows):
        rows = np.asarray(rows, np.float64)
        lo, hi = self.next_row, self.next_row + rows.shape[0]
        assert hi <= self.n
        if hi == lo:
            return self
        if lo == 0:
            self.x0 = rows[0].copy()
        for b in range(lo // self.rpb, (hi - 1) // self.rpb + 1):
            b0 = b * self.rpb
            r0, r1 = max(b0, lo), min(b0 + self.rpb, hi)
            a1 = np.zeros(self.f) if r0 == b0 else self.p1[b].copy()
            a2 = np.zeros(self.f) if r0 == b0 else self.p2[b].copy()
            for r in range(r0, r1):
                t = rows[r - lo] - self.x0
                a1 = a1 + t
                a2 = a2 + t * t
            self.p1[b], self.p2[b] = a1, a2
        self.next_row = hi
        return self

    def result(self):
        assert self.next_row == self.n
        return self.x0, self.p1, self.p2


def finish(x0, p1, p2, n):
    """col_finish_kernel: 16 groups of row blocks (block b in group b % 16) added in block order, the groups added in group order
    -> (mean, scale) as sklearn's StandardScaler defines them (population variance; scale below 10 eps -> 1)"""
    blocks, f = p1.shape
    t1, t2 = np.zeros(f), np.zeros(f)
    for g in range(16):
        a1, a2 = np.zeros(f), np.zeros(f)
        for b in range(g, blocks, 16):
            a1 = a1 + p1[b]
            a2 = a2 + p2[b]
        t1 = t1 + a1
        t2 = t2 + a2
    dn = float(n)
    mean = x0 + t1 / dn
    var = np.maximum((t2 - t1 * t1 / dn) / dn, 0.0)
    s = np.sqrt(var)
    s[s < 10.0 * EPS] = 1.0
    return mean, s


def stats_whole(x):
    x0, p1, p2 = shifted_sums_whole(x)
    return finish(x0, p1, p2, np.asarray(x).shape[0])


def stats_chunked(x, chunk):
    x = np.asarray(x, np.float64)
    n, f = x.shape
    acc = ChunkedSums(n, f)
    for lo in range(0, n, chunk):
        acc.add(x[lo:lo + chunk])
    x0, p1, p2 = acc.result()
    return finish(x0, p1, p2, n)
