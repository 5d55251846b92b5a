"""GPU tests of the vectoriser at k = 8 and 9 (the bin-slice kernel, csrc/vectorise_slices.h): every mode, init and out kind,
bit for bit against the CPU oracle, on the inputs that reach the kernel's edges -- first / last bin and slice, a count above
65 535, windows on both sides of a slice boundary, N at every offset around one position, records of k - 1, k and k + 1 bases,
a 3 Mbp record (more than one staged chunk), and four views with edits in both edit_off layouts."""
import os
import random

import numpy as np
import pytest

from conftest import DATA
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KS = (8, 9)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import idelucs_amd
    from idelucs_amd import _lib
    _lib.require_gpu()
    assert torch.cuda.is_available()
    return idelucs_amd


def _pack_batch(seqs):
    import ctypes
    from idelucs_amd import _lib
    n = len(seqs)
    byte_off = np.zeros(n + 1, np.int64); np.cumsum([len(s) for s in seqs], out=byte_off[1:])
    data = np.concatenate(seqs) if n else np.empty(0, np.uint8)
    slots = int(sum((len(s) + 63) // 64 for s in seqs))
    codes = np.zeros(max(slots, 1) * 16, np.uint8); mask = np.zeros(max(slots, 1) * 8, np.uint8)
    slot_off = np.zeros(n + 1, np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(_lib.lib.idl_pack(p(data), p(byte_off), n, p(codes), p(mask), p(slot_off)))
    class FF: pass
    ff = FF(); ff.n = n; ff.codes = codes; ff.mask = mask; ff.slot_off = slot_off
    ff.lengths = np.array([len(s) for s in seqs], np.int64)
    return ff


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


def _edge_batch(k):
    """The sequences of the issue's list, as uint8 arrays (cleaned bytes: A, C, G, T, N)."""
    rng = np.random.default_rng(100 + k)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = [_u8(s) for _, s in O.fasta_records(os.path.join(DATA, "edge.fas"))]
    seqs += [_u8(s) for _, s in list(O.fasta_records(os.path.join(DATA, "influenza_64.fas")))[:8]]
    seqs += [_u8(b"A" * 70000), _u8(b"T" * 70000)]              # first / last bin, first / last slice, a count above 65 535
    # windows on both sides of every slice boundary (a slice is 2^14 bins = the last 7 bases): ...TTTTTTT is the last bin of a
    # slice, the next prefix followed by AAAAAAA the first bin of the next one
    pre = k - 7
    pieces = []
    for p in range(4 ** pre - 1):
        a = "".join("ACGT"[(p >> (2 * (pre - 1 - t))) & 3] for t in range(pre))
        b = "".join("ACGT"[((p + 1) >> (2 * (pre - 1 - t))) & 3] for t in range(pre))
        pieces.append((a + "TTTTTTT" + b + "AAAAAAA") * 3)
    seqs.append(_u8("".join(pieces).encode()))
    base = rng.choice(acgt, size=200)
    for o in range(k + 1):                                       # N at every offset 0..k around one position
        s = base.copy(); s[100 + o] = ord("N"); s[100] = ord("N")
        seqs.append(s)
    seqs += [rng.choice(acgt, size=L) for L in (k - 1, k, k + 1)]
    seqs.append(np.empty(0, np.uint8))                           # an empty record
    seqs.append(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=30000, p=[.24, .24, .24, .24, .04]))   # two staged chunks, N runs
    return seqs


@pytest.mark.parametrize("k", KS)
def test_every_mode_init_and_out_kind_vs_oracle(gpu, k):
    import torch
    from idelucs_amd import _lib, utils as U
    seqs = _edge_batch(k)
    n, F = len(seqs), 4 ** k
    dev = torch.device("cuda")
    din = U._DeviceInput(_pack_batch(seqs), dev)
    km0 = np.zeros((n, F), np.int32); cg0 = np.zeros((n, F), np.int32)
    for i, s in enumerate(seqs):
        O.kmer_counts(s, k, km0[i]); O.cgr(s, k, cg0[i])
    assert km0.max() > 65535 and km0[:, 0].max() > 65535 and km0[:, F - 1].max() > 65535
    for mode, init, kind in ((_lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_FREQ_F32), (_lib.MODE_CGR, _lib.INIT_FROM_OUT, _lib.OUT_COUNTS_I32),
                             (_lib.MODE_CANONICAL, _lib.INIT_ZERO, _lib.OUT_FREQ_F64)):
        plan = U._vectorise_plan(din, k, mode, init, kind)          # the kernel under test is the one that runs
        assert plan.kernel == _lib.VEC_SLICES and plan.redo == 0 and plan.lds_bytes == _lib.lib.idl_vectorise_slices_lds(), (k, mode, plan.kernel)
    with np.errstate(invalid="ignore", divide="ignore"):
        for mode, base in ((_lib.MODE_KMER, km0), (_lib.MODE_CGR, cg0)):
            for init, iv in ((_lib.INIT_ZERO, 0), (_lib.INIT_ONE, 1)):
                want = base + iv
                got = U._vectorise(din, k, mode, init, _lib.OUT_COUNTS_I32)[0].cpu().numpy()
                assert np.array_equal(got, want), (k, mode, init, "i32")
                f64 = want / want.sum(1, keepdims=True).astype(np.float64)
                got = U._vectorise(din, k, mode, init, _lib.OUT_FREQ_F64)[0].cpu().numpy()
                assert np.array_equal(got, f64, equal_nan=True), (k, mode, init, "f64")
                got = U._vectorise(din, k, mode, init, _lib.OUT_FREQ_F32)[0].cpu().numpy()
                assert np.array_equal(got, f64.astype(np.float32), equal_nan=True), (k, mode, init, "f32")
            # accumulate on top of the caller's rows
            start = np.random.default_rng(k).integers(0, 1000, (1, n, F)).astype(np.int32)
            out = torch.from_numpy(start.copy()).to(dev)
            U._vectorise(din, k, mode, _lib.INIT_FROM_OUT, _lib.OUT_COUNTS_I32, out=out)
            assert np.array_equal(out[0].cpu().numpy(), start[0] + base), (k, mode, "from_out")
        for init, iv in ((_lib.INIT_ZERO, 0), (_lib.INIT_ONE, 1)):
            want = np.stack([O.kmer_rev_comp((km0[i] + iv).astype(np.int32), k) for i in range(n)])
            assert want.shape[1] == O.n_canonical(k)
            got = U._vectorise(din, k, _lib.MODE_CANONICAL, init, _lib.OUT_COUNTS_I32)[0].cpu().numpy()
            assert np.array_equal(got, want), (k, "canon", init, "i32")
            f64 = want / want.sum(1, keepdims=True).astype(np.float64)
            got = U._vectorise(din, k, _lib.MODE_CANONICAL, init, _lib.OUT_FREQ_F64)[0].cpu().numpy()
            assert np.array_equal(got, f64, equal_nan=True), (k, "canon", init, "f64")
            got = U._vectorise(din, k, _lib.MODE_CANONICAL, init, _lib.OUT_FREQ_F32)[0].cpu().numpy()
            assert np.array_equal(got, f64.astype(np.float32), equal_nan=True), (k, "canon", init, "f32")


@pytest.mark.parametrize("k", KS)
def test_three_mbp_record_with_edits(gpu, k):
    """One 3 Mbp record: staging takes 147 chunks per slice; view 1 carries edits spread over all of them."""
    import torch
    from idelucs_amd import _lib, utils as U
    rng = np.random.default_rng(5 + k)
    s = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=3_000_000, p=[.2499, .2499, .2499, .2499, .0004])
    pos = np.sort(rng.integers(0, s.size, 20000)).astype(np.uint32)
    e = pos | (rng.integers(0, 4, pos.size).astype(np.uint32) << np.uint32(30))
    mut = O.apply_edits(s.tobytes(), e)
    dev = torch.device("cuda")
    din = U._DeviceInput(_pack_batch([s]), dev)
    d_e = torch.from_numpy(e.view(np.int32)).to(dev)
    d_eo = torch.tensor([0, 0, e.size], dtype=torch.int64, device=dev)
    F = 4 ** k
    want = np.zeros((2, F), np.int32)
    O.kmer_counts(s, k, want[0]); O.kmer_counts(mut, k, want[1])
    assert U._vectorise_plan(din, k, _lib.MODE_KMER, _lib.INIT_ZERO, _lib.OUT_COUNTS_I32, 2, d_e).kernel == _lib.VEC_SLICES
    got = U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ZERO, _lib.OUT_COUNTS_I32, 2, d_e, d_eo).cpu().numpy()
    assert np.array_equal(got[:, 0], want)
    cg = np.zeros(F, np.int32); O.cgr(mut, k, cg)
    got = U._vectorise(din, k, _lib.MODE_CGR, _lib.INIT_ZERO, _lib.OUT_COUNTS_I32, 2, d_e, d_eo).cpu().numpy()
    assert np.array_equal(got[1, 0], cg)
    c = O.kmer_rev_comp((want[1] + 1).astype(np.int32), k)
    got = U._vectorise(din, k, _lib.MODE_CANONICAL, _lib.INIT_ONE, _lib.OUT_FREQ_F32, 2, d_e, d_eo).cpu().numpy()
    assert np.array_equal(got[1, 0], (c / np.sum(c)).astype(np.float32))


def _check_views(U, _lib, din, seqs, k, P, d_e, d_eo, e_host, ranges):
    """Decode every (view, sequence)'s edits, apply them to the bytes, count with the oracle."""
    n = len(seqs)
    got = U._vectorise(din, k, _lib.MODE_KMER, _lib.INIT_ONE, _lib.OUT_COUNTS_I32, P, d_e, d_eo).cpu().numpy()
    can = U._vectorise(din, k, _lib.MODE_CANONICAL, _lib.INIT_ONE, _lib.OUT_FREQ_F64, P, d_e, d_eo).cpu().numpy()
    n_edits = 0
    for v in range(P):
        for i in range(n):
            b, e = ranges[v * n + i]
            n_edits += e - b
            mut = O.apply_edits(seqs[i].tobytes(), e_host[b:e])
            want = np.ones(4 ** k, np.int32); O.kmer_counts(mut, k, want)
            assert np.array_equal(got[v, i], want), (k, v, i)
            c = O.kmer_rev_comp(want, k)
            assert np.array_equal(can[v, i], c / np.sum(c)), (k, v, i)
    return n_edits


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("slots", [True, False])
def test_four_views_with_device_drawn_edits(gpu, k, slots):
    """Philox sites in both edit_off layouts: slots=True gives [n_views * n, 2] ranges, slots=False the CSR array."""
    import torch
    from idelucs_amd import _lib, utils as U
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGTN", np.uint8)
    seqs = [rng.choice(acgt, size=L, p=[.2475, .2475, .2475, .2475, .01]) for L in (2000, 2311, 9000, 25000, 64, 300)]
    n, P = len(seqs), 4
    dev = torch.device("cuda")
    din = U._DeviceInput(_pack_batch(seqs), dev)
    edits, edit_off = U._philox_edits(din, [t.spec() for t in U.mimic_transforms(P - 1)], 3, slots=slots)
    assert edit_off.dim() == (2 if slots else 1)
    e_host = edits.cpu().numpy().view(np.uint32)
    eo = edit_off.cpu().numpy()
    ranges = eo if slots else np.stack([eo[:-1], eo[1:]], 1)
    assert _check_views(U, _lib, din, seqs, k, P, edits, edit_off, e_host, ranges) > 100


@pytest.mark.parametrize("k", KS)
def test_four_views_with_host_drawn_edits(gpu, k, tmp_path):
    """The reference's transforms drawn on the host (rng='compat'), as CSR and as (begin, end) ranges."""
    import torch
    from idelucs_amd import _lib, utils as U
    recs = list(O.fasta_records(os.path.join(DATA, "influenza_64.fas")))[:6]
    p = tmp_path / "six.fas"
    with open(p, "wb") as f:
        for i, s in recs:
            f.write(b">" + i.encode() + b"\n" + bytes(s) + b"\n")
    ff = U.FastaFile(str(p), keep_bytes=True)
    np.random.seed(0); random.seed(0)
    P = 4
    e, eo = U._compat_edits(ff, [None] + list(U.mimic_transforms(P - 1)))
    seqs = [np.array(ff.bytes[ff.byte_off[i]:ff.byte_off[i + 1]]) for i in range(ff.n)]
    dev = torch.device("cuda")
    din = U._DeviceInput(ff, dev)
    d_e = torch.from_numpy(e.view(np.int32)).to(dev)
    ranges = np.ascontiguousarray(np.stack([eo[:-1], eo[1:]], 1))
    for d_eo in (torch.from_numpy(eo).to(dev), torch.from_numpy(ranges).to(dev)):
        assert _check_views(U, _lib, din, seqs, k, P, d_e, d_eo, e, ranges) > 100


def test_scalar_entry_points_accumulate_on_top(gpu):
    rng = np.random.default_rng(23)
    alphabet = np.frombuffer(b"ACGTNacgtX-", np.uint8)
    for k in KS:
        for L in (0, 5, k, 1000, 21000):
            s = rng.choice(alphabet, size=L, p=[.23, .23, .23, .23, .03, .01, .01, .01, .01, .005, .005])
            init = rng.integers(0, 5, 4 ** k).astype(np.int32)
            want = init.copy(); O.kmer_counts(s, k, want)
            got = init.copy(); gpu.kmer_counts(s.copy(), k, got)
            assert np.array_equal(got, want), (L, k)
            want = init.copy(); O.cgr(s, k, want)
            got = init.copy(); gpu.cgr(s.copy(), k, got)
            assert np.array_equal(got, want), (L, k)


def test_kmer_rev_comp_at_k8_and_k9(gpu):
    rng = np.random.default_rng(3)
    for k in KS:
        c = rng.integers(0, 1000, 4 ** k).astype(np.int32)
        c2 = c.copy(); want = O.kmer_rev_comp(c2, k)
        c3 = c.copy(); got = gpu.kmer_rev_comp(c3, k)
        assert got.shape == (O.n_canonical(k),)
        assert np.array_equal(got, want) and np.array_equal(c2, c3), k   # in-place side effect identical too
        assert not np.array_equal(c3, c)


@pytest.mark.parametrize("k", KS)
def test_fasta_entry_points_vs_oracle(gpu, k):
    fn = os.path.join(DATA, "edge.fas")
    names, f = gpu.kmersFasta(fn, k=k)
    wn, wf = O.kmersFasta(fn, k)
    assert list(names) == list(wn) and f.dtype == np.float64 and np.array_equal(f, wf)
    _, fr = gpu.kmersFasta(fn, k=k, reduce=True)
    assert np.array_equal(fr, O.kmersFasta(fn, k, None, True)[1])
    _, cf = gpu.cgrFasta(fn, k=k)
    assert np.array_equal(cf, O.cgrFasta(fn, k)[1])
    with pytest.raises(ValueError, match="no projection kernel"):
        gpu.kmersFasta(fn, k=k, project=True)                    # no kernel file for this k


def test_k10_is_refused_with_the_new_bound(gpu):
    import torch
    from idelucs_amd import _lib, utils as U
    with pytest.raises(ValueError, match=r"1\.\.9"):
        gpu.kmer_counts(bytearray(b"ACGTACGTACGTACGT"), 10, np.zeros(4 ** 10, np.int32))
    with pytest.raises(ValueError, match=r"1\.\.9"):
        gpu.kmersFasta(os.path.join(DATA, "edge.fas"), k=10)
    din = U._DeviceInput(_pack_batch([_u8(b"ACGTACGTACGT")]), torch.device("cuda"))
    with pytest.raises(ValueError, match=r"1\.\.9"):
        U._vectorise(din, 10, _lib.MODE_KMER, _lib.INIT_ZERO, _lib.OUT_COUNTS_I32)
