#!/usr/bin/env python3
"""Generate tests/golden/large_k.npz and augment_k8.npz (k = 8 and 9) from the REAL reference.

Like make_golden.py: the reference package is copied to a scratch directory at run time, its Cython module is compiled there and
the copy is imported; nothing of the reference is written into this repository, only data its functions return.  4^8 / 4^9-wide
rows are stored SPARSELY -- the non-zero (index, count) pairs, or the entries that differ from the row's background value -- and
the generator asserts that every entry it does not store has that background value.

Usage:  python tests/golden/make_golden_large_k.py <path to the reference checkout>     (or IDELUCS_REFERENCE=<path>)
"""
import os
import random
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(os.path.dirname(HERE), "data")
KS = (8, 9)
AUG_COLS_SEED, AUG_COLS = 8, 2048


def build_reference(ref, scratch):
    os.makedirs(os.path.join(scratch, "idelucs"))
    for fn in os.listdir(os.path.join(ref, "idelucs")):
        if fn.endswith(".py") or fn.endswith(".pyx"):
            shutil.copy(os.path.join(ref, "idelucs", fn), os.path.join(scratch, "idelucs", fn))
    with open(os.path.join(scratch, "setup_ref.py"), "w") as f:
        f.write("from setuptools import setup, Extension\n"
                "from Cython.Build import cythonize\n"
                "setup(ext_modules=cythonize([Extension('idelucs.kmers', ['idelucs/kmers.pyx'])]))\n")
    subprocess.run([sys.executable, "setup_ref.py", "build_ext", "--inplace"], cwd=scratch, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, scratch)


def read_records_like_reference(fname):
    """(id, cleaned bytearray) per record, using the reference's own check_sequence."""
    from idelucs.utils import check_sequence
    out, lines, seq_id = [], [], ""
    for line in open(fname, "rb"):
        if line.startswith(b"#"):
            continue
        if line.startswith(b">"):
            if seq_id != "":
                out.append((seq_id, check_sequence(seq_id, bytearray().join(lines))))
                lines = []
            seq_id = line[1:-1].decode()
        else:
            lines.append(line.strip())
    out.append((seq_id, check_sequence(seq_id, bytearray().join(lines))))
    return out


def write_records(path, recs):
    with open(path, "wb") as f:
        for i, s in recs:
            f.write(b">" + i.encode() + b"\n" + bytes(s) + b"\n")


class Sparse:
    """CSR over the records of a file: the entries of every row that differ from the row's background value."""

    def __init__(self):
        self.idx, self.val, self.off, self.bg = [], [], [0], []

    def add(self, row, bg):
        at = np.flatnonzero(row != bg)
        self.idx.append(at.astype(np.int32)); self.val.append(row[at]); self.off.append(self.off[-1] + at.size); self.bg.append(bg)

    def put(self, out, key, dtype):
        out[key + "_idx"] = np.concatenate(self.idx) if self.idx else np.empty(0, np.int32)
        out[key + "_val"] = (np.concatenate(self.val) if self.val else np.empty(0)).astype(dtype)
        out[key + "_off"] = np.array(self.off, np.int64)
        out[key + "_bg"] = np.array(self.bg, dtype)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IDELUCS_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "idelucs")):
        sys.exit(__doc__)
    scratch = tempfile.mkdtemp(prefix="idelucs_ref_build_")
    try:
        build_reference(ref, scratch)
        from idelucs.kmers import kmer_counts, cgr
        from idelucs import utils as U

        inf8 = os.path.join(scratch, "influenza_8.fas")
        write_records(inf8, read_records_like_reference(os.path.join(DATA, "influenza_64.fas"))[:8])
        out = {}
        for name, fn in (("edge", os.path.join(DATA, "edge.fas")), ("influenza_8", inf8)):
            recs = read_records_like_reference(fn)
            out[f"{name}_names"] = np.array([r[0] for r in recs])
            for k in KS:
                F = 4 ** k
                km, km1, cg, canon, freq, canon_sum = Sparse(), Sparse(), Sparse(), Sparse(), Sparse(), []
                names, f64 = U.kmersFasta(fn, k=k)
                assert list(names) == [r[0] for r in recs] and f64.shape == (len(recs), F)
                _, f64r = U.kmersFasta(fn, k=k, reduce=True)
                _, c64 = U.cgrFasta(fn, k=k)          # (cgrFasta skips check_sequence; ones-initialised like kmersFasta)
                cgfreq = Sparse()
                for i, (_, s) in enumerate(recs):
                    c0 = np.zeros(F, np.int32); kmer_counts(bytearray(s), k, c0)
                    c1 = np.ones(F, np.int32); kmer_counts(bytearray(s), k, c1)
                    g0 = np.zeros(F, np.int32); cgr(bytearray(s), k, g0)
                    km.add(c0, 0); km1.add(c1, 1); cg.add(g0, 0)
                    cr = np.asarray(U.kmer_rev_comp(c1.copy(), k)).astype(np.int32)
                    canon.add(cr, 1); canon_sum.append(int(cr.sum()))
                    assert np.array_equal(f64[i], c1 / np.sum(c1)) and np.array_equal(f64r[i], cr / np.sum(cr))
                    freq.add(f64[i], 1.0 / float(np.sum(c1)))
                    cgfreq.add(c64[i], float(c64[i].min()))
                key = f"{name}_k{k}"
                km.put(out, key + "_kmer", np.int32); km1.put(out, key + "_kmer1", np.int32); cg.put(out, key + "_cgr", np.int32)
                canon.put(out, key + "_canon", np.int32); freq.put(out, key + "_freq", np.float64)
                cgfreq.put(out, key + "_cgrfreq", np.float64)
                out[key + "_canon_sum"] = np.array(canon_sum, np.int64)
                out[key + "_canon_len"] = np.int64(f64r.shape[1])
        np.savez_compressed(os.path.join(HERE, "large_k.npz"), **out)

        # AugmentFasta(8 records, n_mimics = 3, k = 8) under the seeds a fresh import of the reference's models module leaves behind
        np.random.seed(0); random.seed(0)
        x = U.AugmentFasta(inf8, 3, k=8, reduce=False)
        n, two, f = x.shape
        cols = np.sort(np.random.default_rng(AUG_COLS_SEED).choice(np.arange(1, f - 1), AUG_COLS - 2, replace=False))
        cols = np.concatenate([[0], cols, [f - 1]]).astype(np.int64)
        np.savez_compressed(os.path.join(HERE, "augment_k8.npz"), shape=np.array(x.shape, np.int64), cols=cols, values=x[:, :, cols],
                            row_sums=x.astype(np.float64).sum(2))
        print("done; fixtures in", HERE)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
