"""The CPU oracle at k = 8 and 9 against fixtures generated from the real reference (tests/golden/make_golden_large_k.py), the way
test_oracle_golden.py pins k = 1..7: every stored row is reproduced exactly.  The 4^k-wide rows are stored sparsely (entries that
differ from the row's background value); large_k_rows() expands them and is shared with the GPU tests."""
import os
import random

import numpy as np
import pytest

from conftest import DATA, GOLDEN
from oracle import oracle as O

KS = (8, 9)
FILES = ("edge", "influenza_8")


def large_k_rows(g, name, k, what, width=None):
    """Dense [records, width] array of fixture `what` (kmer, kmer1, cgr, canon, freq, cgrfreq) of file `name` at k."""
    key = f"{name}_k{k}_{what}"
    idx, val, off, bg = g[key + "_idx"], g[key + "_val"], g[key + "_off"], g[key + "_bg"]
    width = width or 4 ** k
    rows = np.empty((bg.size, width), val.dtype)
    for i in range(bg.size):
        rows[i] = bg[i]
        rows[i, idx[off[i]:off[i + 1]]] = val[off[i]:off[i + 1]]
    return rows


def influenza_8(tmp_dir):
    recs = list(O.fasta_records(os.path.join(DATA, "influenza_64.fas")))[:8]
    p = os.path.join(str(tmp_dir), "influenza_8.fas")
    with open(p, "wb") as f:
        for i, s in recs:
            f.write(b">" + i.encode() + b"\n" + bytes(s) + b"\n")
    return p


def fixture_file(name, tmp_dir):
    return os.path.join(DATA, "edge.fas") if name == "edge" else influenza_8(tmp_dir)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "large_k.npz"))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", FILES)
def test_oracle_reproduces_the_reference_rows(golden, tmp_path, name, k):
    g, fn = golden, fixture_file(name, tmp_path)
    recs = list(O.fasta_records(fn))
    assert [r[0] for r in recs] == g[f"{name}_names"].tolist()
    F = 4 ** k
    km, km1, cg = large_k_rows(g, name, k, "kmer"), large_k_rows(g, name, k, "kmer1"), large_k_rows(g, name, k, "cgr")
    n_canon = int(g[f"{name}_k{k}_canon_len"])
    assert n_canon == O.n_canonical(k) == ((F + 2 ** k) // 2 if k % 2 == 0 else F // 2)
    canon = large_k_rows(g, name, k, "canon", n_canon)
    for i, (_, s) in enumerate(recs):
        c = np.zeros(F, np.int32); O.kmer_counts(s, k, c)
        assert np.array_equal(c, km[i]), (name, k, i)
        c1 = np.ones(F, np.int32); O.kmer_counts(s, k, c1)
        assert np.array_equal(c1, km1[i]), (name, k, i)
        c = np.zeros(F, np.int32); O.cgr(s, k, c)
        assert np.array_equal(c, cg[i]), (name, k, i)
        cr = O.kmer_rev_comp(c1.copy(), k)
        assert np.array_equal(cr, canon[i]) and int(cr.sum()) == int(g[f"{name}_k{k}_canon_sum"][i]), (name, k, i)
    names, f = O.kmersFasta(fn, k)
    assert names == [r[0] for r in recs] and np.array_equal(f, large_k_rows(g, name, k, "freq"))
    _, fr = O.kmersFasta(fn, k, None, True)
    assert np.array_equal(fr, canon / canon.sum(1, keepdims=True))
    _, cf = O.cgrFasta(fn, k)
    assert np.array_equal(cf, large_k_rows(g, name, k, "cgrfreq"))


def test_oracle_augment_fasta_k8(tmp_path):
    g = np.load(os.path.join(GOLDEN, "augment_k8.npz"))
    np.random.seed(0); random.seed(0)
    x = O.AugmentFasta(influenza_8(tmp_path), 3, k=8)
    assert x.dtype == np.float32 and list(x.shape) == g["shape"].tolist() == [24, 2, 4 ** 8]
    assert np.array_equal(x[:, :, g["cols"]], g["values"])
    assert np.array_equal(x.astype(np.float64).sum(2), g["row_sums"])
