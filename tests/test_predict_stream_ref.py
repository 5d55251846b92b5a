"""CPU tests of the streamed predict inputs (utils.predict_feature_chunks): the arithmetic its statistics kernels implement, replayed in
numpy float64 (tests/stats_ref.py) -- the sums do not depend on where the row chunks were cut, and they are StandardScaler's statistics --
and the build: the new entry points are exported, declared and bound."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stats_ref as R
from conftest import ROOT

NEW_SYMBOLS = ("idl_row_totals_i32", "idl_counts_stream_workspace", "idl_counts_stream_stats", "idl_counts_stream_finish")
F = 12          # columns: 0..8 frequencies, 9 constant, 10 all zero, 11 constant but for one row


def _rows(n, seed):
    """frequency-like float64 rows counts / sum(counts), with constant columns (variance exactly 0 -> scale 1)"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 4000, size=(n, F)).astype(np.float64)
    x = counts / counts.sum(1, keepdims=True)
    x[:, 9] = 0.25
    x[:, 10] = 0.0
    x[:, 11] = 1.0 / 3.0
    if n > 2:
        x[n // 2, 11] = 0.5
    return x


@pytest.mark.parametrize("n", [1, 5, 300, 600, 1000])
def test_chunked_sums_equal_the_whole_matrix_bit_for_bit(n):
    x = _rows(n, n)
    x0, p1, p2 = R.shifted_sums_whole(x)
    mean, scale = R.finish(x0, p1, p2, n)
    for chunk in (1, 7, 64, n, n + 5):
        acc = R.ChunkedSums(n, F)
        for lo in range(0, n, chunk):
            acc.add(x[lo:lo + chunk])
        c0, c1, c2 = acc.result()
        assert np.array_equal(c0, x0) and np.array_equal(c1, p1) and np.array_equal(c2, p2), (n, chunk)
        m2, s2 = R.finish(c0, c1, c2, n)
        assert np.array_equal(m2, mean) and np.array_equal(s2, scale), (n, chunk)
        m3, s3 = R.stats_chunked(x, chunk)
        assert np.array_equal(m3, mean) and np.array_equal(s3, scale)


def test_chunks_cut_at_uneven_rows():
    """cuts that fall before, on and after the row-block boundaries of n = 600 (blocks of 200 rows), chunk lengths all different"""
    n = 600
    x = _rows(n, 77)
    want = R.shifted_sums_whole(x)
    acc = R.ChunkedSums(n, F)
    for lo, hi in zip((0, 1, 199, 200, 201, 450), (1, 199, 200, 201, 450, 600)):
        acc.add(x[lo:hi])
    for g, w in zip(acc.result(), want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("n", [1, 5, 300, 600, 1000])
def test_replay_agrees_with_sklearn(n):
    from sklearn.preprocessing import StandardScaler
    x = _rows(n, 1000 + n)
    sk = StandardScaler().fit(x)
    mean, scale = R.stats_chunked(x, 64)
    assert np.allclose(mean, sk.mean_, rtol=1e-12, atol=0.0)
    assert np.allclose(scale, sk.scale_, rtol=1e-12, atol=0.0)
    assert scale[9] == 1.0 and scale[10] == 1.0 and sk.scale_[9] == 1.0 and sk.scale_[10] == 1.0      # zero variance
    if n > 2:
        assert scale[11] != 1.0
    y = (x - mean) / scale
    assert np.allclose(y, sk.transform(x), rtol=1e-9, atol=1e-12)


def test_every_row_block_has_rows():
    """the finish adds the partials of ALL stat_row_blocks(n) blocks: each must have been written, so none may be empty"""
    for n in list(range(1, 3000)) + [65279, 65280, 65281, 65535, 65536, 65537, 70000, 10 ** 6, 2 ** 31 - 1]:
        blocks, rpb = R.stat_row_blocks(n), R.rows_per_block(n)
        assert 1 <= blocks <= 256 and (blocks - 1) * rpb < n <= blocks * rpb, n


def test_new_entry_points_are_exported_declared_and_bound():
    from idelucs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(_lib.lib, name), name                     # exported by the built library
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, hdr), name
    assert _lib.lib.idl_counts_stream_workspace(600, 65536) == (2 * 3 + 1) * 65536 * 8
    assert _lib.lib.idl_counts_stream_workspace(1, 4) == 3 * 4 * 8


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_stream_kernels_compile_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "idelucs_amd", "csrc", "scaler.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "scaler.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        if "row_totals_kernel" in name or "counts_slab_stats_kernel" in name:
            seen[name] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)))
    assert len(seen) == 3, seen                                  # the totals kernel per row width, the slab kernel
    for name, (scratch, vgprs) in seen.items():
        assert scratch == 0 and vgprs <= 128, (name, scratch, vgprs)        # 256 threads: four waves a SIMD at least


def test_stream_route_shapes_and_chunk_size():
    from idelucs_amd import utils as U
    assert U.PREDICT_STREAM_CHUNK_BYTES == 8 << 30
    assert U.OPTIONS["predict_stream"] in ("", "0", "1")
    for k in range(1, 10):
        assert U.stream_route_ok(k, False)                       # 4^k
    assert U.stream_route_ok(8, True) and U.stream_route_ok(9, True) and U.stream_route_ok(6, True)
    assert not U.stream_route_ok(2, True) and not U.stream_route_ok(1, True)          # 10 and 2 columns
    assert U.predict_chunk_rows(4 ** 8) == 16384 and U.predict_chunk_rows(4 ** 9) == 4096
    assert U.predict_chunk_rows(4 ** 6) == 32768 and U.predict_chunk_rows(4 ** 9, 37) == 37
    assert U.predict_chunk_rows(4 ** 9 * 64) == 256
    assert U.counts_route_ok(7, False) and not U.counts_route_ok(8, False)             # the resident counts route is where it was
