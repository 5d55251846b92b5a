"""CPU tests of the k = 8 / 9 vectoriser (csrc/vectorise_slices.h): its kernels compile for gfx950 without scratch, within their
launch bounds and within a CU's LDS at the residency the launcher assumes (hipcc cross-compiles); the k range of the ABI and of
the CLI."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

THREADS = 512           # __launch_bounds__ of vectorise_slices_kernel
CU_LDS = 160 * 1024     # bytes of LDS of a gfx950 CU


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_slice_kernels_have_no_scratch_and_fit_their_launch_bounds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "idelucs_amd", "csrc", "vectorise.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "vectorise.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        mt = re.search(r"vectorise_slices_kernelILi(\d+)E", name)
        if mt:
            agpr = re.search(r" AGPRs: (\d+)", b)
            seen[int(mt.group(1))] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)),
                                      int(agpr.group(1)) if agpr else 0, int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    assert set(seen) == {8, 9}, seen
    for k, (scratch, vgprs, agprs, static_lds) in seen.items():
        waves_per_simd = -(-THREADS // 256)             # a workgroup's waves spread over the CU's four SIMDs
        assert scratch == 0, (k, scratch)
        assert vgprs + agprs <= 512 // waves_per_simd, (k, vgprs, agprs)
        assert static_lds == 0, (k, static_lds)         # all of it is dynamic: idl_vectorise_slices_lds() below


def test_slice_kernel_lds_fits_a_cu_at_the_launchers_residency():
    from idelucs_amd import _lib
    lds, per_cu = _lib.lib.idl_vectorise_slices_lds(), _lib.lib.idl_vectorise_slices_per_cu()
    assert lds >= 4 * (1 << 14) and per_cu >= 1         # a slice of 2^14 uint32 bins and the staged chunk
    assert lds * per_cu <= CU_LDS, (lds, per_cu)
    assert per_cu * (THREADS // 64) <= 32               # wave slots of a CU


def test_k_range_of_the_abi_and_the_header():
    from idelucs_amd import _lib
    assert _lib.MAX_K == 9
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    assert re.search(r"#define\s+IDL_MAX_K\s+9\b", hdr)
    for k in (8, 9):
        assert _lib.lib.idl_row_len(_lib.MODE_KMER, k) == 4 ** k and _lib.lib.idl_row_len(_lib.MODE_CGR, k) == 4 ** k
    assert _lib.lib.idl_row_len(_lib.MODE_CANONICAL, 8) == (4 ** 8 + 2 ** 8) // 2          # even k: palindromes
    assert _lib.lib.idl_row_len(_lib.MODE_CANONICAL, 9) == 4 ** 9 // 2                      # odd k: none


def test_kmers_error_names_the_new_bound():
    import numpy as np
    from idelucs_amd import kmers
    with pytest.raises(ValueError, match=r"k=10 is outside 1\.\.9"):
        kmers.kmer_counts(bytearray(b"ACGT"), 10, np.zeros(4, np.int32))
    with pytest.raises(ValueError, match=r"counts has 4 entries; k=8 needs 65536"):         # k = 8 passes the range check
        kmers.kmer_counts(bytearray(b"ACGT"), 8, np.zeros(4, np.int32))


def test_predict_counts_route_stays_at_k7():
    from idelucs_amd import utils as U
    assert U.counts_route_ok(7, False) and not U.counts_route_ok(8, False) and not U.counts_route_ok(9, False)


def test_parser_accepts_k8(capsys, monkeypatch):
    from idelucs_amd import __main__ as M
    p = M.build_parser()
    assert vars(p.parse_args(["--k", "8"]))["k"] == 8 and vars(p.parse_args(["--k", "9"]))["k"] == 9
    got = []
    monkeypatch.setattr(M, "run", lambda args: got.append(dict(args)))
    M.main(["--sequence_file", "x.fas", "--k", "8"])
    assert got[0]["k"] == 8
    capsys.readouterr()
