"""CPU tests of the native SGD / Adam step of NetLinear: csrc/opt_step.hip compiles for gfx950 without scratch and within its launch
bounds (hipcc cross-compiles), and the CLI's --linear_step flag leaves no trace when it is not given."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

KERNELS = {"opt_step_kernelILi1E": 256, "opt_step_kernelILi2E": 256}           # kernel<kind> -> its __launch_bounds__
# the waves a SIMD holds of each (the streaming blocks hide HBM latency with them): SGD 4 (<= 128 registers), Adam, with a fourth
# stream in flight, 3 (<= 168)
WAVES = {"opt_step_kernelILi1E": 4, "opt_step_kernelILi2E": 3}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_opt_step_kernels_have_no_scratch_and_fit_their_launch_bounds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "idelucs_amd", "csrc", "opt_step.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "opt_step.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        for k in KERNELS:
            if k in name:
                agpr = re.search(r" AGPRs: (\d+)", b)
                seen[k] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)),
                           int(agpr.group(1)) if agpr else 0, int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    assert set(seen) == set(KERNELS), (seen, [b.split()[0] for b in blocks])
    for k, (scratch, vgprs, agprs, lds) in seen.items():
        waves_per_simd = -(-KERNELS[k] // 256)          # a workgroup's waves spread over the CU's four SIMDs
        assert scratch == 0, (k, scratch)
        assert vgprs + agprs <= 512 // waves_per_simd, (k, vgprs, agprs)
        assert vgprs + agprs <= 512 // WAVES[k] // 8 * 8, (k, vgprs, agprs, WAVES[k])
        assert lds <= 65536, (k, lds)


def test_opt_step_source_is_built_and_declared():
    mk = open(os.path.join(ROOT, "idelucs_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC_HIP :=.*\bopt_step\.hip\b", mk, re.M)
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    assert "idl_opt_step_gather_wgrad(" in hdr and "models.py:89-92" in hdr


def test_parser_linear_step_flag(capsys, monkeypatch):
    from idelucs_amd import __main__ as M
    p = M.build_parser()
    for v in ("native", "autograd"):
        assert vars(p.parse_args(["--linear_step", v]))["linear_step"] == v
    with pytest.raises(SystemExit):
        p.parse_args(["--linear_step", "fused"])
    capsys.readouterr()
    assert "linear_step" not in vars(p.parse_args([]))
    # without the flag, what main() prints and hands on (the results table's Parameters cell) has no linear_step entry
    got = []
    monkeypatch.setattr(M, "run", lambda args: got.append(dict(args)))
    M.main(["--sequence_file", "x.fas", "--optimizer", "Adam"])
    assert "linear_step" not in got[0] and "linear_step" not in capsys.readouterr().out
    M.main(["--sequence_file", "x.fas", "--optimizer", "Adam", "--linear_step", "native"])
    assert got[1]["linear_step"] == "native" and "linear_step \t -> native" in capsys.readouterr().out
    from idelucs import __main__ as M2                 # `python -m idelucs` shares the parser
    assert M2.main is M.main
