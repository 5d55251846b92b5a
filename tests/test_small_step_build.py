"""CPU tests of the native step of model_size='small': its kernels compile for gfx950 without scratch and within their launch
bounds (hipcc cross-compiles), and the CLI's --small_step flag."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

KERNELS = {"small_l1_fwd_kernel": 512, "small_mid_fwd_kernel": 256, "small_mid_bwd_kernel": 256, "small_wgrad_rms_kernel": 512,
           "small_masks_kernel": 256}           # kernel -> its __launch_bounds__


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_small_step_kernels_have_no_scratch_and_fit_their_launch_bounds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "idelucs_amd", "csrc", "small_step.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "small_step.o"),
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
    assert set(seen) == set(KERNELS), seen
    for k, (scratch, vgprs, agprs, lds) in seen.items():
        waves_per_simd = -(-KERNELS[k] // 256)          # a workgroup's waves spread over the CU's four SIMDs
        assert scratch == 0, (k, scratch)
        assert vgprs + agprs <= 512 // waves_per_simd, (k, vgprs, agprs)
        assert lds <= 65536, (k, lds)


def test_parser_small_step_flag(capsys, monkeypatch):
    from idelucs_amd import __main__ as M
    p = M.build_parser()
    for v in ("native", "autograd"):
        assert vars(p.parse_args(["--small_step", v]))["small_step"] == v
    with pytest.raises(SystemExit):
        p.parse_args(["--small_step", "fused"])
    capsys.readouterr()
    defaults = vars(p.parse_args([]))
    assert defaults.pop("small_step") is None
    assert defaults == {"sequence_file": None, "n_clusters": 0, "n_epochs": 100, "n_mimics": 3, "batch_sz": 256, "GT_file": None, "k": 6,
                        "optimizer": "RMSprop", "scheduler": "None", "weight": 0.25, "lambda": 2.8, "lr": 1e-3, "n_voters": 5,
                        "model_size": "linear", "plot": False, "rng": None, "seed": 0}
    # without the flag, what main() prints and hands on (the results table's Parameters cell) has no small_step entry
    got = []
    monkeypatch.setattr(M, "run", lambda args: got.append(dict(args)))
    M.main(["--sequence_file", "x.fas"])
    assert "small_step" not in got[0] and "small_step" not in capsys.readouterr().out
    M.main(["--sequence_file", "x.fas", "--model_size", "small", "--small_step", "native"])
    assert got[1]["small_step"] == "native" and "small_step \t -> native" in capsys.readouterr().out
