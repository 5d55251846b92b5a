"""Register / scratch / LDS budget of the sums + forward-middle kernel and of the sums + tail kernel (CPU: hipcc cross-compiles)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_sums_fwd_instances_fit_a_1024_thread_workgroup(tmp_path):
    """csrc/train_step.hip: sums_fwd_kernel runs 1024-thread workgroups -- at most 128 VGPRs -- and issues every load before the first dependent
    instruction: a spilled register would be reloaded from scratch.  No scratch, at most 128 VGPRs, at most 4 KB of static LDS (its partial-tile image is
    dynamic LDS); the 256-thread reduce_rms_kernel keeps its budget too."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "idelucs_amd", "csrc", "train_step.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "train_step.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        m = re.search(r"\d+(sums_fwd_kernel|reduce_rms_kernel)E", name)
        if m:
            seen[m.group(1)] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)),
                                int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    assert set(seen) == {"sums_fwd_kernel", "reduce_rms_kernel"}, seen
    for kernel, (scratch, vgprs, lds) in seen.items():
        assert scratch == 0 and lds <= 4096 and vgprs <= (128 if kernel == "sums_fwd_kernel" else 256), (kernel, scratch, vgprs, lds)
