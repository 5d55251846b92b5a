"""CPU tests of the batched kernels behind lockstep training at 48 < n_clusters <= 200: they exist in a gfx950 cross-compile (hipcc needs no GPU), cost
no more scratch than the lone voter's kernels whose bodies they call, fit their launch bounds, and leave the n_clusters <= 48 middle backward's batched
kernel what it was."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

# batched kernel -> (its unbatched counterpart in the same compile, its __launch_bounds__)
NEW = {
    "train_step.hip": {"iic_core_rows_batched_kernel": ("iic_core_rows_kernel", 1024),
                       "iic_dz_batched_kernel": ("iic_dz_kernel", 256),
                       "mid_bwd_big_batched_kernel": ("mid_bwd_kernelILb1ELb1EE", 1024)},       # mid_bwd_kernel<true, true>: n_clusters > 48, dr1 as planes
    "nce_fused.hip": {"at_b_batched_kernel": ("at_b_kernel", 256),
                      "nce_pass1_batched_kernel": ("nce_pass1_kernel", 256),                 # (not new: the joint's rider branch is now reached through them)
                      "nce_pass2_batched_kernel": ("nce_pass2_kernel", 256)},
}
# mid_bwd_batched_kernel (n_clusters <= 48) as the same compile of the commit before mid_bwd_big_batched_kernel existed gives it: the big form is a kernel
# of its own so that this one inherits nothing of it
MID_BWD_BATCHED_BEFORE = dict(vgprs=128, agprs=0, scratch=0, lds=125448)


def _resources(tmp_path, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "idelucs_amd", "csrc", name)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / (name + ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        agpr = re.search(r" AGPRs: (\d+)", b)
        seen[b.split()[0]] = dict(scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), vgprs=int(re.search(r" VGPRs: (\d+)", b).group(1)),
                                  agprs=int(agpr.group(1)) if agpr else 0, lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    return seen


def _one(seen, key):
    hits = [v for name, v in seen.items() if key in name]
    assert len(hits) == 1, (key, sorted(seen))
    return hits[0]


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("name", sorted(NEW))
def test_batched_kernels_of_the_rows_step_cost_what_the_lone_kernels_cost(tmp_path, name):
    seen = _resources(tmp_path, name)
    for k, (lone, bounds) in NEW[name].items():
        got, ref = _one(seen, k), _one(seen, lone)
        waves_per_simd = -(-bounds // 256)              # a workgroup's waves spread over the CU's four SIMDs
        assert got["scratch"] <= ref["scratch"], (k, got, ref)
        assert got["vgprs"] + got["agprs"] <= 512 // waves_per_simd, (k, got)
        assert got["lds"] <= 65536, (k, got)
    if name == "train_step.hip":
        assert _one(seen, "mid_bwd_batched_kernel") == MID_BWD_BATCHED_BEFORE
