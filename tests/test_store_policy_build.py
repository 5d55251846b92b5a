"""csrc/store_policy.h in the ISA (CPU: hipcc cross-compiles): the helper's store is a 16-byte store with the write-through bit, the step's kernels carry
such stores at every site and no narrower write-through store, and the 1024-thread kernels that inline the batch assembly keep their register budget."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "idelucs_amd", "csrc")
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def _functions(asm):
    """name -> instruction lines of every function of an assembly listing"""
    out, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        ins = line.split(";")[0].strip()
        if cur is not None and ins and not ins.startswith("."):
            cur.append(ins)
    return out


def _wt_stores(lines):
    """(16-byte write-through stores, narrower write-through stores, plain 16-byte stores) of a function; every asm write-through store is followed by its s_nop 1"""
    wide = narrow = plain = 0
    for i, ins in enumerate(lines):
        op = ins.split()[0]
        if not re.match(r"(global|buffer|flat)_store_", op):
            continue
        if re.search(r"\bsc1\b", ins):
            if op.endswith("dwordx4"):
                wide += 1
                assert lines[i + 1].split() == ["s_nop", "1"], (ins, lines[i + 1])
            else:
                narrow += 1
        elif op.endswith("dwordx4"):
            plain += 1
    return wide, narrow, plain


@needs_hipcc
def test_the_helpers_store_is_a_16_byte_write_through_store(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "t.hip"
    src.write_text('#include "store_policy.h"\n'
                   '__global__ void always(float4 *p, float4 v) { idl_store::store16(p + threadIdx.x, v, true); }\n'
                   '__global__ void never(float4 *p, float4 v) { idl_store::store16(p + threadIdx.x, v, false); }\n'
                   '__global__ void either(float4 *p, float4 v, int wt) { idl_store::store16(p + threadIdx.x, v, (wt & idl_store::WT_PART) != 0); }\n'
                   '__global__ void paired(uint2 *hi, uint2 *lo, uint2 h, uint2 l) { const bool odd = threadIdx.x & 1;\n'
                   '    idl_store::store16_wt((odd ? lo : hi) + (threadIdx.x - odd), idl_store::pair_planes(h, l, odd)); }\n')
    out = tmp_path / "t.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-I", CSRC, "-S", str(src), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    fns = {re.search(r"\d+([a-z]+)", k).group(1): v for k, v in _functions(out.read_text()).items()}
    assert _wt_stores(fns["always"]) == (1, 0, 0)
    assert _wt_stores(fns["never"]) == (0, 0, 1)
    assert _wt_stores(fns["either"]) == (1, 0, 1)
    assert _wt_stores(fns["paired"]) == (1, 0, 0) and sum("quad_perm:[1,0,3,2]" in i for i in fns["paired"]) == 2


@needs_hipcc
def test_the_step_kernels_carry_the_stores_and_keep_their_budget(tmp_path):
    """train_step.hip: the riders' kernels (sums_fwd, mid_fwd, mid_bwd at n_clusters <= 48: 1024 threads, at most 128 VGPRs, no scratch -- the figures of test_build_resources.py and
    test_build_sums_fwd.py), the batched layer-1 kernel and the dW1 kernels (no scratch; that nothing of the compiler's reaches the K-steps' operand sets at v200 and above is
    test_build_resources.py's check) each hold 16-byte write-through stores behind their bit, and no write-through store is narrower than 16 bytes."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(CSRC, "train_step.hip")
    out = tmp_path / "train_step.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    res = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        res[b.split()[0]] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)))
    fns = _functions(out.read_text())
    # kernel -> (VGPR limit, the fewest 16-byte write-through stores it must hold)
    want = {"sums_fwd_kernel": (128, 2), "mid_fwd_kernelILb0E": (128, 2), "mid_fwd_kernelILb1E": (128, 2), "mid_bwd_kernelILb0ELb0E": (128, 2), "mid_bwd_kernelILb0ELb1E": (128, 2),
            "l1_planes_batched_kernel": (256, 2), "wgrad_dplanes_rms_kernel": (256, 3),
            "wgrad_xplanes_rms_batched_kernel": (256, 3)}
    seen = set()
    for name, lines in fns.items():
        wide, narrow, _ = _wt_stores(lines)
        assert narrow == 0, (name, narrow)
        for k, (limit, least) in want.items():
            if (k + "E") in name:
                scratch, vgprs = res[name]
                assert scratch == 0 and vgprs <= limit and wide >= least, (k, scratch, vgprs, wide)
                seen.add(k)
    assert seen == set(want), sorted(set(want) - seen)
