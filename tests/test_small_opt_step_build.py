"""CPU tests of the native SGD / Adam step of model_size='small' (--small_opt_step native): small_wgrad_opt_kernel<1|2> compile for gfx950
without scratch and within their launch bounds (hipcc cross-compiles), no kernel's name collides with another wgrad kernel's, the entry
point is declared, the update's one definition is the header both step files include, the CLI flag leaves no trace when it is not given,
and the golden's own float32-against-float64 figures stay under the caps its generator kept the weight seed by."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

KERNELS = {"small_wgrad_opt_kernelILi1E": 512, "small_wgrad_opt_kernelILi2E": 512}           # kernel<kind> -> its __launch_bounds__
WGRAD_NAMES = ("small_wgrad_rms_kernel", "small_wgrad_momentum_kernel", "small_wgrad_opt_kernel")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "idelucs_amd", "csrc")


def _resource_blocks(fname, tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(CSRC, fname), "-o",
                        str(tmp_path / "out.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_small_wgrad_opt_kernels_have_no_scratch_and_fit_their_launch_bounds(tmp_path):
    blocks = _resource_blocks("small_step.hip", tmp_path)
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
        assert lds <= 65536, (k, lds)
    # (the build tests of the RMSprop forms match kernels by substring: no name may hold two of the three)
    for b in blocks:
        name = b.split()[0]
        assert sum(w in name for w in WGRAD_NAMES) <= 1, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_opt_step_still_builds_on_the_shared_update(tmp_path):
    names = [b.split()[0] for b in _resource_blocks("opt_step.hip", tmp_path)]
    for kind in (1, 2, 3):
        assert [n for n in names if f"opt_step_kernelILi{kind}E" in n], names
    for fname in ("opt_step.hip", "small_step.hip"):
        src = open(os.path.join(CSRC, fname)).read()
        assert '#include "opt_update_device.h"' in src, fname
        assert "struct Coef" not in src and "void opt_update(" not in src, fname        # one definition: the header's
    hdr = open(os.path.join(CSRC, "opt_update_device.h")).read()
    for what in ("struct Coef", "pow_int(", "make_coef(const double *hyper, const int64_t *step_in)", "void opt_update("):
        assert what in hdr, what
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HDR :=.*\bopt_update_device\.h\b", mk, re.M)


def test_small_wgrad_opt_is_declared():
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    assert "idl_small_wgrad_opt(" in hdr
    doc = hdr[:hdr.index("int idl_small_wgrad_opt(")].rsplit("/*", 1)[1]
    assert "models.py:89-92" in doc and "models.py:131-132" in doc
    from idelucs_amd import _lib
    sig = _lib.SIGNATURES
    assert "idl_small_wgrad_opt" in sig
    # the optimizer's state, hyperparameters and step words travel as one idl_opt_state_t in front, where the RMSprop form has square_avg,
    # momentum_buffer and its float hyper: two fewer
    assert len(sig["idl_small_wgrad_opt"][1]) == len(sig["idl_small_wgrad_rms_momentum"][1]) - 2 == 21
    assert sig["idl_small_wgrad_opt"][1][0] == ctypes.POINTER(_lib.idl_opt_state_t)
    assert sig["idl_small_wgrad_opt"][1][4:] == sig["idl_small_wgrad_rms_momentum"][1][6:]         # from x on: the same arguments
    assert hasattr(_lib.lib, "idl_small_wgrad_opt")                                                    # exported by the library


def test_parser_small_opt_step_flag(capsys, monkeypatch):
    from idelucs_amd import __main__ as M
    p = M.build_parser()
    for v in ("native", "autograd"):
        assert vars(p.parse_args(["--small_opt_step", v]))["small_opt_step"] == v
    with pytest.raises(SystemExit):
        p.parse_args(["--small_opt_step", "fused"])
    capsys.readouterr()
    assert "small_opt_step" not in vars(p.parse_args([]))
    # without the flag, what main() prints and hands on (the results table's Parameters cell) has no small_opt_step entry
    got = []
    monkeypatch.setattr(M, "run", lambda args: got.append(dict(args)))
    M.main(["--sequence_file", "x.fas", "--model_size", "small", "--optimizer", "Adam"])
    assert "small_opt_step" not in got[0] and "small_opt_step" not in capsys.readouterr().out
    M.main(["--sequence_file", "x.fas", "--model_size", "small", "--optimizer", "Adam", "--small_opt_step", "native"])
    assert got[1]["small_opt_step"] == "native" and "small_opt_step \t -> native" in capsys.readouterr().out
    from idelucs import __main__ as M2                 # `python -m idelucs` shares the parser
    assert M2.main is M.main


def test_golden_stays_within_its_float64_twin():
    """small_optimizers.json, from the reference's own IID_model: the share of a tensor's entries where its float32 steps leave rtol 1e-4 /
    atol 1e-6 of their float64 twin is 0 for SGD and at most 1e-3 for Adam (half of what the GPU test allows Adam), at the recorded seed."""
    import numpy as np
    meta = json.load(open(os.path.join(GOLDEN, "small_optimizers.json")))
    assert (meta["F"], meta["C"], meta["B"], meta["k"], meta["steps"]) == (10, 5, 9, 2, 3)
    assert isinstance(meta["weight_seed"], int) and (meta["rtol"], meta["atol"]) == (1e-4, 1e-6)
    assert meta["cap"] == {"SGD": 0.0, "Adam": 1e-3}
    for opt in ("SGD", "Adam"):
        shares = meta[f"{opt}.share_outside_float64_twin"]
        assert len(shares) == 3 and all(len(s) == 8 for s in shares)
        worst = max(max(s.values()) for s in shares)
        assert worst <= meta["cap"][opt], (opt, worst)
    assert meta["SGD.defaults"]["momentum"] == 0.9 and meta["SGD.defaults"]["weight_decay"] == 0.01 and not meta["SGD.defaults"]["nesterov"]
    assert meta["Adam.defaults"]["betas"] == [0.9, 0.999] and not meta["Adam.defaults"]["amsgrad"]
    g = np.load(os.path.join(GOLDEN, "small_optimizers.npz"))
    assert g["x1"].shape == (9, 10) and g["w.layers.3.weight"].shape == (128, 400)
    for opt in ("SGD", "Adam"):
        assert g[f"{opt}.step2.p.layers.3.weight"].shape == (16, 400) and g[f"{opt}.step2.p.layers.0.weight"].shape == (400, 10)
        assert f"{opt}.step0.p.layers.0.bias" in g.files and f"{opt}.step0.p.layers.0.weight" not in g.files
    assert os.path.getsize(os.path.join(GOLDEN, "small_optimizers.npz")) < 1 << 20
