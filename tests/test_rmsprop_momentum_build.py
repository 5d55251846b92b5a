"""CPU tests of the native RMSprop steps that follow CyclicLR's momentum (--rmsprop_momentum follow): opt_step_kernel<3> and the
momentum form of the small step's last launch compile for gfx950 without scratch and within their launch bounds (hipcc
cross-compiles), the new entry point is declared, the CLI flag leaves no trace when it is not given, and the momentum trace of the
reference's golden equals what torch's CyclicLR writes into a fresh RMSprop here."""
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

# file -> {kernel name (substring of the mangled name): (its __launch_bounds__, the waves a SIMD must hold of it or None)}
# opt_step_kernel<3> keeps the same four read streams in flight as Adam's instantiation (p, g, square_avg, momentum_buffer): its bound
KERNELS = {"opt_step.hip": {"opt_step_kernelILi3E": (256, 3)},
           "small_step.hip": {"small_wgrad_momentum_kernel": (512, None)}}
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("fname", sorted(KERNELS))
def test_momentum_kernels_have_no_scratch_and_fit_their_launch_bounds(tmp_path, fname):
    src = os.path.join(ROOT, "idelucs_amd", "csrc", fname)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "out.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        for k in KERNELS[fname]:
            if k in name:
                agpr = re.search(r" AGPRs: (\d+)", b)
                seen[k] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)),
                           int(agpr.group(1)) if agpr else 0, int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    assert set(seen) == set(KERNELS[fname]), (seen, [b.split()[0] for b in blocks])
    for k, (scratch, vgprs, agprs, lds) in seen.items():
        threads, waves = KERNELS[fname][k]
        waves_per_simd = -(-threads // 256)             # a workgroup's waves spread over the CU's four SIMDs
        assert scratch == 0, (k, scratch)
        assert vgprs + agprs <= 512 // waves_per_simd, (k, vgprs, agprs)
        if waves is not None:
            assert vgprs + agprs <= 512 // waves // 8 * 8, (k, vgprs, agprs, waves)
        assert lds <= 65536, (k, lds)
    if fname == "small_step.hip":                       # (tests/test_small_step_build.py matches by substring: the new name must not collide)
        assert not [b.split()[0] for b in blocks if "small_wgrad_momentum_kernel" in b.split()[0] and "small_wgrad_rms_kernel" in b.split()[0]]


def test_momentum_entry_points_are_declared():
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    assert "idl_small_wgrad_rms_momentum(" in hdr
    assert re.search(r"kind 3: RMSprop[^\n]*models\.py:87-88", hdr) and "models.py:99" in hdr
    from idelucs_amd import _lib
    assert "idl_small_wgrad_rms_momentum" in _lib.SIGNATURES
    # one more pointer array than idl_small_wgrad_rms, otherwise the same arguments
    assert len(_lib.SIGNATURES["idl_small_wgrad_rms_momentum"][1]) == len(_lib.SIGNATURES["idl_small_wgrad_rms"][1]) + 1


def test_parser_rmsprop_momentum_flag(capsys, monkeypatch):
    from idelucs_amd import __main__ as M
    p = M.build_parser()
    for v in ("ignore", "follow"):
        assert vars(p.parse_args(["--rmsprop_momentum", v]))["rmsprop_momentum"] == v
    with pytest.raises(SystemExit):
        p.parse_args(["--rmsprop_momentum", "cycle"])
    capsys.readouterr()
    assert "rmsprop_momentum" not in vars(p.parse_args([]))
    # without the flag, what main() prints and hands on (the results table's Parameters cell) has no rmsprop_momentum entry
    got = []
    monkeypatch.setattr(M, "run", lambda args: got.append(dict(args)))
    M.main(["--sequence_file", "x.fas", "--scheduler", "Triangle"])
    assert "rmsprop_momentum" not in got[0] and "rmsprop_momentum" not in capsys.readouterr().out
    M.main(["--sequence_file", "x.fas", "--scheduler", "Triangle", "--rmsprop_momentum", "follow"])
    assert got[1]["rmsprop_momentum"] == "follow" and "rmsprop_momentum \t -> follow" in capsys.readouterr().out
    from idelucs import __main__ as M2                 # `python -m idelucs` shares the parser
    assert M2.main is M.main


def test_golden_momentum_trace_is_what_cyclic_lr_writes_here():
    """triangle.json, from the reference's own IID_model: 30 scheduler steps of CyclicLR(base 1e-3, max 1e-1, step_size_up 5, triangular2)
    on RMSprop(lr, weight_decay 0.01) -- the same objects built here give the same (lr, momentum), value for value."""
    import torch
    meta = json.load(open(os.path.join(GOLDEN, "triangle.json")))
    w = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.RMSprop([w], lr=1e-3, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.CyclicLR(opt, base_lr=0.001, max_lr=0.1, step_size_up=5, mode="triangular2")
    grp = opt.param_groups[0]
    assert [grp['lr'], grp['momentum']] == meta["at_construction"] == [0.001, 0.9]
    lr, mom = [], []
    for _ in range(30):
        w.grad = torch.zeros_like(w)
        opt.step()
        sched.step()
        lr.append(grp['lr'])
        mom.append(grp['momentum'])
    assert mom == meta["momentum_trace"] and lr == meta["lr_trace"]
    assert [round(v, 6) for v in mom[:10]] == [0.88, 0.86, 0.84, 0.82, 0.80, 0.82, 0.84, 0.86, 0.88, 0.90]
    # after one step torch's RMSprop holds a momentum buffer: the algorithm the reference trains under --scheduler Triangle
    assert sorted(opt.state[w]) == ["momentum_buffer", "square_avg", "step"]
    # the generator's own float32-against-float64 figure stays under its cap (the tests allow 5e-3 of a tensor's entries outside)
    for size in ("linear", "small"):
        worst = max(max(o.values()) for o in meta[f"{size}.share_outside_float64_twin"])
        assert worst <= meta["twin_cap"] == 2e-3, (size, worst)
