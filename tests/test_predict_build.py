"""predict='native' is part of the build: predict.hip among the library's sources, its kernel without scratch, idl_predict_mid declared, bound and
exported with its argument refusals (NULL buffers: nothing touches a device), the CLI flag, and IID_model's validator -- all without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

BASE = {'sequence_file': 'x.fas', 'GT_file': None, 'n_clusters': 5, 'k': 6, 'model_size': 'linear', 'n_mimics': 3, 'batch_sz': 64,
        'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 1, 'n_voters': 1}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_predict_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    """The kernel keeps a lane's eight layer-1 values, four W2 fragments and a W3 fragment in registers from its first instruction on: no scratch, and the
    64 KB of LDS of mid_fwd_body's layout."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    mk = open(os.path.join(ROOT, "idelucs_amd", "csrc", "Makefile")).read()
    assert "predict.hip" in re.search(r"^SRC_HIP\s*:=\s*(.*)$", mk, re.M).group(1).split()
    src = os.path.join(ROOT, "idelucs_amd", "csrc", "predict.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "predict.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        if "predict_mid_kernel" in b.split()[0]:
            seen["predict_mid_kernel"] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)),
                                          int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    assert set(seen) == {"predict_mid_kernel"}, r.stderr[-2000:]
    scratch, vgprs, lds = seen["predict_mid_kernel"]
    assert scratch == 0 and vgprs <= 128 and lds == 65536, seen        # (128 registers: what a 1024-thread workgroup may use)


def test_predict_mid_is_declared_bound_and_exported():
    from idelucs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    m = re.search(r"\bidl_predict_mid\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, "idl_predict_mid is not declared in include/idelucs_hip.h"
    n_params = len([p for p in m.group(1).split(",") if p.strip()])
    assert n_params == 13 and len(_lib.SIGNATURES["idl_predict_mid"][1]) == n_params
    assert hasattr(_lib.lib, "idl_predict_mid") and _lib.lib.idl_abi_version() == 1
    assert "PytorchUtils.py:38-50" in hdr and "models.py:158-170" in hdr       # the contract cites the reference


def test_predict_mid_argument_refusals():
    from idelucs_amd import _lib
    f = _lib.lib.idl_predict_mid
    p = 4096                                    # (a non-NULL, aligned address: every call below is refused before anything is launched)
    bufs = lambda: [p] * 6
    assert f(*bufs(), 40, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG and "multiple of 16" in _lib.last_error()
    assert f(*bufs(), 0, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG
    assert f(*bufs(), 32, 0, p, p, p, p, None) == _lib.IDL_ERR_ARG
    assert f(*bufs(), 32, 257, p, p, p, p, None) == _lib.IDL_ERR_ARG
    assert f(None, p, p, p, p, p, 32, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG and "NULL" in _lib.last_error()
    assert f(*bufs(), 32, 5, None, p, p, p, None) == _lib.IDL_ERR_ARG           # lat
    assert f(*bufs(), 32, 5, p, None, None, p, None) == _lib.IDL_ERR_ARG        # prob (z alone may be NULL)
    assert f(p, p + 4, p, p, p, p, 32, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG and "aligned" in _lib.last_error()


def test_the_flag_parses_and_is_absent_by_default():
    from idelucs_amd.__main__ import build_parser
    p = build_parser()
    assert "predict" not in vars(p.parse_args(["--sequence_file", "x.fas"]))
    assert vars(p.parse_args(["--sequence_file", "x.fas", "--predict", "native"]))["predict"] == "native"
    assert vars(p.parse_args(["--sequence_file", "x.fas", "--predict", "torch"]))["predict"] == "torch"
    ns = vars(p.parse_args(["--assign", "new.fas", "--model", "out", "--predict", "native"]))
    assert ns["predict"] == "native" and ns["assign"] == "new.fas"
    with pytest.raises(SystemExit):
        p.parse_args(["--sequence_file", "x.fas", "--predict", "fast"])


def test_the_validator_accepts_its_scope_and_says_why_not():
    from idelucs_amd.models import IID_model
    mode = IID_model._predict_mode
    assert mode(dict(BASE)) == 'torch' and mode(dict(BASE, predict=None)) == 'torch' and mode(dict(BASE, predict='torch')) == 'torch'
    assert mode(dict(BASE, predict='torch', model_size='small', k=3, n_clusters=300)) == 'torch'        # today's path asks for nothing
    for k in (4, 6, 9):
        for c in (1, 5, 200, 256):
            assert mode(dict(BASE, predict='native', k=k, n_clusters=c)) == 'native'
    # independent of optimizer, store mode, step form and scheduler
    assert mode(dict(BASE, predict='native', optimizer='Adam', linear_step='native', scheduler='Triangle')) == 'native'
    assert mode(dict(BASE, predict='native', store='streamed', rmsprop_momentum='follow')) == 'native'
    with pytest.raises(ValueError, match="model_size='linear'"):
        mode(dict(BASE, predict='native', model_size='small'))
    with pytest.raises(ValueError, match="k=3"):
        mode(dict(BASE, predict='native', k=3))
    with pytest.raises(ValueError, match="n_clusters=300"):
        mode(dict(BASE, predict='native', n_clusters=300))
    with pytest.raises(ValueError, match="n_clusters=0"):
        mode(dict(BASE, predict='native', n_clusters=0))
    with pytest.raises(ValueError, match="'torch' or 'native'"):
        mode(dict(BASE, predict='fast'))


def test_the_predictors_shapes():
    from idelucs_amd import predict_native as P
    assert P.supported(256, 5) and P.supported(192, 1) and P.supported(4 ** 9, 256)
    assert not P.supported(128, 5) and not P.supported(224, 5) and not P.supported(256, 0) and not P.supported(256, 257)
    for F in (192, 256, 4096, 4 ** 8, 4 ** 9):
        b = P.block_rows(F)
        assert b % 32 == 0 and 32 <= b <= P.MAX_BLOCK_ROWS and b * F < 2 ** 29 and (b == P.MAX_BLOCK_ROWS or (b + 32) * F >= 2 ** 29)


def test_a_saved_ensemble_refuses_native_predict_outside_its_scope():
    import torch
    from idelucs_amd.ensemble import FittedEnsemble
    from idelucs_amd.PytorchUtils import myNet
    f = (4 ** 4 + 4 ** 2) // 2
    state = {name: t.detach().clone() for name, t in myNet(f, 7).state_dict().items()}
    ens = FittedEnsemble(4, "small", 7, "ensemble", torch.zeros(f, dtype=torch.float64), torch.ones(f, dtype=torch.float64), [state],
                         unit_maps=torch.zeros((1, 7), dtype=torch.int32), counts=torch.zeros((7, 1, 7), dtype=torch.int64), cnt=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match="model_size='linear'"):
        ens.voter_outputs("none.fas", predict='native')
    with pytest.raises(ValueError, match="'torch' or 'native'"):
        ens.assign("none.fas", predict='fast')
