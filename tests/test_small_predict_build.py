"""small_predict='native' is part of the build: small_predict.hip among the library's sources, its kernels without scratch, both symbols declared,
bound and exported with their argument refusals (nothing touches a device), the CLI flag on both parsers, IID_model's validator and the predictor's
shape arithmetic -- all without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

BASE = {'sequence_file': 'x.fas', 'GT_file': None, 'n_clusters': 5, 'k': 6, 'model_size': 'small', 'n_mimics': 3, 'batch_sz': 64,
        'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None, 'n_epochs': 1, 'n_voters': 1}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_both_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """Layer 1 keeps 25 accumulators (100 registers), nine staged float4s and a group of five W1 fragments a lane: two waves a SIMD need it below 256
    registers; its LDS is dynamic (two stages of 528 rows).  The middle launch holds a 16-row tile of a1, a2 and the logits: below 64 KB."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    mk = open(os.path.join(ROOT, "idelucs_amd", "csrc", "Makefile")).read()
    assert "small_predict.hip" in re.search(r"^SRC_HIP\s*:=\s*(.*)$", mk, re.M).group(1).split()
    src = os.path.join(ROOT, "idelucs_amd", "csrc", "small_predict.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "small_predict.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        for name in ("small_predict_l1_kernel", "small_predict_mid_kernel"):
            if name in b.split()[0]:
                seen[name] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r" VGPRs: (\d+)", b).group(1)),
                              int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    assert set(seen) == {"small_predict_l1_kernel", "small_predict_mid_kernel"}, r.stderr[-2000:]
    scratch, vgprs, lds = seen["small_predict_l1_kernel"]
    assert scratch == 0 and vgprs <= 256 and lds == 0, seen
    scratch, vgprs, lds = seen["small_predict_mid_kernel"]
    assert scratch == 0 and vgprs <= 128 and lds <= 65536, seen


def test_both_symbols_are_declared_bound_and_exported():
    from idelucs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    for name, n_want in (("idl_small_predict_l1", 6), ("idl_small_predict_mid", 15)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, f"{name} is not declared in include/idelucs_hip.h"
        n_params = len([p for p in m.group(1).split(",") if p.strip()])
        assert n_params == n_want and len(_lib.SIGNATURES[name][1]) == n_params
        assert hasattr(_lib.lib, name)
    assert _lib.lib.idl_abi_version() == 1
    assert "PytorchUtils.py:13-22" in hdr and "PytorchUtils.py:15-22" in hdr       # the contract cites the reference


def test_small_predict_mid_argument_refusals():
    from idelucs_amd import _lib
    f = _lib.lib.idl_small_predict_mid
    p = 4096                                    # (a non-NULL, aligned address: every call below is refused before anything is launched)
    bufs = lambda: [p] * 8
    assert f(*bufs(), 0, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG and "m >= 1" in _lib.last_error()
    assert f(*bufs(), -3, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG
    assert f(*bufs(), 32, 0, p, p, p, p, None) == _lib.IDL_ERR_ARG and "1..256" in _lib.last_error()
    assert f(*bufs(), 32, 257, p, p, p, p, None) == _lib.IDL_ERR_ARG
    for i in range(8):                          # every input
        a = bufs()
        a[i] = None
        assert f(*a, 32, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG and "NULL" in _lib.last_error(), i
    assert f(*bufs(), 32, 5, None, p, p, p, None) == _lib.IDL_ERR_ARG           # lat
    assert f(*bufs(), 32, 5, p, None, None, p, None) == _lib.IDL_ERR_ARG        # prob (z alone may be NULL)
    assert f(*bufs(), 32, 5, p, None, p, None, None) == _lib.IDL_ERR_ARG        # unit
    for i in (0, 1, 2, 4, 6):                   # a1, b1, W2, Wi, Wc: read as float4
        a = bufs()
        a[i] = p + 4
        assert f(*a, 32, 5, p, p, p, p, None) == _lib.IDL_ERR_ARG and "aligned" in _lib.last_error(), i


def test_small_predict_l1_argument_refusals():
    from idelucs_amd import _lib
    f = _lib.lib.idl_small_predict_l1
    p = 4096
    assert f(None, p, 16, 136, p, None) == _lib.IDL_ERR_ARG and "NULL" in _lib.last_error()
    assert f(p, None, 16, 136, p, None) == _lib.IDL_ERR_ARG and f(p, p, 16, 136, None, None) == _lib.IDL_ERR_ARG
    assert f(p, p, 0, 136, p, None) == _lib.IDL_ERR_ARG and "m >= 1" in _lib.last_error()
    for F in (0, 2, 135, 138):
        assert f(p, p, 16, F, p, None) == _lib.IDL_ERR_ARG and "multiple of 4" in _lib.last_error(), F
    assert f(p + 8, p, 16, 136, p, None) == _lib.IDL_ERR_ARG and "aligned" in _lib.last_error()
    assert f(p, p + 4, 16, 136, p, None) == _lib.IDL_ERR_ARG and "aligned" in _lib.last_error()


def test_the_flag_parses_and_is_absent_by_default_on_both_parsers():
    import idelucs.__main__ as ref_cli
    import idelucs_amd.__main__ as cli
    assert ref_cli.main is cli.main                                 # `python -m idelucs` is the same parser
    p = cli.build_parser()
    assert "small_predict" not in vars(p.parse_args(["--sequence_file", "x.fas"]))
    assert "small_predict" not in vars(p.parse_args(["--sequence_file", "x.fas", "--model_size", "small", "--predict", "torch"]))
    assert vars(p.parse_args(["--sequence_file", "x.fas", "--small_predict", "native"]))["small_predict"] == "native"
    assert vars(p.parse_args(["--sequence_file", "x.fas", "--small_predict", "torch"]))["small_predict"] == "torch"
    ns = vars(p.parse_args(["--assign", "new.fas", "--model", "out", "--small_predict", "native"]))
    assert ns["small_predict"] == "native" and ns["assign"] == "new.fas"
    with pytest.raises(SystemExit):
        p.parse_args(["--sequence_file", "x.fas", "--small_predict", "fast"])


def test_the_validator_accepts_its_scope_and_says_why_not():
    from idelucs_amd import utils
    from idelucs_amd.models import IID_model
    mode = IID_model._small_predict_mode
    assert mode(dict(BASE)) == 'torch' and mode(dict(BASE, small_predict=None)) == 'torch' and mode(dict(BASE, small_predict='torch')) == 'torch'
    assert mode(dict(BASE, small_predict='torch', model_size='linear', k=1, n_clusters=300)) == 'torch'     # today's path asks for nothing
    assert mode(dict(BASE, small_predict='torch', model_size='linear', predict='native')) == 'torch'
    for k in (4, 5, 6, 7, 9):
        assert utils.stream_route_ok(k, True)
        for c in (1, 5, 200, 256):
            assert mode(dict(BASE, small_predict='native', k=k, n_clusters=c)) == 'native'
    # independent of optimizer, step form and scheduler
    assert mode(dict(BASE, small_predict='native', small_step='native', scheduler='Triangle', rmsprop_momentum='follow')) == 'native'
    assert mode(dict(BASE, small_predict='native', optimizer='Adam', small_opt_step='native')) == 'native'
    with pytest.raises(ValueError, match="model_size='small', got 'linear'"):
        mode(dict(BASE, small_predict='native', model_size='linear'))
    k_bad = next(k for k in range(1, 10) if not utils.stream_route_ok(k, True))
    with pytest.raises(ValueError, match=f"k={k_bad}"):
        mode(dict(BASE, small_predict='native', k=k_bad))
    with pytest.raises(ValueError, match="n_clusters=300"):
        mode(dict(BASE, small_predict='native', n_clusters=300))
    with pytest.raises(ValueError, match="n_clusters=0"):
        mode(dict(BASE, small_predict='native', n_clusters=0))
    with pytest.raises(ValueError, match="'torch' or 'native', not 'fast'"):
        mode(dict(BASE, small_predict='fast'))
    with pytest.raises(ValueError, match="exclude each other"):
        mode(dict(BASE, small_predict='native', predict='native'))
    # predict='native' itself keeps refusing model_size='small', with its message
    with pytest.raises(ValueError, match="model_size='linear'"):
        IID_model._predict_mode(dict(BASE, predict='native'))


def test_the_predictors_shapes():
    from idelucs_amd import predict_native as P
    assert P.small_supported(136, 5) and P.small_supported(4, 1) and P.small_supported(131072, 256) and P.small_supported(2080, 200)
    assert not P.small_supported(0, 5) and not P.small_supported(2, 5) and not P.small_supported(138, 5)
    assert not P.small_supported(136, 0) and not P.small_supported(136, 257)
    for F in (4, 136, 512, 2080, 8192, 32896, 131072):
        b = P.small_block_rows(F)
        assert 1 <= b <= P.MAX_BLOCK_ROWS and b * F < 2 ** 29 and (b == P.MAX_BLOCK_ROWS or (b + 1) * F >= 2 ** 29)
    assert P.small_block_rows(2080) == 32768 and P.small_block_rows(131072) == 4095


def test_the_predictor_checks_mynets_shapes():
    import torch
    from idelucs_amd import predict_native as P
    from idelucs_amd.PytorchUtils import myNet
    pred = P.NativeSmallPredictor(myNet(136, 7))
    assert (pred.F, pred.C) == (136, 7) and pred._a1 is None
    with pytest.raises(ValueError, match="n_clusters in 1..256"):
        P.NativeSmallPredictor(myNet(136, 300))
    with pytest.raises(ValueError, match="F % 4 == 0"):
        P.NativeSmallPredictor(myNet(32 // 2 - 2, 5))
    net = myNet(136, 7)
    net.instance = torch.nn.Linear(128, 32)
    with pytest.raises(ValueError, match="takes a myNet"):
        P.NativeSmallPredictor(net)
    with pytest.raises(ValueError, match="float32 device matrix"):
        pred.forward(torch.zeros((4, 136)))


def test_a_saved_ensemble_takes_the_key_and_refuses_outside_its_scope():
    import torch
    from idelucs_amd.ensemble import FittedEnsemble
    from idelucs_amd.PytorchUtils import NetLinear, myNet

    def ens_of(model_size, f, net):
        state = {name: t.detach().clone() for name, t in net.state_dict().items()}
        return FittedEnsemble(4, model_size, 7, "ensemble", torch.zeros(f, dtype=torch.float64), torch.ones(f, dtype=torch.float64), [state],
                              unit_maps=torch.zeros((1, 7), dtype=torch.int32), counts=torch.zeros((7, 1, 7), dtype=torch.int64),
                              cnt=torch.zeros(7, dtype=torch.int64))

    small, linear = ens_of("small", 136, myNet(136, 7)), ens_of("linear", 256, NetLinear(256, 7))
    assert small._small_predict_mode('native') == 'native' and small._small_predict_mode(None) == 'torch'
    with pytest.raises(ValueError, match="model_size='small', got 'linear'"):
        linear.voter_outputs("none.fas", small_predict='native')
    with pytest.raises(ValueError, match="'torch' or 'native'"):
        small.assign("none.fas", small_predict='fast')
    with pytest.raises(ValueError, match="exclude each other"):
        linear.assign("none.fas", predict='native', small_predict='native')
    with pytest.raises(ValueError, match="model_size='linear'"):            # as before
        small.voter_outputs("none.fas", predict='native')
