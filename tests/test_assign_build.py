"""Saving an ensemble and assigning new sequences is part of the build: nn_rows.hip among the library's sources, idl_nn_rows declared,
bound and exported, its argument refusals (called with NULL buffers: nothing touches a device), the two CLI flags, and FittedEnsemble's
file format and scope limits -- all without a GPU."""
import os
import re

import pytest

from conftest import ROOT


def _header_params(name):
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
    assert m, f"{name} is not declared in include/idelucs_hip.h"
    return [p for p in m.group(1).split(",") if p.strip()]


def test_nn_rows_is_built_declared_bound_and_exported():
    from idelucs_amd import _lib
    mk = open(os.path.join(ROOT, "idelucs_amd", "csrc", "Makefile")).read()
    assert "nn_rows.hip" in re.search(r"^SRC_HIP\s*:=\s*(.*)$", mk, re.M).group(1).split()
    for name, n_params in (("idl_nn_rows", 9), ("idl_nn_rows_slices", 2)):
        assert len(_header_params(name)) == n_params
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_params, f"{name}: the binding's parameter count is not the header's"
        assert hasattr(_lib.lib, name), f"{name} is not exported"


def test_nn_rows_argument_refusals():
    from idelucs_amd import _lib
    f = _lib.lib.idl_nn_rows
    ok, bad = _lib.IDL_OK, _lib.IDL_ERR_ARG
    null = (None, None, None)
    assert f(None, 5, None, 10, 32, -1, *null) == bad and "64" in _lib.last_error()              # d != 64
    assert f(None, 5, None, 0, 64, -1, *null) == bad                                             # n < 1
    assert f(None, 5, None, 2 ** 31, 64, -1, *null) == bad                                       # n >= 2^31
    assert f(None, 5, None, -3, 64, -1, *null) == bad
    assert f(None, 1, None, 1, 64, 0, *null) == bad and "two rows" in _lib.last_error()          # self-exclusion with one corpus row
    assert f(None, -1, None, 10, 64, -1, *null) == bad                                           # m < 0
    assert f(None, 0, None, 10, 64, -1, *null) == ok                                             # m == 0: nothing to do, no launch
    assert f(None, 0, None, 2, 64, 0, *null) == ok
    assert f(None, 5, None, 10, 64, -1, *null) == bad and "NULL" in _lib.last_error()            # NULL buffers
    # the slicing is a function of the sizes alone: none below 2048 corpus rows, at most 64, none where the query tiles fill the device
    g = _lib.lib.idl_nn_rows_slices
    assert g(70, 1000) == 1 and g(70, 2047) == 1 and g(70, 5000) == 4 and g(1, 10 ** 6) == 64 and g(10 ** 6, 10 ** 6) == 1
    assert g(10 ** 5, 10 ** 6) == 3 and g(0, 10) == 1 and g(5, 0) == bad


def test_flags_parse_and_are_absent_by_default():
    from idelucs_amd.__main__ import build_parser
    import idelucs.__main__ as alias
    import idelucs_amd.__main__ as cli
    assert alias.main is cli.main
    p = build_parser()
    ns = vars(p.parse_args(["--sequence_file", "x.fas"]))
    assert not {"save_model", "assign", "model"} & set(ns)
    ns = vars(p.parse_args(["--sequence_file", "x.fas", "--save_model", "out"]))
    assert ns["save_model"] == "out" and "assign" not in ns and "model" not in ns
    ns = vars(p.parse_args(["--assign", "new.fas", "--model", "out"]))
    assert ns["assign"] == "new.fas" and ns["model"] == "out" and ns["sequence_file"] is None
    for argv in (["--assign", "new.fas"], ["--model", "out"], ["--assign", "new.fas", "--model", "out", "--save_model", "again"]):
        with pytest.raises(SystemExit):
            cli.main(argv)


def _by_hand(mode):
    import torch
    from idelucs_amd.ensemble import FittedEnsemble
    from idelucs_amd.PytorchUtils import NetLinear
    g = torch.Generator().manual_seed(3)
    k, f, units = 4, 256, 7
    mean = torch.rand(f, dtype=torch.float64, generator=g)
    scale = torch.rand(f, dtype=torch.float64, generator=g) + 0.5
    states = [{name: t.detach().clone() for name, t in NetLinear(f, units).state_dict().items()} for _ in range(3)]
    if mode == "ensemble":
        return FittedEnsemble(k, "linear", units, "ensemble", mean, scale, states,
                              unit_maps=torch.randint(-1, units, (3, units), generator=g, dtype=torch.int32),
                              counts=torch.randint(0, 50, (units, 3, units), generator=g, dtype=torch.int64),
                              cnt=torch.randint(0, 50, (units,), generator=g, dtype=torch.int64))
    n = 40
    return FittedEnsemble(k, "linear", units, "fine", mean, scale, states[:1], latent=torch.randn(n, 64, generator=g),
                          labels=torch.randint(0, 5, (n,), generator=g, dtype=torch.int64), prob=torch.rand(n, dtype=torch.float64, generator=g),
                          spacing=torch.rand(n, dtype=torch.float64, generator=g))


@pytest.mark.parametrize("mode", ["ensemble", "fine"])
def test_save_load_round_trip(tmp_path, mode):
    import torch
    from idelucs_amd.ensemble import FORMAT_VERSION, FittedEnsemble
    ens = _by_hand(mode)
    path = ens.save(str(tmp_path / "m"))
    assert path == str(tmp_path / "m" / "ensemble.pt") and os.path.exists(path)
    raw = torch.load(path, weights_only=True)                        # tensors and plain Python values only
    assert raw["format_version"] == FORMAT_VERSION and raw["mode"] == mode
    back = FittedEnsemble.load(str(tmp_path / "m"))
    for name in ("version", "k", "model_size", "n_units", "mode"):
        assert getattr(back, name) == getattr(ens, name), name
    for name in FittedEnsemble.TENSORS:
        a, b = getattr(ens, name), getattr(back, name)
        assert (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b)), name
    assert len(back.states) == len(ens.states)
    for s, t in zip(ens.states, back.states):
        assert list(s) == list(t) and all(s[n].dtype == t[n].dtype and torch.equal(s[n], t[n]) for n in s)
    with pytest.raises(FileExistsError):                             # an existing file is not overwritten
        ens.save(str(tmp_path / "m"))
    assert torch.equal(torch.load(path, weights_only=True)["mean"], ens.mean)


def test_scope_refusals(tmp_path, monkeypatch):
    import torch
    from idelucs_amd import ensemble
    from idelucs_amd.ensemble import FittedEnsemble
    ens = _by_hand("ensemble")
    # another format version, in the file and in the constructor
    path = ens.save(str(tmp_path / "v"))
    raw = torch.load(path, weights_only=True)
    raw["format_version"] = ensemble.FORMAT_VERSION + 1
    torch.save(raw, path)
    with pytest.raises(ValueError, match="format version"):
        FittedEnsemble.load(str(tmp_path / "v"))
    # a (k, model_size) whose row length the chunked predict inputs refuse: the canonical rows of k = 2 are 10 long
    with pytest.raises(ValueError, match="multiple of 4"):
        ensemble.check_scope(2, "small")
    with pytest.raises(ValueError, match="multiple of 4"):
        FittedEnsemble(2, "small", 7, "ensemble", ens.mean[:10], ens.scale[:10], ens.states, unit_maps=ens.unit_maps, counts=ens.counts, cnt=ens.cnt)
    ensemble.check_scope(6, "linear")
    ensemble.check_scope(6, "small")
    # several ranks: the voters' weights live elsewhere
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one rank"):
        ensemble.check_scope(6, "linear")
    ens_dir = str(tmp_path / "good")
    monkeypatch.delenv("WORLD_SIZE")
    ens.save(ens_dir)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one rank"):
        FittedEnsemble.load(ens_dir)
    # the CLI refuses before it trains: an existing file, several ranks
    from idelucs_amd.__main__ import run
    args = {"sequence_file": "none.fas", "n_clusters": 5, "k": 6, "model_size": "linear", "n_voters": 3, "save_model": str(tmp_path / "v")}
    with pytest.raises(ValueError, match="one rank"):
        run(dict(args))
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(FileExistsError):
        run(dict(args))
    assert not os.path.exists(os.path.join(os.getcwd(), "Results", "none"))
