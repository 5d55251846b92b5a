"""The embedding behind --plot is part of the build: embed.hip among the library's sources, its entry points declared in the
header, bound in _lib.py and exported, and --plot still the reference's flag."""
import os
import re

from conftest import ROOT

SYMBOLS = ("idl_knn_graph", "idl_umap_smooth_knn", "idl_umap_layout_epoch", "idl_umap_draws", "idl_umap_jitter")


def test_embed_hip_is_a_library_source():
    mk = open(os.path.join(ROOT, "idelucs_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC_HIP\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "embed.hip" in src and "knn.hip" in src
    assert os.path.exists(os.path.join(ROOT, "idelucs_amd", "csrc", "embed.hip"))


def test_symbols_declared_bound_and_exported():
    from idelucs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/idelucs_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
    assert len(_lib.SIGNATURES["idl_umap_layout_epoch"][1]) == 14 and len(_lib.SIGNATURES["idl_knn_graph"][1]) == 17


def test_public_surface():
    import inspect
    from idelucs_amd import posthoc
    sig = inspect.signature(posthoc.umap_embedding_device)
    assert list(sig.parameters)[:6] == ["latent", "n_neighbors", "min_dist", "n_epochs", "seed", "device"]
    assert [sig.parameters[p].default for p in ("n_neighbors", "min_dist", "n_epochs", "seed", "device")] == [15, 0.1, None, 42, None]
    assert list(inspect.signature(posthoc.knn_graph_device).parameters)[:3] == ["x", "k", "device"]
    assert posthoc.umap_default_epochs(10000) == 500 and posthoc.umap_default_epochs(10001) == 200
    a, b = posthoc.umap_ab_params()
    assert abs(a - 1.5769434603) < 1e-6 and abs(b - 0.8950608779) < 1e-6


def test_plot_flag_is_the_references():
    from idelucs_amd.__main__ import build_parser
    p = build_parser()
    act = {a.dest: a for a in p._actions}["plot"]
    assert act.type is bool and act.default is False and act.option_strings == ["--plot"]
    assert p.parse_args(["--plot", "True"]).plot is True
