"""CPU tests of the streamed feature store (utils.StreamedFeatureStore, csrc/vectorise_pairs.h, idl_col_stats_stream*): the new entries
are declared, exported and bound; what they do not build is refused with a message, at the C entry and at IID_model / parser level; the
--store flag parses and leaves the namespace alone when it is not given."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ["idl_vectorise_pairs_supported", "idl_vectorise_pairs_at", "idl_vectorise_pairs_planes_at", "idl_col_stats_stream_workspace", "idl_col_stats_stream", "idl_col_stats_stream_finish"]


def test_new_entries_are_declared_exported_and_bound():
    from idelucs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "idelucs_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/idelucs_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        fn = getattr(_lib.lib, name)                    # exported by the shared library
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0]
    # the header's parameter count is the binding's
    for name in NEW:
        decl = re.search(r"^(?:int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S | re.M).group(1)
        assert len([p for p in decl.split(",") if p.strip() and p.strip() != "void"]) == len(_lib.SIGNATURES[name][1]), name


def test_supported_predicate_states_the_kernels_bounds():
    from idelucs_amd import _lib
    ok = _lib.lib.idl_vectorise_pairs_supported
    for k in range(4, 10):
        assert ok(k, 4 ** k, 512, 10_000) == 1, k
    assert ok(3, 64, 512, 100) == 0 and ok(10, 4 ** 10, 512, 100) == 0          # k outside 4..9
    assert ok(6, 2080, 512, 100) == 0                                           # a canonical row length
    assert ok(6, 4096, 512, 1 << 30) == 0 and ok(6, 4096, (1 << 30) + 1, 100) == 0 and ok(6, 4096, -1, 100) == 0
    assert ok(6, 4096, 0, 0) == 1                                               # max_len 0 = unknown


def _pairs_at(_lib, k=6, mode=None, init=None, n_views=4):
    """The entry with NULL buffers: the argument checks come before anything touches a device."""
    mode = _lib.MODE_KMER if mode is None else mode
    init = _lib.INIT_ONE if init is None else init
    return _lib.lib.idl_vectorise_pairs_at(None, None, None, None, 10, k, mode, init, n_views, None, None, 100, None, None, None, None, None, 0,
                                           4, 30, None, None)


def test_the_c_entry_refuses_what_it_does_not_build():
    from idelucs_amd import _lib
    for kw, word in ((dict(mode=_lib.MODE_CANONICAL), "canonical"), (dict(mode=_lib.MODE_CGR), "CGR"), (dict(init=_lib.INIT_FROM_OUT), "IDL_INIT_FROM_OUT"),
                     (dict(init=_lib.INIT_ZERO), "IDL_INIT_ONE"), (dict(k=3), "k outside 4"), (dict(k=1), "k outside 4"), (dict(k=10), "k outside 4"),
                     (dict(n_views=1), "n_views")):
        assert _pairs_at(_lib, **kw) == _lib.IDL_ERR_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    with pytest.raises(ValueError, match="canonical"):
        _lib.check(_pairs_at(_lib, mode=_lib.MODE_CANONICAL))
    # a supported call with NULL buffers is refused as such, not launched
    assert _pairs_at(_lib) == _lib.IDL_ERR_ARG and "NULL" in _lib.last_error()


def test_col_stats_stream_refuses_bad_chunks():
    from idelucs_amd import _lib
    L = _lib.lib
    assert L.idl_col_stats_stream_workspace(1000, 4096) == L.idl_counts_stream_workspace(1000, 4096) > 0
    buf = ctypes.create_string_buffer(64)
    x = ctypes.c_void_p(ctypes.addressof(buf) & ~15)
    assert L.idl_col_stats_stream(x, 0, 4, 10, 6, x, None) == _lib.IDL_ERR_ARG          # 4 | f
    assert L.idl_col_stats_stream(x, 8, 4, 10, 8, x, None) == _lib.IDL_ERR_ARG and "leaves the matrix" in _lib.last_error()
    assert L.idl_col_stats_stream(x, -1, 4, 10, 8, x, None) == _lib.IDL_ERR_ARG
    assert L.idl_col_stats_stream(None, 0, 4, 10, 8, x, None) == _lib.IDL_ERR_ARG and "NULL" in _lib.last_error()
    assert L.idl_col_stats_stream(x, 3, 0, 10, 8, x, None) == _lib.IDL_OK               # an empty chunk is nothing to do
    assert L.idl_col_stats_stream_finish(10, 6, x, x, x, None) == _lib.IDL_ERR_ARG


BASE = {'sequence_file': 'x.fas', 'GT_file': None, 'n_clusters': 5, 'k': 6, 'model_size': 'linear', 'n_mimics': 3, 'batch_sz': 64,
        'optimizer': 'RMSprop', 'lambda': 2.8, 'lr': 1e-3, 'weight': 0.25, 'scheduler': None}


def test_store_argument_of_the_model():
    from idelucs_amd.models import IID_model
    mode = IID_model._store_mode
    assert mode(BASE) == 'resident' and mode({**BASE, 'store': None}) == 'resident' and mode({**BASE, 'store': 'resident'}) == 'resident'
    assert mode({**BASE, 'store': 'streamed'}) == 'streamed'
    for k in (4, 9):
        assert mode({**BASE, 'store': 'streamed', 'k': k}) == 'streamed'
    with pytest.raises(ValueError, match="store must be 'resident' or 'streamed'"):
        mode({**BASE, 'store': 'disk'})
    # the resident store takes every configuration it took
    assert mode({**BASE, 'model_size': 'small', 'small_step': 'native', 'rng': 'compat', 'k': 3}) == 'resident'


@pytest.mark.parametrize("extra, word", [
    ({'model_size': 'small'}, "canonical"),
    ({'k': 3}, "4 <= k <= 9"),
    ({'rng': 'compat'}, "rng='philox'"),
    ({'optimizer': 'SGD', 'linear_step': 'native'}, "linear_step='native'"),
    ({'model_size': 'linear', 'small_step': 'native'}, "small_step='native'"),
    ({'optimizer': 'Adam', 'small_opt_step': 'native'}, "small_opt_step='native'"),
    ({'scheduler': 'Triangle', 'rmsprop_momentum': 'follow'}, "rmsprop_momentum='follow'"),
])
def test_streamed_store_names_the_limit_it_refuses(extra, word):
    from idelucs_amd.models import IID_model
    with pytest.raises(ValueError, match=re.escape(word)):
        IID_model._store_mode({**BASE, 'store': 'streamed', **extra})


def test_build_feature_store_refuses_compat_and_canonical_rows_before_reading_the_file(monkeypatch):
    from idelucs_amd import utils as U
    monkeypatch.setattr(U, "_device", lambda device=None: "cpu")        # (the refusals need no device)
    with pytest.raises(ValueError, match="rng='philox'"):
        U.build_feature_store("no_such_file.fas", 3, k=6, rng="compat", resident=False)
    with pytest.raises(ValueError, match="canonical"):
        U.build_feature_store("no_such_file.fas", 3, k=6, rng="philox", reduce=True, resident=False)
    with pytest.raises(ValueError, match="4 <= k <= 9"):
        U.build_feature_store("no_such_file.fas", 3, k=3, rng="philox", resident=False)


def test_can_batch_is_false_on_a_streamed_store():
    import types
    from idelucs_amd import training
    m = types.SimpleNamespace(_use_fused=True, batch_sz=64, schedule="None", n_clusters=5, _streamed_store=False)
    assert training.can_batch(m)
    m._streamed_store = True
    assert not training.can_batch(m)


def test_store_flag_parses_and_is_absent_without_it(capsys, monkeypatch):
    from idelucs_amd import __main__ as M
    p = M.build_parser()
    assert "store" not in vars(p.parse_args(["--sequence_file", "x.fas"]))
    assert vars(p.parse_args(["--sequence_file", "x.fas", "--store", "streamed"]))["store"] == "streamed"
    assert vars(p.parse_args(["--store", "resident"]))["store"] == "resident"
    with pytest.raises(SystemExit):
        p.parse_args(["--store", "disk"])
    capsys.readouterr()
    got = []
    monkeypatch.setattr(M, "run", lambda args: got.append(dict(args)))
    M.main(["--sequence_file", "x.fas"])
    assert "store" not in got[0] and "store" not in capsys.readouterr().out          # the printed parameters are unchanged
    M.main(["--sequence_file", "x.fas", "--store", "streamed"])
    assert got[1]["store"] == "streamed" and "store \t -> streamed" in capsys.readouterr().out
    import idelucs.__main__ as R                    # `python -m idelucs` is the same parser
    assert R.main is M.main


def test_cluster_entry_point_takes_the_store_keyword():
    from idelucs_amd.cluster import iDeLUCS_cluster
    assert "store" not in iDeLUCS_cluster("x.fas").args
    assert iDeLUCS_cluster("x.fas", store="streamed").args["store"] == "streamed"
