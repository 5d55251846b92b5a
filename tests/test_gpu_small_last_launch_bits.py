"""The small step's last launch computes what it computed before its four kernels were put on one tile body, bit for bit:
tools/small_last_launch_bits.py's cases (the four forms at five shapes, without and with the riding assembly of the next batch, one
launch each) replayed on the current build against tests/small_last_launch_parent.jsonl, that tool's output on the library built from
the commit before the change."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("small_last_launch_bits", os.path.join(ROOT, "tools", "small_last_launch_bits.py"))
BITS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(BITS)
PARENT = os.path.join(ROOT, "tests", "small_last_launch_parent.jsonl")


def test_the_recorded_cases_are_the_tools():
    """Four forms x five shapes x (no rider, rider), in the tool's order, every written tensor hashed."""
    rec = [json.loads(line) for line in open(PARENT)]
    assert [r["case"] for r in rec] == [BITS.case_name(*c) for c in BITS.CASES] and len(rec) == 40
    assert {(m, F, C) for _, m, F, C, _ in BITS.CASES} == {(2, 1, 1), (18, 63, 31), (34, 136, 200), (66, 2080, 256), (1022, 63, 5)}
    names = {f"{k}{i}" for k in ("param", "state1_", "state2_", "grad") for i in range(8)} | {"out", "ctl", "steps", "next"}
    for r in rec:
        assert set(r["sha256"]) == names and all(len(h) == 64 for h in r["sha256"].values()), r["case"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BITS.CASES, ids=[BITS.case_name(*c).replace(" ", "-") for c in BITS.CASES])
def test_last_launch_bits_are_the_parents(case):
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    want = {r["case"]: r["sha256"] for r in map(json.loads, open(PARENT))}[BITS.case_name(*case)]
    got = BITS.run_case(*case, torch.device("cuda"))
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
