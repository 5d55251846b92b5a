"""NetLinear's opt-in native step computes what it computed before its last launch, idl_opt_step_gather_wgrad, took its arguments as structs
and its dW2 tile took its operand loops from a shared text, bit for bit: tools/linear_opt_last_launch_bits.py's cases (SGD, Adam and RMSprop
with momentum on five routes to the last launch, two eager epochs of the trainer each) replayed on the current tree against
tests/linear_opt_last_launch_parent.jsonl, that tool's output on the tree and library of the commit before the change."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("linear_opt_last_launch_bits", os.path.join(ROOT, "tools", "linear_opt_last_launch_bits.py"))
BITS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(BITS)
PARENT = os.path.join(ROOT, "tests", "linear_opt_last_launch_parent.jsonl")


def test_the_recorded_cases_are_the_tools():
    """Three optimizers x five routes, in the tool's order, every tensor the steps leave behind hashed (SGD keeps no second state)."""
    rec = [json.loads(line) for line in open(PARENT)]
    assert [r["case"] for r in rec] == [BITS.case_name(*c) for c in BITS.CASES] and len(rec) == 15
    assert {(b, F, C) for _, b, F, C, _ in BITS.CASES} == {(16, 256, 5), (256, 256, 5), (24, 68, 5), (9, 68, 60), (24, 68, 60)}
    for r, (kind, *_) in zip(rec, BITS.CASES):
        names = {f"{k}{i}" for k in ("param", "state1_") + (("state2_",) if kind != "SGD" else ()) for i in range(6)}
        names |= {"grad2", "out", "ctl", "steps", "x"}
        assert set(r["sha256"]) == names and all(len(h) == 64 for h in r["sha256"].values()), r["case"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BITS.CASES, ids=[BITS.case_name(*c).replace(" ", "-") for c in BITS.CASES])
def test_opt_step_bits_are_the_parents(case):
    import torch
    from idelucs_amd import _lib
    _lib.require_gpu()
    want = {r["case"]: r["sha256"] for r in map(json.loads, open(PARENT))}[BITS.case_name(*case)]
    got = BITS.run_case(*case, torch.device("cuda"))
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
