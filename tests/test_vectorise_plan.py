"""csrc/vectorise_plan.h on a CPU: the vectoriser's launch policy is one pure function, so what the launcher did BEFORE the policy was gathered there
can be replayed through it.  tests/vectorise_routes_parent.jsonl holds, for every case of a grid that crosses each boundary the old launchers tested
(k, mode / init / out kind, views, edits, the length bounds of v4 and v3, v3's 80 KB and its workgroups per CU, 16-bit bins, every IDELUCS_DEV key), the
arguments, the device's three numbers and the line the old launcher printed under IDELUCS_DEBUG on an MI355X (n = 4 sequences of 100 bases each)."""
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "idelucs_amd", "csrc")
ROUTES = os.path.join(ROOT, "tests", "vectorise_routes_parent.jsonl")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("plan") / "driver"
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "vectorise_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture(scope="module")
def replay(driver):
    """(recorded case, the driver's line, the driver's plan fields) for every recorded case."""
    cases = [json.loads(l) for l in open(ROUTES)]
    assert len(cases) > 300
    feed = []
    for c in cases:
        m = re.search(r"-> (\d+) workgroups/CU$", c["line"] or "")
        feed.append(" ".join(str(x) for x in (c["k"], c["mode"], c["init"], c["out_kind"], c["n_views"], c["has_edits"], c["n"], c["max_len"], c["cus"],
                                              c["lds_per_cu"], c["max_dyn_lds"], m.group(1) if m else 0, c["dev"] or "-")))
    out = subprocess.run([driver], input="\n".join(feed) + "\n", capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "IDELUCS_DEV"})
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert len(lines) == 2 * len(cases) + 1, "the driver answered %d lines for %d cases" % (len(lines) - 1, len(cases))     # (no case skipped)
    return [(c, lines[2 * i], dict(kv.split("=") for kv in lines[2 * i + 1].split())) for i, c in enumerate(cases)]


def test_the_plan_prints_what_the_five_launchers_printed(replay):
    seen = set()
    for c, line, f in replay:
        if c["line"] is None:       # the launcher refused: more LDS than a workgroup may take
            assert line == "too large" and ("needs %s bytes of LDS" % f["lds"]) in c["error"], (c, line, f)
        else:
            assert line == c["line"], (c, line)
        seen.add((f["kernel"], f["rl"], f["om"]))
    # every kernel and every instance the launcher's switch names was recorded (DIAG, a timing build of v3, aside)
    names = {"v1": 1, "v2": 2, "v2b16": 3, "v3": 4, "v4": 5, "slices": 6}
    want = {(names["v1"], 0, 0), (names["v2"], 0, 0), (names["v2b16"], 0, 0), (names["slices"], 0, 0), (names["v3"], 0, 0)}
    want |= {(names["v3"], rl, 0) for rl in (3, 4, 5)} | {(names["v4"], rl, om) for rl in (0, 2, 3, 4) for om in (0, 1)}
    assert want <= {(int(a), int(b), int(c_)) for a, b, c_ in seen}, want - {(int(a), int(b), int(c_)) for a, b, c_ in seen}


def test_the_plans_lds_is_the_layout_functions(replay):
    """The bytes the plan asks for are the layout function's value at the kernel arguments the plan sets (vectorise_layout.h: the one statement of each
    kernel's LDS); a second pass is v2's function at 160 staged slots, and is planned behind v3 and v4 and nowhere else."""
    for c, _, f in replay:
        assert int(f["lds"]) == int(f["layout"]) > 0, (c, f)
        if int(f["redo"]):
            assert int(f["redo_sc"]) == 160 and int(f["redo_lds"]) == int(f["redo_layout"]) and int(f["redo_grid"]) == min(4 * c["cus"], c["n"]), (c, f)
        assert (int(f["redo"]) != 0) == (int(f["kernel"]) in (4, 5)) and int(f["redo"]) == {4: 1, 5: 2}.get(int(f["kernel"]), 0), (c, f)


def test_each_lds_sum_is_written_once():
    """No kernel's LDS size is restated beside its layout function."""
    text = {fn: open(os.path.join(CSRC, fn)).read() for fn in ("vectorise.hip", "vectorise_pairs.h", "vectorise_slices.h", "vectorise_plan.h", "vectorise_layout.h")}
    assert sum(t.count("V2_EDIT_CAP + V2_LIST_CAP") for t in text.values()) == 1 and "V2_EDIT_CAP + V2_LIST_CAP" in text["vectorise_layout.h"]
    assert sum(t.count("3 * V3_META + 2 * V3_VTAB + 16") for t in text.values()) == 1
    for key in ("v3_chunk", "wg_per_cu", "v4_waves"):        # the keys nothing used
        assert not any(('"%s"' % key) in t for t in text.values()), key
