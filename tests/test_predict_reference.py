"""CPU tests of tests/predict_ref.py, the yardstick of test_gpu_predict_native.py: the float64 restatement is NetLinear's eval forward; the a-priori bar
lets the kernels' arithmetic through and catches what it has to catch, on every input the GPU test runs; the exact cases are exact; the argmax test's
skip set stays under its cap by the reference alone."""
import numpy as np
import pytest
import torch

import predict_ref as R


def test_the_restatement_is_netlinears_eval_forward():
    from idelucs_amd.PytorchUtils import NetLinear
    torch.manual_seed(5)
    for F, C in ((256, 5), (320, 200)):
        net = NetLinear(F, C).double().eval()
        for p in net.parameters():
            torch.nn.init.normal_(p, std=0.2)
        x = torch.randn(24, F, dtype=torch.float64)
        with torch.no_grad():
            z, lat = net(x)
        w = [p.detach().numpy() for p in (net.layers[0].weight, net.layers[0].bias, net.layers[3].weight, net.layers[3].bias,
                                          net.classifier[2].weight, net.classifier[2].bias)]
        r = R.forward64(x.numpy(), *w)
        assert np.abs(r["lat"] - lat.numpy()).max() <= 1e-12 and np.abs(r["z"] - z.numpy()).max() <= 1e-12
        prob, unit = torch.max(z, 1)
        assert np.array_equal(r["unit"], unit.numpy()) and np.abs(r["prob"] - prob.numpy()).max() <= 1e-12


def test_unit_is_the_lowest_index_among_equal_values():
    o = R.random_operands(*R.RANDOM_CASES[0])
    W3 = np.array(o["W3"]); b3 = np.array(o["b3"])
    W3[3], b3[3] = W3[1], b3[1]                                   # classes 1 and 3 are the same class
    r = R.forward64(o["x"], o["W1"], o["b1"], o["W2"], o["b2"], W3, b3)
    assert np.array_equal(r["z"][:, 1], r["z"][:, 3]) and 1 in r["unit"] and 3 not in r["unit"]


@pytest.mark.parametrize("case", R.RANDOM_CASES + [R.ROWS_ALONE + (1.0,)], ids=str)
def test_the_float32_replay_passes_the_bar_and_the_broken_ones_fail_it(case):
    o = R.random_operands(*case)
    r, b = R.reference("random", case)

    def worst(**broken):
        g = R.replay32(**o, **broken)
        return max(R.over_bar(g["lat"], r["lat"], b["lat"]), R.over_bar(g["z"], r["z"], b["z"]))

    assert worst() <= 1.0
    F = case[1]
    for chunk in (0, F // 64 - 1):
        assert worst(drop_l1_chunk=chunk) > 1.0, f"a replay without K chunk {chunk} of layer 1 passes the bar"
    assert worst(drop_b1=True) > 1.0, "a replay without b1 passes the bar"
    for s in (0, 15):
        assert worst(drop_l2_slice=s) > 1.0, f"a replay without K slice {s} of layer 2 passes the bar"
    ok = R.replay32(**o)
    skip = R.margin_rows(r["z"], b["z"])
    assert np.array_equal(ok["unit"][~skip], r["unit"][~skip])


def test_a_softmax_without_the_max_subtraction_fails_the_bar_on_large_logits():
    o = R.random_operands(*R.LARGE_LOGIT_CASE)
    r, b = R.reference("random", R.LARGE_LOGIT_CASE)
    assert r["logit"].max() > 100.0                                # exp overflows fp32 beyond 88.7
    assert R.over_bar(R.replay32(**o)["z"], r["z"], b["z"]) <= 1.0
    assert R.over_bar(R.replay32(**o, subtract_max=False)["z"], r["z"], b["z"]) > 1.0


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=str)
def test_every_exact_case_has_exact_partial_sums(case):
    o = R.exact_operands(*case)
    assert R.exact_ok(**o)
    r, b = R.reference("exact", case)
    g = R.replay32(**o)
    assert R.first_mismatch(g["lat"], r["lat"]) is None            # any float32 order gives the float64 value
    assert R.over_bar(g["z"], r["z"], b["z"]) <= 1.0
    assert (r["lat"] > 0).any() and (r["lat"] < 0).any()
    bad = dict(o, x=np.array(o["x"]) * np.float32(2.0 ** 12))      # the condition is one on the inputs: larger entries break it
    assert not R.exact_ok(**bad)


@pytest.mark.parametrize("case", R.RANDOM_CASES, ids=str)
def test_the_reference_alone_keeps_the_argmax_tests_skip_set_under_its_cap(case):
    r, b = R.reference("random", case)
    share = float(R.margin_rows(r["z"], b["z"]).mean())
    assert share <= R.MARGIN_CAP, f"{share:.3f} of the rows have a top-two margin inside twice the bar"
    assert len(set(r["unit"].tolist())) == min(case[2], 64)        # ... and the rows do not all name one unit


def test_mismatch_messages_name_row_column_and_tile():
    want = np.arange(64 * 64, dtype=np.float64).reshape(64, 64)
    got = want.astype(np.float32)
    assert R.first_mismatch(got, want) is None
    got[37, 5] += 1
    msg = R.first_mismatch(got, want)
    assert "row 37, column 5 (tile 2, row 5 of the tile)" in msg
