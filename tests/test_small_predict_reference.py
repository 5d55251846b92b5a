"""CPU tests of tests/small_predict_ref.py, the yardstick of test_gpu_small_predict_native.py: the float64 restatement is myNet's eval forward; the
a-priori bars let the kernels' arithmetic through and catch every broken form, on every input the GPU test runs; the exact cases are exact; the
argmax test's skip set stays under its cap by the reference alone."""
import numpy as np
import pytest
import torch

import small_predict_ref as R


def _weights(net):
    return [p.detach().numpy() for p in (net.layers[0].weight, net.layers[0].bias, net.layers[3].weight, net.layers[3].bias, net.instance.weight,
                                         net.instance.bias, net.classifier[1].weight, net.classifier[1].bias)]


def test_the_restatement_is_mynets_eval_forward():
    from idelucs_amd.PytorchUtils import myNet
    torch.manual_seed(5)
    for F, C in ((136, 5), (512, 200)):
        net = myNet(F, C).double().eval()
        for p in net.parameters():
            torch.nn.init.normal_(p, std=0.2)
        x = torch.randn(24, F, dtype=torch.float64)
        with torch.no_grad():
            z, lat = net(x)
        r = R.forward64(x.numpy(), *_weights(net))
        assert (r["p2"] < 0).any() and (r["p2"] > 0).any()
        assert np.abs(r["lat"] - lat.numpy()).max() <= 1e-11 and np.abs(r["z"] - z.numpy()).max() <= 1e-12
        prob, unit = torch.max(z, 1)
        assert np.array_equal(r["unit"], unit.numpy()) and np.abs(r["prob"] - prob.numpy()).max() <= 1e-12


def test_the_row_lengths_are_the_small_models():
    assert [R.n_features(k) for k in (4, 5, 6, 7)] == [136, 512, 2080, 8192] and R.WIDEST_F == 131072
    assert 136 % R.STAGE != 0 and 136 % 16 != 0 and 2080 % 64 != 0        # the tail stages the cases are there for


@pytest.mark.parametrize("case", R.RANDOM_CASES + [c + (1.0,) for c in R.ROWS_ALONE], ids=str)
def test_the_float32_replay_passes_the_bars_and_the_broken_ones_fail_them(case):
    o = R.random_operands(*case)
    r, b = R.reference("random", case)

    def worst(**broken):
        g = R.replay32(**o, **broken)
        return max(R.over_bar(g["lat"], r["lat"], b["lat"]), R.over_bar(g["z"], r["z"], b["z"]))

    assert worst() <= 1.0
    F = case[1]
    last = (F + R.STAGE - 1) // R.STAGE - 1
    assert worst(drop_l1_stage=last) > 1.0, f"a replay without the last K stage of layer 1 (F' = {F}) passes the bars"
    assert worst(drop_l1_stage=0) > 1.0
    # (F' = 2080: the planted rows are long and lat's worst-case bar is wider than bi and than LeakyReLU's negative side; there these two forms leave
    #  the exact value instead: test_the_negative_cases_pin_the_slope_product, which has a case at 2080)
    for name in ("drop_b1", "drop_b2") + (("drop_bi", "relu2") if F == 136 else ()):
        assert worst(**{name: True}) > 1.0, f"a replay with {name} passes the bars"
    assert worst(slope=0.1) > 1.0, "a replay with slope 0.1 passes the bars"
    assert worst(dropout1=2.0) > 1.0, "a replay with the first Dropout's factor 2 passes the bars"
    if case[3] == 1.0:          # (the classifier's Dropout reaches z alone, and at Wc x 10 z's bar is as wide as z: the other cases hold it)
        assert worst(dropout2=2.0) > 1.0, "a replay with the classifier's Dropout's factor 2 passes the bars"
    for c in (0, R.H1 // 16 - 1):
        assert worst(drop_l2_chunk=c) > 1.0, f"a replay without K chunk {c} of layer 2 passes the bars"
    ok = R.replay32(**o)
    skip = R.margin_rows(r["z"], b["z"])
    assert np.array_equal(ok["unit"][~skip], r["unit"][~skip])
    assert np.array_equal(ok["prob"], ok["z"][np.arange(len(ok["unit"])), ok["unit"]])


def test_unit_is_the_lowest_class_among_equal_values():
    o = R.random_operands(*R.RANDOM_CASES[0])
    Wc = np.array(o["Wc"]); bc = np.array(o["bc"])
    Wc[3], bc[3] = Wc[1], bc[1]                                        # classes 1 and 3 are the same class
    tied = dict(o, Wc=Wc, bc=bc)
    r = R.forward64(**tied)
    assert np.array_equal(r["z"][:, 1], r["z"][:, 3]) and 1 in r["unit"] and 3 not in r["unit"]
    assert np.array_equal(R.replay32(**tied)["unit"], r["unit"])
    high = R.replay32(**tied, top_highest=True)["unit"]
    assert 3 in high and not np.array_equal(high, r["unit"]), "taking the highest class on a tie goes unnoticed"


def test_a_large_logit_case_is_one():
    r, _ = R.reference("random", R.LARGE_LOGIT_CASE)
    assert r["logit"].max() > 100.0                                    # exp overflows fp32 beyond 88.7 unless the row's largest logit is subtracted


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=str)
def test_every_exact_case_has_exact_partial_sums(case):
    o = R.exact_operands(*case)
    assert R.exact_ok(**o)
    r, b = R.reference("exact", case)
    assert (r["p2"] >= 0).all()
    g = R.replay32(**o)
    assert R.first_mismatch(g["lat"], r["lat"]) is None                # any float32 order gives the float64 value
    assert R.over_bar(g["z"], r["z"], b["z"]) <= 1.0
    if case[0] >= 15:
        assert (r["lat"] > 0).any() and (r["lat"] < 0).any()
    if case[1] < R.WIDEST_F:
        bad = dict(o, x=np.array(o["x"]) * np.float32(2.0 ** 12))      # the condition is one on the inputs: larger entries break it
        assert not R.exact_ok(**bad)
        F = case[1]
        cut = R.replay32(**o, drop_l1_stage=(F + R.STAGE - 1) // R.STAGE - 1)
        assert R.first_mismatch(cut["lat"], r["lat"]) is not None, "the last stage of layer 1 does not reach the latent"


@pytest.mark.parametrize("case", R.NEGATIVE_CASES, ids=str)
def test_the_negative_cases_pin_the_slope_product(case):
    o = R.exact_operands(*case, negative=True)
    assert R.exact_ok(**o)
    r, b = R.reference("negative", case)
    want = R.negative_latent32(o)
    neg = r["p2"][:, 1::2] < 0
    assert neg.any() and (~neg).any()
    g = R.replay32(**o)
    assert np.array_equal(g["lat"].view(np.int32), want.view(np.int32))
    assert R.over_bar(want, r["lat"], b["lat"]) <= 1.0
    for broken in (dict(relu2=True), dict(slope=0.1), dict(drop_b2=True), dict(drop_bi=True)):
        bad = R.replay32(**o, **broken)["lat"]
        assert not np.array_equal(bad.view(np.int32), want.view(np.int32)), broken


@pytest.mark.parametrize("case", R.RANDOM_CASES, ids=str)
def test_the_reference_alone_keeps_the_argmax_tests_skip_set_under_its_cap(case):
    r, b = R.reference("random", case)
    share = float(R.margin_rows(r["z"], b["z"]).mean())
    assert share <= R.MARGIN_CAP, f"{share:.3f} of the rows have a top-two margin inside twice the bar"
    assert len(set(r["unit"].tolist())) == min(case[2], 96, R.H2)      # ... and the rows do not all name one class
