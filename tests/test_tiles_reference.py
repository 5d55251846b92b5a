"""CPU tests of tests/tiles_ref.py: the exactness condition holds for every (kernel, shape, case) test_gpu_tiles_exact.py runs, fp32 accumulation of
those operands is the float64 reference bit for bit in three different orders (what lets the GPU test ignore the kernels' summation order), the plane
reference is distinguishable from a product with the w1 x1 term, first_mismatch names planted errors, and a correctly rounded fp32 RMSprop update sits
inside half of the bars the GPU test asserts."""
import numpy as np
import pytest

import tiles_ref as R

ALL = [(kern, shape, case) for kern in R.SHAPES for shape in R.SHAPES[kern] for case in R.CASES]
_id = lambda p: f"{p[0]}-{'x'.join(map(str, p[1]))}-{p[2]}"


def _ks(kernel):
    return R.XPLANES_K if kernel == "xplanes" else (0,)


@pytest.mark.parametrize("kern", list(R.SHAPES))
def test_exactness_condition_holds_for_every_case_the_gpu_test_runs(kern):
    for shape in R.SHAPES[kern]:
        for case in R.CASES:
            o = R.operands(kern, shape, case)
            for k in _ks(kern):
                pairs, scale = R.terms(kern, o, k)
                assert R.exact_ok(pairs, scale), (kern, shape, case, k)
                ref = R.reference(kern, shape, case, k)
                assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    # ... and it is a condition: entries of 2^11 over K = 4096 break it, a fraction breaks it
    big = np.full((4, 4096), 2048.0)
    assert not R.exact_ok([(big, big.T)]) and R.exact_ok([(big[:, :3], big[:, :3].T)])
    assert not R.exact_ok([(np.array([[0.5]]), np.array([[1.0]]))]) and not R.exact_ok([(np.ones((1, 1)), np.ones((1, 1)))], scale=3.0)


def test_operands_are_what_the_issue_asks_for():
    o = R.operands("l1_fwd", (256, 4096), "dense")
    for a in (o["W"], o["x"]):
        assert a.dtype == np.float32 and np.abs(a).max() == R.LIM and 0.28 < (a == 0).mean() < 0.39
    o = R.operands("l1_planes", (384, 256, 2048), "dense")
    for name in ("wh", "wl", "xh", "xl"):                  # both planes of BOTH operands: all three plane products matter
        assert o[name].dtype == np.int16 and (R.f16_vals(o[name]) != 0).mean() > 0.6, name
    o = R.operands("xplanes", (192, 512, 1024), "dense")
    for name in ("dyh", "dyl", "xh", "xl"):
        assert (R.f16_vals(o[name]) != 0).mean() > 0.6, name
    # the address cases: the output IS the other operand's entry
    o = R.operands("l1_fwd", (96, 192), "address")
    ref = R.reference("l1_fwd", (96, 192), "address")
    assert (o["W"].sum(1) == 1).all() and np.array_equal(ref, o["x"].astype(np.float64)[:, o["k"]].T)
    o = R.operands("wgrad", (96, 128, 256), "address")
    assert np.array_equal(R.reference("wgrad", (96, 128, 256), "address"), o["x"].astype(np.float64)[o["k"], :])
    o = R.operands("at_b", (513, 17, 70), "address")
    assert np.array_equal(R.reference("at_b", (513, 17, 70), "address"), o["B"].astype(np.float64)[o["k"], :])
    shape = (128, 128, 1536)
    o = R.operands("l1_planes", shape, "address")
    ref = R.reference("l1_planes", shape, "address")
    kr = shape[2] // R.KSPLIT
    h, r = 5, 77
    want = np.zeros(R.KSPLIT)
    want[o["k"][h] // kr] += o["k"][h] + 2048 * (r % 8 + 1)
    want[o["k1"][h] // kr] += o["k1"][h]
    assert o["k"][h] // kr != o["k1"][h] // kr and np.array_equal(ref[:, h, r] * 2.0 ** 15, want)
    assert np.array_equal(R.operands("wgrad", (32, 64, 128), "dense")["dy"], R.operands("wgrad", (32, 64, 128), "dense")["dy"])


def _accumulate32(pairs, ks, scale):
    """fp32 accumulation, one k after the other in the order ks, the pairs' terms of a k one after the other"""
    R_, C = pairs[0][0].shape[0], pairs[0][1].shape[1]
    acc = np.zeros((R_, C), np.float32)
    tmp = np.empty_like(acc)
    p32 = [(np.ascontiguousarray(A.T, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)) for A, B in pairs]
    for k in ks:
        for AT, B in p32:
            np.multiply.outer(AT[k], B[k], out=tmp)
            acc += tmp
    return acc * np.float32(scale)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("kern,shape,case", ALL, ids=map(_id, ALL))
def test_fp32_accumulation_is_the_reference_in_any_order(kern, shape, case):
    """forward, reversed, and as 8 K slices added afterwards: the same bits as the float64 reference (the plane kernels' slices each on their own too)"""
    o = R.operands(kern, shape, case)
    k = _ks(kern)[-1]
    pairs, scale = R.terms(kern, o, k)
    ref = R.reference(kern, shape, case, k)
    K = pairs[0][0].shape[1]
    total = ref.sum(0) if kern == "l1_planes" else ref
    want = _bits(total)
    assert np.array_equal(_bits(_accumulate32(pairs, range(K), scale)), want)
    assert np.array_equal(_bits(_accumulate32(pairs, range(K - 1, -1, -1), scale)), want)
    cuts = np.linspace(0, K, R.KSPLIT + 1).astype(int)
    parts = [_accumulate32(pairs, range(cuts[s], cuts[s + 1]), scale) for s in range(R.KSPLIT)]
    acc = np.zeros_like(parts[0])
    for p in parts:
        acc = acc + p
    assert acc.dtype == np.float32 and np.array_equal(_bits(acc), want)
    if kern == "l1_planes":
        for s in range(R.KSPLIT):
            assert np.array_equal(_bits(parts[s]), _bits(ref[s])), s


def test_the_missing_low_plane_product_is_observable():
    for shape in R.SHAPES["l1_planes"]:
        o = R.operands("l1_planes", shape, "dense")
        full = R.ref_full_planes_product(o["wh"], o["wl"], o["xh"], o["xl"])
        ours = R.reference("l1_planes", shape, "dense").sum(0)
        assert (full != ours).mean() > 0.9, shape
        assert np.array_equal(R.ref_l1_planes(o["wh"], o["wl"], o["xh"], o["xl"], rows=True), R.reference("l1_planes", shape, "dense").transpose(0, 2, 1))
    for shape in R.SHAPES["xplanes"]:
        o = R.operands("xplanes", shape, "dense")
        full = (R.f16_vals(o["dyh"]) + R.f16_vals(o["dyl"])).T @ (R.f16_vals(o["xh"]) + R.f16_vals(o["xl"])) * 2.0 ** -R.X_EXP
        assert (full != R.reference("xplanes", shape, "dense", 0)).mean() > 0.9, shape


def test_first_mismatch_names_planted_errors():
    shape = (256, 128, 1024)
    o = R.operands("l1_planes", shape, "dense")
    ref = R.reference("l1_planes", shape, "dense")
    tile = R.TILES["l1_planes"]
    good = ref.astype(np.float32)
    mm = R.first_mismatch(good, ref, tile)
    assert mm["count"] == 0 and mm["index"] is None and "equal" in R.describe(mm, "x")
    # one element changed (by one unit of the last place)
    bad = good.copy()
    bad[5, 100, 131] = np.nextafter(bad[5, 100, 131], np.float32(np.inf))
    mm = R.first_mismatch(bad, ref, tile)
    assert (mm["count"], mm["index"], mm["slice"], mm["tile"], mm["in_tile"]) == (1, (5, 100, 131), 5, (0, 1), (100, 3))
    assert mm["got"] == float(bad[5, 100, 131]) and mm["want"] == float(ref[5, 100, 131])
    msg = R.describe(mm, "idl_l1_planes")
    assert "(5, 100, 131)" in msg and "K slice 5" in msg and "tile (0, 1)" in msg and "(100, 3)" in msg
    # two columns (k = 200, 201: K slice 1) of an operand swapped: only slice 1 differs, and in the rows whose two entries differ
    wh = o["wh"].copy(); wh[:, [200, 201]] = wh[:, [201, 200]]
    got = R.ref_l1_planes(wh, o["wl"], o["xh"], o["xl"]).astype(np.float32)
    mm = R.first_mismatch(got, ref, tile)
    assert mm["count"] > 0 and mm["slice"] == 1 and np.array_equal(got[[0, 2, 3, 4, 5, 6, 7]], good[[0, 2, 3, 4, 5, 6, 7]])
    h = mm["index"][1]
    assert o["wh"][h, 200] != o["wh"][h, 201] and all(o["wh"][i, 200] == o["wh"][i, 201] for i in range(h))
    # one lo entry zeroed: hidden unit 77 at k = 900 (slice 7) -- that row of slice 7, wherever x0 is non-zero there
    assert o["wl"][77, 900] != 0
    wl = o["wl"].copy(); wl[77, 900] = 0
    got = R.ref_l1_planes(o["wh"], wl, o["xh"], o["xl"]).astype(np.float32)
    mm = R.first_mismatch(got, ref, tile)
    x0 = R.f16_vals(o["xh"])[:, 900]
    assert mm["count"] == int((x0 != 0).sum()) and mm["index"] == (7, 77, int(np.flatnonzero(x0)[0])) and mm["tile"] == (0, mm["index"][2] // 128)
    # one K chunk of 64 dropped (k in [320, 384): slice 2)
    xh = o["xh"].copy(); xl = o["xl"].copy(); xh[:, 320:384] = 0; xl[:, 320:384] = 0
    got = R.ref_l1_planes(o["wh"], o["wl"], xh, xl).astype(np.float32)
    mm = R.first_mismatch(got, ref, tile)
    assert mm["slice"] == 2 and mm["count"] > 0.9 * ref[2].size and np.array_equal(np.delete(got, 2, 0), np.delete(good, 2, 0))
    # the same on a 2-D result of the fp32 tiles
    o = R.operands("wgrad", (96, 128, 256), "address")
    ref2 = R.reference("wgrad", (96, 128, 256), "address")
    x = o["x"].copy(); x[:, [130, 131]] = x[:, [131, 130]]
    mm = R.first_mismatch(R.ref_wgrad(o["dy"], x).astype(np.float32), ref2, R.TILES["wgrad"])
    assert (mm["count"], mm["index"], mm["slice"], mm["tile"], mm["in_tile"]) == (2 * 128, (0, 130), None, (0, 1), (0, 2))
    assert mm["got"] == o["k"][0] * 256 + 131                 # the address case says what was read: column 131 of row m_0


@pytest.mark.parametrize("lr,alpha", [(1e-3, 0.99), (0.25, 0.9)])
def test_fp32_replay_of_the_update_is_inside_half_the_bars(lr, alpha, capsys):
    """A correctly rounded fp32 update (no FMA, IEEE sqrt and division) deviates from the float64 one by at most half of what the GPU test allows the
    kernels' epilogue (v_sqrt_f32 and v_rcp_f32 at 1 ulp, FMA contraction): the bars are not vacuous."""
    hy = R.hyper(lr, alpha)
    worst = [0.0, 0.0]
    for kern, shape, k in (("wgrad", (96, 128, 256), 0), ("wgrad", (1024, 64, 128), 0), ("xplanes", (192, 128, 256), 10), ("xplanes", (192, 128, 256), -3)):
        g = R.reference(kern, shape, "dense", k)
        W0, V0 = R.rms_start(g, (kern, shape, k))
        assert (np.abs(W0) <= 1).all() and (W0 != 0).all() and (V0 >= 0).all() and (V0 == 0).any() and (g * W0 >= 0).all()
        W1, V1 = R.rmsprop32(g, W0, V0, hy)
        dv, dw = R.epilogue_deviation(W1, V1, g, W0, V0, hy)
        worst = [max(worst[0], dv), max(worst[1], dw)]
        # the deviation measure sees an error of the size it is meant to catch: V off by 16 ulp, the step off by 2^-19 of itself
        _, _, step = R.rmsprop64(g, W0, V0, hy)
        dv2, _ = R.epilogue_deviation(W1, V1 * np.float32(1 + 2.0 ** -20), g, W0, V0, hy)
        _, dw2 = R.epilogue_deviation((W1.astype(np.float64) - step * 2.0 ** -19).astype(np.float32), V1, g, W0, V0, hy)
        assert dv2 > R.V_BAR and (dw2 > R.W_BAR or lr < 0.01), (dv2, dw2)
    with capsys.disabled():
        print(f"\n  fp32 replay lr={lr} alpha={alpha}: V {worst[0]:.2f} x 2^-24 relative, W 0.5 ulp + {worst[1]:.2f} x 2^-24 |step|")
    assert worst[0] <= R.V_BAR / 2 and worst[1] <= R.W_BAR / 2, worst
