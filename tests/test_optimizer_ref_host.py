"""CPU checks of the reference that tests/test_gpu_optimizer.py holds t2_sumsq and t2_adam_step to (tests/optimizer_ref.py): the
tolerance constants are anchored to the restatement's own float32 error, the restatement equals the oracle's clip + Adam step, the
case list covers what the GPU test needs, and the share of the tolerance that bias corrections evaluated in float32 use up is worked
out from the numbers."""
import math

import numpy as np
import torch

from oracle import tacotron2_ref as R
from tests import optimizer_ref as O


def test_tolerances_are_anchored_to_the_float32_reference():
    """Over CASES and GRID the float32 run of the restatement differs from the float64 run by at most F32_ERR = TOL / 16 per output
    (and by no less than half of it: a stored constant cannot drift away from what it was measured as)."""
    assert set(O.TOL) == set(O.OUTPUTS) == set(O.F32_ERR)
    for k, tol in O.TOL.items():
        assert tol == 16.0 * O.F32_ERR[k] > 0
    worst = O.measure_f32_err()
    print("[optimizer] float32 restatement against float64, worst case per output:")
    for k in O.OUTPUTS:
        print(f"    {k}  {worst[k][0]:.3g} ({worst[k][1]})  stored F32_ERR {O.F32_ERR[k]:.2g}  TOL {O.TOL[k]:.3g}")
    for k, (e, name) in worst.items():
        assert 0.5 * O.F32_ERR[k] <= e <= O.F32_ERR[k], (k, e, name)


def test_case_list_is_what_the_gpu_test_needs():
    """Every value of every axis the kernels branch or round on occurs in CASES, the product of the small axes in GRID; the largest
    size is above both grid caps; the inputs have the zeros, the binades and the norms their description promises."""
    cs = list(O.CASES.values())
    assert {c["n"] for c in cs} >= set(O.NS) and max(O.NS) > 4096 * 256 > 1024 * 256
    assert {c["clip"] for c in cs} == set(O.CLIPS) | {"tiny"}
    assert {c["grad_scale"] for c in cs} == set(O.GRAD_SCALES) and {c["wd"] for c in cs} == set(O.WDS)
    assert {c["step"] for c in cs} == set(O.STEPS) and {c["lr"] for c in cs} == set(O.LRS)
    assert len(O.GRID) == 4 * 3 * 3 * 5 * 2 and all(c["n"] == 257 for c in O.GRID.values())
    assert len({(c["clip"], c["grad_scale"], c["wd"], c["step"], c["lr"]) for c in O.GRID.values()}) == len(O.GRID)
    for name in ("n1", "n257", "clip_inactive", "clip_off", "clip_none", "tiny_norm", "gs0.125_active", "big_inactive"):
        c = O.CASES[name]
        inp = O.make_inputs(c)
        p, g, m, v = (inp[k] for k in "pgmv")
        assert all(x.dtype == np.float32 and x.shape == (c["n"],) for x in (p, g, m, v))
        tot = math.sqrt(inp["ss_g"]) * c["grad_scale"]
        want = {"active": 16.0, "inactive": 0.3, "off": 16.0, "none": 16.0, "tiny": 16e-5}[c["clip"]]
        assert abs(tot / want - 1.0) < 1e-6, (name, tot)
        assert (inp["ss"] is None) == (c["clip"] == "none")
        clip = float(O.clip_coef(inp["ss"], c["max_norm"], c["grad_scale"]))
        assert (clip < 1.0) == (c["clip"] in ("active", "tiny")), (name, clip)
        if c["n"] > 1000:
            pad = inp["pad"]
            assert 0.04 < pad.mean() < 0.09 and not (p[pad].any() or g[pad].any() or m[pad].any() or v[pad].any())
            assert 0.04 < ((g == 0) & (p != 0)).mean() < 0.09 and 0.04 < ((p == 0) & (g != 0)).mean() < 0.09
            e = np.frexp(g[g != 0])[1]
            assert e.max() - e.min() >= 11                                  # twelve binades and the common factor
            assert bool(np.all(np.sign(g)[(g != 0) & (p != 0)] == np.sign(p)[(g != 0) & (p != 0)]))
            assert not np.any((v == 0) & (g != 0))


def _oracle_step(case, inp):
    """oracle.tacotron2_ref: clip_coef + adam_l2_step in float64 on the case's buffers, the hyper-parameters as the ABI rounds them."""
    t = lambda k: torch.from_numpy(inp[k]).double()
    if inp["ss"] is not None and case["max_norm"] > 0:
        coef, tot = R.clip_coef([t("g")], O.f32(case["max_norm"]))
        assert abs(tot - math.sqrt(inp["ss"])) <= 1e-12 * tot
    else:
        coef = 1.0
    return R.adam_l2_step(t("p"), t("g") * coef, t("m"), t("v"), case["step"], O.f32(case["lr"]), O.f32(case["wd"]),
                          b1=O.f32(O.BETA1), b2=O.f32(O.BETA2), eps=O.f32(O.EPS))


def test_restatement_equals_the_oracle_step():
    """grad_scale = 1: the float64 restatement against oracle.tacotron2_ref.clip_coef + adam_l2_step in float64 - to 1e-10 relative in
    m and v and 1e-3 of p's unit (the two differ in the order of a few float64 operations and in 1e-6 against 1e-6f, which is
    1.6e-11 of the smallest norm of the list, 1.6e-4)."""
    names = [n for n, c in O.CASES.items() if c["grad_scale"] == 1.0 and c["n"] <= 100003]
    grid = [n for n, c in O.GRID.items() if c["grad_scale"] == 1.0]
    assert {O.CASES[n]["clip"] for n in names} >= {"active", "inactive", "tiny"} and len(grid) == 120
    worst = {k: 0.0 for k in O.OUTPUTS}
    for name in names + grid:
        case = O.CASES.get(name) or O.GRID[name]
        inp = O.make_inputs(case)
        ref = O.reference(case, inp)
        p, m, v = _oracle_step(case, inp)
        e = O.errors(dict(p=p.numpy(), m=m.numpy(), v=v.numpy()), ref, case["lr"])
        worst = {k: max(worst[k], e[k]) for k in worst}
        assert e["p"] < 1e-3 and e["m"] < 1e-10 and e["v"] < 1e-10, (name, e)
    print(f"[optimizer] restatement against the oracle over {len(names) + len(grid)} cases: {worst}")


def test_grad_scale_scales_the_norm_and_the_gradient():
    """What grad_scale means, on the reference: a step on (g, grad_scale = s) is the step on (s g, 1) under ITS OWN sumsq - in
    float64 to rounding, and it is not the step that scales the gradient alone."""
    case = O.CASES["gs0.5_active"]
    inp = O.make_inputs(case)
    ref = O.reference(case, inp)
    g2 = (inp["g"] * np.float32(0.5)).astype(np.float32)
    kw = dict(O.step_kwargs(case), grad_scale=1.0)
    same = O.adam_clip_step(inp["p"], g2, inp["m"], inp["v"], O.sumsq(g2), **kw)
    assert all(np.array_equal(same[k], ref[k]) for k in O.OUTPUTS)                 # powers of two commute with every rounding
    wrong = O.adam_clip_step(inp["p"], g2, inp["m"], inp["v"], inp["ss"], **kw)     # the norm of the unscaled gradient
    assert O.errors(wrong, ref, case["lr"])["m"] > 1e-2


def test_non_finite_norm_skips_the_step():
    case = O.CASES["n257"]
    inp = O.make_inputs(case)
    for ss in (float("inf"), float("nan")):
        out = O.adam_clip_step(inp["p"], inp["g"], inp["m"], inp["v"], ss, **O.step_kwargs(case))
        assert all(np.array_equal(out[k], inp[k].astype(np.float64)) for k in O.OUTPUTS)


def test_padding_keeps_its_parameter():
    """g = m = v = 0 and wd p = 0: the update ratio is 0 / (0 + eps) = 0 and p' = p exactly, in both precisions."""
    for name in ("n100003", "wd0.0", "wd0.1"):
        case = O.CASES[name]
        inp = O.make_inputs(case)
        still = (inp["g"] == 0) & (inp["m"] == 0) & (inp["v"] == 0) & ((inp["p"] == 0) | (case["wd"] == 0.0))
        assert still.sum() >= inp["pad"].sum() > 0
        for dt in (np.float64, np.float32):
            out = O.reference(case, inp, dt)
            assert np.array_equal(out["p"][still], inp["p"][still].astype(dt)) and not out["m"][still].any()


def test_float32_bias_corrections_stay_inside_the_tolerance():
    """1 - powf(beta, step) in float32 against 1 - beta^step in float64, beta the float32 value: the relative error of bc1 enters
    p's update ratio once, that of bc2 through the square root, half.  Where p_ref = 0 the unit of p is the update alone, so the sum
    in units of 2^-24 is what such corrections add to p's deviation.  Worst over steps 1 .. 200000: step 2, 1.3 + 55.8 units
    (0.999f^2 rounded to 24 bits in a difference of 0.002) - inside TOL[p] - F32_ERR[p] = 60, which is what the factor 16 is for (the per-step
    figures of the case list are printed)."""
    s = np.arange(1, 200001)
    units = np.zeros(len(s))
    for beta, weight in ((O.BETA1, 1.0), (O.BETA2, 0.5)):
        b = np.float32(beta)
        bc32 = (np.float32(1.0) - np.power(b, s.astype(np.float32))).astype(np.float64)
        bc64 = 1.0 - np.float64(b) ** s
        units += weight * np.abs(bc32 / bc64 - 1.0) / 2.0 ** -24
    i = int(np.argmax(units))
    print(f"[optimizer] float32 bias corrections: worst step {int(s[i])}, {units[i]:.1f} units of p; at the case list's steps "
          + ", ".join(f"{k}: {units[k - 1]:.2f}" for k in O.STEPS))
    assert units[0] == 0.0                                   # step 1: 1 - beta, exact
    assert int(s[i]) == 2 and 50.0 < units[i] < O.TOL["p"] - O.F32_ERR["p"]
