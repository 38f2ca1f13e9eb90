"""Reference for the kernel-level tests of the update's options: a float64 numpy restatement of t2_adam_step_opt as
include/tacotron2_amd.h defines it, with the dtype as a parameter - float64 is the reference, float32 only yields the tolerances.
CPU only, no torch.  Inputs, the clip and the p / m / v metrics are tests/optimizer_ref.py's (O below); this module adds the two
options and the fifth buffer.

    clip, bc1, bc2 as in optimizer_ref (clip contains grad_scale)
    coupled   (decoupled = 0):  O.adam_clip_step, unchanged
    decoupled (decoupled = 1):  g' = g * clip;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
                                p1 = p * (1 - lr * wd);  p' = p1 - lr * (m' / bc1) / (sqrt(v' / bc2) + eps)
    EMA (d is not None):        ema' = ema + (1 - d) * (p' - ema)
A sumsq that is not finite leaves p, m, v and ema as they are.  d, like every other hyper-parameter, is the float32-ROUNDED value in
float64 (optimizer_ref.f32): 1 - d is then exact in both runs.

The ema input (make_inputs): p * (1 + u 2^-3), u uniform in (-1, 1) from a generator of its own, rounded to float32 - the same sign
as p, 0 where p is 0 (the padding, and the elements whose p alone is 0): the fixed point ema == p' == 0 of the padding is in every
case.

The ema metric (errors): per element |got - ref| in units of 2^-24 (|ema| + (1 - d) |p' - ema|), ema the input and p' the float64
reference - half a float32 ulp of the two terms ema' is formed from, as optimizer_ref's unit for p.  Where the unit is 0 anything but
equality is infinite.  p' carries its own error into ema', times (1 - d): at d = 0 the ema metric is p's error in another unit.

Tolerances: 16 x the float32 restatement's own largest deviation from the float64 one over the committed list CASES, the project's
convention (optimizer_ref.py, Tolerances), per path: the coupled path's p / m / v constants are optimizer_ref.TOL itself - the same
arithmetic, and the list here stays inside that list's ranges (test_optimizer_options_host.py checks that they hold here too); the
decoupled path has p / m / v constants of its own; `ema` has one constant for both paths.  Measured on the CPU (measure_f32_err;
tests/test_optimizer_options_host.py re-measures them and holds each constant to [measured, 2 x measured]), never from a kernel's
output:
    decoupled p   3.82 units of 2^-24 (|p_ref| + lr |ratio|)        F32_ERR 4.0       TOL 64      (n1049353_adamw_ema)
    decoupled m   1.31e-7 relative                                  F32_ERR 1.5e-7    TOL 2.4e-6  (n1049353_adamw_ema)
    decoupled v   1.66e-7 relative                                  F32_ERR 2.0e-7    TOL 3.2e-6  (n1049353_adamw_ema)
    ema           4.88 units of 2^-24 (|ema| + (1 - d) |p' - ema|)  F32_ERR 5.0       TOL 80      (n1049353_adamw_ema)
    coupled p / m / v over this list: 2.97 / 1.29e-7 / 1.70e-7 (big_adam_ema), inside optimizer_ref.F32_ERR = 4.0 / 1.5e-7 / 2.0e-7
"""
from collections import OrderedDict

import numpy as np

from tests import optimizer_ref as O

f32 = O.f32
OUTPUTS = ("p", "m", "v", "ema")
F32_ERR_DECOUPLED = {"p": 4.0, "m": 1.5e-7, "v": 2.0e-7}
F32_ERR_EMA = 5.0
TOL_COUPLED = dict(O.TOL)
TOL_DECOUPLED = {k: 16.0 * e for k, e in F32_ERR_DECOUPLED.items()}
TOL_EMA = 16.0 * F32_ERR_EMA


def tol(case):
    """{output: tolerance} of a case: p / m / v of its path, ema when the case has one."""
    t = dict(TOL_DECOUPLED if case["decoupled"] else TOL_COUPLED)
    if case["d"] is not None:
        t["ema"] = TOL_EMA
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# The committed case list.  `d`: the EMA decay, None = no EMA buffer (ema = NULL).  `clip` as in optimizer_ref.
# ---------------------------------------------------------------------------------------------------------------------------
NS = (1, 255, 257, 4099, 1048576 + 777)             # the last is above the 4096-block grid cap
DECAYS = (0.0, 0.5, 0.999, 0.9999, 11.0 / 20.0)
WDS = (0.0, 1e-6, 0.1)
CLIPS = O.CLIPS
STEPS = (1, 2, 1000)


def _case(name, n, decoupled, d, clip="active", wd=1e-6, step=1000, lr=1e-3, grad_scale=1.0, seed=0):
    base = O._case(name, n, clip=clip, grad_scale=grad_scale, wd=wd, step=step, lr=lr, seed=seed)[1]
    return name, dict(base, decoupled=int(decoupled), d=d)


CASES = OrderedDict(
    [_case(f"n{n}_adamw_ema", n, 1, 0.999) for n in NS] +
    [_case(f"n{n}_adam_ema", n, 0, 0.9999, step=2) for n in NS[:-1]] +
    [_case("big_adam_ema", NS[-1], 0, 0.5, clip="inactive", wd=0.1, step=1, grad_scale=0.5),
     _case("big_adamw", NS[-1], 1, None, clip="none", wd=0.1, step=2)] +
    [_case(f"dec{dec}_d{d}", 4099, dec, d, step=2) for dec in (0, 1) for d in (None,) + DECAYS] +
    [_case(f"dec{dec}_wd{wd}_{c}", 4099, dec, 0.999, clip=c, wd=wd, step=2, grad_scale=0.5)
     for dec in (0, 1) for wd in WDS for c in CLIPS] +
    [_case(f"dec{dec}_step{s}_d{d}", 257, dec, d, step=s, wd=0.1) for dec in (0, 1) for s in STEPS for d in (0.0, 0.9999)])


def make_inputs(case):
    """optimizer_ref.make_inputs(case) plus ema: float32 [n], p * (1 + u 2^-3) with a generator of its own."""
    inp = O.make_inputs(case)
    rng = np.random.default_rng(9100 + 17 * case["n"] + case["seed"])
    u = rng.uniform(-1.0, 1.0, case["n"])
    inp["ema"] = (inp["p"].astype(np.float64) * (1.0 + u * 2.0 ** -3)).astype(np.float32)
    assert np.array_equal(np.sign(inp["ema"]), np.sign(inp["p"])) and not inp["ema"][inp["pad"]].any()
    return inp


def ema_step(ema, p_new, d, dtype=np.float64):
    """ema + (1 - d) (p' - ema) in `dtype`; p_new is already of that dtype."""
    f = dtype
    e = np.asarray(ema, dtype=np.float32).astype(f)
    return e + (f(1.0) - f(f32(d))) * (np.asarray(p_new, dtype=f) - e)


def adam_opt_step(p, g, m, v, ss, max_norm, lr, wd, step, grad_scale=1.0, decoupled=0, ema=None, d=None, beta1=O.BETA1, beta2=O.BETA2,
                  eps=O.EPS, dtype=np.float64):
    """One t2_adam_step_opt on float32 arrays -> dict(p, m, v, ratio, clip[, ema]) in `dtype`."""
    f = dtype
    assert decoupled in (0, 1) and (d is None) == (ema is None)
    if ss is not None and not np.isfinite(ss):
        out = O.adam_clip_step(p, g, m, v, ss, max_norm, lr, wd, step, grad_scale, beta1, beta2, eps, dtype)
        if d is not None:
            out["ema"] = np.asarray(ema, dtype=np.float32).astype(f)
        return out
    if not decoupled:
        out = O.adam_clip_step(p, g, m, v, ss, max_norm, lr, wd, step, grad_scale, beta1, beta2, eps, dtype)
    else:
        p, g, m, v = (np.asarray(x, dtype=np.float32).astype(f) for x in (p, g, m, v))
        b1, b2, lr_, eps_, wd_, gs = (f(f32(x)) for x in (beta1, beta2, lr, eps, wd, grad_scale))
        bc1, bc2 = f(1.0 - f32(beta1) ** step), f(1.0 - f32(beta2) ** step)
        clip = O.clip_coef(ss, max_norm, grad_scale, f)
        gr = g * (clip * gs)
        m2 = b1 * m + (f(1.0) - b1) * gr
        v2 = b2 * v + (f(1.0) - b2) * gr * gr
        ratio = (m2 / bc1) / (np.sqrt(v2 / bc2) + eps_)
        p2 = p * (f(1.0) - lr_ * wd_) - lr_ * ratio
        assert all(x.dtype == f for x in (p2, m2, v2, ratio))
        out = dict(p=p2, m=m2, v=v2, ratio=ratio, clip=clip)
    if d is not None:
        out["ema"] = ema_step(ema, out["p"], d, f)
        assert out["ema"].dtype == f
    return out


def reference(case, inp, dtype=np.float64):
    return adam_opt_step(inp["p"], inp["g"], inp["m"], inp["v"], inp["ss"], decoupled=case["decoupled"],
                         ema=inp["ema"] if case["d"] is not None else None, d=case["d"], dtype=dtype, **O.step_kwargs(case))


def ema_error(got, ema_in, ref_p, ref_ema, d):
    """The largest deviation of got from the float64 ref_ema in units of 2^-24 (|ema| + (1 - d) |p' - ema|)."""
    e0 = np.asarray(ema_in, dtype=np.float64)
    diff = np.abs(np.asarray(got, dtype=np.float64) - ref_ema)
    unit = 2.0 ** -24 * (np.abs(e0) + (1.0 - f32(d)) * np.abs(ref_p - e0))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(unit > 0.0, diff / unit, np.where(diff == 0.0, 0.0, np.inf))
    return float(np.max(e, initial=0.0))


def errors(got, ref, case, inp):
    """{output: largest per-element deviation of got from the float64 `ref` in the output's unit}; ema when the case has one."""
    out = O.errors(got, ref, case["lr"])
    if case["d"] is not None:
        out["ema"] = ema_error(got["ema"], inp["ema"], ref["p"], ref["ema"], case["d"])
    return out


def measure_f32_err(cases=None):
    """{"coupled" | "decoupled": {p, m, v: (deviation, case)}, "ema": (deviation, case)}: the float32 run's largest deviation from the
    float64 run over CASES."""
    worst = {"coupled": {k: (0.0, None) for k in O.OUTPUTS}, "decoupled": {k: (0.0, None) for k in O.OUTPUTS}, "ema": (0.0, None)}
    for name, case in (cases or CASES).items():
        inp = make_inputs(case)
        e = errors(reference(case, inp, np.float32), reference(case, inp), case, inp)
        path = worst["decoupled" if case["decoupled"] else "coupled"]
        for k in O.OUTPUTS:
            if e[k] > path[k][0]:
                path[k] = (e[k], name)
        if "ema" in e and e["ema"] > worst["ema"][0]:
            worst["ema"] = (e["ema"], name)
    return worst
