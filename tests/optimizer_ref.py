"""Reference for the kernel-level tests of the update: a float64 numpy restatement of t2_sumsq followed by t2_adam_step as
include/tacotron2_amd.h defines them, with the dtype as a parameter - float64 is the reference, float32 only yields the tolerances.
CPU only, no torch (tests/test_optimizer_ref_host.py checks the restatement against oracle.tacotron2_ref, tests/test_gpu_optimizer.py
checks the kernels against the restatement).

    tot  = sqrt(sumsq) * grad_scale
    clip = min(1, max_norm / (tot + 1e-6))      # 1 when max_norm <= 0 or sumsq is None
    g'   = g * clip * grad_scale + wd * p
    m'   = b1 m + (1 - b1) g'
    v'   = b2 v + (1 - b2) g'^2
    p'   = p - lr * (m' / (1 - b1^step)) / (sqrt(v' / (1 - b2^step)) + eps)
A sumsq that is not finite leaves p, m and v as they are.

The ABI takes beta1, beta2, lr, eps, wd, max_norm and grad_scale as float.  The reference uses the float32-ROUNDED value of each as
its hyper-parameter, in float64 (f32): 1 - b2 is then exact and the same number in the kernel and here, and 0.999f - 0.999 is a
1.3e-8 change of a hyper-parameter, not an error.  So is the 1e-6 of the clip (1e-6f in the kernel).  The bias corrections
1 - b^step are formed in float64 from those values in BOTH runs and rounded once to the run's dtype: the float32 run measures the
rounding of the per-element arithmetic, not of powf (the factor 16 has to cover that, see Tolerances).

Inputs (make_inputs), all float32, seeded per case:
    p ~ N(0, 1), g = +-2^e * [1, 2) with e uniform in -14 .. -3 (binades 2^-14 .. 2^-2), scaled by ONE factor k per case so that
    tot = sqrt(sumsq) * grad_scale has the case's ratio to max_norm (16: the clip is active; 0.3: it is not).  One element in 16
    has g = p = 0 (the flat buffer's alignment padding: m = v = 0 too), one in 16 g = 0 alone, one in 16 p = 0 alone.  Where
    both are non-zero g takes p's sign, so that g' = g clip grad_scale + wd p cannot cancel: m and v are judged per element
    relative to |ref|, and the one element of the list with the closest cancellation would otherwise set both constants (a
    float32 rounding of g' divided by an arbitrarily small sum).  m and v are what two steps under the same g' leave from zero,
    m = (1 - b1^2) g', v = (1 - b2^2) g'^2, rounded to float32: no v that underflows in float32, where the two precisions
    legitimately part, and no cancellation between m and g'.  The step number of a case is independent of that history.

Metrics (errors): m and v per element |got - ref| / (|ref| + TINY); p per element in units of 2^-24 (|p_ref| + lr |update ratio|),
update ratio = mhat / (sqrt(vhat) + eps) - half a float32 ulp of the two terms p' is formed from, so that a small parameter is not
hidden behind a large one (where the unit is 0 - padding - anything but equality is infinite).

Tolerances: TOL = 16 x F32_ERR per output, F32_ERR = the float32 run's largest deviation from the float64 run over the committed
case list (measure_f32_err; tests/test_optimizer_ref_host.py re-measures it and holds the constant to [measured, 2 x measured]).
Never from a kernel's output.  The factor 16 - the project's convention for kernels held to a float32 restatement
(tests/decode_chain_ref.py) - covers the kernel's own order of operations and contractions: mv / bc1, sqrtf(vv / bc2), fused
multiply-adds, and the bias corrections as 1 - powf(beta, step) in float32.  The last is most of it: powf(0.999f, 2) is rounded to
24 bits and the difference is 0.002, a relative error of 6.7e-6 in bc2, which is 57 of p's units where p_ref = 0
(test_optimizer_ref_host.py::test_float32_bias_corrections_stay_inside_the_tolerance works it out for every step).

Measured (CPU, numpy, over CASES and GRID; worst case n1049353 for all three), and the largest deviation of the kernels on one
MI355X (tests/test_gpu_optimizer.py):
    p  3.80 units of 2^-24 (|p_ref| + lr |ratio|)   F32_ERR 4.0      TOL 64        kernel 58.3 (step 2; 6.2 at every other step)
    m  1.41e-7 relative                              F32_ERR 1.5e-7   TOL 2.4e-6    kernel 1.39e-7
    v  1.86e-7 relative                              F32_ERR 2.0e-7   TOL 3.2e-6    kernel 1.84e-7
"""
import itertools
import math
from collections import OrderedDict

import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
TINY = 2.0 ** -100
OUTPUTS = ("p", "m", "v")
F32_ERR = {"p": 4.0, "m": 1.5e-7, "v": 2.0e-7}
TOL = {k: 16.0 * e for k, e in F32_ERR.items()}


def f32(x):
    """The float the ABI hands to the kernel, as a Python float."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------
# The committed case list.  `clip`: "active" tot = 16 max_norm, "inactive" tot = 0.3 max_norm, "off" max_norm = 0, "none"
# sumsq = NULL, "tiny" an active clip at max_norm = 1e-5 with tot = 1.6e-4, where the 1e-6 of the denominator is 0.6 % of it (at
# tot = 16 it is one float32 ulp and nothing would notice its absence).
# ---------------------------------------------------------------------------------------------------------------------------
NS = (1, 255, 257, 100003, 1048576 + 777)           # the last is above both grid caps: 4096 blocks (Adam), 1024 (t2_sumsq)
CLIPS = ("active", "inactive", "off", "none")
GRAD_SCALES = (1.0, 0.5, 0.125)
WDS = (0.0, 1e-6, 0.1)
STEPS = (1, 2, 10, 1000, 100000)
LRS = (1e-3, 1e-5)


def _case(name, n, clip="active", grad_scale=1.0, wd=1e-6, step=10, lr=1e-3, seed=0):
    assert clip in CLIPS + ("tiny",)
    max_norm = {"off": 0.0, "tiny": 1e-5}.get(clip, 1.0)
    return name, dict(name=name, n=n, clip=clip, max_norm=max_norm, grad_scale=grad_scale, wd=wd, step=step, lr=lr, seed=seed)


CASES = OrderedDict(
    [_case(f"n{n}", n) for n in NS] +
    [_case(f"clip_{c}", 100003, clip=c, grad_scale=0.5, wd=0.1, step=2) for c in CLIPS] +
    [_case(f"gs{gs}_{c}", 4099, clip=c, grad_scale=gs) for gs in GRAD_SCALES for c in ("active", "inactive")] +
    [_case(f"wd{wd}", 100003, wd=wd, clip="inactive", step=1000) for wd in WDS] +
    [_case(f"step{s}", 100003, step=s, grad_scale=0.125) for s in STEPS] +
    [_case(f"lr{lr}", 100003, lr=lr, step=1, wd=0.1) for lr in LRS] +
    [_case("big_inactive", NS[-1], clip="inactive", wd=0.1, step=2, lr=1e-5, grad_scale=0.5),
     _case("big_none", NS[-1], clip="none", wd=0.0, step=100000, grad_scale=0.125),
     _case("tiny_norm", 257, clip="tiny"), _case("tiny_norm_gs", 100003, clip="tiny", grad_scale=0.125, step=2)])
# every combination of the six axes' other values at one size of two blocks with a tail of one element
GRID = OrderedDict(_case(f"grid_{c}_{gs}_{wd}_{s}_{lr}", 257, clip=c, grad_scale=gs, wd=wd, step=s, lr=lr)
                   for c, gs, wd, s, lr in itertools.product(CLIPS, GRAD_SCALES, WDS, STEPS, LRS))


def sumsq(g):
    """The exactly rounded sum of the squares of float32 values (each square is exact in double)."""
    return math.fsum((np.asarray(g, dtype=np.float64) ** 2).tolist())


def clip_coef(ss, max_norm, grad_scale, dtype=np.float64):
    """min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6)); 1 without a sumsq or with max_norm <= 0."""
    f = dtype
    if ss is None or not f32(max_norm) > 0.0:
        return f(1.0)
    tot = f(math.sqrt(ss)) * f(f32(grad_scale))
    c = f(f32(max_norm)) / (tot + f(f32(1e-6)))
    return c if c < 1.0 else f(1.0)


def adam_clip_step(p, g, m, v, ss, max_norm, lr, wd, step, grad_scale=1.0, beta1=BETA1, beta2=BETA2, eps=EPS, dtype=np.float64):
    """One t2_adam_step on float32 arrays under the gradient norm ss = sumsq(whole gradient buffer) or None ->
    dict(p, m, v, ratio, clip) in `dtype`.  ratio is the update ratio mhat / (sqrt(vhat) + eps)."""
    f = dtype
    assert step >= 1
    p, g, m, v = (np.asarray(x, dtype=np.float32).astype(f) for x in (p, g, m, v))
    if ss is not None and not math.isfinite(ss):
        return dict(p=p, m=m, v=v, ratio=np.zeros_like(p), clip=f(0.0))
    b1, b2, lr_, eps_, wd_, gs = (f(f32(x)) for x in (beta1, beta2, lr, eps, wd, grad_scale))
    bc1, bc2 = f(1.0 - f32(beta1) ** step), f(1.0 - f32(beta2) ** step)        # float64, rounded once (module docstring)
    clip = clip_coef(ss, max_norm, grad_scale, f)
    gr = g * (clip * gs) + wd_ * p
    m2 = b1 * m + (f(1.0) - b1) * gr
    v2 = b2 * v + (f(1.0) - b2) * gr * gr
    ratio = (m2 / bc1) / (np.sqrt(v2 / bc2) + eps_)
    p2 = p - lr_ * ratio
    assert all(x.dtype == f for x in (p2, m2, v2, ratio))
    return dict(p=p2, m=m2, v=v2, ratio=ratio, clip=clip)


def make_inputs(case, seed=None):
    """dict(p, g, m, v: float32 [n]; ss: sumsq(g) or None for the call; ss_g: sumsq(g) always; pad: the padding elements)."""
    n = case["n"]
    rng = np.random.default_rng(7000 + 13 * n + (case["seed"] if seed is None else seed))
    p = rng.standard_normal(n)
    mag = np.ldexp(1.0 + rng.random(n), rng.integers(-14, -2, n))                  # 2^-14 <= |g0| < 2^-2
    kind = rng.integers(0, 16, n)
    if n > 1:
        kind[0] = 15
    else:
        kind[:] = 15
    pad, g_zero, p_zero = kind == 0, kind == 1, kind == 2
    p[pad | p_zero] = 0.0
    p = p.astype(np.float32)
    sign = np.where(p != 0.0, np.sign(p), np.where(rng.random(n) < 0.5, -1.0, 1.0))
    g0 = (sign * mag).astype(np.float32)
    g0[pad | g_zero] = 0.0
    # ONE factor for the whole gradient, from the reference norm: tot = ratio * max_norm (max_norm = 0 / no sumsq: as if it were 1)
    ratio = {"active": 16.0, "tiny": 16.0, "inactive": 0.3, "off": 16.0, "none": 16.0}[case["clip"]]
    target = ratio * (case["max_norm"] if case["max_norm"] > 0.0 else 1.0)
    k = target / (math.sqrt(sumsq(g0)) * case["grad_scale"])
    g = (g0.astype(np.float64) * k).astype(np.float32)
    ss_g = sumsq(g)
    ss = None if case["clip"] == "none" else ss_g
    # the moments two steps under one g' leave from zero
    gr = g.astype(np.float64) * float(clip_coef(ss, case["max_norm"], case["grad_scale"])) * f32(case["grad_scale"]) \
        + f32(case["wd"]) * p.astype(np.float64)
    m = ((1.0 - f32(BETA1) ** 2) * gr).astype(np.float32)
    v = ((1.0 - f32(BETA2) ** 2) * gr * gr).astype(np.float32)
    assert not np.any((v == 0.0) & (gr != 0.0)) and float(np.abs(v[v > 0]).min(initial=1.0)) > 2.0 ** -100
    return dict(p=p, g=g, m=m, v=v, ss=ss, ss_g=ss_g, pad=pad)


def step_kwargs(case):
    return {k: case[k] for k in ("max_norm", "lr", "wd", "step", "grad_scale")}


def reference(case, inp, dtype=np.float64):
    return adam_clip_step(inp["p"], inp["g"], inp["m"], inp["v"], inp["ss"], dtype=dtype, **step_kwargs(case))


def errors(got, ref, lr):
    """{output: largest per-element deviation of got from the float64 `ref` (adam_clip_step's dict) in the output's unit}."""
    out = {}
    for k in ("m", "v"):
        r = ref[k]
        out[k] = float(np.max(np.abs(np.asarray(got[k], dtype=np.float64) - r) / (np.abs(r) + TINY), initial=0.0))
    diff = np.abs(np.asarray(got["p"], dtype=np.float64) - ref["p"])
    unit = 2.0 ** -24 * (np.abs(ref["p"]) + f32(lr) * np.abs(ref["ratio"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(unit > 0.0, diff / unit, np.where(diff == 0.0, 0.0, np.inf))
    out["p"] = float(np.max(e, initial=0.0))
    return out


def measure_f32_err(cases=None):
    """{output: (largest deviation of the float32 run from the float64 run, case name)} over CASES and GRID."""
    worst = {k: (0.0, None) for k in OUTPUTS}
    for name, case in (cases or OrderedDict(list(CASES.items()) + list(GRID.items()))).items():
        inp = make_inputs(case)
        e = errors(reference(case, inp, np.float32), reference(case, inp), case["lr"])
        for k in OUTPUTS:
            if e[k] > worst[k][0]:
                worst[k] = (e[k], name)
    return worst
