"""t2_sumsq and t2_adam_step (csrc/t2_elementwise.hip) called through the C ABI on the case list of tests/optimizer_ref.py and
compared with its float64 restatement: the clip active, inactive, switched off (max_norm = 0) and without a norm (sumsq = NULL),
grad_scale 1 / 0.5 / 0.125, three weight decays, steps 1 .. 100000 in the bias corrections, two learning rates, sizes from one
element to above both grid caps; then what no tolerance can state - the exact identities: padding keeps its parameter, a power-of-two
grad_scale commutes with the step, sub-range calls on odd element offsets are the single call, a non-finite norm changes nothing,
rejected calls launch nothing - and Engine.adam_step with a frozen tensor at mid-size dims.

p, m and v live in buffers with 8 NaN sentinels in front of and behind the n elements; the sentinels must survive every call.
Metrics and tolerances: optimizer_ref.errors / TOL (16 x the float32 restatement's own error, tests/test_optimizer_ref_host.py).
Every test prints "[optimizer] <case>: p <units> /<TOL> m <rel> /<TOL> v <rel> /<TOL>" and then asserts.

Measured on one MI355X (worst case per output; the whole module, 50 tests, takes 2 s):
                                   p /64                        m /2.4e-6    v /3.2e-6
    CASES, every step but 2        6.24 (n1049353)              1.39e-7      1.84e-7
    CASES at step 2                58.3 (step2)                 1.33e-7      1.76e-7
    GRID (360 cases, n = 257)      30.2 (active, step 2)        1.09e-7      1.41e-7
    Engine.adam_step, step 1 / 2   4.01 / 60.0                  2.23e-7      3.92e-7
    t2_sumsq                       relative error at most 4.4e-16 (n = 100003; bound 1.1e-11)
Step 2 carries the float32 rounding of 1 - powf(0.999f, 2), 57 units where p_ref = 0 (tests/optimizer_ref.py, Tolerances).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tacotron2_ref as R  # noqa: E402
from tests import optimizer_ref as O  # noqa: E402
from tests.test_gpu_reduction_factor import MID  # noqa: E402

PAD = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def refs():
    """{case name: (case, inputs, float64 reference)} - computed once per case, shared, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            case = O.CASES.get(name) or O.GRID[name]
            inp = O.make_inputs(case)
            for x in inp.values():
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
            cache[name] = (case, inp, O.reference(case, inp))
        return cache[name]
    return get


def _st():
    return torch.cuda.current_stream().cuda_stream


def _t(a):
    return torch.from_numpy(np.array(a))       # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Bufs:
    """Device copies of p, g, m, v with PAD NaN sentinels on both sides, and the float64 word of the norm (pre-filled with 7)."""

    def __init__(self, dev, inp, g=None):
        self.n = len(inp["p"])
        self.t = {}
        for k in "pgmv":
            x = torch.full((self.n + 2 * PAD,), float("nan"), device=dev)
            x[PAD:PAD + self.n] = torch.from_numpy(np.array(g if (k == "g" and g is not None) else inp[k])).to(dev)
            self.t[k] = x
        self.ss = torch.full((1,), 7.0, dtype=torch.float64, device=dev)

    def ptr(self, k, off=0):
        return self.t[k].data_ptr() + 4 * (PAD + off)

    def sumsq(self):
        from tacotron2_amd import _lib
        _lib.call("t2_sumsq", self.ptr("g"), self.n, self.ss, _st())

    def step(self, case, a=0, b=None, ss="own", fn=None):
        from tacotron2_amd import _lib
        b = self.n if b is None else b
        fn = fn or _lib.call
        return fn("t2_adam_step", self.ptr("p", a), self.ptr("g", a), self.ptr("m", a), self.ptr("v", a), b - a,
                  self.ss if ss == "own" else ss, float(case["max_norm"]), float(case["lr"]), O.BETA1, O.BETA2, O.EPS, float(case["wd"]),
                  int(case["step"]), float(case["grad_scale"]), _st())

    def out(self):
        """dict(p, m, v) of the n elements on the CPU; the sentinels must be intact."""
        torch.cuda.synchronize()
        res = {}
        for k in "pgmv":
            x = self.t[k].cpu()
            assert bool(torch.isnan(x[:PAD]).all() and torch.isnan(x[PAD + self.n:]).all()), f"{k}: a sentinel was overwritten"
            res[k] = x[PAD:PAD + self.n]
        return res


def _run(dev, case, inp):
    b = Bufs(dev, inp)
    if inp["ss"] is not None:
        b.sumsq()
    b.step(case, ss="own" if inp["ss"] is not None else None)
    return b.out()


def _figure(name, case, inp, ref, got):
    e = O.errors({k: got[k].double().numpy() for k in O.OUTPUTS}, ref, case["lr"])
    print(f"[optimizer] {name}: " + " ".join(f"{k} {e[k]:.3g} /{O.TOL[k]:.3g}" for k in O.OUTPUTS))
    # alignment padding, and every other element with nothing to move it, keeps its parameter bit for bit
    still = (inp["g"] == 0) & (inp["m"] == 0) & (inp["v"] == 0) & ((inp["p"] == 0) | (case["wd"] == 0.0))
    assert int(still.sum()) >= int(inp["pad"].sum())
    idx = torch.from_numpy(np.nonzero(still)[0])
    assert torch.equal(_bits(got["p"])[idx], _bits(_t(inp["p"]))[idx]), f"{name}: padding moved"
    assert not bool(got["m"][idx].any() or got["v"][idx].any())
    assert torch.equal(_bits(got["g"]), _bits(_t(inp["g"])))               # the gradient is read only
    return e


@pytest.mark.parametrize("n", O.NS)
def test_sumsq_is_the_exact_sum_to_n_roundings(dev, n):
    """t2_sumsq against math.fsum of the float64 squares: the squares of float32 values are exact in double, so only the additions
    round - relative error at most n 2^-53.  It overwrites its output (pre-filled with 7) and a second call does not accumulate."""
    from tacotron2_amd import _lib
    inp = O.make_inputs(O.CASES[f"n{n}"])
    b = Bufs(dev, inp)
    for _ in range(2):
        b.sumsq()
        torch.cuda.synchronize()
        got = float(b.ss.cpu())
        rel = abs(got - inp["ss_g"]) / inp["ss_g"]
        print(f"[optimizer] sumsq n={n}: relative error {rel:.3g} /{n * 2.0 ** -53:.3g}")
        assert rel <= n * 2.0 ** -53
    # a gradient of zeros (the frozen tensors' share): exactly 0, not 7
    z = torch.zeros(n, device=dev)
    _lib.call("t2_sumsq", z, n, b.ss, _st())
    torch.cuda.synchronize()
    assert float(b.ss.cpu()) == 0.0
    b.out()


@pytest.mark.parametrize("name", list(O.CASES))
def test_step_matches_the_float64_restatement(dev, refs, name):
    case, inp, ref = refs(name)
    e = _figure(name, case, inp, ref, _run(dev, case, inp))
    for k in O.OUTPUTS:
        assert e[k] <= O.TOL[k], (name, k, e[k], O.TOL[k])


def test_grid_matches_the_float64_restatement(dev, refs):
    """All 360 combinations of clip mode x grad_scale x weight decay x step x learning rate at n = 257."""
    worst = {k: (0.0, None) for k in O.OUTPUTS}
    for name in O.GRID:
        case, inp, ref = refs(name)
        got = _run(dev, case, inp)
        e = O.errors({k: got[k].double().numpy() for k in O.OUTPUTS}, ref, case["lr"])
        for k in O.OUTPUTS:
            if e[k] > worst[k][0]:
                worst[k] = (e[k], name)
    print("[optimizer] grid, worst: " + " ".join(f"{k} {worst[k][0]:.3g} /{O.TOL[k]:.3g} ({worst[k][1]})" for k in O.OUTPUTS))
    for k in O.OUTPUTS:
        assert worst[k][0] <= O.TOL[k], (k, worst[k])


@pytest.mark.parametrize("name", ["gs0.5_active", "gs0.5_inactive", "gs0.125_active", "gs0.125_inactive", "clip_off", "clip_none",
                                  "step1", "tiny_norm_gs", "big_inactive"])
def test_power_of_two_grad_scale_commutes_with_the_step(dev, refs, name):
    """A step on (g, grad_scale = s) equals, bit for bit, the step on (s g, grad_scale = 1) with its own t2_sumsq, s = 0.5 and 0.125:
    a power-of-two factor commutes with every rounding of the norm, the clip and the gradient.  A grad_scale that reaches the gradient
    but not the norm, or either of them twice, breaks this."""
    case, inp, _ = refs(name)
    s = case["grad_scale"]
    assert s in (0.5, 0.125)
    a = Bufs(dev, inp)
    scaled = inp["g"] * np.float32(s)
    assert np.array_equal(scaled.astype(np.float64), inp["g"].astype(np.float64) * s)      # exact: no underflow
    b = Bufs(dev, inp, g=scaled)
    use = "own" if inp["ss"] is not None else None
    if use:
        a.sumsq(); b.sumsq()
    a.step(case, ss=use)
    b.step(dict(case, grad_scale=1.0), ss=use)
    ga, gb = a.out(), b.out()
    if use:
        assert float(b.ss.cpu()) == pytest.approx(float(a.ss.cpu()) * s * s, rel=1e-12)
    for k in O.OUTPUTS:
        assert torch.equal(_bits(ga[k]), _bits(gb[k])), (name, k, int((_bits(ga[k]) != _bits(gb[k])).sum()))
    assert not torch.equal(_bits(ga["p"]), _bits(_t(inp["p"])))


def test_sub_range_calls_are_the_single_call(dev, refs):
    """One buffer of n = 100003 split at the element offsets 0, 1, 4099, 65537, n into four t2_adam_step calls on offset pointers
    under ONE shared sumsq - what Engine.adam_step(ranges=...) does: bit-identical to the single call.  With the second range left
    out its p, m and v are untouched bit for bit and its neighbours are what they are in the single call."""
    name = "clip_active"
    case, inp, ref = refs(name)
    n = case["n"]
    cuts = [0, 1, 4099, 65537, n]
    whole = Bufs(dev, inp); whole.sumsq(); whole.step(case)
    parts = Bufs(dev, inp); parts.sumsq()
    holed = Bufs(dev, inp); holed.sumsq()
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        parts.step(case, a, b)
        if i != 1:
            holed.step(case, a, b)
    gw, gp, gh = whole.out(), parts.out(), holed.out()
    e = _figure(name + " (single call)", case, inp, ref, gw)
    assert all(e[k] <= O.TOL[k] for k in O.OUTPUTS)
    hole = slice(cuts[1], cuts[2])
    for k in O.OUTPUTS:
        assert torch.equal(_bits(gp[k]), _bits(gw[k])), k
        before = _bits(_t(inp[k]))
        assert torch.equal(_bits(gh[k])[hole], before[hole]), k
        assert not torch.equal(_bits(gw[k])[hole], before[hole])
        assert torch.equal(_bits(gh[k])[:cuts[1]], _bits(gw[k])[:cuts[1]]) and torch.equal(_bits(gh[k])[cuts[2]:], _bits(gw[k])[cuts[2]:]), k


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), float("-inf")])
def test_non_finite_norm_skips_the_step(dev, refs, bad):
    case, inp, _ = refs("n100003")
    b = Bufs(dev, inp)
    b.ss.fill_(bad)
    b.step(case)
    got = b.out()
    for k in "pgmv":
        assert torch.equal(_bits(got[k]), _bits(_t(inp[k]))), k


def test_argument_errors_launch_nothing(dev, refs):
    """step = 0 and a NULL p, g, m or v are T2_ERR_ARG before any launch: every buffer keeps its bits."""
    from tacotron2_amd import _lib
    case, inp, _ = refs("n257")
    b = Bufs(dev, inp)
    b.sumsq()
    assert b.step(dict(case, step=0), fn=_lib.call_value) == 1
    assert b.step(dict(case, step=-3), fn=_lib.call_value) == 1
    assert "t2_adam_step" in _lib.lib().t2_last_error().decode()
    for k in "pgmv":
        ptrs = {j: (None if j == k else b.ptr(j)) for j in "pgmv"}
        rc = _lib.call_value("t2_adam_step", ptrs["p"], ptrs["g"], ptrs["m"], ptrs["v"], b.n, b.ss, 1.0, 1e-3, O.BETA1, O.BETA2, O.EPS,
                             0.0, 1, 1.0, _st())
        assert rc == 1, k
    assert _lib.call_value("t2_sumsq", None, b.n, b.ss, _st()) == 1 and _lib.call_value("t2_sumsq", b.ptr("g"), b.n, None, _st()) == 1
    with pytest.raises(_lib.T2Error, match="rc=1"):
        b.step(dict(case, step=0))
    got = b.out()
    for k in "pgmv":
        assert torch.equal(_bits(got[k]), _bits(_t(inp[k]))), k
    assert float(b.ss.cpu()) == pytest.approx(inp["ss_g"], rel=1e-12)


def test_engine_adam_step_with_a_frozen_tensor(dev):
    """Engine.adam_step at the mid-size dims over Trainer.trainable_ranges() with one encoder tensor frozen, two steps (step 1 from
    zero moments with grad_scale 1, step 2 on the moments it left with grad_scale 0.5): the frozen tensor, its moments (set to
    sentinels) and its gradient are bit-identical before and after; every other element, the alignment padding included, is within
    TOL of the restatement fed the same flat buffers and the exact norm.  The gradient has optimizer_ref's binades, the sign of its
    parameter and zeros where the parameter is zero (the padding), so that g' cannot cancel (optimizer_ref's docstring); weight
    decay 1e-6 keeps wd p a 500th of the smallest clipped gradient, so a parameter that crosses zero in step 1 changes nothing."""
    from tacotron2_amd.trainer import Trainer
    from tests.test_gpu_model import build_engine
    d = R.default_dims(**MID)
    eng, ps = build_engine(d, R.init_params(d, seed=9), dev)
    tr = Trainer(ps, lr=1e-3, weight_decay=1e-6)
    frozen = "encoder.convolutions.4.weight"
    tr.frozen = {frozen}
    ranges = tr.trainable_ranges()
    fa = ps.offsets[frozen]
    fb = fa + ps.P[frozen].numel()
    assert fa % 4 == 0 and len(ranges) == 2 and ranges[0] == (0, fa) and ranges[1][1] == ps.numel and fb <= ranges[1][0] < fb + 4
    n = ps.numel
    p0 = ps.flat.cpu().numpy().copy()
    rng = np.random.default_rng(11)
    g0 = (np.sign(p0) * np.ldexp(1.0 + rng.random(n), rng.integers(-14, -2, n))).astype(np.float32)
    g0[rng.integers(0, 16, n) == 0] = 0.0
    train = np.zeros(n, dtype=bool)
    for a, b in ranges:
        train[a:b] = True
    assert int((~train).sum()) == fb - fa and int((p0[train] == 0).sum()) > 0
    ps.init_adam()
    ps.exp_avg.zero_(); ps.exp_avg_sq.zero_()
    ps.exp_avg[fa:fb] = 0.25; ps.exp_avg_sq[fa:fb] = 0.5
    for step, gs in ((1, 1.0), (2, 0.5)):
        g = g0.copy() if step == 1 else np.roll(g0, 4) * np.float32(np.sign(np.roll(p0, 4)) * np.sign(p0))
        g[~train] = 0.0                                   # Trainer.train_step zeroes the frozen gradients: the norm excludes them
        g = (g.astype(np.float64) * (16.0 / (math.sqrt(O.sumsq(g)) * gs))).astype(np.float32)
        ps.grad.copy_(torch.from_numpy(g))
        torch.cuda.synchronize()
        before = {k: t.cpu().numpy().copy() for k, t in (("p", ps.flat), ("m", ps.exp_avg), ("v", ps.exp_avg_sq))}
        kw = dict(max_norm=1.0, lr=1e-3, wd=1e-6, step=step, grad_scale=gs)
        ss = eng.adam_step(step, kw["lr"], kw["wd"], kw["max_norm"], grad_scale=gs, ranges=ranges)
        torch.cuda.synchronize()
        exact = O.sumsq(g)
        assert abs(float(ss.cpu()) - exact) <= n * 2.0 ** -53 * exact
        ref = O.adam_clip_step(before["p"], g, before["m"], before["v"], exact, **kw)
        got = {"p": ps.flat.cpu().numpy(), "m": ps.exp_avg.cpu().numpy(), "v": ps.exp_avg_sq.cpu().numpy()}
        for k in O.OUTPUTS:
            assert np.array_equal(got[k][fa:fb].view(np.int32), before[k][fa:fb].view(np.int32)), (step, k)
        assert float(ps.exp_avg[fa]) == 0.25 and float(ps.exp_avg_sq[fb - 1]) == 0.5
        e = O.errors({k: got[k][train].astype(np.float64) for k in O.OUTPUTS}, {k: v[train] for k, v in ref.items() if k != "clip"}, kw["lr"])
        print(f"[optimizer] engine step {step} ({n} elements, {fb - fa} frozen, clip {float(ref['clip']):.4f}): "
              + " ".join(f"{k} {e[k]:.3g} /{O.TOL[k]:.3g}" for k in O.OUTPUTS))
        assert not np.array_equal(got["p"][train], before["p"][train])
        for k in O.OUTPUTS:
            assert e[k] <= O.TOL[k], (step, k, e[k])
