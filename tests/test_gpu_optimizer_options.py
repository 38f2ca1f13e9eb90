"""t2_adam_step_opt (csrc/t2_elementwise.hip) called through the C ABI on the case list of tests/optimizer_options_ref.py and
compared with its float64 restatement: decoupled weight decay on and off, the EMA off and on at five decays, three weight decays, the
four clip kinds, steps 1 / 2 / 1000, sizes from one element to above the grid cap.  Then the exact identities: the coupled path is
t2_adam_step bit for bit, with and without the EMA; the EMA's fixed point (padding, ema == p', and d = 0 wherever p' - ema is exact);
a non-finite norm changes none of the five buffers; sub-range calls on odd offsets are the single call; rejected calls launch
nothing.  And Trainer at the mid-size dims: all options off is the Trainer without the argument, the EMA leaves the live weights
alone and follows the float64 recursion, swap_ema twice is the identity, a frozen tensor's shadow is its parameter.

p, g, m, v and ema live in buffers with 8 NaN sentinels in front of and behind the n elements; the sentinels must survive every call.
Metrics and tolerances: optimizer_options_ref.errors / tol (16 x the float32 restatement's own error, measured on the CPU,
tests/test_optimizer_options_host.py).  Every test prints "[optimizer-options] <case>: <output> <deviation> /<TOL> ..." and then
asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tacotron2_ref as R  # noqa: E402
from tests import optimizer_options_ref as OR  # noqa: E402
from tests import optimizer_ref as O  # noqa: E402
from tests.test_gpu_reduction_factor import MID  # noqa: E402

PAD = 8
KEYS = ("p", "g", "m", "v", "ema")


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
            case = OR.CASES[name]
            inp = OR.make_inputs(case)
            for x in inp.values():
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
            cache[name] = (case, inp, OR.reference(case, inp))
        return cache[name]
    return get


def _st():
    return torch.cuda.current_stream().cuda_stream


def _t(a):
    return torch.from_numpy(np.array(a))       # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Bufs:
    """Device copies of p, g, m, v, ema with PAD NaN sentinels on both sides, and the float64 word of the norm (pre-filled with 7)."""

    def __init__(self, dev, inp, ema=None):
        self.n = len(inp["p"])
        self.t = {}
        for k in KEYS:
            x = torch.full((self.n + 2 * PAD,), float("nan"), device=dev)
            x[PAD:PAD + self.n] = torch.from_numpy(np.array(ema if (k == "ema" and ema is not None) else inp[k])).to(dev)
            self.t[k] = x
        self.ss = torch.full((1,), 7.0, dtype=torch.float64, device=dev)

    def ptr(self, k, off=0):
        return self.t[k].data_ptr() + 4 * (PAD + off)

    def sumsq(self):
        from tacotron2_amd import _lib
        _lib.call("t2_sumsq", self.ptr("g"), self.n, self.ss, _st())

    def struct(self, case, a=0, b=None, ss="own", **over):
        from tacotron2_amd import _lib
        b = self.n if b is None else b
        kw = dict(p=self.ptr("p", a), g=self.ptr("g", a), m=self.ptr("m", a), v=self.ptr("v", a), n=b - a,
                  sumsq=self.ss if ss == "own" else ss, max_norm=float(case["max_norm"]), lr=float(case["lr"]), beta1=O.BETA1,
                  beta2=O.BETA2, eps=O.EPS, weight_decay=float(case["wd"]), step=int(case["step"]), grad_scale=float(case["grad_scale"]),
                  ema=self.ptr("ema", a) if case["d"] is not None else None, ema_decay=float(case["d"] or 0.0),
                  decoupled=int(case["decoupled"]))
        kw.update(over)
        return _lib.make("T2AdamOpt", **kw)

    def step(self, case, a=0, b=None, ss="own", fn=None, **over):
        from tacotron2_amd import _lib
        return (fn or _lib.call)("t2_adam_step_opt", self.struct(case, a, b, ss, **over), _st())

    def plain_step(self, case, ss="own"):
        from tacotron2_amd import _lib
        _lib.call("t2_adam_step", self.ptr("p"), self.ptr("g"), self.ptr("m"), self.ptr("v"), self.n, self.ss if ss == "own" else ss,
                  float(case["max_norm"]), float(case["lr"]), O.BETA1, O.BETA2, O.EPS, float(case["wd"]), int(case["step"]),
                  float(case["grad_scale"]), _st())

    def out(self):
        """dict(p, g, m, v, ema) of the n elements on the CPU; the sentinels must be intact."""
        torch.cuda.synchronize()
        res = {}
        for k in KEYS:
            x = self.t[k].cpu()
            assert bool(torch.isnan(x[:PAD]).all() and torch.isnan(x[PAD + self.n:]).all()), f"{k}: a sentinel was overwritten"
            res[k] = x[PAD:PAD + self.n]
        return res


def _use(inp):
    return "own" if inp["ss"] is not None else None


def _run(dev, case, inp, ema=None):
    b = Bufs(dev, inp, ema=ema)
    if inp["ss"] is not None:
        b.sumsq()
    b.step(case, ss=_use(inp))
    return b.out()


def _unchanged(got, inp, keys=KEYS):
    for k in keys:
        assert torch.equal(_bits(got[k]), _bits(_t(inp[k]))), k


def _figure(name, case, inp, ref, got):
    tol = OR.tol(case)
    e = OR.errors({k: got[k].double().numpy() for k in tol}, ref, case, inp)
    print(f"[optimizer-options] {name}: " + " ".join(f"{k} {e[k]:.3g} /{tol[k]:.3g}" for k in tol))
    assert torch.equal(_bits(got["g"]), _bits(_t(inp["g"])))               # the gradient is read only
    # alignment padding (p = g = m = v = ema = 0) keeps its parameter, and its shadow stays bit-equal to it
    pad = torch.from_numpy(np.nonzero(inp["pad"])[0])
    assert torch.equal(_bits(got["p"])[pad], _bits(_t(inp["p"]))[pad]), f"{name}: padding moved"
    if case["d"] is None:
        assert torch.equal(_bits(got["ema"]), _bits(_t(inp["ema"]))), f"{name}: ema = NULL, yet the ema buffer changed"
    else:
        assert torch.equal(_bits(got["ema"])[pad], _bits(got["p"])[pad]), f"{name}: the padding's shadow left its parameter"
    return e, tol


@pytest.mark.parametrize("name", list(OR.CASES))
def test_step_matches_the_float64_restatement(dev, refs, name):
    case, inp, ref = refs(name)
    e, tol = _figure(name, case, inp, ref, _run(dev, case, inp))
    for k in tol:
        assert e[k] <= tol[k], (name, k, e[k], tol[k])


@pytest.mark.parametrize("name", ["n1_adam_ema", "n257_adam_ema", "big_adam_ema", "dec0_dNone", "dec0_d0.0", "dec0_d0.999",
                                  "dec0_wd0.1_active", "dec0_wd0.1_inactive", "dec0_wd0.1_off", "dec0_wd0.1_none", "dec0_step1_d0.9999",
                                  "dec0_step1000_d0.0"])
def test_coupled_path_is_t2_adam_step_bit_for_bit(dev, refs, name):
    """decoupled = 0: p, m and v after t2_adam_step_opt are those of t2_adam_step on the same inputs, bit for bit - with the case's
    EMA, and with ema = NULL (the very kernel)."""
    case, inp, _ = refs(name)
    assert case["decoupled"] == 0
    plain = Bufs(dev, inp)
    if inp["ss"] is not None:
        plain.sumsq()
    plain.plain_step(case, ss=_use(inp))
    want = plain.out()
    assert not torch.equal(_bits(want["p"]), _bits(_t(inp["p"])))
    for c in (case, dict(case, d=None)):
        got = _run(dev, c, inp)
        for k in O.OUTPUTS:
            assert torch.equal(_bits(got[k]), _bits(want[k])), (name, c["d"], k, int((_bits(got[k]) != _bits(want[k])).sum()))
        if c["d"] is None:
            assert torch.equal(_bits(got["ema"]), _bits(_t(inp["ema"])))
        else:
            assert not torch.equal(_bits(got["ema"]), _bits(_t(inp["ema"]))) or case["n"] == 1


@pytest.mark.parametrize("name", ["n4099_adamw_ema", "n4099_adam_ema", "dec1_d0.5", "dec0_d0.55", "big_adam_ema"])
def test_ema_equal_to_the_new_parameter_is_a_fixed_point(dev, refs, name):
    """With the ema input set to p' itself (the bits a first call produced), ema' == p' bit for bit at any decay: p' - ema is exactly 0
    and ema + w * 0 is ema.  What keeps a tensor that does not move, and the padding, equal to its parameter."""
    case, inp, _ = refs(name)
    first = _run(dev, case, inp)
    got = _run(dev, case, inp, ema=first["p"].numpy())
    assert torch.equal(_bits(got["p"]), _bits(first["p"]))
    assert torch.equal(_bits(got["ema"]), _bits(got["p"])), int((_bits(got["ema"]) != _bits(got["p"])).sum())


@pytest.mark.parametrize("name", ["dec0_d0.0", "dec1_d0.0", "dec0_step1_d0.0", "dec1_step1000_d0.0"])
def test_decay_zero_copies_the_parameter(dev, refs, name):
    """d = 0: ema' = ema + (p' - ema).  Wherever ema / 2 <= p' <= 2 ema (same sign) the difference is exact (Sterbenz) and so is the
    sum: ema' == p' bit for bit.  The inputs keep ema within 2^-3 of p, so that is all but the elements a step moves by more than half
    their size; those are held to the tolerance by the restatement test."""
    case, inp, _ = refs(name)
    assert case["d"] == 0.0
    got = _run(dev, case, inp)
    e0, p1 = _t(inp["ema"]).double(), got["p"].double()
    exact = ((e0 >= 0) == (p1 >= 0)) & (p1.abs() >= e0.abs() / 2) & (p1.abs() <= 2 * e0.abs())
    exact |= (e0 == 0)                       # 0 + (p' - 0) is p'
    assert int(exact.sum()) >= 0.9 * case["n"], (int(exact.sum()), case["n"])
    assert torch.equal(_bits(got["ema"])[exact], _bits(got["p"])[exact]), int((_bits(got["ema"]) != _bits(got["p"]))[exact].sum())


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), float("-inf")])
@pytest.mark.parametrize("name", ["n4099_adamw_ema", "n4099_adam_ema"])
def test_non_finite_norm_changes_none_of_the_five_buffers(dev, refs, name, bad):
    case, inp, _ = refs(name)
    b = Bufs(dev, inp)
    b.ss.fill_(bad)
    b.step(case)
    _unchanged(b.out(), inp)


@pytest.mark.parametrize("name", ["n4099_adamw_ema", "dec0_d0.5"])
def test_sub_range_calls_are_the_single_call(dev, refs, name):
    """One buffer of n = 4099 split at the element offsets 0, 1, 258, 1027, n into four calls on offset pointers under ONE shared
    sumsq - what Engine.adam_step(ranges=...) does: all five buffers bit-identical to the single call.  With the second range left
    out its p, m, v and ema are untouched."""
    case, inp, _ = refs(name)
    n = case["n"]
    cuts = [0, 1, 258, 1027, n]
    whole = Bufs(dev, inp); whole.sumsq(); whole.step(case)
    parts = Bufs(dev, inp); parts.sumsq()
    holed = Bufs(dev, inp); holed.sumsq()
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        parts.step(case, a, b)
        if i != 1:
            holed.step(case, a, b)
    gw, gp, gh = whole.out(), parts.out(), holed.out()
    hole = slice(cuts[1], cuts[2])
    for k in ("p", "m", "v", "ema"):
        assert torch.equal(_bits(gp[k]), _bits(gw[k])), k
        before = _bits(_t(inp[k]))
        assert torch.equal(_bits(gh[k])[hole], before[hole]), k
        assert not torch.equal(_bits(gw[k])[hole], before[hole]), k
        assert torch.equal(_bits(gh[k])[:cuts[1]], _bits(gw[k])[:cuts[1]]) and torch.equal(_bits(gh[k])[cuts[2]:], _bits(gw[k])[cuts[2]:]), k


def test_argument_errors_launch_nothing(dev, refs):
    """Every refusal of the header is T2_ERR_ARG before any launch: all five buffers keep their bits.  n = 0 is T2_OK without one."""
    from tacotron2_amd import _lib
    case, inp, _ = refs("n257_adamw_ema")
    b = Bufs(dev, inp)
    b.sumsq()
    cv = _lib.call_value
    bad = [dict(step=0), dict(step=-3), dict(n=-1), dict(decoupled=2), dict(decoupled=-1),
           dict(ema_decay=1.0), dict(ema_decay=1.5), dict(ema_decay=-0.125), dict(ema_decay=float("nan")), dict(ema_decay=float("inf")),
           dict(ema=b.ptr("p")), dict(ema=b.ptr("p", 256)), dict(ema=b.ptr("p") - 4 * 256), dict(ema=b.ptr("g")), dict(ema=b.ptr("m", 3)),
           dict(ema=b.ptr("v", 100))]
    bad += [{k: None} for k in "pgmv"]
    for over in bad:
        assert b.step(case, fn=cv, **over) == 1, over
        assert "t2_adam_step_opt" in _lib.lib().t2_last_error().decode()
    assert cv("t2_adam_step_opt", None, _st()) == 1
    with pytest.raises(_lib.T2Error, match="rc=1"):
        b.step(case, decoupled=2)
    # without an ema buffer its decay is not read; and n = 0 is a success that launches nothing
    assert b.step(case, fn=cv, n=0) == 0
    assert b.step(dict(case, d=None), fn=cv, n=0, ema_decay=7.0) == 0
    _unchanged(b.out(), inp)
    assert float(b.ss.cpu()) == pytest.approx(inp["ss_g"], rel=1e-12)
    # buffers that merely touch are no overlap: ema directly behind p
    n = 64
    blk = torch.zeros(2 * n, device=dev)
    z = torch.zeros(n, device=dev)
    st = _lib.make("T2AdamOpt", p=blk.data_ptr(), g=z, m=torch.zeros_like(z), v=torch.zeros_like(z), n=n, sumsq=None, max_norm=1.0,
                   lr=1e-3, beta1=O.BETA1, beta2=O.BETA2, eps=O.EPS, weight_decay=0.0, step=1, grad_scale=1.0,
                   ema=blk.data_ptr() + 4 * n, ema_decay=0.5, decoupled=1)
    assert cv("t2_adam_step_opt", st, _st()) == 0
    torch.cuda.synchronize()
    assert not bool(blk.any())


# ---------------------------------------------------------------------------------------------------------------------------
# Trainer at the mid-size dims
# ---------------------------------------------------------------------------------------------------------------------------
def _train(dev, steps=3, frozen=None, record=False, replay=None, **trainer_kw):
    """A fresh store with seeded weights, `steps` steps on one seeded batch (the engine's own Philox masks: a function of the seed and
    the step) -> (trainer, [flat before the first and after each step, on the CPU], [the gradient buffer each update consumed]).
    replay: gradient buffers of another run; each step's own gradient is replaced by them in front of the update.  A full step is not
    bit-reproducible from run to run - the split-K and weight-gradient sums of the backward use atomics, DESIGN.md section 9 - so two
    trainers can only be compared bit for bit when both updates consume the same gradient bits: the forward and the backward still
    run, on the same batch and masks, and everything from Trainer.train_step's call of Engine.adam_step on is the trainer's own."""
    from tacotron2_amd.trainer import Trainer
    from tests.test_gpu_model import build_engine, random_case
    d = R.default_dims(**MID)
    _, ps = build_engine(d, R.init_params(d, seed=9), dev)
    tr = Trainer(ps, lr=1e-3, weight_decay=1e-2, scheduler_milestones=(2,), **trainer_kw)
    if frozen:
        tr.frozen = {frozen}
    ci, lens, mel, tl, gate, _ = random_case(d, 4, 21, 13, 7, None)
    batch = dict(chars_idx=ci.to(dev), chars_idx_len=lens.to(dev), mel_spectrogram=mel.to(dev), mel_spectrogram_len=tl.to(dev),
                 gate=gate.to(dev))
    grads = []
    inner = tr.engine.adam_step

    def adam_step(*a, **kw):
        if replay is not None:
            ps.grad.copy_(replay[len(grads)])
        grads.append(ps.grad.clone())
        return inner(*a, **kw)
    tr.engine.adam_step = adam_step
    rec = [ps.flat.cpu().clone()] if record else []
    for _ in range(steps):
        tr.train_step(batch)
        torch.cuda.synchronize()
        if record:
            rec.append(ps.flat.cpu().clone())
    tr.engine.check_persistent_kernels()
    assert len(grads) == steps
    return tr, rec, grads


@pytest.fixture(scope="module")
def plain_run(dev):
    """The Trainer built without the argument: its weights and first moments after three steps and the three gradient buffers its
    updates consumed (shared, read only)."""
    tr, _, grads = _train(dev)
    return tr.ps.flat.cpu().clone(), tr.ps.exp_avg.cpu().clone(), grads


def test_trainer_with_all_options_off_is_the_trainer_without_them(dev, plain_run):
    """Three chained steps on the same batch, masks and gradient bits (see _train): the weights and moments are those of the Trainer
    built without the argument, bit for bit.  A second Trainer without the argument is the control for the replay itself."""
    from tacotron2_amd.options import OptimizerOptions
    for kw in ({}, dict(optimizer_options=OptimizerOptions()), dict(optimizer_options={})):
        tr, _, _ = _train(dev, replay=plain_run[2], **kw)
        assert tr.ps.ema is None and tr.ema_updates == 0
        assert torch.equal(_bits(tr.ps.flat.cpu()), _bits(plain_run[0])), kw
        assert torch.equal(_bits(tr.ps.exp_avg.cpu()), _bits(plain_run[1])), kw


def test_trainer_ema_leaves_the_live_weights_and_follows_the_recursion(dev, plain_run):
    """EMA on (D = 0.999, so the three updates run under the ramp 2/11, 3/12, 4/13), on the plain run's gradient bits (_train): the
    live weights are the plain run's bits; the
    shadow is the float64 recursion over the three recorded p' from ema_0 = p_0, within the ema tolerance after every step's unit;
    swap_ema twice is the identity, once exchanges."""
    from tacotron2_amd.options import ema_decay_at
    tr, rec, _ = _train(dev, record=True, replay=plain_run[2], optimizer_options=dict(ema_decay=0.999))
    ps = tr.ps
    assert tr.ema_updates == 3
    assert torch.equal(_bits(ps.flat.cpu()), _bits(plain_run[0])), "the EMA changed the live weights"
    ema = rec[0].double().numpy()            # init_ema: the shadow starts as the weights
    for k in (1, 2, 3):
        d = ema_decay_at(0.999, k)
        assert d == (1.0 + k) / (10.0 + k)
        prev, p1 = ema, rec[k].double().numpy()
        ema = prev + (1.0 - O.f32(d)) * (p1 - prev)
    worst = OR.ema_error(ps.ema.cpu().double().numpy(), prev, p1, ema, d)         # in the unit of the last update
    print(f"[optimizer-options] trainer ema after 3 steps ({ps.numel} elements): ema {worst:.3g} /{OR.TOL_EMA:.3g}")
    assert worst <= OR.TOL_EMA
    assert not torch.equal(ps.ema, ps.flat)
    f0, e0 = ps.flat.clone(), ps.ema.clone()
    ptrs = (ps.flat.data_ptr(), ps.ema.data_ptr(), ps.P["prenet.0.weight"].data_ptr())
    ps.swap_ema()
    assert torch.equal(_bits(ps.flat), _bits(e0)) and torch.equal(_bits(ps.ema), _bits(f0))
    ps.swap_ema()
    assert torch.equal(_bits(ps.flat), _bits(f0)) and torch.equal(_bits(ps.ema), _bits(e0))
    assert ptrs == (ps.flat.data_ptr(), ps.ema.data_ptr(), ps.P["prenet.0.weight"].data_ptr())


def test_trainer_frozen_tensor_keeps_its_shadow_equal_to_its_parameter(dev):
    frozen = "encoder.convolutions.4.weight"
    tr, rec, _ = _train(dev, frozen=frozen, record=True, optimizer_options=dict(ema_decay=0.9, decoupled_weight_decay=True, grad_clip=0.5))
    ps = tr.ps
    a = ps.offsets[frozen]
    b = a + ps.P[frozen].numel()
    assert torch.equal(_bits(ps.flat[a:b].cpu()), _bits(rec[0][a:b]))
    assert torch.equal(_bits(ps.ema[a:b]), _bits(ps.flat[a:b]))
    assert not torch.equal(ps.ema[:a], ps.flat[:a]) and not torch.equal(ps.flat[:a].cpu(), rec[0][:a])
    # the alignment padding between tensors: zero in both
    names = list(ps.offsets)
    for i, name in enumerate(names[:-1]):
        end = ps.offsets[name] + ps.P[name].numel()
        assert not bool(ps.flat[end:ps.offsets[names[i + 1]]].any()) and not bool(ps.ema[end:ps.offsets[names[i + 1]]].any())


def test_trainer_decoupled_decay_and_schedule_reach_the_kernel(dev, plain_run):
    """AdamW with wd = 1e-2 and a warm-up must move the weights differently from the plain run, and lr_at is what the step used: a
    warm-up of 3 steps runs step 1 at lr / 3, so its first update is a third of the plain run's (Adam's first step is lr * sign)."""
    tr, rec, _ = _train(dev, steps=1, record=True, optimizer_options=dict(decoupled_weight_decay=True, warmup_steps=3, grad_clip=0.0))
    assert tr.lr_at(0) == pytest.approx(1e-3 / 3) and tr.max_norm == 0.0
    delta = (rec[1].double() - rec[0].double() * (1.0 - O.f32(1e-3 / 3) * O.f32(1e-2))).abs()
    # |update| = lr |g| / (|g| + eps): at most lr, and within 1 % of it wherever |g| >= 100 eps = 1e-6
    lr = 1e-3 / 3
    assert float(delta.max()) <= lr * 1.001
    assert int(((delta - lr).abs() <= 0.01 * lr).sum()) >= 0.1 * delta.numel()
    assert not torch.equal(_bits(rec[1]), _bits(plain_run[0]))
