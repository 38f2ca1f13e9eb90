"""Engine.forward_tf / backward_tf under stream skew (tests/stream_skew.py, DESIGN.md section 5 "Stream skew") against float64.

Every case: one engine; the delay D measured on an engine of its own (median of 3 unskewed steps after a warm-up, HIP events on the
main stream, rounded up to 100 us, D <= the probe's 50 000); one unskewed PRIMING step on other inputs (another seed, L + 2, T + 2:
every shared workspace then holds plausible stale values, and none is re-allocated by the step under test); then the step under
test with one stream held back by D in front of every launch, its outputs, losses and ps.grad cloned on the main stream behind it,
and compared after the synchronise with the float64 reference under the bounds of the test the case comes from.  Each test first
asserts that the two streams do run side by side (ensure_concurrent_streams) - on one hardware queue the harness proves nothing -
and that no launch of the step went to a third stream.  A failing comparison prints the trace's edges and the launch counts.

test_dropped_edge_is_detected is the harness's own proof: with ONE wait skipped (stream_skew.drop_wait) the same comparison must fail.

Timing (profiles/stream_skew_timing.txt, written from the SKEW-TIMING lines these tests print): an unskewed step takes 3.7-4.9 ms (host-bound),
D is 3700-4900 us, a step has ~100 library calls on each stream, a skewed step takes 0.4-0.5 s of wall time and three of them 1.4 s."""
import functools
import math
import time
from typing import NamedTuple, Optional

import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_skew as SK  # noqa: E402
from oracle import tacotron2_ref as R  # noqa: E402
from tests import forward_attention_chain_ref as F  # noqa: E402
from tests import reduction_ref as RR  # noqa: E402
from tests import zoneout_ref as Z  # noqa: E402
from tests.helpers import dekink_masks  # noqa: E402
from tests.test_gpu_model import _dev, _grad_check, build_engine, masks_to_device, random_case  # noqa: E402
from tests.test_guided_attention_host import guided_ref  # noqa: E402

# the dimensions of tests/test_gpu_model.py::test_pipeline_chunking_matches_oracle
DIMS = dict(num_chars=39, encoded_dim=64, prenet_dim=32, att_rnn_dim=64, att_dim=32, rnn_hidden_dim=64, postnet_dim=64, num_mels=16,
            dropout=0.5)
B0, L0, T0 = 5, 17, 12            # six chunks each way at chunk = chunk_bwd = 2, wgrad_group = 2 (tests/test_stream_skew_host.py)
PSEED = 11
GUIDED = (0.4, 100.0)             # tests/test_gpu_guided_attention.py::test_loss_and_grads_with_the_guided_term_matches_the_oracle
N_DEFERRED = 6                    # tests/test_stream_skew_host.py asserts the schedules at this count
POLICIES = {"slow-side": lambda: SK.slow("side"), "slow-main": lambda: SK.slow("main"), "seeded-1": lambda: SK.seeded(1),
            "seeded-2": lambda: SK.seeded(2), "seeded-3": lambda: SK.seeded(3)}
BOTH = ["slow-side", "slow-main"]


class Inputs(NamedTuple):
    ci: torch.Tensor
    lens: torch.Tensor
    mel: torch.Tensor
    tl: torch.Tensor
    gate: torch.Tensor
    masks: dict                       # oracle convention, float32, CPU
    zones: Optional[dict] = None      # zone masks [S][B][H]
    ctl: Optional[torch.Tensor] = None
    spk: Optional[torch.Tensor] = None


class Case(NamedTuple):
    kind: str
    d: dict                           # the engine's dims
    P: dict                           # float32 parameters, reference layout
    x: Inputs
    prime: Inputs                     # the priming step's inputs
    o: tuple                          # float64 reference outputs (mels, post, gates, alignments), detached
    loss3: torch.Tensor               # float64 (gate, mel, post)
    guided: Optional[float]           # the fourth term, when the case has one
    grads: dict
    fkw: dict = {}                    # forward_tf keywords beside the inputs


def _cast64(P):
    return {k: (v.double().clone().requires_grad_(True) if (v.is_floating_point() and not R.is_buffer(k)) else
                (v.double().clone() if v.is_floating_point() else v.clone())) for k, v in P.items()}


def _m64(m):
    return {k: ([x.double() for x in v] if isinstance(v, list) else v.double()) for k, v in m.items()}


def _grads(Pc, total):
    names = [k for k, v in Pc.items() if v.requires_grad]
    gs = torch.autograd.grad(total, [Pc[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(Pc[k]) if g is None else g) for k, g in zip(names, gs)}


def _inputs(d, P, B, L, T, seed, r=1, zones=False, controls=False):
    """random_case with the ReLU-kink elements dropped from both sides (dekink_masks), cut to steps for r > 1 as
    tests/test_gpu_zoneout.py::_train_case does, plus what the option under test needs."""
    ci, lens, mel, tl, gate, masks = random_case(d, B, L, T, seed, None)
    packed = mel
    if r > 1:
        from tests.test_gpu_reduction_factor import _step_masks
        if all(int(x) % r == 0 for x in tl):
            tl[0] -= 1
            mel[0, tl[0]:] = 0.0; gate[0, tl[0] - 1:] = 0.0
        masks = _step_masks(masks, T, r)
        packed = torch.stack([mel[:, i] if i is not None else torch.zeros(B, d["num_mels"]) for i in RR.teacher_slots(T, r)], 1)
    masks, _ = dekink_masks(P, d, ci, packed, masks)
    zn = ctl = spk = None
    S = RR.steps_of(T, r)
    if zones:
        g = torch.Generator().manual_seed(seed + 7)       # drawn at 0.3: the few steps hold plenty of both values
        zn = {k: (torch.rand(S, B, d["att_rnn_dim"] if k.startswith("att") else d["rnn_hidden_dim"], generator=g) < 0.3).float()
              for k in Z.ZONE_KEYS}
    if controls:
        g = torch.Generator().manual_seed(seed + 1)
        ctl = torch.randn(B, d["controls_dim"], generator=g)
        spk = torch.randint(0, d["num_speakers"], (B,), generator=g, dtype=torch.int32)
    return Inputs(ci, lens, mel, tl, gate, masks, zn, ctl, spk)


@functools.lru_cache(maxsize=None)
def _case(kind, B=B0, L=L0, T=T0, seed=77):
    """The float64 reference of one step, computed once per process and left unchanged.  kind: "plain" (R.tacotron2_fwd), "fa+guided"
    (forward_attention_chain_ref.model_fa + the guided term), "zoneout" (zoneout_ref.model_fwd, r = 2), "controls"."""
    d = R.default_dims(**DIMS, **(dict(controls=True, controls_dim=5, speaker_tokens=True, num_speakers=4) if kind == "controls" else {}))
    r = 2 if kind == "zoneout" else 1
    P = RR.grouped_params(R.init_params(d, seed=PSEED), d, r, seed=seed)
    kw = dict(r=r, zones=kind == "zoneout", controls=kind == "controls")
    x = _inputs(d, P, B, L, T, seed, **kw)
    prime = _inputs(d, P, B, L + 2, T + 2, seed + 1000, **kw)
    Pc = _cast64(P)
    mel64, gate64 = x.mel.double(), x.gate.double()
    guided, fkw, dims = None, {}, d
    if kind == "fa+guided":
        # (model_fa makes its own float64 copy of the parameters: the gradients are with respect to THAT copy)
        Pc, o, _ = F.model_fa(P, d, (x.ci, x.lens, x.mel, x.tl, x.gate, x.masks), torch.float64)
        fkw = dict(forward_attention=True)
    elif kind == "zoneout":
        o = Z.model_fwd(Pc, d, r, x.ci, x.lens, True, mel=mel64, mel_len=x.tl, training=True, masks=_m64(x.masks), new_stats={},
                        zones=x.zones)
        dims = dict(d, reduction_factor=r, zoneout=0.1)
    else:
        o = R.tacotron2_fwd(Pc, d, x.ci, x.lens, True, mel64, x.tl, training=True, masks=_m64(x.masks), new_stats={},
                            controls=x.ctl.double() if x.ctl is not None else None, speaker_id=x.spk)
    tot, bce, ml, pl = R.tts_loss(o[0], o[1], o[2], mel64, gate64)
    if kind == "fa+guided":
        gl = guided_ref(o[3], x.lens, x.tl, *GUIDED)[0]
        tot, guided = tot + gl, float(gl.detach())
    grads = _grads(Pc, tot)
    return Case(kind, dims, P, x, prime, tuple(t.detach() for t in o), torch.stack([bce, ml, pl]).detach(), guided, grads, fkw)


# ---- the device side --------------------------------------------------------------------------------------------------------------
def _configure(eng, dec_chain="persistent"):
    eng.chunk, eng.chunk_bwd, eng.wgrad_group, eng.dec_chain = 2, 2, 2, dec_chain
    return eng


def _upload(x, dev):
    """Everything a step reads, on the device BEFORE the step: an upload inside it would synchronise the host with the main stream."""
    masks = masks_to_device(x.masks, dev)
    if x.zones is not None:
        masks.update({k: v.to(dev).contiguous() for k, v in x.zones.items()})
    kw = {}
    if x.ctl is not None:
        kw.update(controls=x.ctl.to(dev), speaker_id=x.spk.to(dev))
    return dict(args=(x.ci.to(dev), x.lens.to(dev), x.mel.to(dev), x.tl.to(dev)), mel=x.mel.to(dev), gate=x.gate.to(dev), masks=masks, kw=kw)


def _step(eng, ps, u, fkw, guided=None):
    outs, ctx = eng.forward_tf(*u["args"], training=True, masks=u["masks"], **u["kw"], **fkw)
    ps.grad.zero_()
    loss3 = eng.loss_and_grads(outs, ctx, u["mel"], u["gate"], guided=guided)
    return outs, loss3, ctx


def _snapshot(eng, ps, outs, loss3):
    """Clones on the main stream, enqueued behind the step: what a consumer on that stream would read."""
    return dict(outs=[t.clone() for t in outs], loss3=loss3.clone(), grad=ps.grad.clone(), flat=ps.flat.clone(),
                guided=eng.guided_loss.clone() if eng.guided_loss is not None else None)


def _measure_delay(make_step, dev):
    """D: the whole unskewed step on an engine of its own, HIP events on the main stream; median of 3 after one warm-up, rounded up
    to 100 us.  Sufficient without analysing the schedule: in D the fast stream finishes everything the edges allow."""
    step = make_step()
    times = []
    for i in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    med = sorted(times[1:])[1]
    D = int(math.ceil(med / 100.0)) * 100
    assert D <= SK.PROBE_MAX_US, f"the unskewed step takes {med:.0f} us: shrink the case, the probe spins {SK.PROBE_MAX_US} us at most"
    return med, D


def _engine(c, dev, dec_chain="persistent"):
    eng, ps = build_engine(c.d, c.P, dev)
    _configure(eng, dec_chain)
    qc = eng.ensure_concurrent_streams()
    assert qc["ok"], f"the engine's two streams share a hardware queue - the skew proves nothing: {qc}"
    return eng, ps


def _timing_line(label, med, D, sk, wall):
    n = sk.counts()
    print(f"SKEW-TIMING {label}: step {med:.0f} us, D {D} us, launches main {n.get('main', (0, 0))[0]} side {n.get('side', (0, 0))[0]} "
          f"other {n.get('other', (0, 0))[0]}, delayed {sum(k for _, k in n.values())}, skewed step {wall:.2f} s wall")


def _run(monkeypatch, c, policy, dev, label, dec_chain="persistent", drop=None):
    """(engine, ParamStore, snapshot, Skew) of the step under test."""
    u, up = _upload(c.x, dev), _upload(c.prime, dev)

    def timing_step():
        te, tps = build_engine(c.d, c.P, dev)
        _configure(te, dec_chain)
        return lambda: _step(te, tps, u, c.fkw, GUIDED if c.guided is not None else None)
    eng, ps = _engine(c, dev, dec_chain)
    med, D = _measure_delay(timing_step, dev)
    g = GUIDED if c.guided is not None else None
    _step(eng, ps, up, c.fkw, g)                      # priming: unskewed, other inputs
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        sk = SK.skew(mp, eng, policy, D)
        if drop is not None:
            SK.drop_wait(mp, drop)
        t0 = time.perf_counter()
        outs, loss3, ctx = _step(eng, ps, u, c.fkw, g)
        snap = _snapshot(eng, ps, outs, loss3)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    _timing_line(label, med, D, sk, wall)
    assert ctx["persist"] == (dec_chain == "persistent")
    assert not sk.launches("other"), sk.launches("other")
    assert sum(k for _, k in sk.counts().values()) > 0
    return eng, ps, snap, sk


def _compare(c, eng, ps, snap):
    """The assertions of the test the case comes from, on the main-stream clones."""
    eng.check_persistent_kernels()
    outs, o = snap["outs"], c.o
    d64 = lambda a, b: (a.cpu().double() - b.double()).abs()
    for a, b in zip(outs, o):
        assert tuple(a.shape) == tuple(b.shape), (a.shape, b.shape)
    mel_l1, post_l1, al = float(d64(outs[0], o[0]).mean()), float(d64(outs[1], o[1]).mean()), float(d64(outs[3], o[3]).max())
    l3, ref3 = snap["loss3"].cpu(), c.loss3
    print(f"skewed {c.kind}: mel L1 {mel_l1:.2e}, post L1 {post_l1:.2e}, align max-abs {al:.2e}, loss {float(l3.sum()):.6f} "
          f"(reference {float(ref3.sum()):.6f})")
    if c.kind in ("plain", "controls"):              # test_pipeline_chunking_matches_oracle
        assert post_l1 < 1e-4 and mel_l1 < 1e-4
        assert al < 1e-5
        assert abs(float(l3.sum()) - float(ref3.sum())) < 2e-5 * max(1.0, abs(float(ref3.sum())))
    elif c.kind == "fa+guided":                      # test_engine_step_matches_the_float64_restatement + the guided test's four values
        assert mel_l1 < 1e-4 and post_l1 < 1e-4 and al < 5e-5
        got, want = [float(v) for v in l3] + [float(snap["guided"].cpu())], [float(v) for v in ref3] + [c.guided]
        for g_, w_ in zip(got, want):
            assert abs(g_ - w_) < 2e-5 * max(1.0, abs(w_)), (got, want)
        assert abs(sum(got) - sum(want)) < 2e-5 * max(1.0, abs(sum(want)))
    else:                                            # zoneout: test_training_step_against_float64 (reduction factor's _check_outputs)
        assert mel_l1 < 1e-4 and post_l1 < 1e-4 and al < 5e-5
        assert torch.equal(outs[2].cpu() == -1000.0, o[2] == -1000.0)
        assert float(d64(outs[2], o[2]).max()) < 2e-4
        assert torch.allclose(l3, ref3, rtol=1e-5, atol=1e-6), (l3, ref3)
    ps.grad.copy_(snap["grad"])                      # _grad_check reads the ParamStore: give it the main-stream clone
    torch.cuda.synchronize()
    _grad_check(ps, c.grads)


def _checked(c, eng, ps, snap, sk):
    try:
        _compare(c, eng, ps, snap)
    except AssertionError:
        print(sk.report())
        raise


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("dec_chain", ["persistent", "steps"])
def test_plain_step(monkeypatch, dec_chain, policy):
    dev = _dev()
    c = _case("plain")
    eng, ps, snap, sk = _run(monkeypatch, c, POLICIES[policy](), dev, f"plain {dec_chain} {policy}", dec_chain)
    assert sk.edge_string() == EDGES                 # the pattern the sensitivity ordinals below were read from
    # the deferred count, read off the engine's own launches: a convolution's weight gradient ends in t2_unpack_conv_wgrad - the
    # encoder's three run at once, the postnet's are deferred, with the projection's behind them
    unpacks = [e for e in sk.launches() if e[2] == "t2_unpack_conv_wgrad"]
    assert len(unpacks) - 3 + 1 == N_DEFERRED and all(e[1] == "side" for e in unpacks)
    _checked(c, eng, ps, snap, sk)


@pytest.mark.parametrize("policy", BOTH)
def test_two_row_blocks(monkeypatch, policy):
    """B = 35: two 32-row blocks in the persistent launches (the known kink case of test_pipeline_chunking_matches_oracle)."""
    dev = _dev()
    c = _case("plain", B=35)
    _checked(c, *_run(monkeypatch, c, POLICIES[policy](), dev, f"B=35 {policy}"))


@pytest.mark.parametrize("policy", BOTH)
def test_forward_attention_with_the_guided_term(monkeypatch, policy):
    """The d_align path: t2_guided_attn in front of the backward, t2_attn_seq_bwd_forward in the chain."""
    dev = _dev()
    c = _case("fa+guided")
    eng, ps, snap, sk = _run(monkeypatch, c, POLICIES[policy](), dev, f"fa+guided {policy}")
    names = {e[2] for e in sk.launches()}
    assert {"t2_guided_attn", "t2_attn_seq_bwd_forward"} <= names and "dprior" in eng._ws
    _checked(c, eng, ps, snap, sk)


@pytest.mark.parametrize("policy", BOTH)
def test_zoneout_with_two_frames_per_step(monkeypatch, policy):
    """Zoneout 0.1, r = 2, T = 24 frames = 12 steps: the zoned chains and the zoned persistent launch."""
    dev = _dev()
    c = _case("zoneout", T=24)
    eng, ps, snap, sk = _run(monkeypatch, c, POLICIES[policy](), dev, f"zoneout r=2 {policy}")
    names = {e[2] for e in sk.launches()}
    assert {"t2_attn_seq_fwd_zone", "t2_attn_seq_bwd_zone"} <= names and "dhz_dec" in eng._ws and "dhz_att" in eng._ws
    assert sk.edge_string() == EDGES                 # twelve steps: the base shape's schedule
    _checked(c, eng, ps, snap, sk)


@pytest.mark.parametrize("policy", BOTH)
def test_controls(monkeypatch, policy):
    """controls_dim = 5: the cterm copy in front of every pre_dec GEMM and the ctl column sums, all on the side stream."""
    dev = _dev()
    c = _case("controls")
    eng, ps, snap, sk = _run(monkeypatch, c, POLICIES[policy](), dev, f"controls {policy}")
    assert "ctl.dgd_sum" in eng._ws and "ctl.dproj_sum" in eng._ws
    _checked(c, eng, ps, snap, sk)


# ---- three optimisation steps without a host synchronisation ---------------------------------------------------------------------
STEP_SHAPES = ((17, 12), (23, 9), (11, 12))
LR, WD = 1e-3, 1e-6


@functools.lru_cache(maxsize=None)
def _three_inputs():
    d = R.default_dims(**DIMS)
    P = R.init_params(d, seed=PSEED)
    return d, P, _inputs(d, P, B0, L0 + 2, T0 + 2, 1100), [_inputs(d, P, B0, L, T, 100 + n) for n, (L, T) in enumerate(STEP_SHAPES, 1)]


@pytest.mark.parametrize("policy", BOTH)
def test_three_optimisation_steps_without_a_host_synchronisation(monkeypatch, policy):
    """forward, loss_and_grads, adam_step at (L, T) = (17, 12), (23, 9), (11, 12), all three skewed, nothing between them but the
    main-stream clones: step n + 1's forward must not overwrite what step n's side stream still reads, and step n + 1 must see
    step n's parameters."""
    dev = _dev()
    d, P, prime, xs = _three_inputs()
    us = [_upload(x, dev) for x in xs]
    up = _upload(prime, dev)

    def three(eng, ps, snaps=None):
        for n, u in enumerate(us, 1):
            outs, loss3, _ = _step(eng, ps, u, {})
            sumsq = eng.adam_step(n, LR, WD, max_norm=1.0)
            if snaps is not None:
                snaps.append(dict(_snapshot(eng, ps, outs, loss3), sumsq=sumsq.clone()))

    eng, ps = build_engine(d, P, dev)
    _configure(eng)
    qc = eng.ensure_concurrent_streams()
    assert qc["ok"], f"the engine's two streams share a hardware queue - the skew proves nothing: {qc}"
    # D: every step timed on its own (events between the steps, adam_step included: at least the step), the LONGEST one counts
    te, tps = build_engine(d, P, dev)
    _configure(te)
    flat0, times = tps.flat.clone(), [[], [], []]
    for rep in range(4):
        tps.flat.copy_(flat0)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        evs[0].record()
        for n, u in enumerate(us, 1):
            _step(te, tps, u, {})
            te.adam_step(n, LR, WD, max_norm=1.0)
            evs[n].record()
        torch.cuda.synchronize()
        if rep:
            for i in range(3):
                times[i].append(evs[i].elapsed_time(evs[i + 1]) * 1e3)
    med = max(sorted(t)[1] for t in times)
    D = int(math.ceil(med / 100.0)) * 100
    assert D <= SK.PROBE_MAX_US
    ps.init_adam()                                     # (allocation and its fill outside the skewed steps)
    _step(eng, ps, up, {})
    torch.cuda.synchronize()
    snaps = []
    with monkeypatch.context() as mp:
        sk = SK.skew(mp, eng, POLICIES[policy](), D)
        t0 = time.perf_counter()
        three(eng, ps, snaps)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    _timing_line(f"three steps {policy}", med, D, sk, wall)
    assert not sk.launches("other"), sk.launches("other")
    eng.check_persistent_kernels()
    # The oracle side of test_train_step_midsize_matches_oracle, in float64: autograd, the global-norm clip, the Adam restatement
    # (its moments carried from step to step), the same well-conditioned rule and drift bound.  That test puts the device back on
    # the oracle's trajectory after every step, which here would be a host synchronisation between the steps; so it is the ORACLE
    # that is put on the device's trajectory, afterwards: step n is restated from the parameters the device held behind step n - 1
    # (its main-stream clone).  Where Adam's ~lr * sign(g) update followed rounding noise, both sides then still start each step
    # from the same point, and every step's gradients can be held to _grad_check - not only the first one's.
    m_ = v_ = None
    flat_prev = None
    try:
        for n, (snap, x) in enumerate(zip(snaps, xs), 1):
            if flat_prev is not None:
                ps.flat.copy_(flat_prev)
            Pc = _cast64({k: v.cpu() for k, v in ps.state_dict().items()} if flat_prev is not None else P)
            names = [k for k, v in Pc.items() if v.requires_grad]
            if m_ is None:
                m_, v_ = {k: torch.zeros_like(Pc[k]) for k in names}, {k: torch.zeros_like(Pc[k]) for k in names}
            mel64, gate64 = x.mel.double(), x.gate.double()
            o = R.tacotron2_fwd(Pc, d, x.ci, x.lens, True, mel64, x.tl, training=True, masks=_m64(x.masks), new_stats={})
            loss = float(R.tts_loss(o[0], o[1], o[2], mel64, gate64)[0].detach())
            grads = torch.autograd.grad(R.tts_loss(o[0], o[1], o[2], mel64, gate64)[0], [Pc[k] for k in names])
            coef, tot = R.clip_coef(list(grads), 1.0)
            d64 = lambda a, b: (a.cpu().double() - b.detach().double()).abs()
            assert float(d64(snap["outs"][1], o[1]).mean()) < 1e-4, n
            assert float(d64(snap["outs"][3], o[3]).max()) < 1e-5, n
            assert abs(float(snap["loss3"].sum()) - loss) < 2e-5 * max(1.0, abs(loss)), n
            assert abs(float(snap["sumsq"].sqrt()) - tot) < 1e-3 * tot, n
            ps.grad.copy_(snap["grad"]); ps.flat.copy_(snap["flat"])
            torch.cuda.synchronize()
            _grad_check(ps, dict(zip(names, grads)))
            worst = 0.0
            with torch.no_grad():
                for k, g in zip(names, grads):
                    p_new, m_[k], v_[k] = R.adam_l2_step(Pc[k].detach(), g * coef, m_[k], v_[k], n, LR, WD)
                    well = (g.abs() * coef) > 1e-4
                    if bool(well.any()):
                        worst = max(worst, float((ps.P[k].double().cpu() - p_new)[well].abs().max()))
            print(f"three steps {policy}: step {n} loss {loss:.6f}, parameter drift {worst:.2e}")
            assert worst < 2e-6, f"parameter drift after step {n}: {worst}"
            flat_prev = snap["flat"]
    except AssertionError:
        print(sk.report())
        raise


# ---- grad_tail_hook -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", BOTH)
def test_grad_tail_hook_sees_the_final_tail(monkeypatch, policy):
    """The hook clones ps.grad from prenet.0.weight onwards on the stream it is called on (tests/dp_hip_check.py): bit for bit the
    tail of the finished gradient, whichever stream lags."""
    dev = _dev()
    c = _case("plain")
    u, up = _upload(c.x, dev), _upload(c.prime, dev)
    eng, ps = _engine(c, dev)
    tail0 = ps.offsets["prenet.0.weight"]
    seen = []

    def hook():
        assert torch.cuda.current_stream().cuda_stream == eng.side_stream().cuda_stream
        seen.append(ps.grad[tail0:].clone())
    te, tps = build_engine(c.d, c.P, dev)
    _configure(te)
    med, D = _measure_delay(lambda: (lambda: _step(te, tps, u, {})), dev)
    _step(eng, ps, up, {})
    torch.cuda.synchronize()
    eng.grad_tail_hook = hook
    with monkeypatch.context() as mp:
        sk = SK.skew(mp, eng, POLICIES[policy](), D)
        t0 = time.perf_counter()
        outs, loss3, _ = _step(eng, ps, u, {})
        snap = _snapshot(eng, ps, outs, loss3)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    _timing_line(f"grad_tail_hook {policy}", med, D, sk, wall)
    assert len(seen) == 1 and not sk.launches("other")
    try:
        assert torch.equal(seen[0], snap["grad"][tail0:]) and torch.equal(seen[0], ps.grad[tail0:])
        assert float(seen[0].abs().max()) > 0.0
    except AssertionError:
        print(sk.report())
        raise
    _checked(c, eng, ps, snap, sk)


# ---- sensitivity: the harness sees a missing edge ---------------------------------------------------------------------------------
# The base shape's edges, one letter each (stream_skew.Skew.edge_string), read off Engine.forward_tf / backward_tf:
EDGES_FWD = "sMs" + "Re" * 6 + "M"                   # prenet fork / join, the loop's fork, six chunks, the loop's join
EDGES_BWD = "s" + "rER" * 2 + "reER" + "reeER" + "reER" + "reeER" + "eere" + "Es" + "Re" * 4 + "M"
EDGES = EDGES_FWD + EDGES_BWD
# The waits to drop, as (position in EDGES, what it is).  Every one of their consumers reads float data inside an allocated
# workspace (pre_att / p2, dxdec, dpmT, ps.grad): a dropped edge is wrong numbers and nothing else.
DROPS = {
    "fwd-pre_att-join": (1, "M"),                                    # main waits for the side stream's prenet + pre_att GEMMs
    "bwd-chunk0-bptt": (len(EDGES_FWD) + 2, "E"),                    # main waits for chunk 0's decoder BPTT + dxdec GEMM
    "bwd-acc_done": (len(EDGES_FWD) + EDGES_BWD.index("Es"), "E"),   # main waits for dpmT in front of its first reader
    "bwd-final-join": (len(EDGES) - 1, "M"),                         # main waits for the side stream's last weight gradients
}


@pytest.mark.parametrize("edge", list(DROPS))
def test_dropped_edge_is_detected(monkeypatch, edge):
    """The plain step under slow("side") with ONE main-stream wait skipped: the comparison that test_plain_step[persistent-slow-side]
    passes with the edge in place must fail.  None of the four is implied by another edge: each is the only wait of the main stream
    between the side stream's producer and the main stream's consumer."""
    dev = _dev()
    c = _case("plain")
    pos, letter = DROPS[edge]
    assert EDGES[pos] == letter
    n = sum(1 for ch in EDGES[:pos] if ch not in "rR")               # its ordinal among the waits
    eng, ps, snap, sk = _run(monkeypatch, c, SK.slow("side"), dev, f"dropped {edge}", drop=n)
    assert sk.edge_string() == EDGES and sk.dropped == [pos] and sk.wait_ordinals()[n] == pos
    with pytest.raises(AssertionError):
        _compare(c, eng, ps, snap)
