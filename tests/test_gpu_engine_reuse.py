"""ONE engine over many calls - training steps across shapes, training / eval forward / decode interleaved, options toggled between
steps - with every float workspace poisoned before every call (tests/workspace_poison.py, DESIGN.md section 5 "Workspace poison").

Training, `say` and bench.py use one Engine for thousands of calls whose (B, L, T) changes from batch to batch; almost every other GPU
test builds a fresh engine per case, where a missing clear reads the zeros of a fresh allocation.  Here every sequence runs on one
engine with guard_bytes = 0 (so Engine.buf hands out `t[:n]` of the larger earlier tensor), and before every call: the parameters
and BatchNorm statistics are restored (every call has an independent reference), ps.grad is zeroed, every float workspace is filled
with +P or -Q over its whole allocation, and the caching allocator's free blocks are filled too.  Every result is held to the bounds
of the test its case comes from; check_persistent_kernels follows every call.

  (a) seven training steps at TINY dims across row blocks and growing / shrinking shapes (oracle jobs guard_tiny:B-L-T-reuse);
  (b) training step, decodes of two groups and of three utterances with and without the window, eval forward, a forward without
      stashes, another training step - MID dims, references of tests/test_gpu_guarded_edges.py;
  (c) reduction factor 2 with zoneout: plain / forward attention + guided term / other chunks and chain / forward attention alone
      (references of tests/test_gpu_zoneout.py);
  (d) the harness's own proof: with one accumulator left uncleared (workspace_poison.skip_clear) the comparison of (a) must fail
      under poison; what a fresh engine without poison makes of the same omission is printed - the gap this file closes;
  (e) sequence (a) once more with guard bands: every size change reallocates, every band intact after every step.

The figures the tests print (ENGINE-REUSE lines) are recorded in profiles/engine_reuse.txt."""
import functools
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import workspace_poison as WP  # noqa: E402
from oracle import tacotron2_ref as R  # noqa: E402
from tests.helpers import dekink_masks  # noqa: E402
from tests.oracle_jobs import case as job_case, edge_lengths_case, oracle_train  # noqa: E402
from tests.oracle_pool import oracle  # noqa: E402
from tests.test_attention_window_host import windowed_ref  # noqa: E402
from tests.test_gpu_fullsize import _compare_train_step  # noqa: E402
from tests.test_gpu_guarded_edges import GUARD, _paths, decode_case  # noqa: E402
from tests.test_gpu_model import (MEL_L1_TOL, ZERO_GRADIENT_BY_CONSTRUCTION, _dev, build_engine, l1, masks_to_device,  # noqa: E402
                                  mx)

VALUES = {"+P": WP.P_POS, "-Q": WP.Q_NEG}


def _engine(st, dev, guard_bytes=0):
    eng, ps = build_engine(st["d"], st["P"], dev, guard_bytes=guard_bytes)
    eng.guard_bytes = guard_bytes        # explicit: 0 keeps the `t[:n]` reuse path also in a guarded whole-suite run
    assert ps.guard_bytes == guard_bytes
    return eng, ps


def _before_call(eng, ps, dev, P, value, sizes):
    """What every call of a sequence starts from.  value None: nothing is poisoned (the priming step and the fresh engine of (d))."""
    ps.load_state_dict(P)                 # parameters and BatchNorm running statistics: every call has an independent reference
    ps.grad.zero_()
    if value is None:
        return [], []
    names = WP.poison(eng, value)
    WP.dirty_allocator(dev, sizes, value)
    return names


def _sizes(B, L, T, M):
    """Byte sizes of what a call allocates with torch.empty: outputs (B, T, M) x 3, gates, alignments, length vectors; each twice, and
    a few larger blocks for the allocator to split."""
    return [4 * B * T * M] * 4 + [4 * B * T, 4 * B * T * L, 4 * B, 8 * B] * 2 + [1 << 16, 1 << 20, 2 << 20]


def _train_step(eng, ps, dev, st, value, guided=None, **fkw):
    """One poisoned training step of the case `st` on the shared engine: (outs, ctx, loss3, (poisoned, skipped))."""
    ci, lens, mel, tl, gate, masks = st["case"]
    args = (ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev))
    dm = masks_to_device(masks, dev)
    if st.get("zones"):
        dm.update({k: v.to(dev).contiguous() for k, v in st["zones"].items()})
    kw = {k: v.to(dev) for k, v in st.get("kw", {}).items()}
    meld, gated = mel.to(dev), gate.to(dev)
    names = _before_call(eng, ps, dev, st["P"], value, _sizes(ci.shape[0], ci.shape[1], mel.shape[1], mel.shape[2]))
    outs, ctx = eng.forward_tf(*args, training=True, masks=dm, **kw, **fkw)
    loss3 = eng.loss_and_grads(outs, ctx, meld, gated, guided=guided)
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    return outs, ctx, loss3, names


def _grad_worst(ps, grads):
    """(worst error of any parameter gradient relative to its tensor's largest element, its name): _grad_check's measure."""
    worst = (0.0, None)
    for name, g in ps.reference_layout(ps.G).items():
        if name in ZERO_GRADIENT_BY_CONSTRUCTION:
            continue
        ref = torch.as_tensor(grads[name]).double()
        err = float((g.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-3)
        if err > worst[0]:
            worst = (err, name)
    return worst


def _line(seq, label, fig):
    print(f"ENGINE-REUSE {seq} {label}: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()))


def _wall(test, t0):
    print(f"ENGINE-REUSE wall {test}: {time.perf_counter() - t0:.2f} s")


def _print_names(seq, names):
    poisoned, skipped = names
    print(f"ENGINE-REUSE {seq} poisoned ({len(poisoned)}): {' '.join(poisoned)}")
    print(f"ENGINE-REUSE {seq} skipped ({len(skipped)}): {' '.join(skipped)}")


def _check_forward(outs, ref):
    """The output bounds of the training comparison (tests/test_gpu_fullsize.py) for a forward without a backward."""
    fig = dict(mel_l1=l1(outs[0], ref[0]), post_l1=l1(outs[1], ref[1]), mel_max=mx(outs[0], ref[0]), post_max=mx(outs[1], ref[1]),
               align_max=mx(outs[3], ref[3]))
    print("forward: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["mel_l1"] < MEL_L1_TOL and fig["post_l1"] < MEL_L1_TOL
    assert fig["mel_max"] < 1e-3 and fig["post_max"] < 2e-3
    assert fig["align_max"] < 2e-5
    assert ((outs[2].cpu() == -1000.0) == (ref[2] == -1000.0)).all()
    return fig


# ---- the allocator side of the poison ------------------------------------------------------------------------------------------------
def test_dirty_allocator_hands_poisoned_memory_to_the_next_empty():
    """Of five freed blocks of unusual sizes at least one comes back from torch.empty holding the value (in practice all of them):
    without that, Engine.out would still start from whatever the allocator had."""
    dev = _dev()
    counts = [37123, 5003, 291, 70001, 1234567]
    WP.dirty_allocator(dev, [4 * n for n in counts], WP.Q_NEG)
    back = [torch.empty(n, dtype=torch.float32, device=dev) for n in counts]
    torch.cuda.synchronize()
    hit = [bool((t == WP.Q_NEG).all()) for t in back]
    print(f"ENGINE-REUSE allocator: poisoned blocks handed back {sum(hit)} of {len(hit)}")
    assert any(hit), hit


# ---- (a) / (e): training steps across shapes ---------------------------------------------------------------------------------------------
# step: (B, L, T)                what it follows
STEPS = [(33, 21, 12),         # fresh engine; two 32-row persistent blocks; encoder by step launches
         (5, 9, 5),            # everything is a view of a larger tensor; tile pad rows 5..15 held real rows
         (17, 33, 7),          # L grows past anything seen; B spans two 16-row tiles
         (16, 8, 19),          # T grows past anything seen; B is exactly one tile
         (65, 5, 3),           # B above 64: the decoder chain as step launches, a last 64-row block of one row
         (1, 1, 1),            # the minimum
         (33, 21, 12)]         # step 1 again, same inputs
_RUNS = {}                     # poison label -> the sequence's snapshots (for the +P / -Q diagnostic)


def _job(B, L, T):
    return f"guard_tiny:{B}-{L}-{T}-reuse"       # (the tag only names the job)


@functools.lru_cache(maxsize=None)
def _tiny(B, L, T):
    """Case and oracle side of one TINY step: computed once per process, shared by (a), (d) and (e), never changed."""
    name = _job(B, L, T)
    c, o = job_case(name), oracle(name)
    ci, lens, mel, tl, gate, masks = c["case"]
    masks = dict(masks, enc_drop=o["enc_drop"], prenet_drop=o["prenet_drop"])     # the (dekinked) masks the oracle ran with
    return dict(d=c["d"], P=c["P"], case=(ci, lens, mel, tl, gate, masks),
                reference=(o["ref"], o["loss"], o["grads"], o["new_stats"]))


def _sequence_a(dev, seq, value, guard_bytes):
    eng, ps = _engine(_tiny(*STEPS[0]), dev, guard_bytes)
    snaps = []
    for n, (B, L, T) in enumerate(STEPS, 1):
        st = _tiny(B, L, T)
        outs, ctx, loss3, names = _train_step(eng, ps, dev, st, value)
        _paths(B)(ctx)                                  # the path the step is named for
        assert (ctx["L"], ctx["T"]) == (L, T)
        if guard_bytes:
            assert eng.guard_check() == [], f"step {n}"
        else:
            assert not eng._guards
            if n == 2:          # the unguarded reuse path: this step's stash is a view of step 1's larger tensor
                assert eng._ws["xdec"].numel() == 13 * 33 * (st["d"]["att_rnn_dim"] + st["d"]["encoded_dim"]) > 6 * 5 * 128
        fig = _compare_train_step(eng, ps, outs, ctx, loss3, st["reference"])
        fig["grad_worst"], fig["grad_worst_name"] = _grad_worst(ps, st["reference"][2])
        _line(seq, f"step {n} (B,L,T)=({B},{L},{T})", fig)
        if n == 2:                                      # (the first poisoned call that finds workspaces: step 1 starts from none)
            _print_names(seq, names)
            assert names[1] == [] and len(names[0]) > 80, names          # TINY training steps have no integer workspace
        snaps.append(dict(outs=[x.clone() for x in outs], grad=ps.grad.clone()))
    worst = 0.0
    for a, b in zip(snaps[0]["outs"], snaps[6]["outs"]):          # the bound of test_long_forward_then_decode_then_the_same_forward
        diff, bound = float((a - b).abs().max()), 1e-5 * max(1.0, float(a.abs().max()))
        worst = max(worst, diff / bound)
        assert diff <= bound, (diff, bound)
    _line(seq, "step 7 against step 1", dict(worst_share_of_bound=worst))
    return ps, snaps


def _two_run_diagnostic(ps):
    """Largest difference between the +P and the -Q run, per output and per gradient: printed, not asserted (the split-K weight
    gradients use atomics)."""
    a, b = _RUNS["+P"], _RUNS["-Q"]
    for n, (sa, sb) in enumerate(zip(a, b), 1):
        outs = [float((x - y).abs().max()) for x, y in zip(sa["outs"], sb["outs"])]
        worst = (0.0, None)
        for name, p in ps.P.items():
            if name in ZERO_GRADIENT_BY_CONSTRUCTION:      # (rounding residue on both sides: tests/test_gpu_model.py)
                continue
            o_, k = ps.offsets[name], p.numel()
            ga, gb = sa["grad"][o_:o_ + k], sb["grad"][o_:o_ + k]
            d = float((ga - gb).abs().max()) / max(float(ga.abs().max()), 1e-3)
            if d > worst[0]:
                worst = (d, name)
        _line("a", f"+P against -Q, step {n}", dict(mels=outs[0], post=outs[1], gates=outs[2], align=outs[3], grad_worst=worst[0],
                                                    grad_worst_name=worst[1]))


def _oracle_marks(fn):
    for B, L, T in dict.fromkeys(STEPS):
        fn = pytest.mark.oracle(_job(B, L, T))(fn)
    return fn


@_oracle_marks
@pytest.mark.parametrize("label", list(VALUES))
def test_training_steps_across_shapes_on_one_engine(label):
    t0 = time.perf_counter()
    ps, _RUNS[label] = _sequence_a(_dev(), f"a[{label}]", VALUES[label], 0)
    if len(_RUNS) == 2:
        _two_run_diagnostic(ps)
    _wall(f"a[{label}]", t0)


@_oracle_marks
def test_training_steps_across_shapes_on_one_guarded_engine():
    """(e): with guard bands every size change reallocates, so every prezero / buf(zero=True) pair must agree on its size across the
    shape changes (the assertion in Engine.buf), and no band may be touched."""
    t0 = time.perf_counter()
    _sequence_a(_dev(), "e[+P]", WP.P_POS, GUARD)
    _wall("e[+P]", t0)


# ---- (d) the harness's own proof -----------------------------------------------------------------------------------------------------------
@_oracle_marks
@pytest.mark.parametrize("name,phase", [("pre_dec", "forward"), ("dpmT", "backward")])
def test_uncleared_accumulator_is_detected_under_poison(monkeypatch, name, phase):
    """pre_dec: the split-K blocks of the hoisted decoder-LSTM input GEMM (cleared ahead, accumulated into by K slices); dpmT: the
    processed-memory gradient that t2_attn_acc_bwd adds every chunk's share to.  Step 1 of (a) with that one clear left out:
    on a FRESH engine without poison the outcome is printed (profiles/engine_reuse.txt: it passes when this test runs alone in a
    fresh process, and fails behind tests that left non-zero memory in the process); on a reused, poisoned engine the comparison
    must fail."""
    from tacotron2_amd.engine import Engine
    t0 = time.perf_counter()
    dev = _dev()
    st = _tiny(*STEPS[0])

    def passes(eng, ps, outs, ctx, loss3):
        try:
            _compare_train_step(eng, ps, outs, ctx, loss3, st["reference"])
        except AssertionError:
            return False
        return True

    with monkeypatch.context() as mp:
        skipped = WP.skip_clear(mp, Engine, name)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()      # as in a fresh process: the workspaces come from the driver, not from blocks poisoned above
        eng, ps = _engine(st, dev)
        outs, ctx, loss3, _ = _train_step(eng, ps, dev, st, None)
        assert skipped, f"{name}: the step never asked for this region to be zero"
        assert eng._ws[name].is_floating_point()
    print(f"ENGINE-REUSE d {name} ({phase}): fresh engine, no poison, clear left out: the comparison "
          f"{'PASSES - invisible without poison' if passes(eng, ps, outs, ctx, loss3) else 'fails'}")
    eng, ps = _engine(st, dev)
    _train_step(eng, ps, dev, st, None)                 # an ordinary first step: the workspaces exist
    with monkeypatch.context() as mp:
        skipped = WP.skip_clear(mp, Engine, name)
        outs, ctx, loss3, names = _train_step(eng, ps, dev, st, WP.P_POS)
        assert skipped and name in names[0]
    with pytest.raises(AssertionError):
        _compare_train_step(eng, ps, outs, ctx, loss3, st["reference"])
    _wall(f"d[{name}]", t0)


# ---- (b) modes interleaved on one engine ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid():
    return decode_case(1)[:2]             # MID dims with speaker tokens; the parameters of every decode_case


def _mid_inputs(B, L, T, seed):
    d, P = _mid()
    case = edge_lengths_case(d, B, L, T, seed)
    spk = torch.randint(0, 4, (B,), generator=torch.Generator().manual_seed(B), dtype=torch.int32)
    return d, P, case, spk


@functools.lru_cache(maxsize=None)
def _mid_train(B, L, T, seed):
    d, P, (ci, lens, mel, tl, gate, masks), spk = _mid_inputs(B, L, T, seed)
    masks, _ = dekink_masks(P, d, ci, mel, masks)      # ReLU-kink elements out of both sides (tests/helpers.py)
    return dict(d=d, P=P, case=(ci, lens, mel, tl, gate, masks), kw=dict(speaker_id=spk),
                reference=oracle_train(P, d, ci, lens, mel, tl, gate, masks, speaker_id=spk))


@functools.lru_cache(maxsize=None)
def _mid_eval(B, L, T, seed):
    """Eval-mode teacher-forced forward: only the prenet's dropout stays on (running BatchNorm statistics, no other mask)."""
    d, P, (ci, lens, mel, tl, gate, masks), spk = _mid_inputs(B, L, T, seed)
    masks = dict(prenet_drop=masks["prenet_drop"])
    with torch.no_grad():
        ref = R.tacotron2_fwd(P, d, ci, lens, True, mel, tl, speaker_id=spk, training=False, masks=masks)
    return dict(d=d, P=P, case=(ci, lens, mel, tl, gate, masks), kw=dict(speaker_id=spk), ref=ref)


@functools.lru_cache(maxsize=None)
def _decode(B, window, N):
    d, P, ci, lens, spk, pm, N = decode_case(B, N)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    L = ci.shape[1]
    with torch.no_grad():
        ref = windowed_ref(P64, d, ci, lens, N, window or (L, L), speaker_id=spk, prenet_drop=pm)
    return dict(P=P, inputs=(ci, lens, spk, pm), N=N, ref=ref)


def _decode_step(eng, ps, dev, seq, n, B, window, N, check_every, value):
    """The criteria of test_guarded_decode_across_groups_matches_oracle on the shared engine."""
    c = _decode(B, window, N)
    (ci, lens, spk, pm), (rm, rp, rg, ra, rl) = c["inputs"], c["ref"]
    assert len(set(rl.tolist())) > 1, rl                # ragged stops, or the case would not test the stop path
    args = (ci.to(dev), lens.to(dev))
    spkd, pmd = spk.to(dev), pm.to(dev).contiguous()
    M = rm.shape[2]
    _before_call(eng, ps, dev, c["P"], value, _sizes(B, ci.shape[1], N, M) + _sizes(min(B, 64), ci.shape[1], N, M))
    mels, post, gates, al, lengths = eng.infer(*args, N, speaker_id=spkd, prenet_masks=pmd, check_every=check_every,
                                               attention_window=window, training=False)
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    assert all(f"inf{g}.state" in eng._ws for g in range((B + 63) // 64))
    if window is not None:
        assert "inf0.win_peak" in eng._ws
    fig = dict(frames=mels.shape[1], stops=sorted(set(rl.tolist())), mel_l1=l1(mels, rm), post_l1=l1(post, rp), align_max=mx(al, ra))
    _line(seq, f"step {n} infer B={B} window={window} N={N} check_every={check_every}", fig)
    assert mels.shape == rm.shape, (mels.shape, rm.shape)
    assert torch.equal(lengths.cpu(), rl)
    assert fig["mel_l1"] < MEL_L1_TOL and fig["post_l1"] < MEL_L1_TOL
    assert fig["align_max"] < 5e-5
    assert torch.equal(gates.cpu() == -1000.0, rg == -1000.0)


def _forward_only(eng, ps, dev, st, value, training):
    ci, lens, mel, tl, gate, masks = st["case"]
    args = (ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev))
    dm = masks_to_device(masks, dev)
    kw = {k: v.to(dev) for k, v in st["kw"].items()}
    _before_call(eng, ps, dev, st["P"], value, _sizes(ci.shape[0], ci.shape[1], mel.shape[1], mel.shape[2]))
    outs, ctx = eng.forward_tf(*args, training=training, masks=dm, save_for_backward=False, **kw)
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    return outs, ctx


@pytest.mark.parametrize("label", list(VALUES))
def test_training_eval_forward_and_decode_interleaved_on_one_engine(label):
    t0 = time.perf_counter()
    dev, value, seq = _dev(), VALUES[label], f"b[{label}]"
    first, last = _mid_train(33, 19, 12, 7033), _mid_train(5, 11, 21, 7005)
    ev = _mid_eval(17, 27, 9, 7017)
    eng, ps = _engine(first, dev)

    def train(n, st):
        outs, ctx, loss3, names = _train_step(eng, ps, dev, st, value)
        _paths(st["case"][0].shape[0])(ctx)
        fig = _compare_train_step(eng, ps, outs, ctx, loss3, st["reference"])
        fig["grad_worst"], fig["grad_worst_name"] = _grad_worst(ps, st["reference"][2])
        _line(seq, f"step {n} training (B,L,T)=({ctx['B']},{ctx['L']},{ctx['T']})", fig)
        return names

    train(1, first)                                                            # 1. training step, B = 33
    _decode_step(eng, ps, dev, seq, 2, 65, None, 24, 3, value)                  # 2. two decode groups, no window
    _decode_step(eng, ps, dev, seq, 3, 3, (1, 3), 16, 1, value)                 # 3. three utterances, the window, fewer frames
    outs, ctx = _forward_only(eng, ps, dev, ev, value, training=False)          # 4. eval forward, B = 17
    _paths(17)(ctx)
    _line(seq, "step 4 eval forward (B,L,T)=(17,27,9)", _check_forward(outs, ev["ref"]))
    _decode_step(eng, ps, dev, seq, 5, 65, (1, 3), 24, 1, value)                # 5. two decode groups with the window
    outs, ctx = _forward_only(eng, ps, dev, first, value, training=True)        # 6. a forward without stashes ...
    _paths(33)(ctx)
    _line(seq, "step 6 forward without stashes (B,L,T)=(33,19,12)", _check_forward(outs, first["reference"][0]))
    names = train(6, last)                                                      #    ... then a training step at another shape
    _print_names(seq, names)
    ints = [k for k in names[1] if not eng._ws[k].is_floating_point()]
    assert ints == names[1] and {"inf0.done", "inf0.state", "inf1.state", "inf0.win_peak", "inf.lengths"} <= set(ints), names[1]
    _wall(seq, t0)


# ---- (c) options toggled between steps ------------------------------------------------------------------------------------------------------
def _zone_case(*args):
    from tests.test_gpu_zoneout import _train_case
    c = _train_case(*args)
    return dict(d=c[0], P=c[1], case=c[2], zones=c[3], c=c)


@pytest.mark.parametrize("label", list(VALUES))
def test_options_toggled_between_steps_on_one_engine(label):
    """Reduction factor 2 with zoneout (dims and float64 references of tests/test_gpu_zoneout.py, its criteria)."""
    from tests.test_gpu_reduction_factor import _check_outputs, _grad_report
    from tests.test_gpu_zoneout import _guided_term, _ref_grads
    t0 = time.perf_counter()
    dev, value, seq = _dev(), VALUES[label], f"c[{label}]"
    sigma, alpha = 0.4, 1.0
    # (B, L, T, r, seed, forward-attention reference); the second pair is smaller than the first
    steps = [(_zone_case(33, 21, 10, 2, 435), False, False, (64, "persistent")),
             (_zone_case(33, 21, 10, 2, 436, True), True, True, (64, "persistent")),
             (_zone_case(5, 17, 8, 2, 437), False, False, (2, "steps")),
             (_zone_case(5, 17, 8, 2, 438, True), True, False, (64, "persistent"))]
    eng, ps = _engine(steps[0][0], dev)
    assert eng.r == 2 and eng.zoneout > 0.0
    for n, (st, fa, with_guided, (chunk, chain)) in enumerate(steps, 1):
        c = st["c"]
        (ci, lens, mel, tl, gate, m), o = c[2], c[5]
        tot, bce, ml, pl = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())
        g_tot = _guided_term(o[3], lens, tl, 2, sigma, alpha) if with_guided else None
        eng.chunk = eng.chunk_bwd = chunk
        eng.dec_chain = chain
        outs, ctx, loss3, names = _train_step(eng, ps, dev, st, value, guided=(sigma, alpha) if with_guided else None,
                                              **(dict(forward_attention=True) if fa else {}))
        B = ci.shape[0]
        _paths(B, chain)(ctx)
        assert bool(ctx["forward_attention"]) == fa and ("dprior" in eng._ws) == (n >= 2)
        label_n = f"step {n} (B,L,T)=({B},{ci.shape[1]},{mel.shape[1]}) forward_attention={fa} guided={with_guided} chunk={chunk} {chain}"
        _check_outputs(outs, o, f"{seq} {label_n}")
        ref3 = torch.stack([bce, ml, pl]).detach()
        assert torch.allclose(loss3.cpu(), ref3, rtol=1e-5, atol=1e-6), (loss3.cpu(), ref3)
        fig = dict(mel_l1=l1(outs[0], o[0].detach()), post_l1=l1(outs[1], o[1].detach()), align_max=mx(outs[3], o[3].detach()),
                   gates_max=mx(outs[2], o[2].detach()), loss_rel=float(((loss3.cpu() - ref3).abs() / ref3.abs().clamp(min=1e-6)).max()))
        if with_guided:
            want = float(g_tot.detach())
            fig["guided_rel"] = abs(float(eng.guided_loss.cpu()) - want) / max(1.0, want)
            assert fig["guided_rel"] < 1e-5
        else:
            assert eng.guided_loss is None
        grads = _ref_grads(c, tot + g_tot if with_guided else tot)
        fig["grad_worst"], fig["grad_worst_name"] = _grad_worst(ps, grads)
        _line(seq, label_n, fig)
        _grad_report(ps, grads, f"{seq} {label_n}")
        if n == 4:
            _print_names(seq, names)
    _wall(seq, t0)
