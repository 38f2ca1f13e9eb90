"""Loss options (l1 / l1+l2 mel terms, the masked mean, the stop-class weight) and the decode stop threshold on the GPU: the one loss
kernel body through `t2_loss_fwd_bwd_opt` and `t2_loss_terms_opt` and the scan through `t2_stop_scan_thr` against the float64
restatement (tests/loss_options_ref.py), the defaults bit for bit against the entries without the suffix, NaN in the padding under
the masked mean, refusals, and the engine / module / driver surface end to end."""
import itertools

import pytest
import torch

from tests import loss_options_ref as LR

pytestmark = pytest.mark.gpu

OPTION_GRID = list(itertools.product(LR.MEL_LOSSES, (False, True), (1.0, 8.0)))
SMALL = dict(B=3, T=7, M=5, lens=(7, 4, 1))
WIDE = dict(B=4, T=130, M=80, lens=(130, 77, 1, 0))        # 165 workgroups: cross-workgroup sums, n_f formed by each of them


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _behind_nan(t, dev):
    """`t` on the device as a view with NaN written behind its last element (a read past the end poisons the result)."""
    fill = float("nan") if t.is_floating_point() else 2 ** 30
    flat = torch.full((t.numel() + 4096,), fill, dtype=t.dtype, device=dev)
    flat[:t.numel()] = t.reshape(-1).to(dev)
    return flat[:t.numel()].view(t.shape)


def _opts(mel_loss="l2", masked=False, stop_weight=1.0):
    from tacotron2_amd import _lib
    return _lib.make("T2LossOpts", mel_loss=LR.MEL_LOSSES.index(mel_loss), masked=int(masked), stop_weight=float(stop_weight))


@pytest.fixture(scope="module")
def cases():
    """The operands of both shapes, built once and left unchanged: outputs masked as the forward masks them (0 / -1000 at or beyond
    len), a target with its own padding values, and in every utterance a few predictions that EQUAL the target (sign(0) = 0)."""
    out = {}
    for name, c in (("small", SMALL), ("wide", WIDE)):
        B, T, M = c["B"], c["T"], c["M"]
        g = torch.Generator().manual_seed(5800 + T)
        lens = torch.tensor(c["lens"], dtype=torch.int32)
        mm = ~LR.valid_mask(lens, T)[:, :, None]
        tgt = torch.randn(B, T, M, generator=g) - 2
        raw = torch.randn(B, T, M, generator=g) - 2
        raw_post = raw + 0.3 * torch.randn(B, T, M, generator=g)
        raw[:, 0, ::2] = tgt[:, 0, ::2]                     # errors that are exactly 0, at valid positions (frame 0)
        raw_post[:, 0, 1::3] = tgt[:, 0, 1::3]
        mels, post = raw.masked_fill(mm, 0.0), raw_post.masked_fill(mm, 0.0)
        gates = (1.5 * torch.randn(B, T, 1, generator=g)).masked_fill(mm, -1000.0)
        gtgt = (torch.rand(B, T, 1, generator=g) > 0.3).float()
        out[name] = dict(B=B, T=T, M=M, lens=lens, mels=mels, post=post, gates=gates, tgt=tgt, gtgt=gtgt)
    return out


def _reference(c, mel_loss, masked, w, r):
    d = lambda t: t.double()
    args = (d(c["mels"]), d(c["post"]), d(c["gates"]), d(c["tgt"]), d(c["gtgt"]), c["lens"])
    l3 = torch.stack(LR.loss_terms(*args, mel_loss=mel_loss, masked=masked, stop_weight=w))
    gm, gp, gg = LR.loss_grads(*args, mel_loss=mel_loss, masked=masked, stop_weight=w)
    return l3, gm, gp, gg, LR.pack_dproj(gm, gp, gg, r)


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _run_fused(c, opts, r, dev, guard=True, entry="t2_loss_fwd_bwd_opt"):
    from tacotron2_amd import _lib
    B, T, M = c["B"], c["T"], c["M"]
    S = (T + r - 1) // r
    put = (lambda t: _behind_nan(t, dev)) if guard else (lambda t: t.to(dev))
    loss3 = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    d_post = torch.full((B, T, M), 7.0, device=dev)
    dproj = torch.full((S, B, r * M + 1), 7.0, device=dev)
    ops = [put(c[k]) for k in ("mels", "post", "gates", "tgt", "gtgt", "lens")]
    if entry == "t2_loss_fwd_bwd_opt":
        _lib.call(entry, *ops, B, T, M, r, loss3, d_post, dproj, 1.0, opts, _st())
    elif entry == "t2_loss_fwd_bwd_r":
        _lib.call(entry, *ops, B, T, M, r, loss3, d_post, dproj, 1.0, _st())
    else:
        assert entry == "t2_loss_fwd_bwd" and r == 1
        _lib.call(entry, *ops, B, T, M, loss3, d_post, dproj, 1.0, _st())
    torch.cuda.synchronize()
    return loss3, d_post, dproj


def _run_terms(c, opts, dev, guard=True, entry="t2_loss_terms_opt"):
    from tacotron2_amd import _lib
    B, T, M = c["B"], c["T"], c["M"]
    put = (lambda t: _behind_nan(t, dev)) if guard else (lambda t: t.to(dev))
    loss3 = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    d_mels, d_post = torch.full((B, T, M), 7.0, device=dev), torch.full((B, T, M), 7.0, device=dev)
    d_gates = torch.full((B, T, 1), 7.0, device=dev)
    ops = [put(c[k]) for k in ("mels", "post", "gates", "tgt", "gtgt", "lens")]
    if entry == "t2_loss_terms_opt":
        _lib.call(entry, *ops, B, T, M, loss3, d_mels, d_post, d_gates, 1.0, opts, _st())
    else:
        _lib.call("t2_loss_terms", *ops, B, T, M, loss3, d_mels, d_post, d_gates, 1.0, _st())
    torch.cuda.synchronize()
    return loss3, d_mels, d_post, d_gates


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _check_against_reference(c, mel_loss, masked, w, r, dev):
    """loss3 rtol 1e-5 / atol 1e-6 against float64, gradients to 1e-5 of the reference's largest element: the project's tolerances
    for this kernel (tests/test_gpu_reduction_factor.py, test_grouped_loss_kernel_matches_torch)."""
    ref3, gm, gp, gg, want = _reference(c, mel_loss, masked, w, r)
    opts = _opts(mel_loss, masked, w)
    loss3, d_post, dproj = _run_fused(c, opts, r, dev)
    print(f"{mel_loss} masked {masked} w {w} r {r}: loss3 {loss3.tolist()} ref {ref3.tolist()} "
          f"d_post {_rel(d_post, gp):.2e} dproj {_rel(dproj, want):.2e}")
    assert torch.allclose(loss3.cpu(), ref3, rtol=1e-5, atol=1e-6)
    assert _rel(d_post, gp) < 1e-5 and _rel(dproj, want) < 1e-5
    if r == 1:
        l3, d_mels, d_post_t, d_gates = _run_terms(c, opts, dev)
        print(f"  terms: d_mels {_rel(d_mels, gm):.2e} d_post {_rel(d_post_t, gp):.2e} d_gates {_rel(d_gates, gg):.2e}")
        assert torch.allclose(l3.cpu(), ref3, rtol=1e-5, atol=1e-6)
        assert _rel(d_mels, gm) < 1e-5 and _rel(d_post_t, gp) < 1e-5 and _rel(d_gates, gg) < 1e-5
        # sign(0) = 0: where the prediction equals the target an l1 gradient is exactly 0
        if mel_loss == "l1":
            hit = (c["mels"] == c["tgt"]) & LR.valid_mask(c["lens"], c["T"])[:, :, None]
            assert int(hit.sum()) > 0 and float(d_mels.cpu()[hit].abs().max()) == 0.0


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("mel_loss,masked,w", OPTION_GRID)
def test_loss_kernel_options_match_the_restatement(cases, mel_loss, masked, w, r):
    _check_against_reference(cases["small"], mel_loss, masked, w, r, _dev())


@pytest.mark.parametrize("mel_loss,masked,w", OPTION_GRID)
def test_loss_kernel_options_over_many_workgroups(cases, mel_loss, masked, w):
    _check_against_reference(cases["wide"], mel_loss, masked, w, 1, _dev())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. off is bit-identical
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2])
def test_default_options_are_the_existing_entries_bit_for_bit(cases, r):
    dev = _dev()
    for c in (cases["small"], cases["wide"]):
        got = _run_fused(c, _opts(), r, dev)
        old = _run_fused(c, None, r, dev, entry="t2_loss_fwd_bwd_r")
        assert all(torch.equal(a, b) for a, b in zip(got[1:], old[1:]))
        # (the three sums are double atomics over the workgroups: one workgroup - the small shape - adds in one order)
        assert torch.equal(got[0], old[0]) if c is cases["small"] else torch.allclose(got[0], old[0], rtol=1e-12, atol=0)
        if r == 1:
            plain = _run_fused(c, None, 1, dev, entry="t2_loss_fwd_bwd")
            assert all(torch.equal(a, b) for a, b in zip(got[1:], plain[1:]))
            gt, ot = _run_terms(c, _opts(), dev), _run_terms(c, None, dev, entry="t2_loss_terms")
            assert all(torch.equal(a, b) for a, b in zip(gt[1:], ot[1:]))
            assert torch.equal(gt[0], ot[0]) if c is cases["small"] else torch.allclose(gt[0], ot[0], rtol=1e-12, atol=0)


SIGN = {0: [1, -1, 1, 1, -1], 1: [1, 1, 1, -1, 1], 2: [1, 1, 1, 1, 1], 3: [-1, 1, -1, 1, -1], 4: [1, 1, -1, -1, 1]}


def _scan(utts, groups, max_len, r, dev, thr=None, mag=None, entry=None):
    """The hand-made sign table of tests/test_gpu_reduction_factor.py's stop-scan test (5 stored steps), each logit 0.5 * sign - or
    mag[utterance][step] * sign - in column r*2 of projection rows of width 2r + 2 whose padding columns are NaN."""
    from tacotron2_amd import _lib
    N, Mr, ld = 5, 2 * r, 2 * r + 2
    projs, k, table = [], 0, []
    for Bg in groups:
        p = torch.full((N, Bg, ld), float("nan"))
        p[:, :, :Mr] = 0.25
        for b in range(Bg):
            u = utts[k]; k += 1
            m = torch.tensor(mag[u], dtype=torch.float32) if mag is not None else torch.full((N,), 0.5)
            p[:, b, Mr] = m * torch.tensor(SIGN[u], dtype=torch.float32)
            table.append(p[:, b, Mr].clone())
        projs.append(_behind_nan(p, dev))
    scan = _lib.make("T2StopScan", proj=projs + [0] * (64 - len(projs)), Bg=list(groups) + [0] * (64 - len(groups)),
                     ngroups=len(groups), ld_proj=ld, M=Mr, nframes=N)
    lengths = torch.full((len(utts),), -7, dtype=torch.int64, device=dev)
    out2 = torch.full((2,), -7, dtype=torch.int32, device=dev)
    if entry == "t2_stop_scan_r":
        _lib.call("t2_stop_scan_r", scan, r, max_len, lengths, out2, _st())
    else:
        _lib.call("t2_stop_scan_thr", scan, r, max_len, float(thr), lengths, out2, _st())
    torch.cuda.synchronize()
    return lengths.cpu().tolist(), out2.cpu().tolist(), torch.stack(table, 1)


def test_stop_scan_at_logit_zero_is_the_existing_scan():
    dev = _dev()
    for utts, groups, max_len, r in (([0, 1, 2, 3, 4], (2, 3), 13, 3), ([0, 1, 3, 4], (2, 2), 13, 3), ([0, 1, 3, 4], (4,), 100, 3),
                                     ([0, 1, 2, 3, 4], (2, 3), 3, 1), ([0, 1, 3, 4], (2, 2), 100, 1)):
        assert _scan(utts, groups, max_len, r, dev, thr=0.0)[:2] == _scan(utts, groups, max_len, r, dev, entry="t2_stop_scan_r")[:2]
    assert _scan([0, 1, 2, 3, 4], (2, 3), 13, 3, dev, thr=0.0)[:2] == ([9, 12, 13, 6, 9], [13, 5])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. masked means masked
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mel_loss,w", [("l2", 1.0), ("l1+l2", 8.0)])
def test_masked_mean_reads_nothing_in_the_padding(cases, mel_loss, w):
    dev = _dev()
    for c in (cases["small"], cases["wide"]):
        inv = ~LR.valid_mask(c["lens"], c["T"])[:, :, None]
        zero = dict(c, **{k: c[k].masked_fill(inv, 0.0) for k in ("mels", "post", "gates", "tgt", "gtgt")})
        nan = dict(c, **{k: c[k].masked_fill(inv, float("nan")) for k in ("mels", "post", "gates", "tgt", "gtgt")})
        assert int(inv.sum()) > 0 and bool(torch.isnan(nan["gates"]).any())
        opts = _opts(mel_loss, True, w)
        for r in (1, 2):
            a, b = _run_fused(zero, opts, r, dev), _run_fused(nan, opts, r, dev)
            assert all(bool(torch.isfinite(t).all()) for t in b)
            assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
            # (one workgroup on the small shape: one order of the double atomics, so loss3 is equal to the bit; 165 workgroups on the wide one)
            assert torch.equal(a[0], b[0]) if c is cases["small"] else torch.allclose(a[0], b[0], rtol=1e-12, atol=0)
            assert float(b[1].cpu()[inv.expand_as(b[1])].abs().max()) == 0.0
        a, b = _run_terms(zero, opts, dev), _run_terms(nan, opts, dev)
        assert all(bool(torch.isfinite(t).all()) for t in b)
        assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
        assert torch.equal(a[0], b[0]) if c is cases["small"] else torch.allclose(a[0], b[0], rtol=1e-12, atol=0)
        for t in b[1:]:
            assert float(t.cpu()[inv.expand_as(t)].abs().max()) == 0.0
        # against the restatement too (which indexes the valid frames)
        ref3 = _reference(nan, mel_loss, True, w, 1)[0]
        assert torch.allclose(b[0].cpu(), ref3, rtol=1e-5, atol=1e-6)


def test_masked_mean_of_an_empty_batch_is_zero(cases):
    dev = _dev()
    c = dict(cases["small"], lens=torch.zeros(3, dtype=torch.int32))
    for r in (1, 3):
        for t in _run_fused(c, _opts("l1+l2", True, 8.0), r, dev):
            assert float(t.abs().max()) == 0.0
    for t in _run_terms(c, _opts("l1", True, 1.0), dev):
        assert float(t.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_bad_options_are_refused_before_anything_is_launched():
    from tacotron2_amd import _lib
    dev = _dev()
    B, T, M = 1, 4, 4
    x = torch.zeros(256, device=dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    outs = [torch.full((256,), 7.0, device=dev) for _ in range(3)]
    loss3 = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    lengths = torch.full((B,), -7, dtype=torch.int64, device=dev)
    out2 = torch.full((2,), -7, dtype=torch.int32, device=dev)
    scan = _lib.make("T2StopScan", proj=[x] + [0] * 63, Bg=[B] + [0] * 63, ngroups=1, ld_proj=M + 1, M=M, nframes=T)
    mk = lambda m, w: _lib.make("T2LossOpts", mel_loss=m, masked=0, stop_weight=w)
    bad = [None, mk(3, 1.0), mk(-1, 1.0), mk(0, 0.0), mk(0, -2.0), mk(1, float("nan")), mk(2, float("inf"))]
    for o in bad:
        with pytest.raises(_lib.T2Error, match="rc=1"):
            _lib.call("t2_loss_fwd_bwd_opt", x, x, x, x, x, lens, B, T, M, 1, loss3, outs[0], outs[1], 1.0, o, _st())
        with pytest.raises(_lib.T2Error, match="rc=1"):
            _lib.call("t2_loss_terms_opt", x, x, x, x, x, lens, B, T, M, loss3, outs[0], outs[1], outs[2], 1.0, o, _st())
    with pytest.raises(_lib.T2Error, match="rc=1"):       # r >= 1, as the _r entry
        _lib.call("t2_loss_fwd_bwd_opt", x, x, x, x, x, lens, B, T, M, 0, loss3, outs[0], outs[1], 1.0, mk(1, 1.0), _st())
    for thr in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(_lib.T2Error, match="rc=1"):
            _lib.call("t2_stop_scan_thr", scan, 1, 100, thr, lengths, out2, _st())
    with pytest.raises(_lib.T2Error, match="rc=1"):
        _lib.call("t2_stop_scan_thr", scan, 0, 100, 0.0, lengths, out2, _st())
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((loss3 == 7.0).all())
    assert bool((lengths == -7).all()) and bool((out2 == -7).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the stop scan with a threshold
# ---------------------------------------------------------------------------------------------------------------------------
# magnitudes on both sides of |logit(0.3)| = |logit(0.7)| = 0.8473: a positive logit of 0.3 continues at 0.5 and stops at 0.7, a
# negative one of -0.3 stops at 0.5 and continues at 0.3
MAG = {0: [0.3, 0.3, 2.0, 0.9, 1.1], 1: [1.5, 0.2, 0.86, 0.3, 0.84], 2: [2.0, 0.9, 0.3, 1.0, 3.0], 3: [0.84, 0.5, 0.86, 0.1, 0.2],
       4: [0.9, 0.4, 0.7, 1.3, 0.6]}


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("tau", [0.3, 0.5, 0.7])
def test_stop_scan_with_a_threshold_matches_the_restatement(tau, r):
    dev = _dev()
    thr = LR.stop_logit(tau)
    for utts, groups in (([0, 1, 2, 3, 4], (5,)), ([0, 1, 2, 3, 4], (2, 3)), ([0, 1, 3, 4], (4,)), ([3, 4, 0], (1, 2))):
        for max_len in (5 * r - 2, 100):          # a cap that binds where the loop runs long, and one that does not
            lengths, out2, table = _scan(utts, groups, max_len, r, dev, thr=thr, mag=MAG)
            want, frames, steps = LR.stop_count(table, thr, r, max_len)
            assert lengths == want.tolist() and out2 == [frames, steps], (utts, groups, max_len, lengths, out2)
    if tau != 0.5:       # the threshold matters on this table: the 0.5 rule gives other lengths somewhere
        lengths, out2, table = _scan([0, 1, 3, 4], (4,), 100, r, dev, thr=thr, mag=MAG)
        assert (lengths, out2) != (LR.stop_count(table, 0.0, r, 100)[0].tolist(), list(LR.stop_count(table, 0.0, r, 100)[1:]))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. end to end, training
# ---------------------------------------------------------------------------------------------------------------------------
E2E_OPTS = ("l1+l2", True, 8.0)


def _e2e_case():
    """The oracle case of test_loss_and_grads_with_the_guided_term_matches_the_oracle (MID dims, (4, 33, 29), seed 101) with the
    float64 oracle forward; cached there, so the tests here and there share one forward."""
    from tests.test_gpu_guided_attention import _oracle_case
    return _oracle_case(4, 33, 29, 101)


def _restated_total(c, guided=None):
    from tests.test_guided_attention_host import guided_ref
    d, P, (ci, lens, mel, tl, gate, masks), Pc, o, names = c
    terms = LR.loss_terms(o[0], o[1], o[2], mel.double(), gate.double(), tl, *E2E_OPTS)
    total = terms[0] + terms[1] + terms[2]
    gl = guided_ref(o[3], lens, tl, *guided)[0] if guided is not None else None
    return terms, gl, (total if gl is None else total + gl)


@pytest.mark.parametrize("guided", [None, (0.4, 100.0)])
def test_loss_and_grads_with_loss_options_matches_the_oracle(guided):
    """Engine.loss_and_grads(loss=("l1+l2", True, 8.0)) + backward_tf against the float64 oracle forward with the restated loss and
    autograd: the three terms to 2e-5 and every parameter gradient with the relative-to-scale rule, as the guided-attention test
    this follows; once more with guided=(0.4, 100.0): the two compose."""
    from oracle import tacotron2_ref as R
    from tests.test_gpu_guided_attention import _oracle_grads
    from tests.test_gpu_model import _grad_check, build_engine, masks_to_device
    dev = _dev()
    c = _e2e_case()
    d, P, (ci, lens, mel, tl, gate, masks), Pc, o, names = c
    terms, gl, total = _restated_total(c, guided)
    grads = _oracle_grads(c, lambda o_: total)
    eng, ps = build_engine(d, P, dev)
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev))
    ps.grad.zero_()
    loss3 = eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev), guided=guided, loss=E2E_OPTS)
    torch.cuda.synchronize()
    got, want = [float(x) for x in loss3.cpu()], [float(x.detach()) for x in terms]
    print("three terms (gate, mel, post):", got, "restated on the oracle:", want)
    for g_, w_ in zip(got, want):
        assert abs(g_ - w_) < 2e-5 * max(1.0, abs(w_)), (got, want)
    if guided is not None:
        assert abs(float(eng.guided_loss.cpu()) - float(gl)) < 2e-5 * max(1.0, abs(float(gl)))
    _grad_check(ps, grads)
    # the options matter here: the reference's three-term gradients are far outside the tolerance for the output layers
    plain = _oracle_grads(c, lambda o_: R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())[0] + (gl if gl is not None else 0))
    for n in ("decoder.mel_out.weight", "decoder.gate.weight", "postnet.convolutions.16.weight"):
        if n in grads:
            assert float((grads[n] - plain[n]).abs().max()) > 100 * 3e-4 * max(float(grads[n].abs().max()), 1e-3), n


def test_module_training_step_with_loss_options_is_the_fused_step():
    """TTSModel.loss_options through training_step (t2_loss_terms_opt, then the packed backward) against Engine.loss_and_grads(loss=...)
    on the same batch, parameters and masks (the module's own Philox masks): the same three terms, every parameter gradient with
    the relative-to-scale rule of the module comparisons in tests/test_gpu_guided_attention.py."""
    from tacotron2_amd.model import TTSModel
    from tests.test_gpu_guided_attention import MID
    from tests.test_gpu_model import _grad_check
    dev = _dev()
    d, P, (ci, lens, mel, tl, gate, masks) = _e2e_case()[:3]
    tm = TTSModel(lr=1e-3, weight_decay=1e-6, device=dev, **MID)
    tm.tacotron2.load_state_dict(P)
    tm.train()
    t2 = tm.tacotron2
    eng, ps = t2._engine, t2.store
    pm = eng.make_masks(4, 33, 29, True, t2._seed, t2._calls)
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=pm)
    ps.grad.zero_()
    loss3 = eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev), loss=E2E_OPTS).cpu().clone()
    torch.cuda.synchronize()
    fused = {k: v.detach().cpu().clone() for k, v in ps.reference_layout(ps.G).items()}
    default3 = eng.loss_and_grads(*eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=pm),
                                  mel.to(dev), gate.to(dev)).cpu().clone()
    batch = ({"chars_idx": ci.to(dev), "mel_spectrogram": mel.to(dev), "gate": gate.to(dev)},
             {"chars_idx_len": lens.to(dev), "mel_spectrogram_len": tl.to(dev)}, {})
    tm.zero_grad()
    tm.loss_options = {"mel": "l1+l2", "masked": True, "stop_weight": 8.0}
    calls = t2._calls
    loss = tm.training_step(batch, 0)                 # (its Philox masks are those of `pm`: the same seed and call count)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(loss3.sum())) < 1e-6 * max(1.0, float(loss3.sum()))
    _grad_check(ps, fused)
    t2._calls = calls
    with torch.no_grad():
        terms = tm._loss(batch)[1]
    got = [float(x) for x in terms]
    print("module terms", got, "fused", loss3.tolist(), "default", default3.tolist())
    for g_, w_ in zip(got, loss3.tolist()):
        assert abs(g_ - w_) < 1e-6 * max(1.0, abs(w_))
    assert abs(float(loss3.sum()) - float(default3.sum())) > 1e-2      # not the default loss
    assert "loss_options" not in tm.hparams
    tm.loss_options = {"mel": "l3"}
    with pytest.raises(ValueError, match="l3"):
        tm.training_step(batch, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. end to end, decoding
# ---------------------------------------------------------------------------------------------------------------------------
def _firsts(logits, thr):
    below = logits < thr
    return [int(torch.nonzero(below[:, b])[0]) if bool(below[:, b].any()) else -1 for b in range(logits.shape[1])]


def _pick_threshold(logits, want):
    """A threshold logit in the widest gap (>= 2.5e-3 wide: 1e-3 clear on both sides with room for the float32 rounding of tau) of
    the sorted stored logits [N][B] at which `want(firsts)` holds; host arithmetic on the first run's logits only."""
    flat = logits.flatten().sort().values
    gaps = flat[1:] - flat[:-1]
    for i in torch.argsort(gaps, descending=True).tolist():
        if float(gaps[i]) < 2.5e-3:
            break
        thr = float((flat[i] + flat[i + 1]) / 2)
        if want(_firsts(logits, thr)):
            return thr
    raise AssertionError("no threshold with a clear margin on this case")


def test_decode_with_a_stop_threshold_is_the_prefix_of_the_unstopped_decode():
    """The B = 70, L = 23, N = 14 case of tests/test_gpu_model.py (vanilla dims, two decode groups, check_every = 3).  That case's 980
    stop logits lie within 0.16 of each other - no gap of 2e-3 between them where a threshold must go - so the gate weight is scaled
    by a further 10 (which changes no other output), and the gate bias is raised until the 0.5 rule never stops in 14 frames.
    tau comes from the stored logits of that run: (a) some utterances stop within 5 frames, one stops at frame 8 or later and one
    never stops; (b) every utterance stops within 7 frames, so the loop ends early.  Each decode with stop_threshold = tau must
    give the restated count rule on the first run's logits, the first run's frames bit for bit (masked from `lengths` on), and
    a loop that ends at most one chunk after the chunk of the break frame."""
    import math
    from oracle import tacotron2_ref as R
    from tests.test_gpu_model import build_engine
    dev = _dev()
    d = R.default_dims()
    P = R.init_params(d, seed=70)
    P["decoder.gate.weight"] = P["decoder.gate.weight"] * 80.0
    P["decoder.gate.bias"] = P["decoder.gate.bias"] - 0.05 + 1.5
    g = torch.Generator().manual_seed(70)
    B, L, N, CE, M = 70, 23, 14, 3, 80
    lens = torch.randint(4, L + 1, (B,), generator=g); lens[0] = L
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    pm = (torch.rand(N + 1, 2, B, 256, generator=g) >= 0.5).float() * 2
    eng, ps = build_engine(d, P, dev)
    run = lambda **kw: eng.infer(ci.to(dev), lens.to(dev), N, prenet_masks=pm.to(dev).contiguous(), check_every=CE, **kw)

    def stored():
        ldo = (M + 1 + 3) // 4 * 4
        cols = [eng._ws[f"inf{g_}.proj"][:N * Bg * ldo].view(N, Bg, ldo)[:, :, M] for g_, Bg in ((0, 64), (1, 6))]
        return torch.cat(cols, 1).cpu().clone(), max(int(eng._ws[f"inf{g_}.state"][1]) for g_ in (0, 1))

    mels0, post0, gates0, al0, len0 = [t.clone() for t in run()]
    torch.cuda.synchronize()
    logits, ran0 = stored()
    assert float(logits.min()) > 0 and mels0.shape[1] == N and len0.tolist() == [N] * B and ran0 == N      # 0.5 never stops
    assert torch.equal(gates0[:, :, 0].cpu(), logits.t())
    cases = (("ragged", lambda f: any(0 <= x < 5 for x in f) and any(x >= 8 for x in f) and any(x < 0 for x in f)),
             ("all stop", lambda f: all(0 <= x < 7 for x in f) and len(set(f)) > 1))
    for label, want in cases:
        thr = _pick_threshold(logits, want)
        tau = 1.0 / (1.0 + math.exp(-thr))
        thr32 = LR.stop_logit(tau)
        clear = float((logits - thr32).abs().min())
        lengths_w, frames_w, steps_w = LR.stop_count(logits, thr32, 1, N)
        print(f"{label}: tau {tau:.6f} logit {thr32:.5f} nearest stored logit {clear:.2e} frames {frames_w} lengths {lengths_w.tolist()}")
        assert clear > 1e-3
        mels, post, gates, al, lengths = run(stop_threshold=tau)
        torch.cuda.synchronize()
        _, ran = stored()
        n = mels.shape[1]
        assert lengths.cpu().tolist() == lengths_w.tolist() and n == frames_w
        keep = (torch.arange(n)[None, :] < lengths_w[:, None]).to(dev)
        assert torch.equal(mels, mels0[:, :n] * keep[:, :, None])
        assert torch.equal(gates, torch.where(keep[:, :, None], gates0[:, :n], torch.full_like(gates0[:, :n], -1000.0)))
        assert torch.equal(al, al0[:, :n])
        assert post.shape == mels.shape and bool(torch.isfinite(post).all())
        assert ran <= min(N, ((frames_w + CE - 1) // CE + 1) * CE), (ran, frames_w)
        if label == "all stop":
            assert frames_w <= 7 and ran < N and max(lengths_w.tolist()) < N
        else:
            assert frames_w == N and min(lengths_w.tolist()) < 5 and max(lengths_w.tolist()) == N
    with pytest.raises(ValueError, match="stop_threshold"):
        run(stop_threshold=1.0)
    # t2_decoder_infer refuses a stop_logit that is not finite before it launches anything (rc = 1)
    from tacotron2_amd import _lib
    a = eng._infer_group(0, torch.zeros(2, L, d["encoded_dim"], device=dev), lens[:2].to(dev), 4, None, None, False, None, None)["a"]
    for bad in (float("nan"), float("inf"), float("-inf")):
        a.stop_logit = bad
        with pytest.raises(_lib.T2Error, match="rc=1"):
            _lib.call("t2_decoder_infer", a, 0, 1, torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. drivers
# ---------------------------------------------------------------------------------------------------------------------------
def _infer_fixture(tmp_path, stop_threshold=None):
    """Checkpoint and config of the golden `infer` weights (small dims; the stop logit falls below zero within a few frames), as
    tests/test_gpu_cli.py's `test` case builds them."""
    import json
    from tests.helpers import load_golden, params_from
    from tests.test_gpu_cli import ALLOWED
    z = load_golden("infer")
    sd = {"tacotron2." + k: v for k, v in params_from(z).items()}
    hp = dict(lr=1e-3, weight_decay=1e-6, num_chars=39, encoded_dim=32, num_mels=16, prenet_dim=16, att_rnn_dim=32, att_dim=16,
              rnn_hidden_dim=32, postnet_dim=32, dropout=0.5)
    ck = tmp_path / "m.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hp, "global_step": 0, "epoch": 0}, ck)
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv", "test": "none.csv",
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "num_mels": 16}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "args": {"max_steps": 6}},
           "model": {"scheduler_milestones": [], "args": {"prenet_dim": 16, "att_rnn_dim": 32, "att_dim": 16, "rnn_hidden_dim": 32,
                                                          "postnet_dim": 32, "dropout": 0.5, "char_embedding_dim": 32}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    if stop_threshold is not None:
        cfg["model"]["stop_threshold"] = stop_threshold
    p = tmp_path / (f"cfg_{stop_threshold}.json")
    p.write_text(json.dumps(cfg))
    return ck, p, cfg


def _say(tmp_path, ck, cfgp, name, extra):
    """`main.py say` through its click entry in this process (option parsing, config, driver, decode; no interpreter start)."""
    import numpy as np
    from click.testing import CliRunner
    import main as cli
    out = tmp_path / f"{name}.npy"
    r = CliRunner().invoke(cli.main, ["--config", str(cfgp), "--device", "0", "say", "--checkpoint", str(ck), "--text",
                                      "A somewhat longer sentence, Dr. Who!", "--out", str(out), "--random-seed", "3"] + extra, obj={})
    assert r.exit_code == 0, (r.output, r.exception)
    return np.load(out)


def test_say_stop_threshold_orders_the_lengths_and_the_config_key_is_the_flag(tmp_path):
    import numpy as np
    ck, cfgp, _ = _infer_fixture(tmp_path)
    m5 = _say(tmp_path, ck, cfgp, "t5", [])
    m3 = _say(tmp_path, ck, cfgp, "t3", ["--stop-threshold", "0.3"])
    m7 = _say(tmp_path, ck, cfgp, "t7", ["--stop-threshold", "0.7"])
    print("say frames at 0.3 / 0.5 / 0.7:", len(m3), len(m5), len(m7))
    assert len(m3) >= len(m5) >= len(m7) >= 1
    assert np.array_equal(_say(tmp_path, ck, cfgp, "t5b", ["--stop-threshold", "0.5"]), m5)
    _, cfg3, _ = _infer_fixture(tmp_path, 0.3)
    assert np.array_equal(_say(tmp_path, ck, cfg3, "c3", []), m3)                                   # the config key alone
    assert np.array_equal(_say(tmp_path, ck, cfg3, "c3f", ["--stop-threshold", "0.7"]), m7)         # the command line wins
    from click.testing import CliRunner
    import main as cli
    r = CliRunner().invoke(cli.main, ["--config", str(cfgp), "say", "--checkpoint", str(ck), "--text", "x", "--stop-threshold", "1"],
                           obj={})
    assert r.exit_code == 2 and "0 < P < 1" in r.output


def test_test_driver_lengths_under_a_threshold_are_the_decode_lengths(tmp_path):
    """run/test.py's `mel_lengths` against the decode's own `lengths`, one utterance per decode (the reference's count rule counts
    on after an utterance's first stop while others still run; alone, `lengths` is the first stop): equal under a threshold, where
    the reference's `(gate < 0).argmax` would cut at the first kept frame with a logit in [logit(tau), 0)."""
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.run.test import load_test_model, mel_lengths_of
    from tests.test_gpu_cli import ALLOWED
    dev = _dev()
    ck, cfgp, cfg = _infer_fixture(tmp_path, 0.3)
    model = load_test_model(cfg["dataset"], cfg["training"], cfg["model"], cfg["extensions"], str(ck), dev, random_seed=3)
    assert model.stop_threshold == 0.3
    enc = TextEncoder(ALLOWED, "^", True)
    seen = []
    for text in ("Hi there.", "A somewhat longer sentence, Dr. Who!", "Testing: one; two? three."):
        ids = torch.tensor([enc.encode(text)], dtype=torch.int64, device=dev)
        n_ids = torch.tensor([ids.shape[1]], dtype=torch.int64, device=dev)
        for tau in (0.3, 0.4, 0.45, 0.49, 0.5, 0.7):
            model.tacotron2._calls = 0
            mels, post, gates, al, lengths = model.tacotron2._engine.infer(ids, n_ids, 40, seed=3, stop_threshold=tau)
            got = int(mel_lengths_of(gates, tau)[0])
            stopped = int(lengths[0]) < gates.shape[1]
            assert got == (int(lengths[0]) if stopped else 0), (text, tau, got, lengths.tolist(), gates[0, :, 0].tolist())
            seen.append((tau, int(lengths[0]), stopped))
    print("tau, lengths, stopped:", seen)
    assert any(s for _, _, s in seen)


def test_train_loss_options_flags_and_config_keys_give_the_same_steps(tmp_path):
    """`main.py train --mel-loss l1+l2 --masked-loss --stop-weight 8` for two steps on synthetic batches prints three finite terms;
    the config keys alone print the same numbers; both differ from the default loss."""
    import json
    import re
    from tests.test_gpu_cli import _cfg, _run

    def terms(out):
        rows = re.findall(r"training_gate_loss ([-\w.+]+) training_mel_loss ([-\w.+]+) training_mel_post_loss ([-\w.+]+)", out)
        assert len(rows) >= 1, out[-1500:]
        return [[float(v) for v in row] for row in rows]

    cfg = _cfg(tmp_path)
    base = ["--config", str(cfg), "--device", "0", "train", "--speech-dir", "unused", "--synthetic", "--max-steps", "2"]
    flags = terms(_run(base + ["--results-dir", str(tmp_path / "a"), "--mel-loss", "l1+l2", "--masked-loss", "--stop-weight", "8"]))
    c = json.loads(cfg.read_text())
    c["training"]["loss"] = {"mel": "l1+l2", "masked": True, "stop_weight": 8.0}
    cfg2 = tmp_path / "cfg_loss.json"
    cfg2.write_text(json.dumps(c))
    keys = terms(_run(["--config", str(cfg2)] + base[2:] + ["--results-dir", str(tmp_path / "b")]))
    plain = terms(_run(base + ["--results-dir", str(tmp_path / "c")]))
    print("flags", flags, "config", keys, "default", plain)
    # the options are not ignored: each of the three terms of the first step differs from the default loss's (same batch, same weights)
    assert all(abs(x - y) > 1e-3 * max(1.0, abs(y)) for x, y in zip(flags[0], plain[0])), (flags, plain)
    assert all(all(v == v and abs(v) < 1e6 for v in row) and len(row) == 3 for row in flags)
    assert len(flags) == len(keys)
    for a, b in zip(flags, keys):
        assert all(abs(x - y) <= 2e-5 * max(1.0, abs(y)) for x, y in zip(a, b)), (flags, keys)
