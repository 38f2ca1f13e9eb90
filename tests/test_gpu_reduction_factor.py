"""Reduction factor (r mel frames per decoder step) on the GPU: the grouped boundary kernels through the C ABI against a few lines
of torch (at r = 1 also bit for bit against the entry points without the suffix), the engine's training step and decode loop
against the float64 restatement (tests/reduction_ref.py), guard bands, the composition with forward and guided attention, r = 1
against an engine without the key, and the module / trainer / CLI surface."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import tacotron2_ref as R
from tests import reduction_ref as RR
from tests.helpers import dekink_masks
from tests.test_gpu_model import ZERO_GRADIENT_BY_CONSTRUCTION, _grad_check, build_engine, masks_to_device, random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MID = dict(num_chars=39, encoded_dim=128, prenet_dim=64, att_rnn_dim=256, att_dim=64, rnn_hidden_dim=256, postnet_dim=128,
           num_mels=80, dropout=0.5)
GUARD = 65536


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------
# boundary kernels through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(5, 2), (7, 3), (8, 2), (1, 2), (5, 1), (1, 1)]
B_K, M_K = 3, 80


def _behind_nan(t, dev):
    """`t` on the device as a view with NaN written behind its last element (a read past the end poisons the result)."""
    fill = float("nan") if t.is_floating_point() else 2 ** 30          # (integer inputs - the lengths: a large value behind them)
    flat = torch.full((t.numel() + 4096,), fill, dtype=t.dtype, device=dev)
    flat[:t.numel()] = t.reshape(-1).to(dev)
    return flat[:t.numel()].view(t.shape)


def _kernel_lens(T, r):
    """0, a length in the middle of a group (or 1 when T = 1; r = 1 has no middle), and T."""
    mid = min(T, r + 1) if r + 1 < T else max(T - 1, 1)
    assert T == 1 or r == 1 or mid % r != 0
    return torch.tensor([0, mid, T], dtype=torch.int32)


@pytest.mark.parametrize("T,r", KERNEL_CASES)
def test_teacher_pack_and_finalize_move_the_right_elements(T, r):
    from tacotron2_amd import _lib
    dev = _dev()
    B, M, S = B_K, M_K, RR.steps_of(T, r)
    g = torch.Generator().manual_seed(10 * T + r)
    lens = _kernel_lens(T, r)
    # teacher pack
    mel = torch.randn(B, T, M, generator=g)
    out = torch.full((S + 1, B, M), 7.0, device=dev)
    _lib.call("t2_mel_to_tm_r", _behind_nan(mel, dev), out, B, T, M, r, _st())
    want = torch.zeros(S + 1, B, M)
    for s, src in enumerate(RR.teacher_slots(T, r), start=1):
        if src is not None:
            want[s] = mel[:, src]
    assert torch.equal(out.cpu(), want)
    if r == 1:       # the entry point without the suffix on the same inputs: the same bits (here and below)
        out1 = torch.full((T + 1, B, M), 7.0, device=dev)
        _lib.call("t2_mel_to_tm", _behind_nan(mel, dev), out1, B, T, M, _st())
        assert torch.equal(out1, out)
    # finalize forward
    ld = r * M + 1
    proj = torch.randn(S, B, ld, generator=g)
    mels = torch.full((B, T, M), 7.0, device=dev); gates = torch.full((B, T, 1), 7.0, device=dev)
    post_in = torch.full((B, T + 4, M), 7.0, device=dev)
    _lib.call("t2_finalize_fwd_r", _behind_nan(proj, dev), ld, _behind_nan(lens, dev), mels, gates, post_in, B, T, M, r, _st())
    fr = proj[:, :, :r * M].reshape(S, B, r, M).permute(1, 0, 2, 3).reshape(B, S * r, M)[:, :T]      # frame s*r + j = block j of step s
    lg = proj[:, :, r * M].t()[:, :, None].expand(B, S, r).reshape(B, S * r)[:, :T]                  # the logit repeated
    mm = torch.arange(T)[None, :] >= lens[:, None]
    assert torch.equal(mels.cpu(), fr.masked_fill(mm[:, :, None], 0.0))
    assert torch.equal(gates.cpu()[:, :, 0], lg.masked_fill(mm, -1000.0))
    assert torch.equal(post_in.cpu()[:, 2:T + 2], fr) and float(post_in.cpu()[:, :2].abs().max()) == 0.0 \
        and float(post_in.cpu()[:, T + 2:].abs().max()) == 0.0
    if r == 1:
        mels1, gates1, post_in1 = torch.full_like(mels, 7.0), torch.full_like(gates, 7.0), torch.full_like(post_in, 7.0)
        _lib.call("t2_finalize_fwd", _behind_nan(proj, dev), ld, _behind_nan(lens, dev), mels1, gates1, post_in1, B, T, M, _st())
        assert torch.equal(mels1, mels) and torch.equal(gates1, gates) and torch.equal(post_in1, post_in)
    # finalize backward: its transpose, accumulating; the columns of frames >= T and the gate column stay
    dpost = torch.randn(B, T + 4, M, generator=g)
    base = torch.randn(S, B, ld, generator=g)
    dproj = base.clone().to(dev)
    _lib.call("t2_finalize_bwd_r", _behind_nan(dpost, dev), dproj, B, T, M, r, _st())
    want = base.clone()
    for t in range(T):
        want[t // r, :, (t % r) * M:(t % r + 1) * M] += dpost[:, t]          # (shifted rows b*Tp + t: row t of the padded layout)
    assert torch.equal(dproj.cpu(), want)
    if r == 1:
        dproj1 = base.clone().to(dev)
        _lib.call("t2_finalize_bwd", _behind_nan(dpost, dev), dproj1, B, T, M, _st())
        assert torch.equal(dproj1, dproj)


@pytest.mark.parametrize("T,r", KERNEL_CASES)
def test_outgrad_pack_sums_the_stop_logit_gradient_over_the_group(T, r):
    from tacotron2_amd import _lib
    dev = _dev()
    B, M, S = B_K, M_K, RR.steps_of(T, r)
    g = torch.Generator().manual_seed(20 * T + r)
    lens = _kernel_lens(T, r)
    dm, dp, dg = torch.randn(B, T, M, generator=g), torch.randn(B, T, M, generator=g), torch.randn(B, T, 1, generator=g)
    d_post_out = torch.full((B, T, M), 7.0, device=dev)
    dproj = torch.full((S, B, r * M + 1), 7.0, device=dev)
    _lib.call("t2_outgrad_pack_r", _behind_nan(dm, dev), _behind_nan(dp, dev), _behind_nan(dg, dev), _behind_nan(lens, dev),
              d_post_out, dproj, B, T, M, r, _st())
    live = (torch.arange(T)[None, :] < lens[:, None])[:, :, None].float()
    want_post = dp * live
    want = torch.zeros(S, B, r * M + 1)
    for t in range(T):
        want[t // r, :, (t % r) * M:(t % r + 1) * M] = (dm * live + dp * live)[:, t]
    for s in range(S):
        for j in range(r):            # in the kernel's order: one thread walks the group
            if s * r + j < T:
                want[s, :, r * M] += (dg * live)[:, s * r + j, 0]
    assert torch.equal(d_post_out.cpu(), want_post) and torch.equal(dproj.cpu(), want)
    if r == 1:       # the entry point without the suffix on the same inputs: the same bits
        d_post_out1, dproj1 = torch.full_like(d_post_out, 7.0), torch.full_like(dproj, 7.0)
        _lib.call("t2_outgrad_pack", _behind_nan(dm, dev), _behind_nan(dp, dev), _behind_nan(dg, dev), _behind_nan(lens, dev),
                  d_post_out1, dproj1, B, T, M, _st())
        assert torch.equal(d_post_out1, d_post_out) and torch.equal(dproj1, dproj)
    # the optional operands
    _lib.call("t2_outgrad_pack_r", None, _behind_nan(dp, dev), None, _behind_nan(lens, dev), d_post_out, dproj, B, T, M, r, _st())
    assert float(dproj.cpu()[:, :, r * M].abs().max()) == 0.0


@pytest.mark.parametrize("T,r", KERNEL_CASES)
def test_grouped_loss_kernel_matches_torch(T, r):
    """The three sums to the tolerance of the loss check in tests/test_gpu_model.py (rtol 1e-5, atol 1e-6 against float64), d_post and
    dproj to 1e-5 of their largest element; the gate column of dproj is the sum over the group's live frames."""
    from tacotron2_amd import _lib
    dev = _dev()
    B, M, S = B_K, M_K, RR.steps_of(T, r)
    g = torch.Generator().manual_seed(30 * T + r)
    lens = _kernel_lens(T, r)
    mm = (torch.arange(T)[None, :] >= lens[:, None])[:, :, None]
    raw = torch.randn(B, T, M, generator=g) - 2
    logit = torch.randn(B, S, 1, generator=g)[:, :, None, :].expand(B, S, r, 1).reshape(B, S * r, 1)[:, :T]
    mels = raw.masked_fill(mm, 0.0); post = (raw + 0.3 * torch.randn(B, T, M, generator=g)).masked_fill(mm, 0.0)
    gates = logit.masked_fill(mm, -1000.0)
    tgt = torch.randn(B, T, M, generator=g) - 2
    gtgt = (torch.rand(B, T, 1, generator=g) > 0.5).float()
    x = [v.double().requires_grad_(True) for v in (mels, post, gates)]
    tot, bce, ml, pl = R.tts_loss(x[0], x[1], x[2], tgt.double(), gtgt.double())
    gm, gp, gg = torch.autograd.grad(tot, x)
    live = (~mm).double()
    gm, gp, gg = gm * live, gp * live, gg * live            # masked positions are constants
    want = torch.zeros(S, B, r * M + 1, dtype=torch.float64)
    for t in range(T):
        want[t // r, :, (t % r) * M:(t % r + 1) * M] = (gm + gp)[:, t]
        want[t // r, :, r * M] += gg[:, t, 0]
    loss3 = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    d_post = torch.full((B, T, M), 7.0, device=dev); dproj = torch.full((S, B, r * M + 1), 7.0, device=dev)
    _lib.call("t2_loss_fwd_bwd_r", _behind_nan(mels, dev), _behind_nan(post, dev), _behind_nan(gates, dev), _behind_nan(tgt, dev),
              _behind_nan(gtgt, dev), _behind_nan(lens, dev), B, T, M, r, loss3, d_post, dproj, 1.0, _st())
    l3 = loss3.cpu()
    ref3 = torch.stack([bce, ml, pl]).detach()
    print(f"T {T} r {r}: loss3 {l3.tolist()} ref {ref3.tolist()}")
    assert torch.allclose(l3, ref3, rtol=1e-5, atol=1e-6)
    rel = lambda a, b: float((a.double().cpu() - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    print(f"  d_post {rel(d_post, gp):.2e}  dproj {rel(dproj, want):.2e}")
    assert rel(d_post, gp) < 1e-5 and rel(dproj, want) < 1e-5
    # the gate column is the group sum, and exactly zero where no frame of the group is live
    gcol = dproj.cpu()[:, :, r * M]
    for b in range(B):
        for s in range(S):
            if s * r >= int(lens[b]):
                assert float(gcol[s, b]) == 0.0
    # the r = 1 entry point on the same frames agrees on the three sums (one logit per frame there; double atomics: 1e-12), and at
    # r = 1, where it has the same inputs, on every bit of d_post and dproj
    loss1 = torch.empty(3, dtype=torch.float64, device=dev)
    d_post1 = torch.full((B, T, M), 7.0, device=dev); dproj1 = torch.full((T, B, M + 1), 7.0, device=dev)
    _lib.call("t2_loss_fwd_bwd", mels.to(dev), post.to(dev), gates.to(dev), tgt.to(dev), gtgt.to(dev), lens.to(dev), B, T, M, loss1,
              d_post1, dproj1, 1.0, _st())
    assert torch.allclose(loss1.cpu(), l3, rtol=1e-12, atol=0)
    if r == 1:
        assert torch.equal(d_post1, d_post) and torch.equal(dproj1, dproj)


def test_grouped_entries_reject_r_below_2():
    """The contract of the six `_r` entries, which was r >= 2 (hence the name) and is r >= 1.  r = 0 and r = -1 are refused with rc = 1 before anything is launched (every
    output keeps its fill); r = 1 is accepted."""
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
    for r in (0, -1):
        for name, args in (("t2_mel_to_tm_r", (x, outs[0], B, T, M, r)),
                           ("t2_finalize_fwd_r", (x, M + 1, lens, outs[0], outs[1], outs[2], B, T, M, r)),
                           ("t2_finalize_bwd_r", (x, outs[0], B, T, M, r)),
                           ("t2_outgrad_pack_r", (x, x, x, lens, outs[0], outs[1], B, T, M, r)),
                           ("t2_loss_fwd_bwd_r", (x, x, x, x, x, lens, B, T, M, r, loss3, outs[0], outs[1], 1.0)),
                           ("t2_stop_scan_r", (scan, r, 100, lengths, out2))):
            with pytest.raises(_lib.T2Error, match="rc=1"):
                _lib.call(name, *args, _st())
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((loss3 == 7.0).all())
    assert bool((lengths == -7).all()) and bool((out2 == -7).all())
    _lib.call("t2_mel_to_tm_r", x, outs[0], B, T, M, 1, _st())
    torch.cuda.synchronize()
    assert float(outs[0][:(T + 1) * B * M].abs().max()) == 0.0 and bool((outs[0][(T + 1) * B * M:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# engine step against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _step_masks(masks, T, r):
    """random_case's per-frame masks cut to the steps: prenet S + 1 rows, attention / decoder cells S rows; postnet per frame."""
    S = RR.steps_of(T, r)
    return dict(masks, prenet_drop=[m[:, :S + 1].contiguous() for m in masks["prenet_drop"]],
                att_drop=masks["att_drop"][:S].contiguous(), dec_drop=masks["dec_drop"][:S].contiguous())


@functools.lru_cache(maxsize=None)
def _model_case(B, L, T, r, seed, hook=False, controls=0):
    """(dims with the key, float32 parameters, case with step masks, float64 parameters with grad, restatement outputs, names,
    (r = 1 parameters, per-frame masks, controls (B, C) or None)).  controls: that many prosody controls (the extension is on)."""
    d = R.default_dims(**MID, controls=bool(controls), controls_dim=controls)
    ctl = torch.randn(B, controls, generator=torch.Generator().manual_seed(seed + 1)) if controls else None
    P1 = R.init_params(d, seed=5)
    P = RR.grouped_params(P1, d, r, seed=seed)
    ci, lens, mel, tl, gate, masks = random_case(d, B, L, T, seed, None)
    if r > 1 and all(int(x) % r == 0 for x in tl):      # at least one length in the middle of a group
        tl[0] -= 1
        mel[0, tl[0]:] = 0.0; gate[0, tl[0] - 1:] = 0.0
    assert r == 1 or any(int(x) % r != 0 for x in tl)
    m = _step_masks(masks, T, r)
    packed = torch.stack([mel[:, i] if i is not None else torch.zeros(B, d["num_mels"]) for i in RR.teacher_slots(T, r)], 1)
    m, _ = dekink_masks(P, d, ci, packed, m)             # ReLU-kink elements out of both sides (tests/helpers.py)
    Pc = {k: (v.double().clone().requires_grad_(True) if (v.is_floating_point() and not R.is_buffer(k)) else
              (v.double().clone() if v.is_floating_point() else v.clone())) for k, v in P.items()}
    names = [k for k, v in Pc.items() if v.requires_grad]
    m64 = {k: ([x.double() for x in v] if isinstance(v, list) else v.double()) for k, v in m.items()}
    o = RR.reduction_fwd(Pc, d, r, ci, lens, True, mel=mel.double(), mel_len=tl, training=True, masks=m64, new_stats={},
                         attention_hook=RR.forward_attention_hook if hook else None, controls=ctl.double() if controls else None)
    return dict(d, reduction_factor=r), P, (ci, lens, mel, tl, gate, m), Pc, o, names, (P1, masks, ctl)


def _ref_grads(c, total):
    Pc, names = c[3], c[5]
    gs = torch.autograd.grad(total, [Pc[k] for k in names], allow_unused=True, retain_graph=True)
    return {k: (torch.zeros_like(Pc[k]) if g is None else g) for k, g in zip(names, gs)}


def _hip_step(d, P, case, dev, chunk_bwd=None, guard_bytes=None, guided=None, **fkw):
    ci, lens, mel, tl, gate, masks = case
    eng, ps = build_engine(d, P, dev, guard_bytes=guard_bytes)
    if chunk_bwd is not None:
        eng.chunk_bwd = chunk_bwd
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev), **fkw)
    ps.grad.zero_()
    loss3 = eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev), guided=guided)
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    return eng, ps, outs, loss3


def _check_outputs(outs, o, label):
    mel_l1 = float((outs[0].cpu().double() - o[0].detach()).abs().mean())
    post_l1 = float((outs[1].cpu().double() - o[1].detach()).abs().mean())
    al = float((outs[3].cpu().double() - o[3].detach()).abs().max())
    print(f"reduction factor engine {label}: mel L1 {mel_l1:.2e}, post L1 {post_l1:.2e}, align max-abs {al:.2e}")
    for a, b in zip(outs, o):
        assert tuple(a.shape) == tuple(b.shape), (a.shape, b.shape)
    assert mel_l1 < 1e-4 and post_l1 < 1e-4 and al < 5e-5
    assert torch.equal(outs[2].cpu() == -1000.0, o[2].detach() == -1000.0)
    assert float((outs[2].cpu().double() - o[2].detach()).abs().max()) < 2e-4


def _grad_report(ps, grads, label):
    """_grad_check (the project's criterion) after printing the worst ratio (DESIGN.md 5.5 records it per shape)."""
    worst = (0.0, None)
    for name, g in ps.reference_layout(ps.G).items():
        if name in ZERO_GRADIENT_BY_CONSTRUCTION:
            continue
        ref = grads[name].double()
        err = float((g.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-3)
        if err > worst[0]:
            worst = (err, name)
    print(f"reduction factor gradients {label}: worst {worst[0]:.2e} of the tensor's largest element ({worst[1]})")
    _grad_check(ps, grads)


ENGINE_CASES = [(4, 33, 29, 2, None), (3, 300, 21, 3, None), (5, 40, 23, 2, 5), (33, 21, 10, 3, None)]


@pytest.mark.parametrize("B,L,T,r,chunk_bwd", ENGINE_CASES)
def test_engine_step_matches_the_float64_restatement(B, L, T, r, chunk_bwd):
    dev = _dev()
    c = _model_case(B, L, T, r, 200 + B)
    d, P, case, Pc, o, names, (P1, masks1, _) = c
    ci, lens, mel, tl, gate, masks = case
    S = RR.steps_of(T, r)
    tot, bce, ml, pl = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())
    grads = _ref_grads(c, tot)
    eng, ps, outs, loss3 = _hip_step(d, P, case, dev, chunk_bwd=chunk_bwd)
    label = f"(B,L,T,r)=({B},{L},{T},{r})"
    # the chains are sized by steps, the boundary by frames
    assert outs[3].shape == (B, S, L) and eng._ws["th"].numel() == S * B * 64 * ((L + 3) // 4 * 4)
    assert eng._ws["proj"].numel() == S * B * (r * 80 + 1) and eng._ws["xdec"].numel() == (S + 1) * B * (256 + 128)
    assert eng._ws["post.x0"].numel() == B * (T + 4) * 80
    _check_outputs(outs, o, label)
    ref3 = torch.stack([bce, ml, pl]).detach()
    assert torch.allclose(loss3.cpu(), ref3, rtol=1e-5, atol=1e-6), (loss3.cpu(), ref3)      # (tests/test_gpu_model.py's loss check)
    _grad_report(ps, grads, label)
    # r = 1 on the same inputs (per-frame masks, the M-row projection) is another model: far outside the tolerance
    d1 = {k: v for k, v in d.items() if k != "reduction_factor"}
    plain = _hip_step(d1, P1, (ci, lens, mel, tl, gate, masks1), dev, chunk_bwd=chunk_bwd)
    assert plain[2][3].shape == (B, T, L)
    n = "decoder.attention.v.weight"
    g0 = plain[1].reference_layout(plain[1].G)[n].cpu().double()
    assert float((g0 - grads[n]).abs().max()) > 30 * 3e-4 * float(grads[n].abs().max())


def test_engine_under_guard_bands():
    """r = 2, T = 7 (odd: the last step's second frame does not exist) with guard bands on every workspace, every output and the
    ParamStore's flat buffers: every band intact, outputs and gradients match."""
    dev = _dev()
    B, L, T, r = 3, 37, 7, 2
    c = _model_case(B, L, T, r, 211)
    d, P, case, Pc, o, names, _ = c
    tot = R.tts_loss(o[0], o[1], o[2], case[2].double(), case[4].double())[0]
    eng, ps, outs, _ = _hip_step(d, P, case, dev, guard_bytes=GUARD)
    assert eng.guard_bytes == GUARD and ps.guard_bytes == GUARD
    assert eng.guard_check() == [] and ps.guard_check() == []
    for name in ("mel_tm", "proj", "dproj", "p1", "xdec", "th", "post.x0", "out.mels", "out.gates", "out.align"):
        assert name in eng._guards, name
    S = RR.steps_of(T, r)
    assert eng._guards["proj"][2] == S * B * (r * 80 + 1) and eng._guards["mel_tm"][2] == (S + 1) * B * 80
    assert eng._guards["out.align"][2] == B * S * L and eng._guards["out.mels"][2] == B * T * 80
    _check_outputs(outs, o, "(3,37,7,2), guard bands")
    _grad_report(ps, _ref_grads(c, tot), "(3,37,7,2), guard bands")


# ---------------------------------------------------------------------------------------------------------------------------
# decoding
# ---------------------------------------------------------------------------------------------------------------------------
# (B, L, r, cap in frames, stop bias): bias chosen on the CPU restatement so that utterances stop at different steps, at least one
# before the cap and at least one not at all, every stop logit of the run at least 1e-3 from zero (asserted below)
DECODE_CASES = [(3, 19, 2, 21, -0.4545), (5, 33, 3, 25, -0.46)]


def _decode_case(B, L, r, cap, seed, bias, controls=0):
    d = R.default_dims(**MID, controls=bool(controls), controls_dim=controls)
    P = RR.grouped_params(R.init_params(d, seed=9), d, r, seed=seed)
    P["decoder.gate.weight"] = P["decoder.gate.weight"] * -40.0       # (the logits then fall along the utterance, and spread)
    P["decoder.gate.bias"] = P["decoder.gate.bias"] + bias
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(3, L // 2), L + 1, (B,), generator=g); lens[0] = L
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    S = RR.steps_of(cap, r)
    pm = (torch.rand(S + 1, 2, B, d["prenet_dim"], generator=g) >= 0.5).float() * 2
    return d, P, ci, lens, pm


def _decode_ref(d, P, r, ci, lens, pm, cap, hook=None, controls=None):
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        return RR.reduction_fwd(P64, d, r, ci, lens, False, max_len=cap, training=False,
                                masks=dict(prenet_drop=[[pm[i, 0].double(), pm[i, 1].double()] for i in range(pm.shape[0])]),
                                attention_hook=hook, controls=controls.double() if controls is not None else None)


def _check_decode(out, ref, r, cap, need_both=True):
    mels, post, gates, al, lengths = out
    rm, rp, rg, ra, rl = ref
    l1 = lambda a, b: float((a.double().cpu() - b).abs().mean())
    amax = float((al.double().cpu() - ra).abs().max())
    print(f"decode r {r} cap {cap}: mel L1 {l1(mels, rm):.3e} post L1 {l1(post, rp):.3e} align {amax:.3e} lengths {lengths.tolist()} "
          f"ref {rl.tolist()} frames {mels.shape[1]} steps {al.shape[1]}")
    if need_both:       # the case is what it claims (checked on the CPU when it was written)
        assert bool((rl < cap).any()) and bool((rl == cap).any()) and cap % r != 0
    live = rg[:, :, 0] != -1000.0
    assert float(rg[:, :, 0][live].abs().min()) > 1e-3          # no stop decision within float32's reach of zero
    assert mels.shape == rm.shape and post.shape == rp.shape and gates.shape == rg.shape and al.shape == ra.shape
    assert torch.equal(lengths.cpu(), rl)
    assert l1(mels, rm) < 1e-4 and l1(post, rp) < 1e-4 and amax < 5e-5
    assert torch.equal(gates.cpu() == -1000.0, rg == -1000.0)
    assert float((gates.cpu().double() - rg).abs().max()) < 2e-4


@pytest.mark.parametrize("B,L,r,cap,bias", DECODE_CASES)
def test_decode_matches_the_restatement(B, L, r, cap, bias):
    dev = _dev()
    d, P, ci, lens, pm = _decode_case(B, L, r, cap, 300 + B, bias)
    ref = _decode_ref(d, P, r, ci, lens, pm, cap)
    eng, ps = build_engine(dict(d, reduction_factor=r), P, dev)
    out = eng.infer(ci.to(dev), lens.to(dev), cap, prenet_masks=pm.to(dev).contiguous(), check_every=4)
    torch.cuda.synchronize()
    _check_decode(out, ref, r, cap)


def test_decode_that_ends_before_the_cap():
    """The first case with a lower stop bias: every utterance stops at step 5, the loop ends there - 12 frames, lengths 10."""
    dev = _dev()
    B, L, r, cap, _ = DECODE_CASES[0]
    d, P, ci, lens, pm = _decode_case(B, L, r, cap, 300 + B, -0.50)
    ref = _decode_ref(d, P, r, ci, lens, pm, cap)
    assert ref[0].shape[1] == 12 and ref[3].shape[1] == 6 and ref[4].tolist() == [10, 10, 10]
    eng, ps = build_engine(dict(d, reduction_factor=r), P, dev)
    out = eng.infer(ci.to(dev), lens.to(dev), cap, prenet_masks=pm.to(dev).contiguous(), check_every=4)
    torch.cuda.synchronize()
    _check_decode(out, ref, r, cap, need_both=False)


# ---------------------------------------------------------------------------------------------------------------------------
# prosody controls at r > 1: the per-utterance term of the (r*M)-row projection, its weight gradient, the decode loop's row term
# ---------------------------------------------------------------------------------------------------------------------------
def test_engine_step_with_controls_at_r2():
    dev = _dev()
    B, L, T, r, C = 3, 21, 9, 2, 3
    c = _model_case(B, L, T, r, 241, False, C)
    d, P, case, Pc, o, names, (_, _, ctl) = c
    assert P["decoder.mel_out.weight"].shape == (160, 256 + 128 + C)
    tot, bce, ml, pl = R.tts_loss(o[0], o[1], o[2], case[2].double(), case[4].double())
    eng, ps, outs, loss3 = _hip_step(d, P, case, dev, controls=ctl.to(dev))
    assert ps.P["decoder.mel_out.weight#controls"].shape == (160, C) and eng._ws["ctl.mel"].numel() == B * 161
    _check_outputs(outs, o, "(3,21,9,2) controls")
    assert torch.allclose(loss3.cpu(), torch.stack([bce, ml, pl]).detach(), rtol=1e-5, atol=1e-6)
    grads = _ref_grads(c, tot)
    _grad_report(ps, grads, "(3,21,9,2) controls")
    gc = grads["decoder.mel_out.weight"][:, 256 + 128:]           # the case drives the controls columns of every block
    assert float(gc[:80].abs().max()) > 1e-4 and float(gc[80:].abs().max()) > 1e-4


DECODE_CONTROLS_BIAS = -1.10      # (on the CPU restatement: the third utterance stops at step 4, 0.008 / 0.018 from zero; the others never)


def test_decode_with_controls_at_r2():
    """The decode loop's per-utterance row term at r = 2: [W_pre1 . cmel_b[last block] ; cmel_b ; 0] (Engine._infer_group)."""
    dev = _dev()
    B, L, r, cap, C = 3, 19, 2, 21, 3
    d, P, ci, lens, pm = _decode_case(B, L, r, cap, 311, DECODE_CONTROLS_BIAS, controls=C)
    ctl = 2.0 * torch.randn(B, C, generator=torch.Generator().manual_seed(312))
    ref = _decode_ref(d, P, r, ci, lens, pm, cap, controls=ctl)
    none = _decode_ref(d, P, r, ci, lens, pm, cap, controls=torch.zeros(B, C))
    n = min(ref[0].shape[1], none[0].shape[1])
    assert float((ref[0][:, :n] - none[0][:, :n]).abs().max()) > 1e-2         # the controls move the mels: the case tests the term
    eng, ps = build_engine(dict(d, reduction_factor=r), P, dev)
    out = eng.infer(ci.to(dev), lens.to(dev), cap, prenet_masks=pm.to(dev).contiguous(), check_every=4, controls=ctl.to(dev))
    torch.cuda.synchronize()
    _check_decode(out, ref, r, cap, need_both=False)


def test_decoder_submodule_step_at_r2():
    """`model.decoder(...)`, the one-step surface of the reference's Decoder, at r = 2 with controls: the (B, r*M) block of the step
    and its one stop logit against R.decoder_step (the tolerances of tests/test_gpu_model.py's sub-module checks)."""
    from tacotron2_amd.model import Tacotron2
    dev = _dev()
    C, r, B, L = 3, 2, 3, 13
    d = R.default_dims(**MID, controls=True, controls_dim=C)
    P = RR.grouped_params(R.init_params(d, seed=5), d, r, seed=7)
    kw = {k: d[k] for k in ("num_chars", "encoded_dim", "encoder_kernel_size", "num_mels", "prenet_dim", "att_rnn_dim", "att_dim",
                            "rnn_hidden_dim", "postnet_dim", "dropout", "controls", "controls_dim")}
    m = Tacotron2(**kw, device=dev, reduction_factor=r)
    m.load_state_dict(P)
    m.eval()
    g = torch.Generator().manual_seed(3)
    lens = torch.tensor([13, 9, 4])
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    Pd = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        mem, pmem = R.condition(Pd, d, R.encoder_fwd(Pd, ci, lens, False))
    mask = torch.arange(L)[None] >= lens[:, None]
    zr = lambda *s: (torch.randn(*s, generator=g) * 0.3)
    w0 = torch.softmax(torch.randn(B, L, generator=g), 1); cum0 = 1.5 * w0
    pre, ah, ac, cx, dh, dc, ctl = zr(B, 64), zr(B, 256), zr(B, 256), zr(B, 128), zr(B, 256), zr(B, 256), zr(B, C) * 5
    f = lambda t: t.float().to(dev)
    for xe in (ctl,):
        with torch.no_grad():
            rs = R.decoder_step(Pd, pre.double(), ah.double(), ac.double(), cx.double(), w0.double(), cum0.double().clone(), dh.double(),
                                dc.double(), mem, pmem, mask, None, None, extra_decoder_in=xe.double())
        gs = m.decoder(f(pre), (f(ah), f(ac)), f(cx), f(w0), f(cum0).clone(), (f(dh), f(dc)), f(mem), f(pmem), mask.to(dev),
                       extra_decoder_in=f(xe))
        assert gs[0].shape == (B, 160) and gs[1].shape == (B, 1)
        mx = lambda a, b: float((a.double().cpu() - b).abs().max())
        print(f"decoder sub-module at r = 2: block {mx(gs[0], rs[0]):.2e} gate {mx(gs[1], rs[1]):.2e}")
        assert mx(gs[0], rs[0]) < 5e-5 and mx(gs[1], rs[1]) < 5e-5 and mx(gs[6][0], rs[7]) < 2e-5
        # the gate is the gate row, not a row of mel_out; the two blocks are two frames
        assert float((rs[1][:, 0] - rs[0][:, 80]).abs().min()) > 1e-3 and float((rs[0][:, :80] - rs[0][:, 80:]).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the step scan through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_stop_scan_r_with_hand_set_logits():
    """Two groups (2 + 3 utterances), 5 stored steps, r = 3, M' = 6, ld_proj = 8, max_len = 13 (no multiple of r), logits set by hand:
    first negative steps (1, 3, never, 0, 2) -> the loop ends after step n* = 4 (someone never stops): 5 steps, min(15, 13) = 13
    frames; counted steps with logit >= 0 among the first 5: (3, 4, 5, 2, 3) -> lengths min(3 x, 13) = (9, 12, 13, 6, 9).  Then without
    the utterance that never stops: n* = 3, 4 steps, 12 frames, counted among the first 4: (3, 3, 2, 2) -> (9, 9, 6, 6).
    r = 1 (M' = 2, ld_proj = 4) with the same signs: a step is a frame, so lengths are the counts and out2 = {steps, steps} - what
    t2_stop_scan gives on the same logits but for its out2[1] = 0 - and a max_len of 3 cuts lengths and the frames emitted, not the steps."""
    from tacotron2_amd import _lib
    dev = _dev()
    N = 5
    sign = {0: [1, -1, 1, 1, -1], 1: [1, 1, 1, -1, 1], 2: [1, 1, 1, 1, 1], 3: [-1, 1, -1, 1, -1], 4: [1, 1, -1, -1, 1]}

    def run(utts, groups, max_len, r=3, plain=False):
        Mr, ld = 2 * r, 2 * r + 2
        projs, k = [], 0
        for Bg in groups:
            p = torch.full((N, Bg, ld), float("nan"))
            p[:, :, :Mr] = 0.25
            for b in range(Bg):
                p[:, b, Mr] = 0.5 * torch.tensor(sign[utts[k]], dtype=torch.float32); k += 1
            projs.append(_behind_nan(p, dev))
        scan = _lib.make("T2StopScan", proj=projs + [0] * (64 - len(projs)), Bg=list(groups) + [0] * (64 - len(groups)),
                         ngroups=len(groups), ld_proj=ld, M=Mr, nframes=N)
        lengths = torch.full((len(utts),), -7, dtype=torch.int64, device=dev)
        out2 = torch.full((2,), -7, dtype=torch.int32, device=dev)
        if plain:
            _lib.call("t2_stop_scan", scan, lengths, out2, _st())
        else:
            _lib.call("t2_stop_scan_r", scan, r, max_len, lengths, out2, _st())
        torch.cuda.synchronize()
        return lengths.cpu().tolist(), out2.cpu().tolist()
    assert run([0, 1, 2, 3, 4], (2, 3), 13) == ([9, 12, 13, 6, 9], [13, 5])
    assert run([0, 1, 3, 4], (2, 2), 13) == ([9, 9, 6, 6], [12, 4])
    assert run([0, 1, 3, 4], (4,), 100) == ([9, 9, 6, 6], [12, 4])           # one group, a cap that does not bind
    assert run([2], (1,), 14) == ([14], [14, 5])                             # never stops: the stored steps, cut at the cap
    with pytest.raises(_lib.T2Error, match="rc=1"):
        run([2], (1,), 0)
    # r = 1 against the entry point without the suffix, both group splits, a cap that does not bind
    for utts, groups, want, steps in (([0, 1, 2, 3, 4], (2, 3), [3, 4, 5, 2, 3], 5), ([0, 1, 3, 4], (2, 2), [3, 3, 2, 2], 4)):
        got_r, got = run(utts, groups, 100, r=1), run(utts, groups, None, r=1, plain=True)
        assert got_r == (want, [steps, steps]) and got == (want, [steps, 0])
    assert run([0, 1, 2, 3, 4], (2, 3), 3, r=1) == ([3, 3, 3, 2, 3], [3, 5])  # a cap that binds: lengths and frames cut, steps not


# ---------------------------------------------------------------------------------------------------------------------------
# composition with the attention options
# ---------------------------------------------------------------------------------------------------------------------------
def test_forward_attention_training_at_r2():
    dev = _dev()
    B, L, T, r = 4, 33, 15, 2
    c = _model_case(B, L, T, r, 221, True)
    d, P, case, Pc, o, names, _ = c
    tot = R.tts_loss(o[0], o[1], o[2], case[2].double(), case[4].double())[0]
    eng, ps, outs, _ = _hip_step(d, P, case, dev, forward_attention=True)
    assert "dprior" in eng._ws and outs[3].shape == (B, 8, L)
    _check_outputs(outs, o, "(4,33,15,2) forward attention")
    _grad_report(ps, _ref_grads(c, tot), "(4,33,15,2) forward attention")
    plain = _model_case(B, L, T, r, 221)                    # the case exercises the hook
    assert float((plain[4][3] - o[3]).detach().abs().max()) > 1e-2


def test_forward_attention_decoding_at_r2():
    dev = _dev()
    B, L, r, cap, bias = DECODE_CASES[0]
    d, P, ci, lens, pm = _decode_case(B, L, r, cap, 303, bias)
    ref = _decode_ref(d, P, r, ci, lens, pm, cap, hook=RR.forward_attention_hook)
    plain = _decode_ref(d, P, r, ci, lens, pm, cap)
    n = min(ref[3].shape[1], plain[3].shape[1])
    assert float((ref[3][:, :n] - plain[3][:, :n]).abs().max()) > 1e-2
    eng, ps = build_engine(dict(d, reduction_factor=r), P, dev)
    out = eng.infer(ci.to(dev), lens.to(dev), cap, prenet_masks=pm.to(dev).contiguous(), check_every=4, forward_attention=True)
    torch.cuda.synchronize()
    _check_decode(out, ref, r, cap, need_both=False)


def test_guided_attention_at_r2_uses_step_lengths():
    """The guided term over the returned (B, S, L) alignments with T_b = ceil(mel_len / 2): the engine's value equals the closed-form
    mask sum (float64, over the engine's own alignments), and differs from the sum taken with frame lengths."""
    dev = _dev()
    B, L, T, r = 4, 33, 29, 2
    c = _model_case(B, L, T, r, 204)
    d, P, case = c[0], c[1], c[2]
    ci, lens, mel, tl, gate, masks = case
    sigma, alpha = 0.4, 100.0
    eng, ps, outs, loss3 = _hip_step(d, P, case, dev, guided=(sigma, alpha))
    got = float(eng.guided_loss.cpu())
    want = RR.guided_mask_sum(outs[3].cpu(), lens, tl, r, sigma, alpha)
    frames = RR.guided_mask_sum(outs[3].cpu(), lens, tl, 1, sigma, alpha)
    print(f"guided term at r = 2: engine {got:.8f} closed form {want:.8f} (with frame lengths {frames:.8f})")
    tol = 1e-5 * max(1.0, abs(want))
    assert abs(got - want) < tol
    assert abs(frames - want) > 10 * tol                      # the case tells the two length rules apart
    assert eng._ws["guided.dalign"].numel() >= B * 15 * L and bool(torch.isfinite(ps.grad).all())
    # the term reaches the attention parameters: their gradients move against the step without it
    eng0, ps0, _, _ = _hip_step(d, P, case, dev)
    n = "decoder.attention.v.weight"
    assert float((ps.G[n] - ps0.G[n]).abs().max()) > 1e-3 * float(ps0.G[n].abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# off is off
# ---------------------------------------------------------------------------------------------------------------------------
def test_r1_is_the_engine_without_the_key():
    dev = _dev()
    d = R.default_dims(**MID)
    P = R.init_params(d, seed=5)
    case = random_case(d, 4, 33, 29, 101, None)
    res = []
    for dd in (d, dict(d, reduction_factor=1)):
        eng, ps, outs, loss3 = _hip_step(dd, P, case, dev)
        ws = {k: (v.numel(), v.dtype) for k, v in eng._ws.items()}
        res.append((ws, outs, eng, ps))
    assert res[0][0] == res[1][0]                               # workspace names and sizes
    assert torch.equal(res[0][1][3], res[1][1][3])              # alignments: the bit-reproducible output
    assert res[0][3].offsets == res[1][3].offsets and res[0][3].numel == res[1][3].numel
    assert res[1][2].r == 1 and res[0][1][3].shape == (4, 29, 33)


# ---------------------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------------------
def _module_batch(d, B, L, T, seed, dev):
    ci, lens, mel, tl, gate, _ = random_case(d, B, L, T, seed, None)
    data = {"chars_idx": ci.to(dev), "mel_spectrogram": mel.to(dev), "gate": gate.to(dev)}
    meta = {"chars_idx_len": lens.to(dev), "mel_spectrogram_len": tl.to(dev)}
    return data, meta


def test_tacotron2_module_autograd_with_a_loss_on_the_alignments():
    """Tacotron2(reduction_factor=2) through autograd with arbitrary upstream gradients on all four outputs, against the restatement
    differentiated with the same weights (eval-mode dropout masks supplied)."""
    from tacotron2_amd.model import Tacotron2
    dev = _dev()
    B, L, T, r = 3, 21, 9, 2
    c = _model_case(B, L, T, r, 231)
    d, P, (ci, lens, mel, tl, gate, masks), Pc, o, names, _ = c
    kw = {k: d[k] for k in ("num_chars", "encoded_dim", "encoder_kernel_size", "num_mels", "prenet_dim", "att_rnn_dim", "att_dim",
                            "rnn_hidden_dim", "postnet_dim", "dropout")}
    model = Tacotron2(**kw, device=dev, reduction_factor=2)
    model.load_state_dict(P)
    model.train()
    outs = model(ci.to(dev), lens.to(dev), True, mel.to(dev), tl.to(dev), dropout_masks=masks_to_device(masks, dev))
    S = RR.steps_of(T, r)
    assert outs[0].shape == (B, T, 80) and outs[2].shape == (B, T, 1) and outs[3].shape == (B, S, L)
    g = torch.Generator().manual_seed(5)
    W = [torch.randn(x.shape, generator=g) for x in outs]
    sum((x * w.to(dev)).sum() for x, w in zip(outs, W)).backward()
    torch.cuda.synchronize()
    total = sum((x * w.double()).sum() for x, w in zip(o, W))       # (masked positions are constants on both sides)
    grads = _ref_grads(c, total)
    _grad_report(model.store, grads, "(3,21,9,2) autograd, all four outputs")
    assert model.decoder.mel_out.weight.grad is not None and tuple(model.decoder.mel_out.weight.grad.shape) == (160, 256 + 128)


def test_ttsmodel_steps_and_one_trainer_step():
    from tacotron2_amd.model import TTSModel
    from tacotron2_amd.trainer import Trainer
    dev = _dev()
    d = R.default_dims(**MID)
    kw = {k: d[k] for k in ("num_chars", "encoded_dim", "encoder_kernel_size", "num_mels", "prenet_dim", "att_rnn_dim", "att_dim",
                            "rnn_hidden_dim", "postnet_dim", "dropout")}
    tm = TTSModel(lr=1e-3, weight_decay=1e-6, device=dev, reduction_factor=2, **kw)
    tm.guided_attention = (0.4, 1.0)
    data, meta = _module_batch(d, 4, 21, 13, 7, dev)
    tm.train()
    loss = tm.training_step((data, meta))
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(tm.tacotron2.store.grad).all())
    assert float(tm.tacotron2.decoder.mel_out.weight.grad.abs().max()) > 0
    val = tm.validation_step((data, meta))
    ml0, cl0 = int(meta["mel_spectrogram_len"][0]), int(meta["chars_idx_len"][0])
    assert bool(torch.isfinite(val["loss"])) and val["alignment"].shape == ((ml0 + 1) // 2, cl0)
    assert val["mel_spectrogram_pred"].shape == (ml0, 80) and val["gate_pred"].shape == (13, 1)
    # one fused trainer step on the same store
    tr = Trainer(tm.tacotron2.store, lr=1e-3, weight_decay=1e-6, guided_attention=(0.4, 1.0))
    before = tm.tacotron2.store.flat.clone()
    batch = dict(chars_idx=data["chars_idx"], chars_idx_len=meta["chars_idx_len"], mel_spectrogram=data["mel_spectrogram"],
                 mel_spectrogram_len=meta["mel_spectrogram_len"], gate=data["gate"])
    loss3, outs = tr.train_step(batch)
    torch.cuda.synchronize()
    tr.engine.check_persistent_kernels()
    assert bool(torch.isfinite(loss3).all()) and outs[3].shape == (4, 7, 21) and outs[0].shape == (4, 13, 80)
    assert not torch.equal(before, tm.tacotron2.store.flat) and bool(torch.isfinite(tm.tacotron2.store.flat).all())
    assert tr.engine._ws["mask.att"].numel() >= 7 * 4 * 256 and bool(torch.isfinite(tr.last_guided_loss).all())


def _cli(args, ok=True):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert (res.returncode == 0) == ok, res.stdout[-2000:] + res.stderr[-3000:]
    return res


def test_cli_train_then_say_and_the_mismatch_error(tmp_path):
    from tests.test_gpu_cli import ALLOWED
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv",
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "silence": 512,
                                         "trim": False, "num_mels": 80, "cache": True}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "precision": "16-mixed",
                        "args": {"max_steps": 6, "val_check_interval": 0.5}},
           "model": {"scheduler_milestones": [0.5, 0.75],
                     "args": {"prenet_dim": 32, "att_rnn_dim": 64, "att_dim": 32, "rnn_hidden_dim": 64, "postnet_dim": 64, "dropout": 0.5,
                              "char_embedding_dim": 64, "encoder_kernel_size": 5, "reduction_factor": 2}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    res = tmp_path / "res"
    out = _cli(["--config", str(p), "--device", "0", "train", "--speech-dir", "unused", "--results-dir", str(res), "--synthetic",
                "--max-steps", "2"]).stdout
    assert "training_loss" in out
    ck = torch.load(res / "final.ckpt", map_location="cpu", weights_only=True)
    assert ck["hyper_parameters"]["reduction_factor"] == 2
    assert ck["state_dict"]["tacotron2.decoder.mel_out.weight"].shape == (160, 64 + 64)
    assert ck["state_dict"]["tacotron2.decoder.gate.weight"].shape == (1, 64 + 64)
    npy = tmp_path / "say.npy"
    _cli(["--config", str(p), "--device", "0", "say", "--checkpoint", str(res / "final.ckpt"), "--text", "Hello there.", "--out",
          str(npy), "--random-seed", "3"])
    import numpy as np
    mel = np.load(npy)
    assert mel.ndim == 2 and mel.shape[1] == 80 and mel.shape[0] >= 1 and np.isfinite(mel).all()
    # a config whose r disagrees with the checkpoint: the error names both values
    cfg["model"]["args"]["reduction_factor"] = 3
    p.write_text(json.dumps(cfg))
    bad = _cli(["--config", str(p), "--device", "0", "say", "--checkpoint", str(res / "final.ckpt"), "--text", "Hello there.", "--out",
                str(npy)], ok=False)
    assert "written with reduction_factor = 2" in bad.stderr and "configured with reduction_factor = 3" in bad.stderr
