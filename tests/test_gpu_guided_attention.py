"""Alignment gradients and the guided-attention loss on the GPU, each through the C ABI:
 1. t2_guided_attn (value + gradient in one launch) against the float64 restatement of tests/test_guided_attention_host.py;
 2. the attention backward's new operand: alignment-ONLY gradients (d_post and dproj zero, only d_align) against the oracle's autograd;
 3. the guided term end to end through Engine.loss_and_grads, against the oracle and - at the shipped dims - by linearity;
 4. the module API (Tacotron2.forward's alignments are differentiable, TTSModel.guided_attention);
 5. the same alignment-only backward with guard bands on every workspace;
 6. `main.py train --guided-attention`.
At random initialisation the guided term's gradient is 2e-5 ... 3e-2 of the three-term gradient per tensor at alpha = 1, i.e. below the
gradient tolerance for most tensors: a test of the SUM of both would pass without the feature.  Hence the alignment path is driven
alone (2, 4, 5) or with alpha = 100 (3).

Tolerances.  Gradients: 3e-4 of each tensor's own largest reference element, the project's gradient tolerance.  The reference for
the alignment-only gradients is the oracle in float64 (its fp32 run is within 2e-5 of it, worst query_layer.weight at L = 300, so
either would stay well inside; but only in float64 are the three encoder conv biases in front of a training-mode BatchNorm - pure
cancellation residue - at 1e-17, below the 1e-12 under which a tensor is skipped; in fp32 they are 1e-8 of noise).  No absolute
floor otherwise; tensors without a path from the alignments (autograd returns None) must be exactly zero.  Measured worst ratios:
DESIGN.md section 5.2.  Kernel of 1: loss 1e-6 relative; dalign 5e-6 of its scale alpha * grad_scale / (B * N_b * T_b) (fp32 exp(-x)
is off by about x * e^-x ulps, a few 1e-7 of 1; the margin is for the argument's rounding); exact zeros outside the mask."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tacotron2_ref as R  # noqa: E402
from tests.test_gpu_cli import _cfg, _run  # noqa: E402
from tests.test_gpu_model import (ZERO_GRADIENT_BY_CONSTRUCTION, _dev, _grad_check, build_engine, masks_to_device,  # noqa: E402
                                  random_case)
from tests.test_guided_attention_host import guided_ref  # noqa: E402

GRAD_TOL = 3e-4
GUARD = 65536
MID = dict(num_chars=39, encoded_dim=128, prenet_dim=64, att_rnn_dim=256, att_dim=64, rnn_hidden_dim=256, postnet_dim=128,
           num_mels=80, dropout=0.5)
ATTENTION_TENSORS = ("att_encoder.weight", "decoder.attention.query_layer.weight", "decoder.attention.v.weight",
                     "decoder.attention.location_conv.weight", "decoder.attention.location_dense.weight")
NO_PATH_PREFIXES = ("decoder.lstm.", "decoder.mel_out.", "decoder.gate.", "postnet.")


def _guided_kernel(align, chars_len, mel_len, sigma, alpha, grad_scale=1.0, want_grad=True):
    """t2_guided_attn through the C ABI -> (loss float64[1], dalign or None), both on the device."""
    from tacotron2_amd._lib import call
    B, T, L = align.shape
    loss = torch.full((1,), float("nan"), dtype=torch.float64, device=align.device)
    da = torch.full((B, T, L), float("nan"), device=align.device) if want_grad else None
    call("t2_guided_attn", align, chars_len.to(torch.int32), mel_len.to(torch.int32), B, T, L, float(sigma), float(alpha), loss, da,
         float(grad_scale), torch.cuda.current_stream().cuda_stream)
    return loss, da


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _simplex_case(B, L, T, seed):
    """Seeded random simplex rows with ragged lengths: the longest text / mel fill the padded shape, and from B = 5 on the batch holds
    N_b = 1, T_b = 1 and (B = 33) an empty utterance."""
    g = torch.Generator().manual_seed(seed)
    w = torch.softmax(torch.randn(B, T, L, generator=g) * 2, -1)
    cl = torch.randint(1, L + 1, (B,), generator=g)
    ml = torch.randint(1, T + 1, (B,), generator=g)
    cl[0] = L; ml[-1] = T
    if B >= 5:
        cl[1] = 1; ml[2] = 1; ml[1] = T
    if B >= 33:
        cl[7] = 0
    return w, cl, ml


def _check_kernel(w, cl, ml, sigma, alpha, gs, dev):
    loss, da = _guided_kernel(w.to(dev), cl.to(dev), ml.to(dev), sigma, alpha, gs)
    rl, rda, scale = guided_ref(w.double(), cl, ml, sigma, alpha, gs)
    loss, da = float(loss.cpu()), da.cpu().double()
    rel = abs(loss - float(rl)) / max(abs(float(rl)), 1e-300)
    live = scale > 0
    err = ((da - rda).abs().amax((1, 2))[live] / scale[live]).max() if bool(live.any()) else torch.zeros(())
    print(f"guided kernel B={w.shape[0]} T={w.shape[1]} L={w.shape[2]} sigma={sigma}: loss rel {rel:.2e}, dalign/scale {float(err):.2e}")
    assert rel < 1e-6, (loss, float(rl))
    assert float(err) < 5e-6
    assert bool((da[rda == 0] == 0).all()) and bool(torch.isfinite(da).all())     # exact zeros outside [0,T_b) x [0,N_b)
    return loss, da


@pytest.mark.parametrize("sigma", [0.4, 0.05])
@pytest.mark.parametrize("T", [1, 29])
@pytest.mark.parametrize("L", [1, 33, 300])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_guided_kernel_matches_the_float64_restatement(B, L, T, sigma):
    dev = _dev()
    w, cl, ml = _simplex_case(B, L, T, 1000 * B + 10 * L + T)
    assert int(cl.max()) == L and int(ml.max()) == T
    if B >= 5:
        assert int(cl[1]) == 1 and int(ml[2]) == 1 and int(ml[1]) == T
    _check_kernel(w, cl, ml, sigma, 1.0, 1.0, dev)
    if B == 5 and L == 33:
        _check_kernel(w, cl, ml, sigma, 100.0, 0.25, dev)                      # alpha and grad_scale scale the gradient, alpha the loss
        # the loss alone (no gradient output) is the same launch with a null pointer
        l0, none = _guided_kernel(w.to(dev), cl.to(dev), ml.to(dev), sigma, 1.0, want_grad=False)
        assert none is None and abs(float(l0.cpu()) - float(guided_ref(w.double(), cl, ml, sigma, 1.0)[0])) < 1e-6 * float(l0.cpu())


def test_guided_kernel_batch_is_the_mean_of_its_equal_shards():
    """What the per-utterance normalisation was chosen for: loss and dalign of a batch of 6 are the mean of those of its two halves of
    3 at the same padded (L, T) - a data-parallel step of two ranks averages the ranks' gradients."""
    dev = _dev()
    w, cl, ml = _simplex_case(6, 33, 29, 77)
    cl[0], ml[5] = 20, 11                        # (the halves do not both contain the longest text / mel: the padding is shared)
    cl[4], ml[0] = 33, 29
    l6, d6 = _check_kernel(w, cl, ml, 0.4, 1.0, 1.0, dev)
    la, da = _check_kernel(w[:3], cl[:3], ml[:3], 0.4, 1.0, 1.0, dev)
    lb, db = _check_kernel(w[3:], cl[3:], ml[3:], 0.4, 1.0, 1.0, dev)
    assert abs(l6 - 0.5 * (la + lb)) < 1e-6 * abs(l6)
    scale6 = guided_ref(w.double(), cl, ml, 0.4, 1.0)[2]
    halves = 0.5 * torch.cat([da, db])
    assert float(((d6 - halves).abs().amax((1, 2)) / scale6).max()) < 5e-6


# ---------------------------------------------------------------------------------------------------------------------------
# 2. alignment-only gradients against the oracle's autograd
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(B, L, T, seed, pseed=5, dtype=torch.float64):
    """MID dims, random_case(seed): parameters, inputs and the oracle's training-mode forward with its autograd graph (kept: several
    tests differentiate different functions of its outputs).  The oracle runs in float64 unless asked otherwise: for alignment-only
    gradients the three encoder conv biases in front of a training-mode BatchNorm are pure cancellation residue - 1e-17 in float64,
    under the 1e-12 rule that skips them, but 1e-8 in fp32, where they would be compared as if they were signal."""
    d = R.default_dims(**MID)
    P = R.init_params(d, seed=pseed)
    case = random_case(d, B, L, T, seed, None)
    ci, lens, mel, tl, gate, masks = case
    cast = lambda v: v.to(dtype) if v.is_floating_point() else v
    Pc = {k: (cast(v).clone().requires_grad_(True) if (v.is_floating_point() and not R.is_buffer(k)) else cast(v).clone())
          for k, v in P.items()}
    m64 = {k: ([cast(x) for x in v] if isinstance(v, list) else cast(v)) for k, v in masks.items()}
    o = R.tacotron2_fwd(Pc, d, ci, lens, True, cast(mel), tl, training=True, masks=m64, new_stats={})
    names = [k for k, v in Pc.items() if v.requires_grad]
    return d, P, case, Pc, o, names


def _oracle_grads(c, fn, zeros=False):
    """autograd.grad of fn(oracle outputs) w.r.t. every parameter; a tensor without a path is None, or zeros on request."""
    d, P, case, Pc, o, names = c
    gs = torch.autograd.grad(fn(o), [Pc[k] for k in names], allow_unused=True, retain_graph=True)
    return {k: (torch.zeros_like(Pc[k]) if (g is None and zeros) else g) for k, g in zip(names, gs)}


def _dense_weight(B, T, L, seed):
    return torch.randn(B, T, L, generator=torch.Generator().manual_seed(seed))


def _align_only_check(ps, ref, label):
    """Every tensor with a path within GRAD_TOL of its own largest reference element; every tensor without one exactly zero.
    Returns the worst ratio (printed: DESIGN.md section 5.2 records it per shape)."""
    worst, bad, npath = (0.0, None), [], 0
    for name, g in ps.reference_layout(ps.G).items():
        got = g.double().cpu()
        r = ref[name]
        if r is None:
            assert name.startswith(NO_PATH_PREFIXES), name
            if float(got.abs().max()) != 0.0:
                bad.append((name, "no path from the alignments, but", float(got.abs().max())))
            continue
        assert not name.startswith(NO_PATH_PREFIXES), name
        scale = float(r.abs().max())
        if scale < 1e-12:
            continue
        npath += 1
        err = float((got - r.double()).abs().max()) / scale
        if err > worst[0]:
            worst = (err, name)
        if not err <= GRAD_TOL:
            bad.append((name, err, scale))
    print(f"alignment-only gradients {label}: worst {worst[0]:.2e} of the tensor's largest element ({worst[1]}), {npath} tensors")
    assert npath >= 20 and all(ref[n] is not None and float(ref[n].abs().max()) > 1e-12 for n in ATTENTION_TENSORS)
    assert not bad, bad[:8]
    return worst


def _hip_align_only(c, d_align_fn, dev, chunk_bwd=None, guard_bytes=None):
    """forward_tf + backward_tf(ctx, zeros, zeros, d_align=d_align_fn(outs, ctx)) -> (engine, ParamStore, outs)."""
    d, P, (ci, lens, mel, tl, gate, masks) = c[0], c[1], c[2]
    eng, ps = build_engine(d, P, dev, guard_bytes=guard_bytes)
    if chunk_bwd is not None:
        eng.chunk_bwd = chunk_bwd
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev))
    B, T, M = outs[0].shape
    ps.grad.zero_()
    eng.backward_tf(ctx, torch.zeros(B, T, M, device=dev), torch.zeros(T, B, M + 1, device=dev), d_align=d_align_fn(outs, ctx))
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    return eng, ps, outs


@pytest.mark.parametrize("B,L,T,seed,chunk_bwd", [(4, 33, 29, 101, None), (3, 300, 21, 101, None), (5, 40, 23, 103, 5),
                                                   (33, 21, 9, 104, None)])
def test_alignment_only_gradients_match_the_oracle(B, L, T, seed, chunk_bwd):
    """backward_tf(ctx, zeros, zeros, d_align=R) against autograd.grad((aligns * R).sum(), params) of the oracle: a dense seeded randn
    weight R, and the guided mask (the kernel's own dalign against the restated loss).  (3, 300, 21): the tiled per-slice kernel and the
    second round of the dw kernel's position loop; chunk_bwd = 5 at T = 23: five backward chunks, the operand indexed by the absolute
    frame; B = 33: three 16-row tiles."""
    dev = _dev()
    c = _oracle_case(B, L, T, seed)
    lens, tl = c[2][1], c[2][3]
    assert int(lens.max()) == L and int(tl.max()) == T and (B == 1 or int(tl.min()) < T)      # frames behind mel_len count too
    Rw = _dense_weight(B, T, L, seed + 1)
    ref = _oracle_grads(c, lambda o: (o[3] * Rw).sum())
    eng, ps, outs = _hip_align_only(c, lambda outs, ctx: Rw.to(dev), dev, chunk_bwd=chunk_bwd)
    assert float((outs[3].cpu() - c[4][3].detach()).abs().max()) < 2e-5
    if chunk_bwd is not None:
        from tacotron2_amd.engine import _chunk_sizes
        assert len(_chunk_sizes(T, chunk_bwd)) >= 4
    _align_only_check(ps, ref, f"(B,L,T)=({B},{L},{T}) randn")
    # the guided mask as the upstream gradient: t2_guided_attn's dalign on the HIP side, autograd of the restated loss on the other
    ref = _oracle_grads(c, lambda o: guided_ref(o[3], lens, tl, 0.4, 1.0)[0])
    eng, ps, outs = _hip_align_only(c, lambda outs, ctx: _guided_kernel(outs[3], ctx["len32"], ctx["mlen32"], 0.4, 1.0)[1], dev,
                                    chunk_bwd=chunk_bwd)
    _align_only_check(ps, ref, f"(B,L,T)=({B},{L},{T}) guided mask")


def test_backward_refuses_an_alignment_gradient_it_cannot_index():
    """d_align reaches the dw kernel as a raw pointer with the alignments' strides: another shape, dtype, layout or device is a
    ValueError before any launch."""
    dev = _dev()
    c = _oracle_case(4, 33, 29, 101)
    d, P, (ci, lens, mel, tl, gate, masks) = c[0], c[1], c[2]
    eng, ps = build_engine(d, P, dev)
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev))
    B, T, L, M = 4, 29, 33, d["num_mels"]
    z = (torch.zeros(B, T, M, device=dev), torch.zeros(T, B, M + 1, device=dev))
    good = torch.zeros(B, T, L, device=dev)
    for bad, what in [(good[:, :, :32], "shape"), (good.double(), "float32"), (good.cpu(), "cpu"),
                      (torch.zeros(B, L, T, device=dev).transpose(1, 2), "contiguous"), (good.tolist(), "float32"),
                      (torch.zeros(T, B, L, device=dev), "shape")]:
        with pytest.raises(ValueError, match=what):
            eng.backward_tf(ctx, *z, d_align=bad)
    ps.grad.zero_()
    eng.backward_tf(ctx, *z, d_align=good)           # the forward is still live: nothing was consumed by the refusals
    torch.cuda.synchronize()
    assert float(ps.grad.abs().max()) == 0.0         # and a zero upstream gradient is a zero gradient, exactly


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the guided term end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_loss_and_grads_with_the_guided_term_matches_the_oracle():
    """loss_and_grads(..., guided=(0.4, 100.0)) at (4, 33, 29) against the oracle's tts_loss + guided: each of the four values, every
    gradient with the relative-to-scale rule of test_train_step_midsize_matches_oracle.  alpha = 100 puts the term at the size of the
    other three for the attention tensors: the comparison fails if the term is dropped (asserted below, not assumed)."""
    dev = _dev()
    c = _oracle_case(4, 33, 29, 101, dtype=torch.float32)        # (the fp32 oracle, as test_train_step_midsize_matches_oracle)
    d, P, (ci, lens, mel, tl, gate, masks), Pc, o, names = c
    total3, bce, mel_l, post_l = R.tts_loss(o[0], o[1], o[2], mel, gate)
    gl = guided_ref(o[3], lens, tl, 0.4, 100.0)[0]
    grads = _oracle_grads(c, lambda o_: total3 + gl)
    grads3 = _oracle_grads(c, lambda o_: total3)
    eng, ps = build_engine(d, P, dev)
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev))
    ps.grad.zero_()
    loss3 = eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev), guided=(0.4, 100.0))
    torch.cuda.synchronize()
    assert loss3.shape == (3,) and eng.guided_loss.shape == (1,) and eng.guided_loss.dtype == torch.float64
    got = [float(x) for x in loss3.cpu()] + [float(eng.guided_loss.cpu())]
    want = [float(bce), float(mel_l), float(post_l), float(gl)]
    print("four terms (gate, mel, post, guided):", got, "oracle:", want)
    for g_, w_ in zip(got, want):
        assert abs(g_ - w_) < 2e-5 * max(1.0, abs(w_)), (got, want)
    assert abs(sum(got) - float(total3 + gl)) < 2e-5 * max(1.0, abs(float(total3 + gl)))
    _grad_check(ps, grads)
    # without the term the attention tensors are far outside the tolerance: the case does test it
    for n in ATTENTION_TENSORS:
        assert float((grads[n] - grads3[n]).abs().max()) > 100 * GRAD_TOL * max(float(grads[n].abs().max()), 1e-3), n
    # off again: the fourth value is gone and the three-term gradients are back
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev))
    ps.grad.zero_()
    eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev))
    torch.cuda.synchronize()
    assert eng.guided_loss is None
    _grad_check(ps, grads3)


def test_guided_term_is_linear_in_the_gradient_at_the_shipped_dims():
    """Vanilla dims, B = 8, L = 188, T = 120, alpha = 100, no oracle: gradients(guided on) - gradients(guided off), same masks, against
    the alignment-only gradients of the kernel's dalign.  The difference of two full gradients carries the rounding of the full
    gradient: bound 3e-4 of max|g_off| per tensor; the comparison counts only where max|g_align| >= 10 x that bound, and the five
    attention tensors must be among those.  The three encoder conv biases in front of a training-mode BatchNorm take no part: they
    have no gradient in any of the three runs, what each run stores for them is its own cancellation residue, so max|g_off| is not a
    scale of anything there (tests/test_gpu_model.py: ZERO_GRADIENT_BY_CONSTRUCTION)."""
    dev = _dev()
    d = R.default_dims()
    P = R.init_params(d, seed=21)
    B, L, T = 8, 188, 120
    ci, lens, mel, tl, gate, masks = random_case(d, B, L, T, 211, dev)
    eng, ps = build_engine(d, P, dev)
    args = (ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev))
    dm = masks_to_device(masks, dev)
    M = d["num_mels"]

    def run(back):
        outs, ctx = eng.forward_tf(*args, training=True, masks=dm)
        ps.grad.zero_()
        back(outs, ctx)
        torch.cuda.synchronize()
        eng.check_persistent_kernels()
        return {k: v.clone() for k, v in ps.reference_layout(ps.G).items()}
    g_off = run(lambda outs, ctx: eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev)))
    g_on = run(lambda outs, ctx: eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev), guided=(0.4, 100.0)))
    g_al = run(lambda outs, ctx: eng.backward_tf(ctx, torch.zeros(B, T, M, device=dev), torch.zeros(T, B, M + 1, device=dev),
                                                 d_align=_guided_kernel(outs[3], ctx["len32"], ctx["mlen32"], 0.4, 100.0)[1]))
    counted, bad = [], []
    for n in g_off:
        if n in ZERO_GRADIENT_BY_CONSTRUCTION:
            continue
        bound = GRAD_TOL * float(g_off[n].abs().max())
        size = float(g_al[n].abs().max())
        if size >= 10 * bound and bound > 0:
            counted.append(n)
            err = float(((g_on[n].double() - g_off[n].double()) - g_al[n].double()).abs().max())
            print(f"linearity {n}: |g_align|/|g_off| {size / (bound / GRAD_TOL):.3f}, error {err / (bound / GRAD_TOL):.2e} of max|g_off|")
            if not err <= bound:
                bad.append((n, err, bound))
    assert all(n in counted for n in ATTENTION_TENSORS), counted
    assert not bad, bad


def test_trainer_step_exposes_the_term_without_a_host_read():
    """Trainer(guided_attention=...): train_step returns what it returned before (loss3, outs) and keeps the fourth value as a device
    tensor (`last_guided_loss`) - with torch's sync-debug mode on "error" around the step, so no host read hides on the step path -
    equal to the restated value of the step's own alignments; the term changes the update of the attention parameters; off again,
    nothing of it is left."""
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.trainer import Trainer
    dev = _dev()
    d = R.default_dims(**MID)
    P = R.init_params(d, seed=5)
    ci, lens, mel, tl, gate, masks = random_case(d, 4, 33, 29, 101, dev)
    batch = dict(chars_idx=ci.to(dev), chars_idx_len=lens.to(dev), mel_spectrogram=mel.to(dev), mel_spectrogram_len=tl.to(dev),
                 gate=gate.to(dev))
    dm = masks_to_device(masks, dev)
    after = {}
    for tag, guided in (("off", None), ("on", (0.4, 100.0))):
        ps = ParamStore(d, dev)
        ps.load_state_dict(P)
        tr = Trainer(ps, lr=1e-3, weight_decay=1e-6, guided_attention=guided)
        tr.train_step(batch, masks=dm)                                  # (allocations and the first-call set-up may synchronise)
        ps.load_state_dict(P); tr.global_step = 0
        ps.exp_avg.zero_(); ps.exp_avg_sq.zero_()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss3, outs = tr.train_step(batch, masks=dm)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert loss3.shape == (3,) and len(outs) == 4
        if guided is None:
            assert tr.last_guided_loss is None and not [n for n in tr.engine._ws if n.startswith("guided")]
        else:
            assert tr.last_guided_loss.is_cuda and tr.last_guided_loss.dtype == torch.float64
            want = float(guided_ref(outs[3].cpu().double(), lens, tl, *guided)[0])
            assert abs(float(tr.last_guided_loss.cpu()) - want) < 1e-6 * want and want > 0.1
        after[tag] = ps.P["decoder.attention.v.weight"].clone()
    assert float((after["on"] - after["off"]).abs().max()) > 1e-4        # Adam's first update is ~lr * sign(g): the sign pattern moved


# ---------------------------------------------------------------------------------------------------------------------------
# 4. module API
# ---------------------------------------------------------------------------------------------------------------------------
def _module(c, dev):
    from tacotron2_amd.model import Tacotron2
    d, P = c[0], c[1]
    m = Tacotron2(device=dev, **{k: d[k] for k in ("num_chars", "encoded_dim", "encoder_kernel_size", "num_mels", "prenet_dim",
                                                   "att_rnn_dim", "att_dim", "rnn_hidden_dim", "postnet_dim", "dropout")})
    m.load_state_dict(P)
    m.train()
    return m


def test_module_alignments_are_differentiable():
    """(alignment * R).sum().backward() through Tacotron2.forward fills .grad as the engine path does (2); a loss on mels_post alone
    creates no alignment-gradient workspace and gives the oracle's gradients of that loss, as before."""
    dev = _dev()
    c = _oracle_case(4, 33, 29, 101)
    d, P, (ci, lens, mel, tl, gate, masks) = c[0], c[1], c[2]
    m = _module(c, dev)
    dm = masks_to_device(masks, dev)
    Rw = _dense_weight(4, 29, 33, 102)
    mels, post, gates, al = m(ci.to(dev), lens.to(dev), True, mel.to(dev), tl.to(dev), dropout_masks=dm)
    assert al.requires_grad and al.grad_fn is not None
    (al * Rw.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.equal(p.grad, m.store.G[n]) for n, p in m.named_parameters())
    _align_only_check(m.store, _oracle_grads(c, lambda o: (o[3] * Rw).sum()), "module API, (4,33,29) randn")
    # a loss that does not touch the alignments: None reaches the node, no (B,T,L) gradient buffer exists anywhere in the engine
    m.zero_grad()
    before = set(m._engine._ws)
    mels, post, gates, al = m(ci.to(dev), lens.to(dev), True, mel.to(dev), tl.to(dev), dropout_masks=dm)
    torch.nn.functional.mse_loss(post, mel.to(dev)).backward()
    torch.cuda.synchronize()
    names = set(m._engine._ws)
    assert names == before, names - before
    assert not [n for n in names if "dalign" in n or n.startswith("guided")], names
    _grad_check(m.store, _oracle_grads(c, lambda o: ((o[1] - mel) ** 2).mean(), zeros=True))
    # all four outputs in one loss
    m.zero_grad()
    mels, post, gates, al = m(ci.to(dev), lens.to(dev), True, mel.to(dev), tl.to(dev), dropout_masks=dm)
    (torch.nn.functional.mse_loss(post, mel.to(dev)) + 50.0 * (al * Rw.to(dev)).sum() / al.numel()).backward()
    torch.cuda.synchronize()
    _grad_check(m.store, _oracle_grads(c, lambda o: ((o[1] - mel) ** 2).mean() + 50.0 * (o[3] * Rw).sum() / o[3].numel(), zeros=True))


def test_ttsmodel_guided_attention_joins_the_validation_and_training_loss():
    """TTSModel.guided_attention = (0.4, 1.0) on the reference-generated eval fixture (dropout 0: deterministic):
    validation_step()["loss"] = the three terms + the restated guided value of the model's own alignment output."""
    from tacotron2_amd.model import TTSModel
    from tests.helpers import SMALL, load_golden, params_from
    dev = _dev()
    z = load_golden("tf_eval")
    tm = TTSModel(lr=1e-3, weight_decay=1e-6, num_chars=39, dropout=0.0, device=dev, **{k: v for k, v in SMALL.items() if k != "num_chars"})
    tm.tacotron2.load_state_dict(params_from(z))
    tm.eval()
    t = lambda k: torch.from_numpy(z[k]).to(dev)
    batch = ({"chars_idx": t("chars_idx"), "mel_spectrogram": t("mel"), "gate": t("gate")},
             {"chars_idx_len": t("chars_len"), "mel_spectrogram_len": t("mel_len")}, {})
    three = float(tm.validation_step(batch, 0)["loss"])
    with torch.no_grad():
        al = tm(t("chars_idx"), t("chars_len"), True, t("mel"), t("mel_len"))[3]
    gl = float(guided_ref(al.cpu().double(), torch.from_numpy(z["chars_len"]), torch.from_numpy(z["mel_len"]), 0.4, 1.0)[0])
    assert gl > 1e-2                                  # (an untrained model attends almost uniformly: the term is far above the tolerance)
    tm.guided_attention = (0.4, 1.0)
    out = tm.validation_step(batch, 0)
    assert abs(float(out["loss"]) - (three + gl)) < 1e-5 * max(1.0, three + gl), (float(out["loss"]), three, gl)
    assert "guided_attention" not in tm.hparams
    # training_step: the same sum, and its backward reaches the attention parameters through the alignments
    tm.train()
    tm.guided_attention = (0.4, 1000.0)
    loss = tm.training_step(batch, 0)
    loss.backward()
    g_on = tm.tacotron2.store.G["decoder.attention.v.weight"].clone()
    tm.guided_attention = None
    tm.zero_grad()
    tm.tacotron2._calls -= 1                          # the same Philox prenet masks as the step above
    loss0 = tm.training_step(batch, 0)
    loss0.backward()
    torch.cuda.synchronize()
    g_off = tm.tacotron2.store.G["decoder.attention.v.weight"]
    assert float(loss) - float(loss0) > 10.0 and bool(torch.isfinite(g_on).all())
    assert float((g_on - g_off).abs().max()) > 10 * GRAD_TOL * float(g_off.abs().max())
    tm.guided_attention = (0.0, 1.0)
    with pytest.raises(ValueError):
        tm.training_step(batch, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. guard bands
# ---------------------------------------------------------------------------------------------------------------------------
CHAIN_OUTPUTS = ("Zatt", "dctx_tot", "dpmT", "dv_part", "dU_part", "de", "Gcum")


@pytest.mark.parametrize("B,L,T,seed", [(3, 300, 21, 101), (2, 253, 7, 105)])
def test_alignment_only_backward_with_guard_bands(B, L, T, seed):
    """The new operand is one more hand-indexed read: the (3, 300, 21) case of 2 and an L = 253 case (one position past the one-pass
    per-slice kernel) once more with guard bands on every engine workspace and the ParamStore's flat buffers, the upstream gradient
    itself a guarded allocation of exactly B*T*L elements between NaN bands.  Bands intact; what the frame chain itself writes (gate
    gradients, context gradients, the per-sample accumulators - fixed summation order) is bit-identical to the run without bands; the
    parameter gradients, which pass through split-K GEMMs whose atomics land in any order, agree to the last bits and match the oracle."""
    from tacotron2_amd import guard
    dev = _dev()
    c = _oracle_case(B, L, T, seed)
    Rw = _dense_weight(B, T, L, seed + 1)
    ref = _oracle_grads(c, lambda o: (o[3] * Rw).sum())
    eng0, ps0, _ = _hip_align_only(c, lambda outs, ctx: Rw.to(dev), dev)
    keep = []

    def guarded(outs, ctx):
        backing, v, g = guard.alloc(B * T * L, torch.float32, dev, GUARD, 0)
        keep.append((backing, g))
        return v.copy_(Rw.to(dev).view(-1)).view(B, T, L)
    eng1, ps1, _ = _hip_align_only(c, guarded, dev, guard_bytes=GUARD)
    assert eng1.guard_bytes == GUARD and ps1.guard_bytes == GUARD
    assert eng1.guard_check() == [] and ps1.guard_check() == []
    backing, g = keep[0]
    n = B * T * L
    assert guard.scan("d_align", backing, g, n) == []
    _align_only_check(ps1, ref, f"(B,L,T)=({B},{L},{T}) randn, guard bands")
    A4 = 4 * c[0]["att_rnn_dim"]
    for name in CHAIN_OUTPUTS:
        a, b = eng0._ws[name], eng1._ws[name]
        a = a.view(-1)[:b.numel()]
        if name == "Zatt":           # Z[s] = [dgates_s | dq_{s-1}]: slot 0 has no dq part (never written, never read)
            a, b = a.view(T + 1, B, -1), b.view(T + 1, B, -1)
            assert torch.equal(a[0, :, :A4], b[0, :, :A4]), name
            a, b = a[1:], b[1:]
        assert torch.equal(a, b), name
    worst = 0.0
    for name, g1 in ps1.reference_layout(ps1.G).items():
        if name in ZERO_GRADIENT_BY_CONSTRUCTION:        # (cancellation residue of each run's own summation order)
            continue
        g0 = ps0.reference_layout(ps0.G)[name]
        if float(g0.abs().max()) > 0:
            worst = max(worst, float((g1 - g0).abs().max()) / float(g0.abs().max()))
        else:
            assert float(g1.abs().max()) == 0.0, name
    print(f"guarded against unguarded parameter gradients (B,L,T)=({B},{L},{T}): worst {worst:.2e} of the tensor's largest element")
    assert worst <= 2e-6          # (a few ulps of the largest split-K partial: the order of at most 16 atomic adds per element)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. CLI
# ---------------------------------------------------------------------------------------------------------------------------
def test_cli_train_guided_attention_prints_the_fourth_term(tmp_path):
    cfg = _cfg(tmp_path)
    args = ["--config", str(cfg), "--device", "0", "train", "--speech-dir", "unused", "--synthetic", "--max-steps", "2"]
    out = _run(args + ["--results-dir", str(tmp_path / "on"), "--guided-attention", "0.4,1.0"])
    lines = [l for l in out.splitlines() if "training_loss" in l]
    assert len(lines) == 2 and all("training_guided_loss" in l for l in lines), out
    for l in lines:
        f = lambda key: float(l.split(key + " ")[1].split()[0])
        gl = f("training_guided_loss")
        assert np.isfinite(gl) and 0.0 < gl < 1.0                 # a mean of weights under a mask in [0, 1), times alpha = 1
        parts = f("training_gate_loss") + f("training_mel_loss") + f("training_mel_post_loss") + gl
        assert abs(f("training_loss") - parts) < 1e-4
    ck = torch.load(tmp_path / "on" / "final.ckpt", map_location="cpu", weights_only=True)
    assert "guided_attention" not in ck["hyper_parameters"] and ck["global_step"] == 2
    # the config section does the same; the option wins over it
    import json
    cj = json.loads(cfg.read_text()); cj["training"]["guided_attention"] = {"sigma": 0.4, "alpha": 1.0}; cfg.write_text(json.dumps(cj))
    out_cfg = _run(args + ["--results-dir", str(tmp_path / "cfg")])
    first = lambda o: [l for l in o.splitlines() if "training_loss" in l][0]
    assert first(out_cfg).split(" lr ")[0] == lines[0].split(" lr ")[0]          # same seed, same first step, same four values
    out_alpha = _run(args + ["--results-dir", str(tmp_path / "opt"), "--guided-attention", "0.4,3.0"])
    g3 = float(first(out_alpha).split("training_guided_loss ")[1].split()[0])
    g1 = float(lines[0].split("training_guided_loss ")[1].split()[0])
    assert abs(g3 - 3.0 * g1) < 2e-5 * 3
    # without the option and the section the line is as before
    del cj["training"]["guided_attention"]; cfg.write_text(json.dumps(cj))
    out_off = _run(args + ["--results-dir", str(tmp_path / "off")])
    assert "training_guided_loss" not in out_off and "training_mel_post_loss" in out_off
    l0 = first(out_off)
    assert l0.split(" training_loss")[0] == lines[0].split(" training_guided_loss")[0]      # the three terms of step 1 are the same
