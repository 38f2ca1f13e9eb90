"""Forward attention under teacher forcing (training) on the GPU:
 1. kernel level, through the C ABI: t2_attn_seq_fwd with T2AttnSeq.forward and t2_attn_seq_bwd_forward (without a stash, and with
    the stash + t2_attn_acc_bwd) against the float64 autograd restatement of tests/forward_attention_chain_ref.py - every forward
    stash and all six backward outputs within TOL_FA (16 x the restatement's own float32 error, anchored by
    tests/test_forward_attention_chain_host.py), single-position samples within their absolute bounds;
 2. off is exact, argument errors launch nothing;
 3. engine level: forward_tf(forward_attention=True) + backward_tf against a float64 whole-model restatement built from the
    oracle's functions (the way tests/test_gpu_guided_attention.py does it: mid-size dims, replayed masks), also under guard bands;
 4. the module API, one Trainer step with the guided term, the CLI.
A case with a start state (`init`, forward_attention_chain_ref) hands it to the kernels through slot 1 of the time-major stashes and
row 0 of the alignments, and runs the frames from t_begin = 1 / down to t_lo = 1.

Engine-level criteria (the project's): mel / post-net L1 < 1e-4, alignments max-abs < 5e-5, every gradient tensor within 3e-4 of its
largest reference element.  The float32 CPU run of the same restatement stays below 3e-4 / 16 on the seeds used."""
import ctypes
import functools
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tacotron2_ref as R  # noqa: E402
from tests import attention_chain_ref as C  # noqa: E402
from tests import forward_attention_chain_ref as F  # noqa: E402
from tests.test_gpu_attention_chain import XP_COL0, _device_inputs, _dims, _nan, _stream, _untile16  # noqa: E402

KL = C.KL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(inp, init, float64 chain_fa) of a case: computed once, shared, never modified."""
    inp, init = F.make_inputs_fa(F.CASES_FA[name])
    return inp, init, F.chain_fa(inp, torch.float64, init)


def _tile16(x, Bp):
    """(B, K) -> [K/16][Bp][16] (T2LstmStep.xt), pad rows zero."""
    B, K = x.shape
    out = torch.zeros(K // 16, Bp, 16, device=x.device)
    out[:, :B] = x.view(B, K // 16, 16).transpose(0, 1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 1. kernel level
# ---------------------------------------------------------------------------------------------------------------------------
def run_fwd(dev, case, d, init, forward=1, chunks=None):
    """t2_attn_seq_fwd (packed path); everything the call writes is NaN-filled first.  forward=None: the field is not set at all."""
    from tacotron2_amd import _lib
    B, L, T, A, Ad, Ef = _dims(case)
    L4, Bp, ldx = (L + 3) // 4 * 4, (B + 15) // 16 * 16, A + Ef
    s = dict(xdec=_nan(dev, T + 1, B, ldx), att_c=_nan(dev, T + 1, B, A), gates=_nan(dev, T, B, 4 * A), align=_nan(dev, B, T, L),
             cum=_nan(dev, T + 1, B, L), th=_nan(dev, T, B, Ad, L4), xproj=_nan(dev, T, B, XP_COL0 + Ef + 4),
             e_part=_nan(dev, B, Ad // 16, L))
    xdec_t = torch.zeros(T + 1, ldx // 16, Bp, 16, device=dev) if B != Bp else _nan(dev, T + 1, ldx // 16, Bp, 16)
    first = 0
    for k in ("xdec", "att_c", "cum"):
        s[k][0] = 0
    xdec_t[0] = 0
    if init is not None:          # the state after frame 0: slot 1 of the stashes, row 0 of the alignments
        first = 1
        a0 = init["align0"].double()
        ctx0 = torch.einsum("bl,ble->be", a0, d["memory"].cpu().double()).float()
        s["xdec"][1] = torch.cat([init["att_h"], ctx0], 1).to(dev)
        s["att_c"][1] = init["att_c"].to(dev)
        s["cum"][1] = init["cum"].to(dev)
        s["align"][:, 0] = init["align0"].to(dev)
        xdec_t[1] = _tile16(s["xdec"][1], Bp)
    s["xdec_t"] = xdec_t
    segs = (_lib.S["T2Seg"] * 2)()
    segs[0].w = d["W_hh"].data_ptr(); segs[0].ldw = A; segs[0].K = A
    segs[1].w = d["W_ih_ctx"].data_ptr(); segs[1].ldw = Ef; segs[1].K = Ef
    wp = _nan(dev, A // 4 * ((ldx // 16 + 15) // 16 * 16) * 256)
    _lib.call("t2_lstm_pack_fwd", segs, 2, A, wp, _stream())
    kw = {} if forward is None else dict(forward=forward)
    seq = _lib.make("T2AttnSeq", B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, Kl=KL, wpacked=wp, W_ih_ctx=d["W_ih_ctx"], ld_wih=Ef,
                    W_hh=d["W_hh"], Wq=d["Wq"], U=d["U"], v=d["v"], pre=d["pre"], pmT=d["pmT"], memory=d["memory"], len=d["len"],
                    att_drop=d["att_drop"], xdec=s["xdec"], att_c=s["att_c"], gates=s["gates"], align=s["align"], cum=s["cum"],
                    th=s["th"], xproj_ctx=s["xproj"].data_ptr() + 4 * XP_COL0, ld_xproj=XP_COL0 + Ef + 4, e_part=s["e_part"],
                    xdec_t=xdec_t, **kw)
    for t0, t1 in (chunks or [(first, T)]):
        seq.t_begin, seq.t_end = t0, t1
        _lib.call("t2_attn_seq_fwd", seq, _stream())
    torch.cuda.synchronize()
    return s, first


def fwd_to_ref_layout(case, s, first):
    B, L, T, A, Ad, Ef = _dims(case)
    c = {k: x.cpu() for k, x in s.items()}
    return dict(att_h=c["xdec"][first + 1:, :, :A], ctx=c["xdec"][first + 1:, :, A:], att_c=c["att_c"][first + 1:],
                gates=c["gates"][first:].view(T - first, B, A, 4).transpose(2, 3).reshape(T - first, B, 4 * A),
                cum=c["cum"][first + 1:], align=c["align"][:, first:], th=c["th"][first:, ..., :L].transpose(2, 3)), c


def bwd_operands(dev, case, d, s, tiled):
    """The T2AttnSeqBwd block on the forward kernel's stashes; everything the call writes before reading is NaN-filled, only what the
    header tells the caller to zero is zeroed.  Returns (struct, outputs, workspaces, Z, Zt)."""
    from tacotron2_amd import _lib
    B, L, T, A, Ad, Ef = _dims(case)
    Bp, ldz = (B + 15) // 16 * 16, 4 * A + Ad

    def pack_bwd(W, ldw, N4, ncols):
        out = _nan(dev, (ncols + 15) // 16 * ((N4 // 16 + 31) // 32 * 32) * 256)
        _lib.call("t2_lstm_pack_bwd", W, ldw, N4, None, 0, 0, ncols, out, _stream())
        return out
    wtp_ctx, wtp_h, wtp_q = pack_bwd(d["W_ih_ctx"], Ef, 4 * A, Ef), pack_bwd(d["W_hh"], A, 4 * A, A), pack_bwd(d["Wq"], A, Ad, A)
    Z = _nan(dev, T + 1, B, ldz)
    Z[T, :, :4 * A] = 0
    Zt = None
    if tiled:
        Zt = _nan(dev, T + 1, 4 * A // 16, Bp, 16)
        Zt[T] = 0
    o = dict(dctx_tot=_nan(dev, T, B, Ef), dpmT=torch.zeros(B, Ad, L, device=dev), dv=torch.zeros(B, Ad, device=dev),
             dU=torch.zeros(B, Ad * 2 * KL, device=dev))
    ws = dict(dc=torch.zeros(B, A, device=dev), G=_nan(dev, 2, B, L), de=_nan(dev, B, L), din_part=_nan(dev, B, Ad // 16, 2, L),
              dh_rec=_nan(dev, B, A), ws_bd=_nan(dev, Ad // 16 * 16896), dprior=_nan(dev, 2, B, L), de_stash=_nan(dev, T, B * L + 3))
    sb = _lib.make("T2AttnSeqBwd", B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, Kl=KL, W_ih_ctx=d["W_ih_ctx"], ld_wih=Ef, W_hh=d["W_hh"],
                   Wq=d["Wq"], U=d["U"], v=d["v"], wtp_ctx=wtp_ctx, wtp_h=wtp_h, wtp_q=wtp_q, memory=d["memory"], xdec=s["xdec"],
                   att_c=s["att_c"], gates=s["gates"], align=s["align"], cum=s["cum"], th=s["th"], att_drop=d["att_drop"],
                   dh_ext=d["dh_ext"], ld_dh=A, dctx_ext1=d["dctx_ext1"], ld_dc1=Ef, dctx_ext2=d["dctx_ext2"], ld_dc2=Ef,
                   dgates=Z, dctx_tot=o["dctx_tot"], dq=None, dpmT=o["dpmT"], dv_part=o["dv"], dU_part=o["dU"], dc=ws["dc"],
                   G=ws["G"], de=ws["de"], din_part=ws["din_part"], dh_rec=ws["dh_rec"], dgates_t=Zt, ws_bd=ws["ws_bd"],
                   dalign=d["dalign"])
    return sb, o, ws, Z, Zt


def run_bwd(dev, case, d, s, first, tiled, stash, chunks=None):
    """t2_attn_seq_bwd_forward on the forward kernel's stashes, frames T-1 .. first; stash=True: with the de stash, then
    t2_attn_acc_bwd per call.  Returns the outputs in the reference layouts (CPU), the raw Z / dgates_t and the workspaces."""
    from tacotron2_amd import _lib
    B, L, T, A, Ad, Ef = _dims(case)
    sb, o, ws, Z, Zt = bwd_operands(dev, case, d, s, tiled)
    ld_stash = B * L + 3
    for hi, lo in (chunks or [(T, first)]):
        sb.t_hi, sb.t_lo = hi, lo
        _lib.call("t2_attn_seq_bwd_forward", sb, ws["de_stash"] if stash else None, ld_stash if stash else 0, ws["dprior"], _stream())
        if stash:
            _lib.call("t2_attn_acc_bwd", sb, ws["de_stash"], ld_stash, lo, hi, _stream())
    torch.cuda.synchronize()
    Zc = Z.cpu()
    out = dict(dgates=Zc[first:T, :, :4 * A], dq=Zc[first + 1:, :, 4 * A:], dctx_tot=o["dctx_tot"].cpu()[first:],
               dpm=o["dpmT"].cpu().transpose(1, 2), dv=o["dv"].cpu(), dU=o["dU"].cpu().view(B, Ad, 2, KL))
    return out, Zc, (None if Zt is None else Zt.cpu()), ws


def _check(name, got, inp, ref, names, first):
    errs = F.errors_fa(got, ref, inp, names=names)
    line = ", ".join(f"{k} {e:.2e} (b{b}) /{F.TOL_FA[k]:.1e}" for k, (e, b) in errs.items())
    print(f"[forward attention chain] {name}: {line}")
    bad = {k: (e, b) for k, (e, b) in errs.items() if not e <= F.TOL_FA[k]}
    sp = F.single_position_violations_fa(got, inp, ref, first)
    assert not bad and not sp, (f"{name}: outputs over their constant {{output: (per_sample_rel, sample)}} {bad}; "
                                f"single-position samples over their bound [(output, sample, value/bound)] {sp}")


def _calls(T, first, n):
    """Descending (t_hi, t_lo) calls of n frames over frames T-1 .. first."""
    out, hi = [], T
    while hi > first:
        out.append((hi, max(first, hi - n))); hi = max(first, hi - n)
    return out


@pytest.mark.parametrize("name", list(F.CASES_FA))
def test_chain_under_forward_attention_against_float64(dev, name):
    """Forward with T2AttnSeq.forward = 1, then the backward twice - t2_attn_seq_bwd_forward without a stash, and with the stash +
    t2_attn_acc_bwd (texts above 252 positions ignore the stash: the same launches) - every stash and output against float64."""
    case = F.CASES_FA[name]
    B, L, T, A, Ad, Ef = _dims(case)
    inp, init, ref = _ref(name)
    d = _device_inputs(dev, inp)
    first = 0 if init is None else 1
    bch = _calls(T, first, case["chunk"]) if case["chunk"] else None
    fch = [(lo, hi) for hi, lo in reversed(bch)] if bch else None
    if bch:
        assert len(bch) >= 3 and {hi & 1 for hi, _ in bch} == {0, 1}        # the carry crosses a call boundary at both parities
    s, _ = run_fwd(dev, case, d, init, chunks=fch)
    got, raw = fwd_to_ref_layout(case, s, first)
    _check(name + " fwd", got, inp, ref, C.FWD_OUTPUTS, first)
    assert torch.equal(_untile16(raw["xdec_t"], B)[first + 1:], raw["xdec"][first + 1:])
    behind = torch.arange(L)[None, :] >= inp["len"][:, None]
    assert float(raw["align"][:, first:].masked_select(behind[:, None, :].expand(B, T - first, L)).abs().sum()) == 0.0
    rows = raw["align"][:, first:].double().sum(-1)
    assert float((rows - 1).abs().max()) < 1e-5
    for stash in (False, True):
        out, Zc, Ztc, ws = run_bwd(dev, case, d, s, first, tiled=case["tiled"], stash=stash, chunks=bch)
        _check(f"{name} bwd {'stash + acc' if stash else 'plain'}", out, inp, ref, C.BWD_OUTPUTS, first)
        if Ztc is not None:
            assert torch.equal(_untile16(Ztc[first:T], B), Zc[first:T, :, :4 * A])
        # r: every position < L of every row written (zeros behind len), except where no frame >= 1 ran
        pr = ws["dprior"].cpu()
        wrote = [t for t in range(max(first, 1), T)]
        for par in {t & 1 for t in wrote}:
            assert bool(torch.isfinite(pr[par]).all()), par
            assert float(pr[par].masked_select(behind).abs().sum()) == 0.0
        for par in {0, 1} - {t & 1 for t in wrote}:
            assert bool(torch.isnan(pr[par]).all()), par                     # (frame 0 hands nothing back: its prior is a constant)


@pytest.mark.parametrize("name", ["L33_bump30", "L257_bump212"])
def test_chunked_backward_is_bit_identical(dev, name):
    """(t_hi, t_lo) calls of 5 and of 1 frame against one call: r travels through memory in the slot of the absolute frame's parity,
    no atomics anywhere - bit-identical."""
    case = F.CASES_FA[name]
    T = case["T"]
    inp, init, _ = _ref(name)
    d = _device_inputs(dev, inp)
    s, first = run_fwd(dev, case, d, init)
    o1, Z1, _, _ = run_bwd(dev, case, d, s, first, tiled=case["tiled"], stash=False)
    for n in (5, 1):
        o2, Z2, _, _ = run_bwd(dev, case, d, s, first, tiled=case["tiled"], stash=False, chunks=_calls(T, first, n))
        for k in C.BWD_OUTPUTS:
            assert torch.equal(o1[k], o2[k]), (n, k, float((o1[k] - o2[k]).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. off is exact; argument errors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L33_B17_zero", "L257_bump250"])
def test_off_is_exact(dev, name):
    """T2AttnSeq.forward = 0 against a struct on which the new field was never set: every stash bit for bit; and the forward differs
    from the option's (so the comparison compares something)."""
    case = F.CASES_FA[name]
    inp, init, _ = _ref(name)
    d = _device_inputs(dev, inp)
    s0, first = run_fwd(dev, case, d, init, forward=0)
    s1, _ = run_fwd(dev, case, d, init, forward=None)
    for k in ("xdec", "att_c", "gates", "align", "cum", "xproj", "xdec_t", "th", "e_part"):
        assert torch.equal(torch.nan_to_num(s0[k], nan=7.0), torch.nan_to_num(s1[k], nan=7.0)), k
    s2, _ = run_fwd(dev, case, d, init, forward=1)
    assert float((s2["align"][:, first:] - s0["align"][:, first:]).abs().max()) > 1e-2


def test_argument_errors_launch_nothing(dev):
    """t2_attn_seq_bwd_forward without dprior, or without the alignments to read, is T2_ERR_ARG before any launch: the outputs keep
    their fill.  The public single step still refuses forward together with the tanh stash."""
    from tacotron2_amd import _lib
    name = "L33_bump30"
    case = F.CASES_FA[name]
    B, L, T, A, Ad, Ef = _dims(case)
    inp, init, _ = _ref(name)
    d = _device_inputs(dev, inp)
    s, first = run_fwd(dev, case, d, init)
    lib = _lib.lib()
    for what in ("dprior", "align"):
        sb, o, ws, Z, Zt = bwd_operands(dev, case, d, s, True)
        sb.t_hi, sb.t_lo = T, first
        if what == "align":
            sb.align = None
        torch.cuda.synchronize()
        rc = lib.t2_attn_seq_bwd_forward(ctypes.addressof(sb), None, 0, None if what == "dprior" else ws["dprior"].data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 1 and b"t2_attn_seq_bwd_forward" in lib.t2_last_error(), (what, rc, lib.t2_last_error())
        assert bool(torch.isnan(o["dctx_tot"]).all()) and bool(torch.isnan(Z[:T]).all()) and bool(torch.isnan(ws["ws_bd"]).all())
        assert bool(torch.isnan(ws["dprior"]).all()) and bool(torch.isnan(ws["de"]).all())
        assert float(o["dpmT"].abs().sum()) == 0.0
    q = _lib.make("T2AttnStep", B=B, L=L, A=A, Ad=Ad, Ef=Ef, Kl=KL, att_h=s["xdec"][1], ldh=A + Ef, Wq=d["Wq"], U=d["U"], v=d["v"],
                  pmT=d["pmT"], memory=d["memory"], len=d["len"], e_part=s["e_part"], th_out=s["th"], w_out=_nan(dev, B, L), ldwo=L,
                  ctx_out=_nan(dev, B, Ef), ldctx=Ef, forward=1)
    assert lib.t2_attn_step_fwd(ctypes.addressof(q), _stream()) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# 3. engine level
# ---------------------------------------------------------------------------------------------------------------------------
from tests.test_gpu_model import _dev, _grad_check, build_engine, masks_to_device, random_case  # noqa: E402

MID = dict(num_chars=39, encoded_dim=128, prenet_dim=64, att_rnn_dim=256, att_dim=64, rnn_hidden_dim=256, postnet_dim=128,
           num_mels=80, dropout=0.5)
GUARD = 65536


@functools.lru_cache(maxsize=None)
def _model_case(B, L, T, seed, dtype=torch.float64):
    d = R.default_dims(**MID)
    P = R.init_params(d, seed=5)
    case = random_case(d, B, L, T, seed, None)
    Pc, o, names = F.model_fa(P, d, case, dtype)
    return d, P, case, Pc, o, names


def _model_grads(c, fn):
    d, P, case, Pc, o, names = c
    gs = torch.autograd.grad(fn(o), [Pc[k] for k in names], allow_unused=True, retain_graph=True)
    return {k: (torch.zeros_like(Pc[k]) if g is None else g) for k, g in zip(names, gs)}


def _hip_step(c, dev, chunk_bwd=None, guard_bytes=None, forward_attention=True, splitk=True):
    """forward_tf(forward_attention=True) + loss_and_grads -> (engine, ParamStore, outs).  splitk=False: the forward's short-chunk
    GEMMs without split-K (Engine.splitk_small_chunks), whose atomics land in any order - the forward is then bit-reproducible."""
    d, P, (ci, lens, mel, tl, gate, masks) = c[0], c[1], c[2]
    eng, ps = build_engine(d, P, dev, guard_bytes=guard_bytes)
    eng.splitk_small_chunks = splitk
    if chunk_bwd is not None:
        eng.chunk_bwd = chunk_bwd
    kw = dict(forward_attention=True) if forward_attention else {}
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev), **kw)
    ps.grad.zero_()
    eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev))
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    return eng, ps, outs


def _grad_report(ps, grads, label):
    """_grad_check (the project's criterion) after printing the worst ratio (DESIGN.md 5.4 records it per shape)."""
    from tests.test_gpu_model import ZERO_GRADIENT_BY_CONSTRUCTION
    worst = (0.0, None)
    for name, g in ps.reference_layout(ps.G).items():
        if name in ZERO_GRADIENT_BY_CONSTRUCTION:
            continue
        r = grads[name].double()
        err = float((g.double().cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-3)
        if err > worst[0]:
            worst = (err, name)
    print(f"forward attention gradients {label}: worst {worst[0]:.2e} of the tensor's largest element ({worst[1]})")
    _grad_check(ps, grads)


def _check_outputs(outs, o, label):
    mel_l1 = float((outs[0].cpu().double() - o[0].detach().double()).abs().mean())
    post_l1 = float((outs[1].cpu().double() - o[1].detach().double()).abs().mean())
    al = float((outs[3].cpu().double() - o[3].detach().double()).abs().max())
    print(f"forward attention engine {label}: mel L1 {mel_l1:.2e}, post L1 {post_l1:.2e}, align max-abs {al:.2e}")
    assert mel_l1 < 1e-4 and post_l1 < 1e-4 and al < 5e-5


ENGINE_CASES = [(4, 33, 29, 101, None), (3, 300, 21, 101, None), (5, 40, 23, 103, 5), (33, 21, 9, 104, None)]


@pytest.mark.parametrize("B,L,T,seed,chunk_bwd", ENGINE_CASES)
def test_engine_step_matches_the_float64_restatement(B, L, T, seed, chunk_bwd):
    dev = _dev()
    c = _model_case(B, L, T, seed)
    d, P, (ci, lens, mel, tl, gate, masks), Pc, o, names = c
    total = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())[0]
    grads = _model_grads(c, lambda o_: total)
    eng, ps, outs = _hip_step(c, dev, chunk_bwd=chunk_bwd)
    _check_outputs(outs, o, f"(B,L,T)=({B},{L},{T})")
    assert "dprior" in eng._ws
    _grad_report(ps, grads, f"(B,L,T)=({B},{L},{T})")
    # the plain chain's gradients are far outside the tolerance: the case does test the option
    plain = _hip_step(c, dev, chunk_bwd=chunk_bwd, forward_attention=False)
    assert "dprior" not in plain[0]._ws
    n = "decoder.attention.v.weight"
    g0 = plain[1].reference_layout(plain[1].G)[n].cpu().double()
    assert float((g0 - grads[n]).abs().max()) > 30 * 3e-4 * float(grads[n].abs().max())


def _hip_align_only(c, Rw, dev, guard_bytes=None):
    """forward_tf(forward_attention=True) + backward_tf(ctx, zeros, zeros, d_align=Rw): the attention chain driven alone.  Two such
    runs are bit-identical in everything the chain writes (fixed summation orders, no atomics), which a full step is not: its
    upstream gradients pass through split-K GEMMs whose atomics land in any order ("Off means off")."""
    d, P, (ci, lens, mel, tl, gate, masks) = c[0], c[1], c[2]
    eng, ps = build_engine(d, P, dev, guard_bytes=guard_bytes)
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev),
                               forward_attention=True)
    B, T, M = outs[0].shape
    ps.grad.zero_()
    eng.backward_tf(ctx, torch.zeros(B, T, M, device=dev), torch.zeros(T, B, M + 1, device=dev), d_align=Rw.to(dev))
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    return eng, ps, outs


def test_engine_under_guard_bands():
    """(2, 253, 7) - one position past the one-pass per-slice kernel - with guard bands on every workspace and the ParamStore's flat
    buffers.  A full step: no band touched, outputs and every gradient match the restatement.  Then the chain driven alone (zero mel
    gradients, a dense d_align - a full step's upstream gradients pass through split-K atomics and are not bit-reproducible): no band
    touched, what the chain writes (r included) is bit-identical to the unguarded run, gradients of sum(alignments * R) match."""
    from tests.test_gpu_guided_attention import _align_only_check
    dev = _dev()
    B, L, T = 2, 253, 7
    c = _model_case(B, L, T, 105)
    d, P, case, Pc, o, names = c
    ci, lens, mel, tl, gate, masks = case
    total = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())[0]
    engf, psf, outsf = _hip_step(c, dev, guard_bytes=GUARD)
    assert engf.guard_bytes == GUARD and psf.guard_bytes == GUARD and "dprior" in engf._ws
    assert engf.guard_check() == [] and psf.guard_check() == []
    _check_outputs(outsf, o, "(2,253,7) full step, guard bands")
    _grad_report(psf, _model_grads(c, lambda o_: total), "(2,253,7) full step, guard bands")
    Rw = torch.randn(B, T, L, generator=torch.Generator().manual_seed(106))
    gs = torch.autograd.grad((o[3] * Rw.double()).sum(), [Pc[k] for k in names], allow_unused=True, retain_graph=True)
    eng0, ps0, _ = _hip_align_only(c, Rw, dev)
    eng1, ps1, outs = _hip_align_only(c, Rw, dev, guard_bytes=GUARD)
    assert eng1.guard_bytes == GUARD and ps1.guard_bytes == GUARD
    assert eng1.guard_check() == [] and ps1.guard_check() == []
    _check_outputs(outs, o, "(2,253,7) chain alone, guard bands")
    _align_only_check(ps1, dict(zip(names, gs)), "forward attention, (2,253,7) randn, guard bands")
    A4 = 4 * d["att_rnn_dim"]
    for name in ("Zatt", "dctx_tot", "dpmT", "dv_part", "dU_part", "de", "Gcum", "dprior"):
        a, b = eng0._ws[name], eng1._ws[name]
        a = a.view(-1)[:b.numel()]
        if name == "Zatt":           # Z[s] = [dgates_s | dq_{s-1}]: slot 0 has no dq part (never written, never read)
            a, b = a.view(T + 1, B, -1), b.view(T + 1, B, -1)
            assert torch.equal(a[0, :, :A4], b[0, :, :A4]), name
            a, b = a[1:], b[1:]
        assert torch.equal(a, b), name


def test_off_is_the_call_without_the_argument():
    """forward_attention=False against a call without the argument: all four outputs and the attention chain's stashes torch.equal,
    the same workspace set, no dprior.  (The forward's short-chunk GEMMs run without split-K here: with it their atomics land in any
    order and two runs of one tree differ in the mels' last bits, DESIGN.md section 9 "Off means off".)"""
    dev = _dev()
    c = _model_case(4, 33, 29, 101)
    d, P, (ci, lens, mel, tl, gate, masks) = c[0], c[1], c[2]
    res = []
    for kw in ({}, dict(forward_attention=False)):
        eng, ps = build_engine(d, P, dev)
        eng.splitk_small_chunks = False
        outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks_to_device(masks, dev), **kw)
        ps.grad.zero_()
        eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev))
        torch.cuda.synchronize()
        res.append(([x.clone() for x in outs], set(eng._ws), [ctx[k].clone() for k in ("xdec", "att_c", "cum")]))
    for i, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        assert torch.equal(a, b), i
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    assert res[0][1] == res[1][1] and "dprior" not in res[1][1]
    with pytest.raises(ValueError):
        eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), forward_attention=1)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. module API, Trainer, CLI
# ---------------------------------------------------------------------------------------------------------------------------
def test_module_train_forward_attention():
    from tacotron2_amd.model import Tacotron2
    dev = _dev()
    c = _model_case(4, 33, 29, 101)
    d, P, (ci, lens, mel, tl, gate, masks), Pc, o, names = c
    m = Tacotron2(device=dev, **{k: d[k] for k in ("num_chars", "encoded_dim", "encoder_kernel_size", "num_mels", "prenet_dim",
                                                   "att_rnn_dim", "att_dim", "rnn_hidden_dim", "postnet_dim", "dropout")})
    m.load_state_dict(P)
    m.train()
    dm = masks_to_device(masks, dev)
    eng, ps, outs = _hip_step(c, dev, splitk=False)      # (no split-K in the forward: bit-reproducible, see _hip_step)
    m._engine.splitk_small_chunks = False
    mels, post, gates, al = m(ci.to(dev), lens.to(dev), True, mel.to(dev), tl.to(dev), dropout_masks=dm, train_forward_attention=True)
    for i, (a, b) in enumerate(zip((mels, post, gates, al), outs)):
        assert torch.equal(a, b), i
    assert al.requires_grad and al.grad_fn is not None
    Rw = torch.randn(4, 29, 33, generator=torch.Generator().manual_seed(102))
    (al * Rw.to(dev)).sum().backward()
    torch.cuda.synchronize()
    ref = _model_grads(c, lambda o_: (o_[3] * Rw.double()).sum())
    for n in ("decoder.attention.v.weight", "decoder.attention.query_layer.weight", "decoder.attention.location_dense.weight",
              "att_encoder.weight"):
        got = m.store.reference_layout(m.store.G)[n].cpu().double()
        assert float((got - ref[n]).abs().max()) <= 3e-4 * float(ref[n].abs().max()), n
    with pytest.raises(ValueError):
        m(ci.to(dev), lens.to(dev), False, max_len_override=5, train_forward_attention=True)
    with pytest.raises(ValueError):
        m(ci.to(dev), lens.to(dev), True, mel.to(dev), tl.to(dev), forward_attention=True)


def test_ttsmodel_train_forward_attention_reaches_validation_and_training_step():
    """TTSModel.train_forward_attention on the reference-generated eval fixture (dropout 0: deterministic): validation_step()'s
    loss and alignment are those of forward(train_forward_attention=True) - the three terms restated from its outputs - and not
    those of the plain chain; training_step's backward reaches the attention parameters with other gradients than without."""
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
    off = tm.validation_step(batch, 0)
    with torch.no_grad():
        mels, post, gates, al = tm(t("chars_idx"), t("chars_len"), True, t("mel"), t("mel_len"), train_forward_attention=True)
    want = float(R.tts_loss(mels.cpu().double(), post.cpu().double(), gates.cpu().double(), t("mel").cpu().double(),
                            t("gate").cpu().double())[0])
    tm.train_forward_attention = True
    on = tm.validation_step(batch, 0)
    assert abs(float(on["loss"]) - want) < 1e-5 * max(1.0, want), (float(on["loss"]), want)
    ml, cl = int(z["mel_len"][0]), int(z["chars_len"][0])
    assert float((on["alignment"] - al[0, :ml, :cl]).abs().max()) < 1e-6
    assert float((on["alignment"] - off["alignment"]).abs().max()) > 1e-2 and abs(float(on["loss"]) - float(off["loss"])) > 1e-4
    assert "train_forward_attention" not in tm.hparams
    tm.train()
    grads = {}
    for flag in (True, False):
        tm.train_forward_attention = flag
        tm.zero_grad()
        tm.tacotron2._calls = 7                          # the same Philox prenet masks in both steps
        loss = tm.training_step(batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        grads[flag] = tm.tacotron2.store.G["decoder.attention.v.weight"].clone()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grads[flag]).all())
    assert float((grads[True] - grads[False]).abs().max()) > 10 * 3e-4 * float(grads[False].abs().max())


def test_trainer_step_with_forward_and_guided_attention():
    """Trainer(forward_attention=True, guided_attention=(0.4, 1.0)): the four loss values and the gradients of one step against the
    restatement (lr = 0: the optimiser step moves nothing; it reads the flat gradient buffer and leaves it as the backward wrote it)."""
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.trainer import Trainer
    from tests.test_guided_attention_host import guided_ref
    dev = _dev()
    c = _model_case(4, 33, 29, 101)
    d, P, (ci, lens, mel, tl, gate, masks), Pc, o, names = c
    total, bce, mel_l, post_l = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())
    gl = guided_ref(o[3], lens, tl, 0.4, 1.0)[0]
    grads = _model_grads(c, lambda o_: total + gl)
    ps = ParamStore(d, dev)
    ps.load_state_dict(P)
    tr = Trainer(ps, lr=0.0, weight_decay=0.0, guided_attention=(0.4, 1.0), forward_attention=True)
    batch = dict(chars_idx=ci.to(dev), chars_idx_len=lens.to(dev), mel_spectrogram=mel.to(dev), mel_spectrogram_len=tl.to(dev),
                 gate=gate.to(dev))
    loss3, outs = tr.train_step(batch, masks=masks_to_device(masks, dev))
    torch.cuda.synchronize()
    got = [float(x) for x in loss3.cpu()] + [float(tr.last_guided_loss.cpu())]
    want = [float(bce), float(mel_l), float(post_l), float(gl)]
    print("four terms (gate, mel, post, guided):", got, "restatement:", want)
    for g_, w_ in zip(got, want):
        assert abs(g_ - w_) < 2e-5 * max(1.0, abs(w_)), (got, want)
    _check_outputs(outs, o, "Trainer step")
    _grad_report(ps, grads, "Trainer step, guided (0.4, 1.0)")
    with pytest.raises(ValueError):
        Trainer(ps, lr=0.0, weight_decay=0.0, forward_attention="yes")


def test_cli_train_forward_attention(tmp_path):
    from tests.test_gpu_cli import _cfg, _run
    cfg = _cfg(tmp_path)
    args = ["--config", str(cfg), "--device", "0", "train", "--speech-dir", "unused", "--synthetic", "--max-steps", "2"]
    first = lambda out: [l for l in out.splitlines() if "training_loss" in l][0].split(" lr ")[0]
    on = _run(args + ["--results-dir", str(tmp_path / "on"), "--forward-attention"])
    assert "forward attention: training under the monotonic prior" in on and len([l for l in on.splitlines() if "training_loss" in l]) == 2
    ck = torch.load(tmp_path / "on" / "final.ckpt", map_location="cpu", weights_only=True)
    assert "forward_attention" not in ck["hyper_parameters"] and "train_forward_attention" not in ck["hyper_parameters"]
    off = _run(args + ["--results-dir", str(tmp_path / "off")])
    assert "forward attention" not in off and first(off) != first(on)
    cj = json.loads(cfg.read_text()); cj["training"]["forward_attention"] = True; cfg.write_text(json.dumps(cj))
    by_cfg = _run(args + ["--results-dir", str(tmp_path / "cfg")])
    assert first(by_cfg) == first(on)                    # the key alone switches it on: same seed, same first step
    cj["training"]["forward_attention"] = False; cfg.write_text(json.dumps(cj))
    assert first(_run(args + ["--results-dir", str(tmp_path / "flag"), "--forward-attention"])) == first(on)     # the flag wins
