"""Forward attention for autoregressive decoding on the GPU: Engine.infer(forward_attention=True) against the float64
forward-attention reference (tests/test_forward_attention_host.py), one attention step through the C ABI against a float64 step,
the monotonic support at vanilla dimensions, the option switched off, the module surface and a guarded decode."""
import pytest
import torch

from oracle import tacotron2_ref as R
from tests.helpers import SMALL, load_golden, params_from
from tests.test_forward_attention_host import forward_ref, forward_weights
from tests.test_gpu_attention_window import _dev, _engine, _inputs, _mid_params

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _check_rows(al, lens):
    """Every row is a distribution over the utterance's own positions: sums to 1, exactly 0.0 from `len` on."""
    al = al.cpu()
    L = al.shape[2]
    assert float((al.double().sum(2) - 1.0).abs().max()) < 1e-5
    past = (torch.arange(L)[None, :] >= lens.cpu()[:, None])[:, None, :].expand_as(al)
    if bool(past.any()):
        assert float(al[past].abs().max()) == 0.0


def _check_vs_ref(out, ref, lens):
    mels, post, gates, al, lengths = out
    rm, rp, rg, ra, rl = ref
    assert mels.shape == rm.shape, (mels.shape, rm.shape)
    l1 = lambda a, b: float((a.double().cpu() - b.double()).abs().mean())
    amax = float((al.double().cpu() - ra.double()).abs().max())
    print(f"mel L1 {l1(mels, rm):.3e}  post L1 {l1(post, rp):.3e}  alignments max-abs {amax:.3e}  lengths {lengths.tolist()}")
    assert torch.equal(lengths.cpu(), rl)
    assert l1(mels, rm) < 1e-4 and l1(post, rp) < 1e-4
    assert amax < 5e-5
    assert torch.equal(gates.cpu() == -1000.0, rg == -1000.0)
    _check_rows(al, lens)


def _decode_and_ref(d, P, lens, L, N, seed, check_every=5):
    dev = _dev()
    ci, lens, spk, pm = _inputs(lens, L, N, seed, d["prenet_dim"])
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        ref = forward_ref(P64, d, ci, lens, N, speaker_id=spk, prenet_drop=pm)
        plain = forward_ref(P64, d, ci, lens, N, speaker_id=spk, prenet_drop=pm, recursion=False)
    n = min(ref[3].shape[1], plain[3].shape[1])      # the case exercises the option: the plain decoder's alignments are far away
    assert float((ref[3][:, :n] - plain[3][:, :n]).abs().max()) > 1e-2
    eng = _engine(d, P, dev)
    out = eng.infer(ci.to(dev), lens.to(dev), N, speaker_id=spk.to(dev), prenet_masks=pm.to(dev).contiguous(),
                    check_every=check_every, forward_attention=True)
    torch.cuda.synchronize()
    return out, ref, lens


def test_forward_decode_matches_forward_oracle():
    d, P = _mid_params()
    out, ref, lens = _decode_and_ref(d, P, [29, 21, 17, 25, 9, 13], 29, 24, seed=4)
    _check_vs_ref(out, ref, lens)


@pytest.mark.parametrize("L,B", [(300, 1), (300, 17), (1100, 1), (1100, 17)])
def test_forward_decode_long_texts(L, B):
    """Texts above 256 positions: the context kernel walks them in rounds, the prior with them."""
    d, P = _mid_params()
    g = torch.Generator().manual_seed(L + B)
    lens = [L] + [int(x) for x in torch.randint(L // 2, L + 1, (B - 1,), generator=g)]
    out, ref, lens = _decode_and_ref(d, P, lens, L, 24, seed=L + 7 * B, check_every=8)
    _check_vs_ref(out, ref, lens)


def test_forward_decode_two_groups():
    """B = 70: two decode groups of the one-loop stop rule."""
    d, P = _mid_params()
    g = torch.Generator().manual_seed(70)
    lens = [23] + [int(x) for x in torch.randint(5, 24, (69,), generator=g)]
    out, ref, lens = _decode_and_ref(d, P, lens, 23, 16, seed=71)
    _check_vs_ref(out, ref, lens)


# ---------------------------------------------------------------------------------------------------------------------------
# one step through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _step_case(L, first, dev, A=64, Ad=32, Ef=160):
    """Operands of one t2_attn_step_fwd call and its float64 result with forward attention.  first: w_prev = NULL (the one-hot
    prior, zeros in the location features); else random rows that sum to 1."""
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(7 * L + int(first))
    B = 4
    P = {"decoder.attention.query_layer.weight": torch.randn(Ad, A, generator=g) / A ** 0.5,
         "decoder.attention.v.weight": torch.randn(1, Ad, generator=g),
         "decoder.attention.location_conv.weight": torch.randn(32, 2, 31, generator=g) / 8,
         "decoder.attention.location_dense.weight": torch.randn(Ad, 32, generator=g) / 6}
    att_h = torch.randn(B, A, generator=g); mem = torch.randn(B, L, Ef, generator=g); pm = torch.randn(B, L, Ad, generator=g)
    lens = torch.tensor([L, 1, max(1, L - 3), max(1, L // 2)])
    mask = torch.arange(L)[None] >= lens[:, None]
    if first:
        w = torch.zeros(B, L); cum = torch.zeros(B, L)
        prior = torch.zeros(B, L, dtype=torch.float64); prior[:, 0] = 1.0
    else:
        w = torch.softmax(torch.randn(B, L, generator=g), 1); cum = w * 2.5
        prior = w.double()
    Pd_ = {k: v.double() for k, v in P.items()}
    _, y = R.attention_fwd(Pd_, att_h.double(), mem.double(), pm.double(), torch.stack([w, cum], 1).double(), mask)
    w_ref = forward_weights(y, prior, mask)
    ctx_ref = torch.einsum("bl,ble->be", w_ref, mem.double())
    st = torch.cuda.current_stream().cuda_stream
    f = lambda t: t.float().to(dev).contiguous()
    U = torch.empty(Ad, 2, 31, device=dev)
    _lib.call("t2_attn_fold_location", f(P["decoder.attention.location_dense.weight"]),
              f(P["decoder.attention.location_conv.weight"]), U, Ad, 32, 31, st)
    out = dict(w=torch.full((B, L), -7.0, device=dev), cum=torch.full((B, L), -7.0, device=dev),
               ctx=torch.full((B, Ef), -7.0, device=dev))
    kw = dict(B=B, L=L, A=A, Ad=Ad, Ef=Ef, Kl=31, att_h=f(att_h), ldh=A, Wq=f(P["decoder.attention.query_layer.weight"]), U=U,
              v=f(P["decoder.attention.v.weight"]), w_prev=None if first else f(w), ldw=L, cum_prev=None if first else f(cum),
              ldcum=L, pmT=f(pm.transpose(1, 2)), memory=f(mem), len=lens.to(torch.int32).to(dev),
              e_part=torch.empty(B, Ad // 16, L, device=dev), w_out=out["w"], ldwo=L, cum_out=out["cum"], ldco=L,
              ctx_out=out["ctx"], ldctx=Ef)
    return kw, out, (w_ref, cum.double() + w_ref, ctx_ref), lens, st


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("L", [1, 2, 255, 256, 257, 600, 2000])
def test_forward_attention_step_matches_float64_step(L, first):
    """t2_attn_step_fwd with forward = 1 at the edges of the context kernel's 256-position rounds, ragged lengths down to one
    position, against the float64 step - the tolerance of tests/test_gpu_kernels.py::test_attention_step_fwd."""
    from tacotron2_amd import _lib
    dev = _dev()
    kw, out, (w_ref, cum_ref, ctx_ref), lens, st = _step_case(L, first, dev)
    _lib.call("t2_attn_step_fwd", _lib.make("T2AttnStep", forward=1, **kw), st)
    torch.cuda.synchronize()
    print(f"L {L} first {first}: weights {_rel(out['w'], w_ref):.3e}  context {_rel(out['ctx'], ctx_ref):.3e}  "
          f"cum {_rel(out['cum'], cum_ref):.3e}")
    assert _rel(out["w"], w_ref) < 1e-5 and _rel(out["ctx"], ctx_ref) < 1e-5
    assert _rel(out["cum"], cum_ref) < 1e-5
    w = out["w"].cpu()
    assert float((w.double().sum(1) - 1.0).abs().max()) < 1e-5
    for b in range(w.shape[0]):
        if int(lens[b]) < L:
            assert float(w[b, int(lens[b]):].abs().max()) == 0.0


def test_forward_attention_step_argument_errors_launch_nothing():
    """forward with a window, with the tanh stash, or with w_out == w_prev: T2_ERR_ARG and no launch (the outputs keep their fill)."""
    from tacotron2_amd import _lib
    dev = _dev()
    L = 37
    kw, out, _, _, st = _step_case(L, False, dev)
    B, Ad = kw["B"], kw["Ad"]
    peak = torch.zeros(2, B, dtype=torch.int32, device=dev)
    th = torch.empty(B, Ad, (L + 3) // 4 * 4, device=dev)
    bad = [dict(kw, win_back=1, win_fwd=3, win_peak=peak, cum_prev=out["cum"]),
           dict(kw, th_out=th),
           dict(kw, w_out=kw["w_prev"])]
    for k in bad:
        with pytest.raises(_lib.T2Error, match=r"rc=1"):
            _lib.call("t2_attn_step_fwd", _lib.make("T2AttnStep", forward=1, **k), st)
    torch.cuda.synchronize()
    for t in out.values():
        assert bool((t == -7.0).all())
    assert bool((peak == 0).all())
    _lib.call("t2_attn_step_fwd", _lib.make("T2AttnStep", forward=1, **kw), st)      # the same operands without the conflict run
    torch.cuda.synchronize()
    assert bool((out["w"] != -7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# vanilla dimensions
# ---------------------------------------------------------------------------------------------------------------------------
def vanilla_case(B=64, N=120, seed=188):
    """Vanilla dimensions, L = 188, ragged lengths 120..188, seeded weights, replayed prenet masks and a stop bias raised so that
    nothing stops: (d, P, chars_idx, lens, speaker_id, prenet masks, N).  The float32 forward_ref keeps argmax(frame t) <= t + 1
    on exactly these inputs (run on the CPU when the case was chosen), so the property is asked of the engine."""
    from bench import VANILLA
    d = R.default_dims(**VANILLA)
    P = R.init_params(d, seed=0)
    P["decoder.gate.bias"] = P["decoder.gate.bias"] + 10.0
    g = torch.Generator().manual_seed(seed)
    L = 188
    lens = torch.randint(120, L + 1, (B,), generator=g)
    lens[0] = L
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 39, (int(lens[b]),), generator=g)
    spk = torch.randint(0, 4, (B,), generator=g, dtype=torch.int32)
    pm = (torch.rand(N + 1, 2, B, d["prenet_dim"], generator=g) >= 0.5).float() * 2
    return d, P, ci, lens, spk, pm, N


def test_forward_decode_vanilla_dims_is_monotonic():
    """B = 64, L <= 188, 120 frames (no oracle at this size): finite outputs, rows that sum to 1, exact zeros past the text, and
    the peak of frame t at position <= t + 1 - the attention cannot have moved further from position 0."""
    dev = _dev()
    d, P, ci, lens, spk, pm, N = vanilla_case()
    eng = _engine(d, P, dev)
    mels, post, gates, al, lengths = eng.infer(ci.to(dev), lens.to(dev), N, speaker_id=spk.to(dev),
                                               prenet_masks=pm.to(dev).contiguous(), forward_attention=True)
    torch.cuda.synchronize()
    assert al.shape == (ci.shape[0], N, ci.shape[1])
    for x in (mels, post, gates, al):
        assert bool(torch.isfinite(x).all())
    _check_rows(al, lens)
    t = torch.arange(N)[None, :]
    peak = al.cpu().argmax(2)
    print("largest peak position minus frame index:", int((peak - t).max()))
    assert bool((peak <= t + 1).all())


# ---------------------------------------------------------------------------------------------------------------------------
# off means off; the module surface
# ---------------------------------------------------------------------------------------------------------------------------
def test_forward_attention_false_is_the_call_without_it():
    d, P = _mid_params()
    dev = _dev()
    L, N = 29, 24
    ci, lens, spk, pm = _inputs([29, 21, 17, 25, 9, 13], L, N, seed=4)
    eng = _engine(d, P, dev)
    args = (ci.to(dev), lens.to(dev), N)
    kw = dict(speaker_id=spk.to(dev), prenet_masks=pm.to(dev).contiguous(), check_every=5)
    base = [x.clone() for x in eng.infer(*args, **kw)]
    ws = set(eng._ws)
    off = [x.clone() for x in eng.infer(*args, forward_attention=False, **kw)]
    on = [x.clone() for x in eng.infer(*args, forward_attention=True, **kw)]
    torch.cuda.synchronize()
    for a, b in zip(base, off):
        assert a.shape == b.shape and torch.equal(a, b)
    assert set(eng._ws) == ws                         # no workspace of its own, on or off
    n = min(base[3].shape[1], on[3].shape[1])
    assert float((base[3][:, :n] - on[3][:, :n]).abs().max()) > 1e-2
    with pytest.raises(ValueError):
        eng.infer(*args, forward_attention=True, attention_window=(1, 3), **kw)


def test_module_inference_with_forward_attention():
    from tacotron2_amd.model import Tacotron2
    from tacotron2_amd.model.tts_model import TTSModel
    dev = _dev()
    z = load_golden("infer")
    P = params_from(z)
    m = Tacotron2(dropout=0.5, device=dev, **SMALL)
    m.load_state_dict(P)
    m.eval()
    t = lambda k: torch.from_numpy(z[k]).to(dev)
    pm = t("m.prenet_drop").contiguous()
    N = int(z["max_len"])
    with torch.no_grad():
        o = [x.clone() for x in m.inference(t("chars_idx"), t("chars_len"), N, dropout_masks=dict(prenet_drop=pm),
                                            forward_attention=True)]
        plain = [x.clone() for x in m.inference(t("chars_idx"), t("chars_len"), N, dropout_masks=dict(prenet_drop=pm))]
    e = m._engine.infer(t("chars_idx"), t("chars_len"), N, prenet_masks=pm, forward_attention=True)
    torch.cuda.synchronize()
    for a, b in zip(o, e[:4]):
        assert a.shape == b.shape and torch.equal(a, b)
    n = min(o[3].shape[1], plain[3].shape[1])
    assert not torch.equal(o[3][:, :n], plain[3][:, :n])
    mel, ml = torch.zeros(1, 4, 16, device=dev), torch.tensor([4], device=dev)
    with pytest.raises(ValueError):
        m(t("chars_idx"), t("chars_len"), True, mel, ml, forward_attention=True)
    tts = TTSModel(lr=1e-3, weight_decay=0.0, dropout=0.5, device=dev, **SMALL)
    tts.tacotron2.load_state_dict(P)
    tts.train()
    with pytest.raises(ValueError):                   # training mode: teacher forcing is the default
        tts(chars_idx=t("chars_idx"), chars_idx_len=t("chars_len"), mel_spectrogram=mel, mel_spectrogram_len=ml,
            forward_attention=True)
    tts.eval()
    with torch.no_grad():
        p = tts(chars_idx=t("chars_idx"), chars_idx_len=t("chars_len"), teacher_forcing=False, max_len_override=N,
                forward_attention=True)
    torch.cuda.synchronize()
    assert p[3].shape[2] == t("chars_idx").shape[1] and bool(torch.isfinite(p[3]).all())
    _check_rows(p[3], t("chars_len"))


# ---------------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------------
def test_guarded_forward_decode_touches_no_band():
    """B = 33 (two 16-row tiles and one row), L = 23 (not a multiple of 4), ragged texts down to one character, guard bands on
    every engine workspace and on the parameters: no band touched, and the outputs are those of the unguarded engine bit for bit."""
    from tests.test_gpu_model import build_engine
    dev = _dev()
    d, P = _mid_params()
    B, L, N = 33, 23, 24
    g = torch.Generator().manual_seed(133)
    lens = [L, 1] + [int(x) for x in torch.randint(1, L + 1, (B - 2,), generator=g)]
    ci, lens, spk, pm = _inputs(lens, L, N, seed=33, pdim=d["prenet_dim"])
    args = (ci.to(dev), lens.to(dev), N)
    kw = dict(speaker_id=spk.to(dev), prenet_masks=pm.to(dev).contiguous(), check_every=3, forward_attention=True)
    plain = [x.clone() for x in _engine(d, P, dev).infer(*args, **kw)]
    eng, ps = build_engine(d, P, dev, guard_bytes=65536)
    assert eng.guard_bytes == 65536 and ps.guard_bytes == 65536
    out = eng.infer(*args, **kw)
    torch.cuda.synchronize()
    assert eng.guard_check() == []
    eng.check_persistent_kernels()
    for a, b in zip(plain, out):
        assert a.shape == b.shape and torch.equal(a, b)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        ref = forward_ref(P64, d, ci, lens, N, speaker_id=spk, prenet_drop=pm)
    _check_vs_ref(out, ref, lens)
