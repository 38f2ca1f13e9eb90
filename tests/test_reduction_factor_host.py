"""Reduction factor (r mel frames per decoder step), host side: the float64 restatement of tests/reduction_ref.py pinned to the
oracle at r = 1, the parameter manifest, state_dict / checkpoint exchange, argument errors and the hand-computed indices of the rule.
No GPU."""
import json
import os

import pytest
import torch

from oracle import tacotron2_ref as R
from tests import reduction_ref as RR
from tests.helpers import GOLDEN, SMALL


def _small(seed=3, **extra):
    d = R.default_dims(**SMALL, dropout=0.5, **extra)
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in R.init_params(d, seed=seed).items()}
    return d, P


def _tf_case(d, B, L, T, r, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(3, L // 2), L + 1, (B,), generator=g); lens[0] = L
    tl = torch.randint(max(2, T // 2), T + 1, (B,), generator=g); tl[-1] = T
    ci = torch.zeros(B, L, dtype=torch.int64)
    mel = torch.zeros(B, T, d["num_mels"], dtype=torch.float64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
        mel[b, :tl[b]] = torch.randn(int(tl[b]), d["num_mels"], generator=g, dtype=torch.float64) - 2
    S = RR.steps_of(T, r)
    sm = lambda shape, p: (torch.rand(shape, generator=g) >= p).double() / (1 - p)
    E, Pd, A, D, Pn, M = d["encoded_dim"], d["prenet_dim"], d["att_rnn_dim"], d["rnn_hidden_dim"], d["postnet_dim"], d["num_mels"]
    masks = dict(enc_drop=[sm((B, L, E), 0.5) for _ in range(3)], prenet_drop=[sm((B, S + 1, Pd), 0.5) for _ in range(2)],
                 att_drop=sm((S, B, A), 0.1), dec_drop=sm((S, B, D), 0.1), post_drop=[sm((B, T, c), 0.5) for c in (Pn, Pn, Pn, Pn, M)])
    return ci, lens, mel, tl, masks


def _decode_case(d, P, B, L, N, seed):
    P = dict(P)
    P["decoder.gate.bias"] = P["decoder.gate.bias"] + 0.02       # stop logits cross zero at different steps (looked at when written)
    P["decoder.gate.weight"] = P["decoder.gate.weight"] * 6.0
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(3, L // 2), L + 1, (B,), generator=g); lens[0] = L
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    pm = (torch.rand(N + 1, 2, B, d["prenet_dim"], generator=g) >= 0.5).double() * 2
    return P, ci, lens, pm


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement at r = 1 is the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [{}, dict(controls=True, controls_dim=3, speaker_tokens=True, num_speakers=4)])
def test_r1_teacher_forcing_equals_the_oracle_exactly(extra):
    d, P = _small(**extra)
    ci, lens, mel, tl, masks = _tf_case(d, 3, 11, 9, 1, 21)
    kw = {}
    if extra:
        g = torch.Generator().manual_seed(1)
        kw = dict(controls=torch.randn(3, 3, generator=g, dtype=torch.float64), speaker_id=torch.tensor([0, 3, 1]))
    with torch.no_grad():
        ref = R.tacotron2_fwd(P, d, ci, lens, True, mel, tl, training=True, masks=masks, **kw)
        got = RR.reduction_fwd(P, d, 1, ci, lens, True, mel=mel, mel_len=tl, training=True, masks=masks, **kw)
    for a, b in zip(got, ref):
        assert a.dtype == torch.float64 and torch.equal(a, b)


def test_r1_decoding_equals_the_oracle_exactly_lengths_included():
    d, P = _small()
    N = 14
    P, ci, lens, pm = _decode_case(d, P, 4, 13, N, 5)
    masks = dict(prenet_drop=[[pm[i, 0], pm[i, 1]] for i in range(N + 1)])
    trace = {}
    with torch.no_grad():
        ref = R.tacotron2_fwd(P, d, ci, lens, False, max_len_override=N, training=False, masks=masks, trace=trace)
        got = RR.reduction_fwd(P, d, 1, ci, lens, False, max_len=N, training=False, masks=masks)
    for a, b in zip(got[:4], ref):
        assert torch.equal(a, b)
    assert torch.equal(got[4], trace["lengths"])
    assert 0 < int(got[4].min()) and len(set(got[4].tolist())) > 1          # the case stops at different frames


def test_r1_forward_attention_hook_is_the_forward_reference():
    from tests.test_forward_attention_host import forward_ref
    d, P = _small()
    N = 12
    P, ci, lens, pm = _decode_case(d, P, 4, 13, N, 6)
    with torch.no_grad():
        ref = forward_ref(P, d, ci, lens, N, prenet_drop=pm)
        got = RR.reduction_fwd(P, d, 1, ci, lens, False, max_len=N, training=False,
                               masks=dict(prenet_drop=[[pm[i, 0], pm[i, 1]] for i in range(N + 1)]),
                               attention_hook=RR.forward_attention_hook)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule at r > 1, by hand
# ---------------------------------------------------------------------------------------------------------------------------
def test_teacher_pack_indices_by_hand():
    assert RR.steps_of(5, 2) == 3 and RR.teacher_slots(5, 2) == [1, 3, None]          # steps 1, 2 see frames 1, 3
    assert RR.steps_of(7, 3) == 3 and RR.teacher_slots(7, 3) == [2, 5, None]
    assert RR.steps_of(8, 2) == 4 and RR.teacher_slots(8, 2) == [1, 3, 5, 7]
    assert RR.steps_of(1, 2) == 1 and RR.teacher_slots(1, 2) == [None]
    for T in range(1, 20):
        for r in range(1, 6):
            S = RR.steps_of(T, r)
            assert (S - 1) * r < T <= S * r
            assert all(i is not None and i < T for i in RR.teacher_slots(T, r)[:S - 1])     # what a step reads is inside the target


def test_decode_lengths_by_hand():
    # T = 5 (cap), r = 2: at most 3 steps; counted steps (2, 3, 0), 3 steps run -> 4, min(6, 5) = 5, 0 frames; 5 emitted
    lengths, n = RR.decode_lengths(torch.tensor([2, 3, 0]), 3, 2, 5)
    assert lengths.tolist() == [4, 5, 0] and n == 5
    # T = 7, r = 3: counted (1, 2, 3), stopped after 2 steps -> n = 6; after 3 -> n = 7 and lengths cut at 7
    lengths, n = RR.decode_lengths(torch.tensor([1, 2]), 2, 3, 7)
    assert lengths.tolist() == [3, 6] and n == 6
    lengths, n = RR.decode_lengths(torch.tensor([1, 2, 3]), 3, 3, 7)
    assert lengths.tolist() == [3, 6, 7] and n == 7


def test_restatement_at_r2_places_blocks_and_repeats_the_stop_logit():
    """Against a loop written out by hand for T = 5, r = 2 (no masks): frame s*2 + j is block j of step s, the gate repeats, step s
    sees target frame 2s - 1, the sixth frame is dropped."""
    d, P = _small()
    P = RR.grouped_params(P, d, 2, seed=1)
    ci, lens, mel, tl, _ = _tf_case(d, 2, 7, 5, 2, 22)
    tl = torch.tensor([5, 3], dtype=torch.int32)
    with torch.no_grad():
        mels, post, gates, al = RR.reduction_fwd(P, d, 2, ci, lens, True, mel=mel, mel_len=tl, training=False)
        enc = R.encoder_fwd(P, ci, lens, False)
        memory, pm = R.condition(P, d, enc)
        lmask = torch.arange(7)[None] >= lens[:, None]
        z = lambda n: torch.zeros(2, n, dtype=torch.float64)
        st = [z(32), z(32), z(32), z(7), z(7), z(32), z(32)]
        frames, logits = [], []
        for s, src in enumerate([None, 1, 3]):
            x = z(16) if src is None else mel[:, src]
            o = R.decoder_step(P, R.prenet_fwd(P, x, None, None), *st, memory, pm, lmask, None, None)
            st = list(o[2:])
            frames += [o[0][:, :16], o[0][:, 16:]]; logits += [o[1], o[1]]
    raw = torch.stack(frames[:5], 1); lg = torch.stack(logits[:5], 1)
    assert mels.shape == (2, 5, 16) and gates.shape == (2, 5, 1) and al.shape == (2, 3, 7)
    # (the restatement runs the prenet over all slots at once, this loop per step: float64 rounding apart)
    close = lambda x, y: float((x - y).abs().max()) < 1e-12
    assert close(mels[0], raw[0]) and close(mels[1, :3], raw[1, :3]) and float(mels[1, 3:].abs().max()) == 0.0
    assert close(gates[0], lg[0]) and torch.equal(gates[0, 0], gates[0, 1]) and bool((gates[1, 3:] == -1000.0).all())
    assert float((raw[0, 0] - raw[0, 1]).abs().max()) > 1e-3          # the two blocks of a step are different frames


# ---------------------------------------------------------------------------------------------------------------------------
# parameters, state_dict, checkpoints, arguments
# ---------------------------------------------------------------------------------------------------------------------------
def test_manifest_at_r1_is_the_recorded_one_and_r2_changes_only_mel_out():
    """tests/golden/param_manifest_r1.json: names, shapes, order and offsets of the flat buffer as they were before the option
    existed (vanilla dims, and small dims with controls, speaker tokens and descriptions)."""
    from tacotron2_amd.params import ParamStore, param_manifest
    rec = json.load(open(os.path.join(GOLDEN, "param_manifest_r1.json")))
    for name, c in rec.items():
        for d in (c["dims"], dict(c["dims"], reduction_factor=1)):
            ps = ParamStore(d, "cpu", with_grad=False)
            assert [[n, list(s), ps.offsets[n]] for n, s in ps.shapes.items()] == c["entries"], name
            assert ps.numel == c["numel"]
        d, d2 = c["dims"], dict(c["dims"], reduction_factor=2)
        m1, m2 = param_manifest(d), param_manifest(d2)
        assert list(m1) == list(m2)
        changed = [n for n in m1 if m1[n] != m2[n]]
        want = ["decoder.mel_out.weight", "decoder.mel_out.bias"] + (["decoder.mel_out.weight#controls"] if d["controls"] else [])
        assert changed == want
        M, K = m1["decoder.mel_out.weight"]
        assert m2["decoder.mel_out.weight"] == (2 * M, K) and m2["decoder.mel_out.bias"] == (2 * M,)
        assert m2["decoder.gate.weight"] == (1, K) and m2["prenet.0.weight"] == m1["prenet.0.weight"]
        ps2 = ParamStore(d2, "cpu", with_grad=False)      # [mel_out ; gate] stays one (r*M+1, D+Ef) matrix
        assert ps2.offsets["decoder.gate.weight"] == ps2.offsets["decoder.mel_out.weight"] + 2 * M * K
        assert ps2.offsets["decoder.gate.bias"] == ps2.offsets["decoder.mel_out.bias"] + 2 * M
        assert tuple(ps2.cat_view("decoder.mel_out.weight", 2 * M + 1, K).shape) == (2 * M + 1, K)


def test_state_dict_round_trip_at_r2_with_controls():
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    d = R.default_dims(**SMALL, dropout=0.5, controls=True, controls_dim=3, reduction_factor=2)
    ps = ParamStore(d, "cpu", with_grad=False)
    init_parameters(ps, 4)
    sd = ps.state_dict()
    M, K = 16, 32 + 32
    assert tuple(sd["decoder.mel_out.weight"].shape) == (2 * M, K + 3) and tuple(sd["decoder.mel_out.bias"].shape) == (2 * M,)
    assert tuple(sd["decoder.gate.weight"].shape) == (1, K) and tuple(sd["prenet.0.weight"].shape) == (16, M)
    ps2 = ParamStore(d, "cpu", with_grad=False)
    ps2.load_state_dict(sd)
    assert torch.equal(ps2.flat, ps.flat) and float(ps.flat.abs().sum()) > 0
    for k, v in ps2.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("bad", [0, -1, 2.0, "2", True, None])
def test_argument_errors(bad):
    from tacotron2_amd.model import Tacotron2, TTSModel
    from tacotron2_amd.params import ParamStore, check_reduction_factor
    kw = dict(SMALL, dropout=0.5)
    with pytest.raises(ValueError, match="reduction_factor must be an integer >= 1"):
        check_reduction_factor(bad)
    with pytest.raises(ValueError, match="reduction_factor"):
        ParamStore(dict(R.default_dims(**kw), reduction_factor=bad), "cpu")
    with pytest.raises(ValueError, match="reduction_factor"):
        Tacotron2(**kw, device="cpu", reduction_factor=bad)
    with pytest.raises(ValueError, match="reduction_factor"):
        TTSModel(lr=1e-3, weight_decay=0.0, device="cpu", reduction_factor=bad, **kw)


def test_module_surface_and_checkpoint_mismatch_message(tmp_path):
    from tacotron2_amd.model import Tacotron2, TTSModel
    kw = dict(SMALL, dropout=0.5)
    m1 = Tacotron2(**kw, device="cpu")
    assert m1.reduction_factor == 1 and "reduction_factor" not in m1.dims           # r = 1: the dims of before
    tm = TTSModel(lr=1e-3, weight_decay=0.0, device="cpu", reduction_factor=2, **kw)
    assert tm.tacotron2.reduction_factor == 2 and tm.tacotron2.dims["reduction_factor"] == 2
    assert tuple(tm.tacotron2.decoder.mel_out.weight.shape) == (32, 64) and tuple(tm.tacotron2.decoder.gate.weight.shape) == (1, 64)
    ck = tm.checkpoint()
    assert ck["hyper_parameters"]["reduction_factor"] == 2
    assert TTSModel(lr=1e-3, weight_decay=0.0, device="cpu", **kw).checkpoint()["hyper_parameters"]["reduction_factor"] == 1
    path = os.path.join(tmp_path, "r2.ckpt")
    torch.save(ck, path)
    back = TTSModel.load_from_checkpoint(path, device="cpu")
    assert back.tacotron2.reduction_factor == 2 and torch.equal(back.tacotron2.store.flat, tm.tacotron2.store.flat)
    # a configured r that disagrees with the file: the message names both values
    for r_cfg in (1, 3):
        with pytest.raises(ValueError, match=rf"written with reduction_factor = 2.*configured with reduction_factor = {r_cfg}"):
            TTSModel.load_from_checkpoint(path, device="cpu", reduction_factor=r_cfg)
    # ... also for a file from before the option (no key in its hyper_parameters)
    old = TTSModel(lr=1e-3, weight_decay=0.0, device="cpu", **kw).checkpoint()
    del old["hyper_parameters"]["reduction_factor"]
    torch.save(old, path)
    assert TTSModel.load_from_checkpoint(path, device="cpu").tacotron2.reduction_factor == 1
    with pytest.raises(ValueError, match=r"written with reduction_factor = 1.*configured with reduction_factor = 2"):
        TTSModel.load_from_checkpoint(path, device="cpu", reduction_factor=2)


def test_config_key_reaches_the_model_kwargs():
    from tacotron2_amd.run.common import model_kwargs
    cfg = dict(dataset=dict(preprocessing=dict(allowed_chars="abc", end_token="^", num_mels=16)),
               training=dict(lr=1e-3, weight_decay=0.0, args={}), model=dict(args=dict(encoded_dim=32, reduction_factor=2)),
               extensions=dict(controls=dict(active=False), speaker_tokens=dict(active=False)))
    assert model_kwargs(cfg)["reduction_factor"] == 2
    cfg["model"]["args"].pop("reduction_factor")
    assert "reduction_factor" not in model_kwargs(cfg)

