"""Forward attention for autoregressive decoding, host side: the float64 reference of the forward-attention decoder (used by
tests/test_gpu_forward_attention.py) checked against the oracle's plain decoder, the `--forward-attention` CLI flag, the
`model.forward_attention` config key and the argument validators."""
import os
import sys
import types

import pytest
import torch
from click.testing import CliRunner

from oracle import tacotron2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forward_weights(y, prior, lmask):
    """alpha(n) = q(n) y(n) / sum_m q(m) y(m), q(n) = 0.5 prior(n) + 0.5 prior(n-1) + 1e-8 (prior(-1) = 0); exactly 0 where lmask."""
    shifted = torch.cat([torch.zeros_like(prior[:, :1]), prior[:, :-1]], 1)
    q = 0.5 * prior + 0.5 * shifted + 1e-8
    a = q * y
    a = a / a.sum(1, keepdim=True)
    return a.masked_fill(lmask, 0.0)


def forward_ref(P, d, chars_idx, chars_len, max_len, speaker_id=None, prenet_drop=None, training=False, recursion=True):
    """tacotron2_fwd(teacher_forcing=False) with forward attention (Zhang et al. 2018, no transition agent): decoder_step's lines
    around the attention call restated, the softmax y_t replaced by alpha_t in the context, the cumulative weights, the returned
    alignments and the next frame's location features.  alpha_{-1} is one-hot at position 0; the location features of frame 0 see
    zeros.  recursion=False keeps y_t (the oracle's decoder).  prenet_drop: [n][2][B][P] scale masks or None.
    Returns (mels, post, gates, alignments, lengths)."""
    dt = P["prenet.0.weight"].dtype
    B, L = chars_idx.shape
    encoded = R.encoder_fwd(P, chars_idx, chars_len, training, None, None)
    memory, pm = R.condition(P, d, encoded, speaker_id)
    lmask = torch.arange(L)[None, :] >= chars_len[:, None]
    A, D, Ef = d["att_rnn_dim"], d["rnn_hidden_dim"], memory.shape[2]
    att_h = torch.zeros(B, A, dtype=dt); att_c = torch.zeros(B, A, dtype=dt)
    ctx = torch.zeros(B, Ef, dtype=dt)
    w = torch.zeros(B, L, dtype=dt); w_cum = torch.zeros_like(w)
    prior = torch.zeros(B, L, dtype=dt); prior[:, 0] = 1.0
    dec_h = torch.zeros(B, D, dtype=dt); dec_c = torch.zeros(B, D, dtype=dt)
    pd = lambda i, k: prenet_drop[i][k].to(dt) if prenet_drop is not None else None
    prev = R.prenet_fwd(P, torch.zeros(B, d["num_mels"], dtype=dt), pd(0, 0), pd(0, 1))
    done = torch.zeros(B, dtype=torch.bool)
    lengths = torch.zeros(B, dtype=torch.int64)
    mels, gates, aligns = [], [], []
    for i in range(max_len):
        # ---- R.decoder_step, with the recursion between the softmax and the context ----
        g = torch.cat([prev, ctx], -1) @ P["decoder.att_rnn.weight_ih"].T + P["decoder.att_rnn.bias_ih"] \
            + att_h @ P["decoder.att_rnn.weight_hh"].T + P["decoder.att_rnn.bias_hh"]
        att_h, att_c = R.lstm_cell(g, att_c)
        ctx, y = R.attention_fwd(P, att_h, memory, pm, torch.stack([w, w_cum], 1), lmask)
        if recursion:
            w = forward_weights(y, prior, lmask)
            ctx = torch.einsum("bl,ble->be", w, memory)
            prior = w
        else:
            w = y
        w_cum = w_cum + w
        g = torch.cat([att_h, ctx], -1) @ P["decoder.lstm.weight_ih"].T + P["decoder.lstm.bias_ih"] \
            + dec_h @ P["decoder.lstm.weight_hh"].T + P["decoder.lstm.bias_hh"]
        dec_h, dec_c = R.lstm_cell(g, dec_c)
        hc = torch.cat([dec_h, ctx], -1)
        gate_o = hc @ P["decoder.gate.weight"].T + P["decoder.gate.bias"]
        mel_o = torch.cat([hc], -1) @ P["decoder.mel_out.weight"].T + P["decoder.mel_out.bias"]
        # ---- the loop of R.tacotron2_fwd ----
        mels.append(mel_o); gates.append(gate_o); aligns.append(w)
        gg = gate_o[:, 0]
        done = done | (gg < 0.0)
        lengths = lengths + (gg >= 0.0).to(torch.int64)
        if bool(done.all()):
            break
        prev = R.prenet_fwd(P, mel_o, pd(i + 1, 0), pd(i + 1, 1))
    mels = torch.stack(mels, 1); gates = torch.stack(gates, 1); aligns = torch.stack(aligns, 1)
    post = mels + R.postnet_fwd(P, mels, training)
    mm = (torch.arange(mels.shape[1])[None, :] >= lengths[:, None])[:, :, None]
    return (mels.masked_fill(mm, 0.0), post.masked_fill(mm, 0.0), gates.masked_fill(mm, -1000.0), aligns, lengths)


def _small_case():
    d = R.default_dims(num_chars=39, encoded_dim=32, num_mels=16, prenet_dim=16, att_rnn_dim=32, att_dim=16,
                       rnn_hidden_dim=32, postnet_dim=32, dropout=0.5)
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in R.init_params(d, seed=3).items()}
    P["decoder.gate.bias"] = P["decoder.gate.bias"] + 0.3
    P["decoder.gate.weight"] = P["decoder.gate.weight"] * 6.0
    g = torch.Generator().manual_seed(5)
    B, L, N = 4, 17, 12
    lens = torch.tensor([17, 9, 13, 5])
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    pm = (torch.rand(N + 1, 2, B, 16, generator=g) >= 0.5).double() * 2
    return d, P, ci, lens, N, pm


def test_forward_reference_without_the_recursion_is_the_oracle_decoder():
    d, P, ci, lens, N, pm = _small_case()
    with torch.no_grad():
        ref = R.tacotron2_fwd(P, d, ci, lens, False, max_len_override=N, training=False,
                              masks=dict(prenet_drop=[[pm[i, 0], pm[i, 1]] for i in range(N + 1)]))
        got = forward_ref(P, d, ci, lens, N, prenet_drop=pm, recursion=False)
    for r, o in zip(ref, got[:4]):
        assert r.shape == o.shape and torch.equal(r, o)


def test_forward_reference_rows_are_monotonic_distributions():
    d, P, ci, lens, N, pm = _small_case()
    L = ci.shape[1]
    with torch.no_grad():
        plain = forward_ref(P, d, ci, lens, N, prenet_drop=pm, recursion=False)[3]
        al = forward_ref(P, d, ci, lens, N, prenet_drop=pm)[3]
    assert float((al.sum(2) - 1.0).abs().max()) < 1e-12
    past = (torch.arange(L)[None, :] >= lens[:, None])[:, None, :].expand_as(al)
    assert float(al[past].abs().max()) == 0.0
    t = torch.arange(al.shape[1])[None, :]
    assert bool((al.argmax(2) <= t + 1).all())
    # the first frame is the prior (0.5, 0.5, 1e-8, ...) times the softmax, renormalised: it is not the plain decoder's row
    n = min(al.shape[1], plain.shape[1])
    assert float((al[:, :n] - plain[:, :n]).abs().max()) > 1e-2


def test_forward_weights_rule():
    """One step of the rule by hand: the prior of frame 0, the shift, the floor and the zero past the length."""
    y = torch.tensor([[0.1, 0.2, 0.3, 0.4, 0.0]], dtype=torch.float64)
    lmask = torch.tensor([[False, False, False, False, True]])
    prior = torch.tensor([[1.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    a = forward_weights(y, prior, lmask)
    q = torch.tensor([0.5 + 1e-8, 0.5 + 1e-8, 1e-8, 1e-8], dtype=torch.float64)
    want = q * y[0, :4] / (q * y[0, :4]).sum()
    assert torch.allclose(a[0, :4], want, rtol=0, atol=1e-15) and float(a[0, 4]) == 0.0
    # the softmax's mass where the prior is zero: the floor keeps the sum positive, the row is still a distribution
    y2 = torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0]], dtype=torch.float64)
    a2 = forward_weights(y2, prior, lmask)
    assert torch.equal(a2, torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0]], dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# CLI: --forward-attention on say / test / test-correlation (the do_* functions are replaced: no GPU, no checkpoint)
# ---------------------------------------------------------------------------------------------------------------------------
def _cli(monkeypatch, tmp_path, model="{}"):
    sys.path.insert(0, ROOT)
    import main as cli
    import tacotron2_amd.run.say as say
    import tacotron2_amd.run.test as test
    import tacotron2_amd.run.test_correlation as tc
    seen = {}
    for mod, name in ((say, "do_say"), (test, "do_test"), (tc, "do_test_correlation")):
        monkeypatch.setattr(mod, name, lambda _n=name, **kw: seen.__setitem__(_n, kw))
    cfg = tmp_path / "cfg.json"
    cfg.write_text('{"dataset": {"preprocessing": {"allowed_chars": "ab"}}, "training": {}, "model": %s, "extensions": {}}' % model)
    return cli, seen, ["--config", str(cfg)]


CMDS = [
    ("say", "do_say", ["--checkpoint", "k.ckpt", "--text", "hi"]),
    ("test", "do_test", ["--speech-dir", "s", "--checkpoint", "k.ckpt"]),
    ("test-correlation", "do_test_correlation", ["--speech-dir", "s", "--checkpoint", "k.ckpt"]),
]


@pytest.mark.parametrize("cmd,fn,args", CMDS)
def test_cli_forward_attention_reaches_the_driver(monkeypatch, tmp_path, cmd, fn, args):
    cli, seen, pre = _cli(monkeypatch, tmp_path)
    # say / test take the flag as an argument; test-correlation through the model config (load_test_model reads it)
    got = (lambda kw: kw["forward_attention"]) if fn != "do_test_correlation" else \
        (lambda kw: kw["model_config"].get("forward_attention"))
    r = CliRunner().invoke(cli.main, pre + [cmd] + args + ["--forward-attention"], obj={})
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert got(seen[fn]) is True
    seen.clear()
    r = CliRunner().invoke(cli.main, pre + [cmd] + args, obj={})          # default: left to the config, which has no key = off
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert got(seen[fn]) is None


@pytest.mark.parametrize("cmd,fn,args", CMDS)
def test_cli_forward_attention_with_a_window_is_a_usage_error(monkeypatch, tmp_path, cmd, fn, args):
    cli, seen, pre = _cli(monkeypatch, tmp_path)
    r = CliRunner().invoke(cli.main, pre + [cmd] + args + ["--forward-attention", "--attention-window", "1,3"], obj={})
    assert r.exit_code == 2 and "forward-attention" in r.output, r.output
    assert not seen


def test_forward_attention_argument_checks():
    from tacotron2_amd.engine import check_forward_attention
    assert check_forward_attention(False) is False and check_forward_attention(True) is True
    assert check_forward_attention(False, (1, 3)) is False
    for bad in [None, 1, 0, "yes", 1.0, (True,)]:
        with pytest.raises(ValueError):
            check_forward_attention(bad)
    with pytest.raises(ValueError):
        check_forward_attention(True, (1, 3))


def test_engine_and_module_refuse_teacher_forcing_and_windows():
    """The validators run before anything touches a device: Engine.infer and Tacotron2.forward raise on CPU tensors."""
    from tacotron2_amd.engine import Engine
    from tacotron2_amd.model import Tacotron2
    ci, ln = torch.zeros(1, 4, dtype=torch.int64), torch.tensor([4])
    eng = Engine.__new__(Engine)                    # no device state: infer must refuse before it uses any
    with pytest.raises(ValueError):
        eng.infer(ci, ln, 3, attention_window=(1, 3), forward_attention=True)
    with pytest.raises(ValueError):
        eng.infer(ci, ln, 3, forward_attention=1)
    fwd = types.SimpleNamespace(training=False)
    mel = torch.zeros(1, 4, 16)
    with pytest.raises(ValueError):                 # teacher forcing
        Tacotron2.forward(fwd, ci, ln, True, mel, ln, forward_attention=True)
    with pytest.raises(ValueError):                 # with a window
        Tacotron2.forward(fwd, ci, ln, False, max_len_override=3, attention_window=(1, 3), forward_attention=True)
    with pytest.raises(ValueError):                 # not a bool
        Tacotron2.forward(fwd, ci, ln, False, max_len_override=3, forward_attention="on")


def _loader(monkeypatch):
    import tacotron2_amd.run.test as T
    mk = lambda *a, **k: types.SimpleNamespace(eval=lambda: None, tacotron2=types.SimpleNamespace(_seed=0))
    monkeypatch.setattr(T.TTSModel, "load_from_checkpoint", mk)
    ds = {"preprocessing": {"allowed_chars": "ab"}}
    tr = {"lr": 1e-3, "weight_decay": 0.0}
    ext = {"speaker_tokens": {"active": False}, "controls": {"active": False}}
    return lambda md, w=None, f=None: T.load_test_model(ds, tr, md, ext, "k.ckpt", "cpu", None, w, f)


def test_load_test_model_sets_forward_attention_from_argument_or_config(monkeypatch):
    """run/test.py:load_test_model (shared by test and test-correlation): the argument wins, else the config's
    model.forward_attention, else off; a value that is not a bool, or the option together with a window, is refused."""
    load = _loader(monkeypatch)
    assert load({}).forward_attention is False
    assert load({"forward_attention": True}).forward_attention is True
    assert load({"forward_attention": False}, None, True).forward_attention is True      # the flag wins over the config
    assert load({}, None, True).forward_attention is True
    assert load({"attention_window": [1, 3]}).forward_attention is False
    for md, w, f in [({"forward_attention": "yes"}, None, None), ({"forward_attention": 1}, None, None),
                     ({"forward_attention": True, "attention_window": [1, 3]}, None, None),
                     ({"forward_attention": True}, (1, 3), None), ({"attention_window": [1, 3]}, None, True)]:
        with pytest.raises(ValueError):
            load(md, w, f)


def test_cli_config_key_is_honoured_and_the_flag_wins(monkeypatch, tmp_path):
    """main.py hands the config's model section to the drivers untouched and None for the absent flag, so load_test_model / do_say
    take model.forward_attention; with the flag they get True whatever the config says."""
    load = _loader(monkeypatch)
    for model, flag, want in [('{"forward_attention": true}', [], True), ('{"forward_attention": false}', [], False),
                              ('{"forward_attention": false}', ["--forward-attention"], True), ('{}', [], False)]:
        cli, seen, pre = _cli(monkeypatch, tmp_path, model)
        r = CliRunner().invoke(cli.main, pre + ["test", "--speech-dir", "s", "--checkpoint", "k.ckpt"] + flag, obj={})
        assert r.exit_code == 0, r.output + repr(r.exception)
        kw = seen["do_test"]
        assert load(kw["model_config"], kw["attention_window"], kw["forward_attention"]).forward_attention is want
        seen.clear()
        r = CliRunner().invoke(cli.main, pre + ["test-correlation", "--speech-dir", "s", "--checkpoint", "k.ckpt"] + flag, obj={})
        assert r.exit_code == 0, r.output + repr(r.exception)
        assert load(seen["do_test_correlation"]["model_config"]).forward_attention is want


def test_synthesize_manifest_decodes_with_the_models_forward_attention(tmp_path):
    """The batched decode loop of test / test-correlation passes TTSModel.forward_attention to every forward."""
    import pandas as pd
    import tacotron2_amd.run.test as T
    calls = []

    class Model:
        description_embeddings, speaker_tokens, attention_window, forward_attention = False, False, None, True
        tacotron2 = types.SimpleNamespace(store=types.SimpleNamespace(device=torch.device("cpu")))

        def __call__(self, **kw):
            calls.append(kw)
            B = kw["chars_idx"].shape[0]
            return None, torch.zeros(B, 3, 4), torch.full((B, 3, 1), -1.0), None     # never stops: logged, nothing written
    df = pd.DataFrame({"text": ["ab", "ba", "a"]})
    T.synthesize_manifest(Model(), df, {"allowed_chars": "ab"}, None, str(tmp_path), None, object(), 22050, None, batch_size=2)
    assert len(calls) == 2
    assert all(c["forward_attention"] is True and c["attention_window"] is None and not c["teacher_forcing"] for c in calls)
