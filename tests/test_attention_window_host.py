"""Windowed (monotonic) attention for autoregressive decoding, host side: the float64 reference of the windowed decoder (used by
tests/test_gpu_attention_window.py) checked against the oracle's unconstrained decoder, and the `--attention-window` CLI option."""
import os
import sys

import pytest
import torch
from click.testing import CliRunner

from oracle import tacotron2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def window_mask(peak, lens, L, window):
    """(B, L) bool, True = not allowed: positions outside max(0, m - back) .. min(len - 1, m + fwd) around the peaks m."""
    back, fwd = window
    pos = torch.arange(L)[None, :]
    lo = (peak - back).clamp(min=0)[:, None]
    hi = torch.minimum(lens - 1, peak + fwd)[:, None]
    return (pos < lo) | (pos > hi)


def windowed_ref(P, d, chars_idx, chars_len, max_len, window, speaker_id=None, prenet_drop=None, training=False):
    """tacotron2_fwd(teacher_forcing=False) with the attention window: at frame t the mask is the length mask OR the window
    around the previous frame's argmax (0 before the first frame).  prenet_drop: [n][2][B][P] scale masks or None.
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
    dec_h = torch.zeros(B, D, dtype=dt); dec_c = torch.zeros(B, D, dtype=dt)
    pd = lambda i, k: prenet_drop[i][k].to(dt) if prenet_drop is not None else None
    prev = R.prenet_fwd(P, torch.zeros(B, d["num_mels"], dtype=dt), pd(0, 0), pd(0, 1))
    done = torch.zeros(B, dtype=torch.bool)
    lengths = torch.zeros(B, dtype=torch.int64)
    peak = torch.zeros(B, dtype=torch.int64)
    mels, gates, aligns = [], [], []
    for i in range(max_len):
        mask = lmask | window_mask(peak, chars_len, L, window)
        mel_o, gate_o, att_h, att_c, ctx, w, w_cum, dec_h, dec_c = R.decoder_step(
            P, prev, att_h, att_c, ctx, w, w_cum, dec_h, dec_c, memory, pm, mask, None, None)
        peak = w.argmax(1)
        mels.append(mel_o); gates.append(gate_o); aligns.append(w)
        g = gate_o[:, 0]
        done = done | (g < 0.0)
        lengths = lengths + (g >= 0.0).to(torch.int64)
        if bool(done.all()):
            break
        prev = R.prenet_fwd(P, mel_o, pd(i + 1, 0), pd(i + 1, 1))
    mels = torch.stack(mels, 1); gates = torch.stack(gates, 1); aligns = torch.stack(aligns, 1)
    post = mels + R.postnet_fwd(P, mels, training)
    mm = (torch.arange(mels.shape[1])[None, :] >= lengths[:, None])[:, :, None]
    return (mels.masked_fill(mm, 0.0), post.masked_fill(mm, 0.0), gates.masked_fill(mm, -1000.0), aligns, lengths)


def test_windowed_reference_with_full_window_is_the_oracle_decoder():
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
    with torch.no_grad():
        ref = R.tacotron2_fwd(P, d, ci, lens, False, max_len_override=N, training=False,
                              masks=dict(prenet_drop=[[pm[i, 0], pm[i, 1]] for i in range(N + 1)]))
        got = windowed_ref(P, d, ci, lens, N, (L, L), prenet_drop=pm)
    for r, o in zip(ref, got[:4]):
        assert r.shape == o.shape and torch.equal(r, o)
    # a narrow window: every alignment row lives inside the window around the previous row's peak
    with torch.no_grad():
        al = windowed_ref(P, d, ci, lens, N, (0, 1), prenet_drop=pm)[3]
    peak = torch.zeros(B, dtype=torch.int64)
    for t in range(al.shape[1]):
        outside = window_mask(peak, lens, L, (0, 1))
        assert float(al[:, t][outside].abs().max()) == 0.0
        peak = al[:, t].argmax(1)


# ---------------------------------------------------------------------------------------------------------------------------
# CLI: --attention-window BACK,FWD on say / test / test-correlation (the do_* functions are replaced: no GPU, no checkpoint)
# ---------------------------------------------------------------------------------------------------------------------------
def _cli(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    import tacotron2_amd.run.say as say
    import tacotron2_amd.run.test as test
    import tacotron2_amd.run.test_correlation as tc
    seen = {}
    for mod, name in ((say, "do_say"), (test, "do_test"), (tc, "do_test_correlation")):
        monkeypatch.setattr(mod, name, lambda _n=name, **kw: seen.__setitem__(_n, kw))
    cfg = tmp_path / "cfg.json"
    cfg.write_text('{"dataset": {"preprocessing": {"allowed_chars": "ab"}}, "training": {}, "model": {}, "extensions": {}}')
    return cli, seen, ["--config", str(cfg)]


@pytest.mark.parametrize("cmd,fn,args", [
    ("say", "do_say", ["--checkpoint", "k.ckpt", "--text", "hi"]),
    ("test", "do_test", ["--speech-dir", "s", "--checkpoint", "k.ckpt"]),
    ("test-correlation", "do_test_correlation", ["--speech-dir", "s", "--checkpoint", "k.ckpt"]),
])
def test_cli_attention_window_reaches_the_driver(monkeypatch, tmp_path, cmd, fn, args):
    cli, seen, pre = _cli(monkeypatch, tmp_path)
    # say / test take the window as an argument; test-correlation through the model config (load_test_model reads it)
    got = (lambda kw: kw["attention_window"]) if fn != "do_test_correlation" else \
        (lambda kw: kw["model_config"].get("attention_window"))
    r = CliRunner().invoke(cli.main, pre + [cmd] + args + ["--attention-window", "1,3"], obj={})
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert tuple(got(seen[fn])) == (1, 3)
    seen.clear()
    r = CliRunner().invoke(cli.main, pre + [cmd] + args, obj={})          # default: off
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert got(seen[fn]) is None


@pytest.mark.parametrize("bad", ["-1,3", "1", "a,b", "1,2,3", "1,-2", "1.5,3", ""])
def test_cli_attention_window_malformed_is_a_usage_error(monkeypatch, tmp_path, bad):
    cli, seen, pre = _cli(monkeypatch, tmp_path)
    r = CliRunner().invoke(cli.main, pre + ["say", "--checkpoint", "k.ckpt", "--text", "hi", "--attention-window", bad], obj={})
    assert r.exit_code == 2 and "attention-window" in r.output, r.output
    assert not seen


def test_attention_window_argument_checks():
    from tacotron2_amd.engine import check_attention_window
    assert check_attention_window(None) is None
    assert check_attention_window((1, 3)) == (1, 3) and check_attention_window([0, 0]) == (0, 0)
    for bad in [(-1, 3), (1,), (1, 2, 3), (1.0, 3), ("1", "3"), (True, 2), 5]:
        with pytest.raises(ValueError):
            check_attention_window(bad)


def test_load_test_model_sets_the_window_from_argument_or_config(monkeypatch):
    """run/test.py:load_test_model (shared by test and test-correlation): the argument wins, else the config's
    model.attention_window, else off; a malformed config value is refused."""
    import types
    import tacotron2_amd.run.test as T
    mk = lambda *a, **k: types.SimpleNamespace(eval=lambda: None, tacotron2=types.SimpleNamespace(_seed=0))
    monkeypatch.setattr(T.TTSModel, "load_from_checkpoint", mk)
    ds = {"preprocessing": {"allowed_chars": "ab"}}
    tr = {"lr": 1e-3, "weight_decay": 0.0}
    ext = {"speaker_tokens": {"active": False}, "controls": {"active": False}}
    load = lambda md, w=None: T.load_test_model(ds, tr, md, ext, "k.ckpt", "cpu", None, w)
    assert load({}).attention_window is None
    assert load({"attention_window": [1, 3]}).attention_window == (1, 3)
    assert load({"attention_window": [1, 3]}, (0, 2)).attention_window == (0, 2)
    with pytest.raises(ValueError):
        load({"attention_window": [-1, 3]})


def test_synthesize_manifest_decodes_with_the_models_window(tmp_path):
    """The batched decode loop of test / test-correlation passes TTSModel.attention_window to every forward."""
    import types
    import pandas as pd
    import tacotron2_amd.run.test as T
    calls = []

    def fwd(**kw):
        calls.append(kw)
        B = kw["chars_idx"].shape[0]
        return None, torch.zeros(B, 3, 4), torch.full((B, 3, 1), -1.0), None     # never stops: logged, nothing written
    class Model:
        description_embeddings, speaker_tokens, attention_window = False, False, (1, 3)
        tacotron2 = types.SimpleNamespace(store=types.SimpleNamespace(device=torch.device("cpu")))

        def __call__(self, **kw):
            return fwd(**kw)
    df = pd.DataFrame({"text": ["ab", "ba", "a"]})
    T.synthesize_manifest(Model(), df, {"allowed_chars": "ab"}, None, str(tmp_path), None, object(), 22050, None, batch_size=2)
    assert len(calls) == 2 and all(c["attention_window"] == (1, 3) and not c["teacher_forcing"] for c in calls)

