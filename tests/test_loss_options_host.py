"""Loss options and the stop threshold on the host (CPU only): the float64 restatement (tests/loss_options_ref.py) against
torch.autograd on torch's own losses, the option checks of engine.py and the config / command-line parsers of run/common.py and
main.py, and the count rule with a threshold on the hand-made sign table of tests/test_gpu_reduction_factor.py's stop-scan test."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import loss_options_ref as LR


def _case(seed=58, B=3, T=7, M=5, lens=(7, 4, 1)):
    g = torch.Generator().manual_seed(seed)
    d = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    tgt = d(B, T, M) - 2
    mels, post = d(B, T, M) - 2, d(B, T, M) - 2
    mels[:, 0, ::2] = tgt[:, 0, ::2]                  # errors that are exactly 0
    gates = 1.5 * d(B, T, 1)
    gtgt = (torch.rand(B, T, 1, generator=g) > 0.3).double()
    return mels, post, gates, tgt, gtgt, torch.tensor(lens, dtype=torch.int32)


def _torch_terms(mels, post, gates, tgt, gtgt, lens, mel_loss, masked, w):
    """The same three terms from torch's own losses: F.l1_loss / F.mse_loss, and the stop-class weight through the identity
    BCE_w(x, y) = BCE_{pos_weight = w}(-x, 1 - y); the masked means by indexing the valid frames."""
    if masked:
        v = LR.valid_mask(lens, mels.shape[1])
        mels, post, tgt, gates, gtgt = mels[v], post[v], tgt[v], gates[v], gtgt[v]
    mel = lambda a: (F.mse_loss(a, tgt) if "l2" in mel_loss else 0) + (F.l1_loss(a, tgt) if "l1" in mel_loss else 0)
    gate = F.binary_cross_entropy_with_logits(-gates, 1 - gtgt, pos_weight=torch.tensor(w, dtype=torch.float64))
    return gate, mel(mels), mel(post)


@pytest.mark.parametrize("mel_loss,masked,w", list(itertools.product(LR.MEL_LOSSES, (False, True), (1.0, 8.0))))
def test_restatement_matches_autograd_on_torch_losses(mel_loss, masked, w):
    mels, post, gates, tgt, gtgt, lens = _case()
    x = [t.clone().requires_grad_(True) for t in (mels, post, gates)]
    want3 = _torch_terms(x[0], x[1], x[2], tgt, gtgt, lens, mel_loss, masked, w)
    got3 = LR.loss_terms(mels, post, gates, tgt, gtgt, lens, mel_loss, masked, w)
    for a, b in zip(got3, want3):
        assert abs(float(a) - float(b.detach())) < 1e-12 * max(1.0, abs(float(b.detach())))
    gm, gp, gg = torch.autograd.grad(sum(want3), x)
    live = LR.valid_mask(lens, mels.shape[1])[:, :, None].double()       # positions at or beyond len are constants
    dm, dp, dg = LR.loss_grads(mels, post, gates, tgt, gtgt, lens, mel_loss, masked, w)
    for a, b in ((dm, gm * live), (dp, gp * live), (dg, gg * live)):
        assert float((a - b).abs().max()) < 1e-14
    # and autograd on the restatement's own differentiable form
    y = [t.clone().requires_grad_(True) for t in (mels, post, gates)]
    g2 = torch.autograd.grad(sum(LR.loss_terms(y[0], y[1], y[2], tgt, gtgt, lens, mel_loss, masked, w)), y)
    for a, b in zip((dm, dp, dg), g2):
        assert float((a - b * live).abs().max()) < 1e-14
    if "l1" == mel_loss:
        assert float(dm[:, 0, ::2].abs().max()) == 0.0                    # sign(0) = 0


def test_restatement_masked_mode_ignores_nan_padding_and_empty_batches():
    mels, post, gates, tgt, gtgt, lens = _case()
    inv = ~LR.valid_mask(lens, 7)[:, :, None]
    nan = [t.masked_fill(inv, float("nan")) for t in (mels, post, gates, tgt, gtgt)]
    a = LR.loss_terms(mels, post, gates, tgt, gtgt, lens, "l1+l2", True, 8.0)
    b = LR.loss_terms(*nan, lens, "l1+l2", True, 8.0)
    assert all(float(x) == float(y) for x, y in zip(a, b))
    ga, gb = LR.loss_grads(mels, post, gates, tgt, gtgt, lens, "l1+l2", True, 8.0), LR.loss_grads(*nan, lens, "l1+l2", True, 8.0)
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))
    zero = torch.zeros(3, dtype=torch.int32)
    assert all(float(x) == 0.0 for x in LR.loss_terms(*nan, zero, "l1", True, 2.0))
    assert all(float(x.abs().max()) == 0.0 for x in LR.loss_grads(*nan, zero, "l1", True, 2.0))


def test_pack_dproj_sums_the_gate_gradient_over_the_step():
    mels, post, gates, tgt, gtgt, lens = _case()
    dm, dp, dg = LR.loss_grads(mels, post, gates, tgt, gtgt, lens, "l1", True, 8.0)
    q = LR.pack_dproj(dm, dp, dg, 3)                      # T = 7: steps of frames (0,1,2) (3,4,5) (6,-,-)
    assert q.shape == (3, 3, 16)
    assert torch.equal(q[1, :, 5:10], (dm + dp)[:, 4]) and float(q[2, :, 5:15].abs().max()) == 0.0
    assert torch.allclose(q[1, :, 15], dg[:, 3:6, 0].sum(1), rtol=0, atol=1e-15) and torch.equal(q[2, :, 15], dg[:, 6, 0])
    assert torch.equal(LR.pack_dproj(dm, dp, dg, 1)[:, :, 5], dg[:, :, 0].t())


# ---------------------------------------------------------------------------------------------------------------------------
# option checks and parsers
# ---------------------------------------------------------------------------------------------------------------------------
def test_check_loss_options():
    from tacotron2_amd.engine import LOSS_DEFAULTS, MEL_LOSSES, check_loss_options
    assert MEL_LOSSES == LR.MEL_LOSSES and LOSS_DEFAULTS == ("l2", False, 1.0)
    assert check_loss_options(None) == LOSS_DEFAULTS and check_loss_options({}) == LOSS_DEFAULTS
    assert check_loss_options({"mel": "l1+l2"}) == ("l1+l2", False, 1.0)
    assert check_loss_options({"masked": True, "stop_weight": 8}) == ("l2", True, 8.0)
    assert check_loss_options(("l1", True, 2.5)) == ("l1", True, 2.5) and check_loss_options(["l1", False, 1]) == ("l1", False, 1.0)
    assert isinstance(check_loss_options(("l1", True, 8))[2], float)
    for bad, word in (({"mel": "l3"}, "'l3'"), ({"mel": 1}, "1"), ({"masked": 1}, "masked"), ({"masked": "yes"}, "'yes'"),
                      ({"stop_weight": 0}, "0"), ({"stop_weight": -1.0}, "-1.0"), ({"stop_weight": float("nan")}, "nan"),
                      ({"stop_weight": float("inf")}, "inf"), ({"stop_weight": True}, "True"), ({"stop_weight": "8"}, "'8'"),
                      ({"stop_weight": 1e39}, "1e+39"), ({"stop_weight": 1e-50}, "1e-50"), ({"weight": 2.0}, "'weight'"),
                      (("l1", True), "('l1', True)"), (5, "5"), ("l1", "'l1'")):
        with pytest.raises(ValueError, match="loss options") as e:
            check_loss_options(bad)
        assert word in str(e.value), (bad, str(e.value))


def test_stop_threshold_check_and_logit():
    from tacotron2_amd.engine import check_stop_threshold, stop_logit
    assert check_stop_threshold(0.5) == 0.5 and check_stop_threshold(0.4) == 0.4
    assert stop_logit(0.5) == 0.0 and math.copysign(1.0, stop_logit(0.5)) == 1.0          # +0.0: `x < 0.0f`, the comparison as it was
    for tau in (0.3, 0.4, 0.7, 0.999):
        v = stop_logit(tau)
        assert v == LR.stop_logit(tau) and v == float(torch.tensor(math.log(tau / (1 - tau)), dtype=torch.float64).float())
    assert stop_logit(0.3) == -stop_logit(0.7) or abs(stop_logit(0.3) + stop_logit(0.7)) < 1e-6
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), True, "0.4", None):
        with pytest.raises(ValueError, match="stop_threshold") as e:
            check_stop_threshold(bad)
        assert repr(bad) in str(e.value)


def test_config_and_command_line_settings():
    from tacotron2_amd.run.common import loss_options_setting, stop_threshold_setting
    assert loss_options_setting({}) == ("l2", False, 1.0) and loss_options_setting({"loss": None}) == ("l2", False, 1.0)
    sec = {"loss": {"mel": "l1+l2", "masked": True, "stop_weight": 8.0}}
    assert loss_options_setting(sec) == ("l1+l2", True, 8.0)
    assert loss_options_setting({"loss": {"masked": True}}) == ("l2", True, 1.0)                  # any key may be left out
    assert loss_options_setting(sec, mel="l1") == ("l1", True, 8.0)                                # the option wins, key by key
    assert loss_options_setting(sec, stop_weight=2.0) == ("l1+l2", True, 2.0)
    assert loss_options_setting({"loss": {"mel": "l1"}}, masked=True) == ("l1", True, 1.0)
    assert loss_options_setting({}, "l1+l2", True, 8.0) == ("l1+l2", True, 8.0)
    assert loss_options_setting(sec, masked=False) == ("l1+l2", False, 8.0)                        # --no-masked-loss switches the key off
    assert loss_options_setting(sec, "l2", False, 1.0) == ("l2", False, 1.0)
    for bad, word in (({"loss": "l1"}, "'l1'"), ({"loss": {"mel": "L1"}}, "'L1'"), ({"loss": {"stop_weight": 0}}, "0"),
                      ({"loss": {"mask": True}}, "'mask'")):
        with pytest.raises(ValueError) as e:
            loss_options_setting(bad)
        assert word in str(e.value)
    assert stop_threshold_setting({}) == 0.5 and stop_threshold_setting({"stop_threshold": 0.4}) == 0.4
    assert stop_threshold_setting({"stop_threshold": 0.4}, 0.6) == 0.6
    with pytest.raises(ValueError, match="1.2"):
        stop_threshold_setting({"stop_threshold": 1.2})


def test_command_line_options_parse_or_refuse():
    import click
    import main as cli
    assert cli.parse_stop_threshold(None, None, None) is None and cli.parse_stop_threshold(None, None, "0.4") == 0.4
    assert cli.parse_stop_weight(None, None, None) is None and cli.parse_stop_weight(None, None, "8") == 8.0
    for fn, bad in ((cli.parse_stop_threshold, "1"), (cli.parse_stop_threshold, "0"), (cli.parse_stop_threshold, "x"),
                    (cli.parse_stop_weight, "0"), (cli.parse_stop_weight, "-2"), (cli.parse_stop_weight, "nan"),
                    (cli.parse_stop_weight, "w")):
        with pytest.raises(click.BadParameter, match=bad):
            fn(None, None, bad)
    names = {c: {o.name for o in cli.main.commands[c].params} for c in ("train", "say", "test", "test-correlation")}
    assert {"mel_loss", "masked_loss", "stop_weight"} <= names["train"] and "stop_threshold" not in names["train"]
    masked = next(o for o in cli.main.commands["train"].params if o.name == "masked_loss")
    assert masked.opts == ["--masked-loss"] and masked.secondary_opts == ["--no-masked-loss"] and masked.default is None
    assert all("stop_threshold" in names[c] for c in ("say", "test", "test-correlation"))


def test_usage_errors_of_the_module_surface():
    """stop_threshold together with teacher forcing is a usage error, like forward_attention; checked before any device work."""
    from tacotron2_amd.model.tacotron2 import Tacotron2
    x = torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="stop_threshold applies to autoregressive decoding only"):
        Tacotron2.forward(None, x, torch.tensor([3]), True, mel_spectrogram=torch.zeros(1, 2, 80),
                          mel_spectrogram_len=torch.tensor([2]), stop_threshold=0.4)
    with pytest.raises(ValueError, match="stop_threshold must be"):
        Tacotron2.forward(None, x, torch.tensor([3]), False, max_len_override=5, stop_threshold=1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the count rule with a threshold
# ---------------------------------------------------------------------------------------------------------------------------
SIGN = {0: [1, -1, 1, 1, -1], 1: [1, 1, 1, -1, 1], 2: [1, 1, 1, 1, 1], 3: [-1, 1, -1, 1, -1], 4: [1, 1, -1, -1, 1]}


def _table(utts, shift=0.0):
    return torch.tensor([[0.5 * s + shift for s in SIGN[u]] for u in utts], dtype=torch.float32).t().contiguous()


def test_count_rule_on_the_sign_table_shifted_by_a_threshold():
    """The table of tests/test_gpu_reduction_factor.py's stop-scan test and its hand-counted results; logits 0.5 * sign + logit(tau)
    against logit(tau) are the same decisions, for any tau."""
    hand = (([0, 1, 2, 3, 4], 3, 13, [9, 12, 13, 6, 9], 13, 5), ([0, 1, 3, 4], 3, 13, [9, 9, 6, 6], 12, 4),
            ([0, 1, 3, 4], 3, 100, [9, 9, 6, 6], 12, 4), ([2], 3, 14, [14], 14, 5), ([0, 1, 2, 3, 4], 1, 100, [3, 4, 5, 2, 3], 5, 5),
            ([0, 1, 3, 4], 1, 100, [3, 3, 2, 2], 4, 4), ([0, 1, 2, 3, 4], 1, 3, [3, 3, 3, 2, 3], 3, 5))
    for tau in (0.5, 0.3, 0.7, 0.05):
        thr = LR.stop_logit(tau)
        for utts, r, max_len, lengths, frames, steps in hand:
            got = LR.stop_count(_table(utts, thr), thr, r, max_len)
            assert (got[0].tolist(), got[1], got[2]) == (lengths, frames, steps), (tau, utts, r, max_len, got)
    # the unshifted table under a threshold: at tau = 0.7 (logit 0.847) every +0.5 is a stop, at 0.3 (-0.847) nothing is
    got = LR.stop_count(_table([0, 1, 3, 4]), LR.stop_logit(0.7), 1, 100)
    assert (got[0].tolist(), got[1], got[2]) == ([0, 0, 0, 0], 1, 1)
    got = LR.stop_count(_table([0, 1, 3, 4]), LR.stop_logit(0.3), 1, 100)
    assert (got[0].tolist(), got[1], got[2]) == ([5, 5, 5, 5], 5, 5)
    # a logit equal to the threshold continues (the rule is logit < threshold)
    thr = LR.stop_logit(0.3)
    assert LR.stop_count(torch.tensor([[thr], [thr - 1e-3]]), thr)[0].tolist() == [1]


def test_driver_length_rule_follows_the_threshold():
    """run/test.py's mel_lengths: the first frame below logit(threshold); a kept frame with a logit in [logit(tau), 0) is not a stop."""
    from tacotron2_amd.run.test import mel_lengths_of
    gate = torch.tensor([[0.4, -0.3, -0.5, -1000.0, -1000.0], [0.2, 0.1, 0.3, 0.2, 0.1], [-0.1, -1000.0, -1000.0, -1000.0, -1000.0]])
    assert mel_lengths_of(gate[:, :, None], 0.3).tolist() == [3, 0, 1]
    assert mel_lengths_of(gate[:, :, None], 0.5).tolist() == [1, 0, 0]
    assert mel_lengths_of(gate[:, :, None]).tolist() == (gate < 0).to(torch.int64).argmax(-1).tolist()


def test_synthesize_manifest_decodes_and_cuts_by_the_models_threshold(tmp_path):
    """run/test.py's loop (shared by `test` and `test-correlation`) with a stand-in model and vocoder on the CPU: the decode gets the
    model's stop threshold, and the waveform is cut at the first frame below logit(threshold) - 3 frames under 0.3 for gates
    (0.4, -0.3, -0.5, masked ...), where the 0.5 rule cuts at 1."""
    import types
    import wave
    import pandas as pd
    from tacotron2_amd.run.test import synthesize_manifest
    from tests.test_gpu_cli import ALLOWED
    gate_row = torch.tensor([0.4, -0.3, -0.5, -1000.0, -1000.0, -1000.0])
    seen = []

    class Model:
        description_embeddings = speaker_tokens = controls = False
        attention_window, forward_attention = None, False
        tacotron2 = types.SimpleNamespace(store=types.SimpleNamespace(device=torch.device("cpu")))

        def __call__(self, chars_idx, chars_idx_len, **kw):
            seen.append(kw.get("stop_threshold"))
            B = chars_idx.shape[0]
            return None, torch.zeros(B, 6, 16), gate_row[None, :, None].expand(B, 6, 1), None

    gen = lambda mel: torch.zeros(1, 1, mel.shape[1] * 256)
    pre = {"allowed_chars": ALLOWED, "end_token": "^", "expand_abbreviations": True}
    df = pd.DataFrame({"text": ["Hi there.", "ok"], "wav": ["a.wav", "b.wav"], "speaker_id": [0, 0]})
    for tau, frames in ((0.3, 3), (0.5, 1), (None, 1)):
        m = Model()
        if tau is not None:
            m.stop_threshold = tau              # (a model without the attribute decodes and cuts at 0.5)
        out = tmp_path / f"res_{tau}"
        written = synthesize_manifest(m, df, pre, "unused", str(out), gen, None, 22050, None, batch_size=2, max_len=6)
        assert len(written) == 2 and seen[-1] == (tau or 0.5)
        for name in written:
            with wave.open(name, "rb") as w:
                assert w.getnframes() == frames * 256, (tau, w.getnframes())
