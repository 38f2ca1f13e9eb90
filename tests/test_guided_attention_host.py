"""Guided-attention loss, host side: the float64 restatement of the formula (used by tests/test_gpu_guided_attention.py) against a
hand-computed example, the C ABI's new entry and grown operand block, and the `--guided-attention` option / config section."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
from click.testing import CliRunner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def guided_ref(align, chars_len, mel_len, sigma, alpha, grad_scale=1.0):
    """Float64 restatement of t2_guided_attn (include/tacotron2_amd.h), written from the published formula:
        G[b][t][l] = 1 - exp(-(l/N_b - t/T_b)^2 / (2 sigma^2))   for t < T_b and l < N_b, else 0
        loss       = alpha / B * sum_b (sum_{t,l} G * align) / (N_b * T_b)
        dalign     = grad_scale * alpha / (B * N_b * T_b) * G
    N_b / T_b are the lengths clipped to the padded (L, T); an utterance with N_b * T_b == 0 contributes nothing.
    align may require grad (the loss is then differentiable).  Returns (loss, dalign, scale) with scale[b] the size of utterance b's
    gradient, alpha * grad_scale / (B * N_b * T_b) (0 for an empty utterance)."""
    B, T, L = align.shape
    N = chars_len.to(torch.int64).clamp(0, L)
    Tb = mel_len.to(torch.int64).clamp(0, T)
    l = torch.arange(L, dtype=torch.float64)[None, None, :]
    t = torch.arange(T, dtype=torch.float64)[None, :, None]
    Nf, Tf = N.double()[:, None, None], Tb.double()[:, None, None]
    live = (l < Nf) & (t < Tf)
    x = l / Nf.clamp(min=1) - t / Tf.clamp(min=1)
    G = torch.where(live, 1.0 - torch.exp(-x * x / (2.0 * float(sigma) ** 2)), torch.zeros((), dtype=torch.float64))
    cnt = (N * Tb).double()
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1), torch.zeros_like(cnt))
    loss = float(alpha) / B * ((G * align.double()).sum((1, 2)) * inv).sum()
    scale = float(alpha) * float(grad_scale) / B * inv
    return loss, scale[:, None, None] * G, scale


def test_restatement_matches_a_hand_computed_example():
    """One utterance, T = 2 frames, N = 3 characters, sigma = 0.4 (2 sigma^2 = 0.32), alpha = 2: the six mask values written out."""
    e = math.exp
    G = [[0.0, 1 - e(-((1 / 3) ** 2) / 0.32), 1 - e(-((2 / 3) ** 2) / 0.32)],
         [1 - e(-((0 - 1 / 2) ** 2) / 0.32), 1 - e(-((1 / 3 - 1 / 2) ** 2) / 0.32), 1 - e(-((2 / 3 - 1 / 2) ** 2) / 0.32)]]
    assert abs(G[0][1] - 0.293352) < 1e-6 and abs(G[0][2] - 0.750648) < 1e-6 and abs(G[1][0] - 0.542167) < 1e-6
    assert abs(G[1][1] - 0.083145) < 1e-6 and abs(G[1][1] - G[1][2]) < 1e-12     # (exp(-x) to six digits, by calculator)
    w = torch.tensor([[[0.7, 0.2, 0.1], [0.1, 0.3, 0.6]]], dtype=torch.float64)
    want = 2.0 * sum(G[t][l] * float(w[0, t, l]) for t in range(2) for l in range(3)) / 6
    loss, da, scale = guided_ref(w, torch.tensor([3]), torch.tensor([2]), 0.4, 2.0, grad_scale=0.5)
    assert abs(float(loss) - want) < 1e-14
    assert float(scale[0]) == pytest.approx(2.0 * 0.5 / 6)
    assert torch.allclose(da[0], torch.tensor(G, dtype=torch.float64) * (2.0 * 0.5 / 6), rtol=0, atol=1e-15)


def test_restatement_masks_pads_and_takes_the_mean_per_utterance():
    g = torch.Generator().manual_seed(0)
    w = torch.rand(3, 5, 4, generator=g, dtype=torch.float64)
    cl, ml = torch.tensor([4, 2, 0]), torch.tensor([5, 3, 4])
    loss, da, scale = guided_ref(w, cl, ml, 0.4, 1.0)
    assert float(da[1, 3:].abs().max()) == 0.0 and float(da[1, :, 2:].abs().max()) == 0.0 and float(da[2].abs().max()) == 0.0
    assert float(scale[2]) == 0.0 and float(da[0, 4, 0]) > 0
    # per utterance, then over the batch: a batch is the mean of its single utterances (three "shards" of one)
    singles = [guided_ref(w[b:b + 1], cl[b:b + 1], ml[b:b + 1], 0.4, 1.0)[0] for b in range(3)]
    assert abs(float(loss) - float(sum(singles)) / 3) < 1e-15
    # autograd of the restated loss is the restated gradient
    wr = w.clone().requires_grad_(True)
    guided_ref(wr, cl, ml, 0.4, 1.0)[0].backward()
    assert torch.allclose(wr.grad, da, rtol=0, atol=1e-16)
    # lengths beyond the padded shape are clipped to it
    l2 = guided_ref(w, torch.tensor([9, 2, 0]), torch.tensor([7, 3, 4]), 0.4, 1.0)[0]
    assert float(l2) == float(loss)


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: the entry is declared and exported, the attention backward's operand block grew by one pointer
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_guided_attention_entry_and_the_dalign_operand():
    from tacotron2_amd import _lib, build
    assert "t2_guided_attn" in _lib.DECLARED_SYMBOLS
    ret, args = _lib._funcs["t2_guided_attn"]
    assert ret == "int" and [a[0] for a in args] == ["float", "int32_t", "int32_t", "int", "int", "int", "float", "float", "double",
                                                     "float", "float", "void"]
    assert [a[1] for a in args] == [True, True, True, False, False, False, False, False, True, True, False, True]
    fields = [f[0] for f in _lib._structs["T2AttnSeqBwd"]]
    assert fields[-1] == "dalign" and fields[-2] == "ws_bd"              # appended: every earlier field keeps its offset
    build.build(verbose=False)
    lib = _lib.lib()
    assert hasattr(lib, "t2_guided_attn")
    assert lib.t2_sizeof(b"T2AttnSeqBwd") == C.sizeof(_lib.S["T2AttnSeqBwd"])
    assert _lib.S["T2AttnSeqBwd"].dalign.offset == C.sizeof(_lib.S["T2AttnSeqBwd"]) - 8
    # bad arguments are refused before a launch (no GPU needed): null operands, sigma <= 0, alpha < 0
    assert lib.t2_guided_attn(None, None, None, 1, 1, 1, 0.4, 1.0, None, None, 1.0, None) == 1
    assert b"t2_guided_attn" in lib.t2_last_error()
    x = (C.c_double * 4)()
    p = C.addressof(x)
    assert lib.t2_guided_attn(p, p, p, 1, 1, 1, 0.0, 1.0, p, None, 1.0, None) == 1 and b"sigma" in lib.t2_last_error()
    assert lib.t2_guided_attn(p, p, p, 1, 1, 1, 0.4, -1.0, p, None, 1.0, None) == 1
    assert lib.t2_guided_attn(p, p, p, 0, 1, 1, 0.4, 1.0, p, None, 1.0, None) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks, config section, CLI option (do_train is replaced: no GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def test_guided_attention_argument_checks():
    from tacotron2_amd.engine import check_guided_attention
    assert check_guided_attention(None) is None
    assert check_guided_attention((0.4, 1.0)) == (0.4, 1.0) and check_guided_attention([1, 0]) == (1.0, 0.0)
    for bad in [(0.0, 1.0), (-0.4, 1.0), (0.4, -1e-9), (0.4,), (0.4, 1.0, 2.0), ("0.4", "1"), (True, 1.0), 0.4,
                (float("nan"), 1.0), (0.4, float("inf"))]:
        with pytest.raises(ValueError):
            check_guided_attention(bad)


def test_config_section_and_option_precedence():
    from tacotron2_amd.run.common import guided_attention_setting as setting
    assert setting({}) is None and setting({"guided_attention": None}) is None
    assert setting({"guided_attention": {"sigma": 0.2, "alpha": 5}}) == (0.2, 5.0)
    assert setting({"guided_attention": {}}) == (0.4, 1.0) and setting({"guided_attention": {"alpha": 3.0}}) == (0.4, 3.0)
    assert setting({"guided_attention": {"sigma": 0.2, "alpha": 5}}, (0.4, 1.0)) == (0.4, 1.0)          # the option wins
    assert setting({}, (0.3, 2.0)) == (0.3, 2.0)
    for bad in [{"sigma": 0.0}, {"sigma": -1, "alpha": 1}, {"alpha": -1}, [0.4, 1.0], {"sigma": 0.4, "weight": 1.0}, "0.4,1.0", True]:
        with pytest.raises(ValueError):
            setting({"guided_attention": bad})
    with pytest.raises(ValueError):
        setting({}, (0.0, 1.0))


def _cli(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    import tacotron2_amd.run.train as train
    seen = {}
    monkeypatch.setattr(train, "do_train", lambda **kw: seen.update(kw))
    cfg = tmp_path / "cfg.json"
    cfg.write_text('{"dataset": {"preprocessing": {"allowed_chars": "ab"}}, "training": {}, "model": {}, "extensions": {}}')
    return cli, seen, ["--config", str(cfg), "train", "--speech-dir", "s"]


def test_cli_guided_attention_reaches_the_driver(monkeypatch, tmp_path):
    cli, seen, pre = _cli(monkeypatch, tmp_path)
    r = CliRunner().invoke(cli.main, pre + ["--guided-attention", "0.4,1.0"], obj={})
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert seen["guided_attention"] == (0.4, 1.0)
    seen.clear()
    r = CliRunner().invoke(cli.main, pre + ["--guided-attention", " 0.25 , 100 "], obj={})
    assert r.exit_code == 0 and seen["guided_attention"] == (0.25, 100.0)
    seen.clear()
    r = CliRunner().invoke(cli.main, pre, obj={})                         # default: off
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert seen["guided_attention"] is None


@pytest.mark.parametrize("bad", ["0,1", "-0.4,1", "0.4,-1", "0.4", "a,b", "0.4,1,2", "", "nan,1", "0.4;1"])
def test_cli_guided_attention_malformed_is_a_usage_error(monkeypatch, tmp_path, bad):
    cli, seen, pre = _cli(monkeypatch, tmp_path)
    r = CliRunner().invoke(cli.main, pre + ["--guided-attention", bad], obj={})
    assert r.exit_code == 2 and "guided-attention" in r.output and "SIGMA,ALPHA" in r.output, r.output
    assert not seen


def test_ttsmodel_and_trainer_carry_the_setting_outside_the_hyper_parameters():
    """`guided_attention` is an attribute set by the driver: not a constructor argument, not in hparams / the checkpoint."""
    import inspect
    from tacotron2_amd.model import TTSModel
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.trainer import Trainer
    from tests.helpers import SMALL
    assert "guided_attention" not in inspect.signature(TTSModel.__init__).parameters
    tm = TTSModel(lr=1e-3, weight_decay=1e-6, dropout=0.5, device="cpu", **SMALL)
    assert tm.guided_attention is None and "guided_attention" not in tm.hparams
    tm.guided_attention = (0.4, 1.0)
    ck = tm.checkpoint()
    assert "guided_attention" not in ck["hyper_parameters"] and not any("guided" in k for k in ck["state_dict"])
    ps = ParamStore(tm.tacotron2.dims, "cpu")
    tr = Trainer(ps, lr=1e-3, weight_decay=1e-6, guided_attention=[0.3, 2])
    assert tr.guided_attention == (0.3, 2.0) and tr.last_guided_loss is None
    assert Trainer(ps, lr=1e-3, weight_decay=1e-6).guided_attention is None
    with pytest.raises(ValueError):
        Trainer(ps, lr=1e-3, weight_decay=1e-6, guided_attention=(0.0, 1.0))
