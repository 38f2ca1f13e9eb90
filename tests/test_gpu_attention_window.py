"""Windowed (monotonic) attention for autoregressive decoding on the GPU: Engine.infer(attention_window=(back, fwd)) against the
float64 windowed reference (tests/test_attention_window_host.py), the full-width window against the unconstrained decoder, the
window's support at vanilla dimensions, and the module / CLI surface."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import tacotron2_ref as R
from tests.helpers import SMALL, load_golden, params_from
from tests.test_attention_window_host import window_mask, windowed_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MID = dict(num_chars=39, encoded_dim=128, prenet_dim=64, att_rnn_dim=256, att_dim=64, rnn_hidden_dim=256, postnet_dim=128,
           num_mels=80, dropout=0.5, speaker_tokens=True, num_speakers=4)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _engine(d, P, dev):
    from tacotron2_amd.engine import Engine
    from tacotron2_amd.params import ParamStore
    ps = ParamStore(d, dev)
    ps.load_state_dict(P)
    return Engine(ps)


def _mid_params(seed=9):
    d = R.default_dims(**MID)
    P = R.init_params(d, seed=seed)
    P["decoder.gate.bias"] = P["decoder.gate.bias"] + 0.3      # stop logits cross zero at different frames
    P["decoder.gate.weight"] = P["decoder.gate.weight"] * 6.0
    return d, P


def _inputs(lens, L, N, seed, pdim=64):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    lens = torch.tensor(lens)
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    spk = torch.randint(0, 4, (B,), generator=g, dtype=torch.int32)
    pm = (torch.rand(N + 1, 2, B, pdim, generator=g) >= 0.5).float() * 2
    return ci, lens, spk, pm


def _check_vs_ref(out, ref, lens, window):
    mels, post, gates, al, lengths = out
    rm, rp, rg, ra, rl = ref
    assert mels.shape == rm.shape, (mels.shape, rm.shape)
    assert torch.equal(lengths.cpu(), rl)
    l1 = lambda a, b: float((a.double().cpu() - b.double()).abs().mean())
    assert l1(mels, rm) < 1e-4 and l1(post, rp) < 1e-4
    assert float((al.double().cpu() - ra.double()).abs().max()) < 5e-5
    assert torch.equal(gates.cpu() == -1000.0, rg == -1000.0)
    _check_support(al.cpu(), lens, window)


def _check_support(al, lens, window):
    """Alignments are exactly 0.0 outside each frame's window around the previous row's argmax (recomputed on the host)."""
    B, T, L = al.shape
    peak = torch.zeros(B, dtype=torch.int64)
    for t in range(T):
        outside = window_mask(peak, lens.cpu(), L, window)
        assert bool((al[:, t][outside] == 0.0).all()), f"frame {t}: weight outside the window"
        peak = al[:, t].argmax(1)


def _decode_and_ref(d, P, lens, L, N, window, seed, check_every=5):
    dev = _dev()
    ci, lens, spk, pm = _inputs(lens, L, N, seed, d["prenet_dim"])
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        ref = windowed_ref(P64, d, ci, lens, N, window, speaker_id=spk, prenet_drop=pm)
    eng = _engine(d, P, dev)
    out = eng.infer(ci.to(dev), lens.to(dev), N, speaker_id=spk.to(dev), prenet_masks=pm.to(dev).contiguous(),
                    check_every=check_every, attention_window=window)
    torch.cuda.synchronize()
    return out, ref, lens


@pytest.mark.parametrize("window", [(1, 3), (0, 1)])
def test_windowed_decode_matches_windowed_oracle(window):
    d, P = _mid_params()
    out, ref, lens = _decode_and_ref(d, P, [29, 21, 17, 25, 9, 13], 29, 24, window, seed=4)
    _check_vs_ref(out, ref, lens, window)


@pytest.mark.parametrize("L,B", [(300, 1), (300, 17), (1100, 1), (1100, 17)])
def test_windowed_decode_long_texts(L, B):
    """Texts above 256 positions: the unwindowed kernels walk them in rounds, the window reads only its own rows."""
    d, P = _mid_params()
    g = torch.Generator().manual_seed(L + B)
    lens = [L] + [int(x) for x in torch.randint(L // 2, L + 1, (B - 1,), generator=g)]
    out, ref, lens = _decode_and_ref(d, P, lens, L, 24, (2, 6), seed=L + 7 * B, check_every=8)
    _check_vs_ref(out, ref, lens, (2, 6))


def test_windowed_decode_two_groups():
    """B = 70: two decode groups of the one-loop stop rule, each with its own peaks."""
    d, P = _mid_params()
    g = torch.Generator().manual_seed(70)
    lens = [23] + [int(x) for x in torch.randint(5, 24, (69,), generator=g)]
    out, ref, lens = _decode_and_ref(d, P, lens, 23, 16, (1, 3), seed=71)
    _check_vs_ref(out, ref, lens, (1, 3))


def test_window_wider_than_every_text_is_the_unwindowed_decoder():
    d, P = _mid_params()
    dev = _dev()
    L, N = 29, 24
    ci, lens, spk, pm = _inputs([29, 21, 17, 25, 9, 13], L, N, seed=4)
    eng = _engine(d, P, dev)
    args = (ci.to(dev), lens.to(dev), N)
    kw = dict(speaker_id=spk.to(dev), prenet_masks=pm.to(dev).contiguous(), check_every=5)
    base = [x.clone() for x in eng.infer(*args, **kw)]
    wide = eng.infer(*args, attention_window=(L, L), **kw)
    torch.cuda.synchronize()
    assert torch.equal(base[4], wide[4])
    for a, b in zip(base[:4], wide[:4]):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-6


def test_windowed_decode_vanilla_dims_support():
    """Vanilla dimensions, B = 64, L = 188, window (1, 3), 200 frames (the stop bias raised so that nothing stops): finite outputs
    and every alignment row inside its window."""
    from bench import VANILLA
    from tacotron2_amd.engine import Engine
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    dev = _dev()
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, 0)
    with torch.no_grad():
        ps.P["decoder.gate.bias"].add_(10.0)
    eng = Engine(ps)
    g = torch.Generator().manual_seed(188)
    B, L = 64, 188
    lens = torch.randint(120, L + 1, (B,), generator=g)
    lens[0] = L
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 39, (int(lens[b]),), generator=g)
    spk = torch.randint(0, 4, (B,), generator=g)
    mels, post, gates, al, lengths = eng.infer(ci.to(dev), lens.to(dev), 200, speaker_id=spk.to(dev), seed=3,
                                               attention_window=(1, 3))
    torch.cuda.synchronize()
    assert al.shape == (B, 200, L)
    for x in (mels, post, gates, al):
        assert bool(torch.isfinite(x).all())
    _check_support(al.cpu(), lens, (1, 3))


def test_module_inference_with_window_and_cli_say(tmp_path):
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
        o = m.inference(t("chars_idx"), t("chars_len"), N, dropout_masks=dict(prenet_drop=pm), attention_window=(1, 3))
    eng = m._engine
    e = eng.infer(t("chars_idx"), t("chars_len"), N, prenet_masks=pm, attention_window=(1, 3))
    torch.cuda.synchronize()
    for a, b in zip(o, e[:4]):
        assert a.shape == b.shape and torch.equal(a, b)
    with pytest.raises(ValueError):
        m(t("chars_idx"), t("chars_len"), True, torch.zeros(1, 4, 16, device=dev), torch.tensor([4], device=dev),
          attention_window=(1, 3))
    # main.py say --attention-window 1,3 on the fixture's weights
    tts = TTSModel(lr=1e-3, weight_decay=0.0, dropout=0.5, device=dev, **SMALL)
    tts.tacotron2.load_state_dict(P)
    ck = tmp_path / "w.ckpt"
    torch.save(tts.checkpoint(), ck)
    allowed = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"
    args = {k: v for k, v in SMALL.items() if k not in ("num_chars", "num_mels")}
    cfg = {"dataset": {"preprocessing": {"allowed_chars": allowed, "end_token": "^", "num_mels": 16}},
           "training": {"lr": 1e-3, "weight_decay": 0.0, "name": "w", "args": {"max_steps": 1}},
           "model": {"args": dict(args, dropout=0.5)},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    cp = tmp_path / "cfg.json"
    cp.write_text(json.dumps(cfg))
    npy = tmp_path / "say.npy"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", str(cp), "--device", "0", "say",
                        "--checkpoint", str(ck), "--text", "Hello there.", "--out", str(npy), "--random-seed", "3",
                        "--attention-window", "1,3"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    mel = np.load(npy)
    assert mel.ndim == 2 and mel.shape[1] == 16 and np.isfinite(mel).all()
