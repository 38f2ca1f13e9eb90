"""Corpora at another rate than the model's through the training loader, and `say --out-sample-rate`.

One manifest of six analytic multi-tone signals (all partials below 7.7 kHz, inside the passband) is written twice: sampled at
22050 Hz, and sampled at 24000 Hz with n_in a multiple of 160 - the same instants of time, so the 24 kHz copy of utterance i resamples
to exactly the sample count of its 22.05 kHz copy (147 per 160)."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"
BLOCKS = [61, 100, 83, 127, 74, 96]                 # utterance i lasts BLOCKS[i] / 150 s: 160 samples at 24 kHz, 147 at 22.05 kHz each
TEXTS = ["one.", "two, a longer one.", "three", "the fourth and longest of the six.", "five?", "six, six, six"]


def _signal(i, sr, n):
    rng = np.random.default_rng(100 + i)
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in zip(rng.uniform(0.02, 0.12, 6), rng.uniform(80, 7700, 6), rng.uniform(0, 6, 6)))
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("rates")
    for sr, per in ((22050, 147), (24000, 160)):
        os.makedirs(root / str(sr))
        for i, k in enumerate(BLOCKS):
            with wave.open(str(root / str(sr) / f"u{i}.wav"), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
                w.writeframes(np.round(_signal(i, sr, k * per) * 32767).astype("<i2").tobytes())
    # a mixed corpus: the even utterances at 24 kHz, the odd ones at 22.05 kHz
    os.makedirs(root / "mixed")
    for i in range(len(BLOCKS)):
        os.symlink(root / ("24000" if i % 2 == 0 else "22050") / f"u{i}.wav", root / "mixed" / f"u{i}.wav")
    return root


def _dataset(corpus, which, **kw):
    from tacotron2_amd.datasets.tts_dataset import TTSDataset
    return TTSDataset(filenames=[f"u{i}.wav" for i in range(len(BLOCKS))], texts=TEXTS, base_dir=str(corpus / which), silence=512,
                      trim=False, device="cuda:0", **kw)


def _batches(ds, bs=3):
    from tacotron2_amd.datasets.tts_dataset import DeviceBatchLoader
    dev = torch.device("cuda:0")
    return [hb.to_device(dev) for hb in DeviceBatchLoader(ds, batch_size=bs, shuffle=False, drop_last=False, decode_threads=3)]


def test_a_24_khz_corpus_has_the_frames_of_its_22_khz_copy(corpus):
    """The test that fails without the feature: read as 22.05 kHz audio, a 24 kHz file has 160 / 147 of the samples and frames."""
    lo, hi = _batches(_dataset(corpus, "22050")), _batches(_dataset(corpus, "24000"))
    for a, b in zip(lo, hi):
        assert torch.equal(a["mel_spectrogram_len"], b["mel_spectrogram_len"])
        assert a["mel_spectrogram"].shape == b["mel_spectrogram"].shape and torch.equal(a["gate"], b["gate"])
    want = [1 + (147 * k + 512) // 256 for k in BLOCKS]
    assert torch.cat([b["mel_spectrogram_len"] for b in hi]).tolist() == want


def test_loader_mel_is_the_hand_made_one_and_the_item_path(corpus):
    from tacotron2_amd.datasets.resample import Resampler
    from tacotron2_amd.datasets.tts_dataset import collate, load_wav
    dev = torch.device("cuda:0")
    ds = _dataset(corpus, "24000")
    got = _batches(ds)[1]                                            # utterances 3, 4, 5
    idxs = [3, 4, 5]
    wavs = [load_wav(str(corpus / "24000" / f"u{i}.wav")) for i in idxs]
    assert all(sr == 24000 for _, sr in wavs)
    n_in = [len(w) for w, _ in wavs]
    x = torch.zeros(3, max(n_in) + 5)
    for r, (w, _) in enumerate(wavs):
        x[r, :n_in[r]] = torch.from_numpy(w)
    n = [147 * BLOCKS[i] + 512 for i in idxs]
    out, n_out = Resampler(22050, dev).batch(x.to(dev), n_in, 24000, ldy=max(n) + 13)
    assert n_out == [147 * BLOCKS[i] for i in idxs]
    mel, gate, mel_len = ds.melspectrogram.batch(out, torch.tensor(n, dtype=torch.int64, device=dev), max(n))
    assert torch.equal(got["mel_spectrogram"], mel) and torch.equal(got["gate"], gate) and torch.equal(got["mel_spectrogram_len"], mel_len)
    data, meta, _ = collate([_dataset(corpus, "24000")[i] for i in idxs])          # the item path: load_audio resamples one file
    assert torch.equal(got["mel_spectrogram"], data["mel_spectrogram"]) and torch.equal(got["gate"], data["gate"])
    assert torch.equal(got["mel_spectrogram_len"].cpu(), meta["mel_spectrogram_len"])
    one = ds.load_audio(4)
    assert one.dtype == np.float32 and len(one) == 147 * BLOCKS[4] + 512 and float(np.abs(one[-512:]).sum()) == 0.0
    assert np.array_equal(one[:-512], out[1, :n_out[1]].cpu().numpy())
    # the resampled 24 kHz copy IS the 22.05 kHz copy, up to the filter (-80 dB in the passband) and the 16-bit steps of both files
    lo = _dataset(corpus, "22050").load_audio(4)
    edge = 200
    assert np.abs(one[:-512] - lo[:-512])[edge:-edge].max() < 1e-4 * 6 * 0.12 + 2 * 2.0 ** -15


def test_a_mixed_rate_batch_gives_what_the_single_rate_batches_give(corpus):
    lo, hi = _batches(_dataset(corpus, "22050"), bs=6)[0], _batches(_dataset(corpus, "24000"), bs=6)[0]
    mixed = _batches(_dataset(corpus, "mixed"), bs=6)[0]
    assert torch.equal(mixed["mel_spectrogram_len"], hi["mel_spectrogram_len"]) and torch.equal(mixed["gate"], hi["gate"])
    for b in range(6):
        src = hi if b % 2 == 0 else lo
        assert torch.equal(mixed["mel_spectrogram"][b], src["mel_spectrogram"][b]), b
    assert not torch.equal(lo["mel_spectrogram"], hi["mel_spectrogram"])             # (the two copies do differ in their last bits)


# ---- say --out-sample-rate --------------------------------------------------------------------------------------------------------
def _say_setup(tmp_path):
    from helpers import load_golden, params_from
    z = load_golden("infer")
    sd = {"tacotron2." + k: v for k, v in params_from(z).items()}
    hp = dict(lr=1e-3, weight_decay=1e-6, num_chars=39, encoded_dim=32, num_mels=16, prenet_dim=16, att_rnn_dim=32, att_dim=16,
              rnn_hidden_dim=32, postnet_dim=32, dropout=0.5)
    ck = tmp_path / "m.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hp, "global_step": 0, "epoch": 0}, ck)
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv", "test": "none.csv",
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "num_mels": 16}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "args": {"max_steps": 6}},
           "model": {"scheduler_milestones": [], "args": {"prenet_dim": 16, "att_rnn_dim": 32, "att_dim": 16, "rnn_hidden_dim": 32,
                                                          "postnet_dim": 32, "dropout": 0.5, "char_embedding_dim": 32}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps(cfg))
    return cfg, cfgp, ck


def _read(path):
    with wave.open(str(path), "rb") as w:
        return w.getframerate(), w.getnframes(), np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifi_gan"])
def test_say_out_sample_rate_writes_the_resampled_waveform(tmp_path, monkeypatch, vocoder):
    from helpers import write_hifigan_checkpoint
    from tacotron2_amd import vocoder as V
    from tacotron2_amd.datasets.resample import Resampler
    from tacotron2_amd.run.say import do_say
    cfg, cfgp, ck = _say_setup(tmp_path)
    written = []
    real_write = V.write_wav
    monkeypatch.setattr(V, "write_wav", lambda path, y, sr: (written.append((path, y.detach().float().cpu().clone(), sr)), real_write(path, y, sr))[1])
    kw = dict(dataset_config=cfg["dataset"], training_config=cfg["training"], model_config=cfg["model"], extensions_config=cfg["extensions"],
              device=0, checkpoint=str(ck), text="Testing: one; two? three.", random_seed=3, max_len=40)
    if vocoder == "hifi_gan":
        kw["hifi_gan_checkpoint"] = write_hifigan_checkpoint(str(tmp_path / "hifi"), n_mels=16)
    dur = tmp_path / "dur.json"
    mels_a = do_say(output=str(tmp_path / "a.wav"), durations_out=str(dur), **kw)
    dur_a = json.loads(dur.read_text())
    mels_b = do_say(output=str(tmp_path / "b.wav"), durations_out=str(dur), out_sample_rate=16000, **kw)
    assert np.array_equal(mels_a[0], mels_b[0]) and json.loads(dur.read_text()) == dur_a        # times stay in model frames
    (_, y, sr_a), (_, y16, sr_b) = written
    assert (sr_a, sr_b) == (22050, 16000) and len(y) > 0
    # without the option: exactly what write_wav makes of the vocoder's waveform at the model's rate
    real_write(str(tmp_path / "plain.wav"), y, 22050)
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "plain.wav").read_bytes()
    # with it: Resampler.one of that waveform, the header at 16000, ceil(n * 320 / 441) frames
    want = Resampler(16000, "cuda:0").one(y.numpy(), 22050)
    assert np.array_equal(y16.numpy(), want)
    real_write(str(tmp_path / "want.wav"), torch.from_numpy(want), 16000)
    rate, frames, pcm = _read(tmp_path / "b.wav")
    assert rate == 16000 and frames == -(-len(y) * 320 // 441) == len(want)
    assert np.array_equal(pcm, _read(tmp_path / "want.wav")[2])
    peak = max(1.0, float(np.abs(want).max()))
    assert np.array_equal(pcm, np.clip(np.round(want / peak * 32767.0), -32768, 32767).astype("<i2"))
    if vocoder == "griffin_lim":
        with pytest.raises(ValueError, match="out-sample-rate"):          # a log-mel target has no rate
            do_say(output=str(tmp_path / "c.npy"), out_sample_rate=16000, **kw)


def test_cli_say_out_sample_rate(tmp_path):
    cfg, cfgp, ck = _say_setup(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", str(cfgp), "--device", "0", "say", "--checkpoint", str(ck),
                        "--text", "Hi there.", "--out", str(tmp_path / "o.wav"), "--random-seed", "3", "--out-sample-rate", "8000"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rate, frames, pcm = _read(tmp_path / "o.wav")
    assert rate == 8000 and frames > 0 and len(pcm) == frames
