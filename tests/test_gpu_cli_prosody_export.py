"""`main.py prosody-export` on the GPU, through its click entry in this process, on a corpus this test writes: two speakers with six
generator voices each (tests/voice_quality_ref.py: voice k of a speaker is higher and louder than voice k - 1, and more jittered and
noisier from one pair of voices to the next)
and one WAV of silence, split into train / val / test manifests, under a config whose controls name columns the command must write."""
import csv
import json
import wave

import numpy as np
import pandas as pd
import pytest
import torch

import voice_quality_ref as V

pytestmark = pytest.mark.gpu
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"
CONTROLS = ["pitch_mean_log_speaker_norm_clip", "pitch_range_log_speaker_norm_clip", "intensity_mean_vcd_speaker_norm_clip",
            "nhr_vcd_speaker_norm_clip", "rate_speaker_norm_clip"]
SUFFIXES = ("_speaker_norm", "_speaker_norm_clip", "_dataset_norm", "_dataset_norm_clip")
# voice k of a speaker: pitch and loudness rise with k, jitter and noise with the level k // 2.  (A jitter estimate from one second of
# voice scatters by some 20 %, so neighbouring voices share a level and the levels are a factor of two apart; the slow swell of the
# amplitude - `tremor` - is what keeps the smoothed track of these otherwise perfectly steady voices off the double period.)
JITTER, NOISE = [0.003, 0.006, 0.012], [0.004, 0.012, 0.03]
WORDS = ["a", "be", "sea", "deal", "early", "father"]


def _write(path, x, sr=22050):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.clip(np.rint(x * 32767), -32767, 32767).astype("<i2").tobytes())


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("prosody_export")
    speech = tmp / "wavs"
    speech.mkdir()
    rows = {"train": [], "val": [], "test": []}
    for spk, base in ((0, 100.0), (1, 180.0)):
        for k in range(6):
            x, _ = V.voice(base * (1 + 0.08 * k), 20000 + 700 * k + 300 * spk, jitter=JITTER[k // 2], shimmer=0.03,
                           noise=NOISE[k // 2], amp=0.02 * 1.4 ** k, seed=10 * spk + k, tremor=(10.0, 0.3))
            _write(speech / f"s{spk}_{k}.wav", x)
            rows["train" if k < 4 else ("val" if k == 4 else "test")].append(
                f"Voice {WORDS[k]}, number {k}.|s{spk}_{k}.wav|{spk}|{k}")
    _write(speech / "silence.wav", np.zeros(8000))
    rows["train"].insert(2, "Nothing at all.|silence.wav|0|9")
    for name, r in rows.items():
        (tmp / f"{name}.csv").write_text("\n".join(["text|wav|speaker_id|voice"] + r) + "\n")
    cfg = {"dataset": {"train": str(tmp / "train.csv"), "val": str(tmp / "val.csv"), "test": str(tmp / "test.csv"),
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "num_mels": 16}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "args": {"max_steps": 6}},
           "model": {"scheduler_milestones": [], "args": {}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": True, "features": CONTROLS}}}
    (tmp / "cfg.json").write_text(json.dumps(cfg))
    return dict(tmp=tmp, speech=speech, cfg=cfg)


def _export(s, res, cfgp=None, extra=()):
    from click.testing import CliRunner
    import main as cli
    return CliRunner().invoke(cli.main, ["--config", str(cfgp or s["tmp"] / "cfg.json"), "--device", "0", "prosody-export",
                                         "--speech-dir", str(s["speech"]), "--results-dir", str(res), "--batch-size", "5", *extra], obj={})


def _read(p):
    return pd.read_csv(p, delimiter="|", quoting=csv.QUOTE_NONE, engine="c")


def test_prosody_export_writes_manifests_statistics_and_dropped_rows(corpus):
    from tacotron2_amd.datasets.tts_dataset import TTSDataset
    from tacotron2_amd.prosody import FEATURES, MEASURES, ProsodyMeter
    s, res = corpus, corpus["tmp"] / "res"
    r = _export(s, res)
    print(r.output)
    assert r.exit_code == 0, (r.output, r.exception)
    assert sorted(p.name for p in res.iterdir()) == ["prosody_dropped.csv", "prosody_norm.json", "test.csv", "train.csv", "val.csv"]
    assert "utterances/s" in r.output and "13 utterances" in r.output and "1 dropped" in r.output
    # the silent WAV is dropped with its reason, everything else is kept in the manifest's order
    assert (res / "prosody_dropped.csv").read_text().splitlines() == ["manifest|wav|reason", "train.csv|silence.wav|no voiced frame"]
    dfs = {k: _read(res / f"{k}.csv") for k in ("train", "val", "test")}
    for k, df in dfs.items():
        src = _read(s["tmp"] / f"{k}.csv")
        src = src[src.wav != "silence.wav"].reset_index(drop=True)
        assert list(df.columns) == list(src.columns) + FEATURES + [f + x for x in SUFFIXES for f in FEATURES]
        assert (df[list(src.columns)].values == src.values).all()
        assert np.isfinite(df[FEATURES].values).all()
        clip = df[[c for c in df.columns if c.endswith("_clip")]].values
        assert clip.shape[1] == 36 and np.isfinite(clip).all() and (np.abs(clip) <= 1).all()
        assert (df.nhr_vcd == df.nhr).all() and np.allclose(df.pitch_range, df.pitch_95 - df.pitch_5)
    train = dfs["train"]
    assert len(train) == 8 and len(dfs["val"]) == 2 and len(dfs["test"]) == 2 and set(CONTROLS) <= set(train.columns)
    # the normalised columns are the formula on the raw columns of the same file, with the statistics of the train rows
    for k, df in dfs.items():
        for f in FEATURES:
            z, zc = V.normalise(df[f], train[f])
            assert np.allclose(df[f + "_dataset_norm"], z, rtol=1e-9, atol=1e-12), (k, f)
            assert np.allclose(df[f + "_dataset_norm_clip"], zc, rtol=1e-9, atol=1e-12), (k, f)
            for spk in (0, 1):
                m = (df.speaker_id == spk).values
                z, zc = V.normalise(df[f][m], train[f][(train.speaker_id == spk).values])
                assert np.allclose(df[f + "_speaker_norm"][m], z, rtol=1e-9, atol=1e-12), (k, f, spk)
                assert np.allclose(df[f + "_speaker_norm_clip"][m], zc, rtol=1e-9, atol=1e-12), (k, f, spk)
    # prosody_norm.json: the meter (smoothed by default), the statistics and the counts
    norm = json.loads((res / "prosody_norm.json").read_text())
    assert norm["meter"] == ProsodyMeter(22050, "cuda:0", smooth=True).describe() and norm["meter"]["smooth"] is True
    assert norm["features"] == FEATURES and norm["speaker_column"] == "speaker_id" and set(norm["speakers"]) == {"0", "1"}
    assert norm["counts"]["train"] == dict(manifest="train.csv", rows=9, written=8, dropped=1) and norm["counts"]["val"]["written"] == 2
    assert norm["dataset"]["n"] == 8 and norm["speakers"]["1"]["n"] == 4
    assert norm["dataset"]["median"]["pitch_mean_log"] == pytest.approx(np.median(train.pitch_mean_log), rel=1e-9)
    assert norm["speakers"]["0"]["std"]["nhr"] == pytest.approx(np.std(train.nhr[train.speaker_id == 0], ddof=1), rel=1e-9)
    # within a speaker the measures follow the generator's settings
    every = pd.concat(dfs.values(), ignore_index=True)
    for spk, base in ((0, 100.0), (1, 180.0)):
        g = every[every.speaker_id == spk].sort_values("voice")
        assert list(g.voice) == list(range(6))
        print(g[["voice", "pitch_mean", "pitch_mean_log", "intensity_mean", "jitter", "shimmer", "nhr", "rate"]])
        for f in ("pitch_mean_log", "intensity_mean"):
            assert (np.diff(g[f].values) > 0).all(), (spk, f, g[f].values)
        for f in ("jitter", "nhr"):                           # every voice of a level above every voice of the level below
            v = g[f].values.reshape(3, 2)
            assert v[0].max() < v[1].min() and v[1].max() < v[2].min(), (spk, f, v)
        assert np.allclose(np.exp(g.pitch_mean_log.values), base * (1 + 0.08 * np.arange(6)), rtol=0.02)
        assert np.allclose(np.diff(g.intensity_mean.values), 20 * np.log10(1.4), atol=0.5)          # 2.9 dB per voice
    # measure() on the same signals: its own fields, and the numbers the manifest carries under the reference's names
    ds = TTSDataset(filenames=list(train.wav), texts=list(train.text), base_dir=str(s["speech"]), device="cuda:0",
                    **s["cfg"]["dataset"]["preprocessing"])
    wavs = [torch.from_numpy(ds.load_audio(i)).to("cuda:0") for i in range(len(ds))]
    chars = [len(i) for i in ds.ids]
    got = ProsodyMeter(22050, "cuda:0", smooth=True).measure(wavs, chars)
    for i, m in enumerate(got):
        assert list(m) == ["n_frames", "n_voiced"] + MEASURES
        assert m["pitch_mean_log"] == pytest.approx(train.pitch_mean_log[i], rel=1e-12)
        assert m["pitch_range_log"] == pytest.approx(train.pitch_range_log[i], rel=1e-12, abs=1e-15)
        assert m["intensity_mean_db"] == pytest.approx(train.intensity_mean_vcd[i], rel=1e-12)
        assert m["rate"] == pytest.approx(train.rate[i], rel=1e-12) and m["rate"] == pytest.approx(chars[i] / train.duration[i], rel=1e-12)
        assert train.duration_vcd[i] == pytest.approx(m["n_voiced"] * 256 / 22050, rel=1e-12)


def test_prosody_export_names_missing_control_columns_and_unsmoothed_meter(corpus):
    s, res = corpus, corpus["tmp"] / "res_missing"
    cfg = json.loads(json.dumps(s["cfg"]))
    cfg["extensions"]["controls"]["features"] = CONTROLS + ["pitch_mean_gender_norm", "energy"]
    cfgp = s["tmp"] / "cfg_missing.json"
    cfgp.write_text(json.dumps(cfg))
    r = _export(s, res, cfgp, ["--no-smooth-pitch"])
    assert r.exit_code == 1 and "pitch_mean_gender_norm, energy" in r.output and "rate_speaker_norm_clip" not in r.output
    assert (res / "train.csv").exists()                       # the check runs after writing
    assert "smooth" not in json.loads((res / "prosody_norm.json").read_text())["meter"]
