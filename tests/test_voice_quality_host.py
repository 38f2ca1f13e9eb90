"""Host checks of the voice-quality measurement and of `main.py prosody-export` (no GPU): the float64 restatement of the cycle-matching
rule (tests/voice_quality_ref.py) recovers what its synthetic voice was given, the rule's edges, the normalisation against a numpy
restatement of its formula, the dropped-row bookkeeping and the command's usage errors.

Bounds of the sanity checks: this is no parity with Praat.  On the generator the rule reads 0.0098 for a true jitter of 0.0112 and
0.0206 for 0.0224 (ratio 0.88 - 0.92: the parabola smooths), 0.0524 for a true shimmer of 0.0649 and 0.0314 for 0.0390 (ratio 0.80: a
cycle's RMS also holds the tail of the pulse before it), nhr 0.103 at a noise ratio of 0.10, and 0.013 of spurious shimmer at 1 % of
jitter alone.  The bounds below are those ratios with a margin of about 0.2 either way."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import voice_quality_ref as V


def _measured(f, seed=3, **kw):
    x, true = V.voice(f, 16000, seed=seed, **kw)
    return true, V.measure_voice(x, f)


def test_the_reference_recovers_jitter_shimmer_and_noise():
    prev = 0.0
    for j in (0.01, 0.02):
        true, m = _measured(120.0, jitter=j)
        assert m["n"] > 50 and 0.7 <= m["jitter"] / true["jitter"] <= 1.15, (true, m)
        assert m["jitter"] > prev
        prev = m["jitter"]
    for s in (0.05, 0.03):
        true, m = _measured(120.0, shimmer=s)
        assert 0.6 <= m["shimmer"] / true["shimmer"] <= 1.1 and m["jitter"] < 0.001, (true, m)
    true, m = _measured(120.0, jitter=0.005, shimmer=0.03, noise=0.10)
    assert 0.08 <= m["nhr"] <= 0.13 and abs(m["hnr_db"] - 10.0) < 1.0, m
    true, m = _measured(120.0, jitter=0.01)
    assert m["shimmer"] < 0.02, m                             # spurious shimmer of jitter alone
    true, m = _measured(120.0)
    assert m["jitter"] < 0.001 and m["shimmer"] < 0.005 and m["nhr"] < 0.005 and m["hnr_db"] > 23, m
    for f in (90.0, 210.0):                                   # the other two pitches of the GPU test: the same picture
        true, m = _measured(f, jitter=0.01, shimmer=0.03, noise=0.02)
        assert 0.7 <= m["jitter"] / true["jitter"] <= 1.15 and 0.6 <= m["shimmer"] / true["shimmer"] <= 1.3, (f, true, m)
        assert 0.02 <= m["nhr"] <= 0.06, (f, m)


def test_the_setup_of_a_frame_and_its_edges():
    assert V.setup(np.float32(8000 / 37.3), 180, 8000, 10, 100) == (37, 5, 3)              # the measured edge of the tiny configuration
    assert V.setup(np.float32(8000 / 45.0), 180, 8000, 10, 100) == (45, 6, 2)
    assert V.setup(np.float32(8000 / 12.0), 180, 8000, 10, 100) == (12, 2, 13)
    assert V.setup(np.float32(61.0), 1391, 22050, 44, 367) == (361, 46, 2)
    assert V.setup(np.float32(120.0), 1391, 22050, 44, 367) == (184, 23, 6)
    assert V.setup(np.float32(1e-30), 1391, 22050, 44, 367)[0] == 366 and V.setup(np.float32(1e30), 1391, 22050, 44, 367)[0] == 44
    assert V.setup(np.float32(22050 / 44.5), 1391, 22050, 44, 367)[0] == 44                # half to even, as lrintf
    assert V.setup(np.float32(500.0), 4096, 22050, 44, 367)[2] == V.MAX_CYCLES == 32
    # K (2 d + 1) fits the kernel's tables of S / 2 + 160 floats for every lag and span
    for S in (20, 180, 1391, 4096):
        for L in range(2, min(S, 4095)):
            d = max(2, (L + 7) // 8)
            room = S - 2 * L - d
            K = 0 if room < 0 else min(room // L + 1, 32)
            assert K * (2 * d + 1) <= S // 2 + 160, (S, L)


def test_the_rule_on_exact_signals():
    L = 50
    period = np.random.default_rng(0).normal(size=L)
    x = np.tile(period, 12)[:580]
    fr = V.frame(x, np.float32(8000 / L), 8000, 10, 100)
    assert fr["K"] == (580 - 100 - 7) // 50 + 1 and (fr["k"] == fr["d"]).all()           # tau* = L in every cycle
    assert np.allclose(fr["T"], L, atol=1e-9) and np.allclose(fr["r"], 1.0) and fr["jitter"] < 1e-10 and fr["shimmer"] < 1e-12
    assert abs(fr["nhr"] - 1e-6 / (1 - 1e-6)) < 1e-12 and abs(fr["hnr_db"] - 60.0) < 1e-3   # r clamped to 1 - 1e-6
    z = V.frame(np.zeros(580), np.float32(8000 / L), 8000, 10, 100)                        # silence: ncc = 0 everywhere, first argmax
    assert (z["k"] == 0).all() and (z["T"] == L - z["d"]).all() and (z["r"] == 0).all() and (z["A"] == 0).all()
    assert z["jitter"] == 0 and z["shimmer"] == 0 and abs(z["nhr"] - 999.0) < 1e-9 and abs(z["hnr_db"] + 10 * np.log10(999.0)) < 1e-9
    assert V.frame(x, np.float32(0.0), 8000, 10, 100) is None and V.frame(x, np.float32(np.nan), 8000, 10, 100) is None
    assert V.frame(x[:180], np.float32(8000 / L), 8000, 10, 100) is None                   # K = 1
    # amplitude steps of 10 % per cycle, same period: shimmer = mean |dA| / mean A, no jitter
    y = np.concatenate([period * (1.1 ** i) for i in range(12)])[:580]
    fy = V.frame(y, np.float32(8000 / L), 8000, 10, 100)
    A = np.sqrt(np.mean(period ** 2)) * 1.1 ** np.arange(fy["K"])
    assert np.allclose(fy["A"], A) and abs(fy["shimmer"] - np.mean(np.abs(np.diff(A))) / np.mean(A)) < 1e-12 and fy["jitter"] < 1e-9


def test_corpus_stats_reference():
    f0 = np.array([100.0, 0.0, 200.0, 300.0, np.nan], np.float32)
    power = np.array([1e-2, 1e-3, 1e-12, 1e-4, np.nan], np.float32)
    vq = dict(jitter=np.array([0.01, 0, 0.03, 0, np.nan]), shimmer=np.array([0.1, 0, 0.3, 0, np.nan]),
              nhr=np.array([0.2, 0, 0.4, 0, np.nan]), hnr_db=np.array([7.0, 0, 4.0, 0, np.nan]), cycles=np.array([5, 0, 3, 0, 9]))
    row = V.corpus_stats(f0, power, vq, [True, True, True, True, False])
    assert row[:5] == [4.0, 3.0, 2.0, 3.0, 200.0] and np.allclose(row[5:9], [0.02, 0.2, 0.3, 5.5]) and abs(row[9] + 30.0) < 1e-5
    assert V.corpus_stats(f0, power, vq, [False] * 5) == [0.0] * 12


def test_the_abi_knows_the_two_structs():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    for st in ("T2VoiceQuality", "T2CorpusStats"):
        assert lib.t2_sizeof(st.encode()) == C.sizeof(_lib.S[st]) > 0
    assert {"t2_voice_quality", "t2_corpus_stats"} <= set(_lib.DECLARED_SYMBOLS)
    assert lib.t2_voice_quality(None, None) == 1 and b"t2_voice_quality" in lib.t2_last_error()
    assert lib.t2_corpus_stats(None, None) == 1 and b"t2_corpus_stats" in lib.t2_last_error()


# --------------------------------------------------------------------------------------------------------------------------------
# prosody-export: normalisation, bookkeeping, usage
# --------------------------------------------------------------------------------------------------------------------------------
def _frame(rng, speakers, n_each, shift=0.0):
    import pandas as pd
    from tacotron2_amd.prosody import FEATURES
    rows = []
    for spk in speakers:
        for i in range(n_each):
            r = dict(text=f"t {spk} {i}", wav=f"{spk}_{i}.wav", speaker_id=spk)
            r.update({f: float(rng.normal(loc=10.0 * (spk + 1) + shift, scale=1.0 + j)) for j, f in enumerate(FEATURES)})
            rows.append(r)
    return pd.DataFrame(rows)


def test_normalisation_against_the_formula():
    from tacotron2_amd.prosody import FEATURES
    from tacotron2_amd.run import prosody_export as X
    assert FEATURES[:3] == ["duration", "duration_vcd", "pitch_mean"] and len(FEATURES) == 18 and "nhr_vcd" in FEATURES
    rng = np.random.default_rng(1)
    train, val = _frame(rng, (0, 1), 6), _frame(rng, (1, 0), 3, shift=4.0)               # val: other values, far enough to clip
    stats = X.norm_statistics(train, "speaker_id")
    assert set(stats["speakers"]) == {"0", "1"} and stats["dataset"]["n"] == 12 and stats["speakers"]["1"]["n"] == 6
    for df in (train, val):
        out = X.add_norm_columns(df, stats, "speaker_id")
        assert list(out.columns) == list(df.columns) + [f + s for s in ("_speaker_norm", "_speaker_norm_clip", "_dataset_norm",
                                                                        "_dataset_norm_clip") for f in FEATURES]
        assert (out[list(df.columns)].values == df.values).all() and list(out.wav) == list(df.wav)        # rows stay in place
        for f in FEATURES:
            z, zc = V.normalise(df[f], train[f])                                          # statistics of the TRAIN rows only
            assert np.allclose(out[f + "_dataset_norm"], z, rtol=1e-12, atol=1e-12)
            assert np.allclose(out[f + "_dataset_norm_clip"], zc, rtol=1e-12, atol=1e-12)
            for spk in (0, 1):
                m, mt = (df.speaker_id == spk).values, (train.speaker_id == spk).values
                z, zc = V.normalise(df[f][m], train[f][mt])
                assert np.allclose(out[f + "_speaker_norm"][m], z, rtol=1e-12, atol=1e-12)
                assert np.allclose(out[f + "_speaker_norm_clip"][m], zc, rtol=1e-12, atol=1e-12)
            assert out[f + "_speaker_norm_clip"].between(-1, 1).all() and out[f + "_dataset_norm_clip"].between(-1, 1).all()
    out = X.add_norm_columns(val, stats, "speaker_id")
    assert (out["duration_speaker_norm"].abs() > 1).any()                                 # ... and the clip did something
    assert stats["speakers"]["0"]["std"]["jitter"] == pytest.approx(np.std(train.jitter[train.speaker_id == 0], ddof=1), rel=1e-12)
    assert stats["speakers"]["0"]["median"]["jitter"] == pytest.approx(np.median(train.jitter[train.speaker_id == 0]), rel=1e-12)
    # one speaker when the column is absent: the speaker columns are the dataset columns
    one = X.norm_statistics(train.drop(columns="speaker_id"), None)
    o = X.add_norm_columns(val.drop(columns="speaker_id"), one, None)
    assert (o["rate_speaker_norm"] == o["rate_dataset_norm"]).all()
    # errors name the speaker
    with pytest.raises(X.ProsodyExportError, match="speaker 7 has 1 measured train utterance"):
        X.norm_statistics(_frame(rng, (0,), 4).assign(speaker_id=[0, 0, 0, 7]), "speaker_id")
    flat = train.copy()
    flat.loc[flat.speaker_id == 1, "shimmer"] = 0.25
    with pytest.raises(X.ProsodyExportError, match="speaker 1: the train standard deviation of shimmer is 0"):
        X.norm_statistics(flat, "speaker_id")
    with pytest.raises(X.ProsodyExportError, match="speaker 5 has no train utterance"):
        X.add_norm_columns(val.assign(speaker_id=5), stats, "speaker_id")
    with pytest.raises(X.ProsodyExportError, match="another manifest has none"):
        X.add_norm_columns(val.drop(columns="speaker_id"), stats, "speaker_id")


def test_dropped_rows_bookkeeping():
    import pandas as pd
    from tacotron2_amd.prosody import FEATURES
    from tacotron2_amd.run import prosody_export as X
    full = dict({f: 1.0 for f in FEATURES}, n_frames=10, n_voiced=8, n_measured=7)
    none = lambda keys, **kw: dict(full, **{k: None for k in keys}, **kw)
    pitch = [f for f in FEATURES if f.startswith("pitch")] + ["intensity_mean_vcd", "rate_vcd"]
    vq = ["jitter", "shimmer", "nhr", "nhr_vcd"]
    assert X.drop_reason(5000, full, 4096, 256) is None
    assert X.drop_reason(0, none(pitch + vq + ["rate", "intensity_mean"], n_frames=0, n_voiced=0, n_measured=0), 4096, 256) == "empty waveform"
    assert X.drop_reason(900, none(pitch + vq, n_frames=0, n_voiced=0, n_measured=0), 4096, 256) == "shorter than one analysis span"
    assert X.drop_reason(5000, none(pitch + vq, n_voiced=0, n_measured=0), 4096, 256) == "no voiced frame"
    assert X.drop_reason(5000, none(vq, n_measured=0), 4096, 256) == "no measured frame"
    assert X.drop_reason(5000, none(["intensity_mean"]), 4096, 256) == "undefined: intensity_mean"
    assert X.drop_reason(4096 * 256, None, 4096, 256) == "4097 frames, above the limit of 4096"
    df = pd.DataFrame(dict(text=list("abcd"), wav=["a.wav", "b.wav", "c.wav", "d.wav"], jitter=[9.0] * 4))
    feats = [dict(full, jitter=0.5), None, dict(full, jitter=0.7), none(vq, n_measured=0)]
    reasons = [X.drop_reason(5000, f, 4096, 256) for f in feats]
    out, dropped = X.assemble({"train": df}, {"train": feats}, {"train": reasons})
    assert dropped == [["train", "b.wav", "20 frames, above the limit of 4096"], ["train", "d.wav", "no measured frame"]]
    assert list(out["train"].columns) == ["text", "wav"] + FEATURES                        # (an old feature column is replaced)
    assert list(out["train"].wav) == ["a.wav", "c.wav"] and list(out["train"].jitter) == [0.5, 0.7]


def test_host_threads_follow_the_environment_and_never_the_cpu_count(monkeypatch):
    from tacotron2_amd.run import prosody_export as X
    monkeypatch.setattr(os, "cpu_count", lambda: 999)
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert X.host_threads() == 4
    for val, want in (("3", 3), ("16", 16), ("64", 16), ("0", 4), ("many", 4)):
        monkeypatch.setenv("OMP_NUM_THREADS", val)
        assert X.host_threads() == want


def test_prosody_export_usage_errors(tmp_path):
    from click.testing import CliRunner
    import main as cli
    run = lambda args: CliRunner().invoke(cli.main, args, obj={})
    r = run(["prosody-export", "--speech-dir", "x"])
    assert r.exit_code == 2 and "needs --config" in r.output
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"dataset": {"val": "v.csv"}, "training": {}, "model": {}}))
    r = run(["--config", str(cfgp), "prosody-export", "--speech-dir", "x"])
    assert r.exit_code == 2 and "dataset.train" in r.output
    cfgp.write_text(json.dumps({"dataset": {"train": "t.csv"}, "training": {}, "model": {}}))
    r = run(["--config", str(cfgp), "prosody-export"])
    assert r.exit_code == 2 and "--speech-dir" in r.output
    for bad in ("0", "-3", "x", "70000"):
        r = run(["--config", str(cfgp), "prosody-export", "--speech-dir", "x", "--batch-size", bad])
        assert r.exit_code == 2 and "--batch-size" in r.output, bad
    r = run(["--config", str(cfgp), "prosody-export", "--speech-dir", "x", "--checkpoint", "k"])
    assert r.exit_code == 2 and "No such option" in r.output                               # it needs no checkpoint
    assert "prosody-export" in run(["--help"]).output
    # the correlation side keeps its mapping: jitter and shimmer are not measures of test-correlation --measure
    from tacotron2_amd.run.correlation import measure_of
    assert measure_of("jitter") is None and measure_of("nhr_vcd_speaker_norm_clip") == "aperiodicity_mean"
