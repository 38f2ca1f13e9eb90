"""`main.py measure-correlation` and `main.py test-correlation --measure` on the GPU, through their click entries in this process.

measure-correlation runs on a tree this test writes: square waves (|x| is constant, so the frame power - and with it the measured
intensity - does not depend on the pitch at all) whose pitch follows exp(0.2 x) of control 0 and whose amplitude follows control 2.
The three WAVs of a directory are the same signal: the requested value is tied within a directory, and a Spearman coefficient of
exactly 1 needs the measure tied there too.  test-correlation --measure runs on the reference-generated `infer_ctrl` weights, whose
utterances stop after a few frames: for some of them audio shorter than one analysis span, for none enough to correlate."""
import json
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"
FEATS = ["pitch_mean_speaker_norm", "pitch_range_speaker_norm", "intensity_mean_speaker_norm", "nhr_speaker_norm", "rate_speaker_norm"]
HEADER = "i|wav|n_chars|seconds|stopped|n_frames|n_voiced|pitch_mean_log|pitch_range_log|intensity_mean_db|aperiodicity_mean|rate"
LEVELS = [round(float(j), 1) for j in np.arange(-1, 1.1, 0.2)]


def _square(f, n, amp, sr=22050):
    q = int(round(amp * 32767))
    return np.where(np.sin(2 * np.pi * f * np.arange(n) / sr + 0.1) >= 0, q, -q).astype("<i2")


def _write(path, pcm, sr=22050):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes(pcm.tobytes())


def _rows(d):
    lines = (d / "prosody.csv").read_text().splitlines()
    assert lines[0] == HEADER
    return [dict(zip(HEADER.split("|"), l.split("|"))) for l in lines[1:]]


def test_measure_correlation_on_a_written_tree(tmp_path):
    from click.testing import CliRunner
    import main as cli
    tree = tmp_path / "res"
    overrides = {(x, 0.0, 0.0, 0.0, 0.0) for x in LEVELS} | {(0.0, 0.0, x, 0.0, 0.0) for x in LEVELS}
    assert len(overrides) == 21                               # the all-zero override belongs to both sweeps
    for ov in overrides:
        d = tree / str(ov)
        d.mkdir(parents=True)
        pcm = _square(150.0 * np.exp(0.2 * ov[0]), 5000, 0.2 * np.exp(0.8 * ov[2]))
        for i in (1, 2, 3):
            _write(d / f"{i}.wav", pcm)
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps({"dataset": {}, "training": {}, "model": {},
                                "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": True, "features": FEATS}}}))
    r = CliRunner().invoke(cli.main, ["--config", str(cfgp), "--device", "0", "measure-correlation", "--results-dir", str(tree)], obj={})
    assert r.exit_code == 0, (r.output, r.exception)
    t = json.loads((tree / "correlation.json").read_text())
    print(r.output)
    assert t["features"] == FEATS and t["yin"]["W"] == 1024 and t["yin"]["tau_max"] == 367 and t["yin"]["sr"] == 22050
    by = {c["feature"]: c for c in t["controls"]}
    for feat, measure in ((FEATS[0], "pitch_mean_log"), (FEATS[2], "intensity_mean_db")):
        c = by[feat]
        assert c["measure"] == measure and c["n"] == 33 and c["n_dropped"] == 0
        assert c["spearman"] == pytest.approx(1.0, abs=1e-12) and c["pearson"] > 0.99
    assert by[FEATS[0]]["slope"] == pytest.approx(0.2, abs=2e-3)
    assert by[FEATS[2]]["slope"] == pytest.approx(0.8 * 20 / np.log(10), rel=1e-3)          # dB per unit of the control
    cross = t["pearson_matrix"][FEATS[0]]["intensity_mean_db"]
    assert cross is None or -0.2 <= cross <= 0.2             # pitch control against intensity: constant by construction
    assert t["pearson_matrix"][FEATS[2]]["intensity_mean_db"] == by[FEATS[2]]["pearson"]
    assert by[FEATS[1]]["n"] == 3 and by[FEATS[1]]["pearson"] is None                        # only the all-zero override: no sweep
    assert by[FEATS[4]]["n"] == 0 and by[FEATS[4]]["n_dropped"] == 3                        # the WAVs carry no text: no rate
    for ov in overrides:
        rows = _rows(tree / str(ov))
        assert [r_["i"] for r_ in rows] == ["1", "2", "3"] and all(r_["stopped"] == "1" and r_["rate"] == "" for r_ in rows)
        assert all(int(r_["n_frames"]) == 14 == int(r_["n_voiced"]) for r_ in rows)
        assert rows[0]["pitch_mean_log"] == rows[1]["pitch_mean_log"] == rows[2]["pitch_mean_log"]
        assert abs(float(rows[0]["pitch_mean_log"]) - np.log(150.0) - 0.2 * ov[0]) < 2e-3
    # a directory that is no override of this many controls is named, and nothing is rewritten
    (tree / "(0.0, 0.0)").mkdir()
    before = (tree / "correlation.json").read_bytes()
    r = CliRunner().invoke(cli.main, ["--device", "0", "measure-correlation", "--results-dir", str(tree), "--features", ",".join(FEATS)],
                           obj={})
    assert r.exit_code == 2 and "'(0.0, 0.0)'" in r.output and (tree / "correlation.json").read_bytes() == before


@pytest.fixture(scope="module")
def ctrl_setup(tmp_path_factory):
    from helpers import load_golden, params_from, write_hifigan_checkpoint
    tmp = tmp_path_factory.mktemp("prosody_cli")
    sd = {"tacotron2." + k: v for k, v in params_from(load_golden("infer_ctrl")).items()}
    hp = dict(lr=1e-3, weight_decay=1e-6, num_chars=39, encoded_dim=32, num_mels=16, prenet_dim=16, att_rnn_dim=32, att_dim=16,
              rnn_hidden_dim=32, postnet_dim=32, dropout=0.5, controls=True, controls_dim=5)
    ck = tmp / "m.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hp, "global_step": 0, "epoch": 0}, ck)
    rows = ["text|wav|speaker_id|" + "|".join(FEATS)]
    for spk in (0, 1):
        rows += [f"{t}|none{spk}{i}.wav|{spk}|0.1|0.2|0.3|0.4|0.5" for i, t in enumerate(
            ["Hi there.", "A somewhat longer sentence, Dr. Who!", "ok", "Testing: one; two? three."])]
    csvp = tmp / "test.csv"
    csvp.write_text("\n".join(rows) + "\n")
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv", "test": str(csvp),
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "num_mels": 16}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "args": {"max_steps": 6}},
           "model": {"scheduler_milestones": [], "args": {"prenet_dim": 16, "att_rnn_dim": 32, "att_dim": 16, "rnn_hidden_dim": 32,
                                                          "postnet_dim": 32, "dropout": 0.5, "char_embedding_dim": 32}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": True, "features": FEATS}}}
    cfgp = tmp / "cfg.json"
    cfgp.write_text(json.dumps(cfg))
    gck = write_hifigan_checkpoint(str(tmp / "hifi"), n_mels=16)
    return dict(tmp=tmp, ck=ck, cfgp=cfgp, gck=gck)


def _sweep(s, res, extra):
    from click.testing import CliRunner
    import main as cli
    return CliRunner().invoke(cli.main, ["--config", str(s["cfgp"]), "--device", "0", "test-correlation", "--speech-dir", "unused",
                                         "--checkpoint", str(s["ck"]), "--results-dir", str(res), "--samples-per-speaker", "3",
                                         "--max-len", "40", "--limit-overrides", "2", "--hifi-gan-checkpoint", s["gck"]] + extra, obj={})


def test_test_correlation_measure_adds_its_files_and_changes_nothing_else(ctrl_setup):
    from tacotron2_amd.run.test_correlation import feature_overrides
    s = ctrl_setup
    plain, measured = s["tmp"] / "plain", s["tmp"] / "measured"
    r = _sweep(s, plain, [])
    assert r.exit_code == 0, (r.output, r.exception)
    r = _sweep(s, measured, ["--measure"])
    assert r.exit_code == 0, (r.output, r.exception)
    want = [str(o) for o in list(feature_overrides(5))[:2]]
    assert sorted(os.listdir(plain)) == sorted(want)
    assert sorted(os.listdir(measured)) == sorted(want + ["correlation.json"])
    n_stopped, n_short, measured_rows = 0, 0, {}
    for w_ in want:
        files = sorted(os.listdir(plain / w_))
        assert "prosody.csv" not in files and sorted(os.listdir(measured / w_)) == sorted(files + ["prosody.csv"])
        for f in files:
            assert (plain / w_ / f).read_bytes() == (measured / w_ / f).read_bytes(), (w_, f)
        fails = set()
        if "failures.csv" in files:
            fails = {int(l.split("|")[0]) for l in (plain / w_ / "failures.csv").read_text().splitlines()}
        rows = _rows(measured / w_)
        assert [r_["i"] for r_ in rows] == [str(i) for i in range(1, 7)]
        for r_ in rows:
            i = int(r_["i"])
            with wave.open(str(measured / w_ / f"{i}.wav"), "rb") as w:
                n = w.getnframes()
            assert r_["wav"] == f"{i}.wav" and int(r_["n_chars"]) > 0 and abs(float(r_["seconds"]) - n / 22050) < 1e-6
            assert r_["stopped"] == ("0" if i in fails else "1") and (n == 0) == (i in fails)
            # frames whose span of 1391 samples around sample 256 t lies inside the waveform: none for the shorter utterances
            n_frames = sum(1 for t in range(1 + n // 256) if 256 * t - 695 >= 0 and 256 * t + 696 <= n)
            assert int(r_["n_frames"]) == n_frames and 0 <= int(r_["n_voiced"]) <= n_frames
            n_short += n_frames == 0 and i not in fails
            track = [r_[k] for k in ("pitch_mean_log", "pitch_range_log", "intensity_mean_db", "aperiodicity_mean")]
            if int(r_["n_voiced"]) == 0:
                assert track == ["", "", "", ""]
            else:
                assert all(np.isfinite(float(v)) for v in track)
                measured_rows[w_] = measured_rows.get(w_, 0) + 1
            if i in fails:
                assert r_["rate"] == "" and n_frames == 0
            else:
                n_stopped += 1
                assert abs(float(r_["rate"]) - int(r_["n_chars"]) / (n / 22050)) < 1e-3 * float(r_["rate"])
    print(f"{n_stopped} stopped, {n_short} of them shorter than one span, rows with a track: {measured_rows}")
    assert n_stopped >= 3 and n_short >= 1                      # (measured: 6 stopped, 5 of them shorter than one span)
    t = json.loads((measured / "correlation.json").read_text())
    assert t["features"] == FEATS and [c["measure"] for c in t["controls"]] == ["pitch_mean_log", "pitch_range_log", "intensity_mean_db",
                                                                               "aperiodicity_mean", "rate"]
    ovs = list(feature_overrides(5))[:2]
    for k, c in enumerate(t["controls"][:4]):                   # the rows of control k's sweep that carry a track
        n_k = sum(measured_rows.get(str(o), 0) for o in ovs if all(o[j] == 0 for j in range(5) if j != k))
        assert c["n"] == n_k
        if n_k < 3:
            assert c["pearson"] is None and c["spearman"] is None and c["slope"] is None
            assert all(v is None for m, v in t["pearson_matrix"][FEATS[k]].items() if m != "rate")
    assert "-> rate:" in r.output and f"{FEATS[0]} -> pitch_mean_log: n {t['controls'][0]['n']} (dropped" in r.output
