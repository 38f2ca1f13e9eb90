"""`main.py test --score --f0` and `main.py test-correlation --measure --smooth-pitch` on the GPU through their click entries in this
process, on the tiny models and generated recordings of test_gpu_cli_score.py and test_gpu_cli_prosody.py (utterances stop within a few
frames, so most tracks are shorter than one analysis span: these cases check the plumbing and the files), then prosody.f0_scores and
ProsodyMeter(smooth=True) on signals long enough to carry a track."""
import json
import os

import numpy as np
import pytest
import torch

import pitch_ref as P
import prosody_ref as R
from test_gpu_cli_prosody import HEADER as PROSODY_HEADER, _rows as prosody_rows, _sweep, ctrl_setup      # noqa: F401 (fixture)
from test_gpu_cli_score import _rows as score_rows, _test_cmd, setup                                      # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
F0_HEADER = "i|wav|stopped|n_pairs|n_voiced_both|f0_rmse_cents|f0_bias_cents|f0_corr|vuv_error"
MEANS = ["f0_rmse_cents_mean", "f0_bias_cents_mean", "f0_corr_mean", "vuv_error_mean"]


def test_score_f0_adds_its_file_and_its_keys_and_changes_nothing_else(setup):
    s = setup
    scored, with_f0 = s["tmp"] / "res_scored_f0base", s["tmp"] / "res_f0"
    r = _test_cmd(s, scored, ["--score"])
    assert r.exit_code == 0, (r.output, r.exception)
    r = _test_cmd(s, with_f0, ["--score", "--f0"])
    assert r.exit_code == 0, (r.output, r.exception)
    files = sorted(os.listdir(scored))
    assert sorted(os.listdir(with_f0)) == sorted(files + ["f0_scores.csv"])
    for f in files:
        if f != "scores.json":
            assert (scored / f).read_bytes() == (with_f0 / f).read_bytes(), f             # scores.csv and the WAVs, byte for byte
    lines = (with_f0 / "f0_scores.csv").read_text().splitlines()
    assert lines[0] == F0_HEADER and len(lines) == 4
    rows = [dict(zip(F0_HEADER.split("|"), l.split("|"))) for l in lines[1:]]
    print("f0_scores.csv:", rows)
    sc = score_rows(with_f0)
    for k, (row, srow) in enumerate(zip(rows, sc)):
        assert row["i"] == str(k + 1) and row["wav"] == f"u{k}.wav" and row["stopped"] == srow["stopped"]
        if row["stopped"] == "0":
            assert [row[c] for c in F0_HEADER.split("|")[3:]] == [""] * 6
            continue
        assert 0 <= int(row["n_voiced_both"]) <= int(row["n_pairs"]) <= int(srow["path_len"])
        assert (row["vuv_error"] == "") == (int(row["n_pairs"]) == 0)
        assert (row["f0_rmse_cents"] == "") == (int(row["n_voiced_both"]) == 0) == (row["f0_bias_cents"] == "")
        if row["vuv_error"]:
            assert 0.0 <= float(row["vuv_error"]) <= 1.0
    base, agg = json.loads((scored / "scores.json").read_text()), json.loads((with_f0 / "scores.json").read_text())
    assert not any(k in base for k in MEANS) and "f0" not in base["settings"]
    assert agg["settings"].pop("f0") == dict(sr=22050, hop=256, W=1024, fmin=60.0, fmax=500.0, thr=0.1, vthr=0.3, power_floor=1e-10,
                                             tau_min=44, tau_max=367, smooth=True, w=1.0, max_jump=0.25, u=0.3, c_sw=0.15)
    for m in MEANS:
        v = [float(r_[m[:-5]]) for r_ in rows if r_["stopped"] == "1" and r_[m[:-5]] != ""]
        got = agg.pop(m)
        assert (got is None and not v) or abs(got - np.mean(v)) < 1e-5, m
    assert agg == base                                                                  # everything else is what --score wrote


def test_smooth_pitch_keeps_the_csv_header_and_records_its_settings(ctrl_setup):
    s = ctrl_setup
    res = s["tmp"] / "smoothed"
    r = _sweep(s, res, ["--measure", "--smooth-pitch"])
    assert r.exit_code == 0, (r.output, r.exception)
    dirs = [d for d in os.listdir(res) if d != "correlation.json"]
    assert len(dirs) == 2
    for d in dirs:
        rows = prosody_rows(res / d)                                                    # (asserts the unchanged header)
        assert [r_["i"] for r_ in rows] == [str(i) for i in range(1, 7)]
        for r_ in rows:
            assert 0 <= int(r_["n_voiced"]) <= int(r_["n_frames"])
    t = json.loads((res / "correlation.json").read_text())
    assert t["yin"]["smooth"] is True and t["yin"]["w"] == 1.0 and t["yin"]["max_jump"] == 0.25 and t["yin"]["u"] == 0.3 \
        and t["yin"]["c_sw"] == 0.15 and t["yin"]["tau_max"] == 367


def test_smooth_meter_takes_the_octave_out_of_the_pitch_range():
    """The octave signal: the smoothed pitch_range_log lies below the unsmoothed one.  On the whole signal the float64 restatements give
    0.00254 against 0.00117 - only 3 of its 57 voiced frames are read an octave high, and the nearest-rank p95 of 57 values is the
    fourth largest, so the unsmoothed RANGE does not contain the octave there.  Its first 7000 samples (22 voiced frames, the same 3
    among them: p95 is the second largest) show the inflation: ln p95 - ln p5 = 0.694 = ln 2 unsmoothed, 0.0016 smoothed."""
    from tacotron2_amd.prosody import ProsodyMeter
    dev = torch.device("cuda:0")
    x = P.octave_signal()
    wavs = [torch.from_numpy(x).to(dev), torch.from_numpy(x[:7000].copy()).to(dev)]
    raw = ProsodyMeter(22050, dev).measure(wavs, [10, 5])
    smooth = ProsodyMeter(22050, dev, smooth=True).measure(wavs, [10, 5])
    for k in range(2):
        print(f"utterance {k}: pitch_range_log unsmoothed {raw[k]['pitch_range_log']:.6f} (n_voiced {raw[k]['n_voiced']}), smoothed "
              f"{smooth[k]['pitch_range_log']:.6f} (n_voiced {smooth[k]['n_voiced']})")
        assert smooth[k]["pitch_range_log"] < raw[k]["pitch_range_log"]
        assert raw[k]["n_frames"] == smooth[k]["n_frames"] and smooth[k]["n_voiced"] > 0
        assert abs(smooth[k]["pitch_mean_log"] - np.log(110.0)) < 5e-3
        assert smooth[k]["intensity_mean_db"] is not None and smooth[k]["rate"] == raw[k]["rate"]
    assert raw[1]["pitch_range_log"] > 0.6 and smooth[1]["pitch_range_log"] < 0.01         # ln 2 = 0.693 against a steady 110 Hz


def test_f0_scores_of_tones_an_octave_and_a_semitone_apart():
    """Identity paths over two batches of tones: the synthesis at 110 Hz against recordings at 220 and 105 Hz gives -1200 and +80.5
    cents; an empty synthesis scores nothing.  (Tones whose period lies near an integer lag: the decode has no prior towards the
    shorter lag, and a steady tone whose DOUBLED period lies closer to an integer than its period is read an octave low - DESIGN 5.11.)"""
    from tacotron2_amd.prosody import F0_MEASURES, ProsodyMeter, f0_scores
    dev = torch.device("cuda:0")
    n = 9000
    syn = [R.tone(110.0, n), R.tone(110.0, n), np.zeros(0, np.float32)]
    ref = [R.tone(220.0, n), R.tone(105.0, n - 1300), R.tone(110.0, n)]
    T = 1 + n // 256
    path = torch.arange(T, dtype=torch.int32, device=dev)[None, :, None].expand(3, T, 2).contiguous()
    path_len = torch.tensor([T, T, 0], dtype=torch.int32, device=dev)
    meter = ProsodyMeter(22050, dev, smooth=True)
    f0, nn = meter.tracks([torch.from_numpy(x).to(dev) for x in syn])
    assert f0.shape == (3, T) and nn.tolist() == [n, n, 0] and not f0[2].any()
    got = f0_scores(meter, [torch.from_numpy(x).to(dev) for x in syn], [torch.from_numpy(x).to(dev) for x in ref], path, path_len)
    print(got)
    valid = lambda m: sum(1 for t in range(T) if 256 * t - 695 >= 0 and 256 * t + 696 <= m)
    assert got[0]["n_pairs"] == got[0]["n_voiced_both"] == valid(n) and got[0]["vuv_error"] == 0.0
    assert abs(got[0]["f0_bias_cents"] + 1200.0) < 5.0 and abs(got[0]["f0_rmse_cents"] - 1200.0) < 5.0
    assert got[1]["n_pairs"] == got[1]["n_voiced_both"] == valid(n - 1300)
    assert abs(got[1]["f0_bias_cents"] - 1200.0 * np.log2(110.0 / 105.0)) < 5.0
    assert got[0]["f0_corr"] is None or -1.0 <= got[0]["f0_corr"] <= 1.0
    assert got[2] == dict(n_pairs=0, n_voiced_both=0, **{m: None for m in F0_MEASURES})
    with pytest.raises(ValueError):
        f0_scores(meter, [torch.zeros(10, device=dev)], [], path, path_len)
    assert f0_scores(meter, [], [], path, path_len) == []
