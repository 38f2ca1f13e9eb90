"""Host checks of the prosody measurement (no GPU): the float64 restatement of the YIN rule (tests/prosody_ref.py) behaves as a pitch
tracker should, the inputs of tests/test_gpu_prosody.py fit that test's stability cap, the correlation tables of
tacotron2_amd/run/correlation.py against hand-computed values, and the command line."""
import json
import math

import numpy as np
import pytest

import prosody_ref as R


@pytest.mark.parametrize("f", [70.0, 100.0, 155.5, 220.0, 330.0, 440.0])
def test_reference_tracks_steady_tones(f):
    """Steady four-harmonic tones of 6000 samples: all 18 valid frames voiced, f0 within 5e-4 relative (measured: at most 2.5e-4, at
    440 Hz, where one lag is 0.9 % of the period and the parabola through three lags carries the rest)."""
    r = R.yin([R.tone(f, 6000)])
    v = r["valid"][0]
    assert r["valid"].shape == (1, 1 + 6000 // 256) and v.sum() == 18
    assert not v[:3].any() and not v[21:].any()            # the span of 1391 samples must fit around sample 256 t
    assert r["voiced"][0][v].all()
    err = np.max(np.abs(r["f0"][0][v] - f) / f)
    print(f"{f} Hz: max relative f0 error {err:.3e}")
    assert err <= 5e-4
    inv = ~v
    assert (r["f0"][0][inv] == 0).all() and (r["aper"][0][inv] == 1).all() and (r["power"][0][inv] == 0).all()


def test_gpu_test_inputs_fit_the_stability_cap():
    """The five glides of the GPU test: the reference alone leaves at most 5 % of the valid frames unstable (measured: 1 of 151),
    and voiced, unvoiced and digitally silent frames are all present; the 1300-sample signal has no valid frame."""
    sig = R.glides()
    assert [len(s) for s in sig] == [9000, 12001, 7000, 1300, 16000]
    ref = R.yin(sig)
    st = R.stable_frames(ref)
    va = ref["valid"]
    n_unstable = int((va & ~st).sum())
    print(f"valid {va.sum()} per signal {va.sum(1).tolist()}, unstable {n_unstable}, voiced {ref['voiced'].sum()}")
    assert va.sum() == 151 and va.sum(1).tolist() == [30, 42, 22, 0, 57]
    assert n_unstable <= 0.05 * va.sum()
    assert ref["voiced"].sum() >= 80
    assert (va & ~ref["voiced"] & (ref["power"] > 1e-10)).sum() >= 10          # noise: unvoiced by its aperiodicity
    assert (va & (ref["power"] == 0)).sum() >= 1                                # exact zeros: unvoiced by the power floor
    assert (ref["cm"][va][:, 1:] == 1).any()                                    # ... with the `sum not positive` branch taken


def test_reference_pick_rule():
    cm = np.ones(12)
    cm[[4, 5, 6, 8]] = [0.09, 0.05, 0.07, 0.01]
    assert R.pick(cm, 2, 11, 0.1) == 5                    # the first lag under thr, walked down to its trough - not the global one
    assert R.pick(cm, 6, 11, 0.1) == 6                    # (6 is under thr; 7 is not lower)
    assert R.pick(cm, 2, 11, 0.005) == 8                  # none under thr: the argmin
    cm[:] = 0.5
    assert R.pick(cm, 3, 11, 0.1) == 3                    # ... its FIRST occurrence
    cm = np.ones(12)
    cm[[8, 9, 10]] = [0.05, 0.04, 0.03]
    assert R.pick(cm, 2, 11, 0.1) == 10                   # the walk ends at tau_max - 1
    assert R.pick(cm, 2, 10, 0.1) == 9


def test_reference_stats_percentiles_are_elements():
    f0 = np.array([0, 100, 100, 200, 0, 300, 400, 100], float)
    row = R.stats(f0, np.full(8, 0.1), np.full(8, 1e-2), np.array([1, 1, 1, 1, 1, 1, 0, 1], bool))
    assert row[0] == 7 and row[1] == 5                     # (400 sits on an invalid frame)
    assert row[3] == 100 and row[4] == 300                 # indices (5*4+50)//100 = 0 and (95*4+50)//100 = 4 of [100,100,100,200,300]
    assert abs(row[5] + 20.0) < 1e-12 and row[7] == 0
    assert all(math.isnan(v) for v in R.stats(np.zeros(4), np.ones(4), np.zeros(4), np.ones(4, bool))[2:7])


# --------------------------------------------------------------------------------------------------------------------------------
# correlation tables
# --------------------------------------------------------------------------------------------------------------------------------
def test_pearson_spearman_slope_hand_computed():
    from tacotron2_amd.run import correlation as K
    x, y = [1, 2, 3, 4, 5], [2, 1, 4, 3, 5]
    # dx = (-2..2), dy = (-1,-2,1,0,2): sxy = 2+2+0+0+4 = 8, sxx = syy = 10
    assert K.pearson(x, y) == pytest.approx(0.8, abs=1e-15)
    assert K.spearman(x, y) == pytest.approx(0.8, abs=1e-15)           # (the values are their own ranks)
    assert K.slope(x, y) == pytest.approx(0.8, abs=1e-15)
    # ties: x = (1,1,2,3) has ranks (1.5,1.5,3,4); y = (2,1,3,3) has ranks (2,1,3.5,3.5); both means 2.5
    # d_rx = (-1,-1,.5,1.5), d_ry = (-.5,-1.5,1,1): s = .5+1.5+.5+1.5 = 4, sxx = 4.5, syy = 4.5
    assert K.average_ranks([1, 1, 2, 3]).tolist() == [1.5, 1.5, 3.0, 4.0]
    assert K.average_ranks([2, 1, 3, 3]).tolist() == [2.0, 1.0, 3.5, 3.5]
    assert K.spearman([1, 1, 2, 3], [2, 1, 3, 3]) == pytest.approx(4 / 4.5, abs=1e-15)
    assert K.spearman([1, 2, 3, 4], [1, 8, 27, 1000]) == 1.0 and K.pearson([1, 2, 3, 4], [1, 8, 27, 1000]) < 0.9
    assert K.pearson([1, 2, 3], [3, 2, 1]) == -1.0


def test_degenerate_columns_are_null():
    from tacotron2_amd.run import correlation as K
    for fn in (K.pearson, K.spearman, K.slope):
        assert fn([1, 2], [1, 2]) is None                  # fewer than 3 points
        assert fn([], []) is None
        assert fn([1, 1, 1], [1, 2, 3]) is None            # zero variance, either side
        assert fn([1, 2, 3], [5, 5, 5]) is None


def test_feature_names_map_by_prefix():
    from tacotron2_amd.run.correlation import measure_of
    assert measure_of("pitch_mean_speaker_norm") == "pitch_mean_log" and measure_of("pitch_mean") == "pitch_mean_log"
    assert measure_of("pitch_range_norm_clip") == "pitch_range_log"
    assert measure_of("intensity_mean_vcd_speaker_norm") == "intensity_mean_db"
    assert measure_of("nhr_vcd") == "aperiodicity_mean" and measure_of("rate_speaker_norm") == "rate"
    assert measure_of("jitter") is None and measure_of("shimmer_speaker_norm") is None and measure_of("f0") is None


def test_override_directory_names():
    from tacotron2_amd.run.correlation import parse_override_dir
    from tacotron2_amd.run.test_correlation import feature_overrides
    for ov in feature_overrides(5):
        assert parse_override_dir(str(ov), 5) == ov
    assert parse_override_dir("(-0.0, 0.0, 1)", 3) == (0.0, 0.0, 1.0)
    for bad, n in (("(0.0, 0.0)", 5), ("notes", 5), ("[0.0, 0.0]", 2), ("(0.0, 'a')", 2), ("__import__('os')", 1), ("0.5", 1)):
        with pytest.raises(ValueError) as e:
            parse_override_dir(bad, n)
        assert repr(bad) in str(e.value) and f"{n} numbers" in str(e.value)


def test_correlation_tables_sweeps_and_leakage(tmp_path, capsys):
    """Control 0 drives its own measure linearly and leaks into `rate`; control 1 is not measured; control 2 has too few points.
    Rows of overrides that move ANOTHER control stay out of a control's sweep; the all-zero override is in every sweep."""
    from tacotron2_amd.run import correlation as K
    feats = ["pitch_mean_speaker_norm", "jitter", "intensity_mean"]
    row = lambda **kw: dict({m: None for m in K.MEASURES}, **kw)
    per = {(0.0, 0.0, 0.0): [row(pitch_mean_log=5.0, rate=10.0, intensity_mean_db=-20.0)] * 2}
    for x in (-1.0, -0.5, 0.5, 1.0):
        per[(x, 0.0, 0.0)] = [row(pitch_mean_log=5.0 + 0.3 * x, rate=10.0 - x * x, intensity_mean_db=-20.0), row(rate=10.0)]
    per[(0.0, 0.7, 0.0)] = [row(pitch_mean_log=9.0, rate=1.0, intensity_mean_db=0.0)]
    per[(0.0, 0.0, 1.0)] = [row(intensity_mean_db=None)]
    t = K.write_correlation(str(tmp_path), feats, per, {"W": 1024})
    c0, c1, c2 = t["controls"]
    assert c0["measure"] == "pitch_mean_log" and c0["n"] == 6 and c0["n_dropped"] == 4
    assert c0["pearson"] == pytest.approx(1.0, abs=1e-12) and c0["spearman"] == pytest.approx(1.0, abs=1e-12)
    assert c0["slope"] == pytest.approx(0.3, abs=1e-12)
    assert c1 == {"feature": "jitter", "measure": None, "n": 0, "n_dropped": 0, "pearson": None, "spearman": None, "slope": None}
    assert c2["measure"] == "intensity_mean_db" and c2["n"] == 2 and c2["n_dropped"] == 1 and c2["pearson"] is None
    m = t["pearson_matrix"]
    assert set(m) == set(feats) and all(list(v) == K.MEASURES for v in m.values())
    assert m[feats[0]]["pitch_mean_log"] == pytest.approx(1.0, abs=1e-12)
    assert m[feats[0]]["rate"] == pytest.approx(0.0, abs=1e-12)             # x against -x^2 over a symmetric sweep
    assert m[feats[0]]["intensity_mean_db"] is None and m[feats[0]]["aperiodicity_mean"] is None
    on_disk = json.loads((tmp_path / "correlation.json").read_text())
    assert on_disk == json.loads(json.dumps(t)) and on_disk["yin"] == {"W": 1024}
    assert "null" in (tmp_path / "correlation.json").read_text() and "NaN" not in (tmp_path / "correlation.json").read_text()
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 3 and out[0].startswith(f"{feats[0]} -> pitch_mean_log: n 6 (dropped 4), pearson +1.0000")
    assert out[1] == "jitter: not measured"


def test_prosody_csv_layout(tmp_path):
    from tacotron2_amd.run import correlation as K
    assert "|".join(K.PROSODY_HEADER) == ("i|wav|n_chars|seconds|stopped|n_frames|n_voiced|pitch_mean_log|pitch_range_log|"
                                          "intensity_mean_db|aperiodicity_mean|rate")
    K.write_prosody_csv(str(tmp_path), [
        dict(i=1, wav="1.wav", n_chars=9, seconds=0.5, stopped=1, n_frames=3, n_voiced=2, pitch_mean_log=5.25, pitch_range_log=0.0,
             intensity_mean_db=-21.5, aperiodicity_mean=0.0125, rate=18.0),
        dict(i=2, wav="2.wav", n_chars=4, seconds=0.0, stopped=0, n_frames=0, n_voiced=0, pitch_mean_log=None, pitch_range_log=None,
             intensity_mean_db=None, aperiodicity_mean=None, rate=None)])
    lines = (tmp_path / "prosody.csv").read_text().splitlines()
    assert lines[1] == "1|1.wav|9|0.500000|1|3|2|5.250000|0.000000|-21.500000|0.012500|18.000000"
    assert lines[2] == "2|2.wav|4|0.000000|0|0|0|||||"


# --------------------------------------------------------------------------------------------------------------------------------
# command line
# --------------------------------------------------------------------------------------------------------------------------------
def test_cli_help_lists_the_option_and_the_command():
    from click.testing import CliRunner
    import main as cli
    r = CliRunner().invoke(cli.main, ["--help"], obj={})
    assert r.exit_code == 0 and "measure-correlation" in r.output
    r = CliRunner().invoke(cli.main, ["test-correlation", "--help"], obj={})
    assert r.exit_code == 0 and "--measure" in r.output
    r = CliRunner().invoke(cli.main, ["measure-correlation", "--help"], obj={})
    assert r.exit_code == 0 and "--results-dir" in r.output and "--features" in r.output
    assert "--measure" not in CliRunner().invoke(cli.main, ["test", "--help"], obj={}).output


def test_cli_measure_correlation_usage_errors(tmp_path):
    """A directory that is no override tuple of the right length is a usage error that names it, before any GPU work; so are missing
    feature names."""
    from click.testing import CliRunner
    import main as cli
    (tmp_path / "(0.0, 0.0)").mkdir()
    (tmp_path / "(0.0, 0.0, 0.0)").mkdir()
    r = CliRunner().invoke(cli.main, ["measure-correlation", "--results-dir", str(tmp_path), "--features", "pitch_mean,rate"], obj={})
    assert r.exit_code == 2 and "'(0.0, 0.0, 0.0)'" in r.output and "2 numbers" in r.output
    r = CliRunner().invoke(cli.main, ["measure-correlation", "--results-dir", str(tmp_path)], obj={})
    assert r.exit_code == 2 and "--features" in r.output
    r = CliRunner().invoke(cli.main, ["measure-correlation", "--results-dir", str(tmp_path / "nope"), "--features", "rate"], obj={})
    assert r.exit_code == 2 and "not a directory" in r.output


def test_driver_gets_the_flag_through_the_model_config_only_when_asked(monkeypatch):
    """`test-correlation` without --measure calls the driver exactly as before; with it, the model config carries measure_prosody (as
    it carries the attention window: load_test_model reads it), the results directory has a name, and the tables are made from it."""
    from click.testing import CliRunner
    import main as cli
    from tacotron2_amd.run import correlation as K
    from tacotron2_amd.run import test_correlation as tc
    seen, trees = [], []
    monkeypatch.setattr(tc, "do_test_correlation", lambda **kw: seen.append(kw))
    monkeypatch.setattr(K, "correlate_tree", lambda base, feats, yin: trees.append((base, feats, yin)))
    monkeypatch.setattr(cli, "load_config", lambda p: {"dataset": {}, "training": {"name": "tiny"}, "model": {"a": 1},
                                                       "extensions": {"controls": {"active": True, "features": ["rate", "nhr"]}}})
    base = ["--config", "c.json", "test-correlation", "--speech-dir", "s", "--checkpoint", "k.ckpt"]
    assert CliRunner().invoke(cli.main, base, obj={}).exit_code == 0
    assert seen[0]["model_config"] == {"a": 1} and seen[0]["results_dir"] is None and trees == []
    r = CliRunner().invoke(cli.main, base + ["--measure"], obj={})
    assert r.exit_code == 0, (r.output, r.exception)
    assert seen[1]["model_config"] == {"a": 1, "measure_prosody": True}
    assert seen[1]["results_dir"].startswith("results_tiny_test_correlation 2")
    assert {k: v for k, v in seen[1].items() if k not in ("model_config", "results_dir")} == \
        {k: v for k, v in seen[0].items() if k not in ("model_config", "results_dir")}
    assert len(trees) == 1 and trees[0][0] == seen[1]["results_dir"] and trees[0][1] == ["rate", "nhr"]
    assert trees[0][2]["tau_max"] == 367 and trees[0][2]["W"] == 1024
    r = CliRunner().invoke(cli.main, base + ["--measure", "--results-dir", "out/r"], obj={})
    assert r.exit_code == 0 and seen[2]["results_dir"] == "out/r" and trees[1][0] == "out/r"


def test_correlate_tree_reads_the_csv_of_every_override(tmp_path, capsys):
    from tacotron2_amd.run import correlation as K
    row = lambda i, pm: dict(i=i, wav=f"{i}.wav", n_chars=3, seconds=0.5, stopped=1, n_frames=4, n_voiced=int(pm is not None),
                             pitch_mean_log=pm, pitch_range_log=None, intensity_mean_db=None, aperiodicity_mean=None, rate=6.0)
    for x in (-1.0, 0.0, 1.0):
        d = tmp_path / str((x, 0.0))
        d.mkdir()
        K.write_prosody_csv(str(d), [row(1, 5.0 + 0.25 * x), row(2, None)])
    assert K.read_prosody_csv(str(tmp_path / "(1.0, 0.0)"))[1] == dict(pitch_mean_log=None, pitch_range_log=None, intensity_mean_db=None,
                                                                       aperiodicity_mean=None, rate=6.0)
    t = K.correlate_tree(str(tmp_path), ["pitch_mean", "rate"], {"W": 1024})
    assert t["controls"][0]["n"] == 3 and t["controls"][0]["n_dropped"] == 3 and t["controls"][0]["slope"] == pytest.approx(0.25)
    assert t["controls"][1]["n"] == 2 and t["controls"][1]["pearson"] is None           # only the all-zero override is in its sweep
    assert json.loads((tmp_path / "correlation.json").read_text())["yin"] == {"W": 1024}
    (tmp_path / "notes").mkdir()
    with pytest.raises(ValueError, match="'notes'"):
        K.correlate_tree(str(tmp_path), ["pitch_mean", "rate"], {})
