"""The float64 restatement tests/pitch_ref.py held to its own claims on the CPU: the octave signal, the glides, the tie
rules, a silent frame, the path statistics - and the command line's usage errors and the unsmoothed meter's unchanged description.
The kernels are held to this reference in tests/test_gpu_pitch.py."""
import functools
import math

import numpy as np
import pytest

import pitch_ref as P
import prosody_ref as R

CFG = dict(R.DEFAULTS)


@functools.lru_cache(maxsize=None)
def decoded(name):
    """(float64 YIN reference, [Viterbi output per utterance]) with the default settings; the Viterbi reads the reference's cmnd and
    power rounded to float32, as the kernel does."""
    signals = [P.octave_signal()] if name == "octave" else R.glides()
    ref = R.yin(signals, **CFG)
    lw = P.lag_weights(CFG["tau_min"], CFG["tau_max"], P.DEFAULTS["w"])
    T = ref["cm"].shape[1]
    outs = [P.viterbi_fast(ref["cm"][b].astype(np.float32), ref["power"][b].astype(np.float32), min(T, 1 + len(s) // CFG["hop"]),
                           CFG["tau_min"], CFG["tau_max"], lw, P.DEFAULTS["w"] * P.DEFAULTS["max_jump"], P.DEFAULTS["u"],
                           P.DEFAULTS["c_sw"], CFG["power_floor"], CFG["sr"]) for b, s in enumerate(signals)]
    return ref, outs


def test_octave_signal_raw_yin_jumps_and_the_viterbi_track_does_not():
    ref, (vit,) = decoded("octave")
    raw_v, raw_f0 = ref["voiced"][0], ref["f0"][0]
    vit_v = vit["lag"] > 0
    off = lambda f: np.abs(np.log2(f / 110.0)) > 0.5
    print("raw off-octave frames:", raw_f0[raw_v][off(raw_f0[raw_v])], "voiced", raw_v.sum())
    assert raw_v.sum() == 57 and (vit_v == raw_v).all()
    assert off(raw_f0[raw_v]).sum() >= 3
    assert off(vit["f0"][vit_v]).sum() == 0


def test_glides_voicing_equals_the_raw_rule_and_f0_stays_close():
    ref, outs = decoded("glides")
    frames, worst = 0, 0.0
    for b, vit in enumerate(outs):
        raw_v, vit_v = ref["voiced"][b], vit["lag"] > 0
        assert (raw_v == vit_v).all(), b
        frames += len(raw_v)
        if raw_v.any():
            worst = max(worst, float(np.max(np.abs(1200 * np.log2(vit["f0"][raw_v] / ref["f0"][b][raw_v])))))
    print(f"{frames} frames, largest |cents| between the smoothed and the raw track {worst:.1f}")
    assert frames == 315 and worst <= 50.0


def _small(cm_rows, power=None, n=None, w=1.0, trans_max=10.0, u=0.5, c_sw=0.25, fn=P.viterbi):
    """tau_min = 2, tau_max = 5: lags 2, 3, 4 and U - four states; cm_rows[t] = the cmnd of lags 2 .. 4 (lags 0, 1, 5 hold 1)."""
    T = len(cm_rows)
    cm = np.ones((T, 6), np.float32)
    cm[:, 2:5] = np.asarray(cm_rows, np.float32)
    power = np.ones(T, np.float32) if power is None else np.asarray(power, np.float32)
    return fn(cm, power, T if n is None else n, 2, 5, P.lag_weights(2, 5, w), trans_max, u, c_sw, 1e-10, 8000)


@pytest.mark.parametrize("fn", [P.viterbi, P.viterbi_fast])
def test_tie_rules_on_three_frames_and_four_states(fn):
    # w = 0: every transition between lags is free, so whole paths tie
    o = _small([[0.25, 0.25, 0.25]] * 3, w=0.0, fn=fn)
    assert o["lag"].tolist() == [2, 2, 2] and o["cost"] == 0.75              # voiced predecessors ascending: the first one stays
    # every voiced path costs 0.75 and so does U, U, U (u = 0.25): termination takes the voiced states first
    o = _small([[0.25, 0.25, 0.25]] * 3, w=0.0, u=0.25, fn=fn)
    assert o["lag"].tolist() == [2, 2, 2] and o["cost"] == 0.75
    # the last frame is cheapest at lag 4 only; its predecessors tie (0.5 each, U as well: 0.25 + 0.25 + c_sw 0): the first voiced
    o = _small([[0.25, 0.25, 0.25], [0.25, 0.25, 0.25], [0.5, 0.5, 0.125]], w=0.0, u=0.25, c_sw=0.0, fn=fn)
    assert o["lag"].tolist() == [2, 2, 4] and o["cost"] == 0.625
    # target U takes U first: with c_sw = 0, U's predecessors U (0.25) and lag 2 (0.25) tie in frame 1 and U stands; U is chosen in
    # the end because the voiced states are dearer there
    o = _small([[0.25, 0.5, 0.5], [0.75, 0.75, 0.75], [0.75, 0.75, 0.75]], w=0.0, u=0.25, c_sw=0.0, fn=fn)
    assert o["lag"].tolist() == [0, 0, 0] and o["cost"] == 0.75
    # a voiced target takes a voiced predecessor before U on a tie: frame 0 lag 2 (0.25) and U (0.25), c_sw = 0
    o = _small([[0.25, 0.5, 0.5], [0.125, 0.75, 0.75]], w=0.0, u=0.25, c_sw=0.0, fn=fn)
    assert o["lag"].tolist() == [2, 2] and o["cost"] == 0.375
    # max_jump: lag 2 -> 4 is a whole octave; with trans_max = 0.75 w it is not allowed and the path goes through U or stays
    o = _small([[0.0, 0.5, 0.5], [0.5, 0.5, 0.03125]], w=1.0, trans_max=0.75, u=0.125, c_sw=0.0625, fn=fn)
    assert o["lag"].tolist() == [2, 0] and o["cost"] == 0.0 + 0.0625 + 0.125
    o = _small([[0.0, 0.5, 0.5], [0.5, 0.5, 0.03125]], w=0.0625, trans_max=1.0, u=0.125, c_sw=0.0625, fn=fn)
    assert o["lag"].tolist() == [2, 4] and o["cost"] == 0.0625 + 0.03125      # allowed: one octave at 1/16 per octave


@pytest.mark.parametrize("fn", [P.viterbi, P.viterbi_fast])
def test_a_silent_frame_forces_the_unvoiced_state(fn):
    o = _small([[0.0, 0.5, 0.5]] * 4, power=[1, 1, 0, 1], fn=fn)
    assert o["lag"].tolist() == [2, 2, 0, 2] and o["aper"].tolist() == [0, 0, 1, 0] and o["f0"][2] == 0
    assert o["cost"] == 0.0 + 0.0 + (0.25 + 0.5) + 0.25
    o = _small([[0.0, 0.5, 0.5]] * 3, power=[0, 0, 0], fn=fn)                 # all silent
    assert o["lag"].tolist() == [0, 0, 0] and o["cost"] == 1.5
    o = _small([[0.0, 0.5, 0.5]] * 3, n=0, fn=fn)                             # nothing decoded
    assert o["lag"].tolist() == [0, 0, 0] and o["cost"] == 0.0 and o["aper"].tolist() == [1, 1, 1]
    o = _small([[0.0, 0.5, 0.5]] * 3, n=2, fn=fn)                             # frames behind len: f0 0, aper 1, lag 0
    assert o["lag"].tolist() == [2, 2, 0] and o["aper"].tolist() == [0, 0, 1]


def test_fast_restatement_equals_the_plain_one_on_random_inputs():
    rng = np.random.default_rng(3)
    for T, lo, hi, w in [(7, 5, 30, 1.0), (5, 4, 40, 0.0), (6, 10, 25, 0.3)]:
        cm = (rng.integers(0, 8, size=(T, hi + 1)) / 8.0).astype(np.float32) if w == 0.0 else rng.random((T, hi + 1)).astype(np.float32)
        pw = np.ones(T, np.float32)
        pw[T // 2] = 0
        args = (cm, pw, T, lo, hi, P.lag_weights(lo, hi, w), w * 0.25, 0.3, 0.15, 1e-10, 8000)
        a, b = P.viterbi(*args), P.viterbi_fast(*args)
        assert (a["lag"] == b["lag"]).all() and a["cost"] == b["cost"] and (a["f0_32"] == b["f0_32"]).all()


def test_path_statistics_of_a_hand_made_path():
    hop, S = 4, 4                                               # frame t valid iff 4 t - 2 >= 0 and 4 t + 2 <= n: t = 1 .. (n - 2) / 4
    f0_a = np.array([100, 100, 200, 0, 400, 100], np.float32)   # n_a = 22: frames 1 .. 5 valid
    f0_b = np.array([100, 200, 100, 0, 100], np.float32)        # n_b = 14: frames 1 .. 3 valid
    path = [(0, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (4, 3), (5, 4), (6, 3), (-1, 2), (1, 1)]
    row, mag = P.f0_path_stats(path, 10, f0_a, 22, f0_b, 14, hop, S)       # the last cell lies behind path_len
    # scored: (1,1) (2,1) (2,2) (3,2) (3,3) (4,3); both voiced: the first three; only a: (4,3); only b: (3,2); neither: (3,3)
    assert row[:4].tolist() == [6, 3, 1, 1]
    d = [-1200.0, 0.0, 1200.0]
    assert row[4] == sum(d) and row[5] == sum(x * x for x in d) and row[11] == 0
    la, lb = np.log2([100.0, 200.0, 200.0]), np.log2([200.0, 200.0, 100.0])
    assert np.allclose(row[6:11], [la.sum(), lb.sum(), (la * la).sum(), (lb * lb).sum(), (la * lb).sum()], rtol=1e-15)
    assert mag[4] == 2400.0 and mag[0] == 0
    fig = P.f0_figures(row)
    assert fig["n_pairs"] == 6 and fig["n_voiced_both"] == 3 and fig["vuv_error"] == 2 / 6 and fig["f0_bias_cents"] == 0
    assert abs(fig["f0_rmse_cents"] - 1200 * math.sqrt(2 / 3)) < 1e-9
    assert abs(fig["f0_corr"] - np.corrcoef(la, lb)[0, 1]) < 1e-12
    # undefined figures
    zero = P.f0_figures(np.zeros(12))
    assert zero == dict(n_pairs=0, n_voiced_both=0, f0_rmse_cents=None, f0_bias_cents=None, f0_corr=None, vuv_error=None)
    one, _ = P.f0_path_stats([(1, 1)], 1, f0_a, 22, f0_b, 14, hop, S)
    assert P.f0_figures(one)["f0_corr"] is None and P.f0_figures(one)["f0_rmse_cents"] == 1200.0
    flat, _ = P.f0_path_stats([(1, 1), (5, 1)], 2, f0_a, 22, f0_b, 14, hop, S)          # a constant column
    assert P.f0_figures(flat)["f0_corr"] is None and P.f0_figures(flat)["n_voiced_both"] == 2


def test_engine_f0_figures_equal_the_reference():
    from tacotron2_amd import engine
    rng = np.random.default_rng(2)
    for _ in range(5):
        fa, fb = rng.uniform(80, 400, 9).astype(np.float32), rng.uniform(80, 400, 9).astype(np.float32)
        fa[rng.integers(0, 9)] = 0
        row, _ = P.f0_path_stats([(i, i) for i in range(9)], 9, fa, 1000, fb, 1000, 1, 1)
        assert engine.f0_figures(row.tolist()) == pytest.approx(P.f0_figures(row), rel=1e-12)
    assert engine.f0_figures([0.0] * 12) == P.f0_figures(np.zeros(12))
    assert engine.VITERBI_DEFAULTS == P.DEFAULTS and engine.F0_NSTAT == P.F0_NSTAT


def test_cli_usage_errors():
    from click.testing import CliRunner
    import main as cli
    base = ["test", "--speech-dir", "s", "--checkpoint", "k.ckpt"]
    r = CliRunner().invoke(cli.main, base + ["--f0"], obj={})
    assert r.exit_code == 2 and "--f0 needs --score" in r.output
    r = CliRunner().invoke(cli.main, base + ["--score", "--no-audio", "--f0"], obj={})
    assert r.exit_code == 2 and "--no-audio" in r.output and "--f0" in r.output
    base = ["test-correlation", "--speech-dir", "s", "--checkpoint", "k.ckpt"]
    r = CliRunner().invoke(cli.main, base + ["--smooth-pitch"], obj={})
    assert r.exit_code == 2 and "--smooth-pitch needs --measure" in r.output
    assert "--f0" in CliRunner().invoke(cli.main, ["test", "--help"], obj={}).output
    assert "--smooth-pitch" in CliRunner().invoke(cli.main, ["test-correlation", "--help"], obj={}).output


def test_smooth_pitch_travels_in_the_model_config(monkeypatch):
    from click.testing import CliRunner
    import main as cli
    from tacotron2_amd.run import correlation as K
    from tacotron2_amd.run import test_correlation as tc
    seen, trees = [], []
    monkeypatch.setattr(tc, "do_test_correlation", lambda **kw: seen.append(kw))
    monkeypatch.setattr(K, "correlate_tree", lambda base, feats, yin: trees.append(yin))
    monkeypatch.setattr(cli, "load_config", lambda p: {"dataset": {}, "training": {"name": "tiny"}, "model": {"a": 1},
                                                       "extensions": {"controls": {"active": True, "features": ["rate", "nhr"]}}})
    base = ["--config", "c.json", "test-correlation", "--speech-dir", "s", "--checkpoint", "k.ckpt", "--measure"]
    assert CliRunner().invoke(cli.main, base, obj={}).exit_code == 0
    assert seen[0]["model_config"] == {"a": 1, "measure_prosody": True} and "smooth" not in trees[0]
    r = CliRunner().invoke(cli.main, base + ["--smooth-pitch"], obj={})
    assert r.exit_code == 0, (r.output, r.exception)
    assert seen[1]["model_config"] == {"a": 1, "measure_prosody": True, "smooth_pitch": True}
    assert trees[1]["smooth"] is True and trees[1]["w"] == 1.0 and trees[1]["max_jump"] == 0.25 and trees[1]["u"] == 0.3 \
        and trees[1]["c_sw"] == 0.15


def test_meter_description_without_smooth_is_what_it_was():
    from tacotron2_amd.prosody import ProsodyMeter
    assert ProsodyMeter(22050, "cuda:0").describe() == dict(sr=22050, hop=256, W=1024, fmin=60.0, fmax=500.0, thr=0.1, vthr=0.3,
                                                            power_floor=1e-10, tau_min=44, tau_max=367)
    d = ProsodyMeter(22050, "cuda:0", smooth=True, vthr=0.25, c_sw=0.2).describe()
    assert d["smooth"] is True and d["u"] == 0.25 and d["c_sw"] == 0.2 and d["w"] == 1.0 and d["max_jump"] == 0.25 and d["vthr"] == 0.25
    with pytest.raises(ValueError):
        ProsodyMeter(22050, "cuda:0", c_sw=0.2)               # a Viterbi setting without smooth
    with pytest.raises(ValueError):
        ProsodyMeter(22050, "cuda:0", smooth=True, window=3)


def test_f0_csv_layout(tmp_path):
    from tacotron2_amd.run import test as T
    assert "|".join(T.F0_HEADER) == "i|wav|stopped|n_pairs|n_voiced_both|f0_rmse_cents|f0_bias_cents|f0_corr|vuv_error"
    means = T.write_f0_scores(str(tmp_path), [
        dict(i=1, wav="a.wav", stopped=True, n_pairs=10, n_voiced_both=4, f0_rmse_cents=50.0, f0_bias_cents=-12.5, f0_corr=0.5, vuv_error=0.25),
        dict(i=2, wav="b.wav", stopped=False, n_pairs=0, n_voiced_both=0, f0_rmse_cents=None, f0_bias_cents=None, f0_corr=None, vuv_error=None),
        dict(i=3, wav="c.wav", stopped=True, n_pairs=3, n_voiced_both=1, f0_rmse_cents=150.0, f0_bias_cents=150.0, f0_corr=None, vuv_error=0.0)])
    lines = (tmp_path / "f0_scores.csv").read_text().splitlines()
    assert lines[1] == "1|a.wav|1|10|4|50.000000|-12.500000|0.500000|0.250000"
    assert lines[2] == "2|b.wav|0||||||" and lines[3] == "3|c.wav|1|3|1|150.000000|150.000000||0.000000"
    assert means == dict(f0_rmse_cents_mean=100.0, f0_bias_cents_mean=68.75, f0_corr_mean=0.5, vuv_error_mean=0.125)
