"""The float64 restatement of t2_char_variance (tests/variance_ref.py) on the CPU, the argument checks of analysis.char_variance that
need no device, the host arithmetic of the export's statistics and the usage errors `main.py duration-export` gained.

The hand-worked case: 3 characters, 7 frames, pitch in Hz (log_pitch off, so that the numbers can be read), 2 mel bins.
    f0  = [0, 100, 200, 0, 0, 0, 400] Hz          voiced frames: 1, 2, 6
    mel = [ln 3k, ln 4k] for k = 1 .. 7            e(t) = sqrt((3k)^2 + (4k)^2) = 5k = 5, 10, 15, 20, 25, 30, 35
    dur = [3, 2, 2]                                 spans: {0, 1, 2}, {3, 4}, {5, 6}; they sum to 7 = F: consistent
  interpolate off:  q = [0, 100, 200, 0, 0, 0, 400]
    pitch  = [(100 + 200) / 2, 0 (no voiced frame), 400 / 1] = [150, 0, 400]        voiced = [2, 0, 1]
  interpolate on:   u0 = 1, u1 = 6; frame 0 takes p(1); the gap 2 < t < 6 is 200 + 200 (t - 2) / 4
                    q = [100, 100, 200, 250, 300, 350, 400]
    pitch  = [400 / 3, 550 / 2, 750 / 2] = [133.33.., 275, 375]
  energy = [(5 + 10 + 15) / 3, (20 + 25) / 2, (30 + 35) / 2] = [10, 22.5, 32.5]     either way
  stats: F = 7, voiced = 3, sum p = 700, sum p^2 = 210000, sum e = 140, sum e^2 = 25 * 140 = 3500, 1 character unvoiced;
         sum q = 700, sum q^2 = 210000 without interpolation, 1700 and 495000 with it."""
import math
import os

import numpy as np
import pytest
import torch

import variance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0 = np.array([0, 100, 200, 0, 0, 0, 400], dtype=np.float32)
MEL = np.log(np.array([[3.0 * k, 4.0 * k] for k in range(1, 8)])).astype(np.float32)
DUR = [3, 2, 2]
E_TOL = 1e-6          # the float32 rounding of ln(3k): a relative 6e-8 * ln(28) on the exponent, so 2e-7 on e


def test_the_hand_worked_case():
    o = R.char_variance(DUR, 3, 7, F0, MEL, log_pitch=False, interpolate=False)
    assert o["pitch"].tolist() == [150.0, 0.0, 400.0] and o["voiced"].tolist() == [2, 0, 1]
    assert o["q"].tolist() == [0, 100, 200, 0, 0, 0, 400]
    np.testing.assert_allclose(o["e"], [5, 10, 15, 20, 25, 30, 35], rtol=E_TOL)
    np.testing.assert_allclose(o["energy"], [10, 22.5, 32.5], rtol=E_TOL)
    assert o["stats"][[0, 1, 2, 3, 4, 5, 8, 9]].tolist() == [7, 3, 700, 210000, 700, 210000, 1, 1]
    np.testing.assert_allclose(o["stats"][[6, 7]], [140, 3500], rtol=2 * E_TOL)
    i = R.char_variance(DUR, 3, 7, F0, MEL, log_pitch=False, interpolate=True)
    assert i["q"].tolist() == [100, 100, 200, 250, 300, 350, 400]
    np.testing.assert_allclose(i["pitch"], [400 / 3, 275, 375], rtol=1e-15)
    assert i["voiced"].tolist() == [2, 0, 1] and i["stats"][[1, 2, 3, 4, 5, 9]].tolist() == [3, 700, 210000, 1700, 495000, 1]
    np.testing.assert_array_equal(i["energy"], o["energy"])
    # the log domain: the same frames, ln of the same values
    lg = R.char_variance(DUR, 3, 7, F0, MEL, log_pitch=True, interpolate=False)
    np.testing.assert_allclose(lg["pitch"], [(math.log(100) + math.log(200)) / 2, 0, math.log(400)], rtol=1e-15)


def test_the_edges_of_the_rule():
    # durations that do not sum to F: the spans are clipped, consistent is 0; a negative duration counts as 0
    short = R.char_variance([3, 2, 1], 3, 7, F0, MEL, log_pitch=False)
    assert short["stats"][8] == 0 and short["voiced"].tolist() == [2, 0, 0] and short["pitch"].tolist() == [150, 0, 0]
    over = R.char_variance([3, -4, 9], 3, 7, F0, MEL, log_pitch=False)
    assert over["stats"][8] == 0 and over["voiced"].tolist() == [2, 0, 1] and over["energy"][1] == 0
    np.testing.assert_allclose(over["energy"][2], (20 + 25 + 30 + 35) / 4, rtol=E_TOL)
    # no characters or no frames: zeros, consistent apart; a NaN and a negative value are unvoiced
    for n, f, dur, c in ((0, 7, DUR, 0.0), (3, 0, DUR, 0.0), (0, 0, DUR, 1.0), (3, 0, [0, 0, 0], 1.0)):
        z = R.char_variance(dur, n, f, F0, MEL)
        assert not z["pitch"].any() and not z["energy"].any() and not z["voiced"].any()
        assert z["stats"][8] == c and not np.delete(z["stats"], 8).any()
    odd = np.array([np.nan, -5, 100, np.nan], dtype=np.float32)
    q, v = R.frame_pitch(odd, 4, log_pitch=False, interpolate=True)
    assert v.tolist() == [False, False, True, False] and q.tolist() == [100, 100, 100, 100]
    # no voiced frame: q is 0 everywhere, with and without interpolation
    assert not R.frame_pitch(np.zeros(5, np.float32), 5, interpolate=True)[0].any()
    # the characters behind N and the frames behind F are never read
    f0 = np.concatenate([F0, np.full(3, 1000, np.float32)])
    mel = np.concatenate([MEL, np.full((3, 2), np.nan, np.float32)])
    o = R.char_variance(DUR + [10 ** 9], 3, 7, f0, mel, log_pitch=False)
    assert o["pitch"].tolist() == [150, 0, 400, 0] and o["stats"][1] == 3 and np.isfinite(o["stats"]).all()


@pytest.mark.parametrize("seed", range(4))
def test_interpolation_is_np_interp_with_the_end_values_held(seed):
    rng = np.random.default_rng(seed)
    F = 300
    f0 = np.where(rng.random(F) < 0.3, rng.uniform(60, 500, F), 0).astype(np.float32)
    f0[:5] = 0
    f0[-9:] = 0
    for log_pitch in (True, False):
        q, v = R.frame_pitch(f0, F, log_pitch, True)
        idx = np.nonzero(v)[0]
        p = np.log(f0[idx].astype(np.float64)) if log_pitch else f0[idx].astype(np.float64)
        np.testing.assert_allclose(q, np.interp(np.arange(F), idx, p), rtol=1e-12)
        assert (q[:idx[0]] == p[0]).all() and (q[idx[-1]:] == p[-1]).all()


@pytest.mark.parametrize("seed", range(4))
def test_durations_times_energy_is_the_energy_sum(seed):
    rng = np.random.default_rng(seed)
    N, F, M = 23, 181, 80
    cuts = np.sort(rng.integers(0, F + 1, N - 1))
    dur = np.diff(np.concatenate([[0], cuts, [F]])).astype(np.int32)          # zeros included
    mel = rng.normal(-4, 2, (F, M)).astype(np.float32)
    f0 = rng.uniform(60, 500, F).astype(np.float32)
    o = R.char_variance(dur, N, F, f0, mel)
    assert o["stats"][8] == 1
    total = math.fsum(float(d) * float(x) for d, x in zip(dur, o["energy"]))
    assert abs(total - o["stats"][6]) <= 1e-12 * o["stats"][6]
    assert abs(math.fsum(o["e"]) - o["stats"][6]) == 0


def _ok():
    return (torch.ones(2, 5, dtype=torch.int32), torch.tensor([5, 3]), torch.tensor([7, 4]), torch.zeros(2, 7), torch.zeros(2, 7, 80))


def test_char_variance_refuses_what_the_kernel_cannot_take():
    from tacotron2_amd import analysis, variance
    assert analysis.char_variance is variance.char_variance
    assert (analysis.VAR_MAX_T, analysis.VAR_MAX_L, analysis.VAR_NSTAT, len(analysis.VAR_STATS)) == (4096, 4096, 10, 10)
    dur, cl, fl, f0, mel = _ok()
    for bad, word in (((dur, cl, fl, f0.numpy(), mel), "f0 must be a float32"),
                      ((dur, cl, fl, f0.double(), mel), "f0 must be a float32"),
                      ((dur, cl, fl, f0[0], mel), "f0 must be a float32"),
                      ((dur, cl, fl, f0, mel.half()), "mel must be a float32"),
                      ((dur, cl, fl, f0, mel[0]), "mel must be a float32"),
                      ((dur.long(), cl, fl, f0, mel), "dur must be a int32"),
                      ((dur, cl, fl, torch.zeros(2, 4097), torch.zeros(2, 4097, 1)), "T2_VAR_MAX_T"),
                      ((dur, cl, fl, torch.zeros(2, 0), torch.zeros(2, 0, 80)), "T2_VAR_MAX_T"),
                      ((dur, cl, fl, f0, mel[:, :6]), "mel of shape"),
                      ((dur, cl, fl, f0, mel[:1]), "mel of shape"),
                      ((dur, cl, fl, f0, mel[:, :, :0]), "mel of shape"),
                      ((torch.ones(2, 4097, dtype=torch.int32), cl, fl, f0, mel), "T2_VAR_MAX_L"),
                      ((dur[:1], cl, fl, f0, mel), "dur of shape"),
                      ((dur, cl, fl, torch.zeros(7, 2).t(), mel), "last dimension of f0"),
                      ((torch.ones(5, 2, dtype=torch.int32).t(), cl, fl, f0, mel), "last dimension of dur"),
                      ((dur, cl, fl, f0, torch.zeros(2, 80, 7).transpose(1, 2)), "last dimension of mel"),
                      ((dur, cl, fl, f0, torch.zeros(7, 2, 80).transpose(0, 1)[:, :, :]), "overlapping rows of mel"),
                      ((dur, cl, fl, f0.expand(2, 7)[:1].expand(2, 7), mel), "overlapping rows of f0"),
                      ((dur, cl, fl, f0, mel), "f0 must be on the GPU")):          # (everything else in order: only the device is wrong)
        with pytest.raises(ValueError) as e:
            analysis.char_variance(*bad)
        assert str(e.value).startswith("char_variance: ") and word in str(e.value), (word, str(e.value))


def test_the_statistics_arithmetic_of_the_export():
    from tacotron2_amd.run.duration_export import mean_std, moments
    from tacotron2_amd.variance import pooled
    assert mean_std(0, 0.0, 0.0) == ("", "") and mean_std(4, 10.0, 30.0) == ("2.500000", f"{math.sqrt(7.5 - 6.25):.6f}")
    a, b = np.array([1, 2, 3], np.float32), np.array([5, 7], np.float32)
    rows = [moments(a), moments(b), moments(a[:0])]
    assert rows[0] == [3, 6.0, 14.0, 1.0, 3.0] and rows[2][0] == 0
    p = pooled(rows)
    both = np.concatenate([a, b]).astype(np.float64)
    assert p["count"] == 5 and p["min"] == 1.0 and p["max"] == 7.0
    assert abs(p["mean"] - both.mean()) < 1e-15 and abs(p["std"] - both.std()) < 1e-14
    assert pooled([moments(a[:0])]) == dict(count=0, mean=None, std=None, min=None, max=None)


def _cli(monkeypatch, tmp_path):
    import main as cli
    import tacotron2_amd.run.duration_export as de
    seen = {}
    monkeypatch.setattr(de, "do_duration_export", lambda **kw: seen.update(kw))
    cfg = tmp_path / "c.json"
    cfg.write_text('{"dataset": {}, "training": {}, "model": {}, "extensions": {}}')
    monkeypatch.setattr(cli, "load_config", lambda p: {"dataset": {}, "training": {}, "model": {}, "extensions": {}})
    return cli, ["--config", str(cfg), "duration-export", "--speech-dir", "s", "--checkpoint", "k"], seen


@pytest.mark.parametrize("flag", [["--pitch-domain", "hz"], ["--pitch-domain", "log"], ["--interpolate-pitch"], ["--frame-level"],
                                  ["--no-smooth-pitch"]])
def test_cli_variance_sub_options_need_variances(monkeypatch, tmp_path, flag):
    from click.testing import CliRunner
    cli, args, seen = _cli(monkeypatch, tmp_path)
    r = CliRunner().invoke(cli.main, args + flag, obj={})
    assert r.exit_code == 2 and flag[0] in r.output and "--variances" in r.output, r.output
    assert not seen


def test_cli_variance_options_reach_the_driver(monkeypatch, tmp_path):
    from click.testing import CliRunner
    cli, args, seen = _cli(monkeypatch, tmp_path)
    r = CliRunner().invoke(cli.main, args, obj={})
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert (seen["variances"], seen["pitch_domain"], seen["interpolate_pitch"], seen["frame_level"], seen["smooth_pitch"]) == \
        (False, "log", False, False, True) and seen["mode"] == "monotonic"
    seen.clear()
    r = CliRunner().invoke(cli.main, args + ["--variances", "--pitch-domain", "hz", "--interpolate-pitch", "--frame-level",
                                            "--no-smooth-pitch", "--mode", "argmax"], obj={})
    assert r.exit_code == 0, r.output + repr(r.exception)
    assert (seen["variances"], seen["pitch_domain"], seen["interpolate_pitch"], seen["frame_level"], seen["smooth_pitch"]) == \
        (True, "hz", True, True, False) and seen["mode"] == "argmax"
    seen.clear()
    r = CliRunner().invoke(cli.main, args + ["--variances", "--pitch-domain", "mel"], obj={})
    assert r.exit_code == 2 and "pitch-domain" in r.output and not seen
    assert "--variances" in CliRunner().invoke(cli.main, ["duration-export", "--help"], obj={}).output
