"""The numpy restatement of t2_stretch (tests/stretch_ref.py) on the CPU: lengths, silence, the tie rule, the int32 bound,
what a stretched tone keeps, the pitch path through tests/resample_ref.py, and every argument rejection of analysis.time_stretch /
analysis.pitch_shift that needs no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_ref as RS
import stretch_ref as R

SR = 22050


def test_lengths_and_frame_counts():
    want = {0: (0, 0), 1: (2, 1), 7: (14, 6), 8: (16, 7), 17: (34, 14), 997: (1994, 798)}       # n: n_out at P = 500 | 1250
    for n, outs in want.items():
        for P, n_out in zip((500, 1250), outs):
            got, M = R.lengths(n, P, 1000, 16)
            assert got == n_out and M == -(-n_out // 8) + 1, (n, P, got, M)
            y, pos = R.stretch(np.random.default_rng(n).standard_normal(n).astype(np.float32), P, 1000, 16, 4)
            assert len(y) == n_out and len(pos) == M
            a = np.array(R.centres(M, P, 1000, 16))
            assert pos[0] == 0 and (np.abs(pos - a) <= 4).all()
    assert R.lengths(0, 500, 1000, 16) == (0, 1)                       # (an empty row still has frame 0)
    assert R.centres(4, 1250, 1000, 16) == [0, 10, 20, 30] and R.centres(3, 1001, 1000, 16) == [0, 8, 16]
    assert R.centres(3, 3, 2, 4) == [0, 3, 6] and R.centres(2, 1, 3, 4) == [0, 1]      # (2 * 1 + 1) div 3 = 1: rounded half up


def test_window_sums_to_one():
    for N in (4, 16, 1024, 2048):
        w = R.window(N).astype(np.float64)
        assert w.dtype == np.float64 and np.abs(w[:N // 2] + w[N // 2:] - 1.0).max() < 2.0 ** -23
    from tacotron2_amd.stretch import hann_table
    assert np.array_equal(hann_table(1024), R.window(1024))


def test_silence_keeps_every_offset_at_zero():
    for P in (500, 1250):
        y, pos = R.stretch(np.zeros(3000, np.float32), P, 1000, 64, 16)
        assert np.array_equal(pos, np.array(R.centres(len(pos), P, 1000, 64))) and not y.any()


def test_tie_rule_on_a_constant_row():
    assert R.pick(np.array([5, 7, 7, 7, 1]), 2) == 0                  # smaller |d| first
    assert R.pick(np.array([7, 1, 1, 1, 7]), 2) == -2                 # then the negative one
    assert R.pick(np.array([1, 7, 1, 7, 1]), 2) == -1
    assert R.pick(np.array([1, 1, 1, 7, 1]), 2) == 1
    # a constant row: where template and region lie inside the row every offset scores the same, and 0 wins; where the region lies
    # behind the row every score is 0, and 0 wins again
    x = np.ones(3000, np.float32)
    N, D, P = 64, 16, 800
    y, pos = R.stretch(x, P, 1000, N, D)
    a = np.array(R.centres(len(pos), P, 1000, N))
    delta = pos - a
    inside = (a - N // 2 - D >= 0) & (a + N // 2 + D <= len(x)) & (np.concatenate([[0], pos[:-1]]) + N <= len(x))
    assert inside.sum() > 50 and not delta[inside].any()
    assert (delta[a - N // 2 - D > len(x)] == 0).all()                # nothing left to correlate with: all scores 0
    assert np.abs(y[N:2000] - 1.0).max() < 2.0 ** -22


def test_int32_bound_at_the_largest_window():
    N = 2048
    assert 1023 * 1023 * N < 2 ** 31
    x = np.where((np.arange(3 * N) // 64) % 2 == 0, 1.0, -1.0).astype(np.float32)        # a full-scale square wave
    assert np.abs(R.quantise(x)).max() == 1023 and np.abs(R.quantise(0.37 * x)).min() == 1023
    pos, top = R.positions(x, 1000, 1000, N, 128, return_scores=True)
    assert top == 1023 * 1023 * N                                     # the bound is met, and it fits
    assert top < 2 ** 31


def test_quantise_is_fp64_rint():
    x = np.array([0.5, -0.25, 1.0, 3.0, -3.0, 1e-4], np.float32)
    assert R.quantise(x).tolist() == [int(np.rint(float(v) * 1023.0 / 3.0)) for v in x]
    assert R.quantise(np.array([1.5, 3.0], np.float32)).tolist() == [512, 1023]          # 511.5 goes to the even neighbour
    assert R.quantise(np.zeros(0, np.float32)).tolist() == []


@pytest.fixture(scope="module")
def tone220():
    return R.tone(220.0, SR)


@pytest.mark.parametrize("P", [500, 800, 1250, 2000])
def test_a_stretched_tone_keeps_pitch_and_level(tone220, P):
    y, pos = R.stretch(tone220, P)
    assert len(y) == R.cdiv(len(tone220) * 1000, P)
    peak, width = R.spectral_peak(y, SR)
    assert abs(peak - 220.0) <= width, (P, peak, width)
    mid = slice(len(y) // 8, len(y) - len(y) // 8)
    rms = np.sqrt(np.mean(y[mid] ** 2)) / np.sqrt(np.mean(tone220.astype(np.float64) ** 2))
    assert abs(rms - 1.0) <= 0.02, (P, rms)


@pytest.mark.parametrize("semitones", [12, 3])
def test_pitch_path_on_the_references(tone220, semitones):
    from tacotron2_amd.stretch import pitch_plan
    sr_mid, eff, (P, Q) = pitch_plan("pitch_shift", semitones, SR)
    f = 2.0 ** (semitones / 12.0)
    assert sr_mid % 50 == 0 and abs(sr_mid - SR * f) <= 25 and Q == 1000 and P == round(1000 * SR / sr_mid)
    y, _ = R.stretch(tone220, P, Q)
    U, D, K, table = RS.design(sr_mid, SR)
    assert U <= 441
    z, _ = RS.apply(y, table, U, D, K)
    peak, width = R.spectral_peak(z, SR)
    assert abs(peak - 220.0 * f) <= width + 1e-3 * 220.0 * f, (peak, 220.0 * f, width)
    assert abs(len(z) - len(tone220) / eff) <= 2e-3 * len(tone220) / eff
    assert abs(eff - 1.0) < 1e-3


def test_pitch_plan_figures():
    from tacotron2_amd.stretch import pitch_plan
    assert pitch_plan("f", 0, SR) == (SR, 1.0, (1000, 1000))
    assert pitch_plan("f", 12, SR) == (44100, 1.0, (500, 1000))
    sr_mid, eff, ratio = pitch_plan("f", -12, SR, 0.8)
    assert (sr_mid, ratio) == (11000, (1604, 1000)) and abs(eff - 0.8) < 1e-3
    for sr in (SR, 44100):                                            # the pitch error of the rounding to 50 Hz: 25 Hz of sr_mid
        for st in range(-24, 25):
            sr_mid, _, _ = pitch_plan("f", st, sr)
            want = sr * 2.0 ** (st / 12.0)
            cents = abs(1200 * np.log2(sr_mid / want))
            assert abs(sr_mid - want) <= 25 and cents <= 1200 * np.log2(1 + 25 / (want - 25)) * (1 + 1e-9) and (cents <= 2.0 or want < 21700)


def _raises(match, fn, *a, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*a, **kw)


def test_time_stretch_rejections():
    from tacotron2_amd import analysis, engine
    ts = analysis.time_stretch
    assert engine.time_stretch is ts and engine.pitch_shift is analysis.pitch_shift
    x = torch.zeros(2, 100)
    _raises("wav must be a float32", ts, np.zeros((2, 100), np.float32), [1, 2], 0.8)
    _raises("wav must be a float32", ts, torch.zeros(100), [1], 0.8)
    _raises("wav must be a float32", ts, x.double(), [1, 2], 0.8)
    for tempo in (0.2, 4.5, float("nan"), float("inf"), "fast", True, None, (1, 5), (5, 1), (0, 1), (1, 0), (1.0, 2), (1, 2, 3),
                  (1 << 21, 1 << 21)):
        _raises("tempo", ts, x, [1, 2], tempo)
    for frame in (2, 3, 1023, 2050, 1024.0, True):
        _raises("frame", ts, x, [1, 2], 0.8, frame=frame)
    for tol in (-1, 1025, 2.0, False):
        _raises("tolerance", ts, x, [1, 2], 0.8, tolerance=tol)
    _raises("batch of 0", ts, torch.zeros(0, 100), [], 0.8)
    _raises("contiguous", ts, torch.zeros(2, 200)[:, ::2], [1, 2], 0.8)
    _raises("overlapping rows", ts, torch.zeros(200).as_strided((2, 100), (50, 1)), [1, 2], 0.8)
    _raises("n must be 2 integers", ts, x, [1], 0.8)
    _raises("n must be 2 integers", ts, x, [1.0, 2.0], 0.8)
    _raises("n must lie in 0 .. 100", ts, x, [1, 101], 0.8)
    _raises("n must lie in 0 .. 100", ts, x, [-1, 5], 0.8)
    _raises("must be on the GPU", ts, x, [1, 2], 0.8)
    _raises("must be on the GPU", ts, x, [1, 2], 1.0)                 # (the bypass takes the same arguments)


def test_pitch_shift_rejections():
    from tacotron2_amd import analysis
    ps = analysis.pitch_shift
    x = torch.zeros(2, 100)
    for st in (-24.5, 25, float("nan"), "up", True, None):
        _raises("semitones", ps, x, [1, 2], st, SR)
    for sr in (0, 999, 22050.0, True, None):
        _raises("sample_rate", ps, x, [1, 2], 3, sr)
    for tempo in (0.2, 4.5, float("nan"), "slow"):
        _raises("tempo", ps, x, [1, 2], 3, SR, tempo)
    _raises("need a stretch by", ps, x, [1, 2], 24, SR, 0.4)          # 0.4 / 4 = 0.1 < 1/8
    _raises("need a stretch by", ps, x, [1, 2], -24, SR, 2.5)         # 2.5 * 4 = 10 > 8
    _raises("frame", ps, x, [1, 2], 3, SR, frame=1023)
    _raises("tolerance", ps, x, [1, 2], 3, SR, tolerance=-1)
    _raises("wav must be a float32", ps, x.double(), [1, 2], 3, SR)
    _raises("n must lie in", ps, x, [1, 101], 3, SR)
    _raises("must be on the GPU", ps, x, [1, 2], 3, SR)


@pytest.mark.parametrize("rate", [22050, 16000, 24000, 44100, 48000])
def test_every_corner_of_say_s_ranges_passes_the_checks_the_driver_runs(rate):
    """voice_settings accepts a combination before anything is decoded; apply_voice must then not refuse it.  On a CPU tensor the
    calls apply_voice makes run every argument check and stop at the last one, the device."""
    from tacotron2_amd.run.say import apply_voice, voice_settings
    from tacotron2_amd.stretch import pitch_plan
    x = torch.zeros(2, 3000)
    for tempo in (0.5, 0.501, 1.0, 1.999, 2.0, None):
        for semitones in (-12, -11.9, -1, 0, 0.01, 5, 12, None):
            voice = voice_settings(tempo, semitones, rate)
            if voice is None:
                assert tempo is None and semitones is None and apply_voice(x, [1, 2], voice)[0] is x
                continue
            assert abs(voice.tempo - (tempo or 1.0)) <= 2.1e-3 * (tempo or 1.0) and 125 <= voice.ratio[0] <= 8000
            if semitones:
                assert (voice.sr_mid, voice.tempo, voice.ratio) == pitch_plan("pitch_shift", semitones, rate, tempo or 1.0)
            if not voice.active:
                assert apply_voice(x, [1, 2], voice)[0] is x
            else:
                _raises("wav must be on the GPU", apply_voice, x, [3000, 2], voice)
    # the corner the 50 Hz and 1/1000 roundings push past 4: the stretch of a pitch shift may run at up to 8
    assert voice_settings(2.0, -12, 22050).ratio == (4009, 1000) and voice_settings(0.5, 12, 22050).ratio == (250, 1000)
    for tempo, semitones, name in ((2.01, 0, "--tempo"), (0.49, None, "--tempo"), (1, 12.01, "--pitch-shift"), (None, -12.5, "--pitch-shift")):
        _raises(name, voice_settings, tempo, semitones, rate)
    _raises("need a .wav target", voice_settings, 1.0, None, rate, False)


def test_integration_md_stub_mirrors_the_header():
    import os
    import re
    md = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    block = md[md.index("class T2Stretch(C.Structure)"):]
    block = block[:block.index("]\n") + 1]
    from tacotron2_amd import _lib
    assert re.findall(r'\("(\w+)",\s*C\.', block) == [f[0] for f in _lib._structs["T2Stretch"]]
    assert "`t2_stretch(const T2Stretch*, stream)`" in md


def test_abi_has_the_entry():
    from tacotron2_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    assert "t2_stretch" in _lib.DECLARED_SYMBOLS and hasattr(lib, "t2_stretch")
    assert lib.t2_sizeof(b"T2Stretch") == C.sizeof(_lib.S["T2Stretch"]) > 0
    assert [f[0] for f in _lib._structs["T2Stretch"]] == ["x", "ldx", "n", "w", "B", "n_max", "N", "D", "P", "Q", "y", "ldy", "pos",
                                                          "ldp", "n_out"]
