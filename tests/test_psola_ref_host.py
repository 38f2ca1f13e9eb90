"""tests/psola_ref.py itself, the numpy restatement of t2_psola, and the argument checks of tacotron2_amd/psola.py and of
`say`'s settings: no GPU.  The GPU tests compare the kernel with this reference mark by mark; these pin what the reference does -
identity, the pitch it produces, the formants it keeps, the tie rule - on the synthetic vowels of DESIGN 5.18."""
import numpy as np
import pytest

import psola_ref as R

SR = 22050
SHIFTS = (4, -4, 7, -7, 12, -12)


def _q(semitones):
    return int(round(R.ONE * 2.0 ** (-semitones / 12.0)))


@pytest.fixture(scope="module")
def vowels():
    return {v: R.vowel(*v) for v in R.VOWELS}


@pytest.mark.parametrize("v", R.VOWELS)
def test_rho_one_is_the_identity(vowels, v):
    x = vowels[v]
    y, a, r, km, G = R.psola(x, np.full(1 + len(x) // 256, v[0]))
    assert np.array_equal(r, a) and np.array_equal(km, np.arange(len(a))) and G == 2
    assert np.abs(y - x).max() <= 4 * 2.0 ** -24 * np.abs(x).max()
    assert a[0] == 0 and a[-1] == len(x) and np.all(np.diff(a)[:-1] >= 12) and np.all(np.diff(a) <= 5120)


@pytest.mark.parametrize("v", R.VOWELS)
def test_the_pitch_moves_and_the_formant_stays(vowels, v):
    x = vowels[v]
    lag = np.full(1 + len(x) // 256, v[0])
    c0 = R.centroid(x)
    for st in SHIFTS:
        q = _q(st)
        y, a, r, km, G = R.psola(x, lag, q)
        f0, width = R.fundamental(y)
        want = SR / (v[0] * q / R.ONE)
        assert abs(f0 - want) <= width, (v, st, f0, want)
        moved = R.resampled(R.vowel(*v, n=int(len(x) * R.ONE / q) + 200), q / R.ONE)          # the same shift by resampling
        f0r, _ = R.fundamental(moved)
        assert abs(f0r - want) <= width                                                    # (the yardstick does shift the pitch)
        share = abs(R.centroid(y) - c0) / abs(R.centroid(moved) - c0)
        assert share <= 0.25, (v, st, share)
        rms = np.sqrt((y ** 2).mean() / (x.astype(np.float64) ** 2).mean())
        assert 0.6 <= rms <= 1.0, (v, st, rms)                                             # the level drop the README states


def test_ties_go_to_the_first_maximum():
    n = 4000
    lag = np.full(1 + n // 256, 80)
    a = R.analysis_marks(np.zeros(n, np.float32), lag)
    assert np.array_equal(a[:-1], 60 * np.arange(len(a) - 1)) and a[-1] == n and a[-2] + 80 >= n
    plateau = np.zeros(n, np.float32)
    plateau[500:3000] = 0.5
    a = R.analysis_marks(plateau, lag)
    for k in range(len(a) - 2):
        c = a[k] + 80
        lo, hi = c - 20, min(c + 20, n - 1)
        assert a[k + 1] == lo + int(np.argmax(plateau[lo:hi + 1])) and np.all(plateau[lo:a[k + 1]] < plateau[a[k + 1]])
    y, a0, r, km, G = R.psola(np.zeros(n, np.float32), lag, _q(4))
    assert not y.any() and r[-1] == n and km[-1] == len(a0) - 1
    # a synthesis mark midway between two analysis marks copies the earlier one
    r2, km2 = R.synthesis_marks(np.array([0, 100, 200, 300]), np.full(2, 100), 32768)
    assert r2.tolist() == [0, 50, 100, 150, 200, 250, 300] and km2.tolist() == [0, 0, 1, 1, 2, 2, 3]


def test_edge_rows_and_unvoiced_spacing():
    for n in (0, 1, 127, 128, 129):
        x = np.linspace(0.1, 0.2, n).astype(np.float32)
        y, a, r, km, G = R.psola(x, np.zeros(1 + n // 256, np.int64), _q(4))
        assert a.tolist() == ([0, n] if n <= 128 else [0, 128, n]) and np.array_equal(r, a)      # rho is 1 where nothing is voiced
        assert np.abs(y - x).max(initial=0.0) <= 4 * 2.0 ** -24 * 0.2
    x = R.vowel(147, 900.0, 250.0, n=6000)
    lag = np.where(np.arange(1 + 6000 // 256) % 2 == 0, 0, 367)
    a = R.analysis_marks(x, lag, U=64)
    for k in range(len(a) - 2):                                                            # d = min(per(c), step) / 4
        step = int(lag[R.frame(a[k], 256, len(lag))]) or 64
        pc = int(lag[R.frame(a[k] + step, 256, len(lag))])
        assert abs(a[k + 1] - (a[k] + step)) <= (min(pc, step) // 4 if pc else 0)
    assert R.accepted(10, 10, [100], 65536, 256) and not R.accepted(11, 10, [100], 65536, 256)
    assert not R.accepted(10, 10, [5], 65536, 256) and not R.accepted(10, 10, [100], 1000, 256) and R.accepted(10, 10, [0], 1000, 256)


def test_pitch_ratio_reference():
    lag = np.array([0, 100, 200, 0, 50, 100])
    assert np.array_equal(R.pitch_ratio(lag, 6 * 256, 12.0), [R.ONE, 32768, 32768, R.ONE, 32768, 32768])
    short = R.pitch_ratio(lag, 2 * 256, 0.0, 0.0)                                          # three frames count: lags 100 and 200
    assert np.all(short[3:] == R.ONE) and short[0] == R.ONE and abs(short[1] / R.ONE * 100 - 100 * 2 ** 0.5) < 0.01
    flat = R.pitch_ratio(lag, 6 * 256, 0.0, 0.0)                                           # a monotone voice: every period the geometric mean
    voiced = lag > 0
    assert np.abs(flat[voiced] / R.ONE * lag[voiced] - 100.0).max() < 0.01 and np.all(flat[~voiced] == R.ONE)
    wide = R.pitch_ratio(lag, 6 * 256, 0.0, 2.0)
    assert np.abs(wide[voiced] / R.ONE * lag[voiced] - np.array([100.0, 400.0, 25.0, 100.0])).max() < 0.01
    assert R.pitch_ratio(np.array([44, 367, 367, 367]), 4 * 256, 0.0, 2.0).max() <= R.RHO_RANGE[1]


def test_fold_lags_takes_the_smallest_sub_multiple_under_the_threshold():
    import torch
    from tacotron2_amd import analysis
    cm = np.full((1, 6, 368), 0.5, np.float32)
    cm[0, :, 100], cm[0, :, 200], cm[0, :, 300] = 0.01, 0.02, 0.005                       # a steady voice: every multiple is good
    cm[0, 3, 100] = 0.2                                                                   # ... but for one frame
    cm[0, 4, 99], cm[0, 4, 101] = 0.01, 0.01                                              # equal minima: the first
    cm[0, 4, 100] = 0.01
    lag = np.array([[100, 200, 300, 200, 299, 0]], np.int32)
    want = R.fold_lags(cm[0], lag[0], 44, 0.1)
    assert want.tolist() == [100, 100, 100, 200, 99, 0]
    got = analysis.fold_lags(torch.from_numpy(cm), torch.from_numpy(lag), 44, 0.1)
    assert got.dtype == torch.int32 and got[0].tolist() == want.tolist()
    assert R.fold_lags(cm[0], [87, 88], 44, 0.1).tolist() == [87, 88]                     # 44 is tried, 43 is not; nothing under thr
    rng = np.random.default_rng(0)
    cm = rng.uniform(0.0, 0.4, size=(2, 40, 368)).astype(np.float32)
    lag = rng.integers(44, 367, size=(2, 40)).astype(np.int32)
    got = analysis.fold_lags(torch.from_numpy(cm), torch.from_numpy(lag), 44, 0.1).numpy()
    assert np.array_equal(got, np.stack([R.fold_lags(cm[b], lag[b], 44, 0.1) for b in range(2)]))
    for args, msg in (((torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32), 44), "cmnd must be"),
                      ((torch.zeros(2, 3, 368), torch.zeros(2, 4, dtype=torch.int32), 44), "lag must be"),
                      ((torch.zeros(2, 3, 368), torch.zeros(2, 3, dtype=torch.int32), 1), "tau_min must be")):
        with pytest.raises(ValueError, match=msg):
            analysis.fold_lags(*args)


def test_tables_match_the_package():
    from tacotron2_amd.psola import LAG_RANGE, RHO_ONE, RHO_RANGE, grain_table
    W = grain_table()
    assert np.array_equal(W.view(np.uint32), R.table().view(np.uint32)) and W.dtype == np.float32 and W.shape == (1025,)
    assert W[0] == 0.0 and W[1024] == 1.0 and W[512] == 0.5 and np.abs(W + W[::-1] - 1.0).max() <= 2.0 ** -23
    assert (LAG_RANGE, RHO_ONE, RHO_RANGE) == (R.LAG_RANGE, R.ONE, R.RHO_RANGE)


def test_argument_rejections_of_the_python_layer():
    import torch
    from tacotron2_amd import analysis, engine, psola
    assert engine.psola is analysis.psola is psola.psola and engine.pitch_shift_psola is psola.pitch_shift_psola
    assert engine.pitch_ratio is psola.pitch_ratio
    wav, lag = torch.zeros(2, 1000), torch.zeros(2, 4, dtype=torch.int32)
    bad = [((wav[0], [1000, 1000], lag, 65536), "wav must be a float32"), ((wav.double(), [1000, 1000], lag, 65536), "wav must be a float32"),
           ((wav[:, ::2], [500, 500], lag, 65536), "last dimension of wav"), ((wav, [1000, 1001], lag, 65536), "n must lie in"),
           ((wav, [1000], lag, 65536), "n must be 2 integers"), ((wav, [1000, 1000], lag, 65536), "wav must be on the GPU")]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            psola.psola(*args)
    for kw, msg in ((dict(hop=8), "hop must be"), (dict(unvoiced=8), "unvoiced must be"), (dict(unvoiced=5000), "unvoiced must be")):
        with pytest.raises(ValueError, match=msg):
            psola.psola(wav, [1000, 1000], lag, 65536, **kw)
    for args, msg in (((lag.long(), [10, 10]), "lag must be a int32"), ((lag, [10, 10], 25.0), "semitones must lie"),
                      ((lag, [10, 10], 0.0, 2.5), "pitch_range must lie"), ((lag, [10, 10], float("nan")), "semitones must be a finite"),
                      ((lag, [10, 10]), "lag must be on the GPU")):
        with pytest.raises(ValueError, match=msg):
            psola.pitch_ratio(*args)
    for args, kw, msg in (((wav, [1000, 1000], 30.0, 22050), {}, "semitones must lie"), ((wav, [1000, 1000], 2.0, 22050), dict(pitch_range=-0.1), "pitch_range must lie"),
                          ((wav, [1000, 1000], 2.0, 22050), dict(tempo=5.0), "tempo must lie"), ((wav, [1000, 1000], 2.0, 500), {}, "sample_rate must be"),
                          ((wav, [1000, 1000], 2.0, 22050), {}, "wav must be on the GPU")):
        with pytest.raises(ValueError, match=msg):
            psola.pitch_shift_psola(*args, **kw)
    with pytest.raises(ValueError, match="pitch tracker's lags"):
        psola.check_rate("say", 4000)                                                      # 4000 // 500 = 8 < 16
    psola.check_rate("say", 22050)
    psola.check_rate("say", 48000)


def test_say_settings_are_checked_before_anything_is_decoded():
    from tacotron2_amd.run.say import scale_records, voice_settings
    assert voice_settings(None, None, SR) is None and voice_settings(None, None, SR, True, None, None) is None
    plain = voice_settings(0.8, None, SR)
    assert plain.psola is False and plain.ratio == (800, 1000)
    v = voice_settings(1.25, 3, SR, True, True, None)
    assert (v.psola, v.tempo, v.ratio, v.semitones, v.pitch_range, v.sr_mid, v.active) == (True, 1.25, (1250, 1000), 3.0, 1.0, SR, True)
    assert voice_settings(None, None, SR, True, None, 0.5).psola and voice_settings(None, None, SR, True, None, 0.5).active
    assert voice_settings(None, 0, SR, True, True, 1).active is False and voice_settings(1.0, 0.0, SR, True, True, 1.0).active is False
    for args, name in (((None, None, SR, True, True, None), "--preserve-formants needs"), ((None, None, SR, True, None, 2.5), "--pitch-range must lie"),
                       ((None, None, SR, True, None, -0.1), "--pitch-range must lie"), ((None, None, SR, True, None, float("nan")), "--pitch-range"),
                       ((None, None, SR, False, None, 0.5), "--pitch-range need a .wav"), ((None, 2, SR, False, True, None), "--preserve-formants and"),
                       ((None, 13, SR, True, True, None), "--pitch-shift must lie"), ((None, 2, 4000, True, True, None), "pitch tracker's lags")):
        with pytest.raises(ValueError, match=name):
            voice_settings(*args)
    rec = [dict(start_s=[0.0, 1.0], end_s=[1.0, 2.0])]
    out = scale_records(rec, v)[0]
    assert out["end_s"] == [0.8, 1.6] and (out["tempo"], out["pitch_shift_semitones"], out["preserve_formants"], out["pitch_range"]) == (1.25, 3.0, True, 1.0)
    assert "preserve_formants" not in scale_records([dict(start_s=[0.0], end_s=[1.0])], plain)[0]


def test_integration_md_stub_mirrors_the_header_and_the_abi_has_the_entry():
    import ctypes as C
    import os
    import re
    from tacotron2_amd import _lib, build
    md = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    block = md[md.index("class T2Psola(C.Structure)"):]
    block = block[:block.index("]\n") + 1]
    fields = [f[0] for f in _lib._structs["T2Psola"]]
    assert re.findall(r'\("(\w+)",\s*C\.', block) == fields and "`t2_psola(const T2Psola*, stream)`" in md
    assert fields == ["x", "ldx", "n", "lag", "rho", "ldt", "w", "B", "n_max", "T", "hop", "U", "y", "ldy", "a", "ldm", "r", "kmap", "lds",
                      "n_marks", "n_syn"]
    build.build(verbose=False)
    lib = _lib.lib()
    assert "t2_psola" in _lib.DECLARED_SYMBOLS and hasattr(lib, "t2_psola")
    assert lib.t2_sizeof(b"T2Psola") == C.sizeof(_lib.S["T2Psola"]) > 0
    from tacotron2_amd.psola import SYN_TAIL
    header = open(os.path.join(os.path.dirname(_lib.HEADER), "tacotron2_amd.h")).read()
    assert f"#define T2_PSOLA_SYN_TAIL {SYN_TAIL}" in header and "#define T2_PSOLA_MAX_LAG 4096" in header
