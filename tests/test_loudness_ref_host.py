"""tests/loudness_ref.py itself, the float64 restatement of t2_loudness, against the figures of ITU-R BS.1770-4, and the
argument checks of tacotron2_amd/loudness.py and of `say --loudness / --true-peak` that need no device."""
import importlib.util
import math
import os

import numpy as np
import pytest

import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_48K = ([1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585], [1.0, -2.0, 1.0],
             [1.0, -1.99004745483398, 0.99007225036621])


def test_coefficients_at_48_khz_are_the_standards_table_and_the_package_forms_the_same():
    from tacotron2_amd.loudness import ABS_GATE, hop, k_weighting
    for got, want in zip(R.k_weighting(48000), TABLE_48K):
        assert np.abs(got - np.array(want)).max() <= 1e-12
    for sr in (8000, 16000, 22050, 24000, 44100, 48000, 96000, 192000):
        for got, want in zip(k_weighting(sr), R.k_weighting(sr)):
            assert isinstance(got, tuple) and len(got) == 3 and np.abs(np.array(got) - want).max() <= 1e-15
    assert k_weighting(22050) is k_weighting(22050)                     # cached
    assert ABS_GATE == R.ABS_GATE and (hop(22050), hop(8000), hop(44100), hop(11025)) == (2205, 800, 4410, 1102)


def test_a_full_scale_997_hz_sine_reads_minus_3_01_lufs():
    got = R.measure(R.sine(48000, 997.0, 5.0), 48000)
    assert abs(got["lufs"] + 3.01) <= 0.01 and got["flags"] == 0 and got["n_blocks"] == 47 and got["n_below_abs"] == got["n_below_rel"] == 0
    for sr in (44100, 24000, 22050, 16000, 8000):                       # (the bilinear re-derivation moves the reading by up to 0.04 LU)
        assert abs(R.measure(R.sine(sr, 997.0, 5.0), sr)["lufs"] + 3.01) <= 0.05, sr


def test_a_tenth_of_the_signal_reads_20_lu_lower():
    x = R.sine(48000, 997.0, 5.0, dtype=np.float64)
    a, b = (R.measure(v, 48000, dtype=np.float64)["lufs"] for v in (x, 0.1 * x))
    assert abs((a - b) - 20.0) <= 1e-9


@pytest.mark.parametrize("sr,gated,ungated", [(8000, -26.24, -28.90), (22050, -26.39, -29.05)])
def test_the_gates_matter_on_the_gate_signal(sr, gated, ungated):
    got = R.measure(R.gate_signal(sr), sr)
    assert (got["n_blocks"], got["n_below_abs"], got["n_below_rel"]) == (37, 7, 10) and got["flags"] == 0
    assert abs(got["lufs"] - gated) <= 0.005 and abs(got["ungated_lufs"] - ungated) <= 0.005
    assert got["lufs"] - got["ungated_lufs"] > 2.0 and got["margin_lu"] > 2.4


def test_short_rows_empty_rows_and_silence():
    sr, H = 8000, 800
    x = R.sine(sr, 440.0, 0.3, 0.1)                                     # 2400 samples: below one block of 3200
    got = R.measure(x, sr)
    y2 = R.weighted(x, sr) ** 2
    assert got["flags"] == R.SHORT and got["n_blocks"] == 1 and len(got["E"]) == 3
    assert abs(got["lufs"] - (-0.691 + 10.0 * math.log10(y2.sum() / len(x)))) <= 1e-12
    one = R.measure(x[:1], sr)                                          # one sample is a block, too
    assert one["n_blocks"] == 1 and one["flags"] & R.SHORT and len(one["E"]) == 0
    full = R.measure(R.sine(sr, 440.0, 0.4, 0.1), sr)
    assert full["flags"] == 0 and full["n_blocks"] == 1 and len(full["E"]) == 4
    for x in (np.zeros(0, np.float32), np.zeros(5000, np.float32), np.full(5000, 1e-5, np.float32)):
        got = R.measure(x, sr, target=-23.0)
        assert got["flags"] == R.UNDEFINED and math.isnan(got["lufs"]) and got["gain"] == 1.0 and got["n_below_rel"] == 0
        assert got["n_below_abs"] == got["n_blocks"] == max(len(x) // H - 3, 0)
    assert R.measure(np.zeros(0, np.float32), sr)["true_peak"] == 0.0 and math.isnan(R.measure(np.zeros(0, np.float32), sr)["momentary_max_lufs"])


def test_the_true_peak_sees_what_the_samples_miss():
    for sr, want in ((8000, 1.014), (22050, 1.072)):
        got = R.measure(R.sine(sr, sr / 4.0, 0.5, 1.0, math.pi / 4.0), sr)
        assert abs(got["sample_peak"] - 0.7071) <= 1e-4 and got["true_peak"] > 1.0 and abs(got["true_peak"] - want) <= 2e-3
        assert abs(R.measure(R.sine(sr, 440.0, 1.0, 0.5), sr)["true_peak"] - 0.5) <= 1e-4


def test_the_gain_is_capped_then_limited():
    sr = 8000
    x = R.sine(sr, 440.0, 1.0, 0.5)
    plain = R.measure(x, sr, target=-23.0)
    assert plain["flags"] == 0 and abs(20.0 * math.log10(plain["gain"]) - (-23.0 - plain["lufs"])) <= 1e-12
    lim = R.measure(x, sr, target=-3.0, ceiling=-1.0)              # (-9 LUFS at a peak of 0.5: 6 dB more would reach full scale)
    assert lim["flags"] == R.LIMITED and abs(lim["gain"] * lim["true_peak"] - 10.0 ** (-1.0 / 20.0)) <= 1e-12
    cap = R.measure(R.sine(sr, 440.0, 1.0, 1e-3), sr, target=-10.0, max_gain_db=30.0)
    assert cap["flags"] == R.CAPPED and cap["gain"] == 10.0 ** 1.5


def test_argument_rejections_of_the_python_layer():
    import torch
    from tacotron2_amd import analysis, engine, loudness
    assert engine.loudness is analysis.loudness is loudness.loudness and engine.normalize_loudness is loudness.normalize_loudness
    assert engine.k_weighting is loudness.k_weighting
    assert loudness.MAX_GAIN_DB == 30.0 and loudness.NSTAT == len(loudness.STATS) == 10
    wav = torch.zeros(2, 1000)
    bad = [((wav[0], [1000, 1000], 8000), "wav must be a float32"), ((wav.double(), [1000, 1000], 8000), "wav must be a float32"),
           ((wav[:, ::2], [500, 500], 8000), "last dimension of wav"), ((wav, [1000, 1001], 8000), "n must lie in"),
           ((wav, [1000, -1], 8000), "n must lie in"), ((wav, [1000], 8000), "n must be 2 integers"), ((wav, [1.5, 2.0], 8000), "n must be 2 integers"),
           ((wav, [1000, 1000], 7999), "sample_rate must be"), ((wav, [1000, 1000], 192001), "sample_rate must be"),
           ((wav, [1000, 1000], 22050.0), "sample_rate must be"), ((wav, [1000, 1000], True), "sample_rate must be"),
           ((wav, [1000, 1000], 8000), "wav must be on the GPU")]
    for args, msg in bad:
        with pytest.raises(ValueError, match="^loudness: .*" + msg):
            loudness.loudness(*args)
        with pytest.raises(ValueError, match="^normalize_loudness: .*" + msg):
            loudness.normalize_loudness(*args)
    for kw, msg in ((dict(target=0.5), "target must lie in -70 .. 0"), (dict(target=-71), "target must lie"), (dict(target=float("nan")), "target must be a finite"),
                    (dict(ceiling=0.1), "ceiling must lie in -40 .. 0"), (dict(ceiling=-41.0), "ceiling must lie"), (dict(ceiling="-1"), "ceiling must be a finite"),
                    (dict(max_gain_db=-1.0), "max_gain_db must lie in 0 .. 120"), (dict(max_gain_db=121), "max_gain_db must lie"),
                    (dict(max_gain_db=True), "max_gain_db must be a finite")):
        with pytest.raises(ValueError, match=msg):
            loudness.normalize_loudness(wav, [1000, 1000], 8000, **kw)
    for sr in (7999, 192001, 22050.0, None):
        with pytest.raises((ValueError, TypeError)):
            loudness.k_weighting(sr)
    with pytest.raises(ValueError, match="batch of 0"):
        loudness.loudness(torch.zeros(0, 10), [], 8000)


def test_say_settings_are_checked_before_anything_is_decoded():
    from tacotron2_amd.run.say import loudness_fields, loudness_line, loudness_settings
    assert loudness_settings(None, None) is None and loudness_settings(None, None, False) is None
    assert loudness_settings(-16, None) == (-16.0, -1.0) and loudness_settings(-23.0, -2.5, True, 16000) == (-23.0, -2.5)
    assert loudness_settings(-40, 0) == (-40.0, 0.0) and loudness_settings(-5, -9, True, 192000) == (-5.0, -9.0)
    for args, msg in (((-4.9, None), "--loudness must lie in -40 .. -5"), ((-40.1, None), "--loudness must lie"), ((float("nan"), None), "--loudness"),
                      ((True, None), "--loudness"), ((-16, 0.1), "--true-peak must lie in -9 .. 0"), ((-16, -9.5), "--true-peak must lie"),
                      ((None, -1.0), "--true-peak needs --loudness"), ((-16, None, False), "--loudness and --true-peak need a .wav"),
                      ((-16, -1.0, False), "need a .wav"), ((-16, None, True, 4000), "--loudness at 4000 Hz")):
        with pytest.raises(ValueError, match=msg):
            loudness_settings(*args)
    rec = dict(loudness_lufs=-27.314, gain_db=7.314, true_peak_dbtp=-3.2, flags=0)
    assert loudness_line("a.wav", rec) == "say: a.wav: -27.31 LUFS, gain +7.31 dB, true peak -3.20 dBTP"
    assert loudness_line("a.wav", dict(rec, flags=4 | 1)).endswith("dBTP, peak-limited, short")
    assert loudness_line("a.wav", dict(rec, flags=8)).endswith(", boost capped")
    assert loudness_line("a.wav", dict(loudness_lufs=None, gain_db=0.0, true_peak_dbtp=None, flags=2)) == "say: a.wav: no loudness (left as it is)"
    assert loudness_fields(rec) == dict(loudness_lufs=-27.314, gain_db=7.314, true_peak_dbtp=-3.2)


def test_usage_errors_of_say_name_the_option(tmp_path):
    from click.testing import CliRunner
    spec = importlib.util.spec_from_file_location("t2_main_cli_loudness", os.path.join(ROOT, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    doc = tmp_path / "d.txt"
    doc.write_text("One came.\n", encoding="utf-8")
    head = ["--device", "0", "say", "--checkpoint", str(tmp_path / "none.ckpt")]
    text, file, npy = ["--text", "Hi."], ["--text-file", str(doc)], str(tmp_path / "o.npy")
    cases = [([*text, "--out", npy, "--loudness", "-16"], "--loudness"), ([*text, "--out", npy, "--loudness", "-16", "--true-peak", "-1"], "--loudness"),
             ([*text, "--out", "o.wav", "--true-peak", "-1"], "--true-peak needs --loudness"), ([*file, "--out", "o.wav", "--true-peak", "-2"], "--true-peak"),
             ([*text, "--out", "o.wav", "--loudness", "-4"], "--loudness must lie"), ([*text, "--out", "o.wav", "--loudness", "-41"], "--loudness must lie"),
             ([*file, "--out", "o.wav", "--loudness", "nan"], "--loudness"), ([*text, "--out", "o.wav", "--loudness", "loud"], "--loudness"),
             ([*text, "--out", "o.wav", "--loudness", "-16", "--true-peak", "0.5"], "--true-peak must lie"),
             ([*file, "--out", "o.wav", "--loudness", "-16", "--true-peak", "-10"], "--true-peak must lie")]
    for args, name in cases:
        r = CliRunner().invoke(mod.main, head + args)
        assert r.exit_code == 2 and name in r.output and "Usage:" in r.output, (args, r.exit_code, r.output, r.exception)
    assert not (tmp_path / "o.npy").exists()


def test_integration_md_stub_mirrors_the_header_and_the_abi_has_the_entry():
    import ctypes as C
    import re
    from tacotron2_amd import _lib, build, loudness
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = md[md.index("class T2Loudness(C.Structure)"):]
    block = block[:block.index("]\n") + 1]
    fields = [f[0] for f in _lib._structs["T2Loudness"]]
    assert re.findall(r'\("(\w+)",\s*C\.', block) == fields and "`t2_loudness(const T2Loudness*, stream)`" in md
    assert fields == ["x", "ldx", "n", "table", "K", "B", "n_max", "H", "b1", "a1", "b2", "a2", "abs_gate", "target", "max_gain", "ceiling",
                      "E", "lde", "stat", "gain", "y", "ldy"]
    build.build(verbose=False)
    lib = _lib.lib()
    assert "t2_loudness" in _lib.DECLARED_SYMBOLS and hasattr(lib, "t2_loudness")
    assert lib.t2_sizeof(b"T2Loudness") == C.sizeof(_lib.S["T2Loudness"]) > 0
    header = open(_lib.HEADER).read()
    assert f"#define T2_LOUD_NSTAT {loudness.NSTAT}" in header
