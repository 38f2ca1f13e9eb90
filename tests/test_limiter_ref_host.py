"""tests/limiter_ref.py itself, the sequential float64 restatement of t2_limit: the bound s <= r that makes it a limiter,
the shape of the curve around one impulse, the start-of-row rule, and the numpy restatement of the kernel's chunked release scan
against the sequential recurrence; and what of tacotron2_amd/limiter.py and `say --limiter` needs no device: the argument checks, the
line, the INTEGRATION.md stub and the constants the header states as an enum."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import limiter_ref as M
import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 8000
C = 10.0 ** (-1.0 / 20.0)


def test_the_curve_stays_under_the_required_gain_on_every_signal_of_the_gpu_test():
    from tacotron2_amd import limiter
    for L, release_ms in ((40, 50.0), (1, 5.0), (2048, 2000.0)):
        a = M.coefficient(release_ms, SR)
        for name, x in M.rows(limiter.PASS, 40, SR):
            out = M.limit(x, SR, C, L, a)
            if len(x):
                assert (out["s"] <= out["r"] + 1e-12).all(), (L, name, (out["s"] - out["r"]).max())
                assert (out["s"] <= 1.0).all() and out["min_gain"] >= min(1.0, float(np.float32(C / out["in_peak"]))) - 1e-12
    names = {name: M.limit(x, SR, C, 40, M.coefficient(50.0, SR)) for name, x in M.rows(limiter.PASS, 40, SR)}
    assert names["below"]["n_over"] == 0 and names["above"]["n_over"] == 3000 and names["2P+77"]["n_over"] > 20


def test_one_impulse_a_ramp_of_l_plus_1_samples_the_floor_and_the_release():
    L, p, n, peak = 40, 500, 3000, 1.6
    a = M.coefficient(50.0, SR)
    env = np.zeros(n, np.float32)
    env[p] = peak
    out = M.gain_curve(env, C, L, a)
    floor = float(np.float32(C / peak))
    s = out["s"]
    assert out["n_over"] == 1 and (s[:p - L] == 1.0).all() and abs(s[p] - floor) <= 1e-15 and abs(out["min_gain"] - floor) <= 1e-15
    ramp = 1.0 - (np.arange(p - L, p + 1) - (p - L) + 1) * (1.0 - floor) / (L + 1)
    assert np.abs(s[p - L:p + 1] - ramp).max() <= 1e-14                # linear over the L + 1 samples in front of the impulse
    m = np.arange(1, 1200)
    assert np.abs(out["e"][p + m] - (1.0 - (1.0 - floor) * a ** m)).max() <= 1e-12          # the release: 1 - (1 - floor) a^m
    tau = int(round(0.050 * SR))
    assert abs((1.0 - out["e"][p + tau]) / (1.0 - floor) - math.exp(-1.0)) <= 1e-3


def test_a_peak_at_sample_0_at_n_minus_1_and_two_closer_than_l():
    L, a = 40, M.coefficient(50.0, SR)
    x = M.pulses(11, 2000, [0, 900, 915, 1999], SR)
    out = M.limit(x, SR, C, L, a)
    r, s, h = out["r"], out["s"], out["h"]
    assert r[0] < 1.0 and s[0] == float(h[0]) <= r[0]                    # the limiter is already down when the row starts
    assert r[1999] < 1.0 and s[1999] <= r[1999] + 1e-12 and (s <= r + 1e-12).all()
    assert (h[900 - L:916] <= max(r[900], r[915])).all() and s[900:918].max() < 1.0       # one dip for the two
    assert out["peak_after"] <= C * (1.0 + 1e-4) and R.true_peak(out["y"], SR) <= C * (1.0 + 1e-6)
    # with e = 1 in front of the row the peak at the sample 0 passes: the bound of the attack needs the start-of-row rule
    e1 = M.release(h, a, start=1.0)
    assert M.attack(np.concatenate([np.ones(L), e1]), L)[0] > r[0] + 0.1


def test_a_row_under_the_ceiling_keeps_its_bits():
    x = M.voice(7, 5000, 0.05, SR)
    out = M.limit(x, SR, C, 40, M.coefficient(50.0, SR))
    assert out["n_over"] == 0 and (out["s"] == 1.0).all() and out["flags"] == 0 and out["trim"] == 1.0
    assert np.array_equal(out["y"].view(np.uint32), x.view(np.uint32))
    empty = M.limit(np.zeros(0, np.float32), SR, C, 40, 0.99)
    assert empty["n_over"] == 0 and empty["flags"] == 0 and len(empty["y"]) == 0 and empty["in_peak"] == 0.0


def test_the_limited_voice_is_closer_to_the_target_than_the_plain_gain():
    for sr, plain_want, lim_want in ((8000, -10.99, -10.25), (22050, -11.20, -10.34)):
        x = M.voice(1, 3 * sr, 0.1, sr)
        m = R.measure(x, sr)
        g_plain, flags = R.gain(m["lufs"], m["true_peak"], -10.0, -1.0)
        assert flags & R.LIMITED
        v = x * np.float32(10.0 ** ((-10.0 - m["lufs"]) / 20.0))
        out = M.limit(v, sr, C, M.lookahead_samples(5.0, sr), M.coefficient(50.0, sr))
        plain, lim = R.measure(x * np.float32(g_plain), sr)["lufs"], R.measure(out["y"], sr)["lufs"]
        print(f"{sr} Hz: plain {plain:.3f} LUFS, limiter {lim:.3f} LUFS, overshoot before the trim {20 * math.log10(out['peak_after'] / C):.2e} dB")
        assert abs(plain - plain_want) <= 0.01 and abs(lim - lim_want) <= 0.01 and abs(lim + 10.0) < abs(plain + 10.0)
        assert 20.0 * math.log10(out["peak_after"] / C) <= 1e-4 and R.true_peak(out["y"], sr) <= C * (1.0 + 1e-6)


@pytest.mark.parametrize("sr,release_ms", [(8000, 5.0), (8000, 50.0), (8000, 2000.0), (22050, 50.0), (192000, 2000.0)])
def test_the_chunked_release_scan_meets_the_sequential_recurrence(sr, release_ms):
    """The bound: tau / e * 2^-53 absolute, tau = release_s * sr, from max_m m a^m - the error of a power a^m formed by squaring,
    times the d it carries.  The sequential recurrence itself stops tau / 2 ulps short of 1 (limiter_ref.stall); a scan that lets d
    decay to 0 differs from it by tau * 2^-54 there, 1.36 times the bound, which is why the kernel holds d at that level."""
    from tacotron2_amd import limiter
    a, tau = M.coefficient(release_ms, sr), release_ms / 1000.0 * sr
    worst = 0.0
    for name, x in M.rows(limiter.PASS, 40, SR):
        if len(x):
            h = M.lookahead(M.required(M.envelope(M.peaks(x, SR)).astype(np.float32), C)[0], 40)
            worst = max(worst, float(np.abs(M.release_chunked(h, a) - M.release(h, a)).max()))
    rng = np.random.default_rng(3)                                        # dips with long and short gaps over five passes
    n = 5 * limiter.PASS + 77
    r = np.ones(n, np.float32)
    r[rng.integers(0, n, 12)] = rng.uniform(0.2, 0.9, 12).astype(np.float32)
    h = M.lookahead(r, 30)
    worst = max(worst, float(np.abs(M.release_chunked(h, a) - M.release(h, a)).max()))
    print(f"{sr} Hz, release {release_ms} ms: worst |chunked - sequential| = {worst:.3e}, bound {tau / math.e * 2.0 ** -53:.3e}")
    assert worst <= tau / math.e * 2.0 ** -53
    assert 0.0 < M.stall(a) <= tau * 2.0 ** -53 and abs(M.stall(a) * 2.0 ** 53 - tau / 2.0) <= 2.0


def test_the_module_api_and_argument_rejections():
    from tacotron2_amd import analysis, engine, limiter, loudness
    assert engine.limit_peaks is analysis.limit_peaks is limiter.limit_peaks
    assert (limiter.NSTAT, limiter.MAX_L, limiter.PASS) == (8, 2048, 4096) and len(limiter.STATS) == 6
    assert (limiter.LOOKAHEAD_MS, limiter.RELEASE_MS) == (5.0, 50.0)
    assert limiter.settings("f", 22050) == (22050, 110, math.exp(-1.0 / (0.05 * 22050)))
    assert limiter.settings("f", 192000, 20.0, 5.0)[1] == 2048 and limiter.settings("f", 8000, 0.1, 2000.0)[1] == 1
    assert limiter.settings("f", 8000, 5.0, 50.0)[1:] == (M.lookahead_samples(5.0, 8000), M.coefficient(50.0, 8000))
    wav = torch.zeros(2, 1000)
    for args, kw, msg in (((torch.zeros(1000), [1000], 8000), {}, r"wav must be a float32 \(B, samples\) tensor"),
                          ((wav.double(), [1000, 1000], 8000), {}, "wav must be a float32"),
                          ((wav, [1000, 1000], 7999), {}, "sample_rate must be an integer in 8000 .. 192000"),
                          ((wav, [1000, 1000], 8000.0), {}, "sample_rate must be an integer"),
                          ((wav, [1000, 1000], 8000), dict(lookahead_ms=0.05), "lookahead_ms must lie in 0.1 .. 20"),
                          ((wav, [1000, 1000], 8000), dict(lookahead_ms=21), "lookahead_ms must lie"),
                          ((wav, [1000, 1000], 8000), dict(release_ms=4.9), "release_ms must lie in 5 .. 2000"),
                          ((wav, [1000, 1000], 8000), dict(release_ms=float("nan")), "release_ms must be a finite number"),
                          ((wav, [1000, 1000], 8000), dict(ceiling=0.1), "ceiling must lie in -40 .. 0"),
                          ((wav, [1000, 1001], 8000), {}, "n must lie in 0 .. 1000"),
                          ((wav, [1000], 8000), {}, "n must be 2 integers"),
                          ((wav, [1000, 1000], 8000), {}, "wav must be on the GPU")):
        with pytest.raises(ValueError, match="^limit_peaks: .*" + msg):
            limiter.limit_peaks(*args, **kw)
    for lim, msg in (("yes", "limiter must be None, True or a dict"), (False, "limiter must be"), (dict(attack_ms=1.0), "limiter must be"),
                     (dict(lookahead_ms=0.01), "lookahead_ms must lie"), (dict(release_ms=3000), "release_ms must lie")):
        with pytest.raises(ValueError, match="^normalize_loudness: .*" + msg):
            loudness.normalize_loudness(wav, [1000, 1000], 8000, limiter=lim)
    with pytest.raises(ValueError, match="^normalize_loudness: .*wav must be on the GPU"):
        loudness.normalize_loudness(wav, [1000, 1000], 8000, limiter=True)


def test_say_settings_the_line_and_the_fields():
    from tacotron2_amd.run.say import limiter_settings, loudness_fields, loudness_line, loudness_settings
    assert limiter_settings(None, None) is False and limiter_settings(False, -16) is False and limiter_settings(None, -16) is False
    assert limiter_settings(True, -16) is True and loudness_settings(-16, None) == (-16.0, -1.0)
    with pytest.raises(ValueError, match="--limiter needs --loudness"):
        limiter_settings(True, None)
    with pytest.raises(ValueError, match="--limiter is a flag"):
        limiter_settings(1, -16)
    rec = dict(loudness_lufs=-27.314, gain_db=11.314, true_peak_dbtp=-1.004, flags=0, limited_samples=412, limiter_max_reduction_db=2.618,
               output_lufs=-16.42)
    assert loudness_line("a.wav", rec) == ("say: a.wav: -27.31 LUFS, gain +11.31 dB, limited 412 samples by up to 2.62 dB, now -16.42 LUFS, "
                                          "true peak -1.00 dBTP")
    assert loudness_line("a.wav", dict(rec, flags=8 | 1)).endswith("true peak -1.00 dBTP, boost capped, short")
    assert loudness_line("a.wav", dict(rec, loudness_lufs=None, output_lufs=None, flags=2)) == "say: a.wav: no loudness (left as it is)"
    assert loudness_fields(rec) == {k: rec[k] for k in rec if k != "flags"}
    plain = dict(loudness_lufs=-27.314, gain_db=7.314, true_peak_dbtp=-3.2, flags=4)
    assert loudness_line("a.wav", plain) == "say: a.wav: -27.31 LUFS, gain +7.31 dB, true peak -3.20 dBTP, peak-limited"
    assert set(loudness_fields(plain)) == {"loudness_lufs", "gain_db", "true_peak_dbtp"}


def test_limiter_without_loudness_is_a_usage_error(tmp_path):
    from click.testing import CliRunner
    spec = importlib.util.spec_from_file_location("t2_main_cli_limiter", os.path.join(ROOT, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    doc = tmp_path / "d.txt"
    doc.write_text("One came.\n", encoding="utf-8")
    head = ["--device", "0", "say", "--checkpoint", str(tmp_path / "none.ckpt")]
    for args in (["--text", "Hi.", "--out", "o.wav", "--limiter"], ["--text-file", str(doc), "--out", "o.wav", "--limiter"],
                 ["--text", "Hi.", "--out", "o.wav", "--limiter", "--true-peak", "-2"]):
        r = CliRunner().invoke(mod.main, head + args)
        assert r.exit_code == 2 and "needs --loudness" in r.output and "Usage:" in r.output, (args, r.exit_code, r.output, r.exception)
    r = CliRunner().invoke(mod.main, head + ["--text", "Hi.", "--out", str(tmp_path / "o.npy"), "--loudness", "-16", "--limiter"])
    assert r.exit_code == 2 and "--loudness" in r.output


def test_integration_md_stub_the_abi_and_the_constants_of_the_header():
    import ctypes as C
    import re
    from tacotron2_amd import _lib, build, limiter
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = md[md.index("class T2Limit(C.Structure)"):]
    block = block[:block.index("]\n") + 1]
    fields = [f[0] for f in _lib._structs["T2Limit"]]
    assert re.findall(r'\("(\w+)",\s*C\.', block) == fields and "`t2_limit(const T2Limit*, stream)`" in md
    assert fields == ["x", "ldx", "n", "table", "K", "B", "n_max", "L", "a", "ceiling", "env", "lde", "curve", "ldc", "y", "ldy", "stat"]
    build.build(verbose=False)
    lib = _lib.lib()
    assert "t2_limit" in _lib.DECLARED_SYMBOLS and hasattr(lib, "t2_limit")
    assert lib.t2_sizeof(b"T2Limit") == C.sizeof(_lib.S["T2Limit"]) > 0
    header = open(_lib.HEADER).read()
    assert f"enum {{ T2_LIMIT_NSTAT = {limiter.NSTAT}, T2_LIMIT_MAX_L = {limiter.MAX_L} }};" in header
    assert not any(k.startswith("LIMIT") for k in _lib.K)                # no `#define T2_<NAME> <integer>` of this entry
    src = open(os.path.join(ROOT, "tacotron2_amd", "csrc", "t2_limit.hip")).read()
    assert "#define LM_CHUNK 16\n" in src and "#define LM_THREADS 256\n" in src and limiter.PASS == 16 * 256
