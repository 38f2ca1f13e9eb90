"""tests/denoise_ref.py itself, the numpy / scipy restatement of t2_denoise: the identity with a zero bias, the divisor,
the stationary hum at half and at full strength, short rows, the float32 restatement's error against the stored constants, the case
list's clearance from its thresholds; and what of tacotron2_amd/denoise.py and `say --denoise` needs no device: the argument checks,
the three usage errors, the line, the INTEGRATION.md stub and the constants the header states as an enum."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = np.zeros(R.BINS, np.float32)


@pytest.mark.parametrize("n", [513, 1024, 2149, 5120])
def test_with_a_zero_bias_the_rule_is_the_identity(n):
    x = R.signal(n)
    out = R.denoise(x, ZERO, 1.0)
    e = float(np.abs(out["y"] - x.astype(np.float64)).max())
    print(f"n = {n}: max |y - x| = {e:.2e}")
    assert e <= 1e-12 and out["frames"] == 1 + n // 256 and out["gated"] == 0 and out["flags"] == 0


def test_the_divisor_is_positive_at_every_length_and_the_file_states_its_minimum():
    low = R.envelope_min()
    print(f"smallest divisor over every n mod 256: {low:.6f}")
    assert low > 0 and R.ENV_MIN <= low <= R.ENV_MIN + 1e-4
    for n in (513, 767, 768, 1024, 2149):                                 # every sample lies under at least two frames with a positive window
        w, cover = R.window().astype(np.float64), np.zeros(n + R.NFFT, int)
        for t in range(R.n_frames(n)):
            cover[t * R.HOP:t * R.HOP + R.NFFT] += w > 0
        assert cover[R.NFFT // 2:R.NFFT // 2 + n].min() >= 2, n
    assert abs(float(R.envelope(5120)[2000]) - 1.5) <= 1e-6               # in the interior it is the window's 1.5


def test_a_stationary_hum_comes_out_at_half_amplitude_and_is_gone_at_full_strength():
    h = R.hum()
    m = R.magnitudes(h)[R.interior_frames(len(h))]
    assert np.abs(m - m[0]).max() <= 1e-12 * m.max()                      # every interior frame sees the same samples
    bias = R.hum_bias()
    half, full = R.interior_db(R.denoise(h, bias, 0.5)["y"], h), R.interior_db(R.denoise(h, bias, 1.0)["y"], h)
    print(f"hum: {half:.6f} dB at strength 0.5, {full:.1f} dB at strength 1.0")
    assert abs(half - 20.0 * np.log10(0.5)) <= 1e-6 and full < -150.0


def test_short_rows_are_copied():
    for n in (0, 1, 512):
        x = R.signal(n)
        for dtype in (np.float64, np.float32):
            out = R.denoise(x, R.hum_bias(), 1.0, dtype)
            assert np.array_equal(out["y"].astype(np.float32).view(np.uint32), x.view(np.uint32)) and out["flags"] == R.FLAG_SHORT
            assert out["frames"] == 0 and out["gated"] == 0 and out["mag"].shape == (0, R.BINS)
    assert R.denoise(R.signal(513), R.hum_bias(), 1.0)["flags"] == 0


def test_the_float32_restatement_lies_within_the_stored_constants():
    got = R.measure_f32_err()
    print({k: (f"{e:.3e}", name) for k, (e, name) in got.items()})
    assert set(got) == set(R.F32_ERR) == set(R.TOL) == {"y", "mag", "roundtrip"}
    for k, (e, name) in got.items():
        assert e <= R.F32_ERR[k] <= 2.0 * e, (k, e, name)                  # audio_ref's rule: no case above, no constant twice what is measured
        assert R.TOL[k] == 16.0 * R.F32_ERR[k]


def test_on_the_case_list_no_bin_lies_on_its_threshold():
    """gated_cap presumes that a bin outside its band cannot flip.  The mag check allows TOL["mag"] x max |m| of error, so the case
    list keeps every such bin farther than that from its threshold (denoise_ref.SEED), and the cap itself stays below 1 % of the bins."""
    bias, bins, cap, margin, gated = R.hum_bias(), 0, 0, np.inf, 0
    for n in R.LENGTHS:
        for s in R.STRENGTHS:
            ref = R.denoise(R.signal(n), bias, s)
            bins, cap, gated = bins + ref["mag"].size, cap + R.gated_cap(ref, R.TOL["mag"]), gated + ref["gated"]
            if ref["mag"].size:
                margin = min(margin, R.threshold_margin(ref, R.TOL["mag"]))
    print(f"{bins} bins, {gated} gated, cap {cap}, nearest |m - thr| / max |m| = {margin:.2e} (TOL {R.TOL['mag']:.1e})")
    assert cap < 0.01 * bins and gated > 100 and margin > R.TOL["mag"]


def test_the_module_api_and_argument_rejections():
    from tacotron2_amd import analysis, denoise, engine
    assert engine.denoise is analysis.denoise is denoise.denoise and engine.stft_magnitudes is analysis.stft_magnitudes is denoise.stft_magnitudes
    assert engine.vocoder_bias is analysis.vocoder_bias is denoise.vocoder_bias
    assert (denoise.NFFT, denoise.HOP, denoise.NSTAT, denoise.BINS) == (R.NFFT, R.HOP, 4, R.BINS) and denoise.BIAS_FRAMES == 88
    assert denoise.STRENGTH_LIMITS == (0.0, 1.0) and denoise.FLAG_SHORT == R.FLAG_SHORT
    wav, bias = torch.zeros(2, 1000), torch.zeros(513)
    for args, msg in (((torch.zeros(1000), [1000], bias, 0.5), r"wav must be a float32 \(B, samples\) tensor"),
                      ((wav.double(), [1000, 1000], bias, 0.5), "wav must be a float32"),
                      ((wav, [1000, 1000], bias, -0.1), "strength must be a finite number >= 0"),
                      ((wav, [1000, 1000], bias, float("nan")), "strength must be a finite number"),
                      ((wav, [1000, 1000], bias, "1"), "strength must be a finite number"),
                      ((wav, [1000, 1000], torch.zeros(512), 0.5), r"bias must be a float32 \(513,\) tensor"),
                      ((wav, [1000, 1000], bias.double(), 0.5), "bias must be a float32"),
                      ((wav, [1000, 1000], [0.0] * 513, 0.5), "bias must be a float32"),
                      ((wav, [1000, 1001], bias, 0.5), "n must lie in 0 .. 1000"),
                      ((wav, [1000], bias, 0.5), "n must be 2 integers"),
                      ((wav, [1000, 1000], bias, 0.5), "wav must be on the GPU"),
                      ((wav, [1000, 1000], bias, 0), "wav must be on the GPU")):
        with pytest.raises(ValueError, match="^denoise: .*" + msg):
            denoise.denoise(*args)
    with pytest.raises(ValueError, match="^stft_magnitudes: .*wav must be on the GPU"):
        denoise.stft_magnitudes(wav, [1000, 1000])
    with pytest.raises(ValueError, match="^stft_magnitudes: .*n must lie in 0 .. 1000"):
        denoise.stft_magnitudes(wav, [1000, -1])
    with pytest.raises(ValueError, match="^vocoder_bias: frames must be an integer in 1 .. 4096"):
        denoise.vocoder_bias(object(), frames=2.0)


def test_say_settings_the_line_and_the_fields():
    from tacotron2_amd.run.say import denoise_fields, denoise_line, denoise_settings
    assert denoise_settings(None, None) is None and denoise_settings(None, "g.pt", "o.npy") is None
    assert denoise_settings(0.01, "g.pt", "o.wav") == 0.01 and denoise_settings(1, "g.pt") == 1.0
    assert denoise_settings(0, "g.pt", "o.wav") is None and denoise_settings(0.0, "g.pt", "o.wav") is None       # nothing runs
    for v in (-0.01, 1.01, float("nan"), float("inf"), True, "0.1"):
        with pytest.raises(ValueError, match="--denoise must lie in 0 .. 1"):
            denoise_settings(v, "g.pt", "o.wav")
    with pytest.raises(ValueError, match="--denoise needs --hifi-gan-checkpoint"):
        denoise_settings(0.1, None, "o.wav")
    with pytest.raises(ValueError, match="--denoise needs --hifi-gan-checkpoint"):
        denoise_settings(0, None, "o.wav")                                # (a usage error even where nothing would run)
    with pytest.raises(ValueError, match="--denoise needs a .wav target"):
        denoise_settings(0.1, "g.pt", "o.npy")
    assert denoise_line("a.wav", 0.01, 0.03217) == "say: a.wav: denoise 0.01, 3.22 % of bins gated"
    assert denoise_line("a.wav", 1.0, 0.0) == "say: a.wav: denoise 1, 0.00 % of bins gated"
    assert denoise_fields(0.1, 0.25) == dict(denoise_strength=0.1, denoise_gated_fraction=0.25)


def test_the_three_usage_errors_of_the_command_line(tmp_path):
    from click.testing import CliRunner
    spec = importlib.util.spec_from_file_location("t2_main_cli_denoise", os.path.join(ROOT, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    doc = tmp_path / "d.txt"
    doc.write_text("One came.\n", encoding="utf-8")
    head = ["--device", "0", "say", "--checkpoint", str(tmp_path / "none.ckpt")]
    hifi = ["--hifi-gan-checkpoint", str(tmp_path / "g.pt")]
    for args, msg in ((["--text", "Hi.", "--out", "o.wav", "--denoise", "0.1"], "--denoise needs --hifi-gan-checkpoint"),
                      (["--text-file", str(doc), "--out", "o.wav", "--denoise", "0.1"], "--denoise needs --hifi-gan-checkpoint"),
                      (["--text", "Hi.", "--out", str(tmp_path / "o.npy"), "--denoise", "0.1"] + hifi, "--denoise needs a .wav target"),
                      (["--text-file", str(doc), "--out", str(tmp_path / "o.npy"), "--denoise", "0.1"] + hifi, "--denoise needs a .wav target"),
                      (["--text", "Hi.", "--out", "o.wav", "--denoise", "1.5"] + hifi, "--denoise must lie in 0 .. 1"),
                      (["--text", "Hi.", "--out", "o.wav", "--denoise", "-0.1"] + hifi, "--denoise must lie in 0 .. 1")):
        r = CliRunner().invoke(mod.main, head + args)
        assert r.exit_code == 2 and msg in r.output and "Usage:" in r.output, (args, r.exit_code, r.output, r.exception)
    assert not (tmp_path / "o.npy").exists()
    r = CliRunner().invoke(mod.main, ["say", "--help"])
    text = " ".join(r.output.split())
    assert "--denoise STRENGTH" in text and "NVIDIA's defaults are 0.01 for" in text and "0.1 for WaveGlow" in text


def test_integration_md_stub_the_abi_and_the_constants_of_the_header():
    import ctypes as C
    import re
    from tacotron2_amd import _lib, build, denoise
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = md[md.index("class T2Denoise(C.Structure)"):]
    block = block[:block.index("]\n") + 1]
    fields = [f[0] for f in _lib._structs["T2Denoise"]]
    assert re.findall(r'\("(\w+)",\s*C\.', block) == fields and "`t2_denoise(const T2Denoise*, stream)`" in md
    assert fields == ["x", "ldx", "n", "B", "n_max", "win", "tw", "bias", "strength", "y", "ldy", "mag", "ldm", "f_max", "gated", "stat"]
    build.build(verbose=False)
    lib = _lib.lib()
    assert "t2_denoise" in _lib.DECLARED_SYMBOLS and hasattr(lib, "t2_denoise")
    assert lib.t2_sizeof(b"T2Denoise") == C.sizeof(_lib.S["T2Denoise"]) > 0
    header = open(_lib.HEADER).read()
    assert f"enum {{ T2_DENOISE_NFFT = {denoise.NFFT}, T2_DENOISE_HOP = {denoise.HOP}, T2_DENOISE_NSTAT = {denoise.NSTAT} }};" in header
    assert (R.NFFT, R.HOP) == (denoise.NFFT, denoise.HOP) and not any(k.startswith("DENOISE") for k in _lib.K)
    src = open(os.path.join(ROOT, "tacotron2_amd", "csrc", "t2_denoise.hip")).read()
    assert "#define DN_N T2_DENOISE_NFFT\n" in src and "#define DN_HOP T2_DENOISE_HOP\n" in src and "#define DN_G 16\n" in src
    assert "sincos" not in src                                            # twiddles from the table
