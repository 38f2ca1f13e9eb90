"""The sample-rate converter's host half, without a GPU: the filter design of tacotron2_amd/datasets/resample.py against the float64
restatement tests/resample_ref.py, what the design achieves (run through the restatement's own apply(), i.e. the kernel's rule in
float64), the length rule, and the errors of the dataset path.

Signals: unit tones at 0.02, 0.3, 0.6 and 0.7 of the LOWER of the two Nyquist rates (the passband: the cut is at 0.90 of it and the
Kaiser transition, beta 9 over 16 zero crossings, is about 0.18 of it on each side) and, for the pairs that go down far enough for
it to exist at the input, a tone at (2 - 0.9) = 1.1 times the new Nyquist rate (the first frequency that aliases into the passband's
upper edge).  Errors are peaks over the interior samples (3 filter half-widths from each end), in dB re the tone's amplitude."""
import functools
import math
from fractions import Fraction
import wave

import numpy as np
import pytest

import resample_ref as R

PAIRS = [8000, 11025, 16000, 22000, 24000, 32000, 44100, 48000]
TARGET = 22050


@functools.lru_cache(maxsize=None)
def designed(sr_in, sr_out=TARGET):
    from tacotron2_amd.datasets.resample import plan
    return R.design(sr_in, sr_out), plan(sr_in, sr_out)


def _tone(f, sr, n, ph=0.3):
    return np.sin(2 * np.pi * f * np.arange(n) / sr + ph)


def _edge(U, D, K):
    return 3 * K * max(1, U // D + 1)


def test_plan_ratios_and_half_widths():
    from tacotron2_amd.datasets.resample import plan
    assert plan(24000, 22050)[:3] == (147, 160, 18)
    assert plan(16000, 22050)[:3] == (441, 320, 16)
    assert plan(44100, 22050)[:3] == (1, 2, 32) and plan(11025, 22050)[:3] == (2, 1, 16)
    U, D, K, table = plan(24000, 22050)
    assert table.dtype == np.float32 and table.shape == (U, 2 * K) and table.flags.c_contiguous
    assert plan(24000, 22050) is plan(24000, 22050)          # cached per rate pair
    for bad in ((0, 22050), (22050, -1), (22050.0, 16000), (True, 16000)):
        with pytest.raises(ValueError):
            plan(*bad)


@pytest.mark.parametrize("sr_in", PAIRS)
def test_plan_is_the_restated_design_rounded_to_fp32_and_rows_sum_to_one(sr_in):
    (U, D, K, ref), (U2, D2, K2, table) = designed(sr_in)
    assert (U, D, K) == (U2, D2, K2)
    assert np.array_equal(ref.astype(np.float32), table)
    assert np.abs(ref.sum(1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    # the fp32 rows: 2K roundings of at most 2^-25 of the largest tap (<= 1) each
    assert np.abs(table.astype(np.float64).sum(1) - 1.0).max() <= 2 * K * 2.0 ** -25


@pytest.mark.parametrize("sr_in", PAIRS)
def test_constant_and_passband_tones_through_the_design(sr_in):
    (U, D, K, ref), _ = designed(sr_in)
    n = int(0.15 * sr_in)
    e = _edge(U, D, K)
    c, _ = R.apply(np.ones(n), ref, U, D, K)
    dev = np.abs(c[e:-e] - 1.0).max()
    print(f"{sr_in} -> {TARGET}: constant deviates by {dev:.1e}")
    assert dev <= 1e-14
    nyq = min(sr_in, TARGET) / 2
    for frac in (0.02, 0.3, 0.6, 0.7):
        y, _ = R.apply(_tone(frac * nyq, sr_in, n), ref, U, D, K)
        assert len(y) == R.out_len(n, U, D)
        err = R.db(np.abs(y - _tone(frac * nyq, TARGET, len(y)))[e:-e].max())
        print(f"{sr_in} -> {TARGET}: tone at {frac} of the lower Nyquist rate: {err:.1f} dB")
        assert err <= -80.0


@pytest.mark.parametrize("sr_in", [32000, 44100, 48000])        # (at 24000 the tone, 12127.5 Hz, lies above the input's Nyquist rate)
def test_stopband_tone_is_rejected(sr_in):
    (U, D, K, ref), _ = designed(sr_in)
    n = int(0.15 * sr_in)
    e = _edge(U, D, K)
    y, _ = R.apply(_tone(1.1 * TARGET / 2, sr_in, n), ref, U, D, K)
    rej = R.db(np.abs(y)[e:-e].max())
    print(f"{sr_in} -> {TARGET}: tone at 1.1 of the new Nyquist rate comes out at {rej:.1f} dB")
    assert rej <= -90.0


def test_output_length_rule():
    from tacotron2_amd.datasets.resample import Resampler, out_len
    for U, D in ((147, 160), (441, 320), (1, 2), (2, 1), (3, 2)):
        for n in (0, 1, 2, 159, 160, 161, 319, 320, 12345, 2 ** 33 + 7):
            assert out_len(n, U, D) == math.ceil(Fraction(n * U, D)) == R.out_len(n, U, D)
    rs = Resampler(22050, "cpu")
    assert rs.out_len(24000, 24000) == 22050 and rs.out_len(161, 24000) == 148 and rs.out_len(160, 24000) == 147


def test_agrees_with_scipy_resample_poly():
    sig = pytest.importorskip("scipy.signal")
    for sr_in in (24000, 16000, 44100):
        (U, D, K, ref), _ = designed(sr_in)
        n = int(0.15 * sr_in)
        nyq = min(sr_in, TARGET) / 2
        x = sum(a * _tone(f * nyq, sr_in, n, ph) for a, f, ph in ((0.4, 0.05, 0.1), (0.3, 0.21, 1.0), (0.2, 0.43, 2.0), (0.1, 0.66, 0.5)))
        y, _ = R.apply(x, ref, U, D, K)
        z = sig.resample_poly(x, U, D, window=("kaiser", 9.0))
        m = min(len(y), len(z))
        e = 3 * 10 * max(1, U // D + 1) + _edge(U, D, K)             # (scipy's filter reaches 10 max(U, D) taps each side)
        err = R.db(np.abs(y[:m] - z[:m])[e:-e].max())
        print(f"{sr_in} -> {TARGET}: against scipy.signal.resample_poly: {err:.1f} dB")
        assert err <= -80.0


def _write_wav(path, x, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.round(np.asarray(x) * 32767).astype("<i2").tobytes())


def test_table_limit_and_resample_false_name_the_file_and_the_rates(tmp_path):
    """A pair in lowest terms U / D whose table of U x 2K floats passes 2^20 is refused, by plan() with both rates and by the dataset
    with the file as well (44057 is coprime to 22050: 22050 phases x 64 taps; 44056 -> 22050 is 11025 / 22028: 705 600 floats, taken).
    `resample: false` refuses any file that is not at the model's rate."""
    from tacotron2_amd.datasets.resample import TABLE_LIMIT, plan
    from tacotron2_amd.datasets.tts_dataset import TTSDataset
    assert TABLE_LIMIT == 2 ** 20
    with pytest.raises(ValueError, match="44057.*22050"):
        plan(44057, 22050)
    U, D, K, _ = plan(44056, 22050)
    assert (U, D, K) == (11025, 22028, 32) and U * 2 * K <= TABLE_LIMIT
    x = 0.3 * _tone(440.0, 22050, 6000)
    _write_wav(tmp_path / "odd.wav", x, 44057)
    _write_wav(tmp_path / "libri.wav", x, 24000)
    _write_wav(tmp_path / "lj.wav", x, 22050)
    kw = dict(filenames=["odd.wav", "libri.wav", "lj.wav"], texts=["a", "b", "c"], base_dir=str(tmp_path), device="cpu")
    ds = TTSDataset(**kw)
    with pytest.raises(ValueError, match=r"odd\.wav.*44057.*22050"):
        ds.load_audio(0)
    strict = TTSDataset(resample=False, **kw)
    with pytest.raises(ValueError, match=r"libri\.wav.*24000.*22050.*resample"):
        strict.load_audio(1)
    assert len(strict.load_audio(2)) == 6000          # a file at the model's rate: today's path, with or without the switch
    assert np.array_equal(strict.load_audio(2), ds.load_audio(2))


def test_loader_host_half_knows_the_resampled_shape(tmp_path, capsys):
    """DeviceBatchLoader.host_batch on files of two rates (no GPU): rows of another rate stay at their own rate in the packed buffer,
    with the rate recorded, and n / frames are what the device WILL make of them - ceil(n_in U / D) + silence, as host integers."""
    from tacotron2_amd.datasets.tts_dataset import DeviceBatchLoader, TTSDataset
    rng = np.random.default_rng(0)
    lens, rates = [16000, 9000, 12800], [24000, 22050, 16000]
    for i, (n, sr) in enumerate(zip(lens, rates)):
        _write_wav(tmp_path / f"u{i}.wav", 0.1 * rng.standard_normal(n), sr)
    ds = TTSDataset(filenames=[f"u{i}.wav" for i in range(3)], texts=["a", "bb", "ccc"], base_dir=str(tmp_path), silence=512, trim=False,
                    device="cpu")
    hb = next(iter(DeviceBatchLoader(ds, batch_size=3, shuffle=False, drop_last=False, decode_threads=2)))
    assert hb.rates == [24000, None, 16000] and hb.n_in == [16000, 9000 + 512, 12800]
    assert hb.n == [16000 * 147 // 160 + 512, 9000 + 512, 12800 * 441 // 320 + 512]
    assert hb.frames == [1 + n // 256 for n in hb.n] and hb.T == max(hb.frames)
    assert hb.wav.shape == (3, 16000) and float(hb.wav[1, 9000:].abs().sum()) == 0.0 and float(hb.wav[2, 12800:].abs().sum()) == 0.0
    out = capsys.readouterr().out
    assert out.count("resampled on the device") == 1 and "22050 Hz" in out          # one line, at the first such file
