"""Per-character pitch and energy on the GPU: t2_char_variance (csrc/t2_variance.hip) against the float64 restatement of
tests/variance_ref.py, then analysis.char_variance, prosody.char_variances, the module surface and the driver.

Criteria, derived and not measured.  char_voiced and the integer stats (frames, voiced frames, consistent, unvoiced characters) must
be EQUAL to the reference: `f0 > 0` has no ties.  Every float32 output must lie within ONE float32 spacing of the reference value,
np.spacing(np.float32(|ref|)): a correctly rounded result lies within half a spacing, and the kernel's fp64 sum order and the
device's fp64 exp / log / sqrt differ from the host's by under 1e-12 relative, which can move a value across one rounding boundary
and no further.  The fp64 stats within 1e-12 relative: up to 4096 positive terms at 2^-53 each are 4.6e-13.  Two calls bit-identical.
Every test pitch lies in 60 .. 500 Hz, so p > 0 in both domains and no sum cancels.

Poison: behind every F_b the f0 rows hold 1000 Hz (an over-read would count as voiced) and the mel rows NaN; dur holds 2^30 behind
every N_b; the outputs are pre-filled with a sentinel that must survive where the rule says "not written"."""
import ctypes as C
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import variance_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_RTOL = 1e-12
INT_STATS = [0, 1, 8, 9]
SENTINEL = -7.0


def _dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def _kernel(f0, mel, dur, chars_len, frames_len, log_pitch, interpolate, dev, frames=True):
    """One t2_char_variance call on device tensors (any strides with a contiguous last dimension) -> dict of numpy arrays."""
    from tacotron2_amd import _lib
    B, T = f0.shape
    L, M = dur.shape[1], mel.shape[2]
    out = dict(pitch=torch.full((B, L), SENTINEL, device=dev), energy=torch.full((B, L), SENTINEL, device=dev),
               voiced=torch.full((B, L), -7, dtype=torch.int32, device=dev),
               stats=torch.full((B, R.NSTAT), float("nan"), dtype=torch.float64, device=dev))
    if frames:
        out.update(q=torch.full((B, T), SENTINEL, device=dev), e=torch.full((B, T), SENTINEL, device=dev))
    cl = torch.as_tensor(np.asarray(chars_len), dtype=torch.int32).to(dev)
    fl = torch.as_tensor(np.asarray(frames_len), dtype=torch.int32).to(dev)
    st = _lib.make("T2CharVariance", f0=f0, ld_f0=f0.stride(0), mel=mel, ld_b=mel.stride(0), ld_t=mel.stride(1), dur=dur,
                   ld_dur=dur.stride(0), B=B, T=T, L=L, M=M, log_pitch=int(log_pitch), interpolate=int(interpolate), chars_len=cl,
                   frames_len=fl, char_pitch=out["pitch"], char_energy=out["energy"], char_voiced=out["voiced"],
                   frame_pitch=out.get("q"), frame_energy=out.get("e"), stats=out["stats"])
    _lib.call("t2_char_variance", st, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _within_one_spacing(got, ref, label):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), label
    tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got - ref) / tol
    print(f"[variance] {label}: worst error {float(err.max()) if err.size else 0.0:.3f} float32 spacings /1")
    assert (err <= 1.0).all(), (label, np.argwhere(err > 1.0)[:8].tolist())


def _check(got, refs, frames_len, label):
    """The kernel's arrays of a batch against the reference dicts of its utterances."""
    for b, ref in enumerate(refs):
        F = len(ref["q"])
        assert np.array_equal(got["voiced"][b], ref["voiced"]), (label, b)
        assert got["stats"][b][INT_STATS].tolist() == ref["stats"][INT_STATS].tolist(), (label, b, got["stats"][b].tolist())
        _within_one_spacing(got["pitch"][b], ref["pitch"], f"{label} b={b} pitch")
        _within_one_spacing(got["energy"][b], ref["energy"], f"{label} b={b} energy")
        serr = np.abs(got["stats"][b] - ref["stats"]) / np.maximum(np.abs(ref["stats"]), 1e-300)
        print(f"[variance] {label} b={b}: stats relative error {float(serr.max()):.3e} /{STATS_RTOL:.0e}")
        assert np.isfinite(got["stats"][b]).all() and (serr <= STATS_RTOL).all(), (label, b, serr.tolist())
        if "q" in got:
            _within_one_spacing(got["q"][b, :F], ref["q"], f"{label} b={b} frame pitch")
            _within_one_spacing(got["e"][b, :F], ref["e"], f"{label} b={b} frame energy")
            assert (got["q"][b, F:] == SENTINEL).all() and (got["e"][b, F:] == SENTINEL).all(), (label, b, "written behind F_b")


def _poison(f0, mel, dur, chars_len, frames_len):
    for b in range(len(f0)):
        F, N = min(max(int(frames_len[b]), 0), f0.shape[1]), min(max(int(chars_len[b]), 0), dur.shape[1])
        f0[b, F:] = 1000.0
        mel[b, F:] = np.nan
        dur[b, N:] = 2 ** 30


def _spread(rng, N, F):
    """N durations >= 0 that sum to F (a cut of [0, F) at sorted random points)."""
    cuts = np.sort(rng.integers(0, F + 1, N - 1)) if N > 1 else np.zeros(0, dtype=np.int64)
    return np.diff(np.concatenate([[0], cuts, [F]])).astype(np.int32)


def _track(rng, F, share=0.6):
    """A track of F frames in 60 .. 500 Hz with unvoiced stretches (0, and a NaN and a negative value among them)."""
    f = rng.uniform(60.0, 500.0, F).astype(np.float32)
    off = rng.random(F) >= share
    f[off] = 0.0
    if F > 8:
        idx = np.nonzero(off)[0]
        if len(idx) > 1:
            f[idx[0]], f[idx[1]] = np.nan, -120.0
    return f


def _run_case(f0, mel, dur, chars_len, frames_len, label, dev, log_pitch=True, views=None):
    """Both interpolation settings of the kernel against the reference, each called twice (bit-identical)."""
    _poison(f0, mel, dur, chars_len, frames_len)
    f0_d, mel_d, dur_d = views if views is not None else (torch.from_numpy(f0).to(dev), torch.from_numpy(mel).to(dev),
                                                          torch.from_numpy(dur).to(dev))
    for interpolate in (False, True):
        refs = R.char_variance_batch(dur, chars_len, frames_len, f0, mel, log_pitch, interpolate)
        got = _kernel(f0_d, mel_d, dur_d, chars_len, frames_len, log_pitch, interpolate, dev)
        again = _kernel(f0_d, mel_d, dur_d, chars_len, frames_len, log_pitch, interpolate, dev)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (label, k, "two calls differ")
        _check(got, refs, frames_len, f"{label} interpolate={int(interpolate)}")


# (T, L, N, M): the smallest shape; the hand-worked size; across the 256-thread stride in T; in L too; a bin count across a wave
# boundary; both caps
SHAPES = [(1, 1, 1, 1), (7, 3, 3, 80), (257, 5, 5, 80), (300, 257, 257, 80), (512, 40, 40, 65), (4096, 4096, 9, 80)]


@pytest.mark.parametrize("T,L,N,M", SHAPES)
def test_kernel_equals_the_reference(T, L, N, M):
    dev = _dev()
    rng = np.random.default_rng(T * 31 + L)
    B = 2
    frames_len = [T, max(1, T - T // 3)]
    chars_len = [N, max(1, N - N // 2)]
    f0 = np.stack([_track(rng, T) for _ in range(B)])
    if T == 1:
        f0[0, 0], f0[1, 0] = 220.0, 0.0
    mel = rng.normal(-4.0, 2.0, (B, T, M)).astype(np.float32)
    dur = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        dur[b, :chars_len[b]] = _spread(rng, chars_len[b], frames_len[b])
    _run_case(f0, mel, dur, chars_len, frames_len, f"T={T} L={L} N={N} M={M}", dev, log_pitch=(T != 7))


def test_the_hand_worked_case_on_the_device():
    from test_variance_ref_host import DUR, F0, MEL
    dev = _dev()
    got = _kernel(torch.from_numpy(F0[None].copy()).to(dev), torch.from_numpy(MEL[None].copy()).to(dev),
                  torch.tensor([DUR], dtype=torch.int32, device=dev), [3], [7], False, True, dev)
    assert got["voiced"][0].tolist() == [2, 0, 1] and got["q"][0].tolist() == [100, 100, 200, 250, 300, 350, 400]
    assert got["pitch"][0].tolist() == [np.float32(400 / 3), 275, 375]
    np.testing.assert_allclose(got["energy"][0], [10, 22.5, 32.5], rtol=1e-6)
    assert got["stats"][0][[0, 1, 2, 3, 4, 5, 8, 9]].tolist() == [7, 3, 700, 210000, 1700, 495000, 1, 1]


VOICING = ["none", "one", "first", "last", "gap", "alternating"]


@pytest.mark.parametrize("pattern", VOICING)
def test_voicing_patterns(pattern):
    dev = _dev()
    rng = np.random.default_rng(VOICING.index(pattern))
    T, L, M, F = 900, 12, 80, 870
    f0 = np.zeros((1, T), dtype=np.float32)
    hz = rng.uniform(60.0, 500.0, T).astype(np.float32)
    at = {"none": [], "one": [431], "first": [0], "last": [F - 1], "gap": [3, 4, 5, 40, 41, 860, 861],    # 41 .. 860: three blocks
          "alternating": list(range(0, F, 2))}[pattern]
    f0[0, at] = hz[at]
    mel = rng.normal(-4.0, 2.0, (1, T, M)).astype(np.float32)
    dur = _spread(rng, L, F)[None].copy()
    _run_case(f0, mel, dur, [L], [F], f"voicing {pattern}", dev)


def test_durations_with_zeros_short_and_long():
    """Zeros as argmax mode produces them; the durations sum below and above F_b: consistent is 0 and the spans are clipped."""
    dev = _dev()
    rng = np.random.default_rng(11)
    T, L, M = 300, 9, 80
    f0 = np.stack([_track(rng, T) for _ in range(3)])
    mel = rng.normal(-4.0, 2.0, (3, T, M)).astype(np.float32)
    dur = np.array([[0, 50, 0, 0, 120, 1, 0, 129, 0],          # sums to 300 = F
                    [10, 0, 40, 0, 0, 30, 20, 0, 5],           # 105 < F = 280: the tail of the utterance belongs to nobody
                    [100, 0, 150, -30, 90, 0, 2 ** 30, 7, 0]], dtype=np.int32)      # far above F = 300: clipped, later spans empty
    frames_len = [300, 280, 300]
    _run_case(f0, mel, dur, [9, 9, 9], frames_len, "zeros / short / long", dev)
    refs = R.char_variance_batch(dur, [9, 9, 9], frames_len, f0, mel)
    assert [r["stats"][8] for r in refs] == [1, 0, 0]


def test_ragged_batch_with_empty_utterances():
    dev = _dev()
    rng = np.random.default_rng(12)
    B, T, L, M = 5, 270, 20, 80
    chars_len, frames_len = [20, 0, 7, 13, -2], [270, 100, 0, 131, 5000]
    f0 = np.stack([_track(rng, T) for _ in range(B)])
    mel = rng.normal(-4.0, 2.0, (B, T, M)).astype(np.float32)
    dur = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        N, F = min(max(chars_len[b], 0), L), min(max(frames_len[b], 0), T)
        if N:
            dur[b, :N] = _spread(rng, N, F)
    _run_case(f0, mel, dur, chars_len, frames_len, "ragged B=5", dev)


def test_batch_rows_further_apart_than_their_extent():
    dev = _dev()
    rng = np.random.default_rng(13)
    B, T, L, M = 3, 140, 10, 65
    frames_len, chars_len = [140, 97, 120], [10, 4, 9]
    f0 = np.stack([_track(rng, T) for _ in range(B)])
    mel = rng.normal(-4.0, 2.0, (B, T, M)).astype(np.float32)
    dur = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        dur[b, :chars_len[b]] = _spread(rng, chars_len[b], frames_len[b])
    _poison(f0, mel, dur, chars_len, frames_len)
    big_f0 = torch.full((B, T + 37), 1000.0, device=dev)
    big_mel = torch.full((B, T + 5, M + 15), float("nan"), device=dev)
    big_dur = torch.full((B, L + 3), 2 ** 30, dtype=torch.int32, device=dev)
    big_f0[:, :T], big_mel[:, :T, :M], big_dur[:, :L] = torch.from_numpy(f0).to(dev), torch.from_numpy(mel).to(dev), \
        torch.from_numpy(dur).to(dev)
    views = (big_f0[:, :T], big_mel[:, :T, :M], big_dur[:, :L])
    assert not any(v.is_contiguous() for v in views)
    _run_case(f0, mel, dur, chars_len, frames_len, "strided views", dev, views=views)
    # the module API takes the same views, and lengths of any integer type
    from tacotron2_amd import analysis
    for interpolate in (False, True):
        out, stats = analysis.char_variance(views[2], torch.tensor(chars_len, device=dev), torch.tensor(frames_len, dtype=torch.int16,
                                            device=dev), views[0], views[1], interpolate=interpolate, return_frames=True)
        got = _kernel(*views, chars_len, frames_len, True, interpolate, dev)
        assert out["pitch"].dtype == out["energy"].dtype == torch.float32 and out["voiced"].dtype == torch.int32
        assert stats.dtype == torch.float64 and stats.shape == (B, 10)
        for k, name in (("pitch", "pitch"), ("energy", "energy"), ("voiced", "voiced")):
            assert np.array_equal(out[name].cpu().numpy(), got[k])
        assert np.array_equal(stats.cpu().numpy(), got["stats"])
        for b, F in enumerate(frames_len):          # the API's frame arrays are zero behind F_b
            assert np.array_equal(out["pitch_frames"][b, :F].cpu().numpy(), got["q"][b, :F]) and not out["pitch_frames"][b, F:].any()
            assert np.array_equal(out["energy_frames"][b, :F].cpu().numpy(), got["e"][b, :F]) and not out["energy_frames"][b, F:].any()
    out, _ = analysis.char_variance(views[2], torch.tensor(chars_len, device=dev), torch.tensor(frames_len, device=dev), views[0], views[1])
    assert sorted(out) == ["energy", "pitch", "voiced"]
    with pytest.raises(ValueError, match="device of the signals"):
        analysis.char_variance(views[2], torch.tensor(chars_len), torch.tensor(frames_len, device=dev), views[0], views[1])


def test_argument_errors_launch_nothing():
    from tacotron2_amd import _lib
    dev = _dev()
    lib = _lib.lib()
    good = dict(B=2, T=8, L=4, M=3, log_pitch=1, interpolate=0, ld_f0=8, ld_b=24, ld_t=3, ld_dur=4)
    cases = [(dict(T=4097, ld_f0=4097, ld_b=4097 * 3), None, b"T2_VAR_MAX_T"), (dict(L=4097, ld_dur=4097), None, b"T2_VAR_MAX_L"),
             (dict(B=0), None, b">= 1"), (dict(M=0), None, b">= 1"), (dict(T=0), None, b">= 1"), (dict(L=0), None, b">= 1"),
             (dict(log_pitch=2), None, b"0 or 1"), (dict(interpolate=-1), None, b"0 or 1"),
             (dict(ld_f0=7), None, b"ld_f0"), (dict(ld_dur=3), None, b"ld_dur"), (dict(ld_t=2), None, b"ld_t"),
             (dict(ld_b=23), None, b"ld_b")] + [({}, name, b"null") for name in ("f0", "mel", "dur", "chars_len", "frames_len",
                                                                                 "char_pitch", "char_energy", "char_voiced", "stats")]
    for change, null, word in cases:
        kw = dict(good, **change)
        pitch, energy = torch.full((2, 4097), SENTINEL, device=dev), torch.full((2, 4097), SENTINEL, device=dev)
        voiced = torch.full((2, 4097), -7, dtype=torch.int32, device=dev)
        stats = torch.full((2, 10), SENTINEL, dtype=torch.float64, device=dev)
        ptr = dict(f0=torch.full((2, 4097), 100.0, device=dev), mel=torch.zeros(2, 4097, 3, device=dev),
                   dur=torch.ones(2, 4097, dtype=torch.int32, device=dev), chars_len=torch.ones(2, dtype=torch.int32, device=dev),
                   frames_len=torch.ones(2, dtype=torch.int32, device=dev), char_pitch=pitch, char_energy=energy, char_voiced=voiced,
                   stats=stats)
        if null:
            ptr[null] = None
        st = _lib.make("T2CharVariance", frame_pitch=None, frame_energy=None, **ptr, **kw)
        assert lib.t2_char_variance(C.addressof(st), None) == 1, (change, null)            # T2_ERR_ARG
        assert word in lib.t2_last_error() and b"t2_char_variance" in lib.t2_last_error(), lib.t2_last_error()
        torch.cuda.synchronize()
        assert bool((pitch == SENTINEL).all()) and bool((energy == SENTINEL).all()) and bool((voiced == -7).all()) \
            and bool((stats == SENTINEL).all())                                             # nothing ran
        with pytest.raises(_lib.T2Error):
            _lib.call("t2_char_variance", st, None)


# ---- end to end: the meter's track, the module surface ------------------------------------------------------------------------------
SR, HOP = 22050, 256


def _harmonic(hz_per_stretch, samples_per_stretch, seed=0):
    """Stretches of a harmonic signal (fundamental and two overtones) with a continuous phase, a little noise."""
    rng = np.random.default_rng(seed)
    f = np.repeat(np.asarray(hz_per_stretch, dtype=np.float64), samples_per_stretch)
    ph = 2 * np.pi * np.cumsum(f) / SR
    x = 0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph) + 0.08 * np.sin(3 * ph) + 0.002 * rng.normal(size=len(f))
    return x.astype(np.float32)


def _reference_of_the_track(meter, wavs, mel, mel_len, dur, chars_len, log_pitch, interpolate):
    f0, _ = meter.tracks(wavs)
    T = f0.shape[1]
    return R.char_variance_batch(dur.cpu().numpy(), chars_len.cpu().numpy(), mel_len.cpu().numpy(), f0.cpu().numpy(),
                                 mel[:, :T].cpu().numpy(), log_pitch, interpolate)


@pytest.mark.parametrize("smooth", [True, False])
def test_char_variances_of_a_harmonic_signal(smooth):
    from tacotron2_amd import prosody
    from tacotron2_amd.datasets.logmel import TacotronMelSpectrogram
    dev = _dev()
    meter = prosody.ProsodyMeter(SR, dev, smooth=smooth)
    sigs = [_harmonic([110, 220, 165], 8820), _harmonic([165, 110, 220], 7000, seed=1)]
    wavs = [torch.from_numpy(s).to(dev) for s in sigs]
    logmel = TacotronMelSpectrogram(device=dev)
    mels = [logmel(w) for w in wavs]
    mel_len = torch.tensor([len(m) for m in mels], dtype=torch.int32, device=dev)
    assert mel_len.tolist() == [1 + len(s) // HOP for s in sigs] == [104, 83]
    mel = torch.nn.utils.rnn.pad_sequence(mels, batch_first=True)
    dur = torch.tensor([[34, 35, 35, 0], [27, 28, 20, 8]], dtype=torch.int32, device=dev)          # hand-given, summing to 104 and 83
    chars_len = torch.tensor([3, 4], device=dev)
    for log_pitch, interpolate in ((True, False), (False, True)):
        out, stats = prosody.char_variances(meter, wavs, mel, mel_len, dur, chars_len, log_pitch=log_pitch, interpolate=interpolate,
                                            return_frames=True)
        refs = _reference_of_the_track(meter, wavs, mel, mel_len, dur, chars_len, log_pitch, interpolate)
        got = dict(pitch=out["pitch"].cpu().numpy(), energy=out["energy"].cpu().numpy(), voiced=out["voiced"].cpu().numpy(),
                   stats=stats.cpu().numpy())
        _check(got, refs, mel_len.tolist(), f"harmonic smooth={smooth} log={log_pitch} interpolate={interpolate}")
        p = out["pitch"].cpu().numpy()
        assert stats[:, 8].tolist() == [1, 1] and bool((out["voiced"][0, :3] > 10).all())
        print(f"[variance] harmonic smooth={smooth} log={log_pitch} interpolate={interpolate}: pitch {p.tolist()}")
        if not smooth:
            # 220 > 165 > 110 Hz: characters 2 > 3 > 1.  Asserted on the raw YIN track only: the Viterbi decode allows a
            # quarter octave per frame, so across a STEP of an octave it keeps its lag and reads the 220 Hz stretch as 110 Hz (the
            # float64 restatement of tests/pitch_ref.py does the same on this signal) - the tracker's accuracy is not under test here
            assert p[0, 1] > p[0, 2] > p[0, 0] > 0, p[0]
            assert p[1, 2] > p[1, 0] > p[1, 1] > 0, p[1]
    with pytest.raises(ValueError, match="not the signals the mels came from"):
        prosody.char_variances(meter, [wavs[0], wavs[1][:-HOP]], mel, mel_len, dur, chars_len)


def test_model_variances_are_durations_plus_the_meters_track():
    from test_gpu_durations import _batch, _tiny_model
    from tacotron2_amd import prosody
    dev = _dev()
    m = _tiny_model(1, dev)
    ci, lens, mel, tl = _batch(dev)
    wavs = [torch.from_numpy(_harmonic([140 + 60 * k], (int(f) - 1) * HOP + 10 * k, seed=k)).to(dev) for k, f in enumerate(tl.tolist())]
    meter = prosody.ProsodyMeter(SR, dev, smooth=True)
    m.train()
    calls = m._calls
    dur, var, stats = m.variances(ci, lens, mel, tl, wavs, meter, interpolate=True, return_frames=True)
    assert m.training and m._calls == calls + 1
    m._calls = calls          # (the prenet's dropout masks, on in eval mode too, are drawn from the seed and the call count)
    d0, s0, _ = m.durations(ci, lens, mel, tl)
    assert torch.equal(dur, d0) and torch.equal(var["alignment_stats"], s0)
    assert sorted(var) == ["alignment_stats", "energy", "energy_frames", "pitch", "pitch_frames", "voiced"]
    refs = _reference_of_the_track(meter, wavs, mel, tl, dur, lens, True, True)
    got = dict(pitch=var["pitch"].cpu().numpy(), energy=var["energy"].cpu().numpy(), voiced=var["voiced"].cpu().numpy(),
               stats=stats.cpu().numpy())
    _check(got, refs, tl.tolist(), "model.variances")
    assert stats[:, 0].tolist() == tl.tolist() and stats[:, 8].tolist() == [1, 1, 1]


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"


def _run(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _moments(xs):
    x = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in xs])
    return len(x), float(x.mean()), float(x.std()), float(x.min()), float(x.max())


def test_cli_duration_export_with_variances(tmp_path):
    """The corpus and the three-step model of test_gpu_durations.py's driver test."""
    sr = 22050
    speech = tmp_path / "wavs"
    speech.mkdir()
    rng = np.random.default_rng(0)
    rows = []
    for i in range(6):
        k = sr // 2 + 997 * i
        x = 0.3 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(k) / sr) + 0.01 * rng.normal(size=k)
        with wave.open(str(speech / f"u{i}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes((x * 32767).astype("<i2").tobytes())
        rows.append(f"Utterance number {i}{', and a few more words' * (i % 3)}, Dr. Who says hi!|u{i}.wav|{i % 4}")
    (tmp_path / "train.csv").write_text("\n".join(["text|wav|speaker_id"] + rows[:4]) + "\n")
    (tmp_path / "val.csv").write_text("\n".join(["text|wav|speaker_id"] + rows[4:]) + "\n")
    cfg = {"dataset": {"train": str(tmp_path / "train.csv"), "val": str(tmp_path / "val.csv"),
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^",
                                         "silence": 512, "trim": False, "num_mels": 80, "cache": True}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "precision": "16-mixed",
                        "args": {"max_steps": 6, "val_check_interval": 0.5}},
           "model": {"scheduler_milestones": [0.5, 0.75],
                     "args": {"prenet_dim": 32, "att_rnn_dim": 64, "att_dim": 32, "rnn_hidden_dim": 64, "postnet_dim": 64,
                              "dropout": 0.5, "char_embedding_dim": 64, "encoder_kernel_size": 5}},
           "extensions": {"speaker_tokens": {"active": True, "num_speakers": 4}, "controls": {"active": False}}}
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps(cfg))
    res = tmp_path / "res"
    _run(["--config", str(cfgp), "--device", "0", "train", "--speech-dir", "unused", "--results-dir", str(res), "--synthetic",
          "--max-steps", "3"])
    ck = str(res / "final.ckpt")
    plain, full = tmp_path / "dur", tmp_path / "var"
    base = ["--config", str(cfgp), "--device", "0", "duration-export", "--speech-dir", str(speech), "--checkpoint", ck]
    _run(base + ["--results-dir", str(plain)])
    _run(base + ["--results-dir", str(full), "--variances", "--frame-level"])
    names = [f"u{i}.wav" for i in range(6)]
    # the durations do not know about the option
    assert sorted(os.listdir(plain)) == sorted([f"{n}.dur.npy" for n in names] + ["durations.csv"])
    for f in os.listdir(plain):
        assert (plain / f).read_bytes() == (full / f).read_bytes(), f
    exts = [".dur.npy", ".pitch.npy", ".energy.npy", ".pitch_frames.npy", ".energy_frames.npy"]
    assert sorted(os.listdir(full)) == sorted([n + e for n in names for e in exts] + ["durations.csv", "variances.csv",
                                                                                      "variance_stats.json", "variances_dropped.csv"])
    assert (full / "variances_dropped.csv").read_text().splitlines() == ["wav|reason"]
    got = {n: {e: np.load(full / (n + e)) for e in exts} for n in names}
    lines = (full / "variances.csv").read_text().splitlines()
    assert lines[0] == "wav|n_chars|n_frames|n_voiced|chars_unvoiced|pitch_mean|pitch_std|energy_mean|energy_std" and len(lines) == 7
    for line in lines[1:]:
        wav, n_chars, n_frames, n_voiced, unvoiced, pm, ps, em, es = line.split("|")
        g = got[wav]
        assert all(g[e].dtype == np.float32 for e in exts[1:])
        assert g[".pitch.npy"].shape == g[".energy.npy"].shape == g[".dur.npy"].shape == (int(n_chars),)
        assert g[".pitch_frames.npy"].shape == g[".energy_frames.npy"].shape == (int(n_frames),) == (int(g[".dur.npy"].sum()),)
        qf = g[".pitch_frames.npy"]
        assert int(n_voiced) == int((qf != 0).sum()) > 0 and int(unvoiced) == int((g[".pitch.npy"] == 0).sum())
        assert abs(float(pm) - qf[qf != 0].astype(np.float64).mean()) < 2e-6 and float(em) > 0 and float(ps) >= 0 and float(es) >= 0
    # the module API on the same batches gives the same files
    from tacotron2_amd import prosody
    from tacotron2_amd.datasets.tts_dataset import TTSDataset, collate
    from tacotron2_amd.model.tts_model import TTSModel
    from tacotron2_amd.run.common import model_kwargs
    from tacotron2_amd.run.train import _to_dev
    dev = _dev()
    model = TTSModel.load_from_checkpoint(ck, device=dev, **model_kwargs(cfg))
    model.eval()
    meter = prosody.ProsodyMeter(sr, dev, smooth=True)
    pre = dict(cfg["dataset"]["preprocessing"], cache=False)
    texts = [r.split("|")[0] for r in rows]
    for idx in ([0, 1, 2, 3], [4, 5]):
        ds = TTSDataset(filenames=[names[i] for i in idx], texts=[texts[i] for i in idx], base_dir=str(speech),
                        speaker_ids=[i % 4 for i in idx], include_filename=True, include_audio=True, device=dev, **pre)
        items = collate([ds[k] for k in range(len(idx))])
        b = _to_dev(items, dev)
        wavs = [torch.from_numpy(a).to(dev) for a in items[2]["audio"]]
        dur, var, stats = model.variances(b["chars_idx"], b["chars_idx_len"], b["mel_spectrogram"], b["mel_spectrogram_len"], wavs, meter,
                                          speaker_id=b["speaker_id"], return_frames=True)
        for k, i in enumerate(idx):
            N, F = int(b["chars_idx_len"][k]), int(b["mel_spectrogram_len"][k])
            g = got[names[i]]
            assert np.array_equal(dur[k, :N].cpu().numpy(), g[".dur.npy"]), names[i]
            assert np.array_equal(var["pitch"][k, :N].cpu().numpy(), g[".pitch.npy"]), names[i]
            assert np.array_equal(var["energy"][k, :N].cpu().numpy(), g[".energy.npy"]), names[i]
            assert np.array_equal(var["pitch_frames"][k, :F].cpu().numpy(), g[".pitch_frames.npy"]), names[i]
            assert np.array_equal(var["energy_frames"][k, :F].cpu().numpy(), g[".energy_frames.npy"]), names[i]
    # variance_stats.json: the train rows only, against a float64 recomputation from the written (float32) files
    js = json.loads((full / "variance_stats.json").read_text())
    assert js["statistics_from"] == "train" and js["meter"]["smooth"] is True and js["meter"]["hop"] == 256
    assert js["options"] == dict(mode="monotonic", pitch_domain="log", interpolate_pitch=False, frame_level=True, smooth_pitch=True)
    assert js["counts"] == dict(train=dict(utterances=4, measured=4, dropped=0), val=dict(utterances=2, measured=2, dropped=0))
    train = [got[n] for n in names[:4]]
    want = dict(pitch=dict(char=_moments([g[".pitch.npy"][g[".pitch.npy"] != 0] for g in train]),
                           frame=_moments([g[".pitch_frames.npy"][g[".pitch_frames.npy"] != 0] for g in train])),
                energy=dict(char=_moments([g[".energy.npy"][g[".dur.npy"] > 0] for g in train]),
                            frame=_moments([g[".energy_frames.npy"] for g in train])))
    for what in ("pitch", "energy"):
        for level in ("char", "frame"):
            s, (n, mean, std, lo, hi) = js[what][level], want[what][level]
            print(f"[variance] stats {what} {level}: count {s['count']}, mean {s['mean']:.9f} (files: {mean:.9f}), std {s['std']:.6f}")
            assert s["count"] == n > 0 and abs(s["mean"] - mean) <= 1e-6 * abs(mean), (what, level, s, mean)
            assert abs(s["std"] - std) <= 1e-4 * max(std, 1e-3) and s["min"] == lo and s["max"] == hi, (what, level, s, std, lo, hi)
