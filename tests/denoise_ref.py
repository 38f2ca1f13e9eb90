"""The rule of t2_denoise (include/tacotron2_amd.h) restated in numpy / scipy, with a `dtype` argument in the manner of
audio_ref.py: float64 is the reference the kernel is held to; float32 - the fp32 tables, scipy.fft in single precision, float32 sums -
is the restatement that anchors the tolerances.  Nothing here knows the kernel: the frames are rows of one strided view, the
transform is scipy's, the overlap-add a loop over the frames in ascending order.

The case list of the GPU test lives here (LENGTHS, STRENGTHS, signal, hum, hum_bias), so that F32_ERR is measured on exactly those
rows."""
import functools

import numpy as np
import scipy.fft

NFFT, HOP, BINS = 1024, 256, 513             # the header's T2_DENOISE_NFFT, T2_DENOISE_HOP; bins 0 .. 512
SHORT, FLAG_SHORT = NFFT // 2, 1             # a row of at most 512 samples has no reflection: copied
SR = 22050
# 0, 1, 512: short; 513: the shortest row with frames; 768, 1024, 5120: whole hops; 2149: odd; 4096 + 77: two tiles; 2 * 4096 + 513: three
# tiles, the middle one with halo frames on both sides
LENGTHS = (0, 1, 512, 513, 768, 1024, 2149, 4096 + 77, 2 * 4096 + 513, 5120)
STRENGTHS = (0.01, 0.5, 1.0)
HUM_N = 5120
SEED = 2251
HUM = ((1, 0.020, 0.3), (2, 0.012, 1.1), (3, 0.006, 2.0), (5, 0.003, 0.7))      # (harmonic of 1 / 64 cycles per sample, amplitude, phase)


@functools.lru_cache(maxsize=None)
def window():
    """The periodic Hann window as the fp32 table the kernel takes: made in float64, rounded once."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT, dtype=np.float64) / NFFT)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def twiddles():
    """(768, 2) float32: cos, sin of 2 pi k / 1024, made in float64 - what a radix-4 transform of 1024 points reads, k <= 3 * 255."""
    a = 2.0 * np.pi * np.arange(3 * NFFT // 4, dtype=np.float64) / NFFT
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def n_frames(n: int) -> int:
    return 0 if n <= SHORT else 1 + n // HOP


def interior_frames(n: int):
    """The frames whose span [256 t - 512, 256 t + 512) lies inside the row: t2m_frame_valid's rule."""
    return [t for t in range(n_frames(n)) if t * HOP - NFFT // 2 >= 0 and t * HOP + NFFT // 2 <= n]


def hum(n: int = HUM_N):
    """(n,) float32: a stationary buzz of period 64, a divisor of the hop - every interior frame sees the same samples, so their
    magnitudes ARE the bias.  One period is rounded to float32 and repeated, which keeps it exactly periodic."""
    i = np.arange(64, dtype=np.float64)
    period = sum(a * np.sin(2.0 * np.pi * h * i / 64.0 + ph) for h, a, ph in HUM).astype(np.float32)
    return np.tile(period, n // 64 + 1)[:n].copy()


def signal(n: int, with_hum: bool = True):
    """(n,) float32, audio_ref.signal's recipe: two sinusoids (one decaying) over a white floor of sigma = 0.01, plus the hum.
    SEED was picked from 2200, 2201, .. so that no reference magnitude of LENGTHS x STRENGTHS outside gated_cap's band lies within
    TOL["mag"] x max |m| of its threshold (threshold_margin; test_denoise_ref_host.py asserts it): a magnitude that passes the mag check
    then cannot sit on the other side of its threshold, which is what the check of `gated` by gated_cap presumes."""
    rng = np.random.default_rng(SEED + n % 997)
    t = np.arange(n, dtype=np.float64) / SR
    x = 0.3 * np.sin(2 * np.pi * 0.017 * SR * t) + 0.15 * np.sin(2 * np.pi * 0.11 * SR * t) * np.exp(-2.0 * t * SR / max(n, 1))
    x = x + 0.01 * rng.normal(size=n)
    if with_hum:
        x = x + hum(n).astype(np.float64)
    return x.astype(np.float32)


def frames(x, dtype=np.float64):
    """(F, 1024): the windowed frames of a row of more than 512 samples, reflect-padded by 512 at its own length."""
    x = np.asarray(x, dtype=dtype)
    p = np.pad(x, NFFT // 2, mode="reflect")
    F = n_frames(len(x))
    rows = np.lib.stride_tricks.as_strided(p, (F, NFFT), (HOP * p.strides[0], p.strides[0]))
    return rows * window().astype(dtype)


def magnitudes(x, dtype=np.float64):
    """(F, 513): m = sqrt(re^2 + im^2) of every frame; (0, 513) for a short row."""
    if len(x) <= SHORT:
        return np.zeros((0, BINS), dtype)
    spec = scipy.fft.rfft(frames(x, dtype), axis=1)
    return np.sqrt(spec.real * spec.real + spec.imag * spec.imag).astype(dtype)


def interior_mean(x):
    """(513,) float64: the mean over the interior frames of a row's float64 magnitudes - the bias of a vocoder's silence."""
    return magnitudes(x)[interior_frames(len(x))].mean(axis=0)


@functools.lru_cache(maxsize=None)
def hum_bias():
    """(513,) float32: the bias of the GPU test, from the hum's interior frames."""
    return interior_mean(hum()).astype(np.float32)


def envelope(n: int, dtype=np.float64):
    """(n,): the divisor - per sample the sum of window^2 over the frames that exist, ascending."""
    w2 = window().astype(dtype) ** 2
    env = np.zeros(n + NFFT, dtype)
    for t in range(n_frames(n)):
        env[t * HOP:t * HOP + NFFT] += w2
    return env[NFFT // 2:NFFT // 2 + n]


def envelope_min():
    """The smallest divisor over every n mod 256 (n = 513 .. 513 + 2 * 256: the row's end moves through two whole hops)."""
    return min(float(envelope(n).min()) for n in range(SHORT + 1, SHORT + 2 + 2 * HOP))


ENV_MIN = 0.2561                             # envelope_min(), rounded down to four digits, at the last sample of a row with n mod 256 =
                                             # 255, which lies under two frames alone: positive, so no clamp is needed


def denoise(x, bias, strength, dtype=np.float64):
    """The rule.  x (n,) float32, bias (513,) float32, strength a float.  Returns a dict: y (n,) in dtype, mag (F, 513) - before the
    gate -, thr (513,), g (F, 513), gated (the bins with g == 0), frames, flags."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    thr = (np.float32(strength) * np.asarray(bias, dtype=np.float32)).astype(dtype)          # one float32 product
    if n <= SHORT:
        return dict(y=x.astype(dtype), mag=np.zeros((0, BINS), dtype), thr=thr, g=np.zeros((0, BINS), dtype), gated=0, frames=0, flags=FLAG_SHORT)
    win = window().astype(dtype)
    spec = scipy.fft.rfft(frames(x, dtype), axis=1)
    m = np.sqrt(spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(m > thr[None, :], (m - thr[None, :]) / m, 0).astype(dtype)
    terms = (scipy.fft.irfft(spec * g, n=NFFT, axis=1).astype(dtype) * win).astype(dtype)
    acc, env, w2 = np.zeros(n + NFFT, dtype), np.zeros(n + NFFT, dtype), (win * win).astype(dtype)
    for t in range(len(terms)):                                                                # ascending t
        acc[t * HOP:t * HOP + NFFT] += terms[t]
        env[t * HOP:t * HOP + NFFT] += w2
    y = (acc[NFFT // 2:NFFT // 2 + n] / env[NFFT // 2:NFFT // 2 + n]).astype(dtype)
    return dict(y=y, mag=m, thr=thr, g=g, gated=int((g == 0).sum()), frames=len(terms), flags=0)


def gated_cap(ref: dict, tol: float) -> int:
    """The reference bins whose |m - thr| lies within tol relative of the threshold: a bin farther away cannot flip."""
    return int((np.abs(ref["mag"] - ref["thr"][None, :]) <= tol * ref["thr"][None, :]).sum())


def threshold_margin(ref: dict, tol: float) -> float:
    """The smallest |m - thr| / max |m| over the reference bins outside gated_cap's band; inf without one."""
    d = np.abs(ref["mag"] - ref["thr"][None, :])
    d = d[d > tol * np.broadcast_to(ref["thr"][None, :], d.shape)]
    return float(d.min() / ref["mag"].max()) if d.size else float("inf")


def rel(got, ref) -> float:
    """audio_ref.rel: max |got - ref| / max |ref|; 0 for two empty arrays, inf for a non-finite result."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return float("inf")
    if ref.size == 0:
        return 0.0
    top = float(np.abs(ref).max())
    return float(np.abs(got - ref).max() / top) if top > 0 else float(np.abs(got - ref).max())


def interior_db(y, x) -> float:
    """20 log10 of rms(y) / rms(x) over the samples that lie under interior frames alone."""
    n = len(x)
    ts = interior_frames(n)
    lo, hi = (ts[0] + 1) * HOP, (ts[-1] - 1) * HOP                      # sample i lies under the frames (i >> 8) - 1 .. (i >> 8) + 2
    a, b = np.asarray(y, np.float64)[lo:hi], np.asarray(x, np.float64)[lo:hi]
    return 10.0 * np.log10(max(float((a * a).mean()), 1e-300) / float((b * b).mean()))


# -----------------------------------------------------------------------------------------------------------------
# Tolerances, audio_ref.TOL's rule:  TOL[k] = 16 x F32_ERR[k],  F32_ERR[k] = the largest `rel` of the float32 run against the float64
# run over LENGTHS x STRENGTHS, measured on the CPU by measure_f32_err() and rounded up to two digits with >= 2 % of headroom;
# test_denoise_ref_host.py re-measures them.  The factor 16 covers what two correct float32 FFTs may differ by.
#   measured (worst case):  y 3.41e-7 n768_s1.0 | mag 1.44e-7 n8705 | roundtrip 3.16e-7 n8705
#   (y and roundtrip: the last samples of a row, where the divisor falls to ENV_MIN, carry up to four times a frame's rounding)
# -----------------------------------------------------------------------------------------------------------------
F32_ERR = {"y": 3.5e-7, "mag": 1.5e-7, "roundtrip": 3.3e-7}
TOL = {k: 16.0 * e for k, e in F32_ERR.items()}


def measure_f32_err():
    """{output: (worst rel of the float32 run against the float64 run, case)} over the GPU test's rows."""
    worst = {}

    def worse(key, e, name):
        if e > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (e, name)
    bias, zero = hum_bias(), np.zeros(BINS, np.float32)
    for n in LENGTHS:
        x = signal(n)
        worse("mag", rel(magnitudes(x, np.float32), magnitudes(x)), f"n{n}")
        worse("roundtrip", rel(denoise(x, zero, 1.0, np.float32)["y"], x), f"n{n}")
        for s in STRENGTHS:
            worse("y", rel(denoise(x, bias, s, np.float32)["y"], denoise(x, bias, s)["y"]), f"n{n}_s{s}")
    return worst
