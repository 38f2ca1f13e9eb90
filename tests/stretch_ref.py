"""t2_stretch restated in numpy (include/tacotron2_amd.h): WSOLA with every position an integer formed in integer
arithmetic, the search on a 10-bit quantised copy of the signal in int64 (the kernel's int32 sums are exact, so both pick the same
offset on every frame), the overlap-add in float64 from the float32 window table.  A restatement of the rule, not a port of the
kernel: one row at a time, no tiling, no chunks."""
import numpy as np


def cdiv(a: int, b: int) -> int:
    return -((-int(a)) // int(b))


def lengths(n: int, P: int, Q: int, N: int):
    """(n_out, M): the output samples and the frames of a row of n samples at tempo P / Q with the window N."""
    n_out = cdiv(int(n) * int(Q), P)
    return n_out, cdiv(n_out, N // 2) + 1


def centres(M: int, P: int, Q: int, N: int):
    """a_m = (m Hs P + Q / 2) div Q for m < M, Python integers."""
    Hs = N // 2
    return [(m * Hs * int(P) + int(Q) // 2) // int(Q) for m in range(M)]


def window(N: int) -> np.ndarray:
    """The periodic Hann window, float32 from fp64: w[k] = 0.5 - 0.5 cos(2 pi k / N)."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def quantise(x: np.ndarray) -> np.ndarray:
    """q[i] = rint(x[i] * 1023 / peak) in fp64 as int64; zeros when peak == 0 (or the row is empty)."""
    x = np.asarray(x, dtype=np.float32)
    peak = float(np.max(np.abs(x))) if len(x) else 0.0
    if peak == 0.0:
        return np.zeros(len(x), dtype=np.int64)
    return np.rint(x.astype(np.float64) * 1023.0 / np.float64(peak)).astype(np.int64)


def span(v: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """v~[lo .. hi): v with zeros outside [0, len(v))."""
    out = np.zeros(hi - lo, dtype=v.dtype)
    s, e = max(lo, 0), min(hi, len(v))
    if e > s:
        out[s - lo:e - lo] = v[s:e]
    return out


def scores(q: np.ndarray, a_m: int, c: int, N: int, D: int) -> np.ndarray:
    """score(d) for d = -D .. D, int64: sum_{k = -Hs .. Hs - 1} q~[a_m + d + k] q~[c + k]."""
    Hs = N // 2
    tmpl = span(q, c - Hs, c + Hs)
    region = span(q, a_m - D - Hs, a_m + D + Hs)
    return np.lib.stride_tricks.sliding_window_view(region, N) @ tmpl


def pick(sc: np.ndarray, D: int) -> int:
    """The d of the largest score; ties to the smaller |d|, then to the negative one."""
    best = sc.max()
    return min((int(e) - D for e in np.nonzero(sc == best)[0]), key=lambda d: (abs(d), d))


def positions(x: np.ndarray, P: int, Q: int, N: int, D: int, return_scores: bool = False):
    """p_m for m < M (int64 array); with return_scores also the largest |score| met (a Python integer)."""
    x = np.asarray(x, dtype=np.float32)
    Hs = N // 2
    _, M = lengths(len(x), P, Q, N)
    a = centres(M, P, Q, N)
    q = quantise(x)
    pos = np.zeros(M, dtype=np.int64)
    pos[0] = a[0]
    top = 0
    for m in range(1, M):
        sc = scores(q, a[m], int(pos[m - 1]) + Hs, N, D)
        top = max(top, int(np.abs(sc).max()))
        pos[m] = a[m] + pick(sc, D)
    return (pos, top) if return_scores else pos


def overlap_add(x: np.ndarray, pos: np.ndarray, n_out: int, N: int) -> np.ndarray:
    """y[m Hs + i] = w[Hs + i] x~[p_m + i] + w[i] x~[p_{m+1} - Hs + i] for m Hs + i < n_out, in float64 from the float32 table."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    Hs = N // 2
    w = window(N).astype(np.float64)
    y = np.zeros((len(pos) - 1) * Hs, dtype=np.float64)
    for m in range(len(pos) - 1):
        p0, p1 = int(pos[m]), int(pos[m + 1])
        y[m * Hs:(m + 1) * Hs] = w[Hs:] * span(x64, p0, p0 + Hs) + w[:Hs] * span(x64, p1 - Hs, p1)
    return y[:n_out]


def stretch(x: np.ndarray, P: int, Q: int = 1000, N: int = 1024, D: int = 256):
    """(y float64 (n_out,), pos int64 (M,)) of one row."""
    n_out, _ = lengths(len(x), P, Q, N)
    pos = positions(x, P, Q, N, D)
    return overlap_add(x, pos, n_out, N), pos


def tone(f0: float, sr: int = 22050, seconds: float = 1.0, seed: int = 0) -> np.ndarray:
    """The test signal of DESIGN 5.17: five harmonics of f0 with amplitudes 0.3 / k plus white noise of 0.003, float32."""
    t = np.arange(int(round(sr * seconds)), dtype=np.float64) / sr
    x = 0.3 * sum(np.sin(2.0 * np.pi * f0 * k * t) / k for k in range(1, 6))
    return (x + 0.003 * np.random.default_rng(seed).standard_normal(len(t))).astype(np.float32)


def spectral_peak(y: np.ndarray, sr: int):
    """(frequency of the largest bin of the Hann-windowed spectrum in Hz, the bin width in Hz)."""
    y = np.asarray(y, dtype=np.float64)
    Y = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    return float(np.argmax(Y)) * sr / len(y), sr / len(y)
