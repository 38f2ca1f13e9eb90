"""t2_psola restated in numpy (include/tacotron2_amd.h): TD-PSOLA with every mark an integer formed in integer
arithmetic - the analysis marks a chain of small argmaxes over the input floats, the synthesis marks a chain in 1/256-sample fixed
point -, the overlap-add in float64 from the float32 window table.  A restatement of the rule, not a port of the kernel: one row at
a time, no staging, no waves."""
import numpy as np

ONE = 65536                                   # rho = 1 in Q16
RHO_RANGE = (16384, 262144)
LAG_RANGE = (16, 4096)


def table() -> np.ndarray:
    """W[u] = 0.5 - 0.5 cos(pi u / 1024), u = 0 .. 1024, float32 from fp64: W[u] + W[1024 - u] = 1 up to the rounding."""
    return (0.5 - 0.5 * np.cos(np.pi * np.arange(1025, dtype=np.float64) / 1024.0)).astype(np.float32)


def frames(n: int, T: int, hop: int) -> int:
    """Tb = min(T, 1 + n / hop): the frames of lag and rho that a row of n samples reads."""
    return min(int(T), 1 + int(n) // int(hop))


def frame(s: int, hop: int, Tb: int) -> int:
    """t(s) = min((s + hop / 2) / hop, Tb - 1)."""
    return min((int(s) + hop // 2) // hop, Tb - 1)


def rho_row(rho, T: int) -> np.ndarray:
    return np.full(T, int(rho), dtype=np.int64) if np.ndim(rho) == 0 else np.asarray(rho, dtype=np.int64)


def accepted(n: int, n_max: int, lag, rho, hop: int) -> bool:
    """The row is run, not refused: 0 <= n <= n_max, every read lag in {0} or 16 .. 4096, every voiced read rho in 16384 .. 262144."""
    if n < 0 or n > n_max:
        return False
    lag = np.asarray(lag, dtype=np.int64)
    Tb = frames(n, len(lag), hop)
    l, r = lag[:Tb], rho_row(rho, len(lag))[:Tb]
    v = l != 0
    return bool(np.all((l[v] >= LAG_RANGE[0]) & (l[v] <= LAG_RANGE[1])) and np.all((r[v] >= RHO_RANGE[0]) & (r[v] <= RHO_RANGE[1])))


def analysis_marks(x, lag, hop: int = 256, U=None) -> np.ndarray:
    """a_0 .. a_K (int64, K + 1 entries, a_K = n the terminal mark)."""
    x = np.asarray(x, dtype=np.float32)
    lag = np.asarray(lag, dtype=np.int64)
    n, U = len(x), hop // 2 if U is None else int(U)
    Tb = frames(n, len(lag), hop)
    per = lambda s: int(lag[frame(s, hop, Tb)])
    a = [0]
    while True:
        step = per(a[-1]) or U
        c = a[-1] + step
        if c >= n:
            a.append(n)
            return np.array(a, dtype=np.int64)
        pc = per(c)
        if pc > 0:
            d = min(pc, step) // 4
            lo, hi = c - d, min(c + d, n - 1)
            a.append(lo + int(np.argmax(x[lo:hi + 1])))          # the first of equal maxima
        else:
            a.append(c)


def synthesis_marks(a, lag, rho, hop: int = 256):
    """(r_0 .. r_J, k(0) .. k(J)), int64, J + 1 entries each; r_J = n = a_K and k(J) = K."""
    a = [int(v) for v in a]
    lag = np.asarray(lag, dtype=np.int64)
    rho = rho_row(rho, len(lag))
    K, n = len(a) - 1, a[-1]
    Tb = frames(n, len(lag), hop)
    r, km, s, k = [0], [0], 0, 0
    while True:
        t = frame(r[-1], hop, Tb)
        q = int(rho[t]) if lag[t] > 0 else ONE
        s += ((a[km[-1] + 1] - a[km[-1]]) * q) >> 8
        rn = (s + 128) >> 8
        if rn >= n:
            r.append(n)
            km.append(K)
            return np.array(r, dtype=np.int64), np.array(km, dtype=np.int64)
        while k + 1 <= K - 1 and abs(a[k + 1] - rn) < abs(a[k] - rn):     # a tie keeps the smaller k
            k += 1
        r.append(rn)
        km.append(k)


def overlap_add(x, a, r, km):
    """(y float64 (n,), G): y = sum_j w_j x[a_k + e] / max(sum_j w_j, 1), G the largest number of grains over one sample."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    W = table().astype(np.float64)
    n, K = len(x64), len(a) - 1
    num, den, cnt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for j in range(len(r)):
        k, rj = int(km[j]), int(r[j])
        ak = int(a[k])
        L = ak - int(a[k - 1]) if k > 0 else 0
        R = int(a[k + 1]) - ak if k < K else 0
        e = np.arange(max(min(-L + 1, 0), -rj), min(max(R, 1), n - rj), dtype=np.int64)      # -L < e < 0, e = 0, 0 < e < R; 0 <= r_j + e < n
        if not len(e):
            continue
        w = np.ones(len(e))
        neg, pos = e < 0, e > 0
        if L > 0:
            w[neg] = W[((L + e[neg]) * 1024) // L]
        if R > 0:
            w[pos] = W[1024 - (e[pos] * 1024) // R]
        num[rj + e] += w * x64[ak + e]
        den[rj + e] += w
        cnt[rj + e] += 1
    return num / np.maximum(den, 1.0), int(cnt.max(initial=0))


def psola(x, lag, rho=ONE, hop: int = 256, U=None):
    """(y float64 (n,), a, r, kmap, G) of one row."""
    a = analysis_marks(x, lag, hop, U)
    r, km = synthesis_marks(a, lag, rho, hop)
    y, G = overlap_add(x, a, r, km)
    return y, a, r, km, G


def pitch_ratio(lag, n: int, semitones: float = 0.0, pitch_range: float = 1.0, hop: int = 256) -> np.ndarray:
    """analysis.pitch_ratio of one row in numpy float64: Q16 int64 (T,)."""
    lag = np.asarray(lag, dtype=np.int64)
    Tb = frames(n, len(lag), hop)
    out = np.full(len(lag), ONE, dtype=np.int64)
    v = (lag > 0) & (np.arange(len(lag)) < Tb)
    if not v.any():
        return out
    if pitch_range == 1.0:
        out[v] = int(round(ONE * 2.0 ** (-semitones / 12.0)))
        return out
    lf = -np.log(lag[v].astype(np.float64))
    rho = np.exp((1.0 - pitch_range) * (lf - lf.mean()) - semitones * np.log(2.0) / 12.0)
    out[v] = np.clip(np.rint(rho * ONE), *RHO_RANGE).astype(np.int64)
    return out


def fold_lags(cm, lag, tau_min: int, thr: float) -> np.ndarray:
    """analysis.fold_lags of one row in numpy: cm (T, tau_max + 1) float32, lag (T,) -> int64 (T,).  A voiced lag L becomes the
    smallest of its sub-multiples that YIN's own threshold accepts: for m = 8 .. 2 in turn, c = (L + m / 2) / m, and the first m at
    which the smallest cm over the lags c - 1, c, c + 1 inside [tau_min, tau_max) lies under thr takes that lag (the first of equal
    minima); L stays where no m does."""
    cm = np.asarray(cm, dtype=np.float32)
    out = np.asarray(lag, dtype=np.int64).copy()
    tau_max = cm.shape[1] - 1
    for t, L in enumerate(out):
        if L <= 0:
            continue
        for m in range(8, 1, -1):
            c = (int(L) + m // 2) // m
            cand = [k for k in (c - 1, c, c + 1) if tau_min <= k < tau_max]
            if not cand:
                continue
            v = [cm[t, k] for k in cand]
            if min(v) < np.float32(thr):
                out[t] = cand[int(np.argmin(v))]
                break
    return out


# ---- the test signals of DESIGN 5.18 and what is measured on them -----------------------------------------------------------------------
VOWELS = ((100, 1000.0, 200.0), (147, 900.0, 250.0), (220, 1200.0, 220.0))     # (period, formant Hz, bandwidth Hz)


def vowel(period: int, formant: float, bandwidth: float, n: int = 12000, sr: int = 22050, amp: float = 0.05) -> np.ndarray:
    """A pulse train of `period` samples through a two-pole resonator, float32: a steady synthetic vowel."""
    rr, th = np.exp(-np.pi * bandwidth / sr), 2.0 * np.pi * formant / sr
    m = np.arange(2000, dtype=np.float64)
    h = rr ** m * np.sin((m + 1.0) * th) / np.sin(th)
    p = np.zeros(n)
    p[period // 2::period] = 1.0
    return (amp * np.convolve(p, h)[:n]).astype(np.float32)


def spectrum(y, n_fft: int = 8000):
    """|FFT| of the Hann-windowed middle n_fft samples."""
    y = np.asarray(y, dtype=np.float64)
    s = (len(y) - n_fft) // 2
    return np.abs(np.fft.rfft(y[s:s + n_fft] * np.hanning(n_fft)))


def fundamental(y, sr: int = 22050, n_fft: int = 8000, strong: float = 0.05):
    """(Hz, bin width): the lowest local maximum of the spectrum that reaches `strong` times the largest bin."""
    Y = spectrum(y, n_fft)
    for i in range(2, len(Y) - 1):
        if Y[i] >= strong * Y.max() and Y[i] >= Y[i - 1] and Y[i] > Y[i + 1]:
            return i * sr / n_fft, sr / n_fft
    raise AssertionError("no harmonic")


def centroid(y, sr: int = 22050, n_fft: int = 8000, band=(400.0, 2500.0)) -> float:
    """The power-weighted mean frequency over `band`."""
    P = spectrum(y, n_fft) ** 2
    f = np.arange(len(P)) * sr / n_fft
    m = (f >= band[0]) & (f <= band[1])
    return float((f[m] * P[m]).sum() / P[m].sum())


def resampled(x, ratio: float) -> np.ndarray:
    """x read `1 / ratio` times as fast (linear interpolation): the period becomes ratio times as long, formants and all."""
    x = np.asarray(x, dtype=np.float64)
    return np.interp(np.arange(int(len(x) * ratio)) / ratio, np.arange(len(x)), x)
