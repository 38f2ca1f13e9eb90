"""t2_loudness restated in float64 (include/tacotron2_amd.h): ITU-R BS.1770-4 for one channel - the K-weighting as
libebur128 re-derives it for any rate, run SEQUENTIALLY by scipy.signal.lfilter, hop energies, 400 ms blocks, both gates decided in
the linear domain, and the true peak from the 4x polyphase table of datasets/resample.plan.  Nothing here is shared with
tacotron2_amd/loudness.py but that table, which tests/resample_ref.py restates on its own."""
import math

import numpy as np
from scipy.signal import lfilter

ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
SHORT, UNDEFINED, LIMITED, CAPPED = 1, 2, 4, 8


def k_weighting(sr):
    def stage(f0, Q):
        K = math.tan(math.pi * f0 / sr)
        return K, 1.0 + K / Q + K * K
    Q = 0.7071752369554196
    K, a0 = stage(1681.974450955533, Q)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    Q = 0.5003270373238773
    K, a0 = stage(38.13547087602444, Q)
    return b1, a1, np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def weighted(x, sr):
    """The K-weighted signal in float64, from a zero state."""
    b1, a1, b2, a2 = k_weighting(sr)
    return lfilter(b2, a2, lfilter(b1, a1, np.asarray(x, np.float64)))


def lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def blocks(x, sr):
    """(E the whole-hop energies, z the block mean squares, short) of one row."""
    n, H = len(x), int(round(sr / 10))
    N = 4 * H
    y2 = weighted(x, sr) ** 2 if n else np.zeros(0)
    E = np.array([y2[h * H:(h + 1) * H].sum() for h in range(n // H)], np.float64)
    if n >= N:
        z = np.array([(((E[j] + E[j + 1]) + E[j + 2]) + E[j + 3]) / N for j in range(n // H - 3)])
        return E, z, False
    if n > 0:
        return E, np.array([y2.sum() / n]), True
    return E, np.zeros(0), False


def true_peak(x, sr):
    """The largest magnitude of the 4 n values of the 4x polyphase interpolation, float64 sums of the float32 table."""
    from tacotron2_amd.datasets.resample import plan
    U, D, K, table = plan(sr, 4 * sr)
    assert (U, D) == (4, 1)
    n = len(x)
    if n == 0:
        return 0.0
    xp = np.concatenate([np.zeros(K - 1), np.asarray(x, np.float64), np.zeros(K)])
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * K)          # win[i] = x[i - K + 1 .. i + K]
    return float(np.abs(win @ table.astype(np.float64).T).max())


def measure(x, sr, target=None, ceiling=-1.0, max_gain_db=30.0, dtype=np.float32, peak=None):
    """One row's stat as a dict, plus margin_lu: the smallest distance in LU of a block from a gate it is compared with (inf without
    one).  target None: measuring only, gain 1.  The kernel's input is float32; dtype=np.float64 measures an unrounded signal.
    peak: the true peak the gain is bounded with, where the caller holds the RULE's value - float32 fmaf sums, which this module's
    float64 sums meet to 1e-5 only, while a limited gain is ceiling / true_peak to one float32 ulp; None: true_peak(x, sr)."""
    x = np.asarray(x, dtype)
    E, z, short = blocks(x, sr)
    flags = SHORT if short else 0
    past_abs = z > ABS_GATE
    margin = np.abs(lufs(z[z > 0]) + 70.0).min() if (z > 0).any() else np.inf
    out = dict(E=E, z=z, n_blocks=len(z), n_below_abs=int((~past_abs).sum()), n_below_rel=0, lufs=np.nan, rel_gate_lufs=np.nan,
               momentary_max_lufs=float(lufs(z.max())) if len(z) else np.nan, gain=1.0, ungated_lufs=np.nan,
               sample_peak=float(np.abs(x).max()) if len(x) else 0.0, true_peak=true_peak(x, sr) if peak is None else float(peak))
    if not past_abs.any():
        flags |= UNDEFINED
    else:
        thr = 0.1 * z[past_abs].mean()
        keep = past_abs & (z > thr)
        margin = min(margin, np.abs(lufs(z[past_abs]) - lufs(thr)).min())
        out.update(n_below_rel=int(past_abs.sum() - keep.sum()), lufs=float(lufs(z[keep].mean())), rel_gate_lufs=float(lufs(thr)),
                   ungated_lufs=float(lufs(z.mean())))
        if target is not None:
            out["gain"], more = gain(out["lufs"], out["true_peak"], target, ceiling, max_gain_db)
            flags |= more
    out.update(flags=flags, margin_lu=float(margin))
    return out


def gain(loudness, peak, target, ceiling=-1.0, max_gain_db=30.0):
    """(the gain in float64, its flags) that brings `loudness` LUFS to `target` under the two bounds."""
    g, flags = 10.0 ** ((target - loudness) / 20.0), 0
    if g > 10.0 ** (max_gain_db / 20.0):
        g, flags = 10.0 ** (max_gain_db / 20.0), flags | CAPPED
    c = 10.0 ** (ceiling / 20.0)
    if g * peak > c:
        g, flags = c / peak, flags | LIMITED
    return g, flags


def sine(sr, f, seconds, amp=1.0, phase=0.0, dtype=np.float32):
    t = np.arange(int(round(seconds * sr)), dtype=np.float64) / sr
    return (amp * np.sin(2.0 * np.pi * f * t + phase)).astype(dtype)


def gate_signal(sr):
    """Four seconds of a 440 Hz sine: one each at -20, -45 and -80 dBFS and at half of -20 dBFS."""
    a = 10.0 ** (-20.0 / 20.0)
    return np.concatenate([sine(sr, 440.0, 1.0, amp) for amp in (a, 10.0 ** (-45.0 / 20.0), 10.0 ** (-80.0 / 20.0), 0.5 * a)])
