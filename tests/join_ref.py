"""t2_join restated in numpy (include/tacotron2_amd.h): spans and sums in float64 by direct summation, the plan in
float64, the output in float32 by the kernel's two multiplications.  No torch, no GPU."""
import numpy as np


def fade_table(fade):
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(fade, dtype=np.float64) + 0.5) / max(fade, 1))).astype(np.float32)


def span_ref(x, top_db=60.0, F=2048, H=512, keep=0, trim=True):
    """(s0, s1, margin) of one signal x (its n samples): margin is the smallest relative distance of a frame energy to the threshold,
    inf where no threshold is applied (no trim, n < F) or it is 0 (an all-zero signal)."""
    n = len(x)
    if not trim or n < F:
        return 0, n, np.inf
    sq = np.square(x.astype(np.float64))
    e = np.empty(n // H + 1)
    for f in range(len(e)):
        lo, hi = max(f * H - F // 2, 0), min(f * H + F // 2, n)
        e[f] = sq[lo:hi].sum() if hi > lo else 0.0
    thr = e.max() * 10.0 ** (-top_db / 10.0)
    act = np.nonzero(e > thr)[0]
    margin = np.inf if thr == 0 else float(np.abs(e - thr).min() / thr)
    if e.max() == 0 or len(act) == 0:
        return 0, 0, margin
    return max(0, int(act[0]) * H - keep), min(n, (int(act[-1]) + 1) * H + keep), margin


def envelope(length, fade, w):
    """e[i] of one piece: the table sampled at (2 i + 1) fade / (2 fl) inside the first and last fl = min(fade, length // 2)."""
    e = np.ones(length, np.float32)
    fl = min(fade, length // 2)
    if fl > 0:
        idx = ((2 * np.arange(fl, dtype=np.int64) + 1) * fade) // (2 * fl)
        e[:fl] = w[idx]
        e[length - fl:] = w[idx][::-1]
    return e


def write_ref(x, s0, length, off, gain, pause, total, fade):
    """y (total,) float32 from a plan: x[b, s0 + i] * (gain_b * e), two float32 multiplications; the pauses are zeros.  Samples
    that no piece covers stay NaN, so a hole in the plan shows."""
    w = fade_table(fade)
    y = np.full(total, np.nan, np.float32)
    for b in range(len(length)):
        L = int(length[b])
        ge = np.float32(gain[b]) * envelope(L, fade, w)
        y[off[b]:off[b] + L] = x[b, s0[b]:s0[b] + L].astype(np.float32) * ge
        y[off[b] + L:off[b] + L + int(pause[b])] = 0.0
    return y


def join_ref(x, n, pause, trim=True, top_db=60.0, F=2048, H=512, keep=0, fade=0, level=False, max_gain=2.0, ceiling=0.0):
    """x (B, ld) float32, n and pause B integers.  A dict: s0, len (int32), off (int64), total, gain (float32) and gain64, y
    (total,) float32, margin (B,), sumsq and peak (float64)."""
    B = len(n)
    s0, s1, margin = (np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B))
    for b in range(B):
        s0[b], s1[b], margin[b] = span_ref(x[b, :n[b]], top_db, F, H, keep, trim)
    length = s1 - s0
    sumsq = np.array([np.square(x[b, s0[b]:s1[b]].astype(np.float64)).sum() for b in range(B)])
    peak = np.array([np.abs(x[b, s0[b]:s1[b]]).astype(np.float64).max() if length[b] else 0.0 for b in range(B)])
    gain = np.ones(B)
    if level and length.sum() > 0:
        rms_doc = np.sqrt(sumsq.sum() / length.sum())
        for b in range(B):
            rms = np.sqrt(sumsq[b] / length[b]) if length[b] else 0.0
            if rms > 0:
                gain[b] = min(max(rms_doc / rms, 1.0 / max_gain), max_gain)
    pk = float((gain * peak).max())
    if ceiling > 0 and pk > ceiling:
        gain = gain * (ceiling / pk)
    seg = length + np.asarray(pause, np.int64)
    off = np.concatenate([[0], np.cumsum(seg)[:-1]]).astype(np.int64)
    total = int(seg.sum())
    g32 = gain.astype(np.float32)
    return dict(s0=s0.astype(np.int32), len=length.astype(np.int32), off=off, total=total, gain=g32, gain64=gain,
                y=write_ref(x, s0, length, off, g32, pause, total, fade), margin=margin, sumsq=sumsq, peak=peak)
