"""The YIN rule of include/tacotron2_amd.h (t2_yin; de Cheveigne & Kawahara 2002, steps 2 to 5) and the statistics of
t2_prosody_stats, restated in numpy: float64 (the reference), and float32 in two summation orders - numpy's pairwise sums and a
strictly sequential sum (cumsum) - whose deviations from float64 on a test's own inputs set that test's tolerances (x 8, for a third
order: the kernel's).  Also the signals of the tests.  Nothing here imports the package."""
import numpy as np

DEFAULTS = dict(sr=22050, hop=256, W=1024, tau_min=44, tau_max=367, thr=0.1, vthr=0.3, power_floor=1e-10)


def pick(cm, tau_min, tau_max, thr):
    """The lag of one frame: the smallest c in [tau_min, tau_max) with cm[c] < thr, walked down while c + 1 < tau_max and
    cm[c+1] < cm[c]; without one, the first argmin over [tau_min, tau_max).  Comparisons in cm's own precision."""
    thr = cm.dtype.type(thr)
    below = np.nonzero(cm[tau_min:tau_max] < thr)[0]
    if len(below) == 0:
        return tau_min + int(np.argmin(cm[tau_min:tau_max]))
    c = tau_min + int(below[0])
    while c + 1 < tau_max and cm[c + 1] < cm[c]:
        c += 1
    return c


def _sum_rows(a, mode):
    """Row sums of a 2-D array: 'pairwise' = numpy's sum over the contiguous axis, 'sequential' = left to right."""
    if mode == "sequential":
        return np.cumsum(a, axis=1, dtype=a.dtype)[:, -1]
    return a.sum(axis=1, dtype=a.dtype)


def frame(x, W, tau_min, tau_max, thr, vthr, power_floor, sr, dtype=np.float64, mode="pairwise"):
    """One valid frame: x = the span of W + tau_max samples.  (cm [tau_max + 1], tau, voiced, f0, aper, power), in `dtype`."""
    ft = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype)
    lagged = np.lib.stride_tricks.sliding_window_view(x, W)          # row tau = x[tau : tau + W]
    assert lagged.shape[0] == tau_max + 1
    diff = x[None, :W] - lagged
    d = _sum_rows(np.ascontiguousarray(diff * diff), mode)
    d[0] = 0
    run = np.cumsum(d, dtype=dtype)                                   # (the prefix over tau: sequential in every mode)
    tau = np.arange(tau_max + 1).astype(dtype)
    cm = np.ones(tau_max + 1, dtype=dtype)
    ok = run > 0
    ok[0] = False
    cm[ok] = d[ok] * tau[ok] / run[ok]
    power = _sum_rows(np.ascontiguousarray((x[:W] * x[:W])[None, :]), mode)[0] / ft(W)
    c = pick(cm, tau_min, tau_max, thr)
    aper = cm[c]
    voiced = bool(aper < ft(vthr) and power > ft(power_floor))
    f0 = ft(0)
    if voiced:
        a, e = cm[c - 1], cm[c + 1]
        den = a - ft(2) * aper + e
        off = ft(0.5) * (a - e) / den if den > 0 else ft(0)
        off = min(max(off, ft(-1)), ft(1))
        f0 = ft(sr) / (ft(c) + off)
    return cm, c, voiced, f0, aper, power


def yin(signals, n_max=None, dtype=np.float64, mode="pairwise", sr=22050, hop=256, W=1024, tau_min=44, tau_max=367, thr=0.1,
        vthr=0.3, power_floor=1e-10):
    """The batch: signals = list of 1-D arrays (their lengths are n[b]).  dict of arrays over (B, T), T = 1 + n_max // hop: valid,
    tau (0 where invalid), voiced, f0, aper, power, and cm (B, T, tau_max + 1).  Invalid frames: f0 0, aper 1, power 0, cm 1."""
    n_max = max(len(s) for s in signals) if n_max is None else n_max
    B, T, S = len(signals), 1 + n_max // hop, W + tau_max
    out = dict(valid=np.zeros((B, T), bool), tau=np.zeros((B, T), np.int64), voiced=np.zeros((B, T), bool),
               f0=np.zeros((B, T), dtype), aper=np.ones((B, T), dtype), power=np.zeros((B, T), dtype),
               cm=np.ones((B, T, tau_max + 1), dtype))
    for b, s in enumerate(signals):
        for t in range(T):
            s0 = t * hop - S // 2
            if s0 < 0 or s0 + S > len(s):
                continue
            cm, c, v, f0, ap, pw = frame(s[s0:s0 + S], W, tau_min, tau_max, thr, vthr, power_floor, sr, dtype, mode)
            out["valid"][b, t], out["tau"][b, t], out["voiced"][b, t] = True, c, v
            out["f0"][b, t], out["aper"][b, t], out["power"][b, t], out["cm"][b, t] = f0, ap, pw, cm
    return out


def stable_frames(ref, tau_min=44, tau_max=367, thr=0.1, vthr=0.3, power_floor=1e-10, **_):
    """(B, T) bool: the float64 reference `ref` picks the same lag and the same voiced flag with thr and vthr both scaled by 0.98
    and by 1.02.  Invalid frames count as stable."""
    st = np.ones(ref["valid"].shape, bool)
    for b, t in zip(*np.nonzero(ref["valid"])):
        cm = ref["cm"][b, t]
        for k in (0.98, 1.02):
            c = pick(cm, tau_min, tau_max, thr * k)
            v = bool(cm[c] < vthr * k and ref["power"][b, t] > power_floor)
            if c != ref["tau"][b, t] or v != ref["voiced"][b, t]:
                st[b, t] = False
    return st


def tolerances(signals, factor=8.0, **cfg):
    """(ref float64, tol): tol[q] = factor x the larger deviation of the two float32 restatements from float64 on these signals -
    relative for f0 (voiced in all three) and power, absolute for aper and cm.  Frames whose lag or voiced flag differs between a
    float32 restatement and float64 are left out of f0 and aper (they are the unstable ones)."""
    ref = yin(signals, dtype=np.float64, **cfg)
    tol = dict(f0=0.0, aper=0.0, power=0.0, cm=0.0)
    for mode in ("pairwise", "sequential"):
        r32 = yin(signals, dtype=np.float32, mode=mode, **cfg)
        same = ref["valid"] & (r32["tau"] == ref["tau"]) & (r32["voiced"] == ref["voiced"])
        v = same & ref["voiced"]
        if v.any():
            tol["f0"] = max(tol["f0"], float(np.max(np.abs(r32["f0"][v] - ref["f0"][v]) / ref["f0"][v])))
        if same.any():
            tol["aper"] = max(tol["aper"], float(np.max(np.abs(r32["aper"][same] - ref["aper"][same]))))
        pw = ref["valid"] & (ref["power"] > 0)
        if pw.any():
            tol["power"] = max(tol["power"], float(np.max(np.abs(r32["power"][pw] - ref["power"][pw]) / ref["power"][pw])))
        tol["cm"] = max(tol["cm"], float(np.max(np.abs(r32["cm"] - ref["cm"]))))
    return ref, {k: factor * v for k, v in tol.items()}


def stats(f0, aper, power, valid):
    """The row of t2_prosody_stats for one utterance, float64: [valid, voiced, mean ln f0, p5, p95, mean 10 log10 power, mean aper,
    0]; the percentiles are elements of f0 (nearest rank); NaN without a voiced frame."""
    f0, aper, power = (np.asarray(a, dtype=np.float64) for a in (f0, aper, power))
    vo = np.asarray(valid, bool) & (f0 > 0)
    nv = int(vo.sum())
    row = [float(np.sum(valid)), float(nv)] + [float("nan")] * 5 + [0.0]
    if nv:
        v = np.sort(f0[vo])
        row[2] = float(np.mean(np.log(f0[vo])))
        row[3] = float(v[(5 * (nv - 1) + 50) // 100])
        row[4] = float(v[(95 * (nv - 1) + 50) // 100])
        row[5] = float(np.mean(10.0 * np.log10(power[vo])))
        row[6] = float(np.mean(aper[vo]))
    return row


def tone(f, n, sr=22050, harmonics=4, amp=0.3, phase=0.0):
    """A steady tone of `harmonics` partials with amplitudes 1/k, scaled to `amp`."""
    t = np.arange(n) / sr
    x = sum(np.sin(2 * np.pi * f * k * t + phase * k) / k for k in range(1, harmonics + 1))
    return (amp * x / sum(1.0 / k for k in range(1, harmonics + 1))).astype(np.float32)


GLIDE_LENGTHS = (9000, 12001, 7000, 1300, 16000)


def glides(seed=0, sr=22050, lengths=GLIDE_LENGTHS):
    """The test signals: each a glide between a random start in 80-160 Hz and a random end in 160-320 Hz with five harmonics (1/k)
    and a rising amplitude (0.1 -> 0.4), plus noise at 0.003; the stretch [n/3, n/3 + n/6) is replaced by noise at 0.05 (unvoiced)
    and [n/3 + n/6, n/3 + n/4) by exact zeros (digital silence).  float32."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        f_a, f_b = rng.uniform(80, 160), rng.uniform(160, 320)
        f = np.linspace(f_a, f_b, n)
        ph = 2 * np.pi * np.cumsum(f) / sr
        x = sum(np.sin(k * ph) / k for k in range(1, 6)) / sum(1.0 / k for k in range(1, 6))
        x = x * np.linspace(0.1, 0.4, n) + 0.003 * rng.normal(size=n)
        a, b, c = n // 3, n // 3 + n // 6, n // 3 + n // 4
        x[a:b] = 0.05 * rng.normal(size=b - a)
        x[b:c] = 0.0
        out.append(x.astype(np.float32))
    return out
