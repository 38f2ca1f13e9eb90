"""The cycle-matching rule of include/tacotron2_amd.h (t2_voice_quality) and the reduction of t2_corpus_stats, restated in
numpy: float64 (the reference), and float32 in two summation orders - numpy's pairwise sums and a strictly sequential sum (cumsum) -
whose deviations from float64 on a test's own inputs set that test's tolerances (x 8, for a third order: the kernel's), as
tests/prosody_ref.py does for YIN.  Also a synthetic voice with known jitter, shimmer and noise, and the normalisation of
`main.py prosody-export` as one formula.  Nothing here imports the package."""
import numpy as np

MAX_CYCLES = 32
DEFAULTS = dict(sr=22050, hop=256, W=1024, tau_min=44, tau_max=367)


def _sum_rows(a, mode):
    """Row sums of a 2-D array: 'pairwise' = numpy's sum over the contiguous axis, 'sequential' = left to right."""
    a = np.ascontiguousarray(a)
    if mode == "sequential":
        return np.cumsum(a, axis=1, dtype=a.dtype)[:, -1]
    return a.sum(axis=1, dtype=a.dtype)


def _sum(v, mode):
    return _sum_rows(np.asarray(v)[None, :], mode)[0]


def setup(f0, S, sr, tau_min, tau_max):
    """(L, d, K) of a valid frame with the float32 pitch f0 > 0: the quotient sr / f0 is float32 in every precision (it is an input
    of the rule, not a result), rounded half to even."""
    q = np.float32(sr) / np.float32(f0)
    q = min(max(q, np.float32(tau_min)), np.float32(tau_max - 1))
    L = int(np.rint(q))
    d = max(2, (L + 7) // 8)
    room = S - 2 * L - d
    K = 0 if room < 0 else min(room // L + 1, MAX_CYCLES)
    return L, d, K


def cycle(x, c, L, d, dtype=np.float64, mode="pairwise"):
    """One cycle at anchor c of the span x: (ncc [2 d + 1] over tau = L-d .. L+d, index of tau*, T_i, r_i, A_i) in `dtype`."""
    ft = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype)
    a = x[c:c + L]
    bs = np.lib.stride_tricks.sliding_window_view(x[c + L - d:c + 2 * L + d], L)          # row k = b of tau = L - d + k
    assert bs.shape[0] == 2 * d + 1
    ab = _sum_rows(a[None, :] * bs, mode)
    ea = _sum(a * a, mode)
    eb = _sum_rows(bs * bs, mode)
    den = ea * eb
    ncc = np.zeros(2 * d + 1, dtype=dtype)
    ok = den > 0
    ncc[ok] = ab[ok] / np.sqrt(den[ok])
    k = int(np.argmax(ncc))                                                               # the first maximum
    off = ft(0)
    if 0 < k < 2 * d:
        lo, m, hi = ncc[k - 1], ncc[k], ncc[k + 1]
        cur = lo - ft(2) * m + hi
        if cur < 0:
            off = min(max(ft(0.5) * (lo - hi) / cur, ft(-1)), ft(1))
    return ncc, k, ft(L - d + k) + off, ncc[k], np.sqrt(ea / ft(L))


def frame(x, f0, sr, tau_min, tau_max, dtype=np.float64, mode="pairwise"):
    """One valid frame: x = its span of S samples, f0 its float32 pitch.  None when the frame is not measured (f0 not > 0, K < 3),
    else a dict: K, L, d, per cycle T, r, A, k (index of tau*) and ncc (K, 2 d + 1), and jitter, shimmer, nhr, hnr_db."""
    ft = np.dtype(dtype).type
    if not f0 > 0:
        return None
    L, d, K = setup(f0, len(x), sr, tau_min, tau_max)
    if K < 3:
        return None
    cyc = [cycle(x, i * L, L, d, dtype, mode) for i in range(K)]
    T, r, A = (np.array([c[q] for c in cyc], dtype=dtype) for q in (2, 3, 4))
    mean = lambda v: _sum(v, "sequential") / ft(len(v))
    mT, mA = mean(T), mean(A)
    rr = min(max(mean(r), ft(1e-3)), ft(1) - ft(1e-6))
    return dict(K=K, L=L, d=d, T=T, r=r, A=A, k=np.array([c[1] for c in cyc]), ncc=np.stack([c[0] for c in cyc]),
                jitter=mean(np.abs(np.diff(T))) / mT, shimmer=(mean(np.abs(np.diff(A))) / mA) if mA > 0 else ft(0),
                nhr=(ft(1) - rr) / rr, hnr_db=ft(10) * np.log10(rr / (ft(1) - rr)))


def voice_quality(signals, f0, n_max=None, dtype=np.float64, mode="pairwise", sr=22050, hop=256, W=1024, tau_min=44, tau_max=367):
    """The batch: signals = list of 1-D arrays (their lengths are n[b]), f0 (B, T) float32 with T = 1 + n_max // hop.  dict of arrays
    over (B, T): valid, cycles, jitter, shimmer, nhr, hnr_db (0 where not measured), cyc (B, T, 32, 3) = T_i, r_i, A_i with zeros
    behind K, and `frames` {(b, t): frame dict} of the measured frames."""
    n_max = max(len(s) for s in signals) if n_max is None else n_max
    B, T, S = len(signals), 1 + n_max // hop, W + tau_max
    assert f0.shape == (B, T) and f0.dtype == np.float32
    out = dict(valid=np.zeros((B, T), bool), cycles=np.zeros((B, T), np.int32), cyc=np.zeros((B, T, MAX_CYCLES, 3), dtype), frames={})
    for q in ("jitter", "shimmer", "nhr", "hnr_db"):
        out[q] = np.zeros((B, T), dtype)
    for b, s in enumerate(signals):
        for t in range(T):
            s0 = t * hop - S // 2
            if s0 < 0 or s0 + S > len(s):
                continue
            out["valid"][b, t] = True
            fr = frame(s[s0:s0 + S], f0[b, t], sr, tau_min, tau_max, dtype, mode)
            if fr is None:
                continue
            out["frames"][(b, t)] = fr
            out["cycles"][b, t] = fr["K"]
            for q in ("jitter", "shimmer", "nhr", "hnr_db"):
                out[q][b, t] = fr[q]
            out["cyc"][b, t, :fr["K"]] = np.stack([fr["T"], fr["r"], fr["A"]], axis=1)
    return out


def tolerances(signals, f0, factor=8.0, **cfg):
    """(ref float64, tol, stable, dev_ncc): tol[q] = factor x the larger deviation of the two float32 restatements from float64 on
    these inputs - absolute for T, r, jitter, shimmer, hnr_db, relative for A and nhr - over the cycles (frames) whose tau* is the
    float64 one in both restatements.  stable[(b, t)] = bool per cycle: the float64 margin between the best and the second-best ncc
    exceeds 16 x dev_ncc, the largest ncc deviation of the two restatements from float64.  Also returned: how many cycles a
    restatement picks differently (`tol["n_differing_picks"]`)."""
    ref = voice_quality(signals, f0, dtype=np.float64, **cfg)
    tol = dict(T=0.0, r=0.0, A=0.0, jitter=0.0, shimmer=0.0, nhr=0.0, hnr_db=0.0)
    dev_ncc, differing = 0.0, 0
    for mode in ("pairwise", "sequential"):
        r32 = voice_quality(signals, f0, dtype=np.float32, mode=mode, **cfg)
        assert (r32["cycles"] == ref["cycles"]).all()
        for key, fr in ref["frames"].items():
            g = r32["frames"][key]
            dev_ncc = max(dev_ncc, float(np.max(np.abs(g["ncc"] - fr["ncc"]))))
            same = g["k"] == fr["k"]
            differing += int((~same).sum())
            if same.any():
                tol["T"] = max(tol["T"], float(np.max(np.abs(g["T"] - fr["T"])[same])))
                tol["r"] = max(tol["r"], float(np.max(np.abs(g["r"] - fr["r"])[same])))
                nz = same & (fr["A"] > 0)
                if nz.any():
                    tol["A"] = max(tol["A"], float(np.max((np.abs(g["A"] - fr["A"]) / np.where(fr["A"] > 0, fr["A"], 1))[nz])))
            if same.all():
                for q in ("jitter", "shimmer", "hnr_db"):
                    tol[q] = max(tol[q], float(abs(g[q] - fr[q])))
                tol["nhr"] = max(tol["nhr"], float(abs(g["nhr"] - fr["nhr"]) / fr["nhr"]))
    tol = {k: factor * v for k, v in tol.items()}
    tol["n_differing_picks"] = differing
    stable = {}
    for key, fr in ref["frames"].items():
        srt = np.sort(fr["ncc"], axis=1)
        stable[key] = (srt[:, -1] - srt[:, -2]) > 16.0 * dev_ncc
    return ref, tol, stable, dev_ncc


def corpus_stats(f0, power, vq, valid, power_floor=1e-10):
    """The row of t2_corpus_stats for one utterance, float64, from (T,) arrays: [valid, voiced, measured, loud, mean f0, mean jitter,
    shimmer, nhr, hnr_db over the measured frames, mean 10 log10 power over the loud frames, 0, 0]; 0 for a mean over nothing."""
    valid = np.asarray(valid, bool)
    f0, power = np.asarray(f0, np.float64), np.asarray(power, np.float64)
    with np.errstate(invalid="ignore"):
        vo, me, lo = valid & (f0 > 0), valid & (np.asarray(vq["cycles"]) > 0), valid & (power > np.float32(power_floor))
    mean = lambda v, m: float(np.mean(np.asarray(v, np.float64)[m])) if m.any() else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(np.where(lo, power, 1.0))
    return [float(valid.sum()), float(vo.sum()), float(me.sum()), float(lo.sum()), mean(f0, vo)] + \
        [mean(vq[q], me) for q in ("jitter", "shimmer", "nhr", "hnr_db")] + [mean(db, lo), 0.0, 0.0]


# ----------------------------------------------------------------------------------------------------------------------------------
# a synthetic voice
# ----------------------------------------------------------------------------------------------------------------------------------
def voice(f0, n, sr=22050, jitter=0.0, shimmer=0.0, noise=0.0, amp=0.3, seed=0, tremor=(6.0, 0.0),
          formants=((700.0, 110.0), (1200.0, 140.0))):
    """A pulse train at f0 Hz through two damped resonances (centre, bandwidth in Hz).  Period k is T0 (1 + jitter g_k) and pulse k
    has the amplitude 1 + shimmer h_k with g, h standard normal; pulses sit at fractional positions (linear interpolation between the
    two neighbouring samples); tremor = (rate in Hz, depth) multiplies the pulse at time t by 1 + depth sin(2 pi rate t), a slow swell
    as natural voices have it (cycles two periods apart then differ more than neighbours do).  White noise is added at the power ratio `noise` (noise power / voice power), and the whole is scaled
    so that the voice part has the RMS `amp`.  (float32 signal, dict: the true relative mean absolute successive differences of the
    periods and of the pulse amplitudes - what jitter and shimmer estimate -, and the noise ratio)."""
    rng = np.random.default_rng(seed)
    T0 = sr / f0
    pos, periods, amps = 0.5 * T0, [], []
    e = np.zeros(n + 2)
    while pos < n:
        a = max(0.05, 1.0 + shimmer * rng.normal())
        amps.append(a)
        a *= 1.0 + tremor[1] * np.sin(2 * np.pi * tremor[0] * pos / sr)
        i = int(np.floor(pos))
        fr = pos - i
        e[i] += a * (1.0 - fr)
        e[i + 1] += a * fr
        per = T0 * max(0.5, 1.0 + jitter * rng.normal())
        periods.append(per)
        pos += per
    y = e[:n]
    for fc, bw in formants:                                   # y[m] = x[m] + 2 r cos(w) y[m-1] - r^2 y[m-2]
        r, w = np.exp(-np.pi * bw / sr), 2 * np.pi * fc / sr
        a1, a2 = 2 * r * np.cos(w), -r * r
        out = np.zeros(n)
        y1 = y2 = 0.0
        for m in range(n):
            v = y[m] + a1 * y1 + a2 * y2
            out[m] = v
            y2, y1 = y1, v
        y = out
    y = y * (amp / np.sqrt(np.mean(y * y)))
    y = y + np.sqrt(noise) * amp * rng.normal(size=n)
    periods, amps = np.array(periods), np.array(amps)
    true = dict(jitter=float(np.mean(np.abs(np.diff(periods))) / np.mean(periods)) if len(periods) > 1 else 0.0,
                shimmer=float(np.mean(np.abs(np.diff(amps))) / np.mean(amps)) if len(amps) > 1 else 0.0, noise=float(noise))
    return y.astype(np.float32), true


def measure_voice(x, f0, **cfg):
    """Means of the float64 rule over the measured frames of one signal, with the constant track f0: dict jitter, shimmer, nhr,
    hnr_db, n (measured frames)."""
    cfg = dict(DEFAULTS, **cfg)
    T = 1 + len(x) // cfg["hop"]
    ref = voice_quality([x], np.full((1, T), f0, np.float32), **cfg)
    m = ref["cycles"][0] > 0
    return dict(n=int(m.sum()), **{q: float(ref[q][0][m].mean()) for q in ("jitter", "shimmer", "nhr", "hnr_db")})


# ----------------------------------------------------------------------------------------------------------------------------------
# the normalisation of prosody-export, as one formula
# ----------------------------------------------------------------------------------------------------------------------------------
def normalise(x, x_train):
    """(norm, clipped) of the values x with the median and the sample standard deviation (ddof 1) of x_train."""
    x, x_train = np.asarray(x, np.float64), np.asarray(x_train, np.float64)
    z = (x - np.median(x_train)) / (3.0 * np.std(x_train, ddof=1))
    return z, np.clip(z, -1.0, 1.0)
