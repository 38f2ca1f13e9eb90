"""t2_limit restated in float64 (include/tacotron2_amd.h): the look-ahead true-peak limiter, every step SEQUENTIAL and as
the rule states it - the envelope from the 4x polyphase table of datasets/resample.plan, the required gain, the sliding minimum, the
release recurrence one sample after the other, the box sum, the product and the trim.  The float32 true-peak bits (env, peak_after)
are the device's where a caller holds them, as loudness_ref.measure(peak=) takes them: float64 sums of the float32 table meet the
kernel's fmaf sums to 1e-5 only, and everything behind env is decided by env's bits.  release_chunked restates the kernel's chunked
scan in numpy, for tests/test_limiter_ref_host.py.  Nothing here is shared with tacotron2_amd/limiter.py but that table."""
import math

import numpy as np

ACTIVE, TRIMMED = 1, 2


def coefficient(release_ms, sr):
    return math.exp(-1.0 / (release_ms / 1000.0 * sr))


def lookahead_samples(lookahead_ms, sr):
    return min(max(int(round(lookahead_ms * sr / 1000.0)), 1), 2048)


def peaks(x, sr):
    """P[i] = max(|x[i]|, |u[4i]|, .., |u[4i+3]|) in float64."""
    from tacotron2_amd.datasets.resample import plan
    U, D, K, table = plan(sr, 4 * sr)
    assert (U, D) == (4, 1)
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.zeros(0)
    xp = np.concatenate([np.zeros(K - 1), x, np.zeros(K)])
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * K)           # win[i] = x[i - K + 1 .. i + K]
    return np.maximum(np.abs(win @ table.astype(np.float64).T).max(axis=1), np.abs(x))


def envelope(P):
    """env[i] = max(P[i-1], P[i]), P[-1] = 0."""
    P = np.asarray(P)
    return np.maximum(P, np.concatenate([np.zeros(1, P.dtype), P[:-1]])) if len(P) else P


def required(env, c):
    """r, float32: one fp64 division, rounded once."""
    env = np.asarray(env, np.float32).astype(np.float64)
    r = np.ones(len(env), np.float32)
    over = env > c
    r[over] = (c / env[over]).astype(np.float32)
    return r, over


def lookahead(r, L):
    """h[i] = min r[i .. min(i + L, n - 1)]."""
    if len(r) == 0:
        return r
    return np.lib.stride_tricks.sliding_window_view(np.concatenate([r, np.ones(L, r.dtype)]), L + 1).min(axis=1)


def release(h, a, start=None):
    """e[i] = min(h[i], a e[i-1] + (1 - a)) in float64, one sample after the other, from e[-1] = start (None: h[0])."""
    e = np.empty(len(h), np.float64)
    prev, oma = float(h[0]) if start is None and len(h) else start, 1.0 - a
    for i, hi in enumerate(np.asarray(h, np.float64).tolist()):
        prev = min(hi, a * prev + oma)
        e[i] = prev
    return e


def stall(a):
    """Where the fp64 recurrence e' = a e + (1 - a) stops short of 1, as d = 1 - e: with e = 1 - k 2^-53 a step is k' = round(a k)
    (1 - a is exact for a >= 0.5), which no longer moves once (1 - a) k < 1/2 - the largest such k, found with the recurrence's own
    arithmetic.  Every release from below ends exactly there, about tau / 2 ulps under 1."""
    u, oma = 2.0 ** -53, 1.0 - a
    for k in range(int(0.5 / oma) + 2, 0, -1):
        e = 1.0 - k * u
        if a * e + oma == e:
            return k * u
    return 0.0


def release_chunked(h, a, chunk=16, threads=256):
    """The kernel's way (csrc/t2_limit.hip): passes of chunk * threads samples; every chunk is run from e = 1 (the first from the
    carried state), the ends d = 1 - e meet in an inclusive Hillis-Steele scan d[t] = max(d[t], a^(chunk 2^k) d[t - 2^k]), the powers
    by squaring and a product that is not zero held at stall(a), and every chunk is run again from 1 - d[t-1]."""
    floor = stall(a)
    n, P, oma = len(h), chunk * threads, 1.0 - a
    steps = int(round(math.log2(threads)))
    m = a
    for _ in range(int(round(math.log2(chunk)))):
        m *= m
    pw = []
    for _ in range(steps):
        pw.append(m)
        m *= m
    e = np.empty(-(-n // P) * P, np.float64)
    carry = float(h[0])
    for p0 in range(0, n, P):
        hp = np.ones((threads, chunk), np.float64)
        hp.reshape(-1)[:min(P, n - p0)] = h[p0:p0 + P]

        def run(state):
            out = np.empty_like(hp)
            for i in range(chunk):
                state = np.minimum(hp[:, i], a * state + oma)
                out[:, i] = state
            return out
        first = np.ones(threads)
        first[0] = carry
        d = 1.0 - run(first)[:, -1]
        for k in range(steps):
            s = 1 << k
            back = pw[k] * d[:-s]
            d = np.concatenate([d[:s], np.maximum(d[s:], np.where(back > 0, np.maximum(back, floor), 0.0))])
        first[1:] = 1.0 - d[:-1]
        out = run(first)
        e[p0:p0 + P] = out.reshape(-1)
        carry = out[-1, -1]
    return e[:n]


def attack(e, L):
    """s[i] = (e[i-L] + .. + e[i]) / (L + 1), e[m] = e-start = h[0] for m < 0; the caller passes e with that front: L + n values."""
    return np.lib.stride_tricks.sliding_window_view(e, L + 1).sum(axis=1) / (L + 1)


def gain_curve(env, c, L, a):
    """Steps 2 - 5 on an envelope: dict(r, h, e, s, curve (float32), n_over, min_gain)."""
    r, over = required(env, c)
    if len(r) == 0:
        z = np.zeros(0)
        return dict(r=r, h=r, e=z, s=z, curve=r, n_over=0, min_gain=1.0)
    h = lookahead(r, L)
    e = release(h, a)
    s = attack(np.concatenate([np.full(L, float(h[0])), e]), L)
    return dict(r=r, h=h, e=e, s=s, curve=s.astype(np.float32), n_over=int(over.sum()), min_gain=float(s.min()))


def trim(peak_after, c):
    """The largest float32 t with (double)t * peak_after <= c; 1 where the peak is under the ceiling."""
    if not peak_after > c:
        return np.float32(1.0)
    t = np.float32(c / peak_after)
    while float(t) * peak_after > c:
        t = np.nextafter(t, np.float32(0.0))
    while float(np.nextafter(t, np.float32(2.0))) * peak_after <= c:
        t = np.nextafter(t, np.float32(2.0))
    return t


def limit(x, sr, c, L, a, env=None, peak_after=None):
    """One row through the rule.  env, peak_after: the device's float32 values where the caller holds them; None: this module's
    float64 sums, rounded to float32.  Returns gain_curve's dict plus env, in_peak, w, peak_after, trim, y, flags."""
    x = np.asarray(x, np.float32)
    env = envelope(peaks(x, sr)).astype(np.float32) if env is None else np.asarray(env, np.float32)
    out = gain_curve(env, c, L, a)
    w = x * out["curve"]
    if peak_after is None:
        peak_after = float(np.float32(peaks(w, sr).max())) if len(x) else 0.0
    t = trim(float(peak_after), c)
    flags = (ACTIVE if out["n_over"] else 0) | (TRIMMED if peak_after > c else 0)
    out.update(env=env, in_peak=float(env.max()) if len(env) else 0.0, w=w, peak_after=float(peak_after), trim=t,
               y=(w * t).astype(np.float32) if peak_after > c else w, flags=flags)
    return out


def voice(seed, n, amp, sr):
    """tests/test_gpu_loudness.py's voice: a 180 Hz tone with four harmonics under a slow swell, plus a little noise; RMS about amp."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = sum(np.sin(2 * np.pi * 180.0 * k * t + k) / k for k in range(1, 5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.9 * t + 1.0))
    return (amp * (x / 0.8 + 0.05 * rng.standard_normal(n))).astype(np.float32)


def pulses(seed, n, at, sr, amp=0.2, tall=1.6):
    """A quiet voice, under any ceiling the tests use, with short tall pulses (three samples, alternating sign) at the indices `at`."""
    x = voice(seed, n, amp * 0.25, sr)
    rng = np.random.default_rng(seed + 1000)
    for i in at:
        for k, sgn in ((0, 1.0), (1, -0.7), (2, 0.4)):
            if 0 <= i + k < n:
                x[i + k] = np.float32(sgn * tall * (0.8 + 0.2 * rng.random()))
    return x


def rows(P, L, sr):
    """The rows of tests/test_gpu_limiter.py's batch, (name, samples): every length at which the kernel takes another path - P its
    pass length -, pulses above any ceiling the tests use within L on either side of every pass boundary, at the sample 0 and at
    n - 1, two of them closer than L, a row above the ceiling throughout and one below it."""
    long = 2 * P + 77
    near = lambda edge: [edge - L + 3, edge - 2, edge + 1, edge + L - 5]
    t = np.arange(3000, dtype=np.float64)
    return [("empty", np.zeros(0, np.float32)),
            ("one", np.array([1.5], np.float32)),
            ("L", pulses(1, L, [L // 2], sr)),
            ("L+1", pulses(2, L + 1, [0], sr)),
            ("P-1", pulses(3, P - 1, [0, 700, P - 2], sr)),
            ("P", pulses(4, P, [P - L - 1, P - 1], sr)),
            ("P+L+1", pulses(5, P + L + 1, near(P) + [P + L], sr)),
            ("2P+77", pulses(6, long, [0, 1500, 1500 + L // 2] + near(P) + near(2 * P) + [long - 1], sr)),
            ("above", (1.3 + 0.1 * np.sin(2 * np.pi * t / 57.0)).astype(np.float32)),
            ("below", voice(7, 5000, 0.05, sr))]
