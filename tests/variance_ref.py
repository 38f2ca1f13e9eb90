"""float64 numpy restatement of t2_char_variance (include/tacotron2_amd.h): per-character pitch and energy from a pitch
track, a log-mel and per-character durations, with the per-utterance sums.  Every sum is math.fsum (exactly rounded), so the
reference carries no summation error of its own.  Inputs are taken at float32 precision where the kernel reads float32."""
import math

import numpy as np

NSTAT = 10


def frame_pitch(f0, F, log_pitch=True, interpolate=False):
    """(q (F,) float64, voiced (F,) bool) of the first F frames of a track in Hz."""
    f = np.asarray(f0, dtype=np.float32)[:F]
    voiced = np.array([bool(x > 0) for x in f], dtype=bool)          # (NaN > 0 is False)
    p = np.zeros(F, dtype=np.float64)
    for t in np.nonzero(voiced)[0]:
        p[t] = math.log(float(f[t])) if log_pitch else float(f[t])
    q = p.copy()
    idx = np.nonzero(voiced)[0]
    if interpolate and len(idx):
        for t in range(F):
            if voiced[t]:
                continue
            if t < idx[0]:
                q[t] = p[idx[0]]
            elif t > idx[-1]:
                q[t] = p[idx[-1]]
            else:
                k = int(np.searchsorted(idx, t))
                a, c = int(idx[k - 1]), int(idx[k])
                q[t] = p[a] + (p[c] - p[a]) * (float(t - a) / float(c - a))
    return q, voiced


def frame_energy(mel, F):
    """e (F,) float64 of the first F rows of a log-mel (T, M): sqrt(sum_m exp(2 mel))."""
    m = np.asarray(mel, dtype=np.float32)[:F].astype(np.float64)
    return np.array([math.sqrt(math.fsum(math.exp(2.0 * float(x)) for x in row)) for row in m], dtype=np.float64).reshape(F)


def char_variance(dur, n_chars, n_frames, f0, mel, L=None, log_pitch=True, interpolate=False):
    """One utterance.  dur: integers (>= n_chars of them are read), f0 (T,), mel (T, M).  Returns a dict: pitch, energy float64 (L,),
    voiced int64 (L,), q, e float64 (F,), stats float64 (10,)."""
    T = len(f0)
    L = len(dur) if L is None else L
    N = min(max(int(n_chars), 0), L)
    F = min(max(int(n_frames), 0), T)
    d = [max(int(x), 0) for x in list(dur)[:N]]
    total = sum(d)
    out = dict(pitch=np.zeros(L), energy=np.zeros(L), voiced=np.zeros(L, dtype=np.int64), q=np.zeros(F), e=np.zeros(F),
               stats=np.zeros(NSTAT))
    out["stats"][8] = 1.0 if total == F else 0.0
    if N == 0 or F == 0:
        return out
    q, voiced = frame_pitch(f0, F, log_pitch, interpolate)
    e = frame_energy(mel, F)
    s, unvoiced_chars = 0, 0
    for n in range(N):
        s0, s1 = min(s, F), min(s + d[n], F)
        s += d[n]
        span = range(s0, s1)
        nv = int(sum(voiced[t] for t in span))
        out["voiced"][n] = nv
        unvoiced_chars += nv == 0
        if interpolate:
            if len(span):
                out["pitch"][n] = math.fsum(q[t] for t in span) / len(span)
        elif nv:
            out["pitch"][n] = math.fsum(q[t] for t in span if voiced[t]) / nv
        if len(span):
            out["energy"][n] = math.fsum(e[t] for t in span) / len(span)
    pv = [q[t] for t in range(F) if voiced[t]]
    out["q"], out["e"] = q, e
    out["stats"][:8] = [F, len(pv), math.fsum(pv), math.fsum(x * x for x in pv), math.fsum(q), math.fsum(x * x for x in q),
                        math.fsum(e), math.fsum(x * x for x in e)]
    out["stats"][9] = unvoiced_chars
    return out


def char_variance_batch(dur, chars_len, frames_len, f0, mel, log_pitch=True, interpolate=False):
    """A batch: dur (B, L), f0 (B, T), mel (B, T, M).  Returns the list of per-utterance dicts."""
    L = np.asarray(dur).shape[1]
    return [char_variance(dur[b], chars_len[b], frames_len[b], f0[b], mel[b], L, log_pitch, interpolate) for b in range(len(dur))]
