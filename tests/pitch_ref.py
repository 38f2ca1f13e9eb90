"""The rules of include/tacotron2_amd.h's t2_pitch_viterbi and t2_f0_path_stats restated in numpy float64, and the
octave signal of their tests.  The Viterbi recurrence has additions only, in the header's association, so the kernel's lags, its
cost and its aperiodicities are these bit for bit on the same float32 inputs.  Nothing here imports the package."""
import numpy as np

DEFAULTS = dict(w=1.0, max_jump=0.25, u=0.3, c_sw=0.15)


def lag_weights(tau_min, tau_max, w):
    """lw[k] = w * log2(tau_min + k), float64 [N], N = tau_max - tau_min: the table the host hands to the kernel."""
    return np.float64(w) * np.log2(np.arange(tau_min, tau_max, dtype=np.float64))


def parabolic_f0(cm, lag, sr, dtype=np.float64):
    """t2_yin's interpolation of one frame around `lag`, in `dtype`."""
    ft = np.dtype(dtype).type
    a, m, e = ft(cm[lag - 1]), ft(cm[lag]), ft(cm[lag + 1])
    den = a - ft(2) * m + e
    off = ft(0.5) * (a - e) / den if den > 0 else ft(0)
    off = min(max(off, ft(-1)), ft(1))
    return ft(sr) / (ft(lag) + off)


def viterbi(cm, power, n_frames, tau_min, tau_max, lw, trans_max, u, c_sw, power_floor, sr):
    """One utterance: cm (T, tau_max + 1) float32, power (T,) float32, n_frames = len[b] already clipped to 0 .. T.
    dict(lag int64 (T,), aper float32 (T,), f0 float64 (T,), f0_32 float32 (T,) - the float32 restatement of the formula -, cost)."""
    T = cm.shape[0]
    N = tau_max - tau_min
    lw = np.asarray(lw, np.float64)
    inf = np.float64(np.inf)
    u, c_sw, trans_max = np.float64(u), np.float64(c_sw), np.float64(trans_max)
    out = dict(lag=np.zeros(T, np.int64), aper=np.ones(T, np.float32), f0=np.zeros(T, np.float64), f0_32=np.zeros(T, np.float32),
               cost=np.float64(0.0))
    if n_frames == 0:
        return out

    def local(t):
        row = np.full(N + 1, inf)
        if power[t] > np.float32(power_floor):
            row[:N] = cm[t, tau_min:tau_max].astype(np.float64)
        row[N] = u
        return row

    trans = np.abs(lw[None, :] - lw[:, None])                    # [from k'][to k]
    allowed = trans <= trans_max
    D = local(0)
    back = np.zeros((n_frames, N + 1), np.int64)
    for t in range(1, n_frames):
        new = np.empty(N + 1)
        for k in range(N):                                       # voiced target: voiced predecessors ascending, then U
            best, arg = inf, -1
            for kp in np.nonzero(allowed[:, k])[0]:
                c = D[kp] + trans[kp, k]
                if arg < 0 or c < best:
                    best, arg = c, kp
            c = D[N] + c_sw
            if arg < 0 or c < best:
                best, arg = c, N
            new[k], back[t, k] = best, arg
        best, arg = D[N] + np.float64(0.0), N                    # target U: U first, then the voiced ascending
        for kp in range(N):
            c = D[kp] + c_sw
            if c < best:
                best, arg = c, kp
        new[N], back[t, N] = best, arg
        D = new + local(t)
    s = 0                                                        # the first minimum over the voiced states, then U
    for k in range(1, N + 1):
        if D[k] < D[s]:
            s = k
    out["cost"] = D[s]
    for t in range(n_frames - 1, -1, -1):
        if s < N:
            lag = tau_min + s
            out["lag"][t] = lag
            out["aper"][t] = cm[t, lag]
            out["f0"][t] = parabolic_f0(cm[t], lag, sr, np.float64)
            out["f0_32"][t] = parabolic_f0(cm[t], lag, sr, np.float32)
        s = back[t, s]
    return out


def viterbi_fast(cm, power, n_frames, tau_min, tau_max, lw, trans_max, u, c_sw, power_floor, sr):
    """The same rule with the inner loops as array operations (np.argmin returns the first minimum, which is the ascending-order,
    strictly-smaller rule); test_pitch_host.py holds it to viterbi() on small inputs, the larger cases use it."""
    T = cm.shape[0]
    N = tau_max - tau_min
    lw = np.asarray(lw, np.float64)
    inf = np.float64(np.inf)
    u, c_sw, trans_max = np.float64(u), np.float64(c_sw), np.float64(trans_max)
    out = dict(lag=np.zeros(T, np.int64), aper=np.ones(T, np.float32), f0=np.zeros(T, np.float64), f0_32=np.zeros(T, np.float32),
               cost=np.float64(0.0))
    if n_frames == 0:
        return out
    trans = np.abs(lw[None, :] - lw[:, None])
    trans = np.where(trans <= trans_max, trans, inf)             # (+inf never wins over U's finite candidate, nor a first finite one)
    first_allowed = np.argmax(np.isfinite(trans), axis=0)

    def local(t):
        row = np.full(N + 1, inf)
        if power[t] > np.float32(power_floor):
            row[:N] = cm[t, tau_min:tau_max].astype(np.float64)
        row[N] = u
        return row

    D = local(0)
    back = np.zeros((n_frames, N + 1), np.int64)
    for t in range(1, n_frames):
        cand = D[:N, None] + trans                               # [k'][k]
        arg = np.argmin(cand, axis=0)
        best = cand[arg, np.arange(N)]
        allinf = ~np.isfinite(best)                              # every candidate +inf: the first ALLOWED one stands
        arg = np.where(allinf, first_allowed, arg)
        cu = D[N] + c_sw
        take_u = cu < best
        new = np.empty(N + 1)
        new[:N] = np.where(take_u, cu, best)
        back[t, :N] = np.where(take_u, N, arg)
        cv = D[:N] + c_sw
        kv = int(np.argmin(cv))
        if cv[kv] < D[N] + np.float64(0.0):
            new[N], back[t, N] = cv[kv], kv
        else:
            new[N], back[t, N] = D[N] + np.float64(0.0), N
        D = new + local(t)
    s = int(np.argmin(D[:N]))
    if D[N] < D[s]:
        s = N
    out["cost"] = D[s]
    for t in range(n_frames - 1, -1, -1):
        if s < N:
            lag = tau_min + s
            out["lag"][t] = lag
            out["aper"][t] = cm[t, lag]
            out["f0"][t] = parabolic_f0(cm[t], lag, sr, np.float64)
            out["f0_32"][t] = parabolic_f0(cm[t], lag, sr, np.float32)
        s = back[t, s]
    return out


def frame_valid(t, n, hop, S, T):
    """t2_prosody_stats' rule, plus `t inside the track`."""
    s0 = t * hop - S // 2
    return 0 <= t < T and s0 >= 0 and s0 + S <= n


F0_NSTAT = 12


def f0_path_stats(path, path_len, f0_a, n_a, f0_b, n_b, hop, S):
    """One pair: path (P, 2) ints, tracks in Hz (0 = unvoiced).  (row [12] float64, abs [12] float64: the sums of |term| behind every
    sum field, for the bound of the GPU test)."""
    row, mag = np.zeros(F0_NSTAT), np.zeros(F0_NSTAT)
    for s in range(int(path_len)):
        i, j = int(path[s][0]), int(path[s][1])
        if not (frame_valid(i, n_a, hop, S, len(f0_a)) and frame_valid(j, n_b, hop, S, len(f0_b))):
            continue
        fa, fb = np.float64(f0_a[i]), np.float64(f0_b[j])
        va, vb = fa > 0, fb > 0
        row[0] += 1
        if va and vb:
            row[1] += 1
            la, lb = np.log2(fa), np.log2(fb)
            d = 1200.0 * (la - lb)
            terms = [d, d * d, la, lb, la * la, lb * lb, la * lb]
            for q, v in enumerate(terms):
                row[4 + q] += v
                mag[4 + q] += abs(v)
        elif va:
            row[2] += 1
        elif vb:
            row[3] += 1
    return row, mag


def f0_figures(row):
    """The host-side figures of one row: dict(n_pairs, n_voiced_both, f0_rmse_cents, f0_bias_cents, f0_corr, vuv_error); None
    where undefined."""
    n, nb = int(row[0]), int(row[1])
    out = dict(n_pairs=n, n_voiced_both=nb, f0_rmse_cents=None, f0_bias_cents=None, f0_corr=None, vuv_error=None)
    if n > 0:
        out["vuv_error"] = (row[2] + row[3]) / n
    if nb > 0:
        out["f0_rmse_cents"] = float(np.sqrt(row[5] / nb))
        out["f0_bias_cents"] = float(row[4] / nb)
    if nb >= 2:
        va = row[8] - row[6] * row[6] / nb
        vb = row[9] - row[7] * row[7] / nb
        if va > 1e-12 * row[8] and vb > 1e-12 * row[9]:          # (a constant column leaves rounding noise, not variance)
            out["f0_corr"] = float((row[10] - row[6] * row[7] / nb) / np.sqrt(va * vb))
    return out


def octave_signal():
    """110 Hz with a strong second harmonic whose fundamental fades twice: the raw YIN rule (smallest lag under the threshold) reads
    frames of the faded stretches an octave high.  float32 [16000] at 22050 Hz."""
    n, sr, f = 16000, 22050, 110.0
    t = np.arange(n) / sr
    fund = np.sin(2 * np.pi * f * t) + 0.3 * np.sin(2 * np.pi * 3 * f * t)
    even = np.sin(2 * np.pi * 2 * f * t)
    g = np.ones(n)
    g[5000:6500] = 0.12
    g[9000:9800] = 0.12
    x = 0.2 * (g * fund + even) + 0.002 * np.random.default_rng(1).normal(size=n)
    return x.astype(np.float32)
