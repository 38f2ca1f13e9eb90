"""Float64 numpy restatement of t2_align_durations (include/tacotron2_amd.h): per-character durations from an alignment matrix, both
modes, and the four statistics - the reference of tests/test_durations_host.py and tests/test_gpu_durations.py.

The rule, per utterance with N characters, F frames, r frames per decoder step and S = ceil(F / r) steps:
  * step s < S - 1 carries r frames, the last one F - r*(S - 1); dur[n] = the frames of the steps assigned to n
  * argmax: pos[s] = the lowest n < N with the largest a[s][n]
  * monotonic: la = log(max(a, 1e-8)) in float64; Q[0][0] = la[0][0], Q[0][n>0] = -inf, Q[s][n] = la[s][n] + max(Q[s-1][n],
    Q[s-1][n-1]); the predecessor is n-1 only when Q[s-1][n-1] > Q[s-1][n] strictly; backtrack from (S-1, N-1)
  * S < N: no monotonic path - the argmax positions, feasible = 0
  * stats = (mean_s max_n a[s][n], mean_s la[s][pos_s], S >= N, share of steps with pos_s == argmax_s)
Only a[:S, :N] is read.  `durations` also returns the smallest |Q[s-1][n] - Q[s-1][n-1]| met at a decision on the chosen path:
equality of two implementations' paths is only meaningful when that margin is far above their rounding."""
import numpy as np

FLOOR = np.float32(1e-8)


def step_weights(F: int, r: int) -> np.ndarray:
    S = (F + r - 1) // r
    w = np.full(S, r, dtype=np.int64)
    if S:
        w[-1] = F - r * (S - 1)
    return w


def log_align(a: np.ndarray) -> np.ndarray:
    """la of the rule: the float32 value floored at 1e-8 (in float32, as fmaxf does), then log in float64."""
    return np.log(np.maximum(np.asarray(a, dtype=np.float32), FLOOR).astype(np.float64))


def monotonic_path(la: np.ndarray):
    """la (S, N) float64 with S >= N >= 1 -> (pos [S], score Q[S-1][N-1], smallest on-path decision margin)."""
    S, N = la.shape
    Q = np.full(N, -np.inf)
    Q[0] = la[0, 0]
    adv = np.zeros((S, N), dtype=bool)
    diff = np.full((S, N), np.inf)
    for s in range(1, S):
        prev = np.concatenate(([-np.inf], Q[:-1]))
        adv[s] = prev > Q
        with np.errstate(invalid="ignore"):
            d = np.abs(Q - prev)              # (-inf) - (-inf) = nan: an unreachable cell, never on the path
        diff[s] = np.where(np.isnan(d), np.inf, d)
        Q = la[s] + np.where(adv[s], prev, Q)
    pos = np.zeros(S, dtype=np.int64)
    n = N - 1
    margin = np.inf
    for s in range(S - 1, -1, -1):
        pos[s] = n
        if s > 0:
            margin = min(margin, diff[s, n])
        if adv[s, n]:
            n -= 1
    assert n == 0
    return pos, float(Q[N - 1]), float(margin)


def durations(a: np.ndarray, N: int, F: int, r: int = 1, mode: str = "monotonic"):
    """a (S_total, L) -> (dur int32 [L], stats float64 [4], margin).  N and F are clipped to L and r * S_total as the kernel does."""
    assert mode in ("monotonic", "argmax")
    St, L = a.shape
    N = min(max(int(N), 0), L)
    F = min(max(int(F), 0), r * St)
    S = (F + r - 1) // r
    dur = np.zeros(L, dtype=np.int32)
    stats = np.zeros(4)
    if N == 0 or S == 0:
        return dur, stats, np.inf
    v = np.asarray(a[:S, :N], dtype=np.float32)
    la = log_align(v)
    am = v.argmax(axis=1)                     # the first (lowest) position of the maximum
    feasible = S >= N
    margin = np.inf
    if mode == "monotonic" and feasible:
        pos, _, margin = monotonic_path(la)
    else:
        pos = am
    np.add.at(dur, pos, step_weights(F, r).astype(np.int32))
    idx = np.arange(S)
    stats[:] = (v.max(axis=1).astype(np.float64).mean(), la[idx, pos].mean(), float(feasible), float((pos == am).mean()))
    return dur, stats, margin


def durations_batch(a: np.ndarray, chars_len, frames_len, r: int = 1, mode: str = "monotonic"):
    """a (B, S, L) -> (dur int32 (B, L), stats float64 (B, 4), the smallest margin of the batch)."""
    out = [durations(a[b], int(chars_len[b]), int(frames_len[b]), r, mode) for b in range(a.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), min(o[2] for o in out)


def brute_force(la: np.ndarray):
    """Every monotonic path of (S, N), S >= N: (pos of the best, its score).  Ties are left to the caller's inputs (random: none)."""
    import itertools
    S, N = la.shape
    best, best_pos = -np.inf, None
    for cuts in itertools.combinations(range(1, S), N - 1):       # the steps at which the path advances
        pos = np.zeros(S, dtype=np.int64)
        for c in cuts:
            pos[c:] += 1
        sc = float(la[np.arange(S), pos].sum())
        if sc > best:
            best, best_pos = sc, pos
    return best_pos, best
