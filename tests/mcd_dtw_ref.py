"""Float64 restatement of the scoring rule of DESIGN 5.9 (include/tacotron2_amd.h: t2_mel_cepstra, t2_dtw): mel-cepstral
coefficients, the frame distance, dynamic time warping with its backtrack, and the score.  numpy only; the recurrence is
vectorised by anti-diagonal (every cell of i + j = k depends on diagonals k-1 and k-2 only), so a 300 x 520 case takes a few
milliseconds.  Also the input generator of the GPU tests: smooth random trajectories and warped noisy copies of them."""
import numpy as np

MCD_SCALE = 10.0 * np.sqrt(2.0) / np.log(10.0)
U = 2.0 ** -24          # unit roundoff of float32


def basis(M: int, K: int) -> np.ndarray:
    """(M, K) float64: columns k = 1 .. K of the orthonormal DCT-II, sqrt(2/M) cos(pi k (m + 1/2) / M)."""
    m = np.arange(M, dtype=np.float64)[:, None] + 0.5
    k = np.arange(1, K + 1, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / M) * np.cos(np.pi * k * m / M)


def cepstra(x: np.ndarray, K: int = 13, w: np.ndarray = None) -> np.ndarray:
    """(..., M) log-mels -> (..., K) coefficients in float64 (w: another basis, e.g. the float32-rounded one)."""
    x = np.asarray(x, dtype=np.float64)
    return x @ (basis(x.shape[-1], K) if w is None else np.asarray(w, dtype=np.float64))


def distances(a: np.ndarray, b: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """(Ta, Tb) float64: scale * Euclidean distance between row i of a and row j of b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d2 = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):                     # (K passes over (Ta, Tb) instead of one (Ta, Tb, K) temporary)
        d2 += (a[:, k][:, None] - b[:, k][None, :]) ** 2
    return scale * np.sqrt(d2)


def dtw_matrix(d: np.ndarray):
    """DTW over a distance matrix (Ta, Tb): (cost, path (n, 2) int in forward order).  D[0][0] = d[0][0];
    D[i][j] = d[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]); ties: the diagonal, then (i-1, j), then (i, j-1)."""
    Ta, Tb = d.shape
    if Ta == 0 or Tb == 0:
        return 0.0, np.zeros((0, 2), dtype=np.int64)
    # Dp[i+1][j+1] = D[i][j]; a border of +inf excludes predecessors outside the matrix, Dp[0][0] = 0 starts the path
    Dp = np.full((Ta + 1, Tb + 1), np.inf)
    Dp[0, 0] = 0.0
    mv = np.zeros((Ta, Tb), dtype=np.uint8)
    for k in range(Ta + Tb - 1):
        i = np.arange(max(0, k - (Tb - 1)), min(Ta - 1, k) + 1)
        j = k - i
        cand = np.stack([Dp[i, j], Dp[i, j + 1], Dp[i + 1, j]])          # diagonal, (i-1, j), (i, j-1)
        m = np.argmin(cand, axis=0)                                      # the FIRST minimum: a later one wins only when strictly smaller
        Dp[i + 1, j + 1] = d[i, j] + cand[m, np.arange(len(i))]
        mv[i, j] = m
    path = []
    i, j = Ta - 1, Tb - 1
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        m = mv[i, j]
        i, j = i - (m != 2), j - (m != 1)
    return float(Dp[Ta, Tb]), np.array(path[::-1], dtype=np.int64)


def dtw(a: np.ndarray, b: np.ndarray, scale: float = 1.0):
    """(cost, path_len, path) between feature sequences (Ta, K) and (Tb, K); an empty side gives (0, 0, empty)."""
    if len(a) == 0 or len(b) == 0:
        return 0.0, 0, np.zeros((0, 2), dtype=np.int64)
    cost, path = dtw_matrix(distances(a, b, scale))
    return cost, len(path), path


def path_cost(d: np.ndarray, path: np.ndarray) -> float:
    return float(d[path[:, 0], path[:, 1]].sum())


def check_path(path: np.ndarray, Ta: int, Tb: int) -> None:
    """A warping path: from (0, 0) to (Ta-1, Tb-1) by steps (1, 1), (1, 0) or (0, 1)."""
    path = np.asarray(path)
    assert path.ndim == 2 and path.shape[1] == 2 and max(Ta, Tb) <= len(path) <= Ta + Tb - 1, (path.shape, Ta, Tb)
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (Ta - 1, Tb - 1), (path[0], path[-1])
    steps = {tuple(s) for s in np.diff(path, axis=0).tolist()}
    assert steps <= {(1, 1), (1, 0), (0, 1)}, steps


def mcd_dtw(mel_a: np.ndarray, mel_b: np.ndarray, K: int = 13):
    """(mcd, cost, path_len, path) between log-mels (Ta, M) and (Tb, M); mcd = cost / path_len, NaN for an empty side."""
    cost, n, path = dtw(cepstra(mel_a, K), cepstra(mel_b, K), MCD_SCALE)
    return (cost / n if n else float("nan")), cost, n, path


# ---- inputs of the GPU tests ------------------------------------------------------------------------------------------------------
def trajectory(rng, T: int, K: int, smooth: int = 9) -> np.ndarray:
    """(T, K) float32: a smooth random trajectory - a random walk under a moving average."""
    x = np.cumsum(rng.normal(size=(T + smooth - 1, K)), axis=0)
    ker = np.ones(smooth) / smooth
    y = np.stack([np.convolve(x[:, k], ker, mode="valid") for k in range(K)], axis=1)
    return (0.5 * y).astype(np.float32)


def warped_copy(rng, a: np.ndarray, Tb: int, noise: float = 0.05) -> np.ndarray:
    """(Tb, K) float32: `a` read along a random monotonic time map (first frame to first, last to last), plus noise."""
    Ta = a.shape[0]
    if Tb == 1 or Ta == 1:
        pos = np.zeros(Tb)
    else:
        inc = rng.uniform(0.2, 1.8, size=Tb - 1)
        pos = np.concatenate([[0.0], np.cumsum(inc)]) * (Ta - 1) / inc.sum()
    lo = np.clip(np.floor(pos).astype(int), 0, Ta - 1)
    hi = np.minimum(lo + 1, Ta - 1)
    f = (pos - lo)[:, None]
    b = (1 - f) * a[lo].astype(np.float64) + f * a[hi].astype(np.float64)
    return (b + noise * rng.normal(size=b.shape)).astype(np.float32)
