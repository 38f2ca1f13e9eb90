"""Float64 restatement of the sample-rate converter: the filter design of tacotron2_amd/datasets/resample.py and the rule of
t2_resample (include/tacotron2_amd.h), written from the formulas, sharing no code with either.

design(sr_in, sr_out) -> (U, D, K, table float64 (U, 2K)); apply(x, table, U, D, K) -> (y, bound): y[m] for m < ceil(n U / D) and the
a-priori fp32 bound of the kernel's result, (2K + 2) * 2^-24 * sum_k |h_k| |x_k| per output - one rounding of each tap to fp32, one
of each product-and-add (2K of them), with room for the input's own."""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 16, 0.90, 9.0


def design(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    U, D = sr_out // g, sr_in // g
    s = min(1.0, U / D)
    fc, W = ROLLOFF * s, ZEROS / s
    K = int(math.ceil(W))
    table = np.zeros((U, 2 * K), np.float64)
    for p in range(U):
        d = np.arange(-K + 1, K + 1) - p / U                   # tap k sits d input samples from the output's instant
        c = np.nonzero(np.abs(d) < W)[0]
        table[p, c] = fc * np.sinc(fc * d[c]) * np.i0(BETA * np.sqrt(1.0 - (d[c] / W) ** 2)) / np.i0(BETA)
        table[p] /= table[p].sum()
        table[p] /= table[p].sum()
    return U, D, K, table


def out_len(n, U, D):
    return (n * U + D - 1) // D


def apply(x, table, U, D, K, first=0):
    """The outputs m = first .. n_out - 1 of one signal x (n samples) in float64, and their fp32 error bounds."""
    x = np.asarray(x, np.float64)
    table = np.asarray(table, np.float64)
    n = len(x)
    m = np.arange(first, out_len(n, U, D), dtype=np.int64)
    md = m * D                                     # (int64: no 2^31 limit)
    i0, p = md // U, md % U
    idx = i0[:, None] + np.arange(-K + 1, K + 1, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < n)
    xs = np.where(ok, x[np.clip(idx, 0, max(n - 1, 0))] if n else 0.0, 0.0)
    h = table[p]
    y = np.zeros(len(m))
    for c in range(2 * K):                         # ascending k, as the kernel sums (float64 here: the order hardly matters)
        y += h[:, c] * xs[:, c]
    bound = (2 * K + 2) * 2.0 ** -24 * (np.abs(h) * np.abs(xs)).sum(1)
    return y, bound


def db(err, ref=1.0):
    return 20 * math.log10(max(float(err), 1e-300) / ref)
