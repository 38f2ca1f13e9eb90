"""Look-ahead true-peak limiter of a padded batch: one call into libtacotron2_amd.so (C-ABI t2_limit) on the current
stream.  analysis.limit_peaks IS this module's function, and loudness.normalize_loudness(limiter=) runs it between two t2_loudness
calls.  It needs no model, and its arguments are checked by _args before a pointer reaches a kernel."""
from __future__ import annotations

import math

import torch

from . import _args
from ._lib import cached, call, make, stream
from .loudness import CEILING_LIMITS, RATE_LIMITS, _limited

NSTAT, MAX_L = 8, 2048                       # the header's enum T2_LIMIT_NSTAT, T2_LIMIT_MAX_L (tests/test_limiter_ref_host.py)
PASS = 4096                                  # the samples of one pass of the curve launch (csrc/t2_limit.hip: LM_PASS)
STATS = ("in_peak", "n_over", "min_gain", "peak_after", "trim", "flags")      # the first columns of stat
FLAG_ACTIVE, FLAG_TRIMMED = 1, 2
LOOKAHEAD_LIMITS, RELEASE_LIMITS = (0.1, 20.0), (5.0, 2000.0)                  # ms
# ffmpeg alimiter's attack and release: product defaults, not measurements
LOOKAHEAD_MS, RELEASE_MS = 5.0, 50.0


def settings(fn: str, sample_rate, lookahead_ms=LOOKAHEAD_MS, release_ms=RELEASE_MS):
    """(sr, L, a) of t2_limit: L = round(lookahead_ms sr / 1000) clamped to 1 .. 2048 samples, a = exp(-1 / (release_s sr)) in float64."""
    sr = _args.int_arg(fn, "sample_rate", sample_rate, *RATE_LIMITS)
    lookahead_ms = _limited(fn, "lookahead_ms", lookahead_ms, LOOKAHEAD_LIMITS)
    release_ms = _limited(fn, "release_ms", release_ms, RELEASE_LIMITS)
    L = min(max(int(round(lookahead_ms * sr / 1000.0)), 1), MAX_L)
    return sr, L, math.exp(-1.0 / (release_ms / 1000.0 * sr))


def limit_peaks(wav, n, sample_rate, ceiling=-1.0, lookahead_ms=LOOKAHEAD_MS, release_ms=RELEASE_MS, return_curve=False):
    """A padded batch held under a true-peak ceiling by a look-ahead limiter (C-ABI t2_limit): wav (B, ld) float32 on
    the GPU (a strided view with a contiguous last dimension will do), n the B sample counts, 0 <= n[b] <= ld - host integers, or an
    integer tensor on the GPU, whose values the kernel checks: an entry out of range raises ValueError after the launch -,
    sample_rate an integer in 8000 .. 192000, ceiling in -40 .. 0 dBTP, lookahead_ms in 0.1 .. 20 (at most 2048 samples),
    release_ms in 5 .. 2000; the defaults 5 / 50 ms are ffmpeg alimiter's, product defaults and not measurements.  The gain curve
    comes down linearly over the look-ahead in front of a peak, sits at ceiling / peak on it and recovers exponentially; a row that
    stays under the ceiling keeps its bits.  Returns (y, stats): y of wav's shape, zeros behind n[b]; stats a dict of (B,) device
    tensors: in_peak (the 4x true peak of wav, linear), n_over (int64: the samples whose envelope is above the ceiling), min_gain
    (the lowest point of the curve), peak_after (the true peak of wav * curve), trim (the one last gain, 1 unless peak_after passed
    the ceiling by a hair), flags (int64: bit 0 active, bit 1 trimmed); with return_curve also env and curve, (B, ld) float32,
    defined inside n[b]."""
    fn = "limit_peaks"
    B, ld, ldx = _args.wav_rows(fn, "wav", wav)
    sr, L, a = settings(fn, sample_rate, lookahead_ms, release_ms)
    ceiling = _limited(fn, "ceiling", ceiling, CEILING_LIMITS)
    dev = wav.device
    n32, n_sum = _args.counts32(fn, "n", n, B, dev, hi=ld)
    _args.on_gpu(fn, "wav", wav)
    from .datasets.resample import plan
    _, _, K, table = plan(sr, 4 * sr)                                   # U = 4, D = 1: t2_resample's table for 4x, t2_loudness's
    with torch.cuda.device(dev):
        table = cached(("loudness", sr, dev), lambda: torch.from_numpy(table).to(dev))
        ldw = max(ld, 1)                                                # (a batch without a column still hands over pointers)
        env, curve, y = (torch.empty(B, ldw, dtype=torch.float32, device=dev) for _ in range(3))
        stat = torch.empty(B, NSTAT, dtype=torch.float64, device=dev)
        arg = make("T2Limit", x=wav if ld > 0 else None, ldx=ldx, n=n32, table=table, K=K, B=B, n_max=ld, L=L, a=a,
                   ceiling=10.0 ** (ceiling / 20.0), env=env, lde=ldw, curve=curve, ldc=ldw, y=y, ldy=ld, stat=stat)
        call("t2_limit", arg, stream())
        if n_sum is None and bool((stat[:, 5] < 0).any()):             # (device counts: the kernel's refusal is the one extra read)
            raise ValueError(f"{fn}: an n[b] outside 0 .. {ld} (refused on the device; nothing was written for it)")
    stats = {k: stat[:, i] for i, k in enumerate(STATS)}
    for k in ("n_over", "flags"):
        stats[k] = stats[k].to(torch.int64)
    if return_curve:
        stats.update(env=env[:, :ld], curve=curve[:, :ld])
    return y[:, :ld], stats
