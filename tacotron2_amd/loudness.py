"""Programme loudness, true peak and loudness normalisation of a padded batch: ITU-R BS.1770-4 for one channel, one call
into libtacotron2_amd.so (C-ABI t2_loudness) on the current stream.  analysis.loudness and analysis.normalize_loudness ARE this
module's functions: they need no model, and their arguments are checked by _args before a pointer reaches a kernel."""
from __future__ import annotations

import functools
import math

import torch

from . import _args
from ._lib import K, cached, call, make, stream

NSTAT = K["LOUD_NSTAT"]
STATS = ("lufs", "gain", "true_peak", "sample_peak", "n_blocks", "n_below_abs", "n_below_rel", "rel_gate_lufs",
         "momentary_max_lufs", "flags")     # the columns of stat
FLAG_SHORT, FLAG_UNDEFINED, FLAG_LIMITED, FLAG_CAPPED = 1, 2, 4, 8
RATE_LIMITS = (8000, 192000)
TARGET_LIMITS, CEILING_LIMITS, MAX_GAIN_LIMITS = (-70.0, 0.0), (-40.0, 0.0), (0.0, 120.0)
# the largest boost normalize_loudness applies unless told otherwise: 30 dB keeps a nearly silent row from being blown up into its
# own noise.  A product default, not a measurement.
MAX_GAIN_DB = 30.0
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)  # the absolute gate, -70 LUFS, as a mean square


@functools.lru_cache(maxsize=None)
def k_weighting(sr: int):
    """The K-weighting of BS.1770 at sr Hz, (b1, a1, b2, a2) as tuples of three float64 each: the shelf and the high-pass, re-derived
    for any rate from the analogue prototypes (libebur128's way) through K = tan(pi f0 / sr).  At 48 000 Hz these are the
    standard's table to 1e-15.  Cached per rate."""
    sr = _args.int_arg("k_weighting", "sr", sr, *RATE_LIMITS)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0)
    a1 = (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    b2 = (1.0, -2.0, 1.0)
    a2 = (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    return b1, a1, b2, a2


def hop(sr: int) -> int:
    """H, the samples of 100 ms: a block is 4 H."""
    return int(round(sr / 10))


def _limited(fn: str, name: str, v, limits) -> float:
    v = _args.real_arg(fn, name, v)
    if not limits[0] <= v <= limits[1]:
        raise ValueError(f"{fn}: {name} must lie in {limits[0]:g} .. {limits[1]:g}, got {v!r}")
    return v


def _run(fn: str, wav, n, sample_rate, target, ceiling, max_gain_db, write: bool, lift: bool = False):
    """lift: the ceiling is checked and then lifted out of reach, so the gain is bounded by max_gain_db alone (the limiter path)."""
    B, ld, ldx = _args.wav_rows(fn, "wav", wav)
    sr = _args.int_arg(fn, "sample_rate", sample_rate, *RATE_LIMITS)
    target = _limited(fn, "target", target, TARGET_LIMITS)
    ceiling = _limited(fn, "ceiling", ceiling, CEILING_LIMITS)
    max_gain_db = _limited(fn, "max_gain_db", max_gain_db, MAX_GAIN_LIMITS)
    dev = wav.device
    n32, n_sum = _args.counts32(fn, "n", n, B, dev, hi=ld)
    _args.on_gpu(fn, "wav", wav)
    b1, a1, b2, a2 = k_weighting(sr)
    H = hop(sr)
    from .datasets.resample import plan
    _, _, K, table = plan(sr, 4 * sr)                                   # U = 4, D = 1, K = 16: t2_resample's table for 4x
    with torch.cuda.device(dev):
        table = cached(("loudness", sr, dev), lambda: torch.from_numpy(table).to(dev))
        lde = max(ld // H, 1)
        E = torch.empty(B, lde, dtype=torch.float64, device=dev)
        stat = torch.empty(B, NSTAT, dtype=torch.float64, device=dev)
        gain = torch.empty(B, dtype=torch.float32, device=dev)
        y = torch.empty(B, ld, dtype=torch.float32, device=dev) if write else None
        a = make("T2Loudness", x=wav if ld > 0 else None, ldx=ldx, n=n32, table=table, K=K, B=B, n_max=ld, H=H, b1=b1, a1=a1, b2=b2,
                 a2=a2, abs_gate=ABS_GATE, target=target, max_gain=10.0 ** (max_gain_db / 20.0), ceiling=1.7e308 if lift else 10.0 ** (ceiling / 20.0),
                 E=E, lde=lde, stat=stat, gain=gain, y=y if write and ld > 0 else None, ldy=ld)
        call("t2_loudness", a, stream())
        if n_sum is None and bool((stat[:, 9] < 0).any()):             # (device counts: the kernel's refusal is the one extra read)
            raise ValueError(f"{fn}: an n[b] outside 0 .. {ld} (refused on the device; nothing was written for it)")
    stats = {k: stat[:, i] for i, k in enumerate(STATS) if k != "gain"}
    for k in ("n_blocks", "n_below_abs", "n_below_rel", "flags"):
        stats[k] = stats[k].to(torch.int64)
    return y, gain, stats


def loudness(wav, n, sample_rate):
    """The programme loudness and the peaks of a padded batch (C-ABI t2_loudness; ITU-R BS.1770-4, one channel): wav (B,
    ld) float32 on the GPU (a strided view with a contiguous last dimension will do), n the B sample counts, 0 <= n[b] <= ld - host
    integers, or an integer tensor on the GPU, whose values the kernel checks: an entry out of range raises ValueError after the
    launch -, sample_rate an integer in 8000 .. 192000.  Returns a dict of (B,) device tensors: lufs (float64, NaN for a row
    without a block above -70 LUFS), true_peak (4x oversampled, linear), sample_peak, n_blocks, n_below_abs, n_below_rel (int64),
    rel_gate_lufs, momentary_max_lufs and flags (int64: bit 0 short - a row below 400 ms is one block of all its samples -, bit 1
    undefined).  Writes no waveform.  Needs no model."""
    _, _, stats = _run("loudness", wav, n, sample_rate, -23.0, -1.0, MAX_GAIN_DB, False)
    return stats


def normalize_loudness(wav, n, sample_rate, target=-23.0, ceiling=-1.0, max_gain_db=MAX_GAIN_DB, limiter=None):
    """A padded batch brought to `target` LUFS (C-ABI t2_loudness): wav, n and sample_rate as loudness takes them;
    target in -70 .. 0 LUFS, ceiling in -40 .. 0 dBTP, max_gain_db in 0 .. 120.  Every row is multiplied by ONE gain,
    10^((target - lufs) / 20), lowered to max_gain_db (flag bit 3, capped) and then until gain * true_peak is at most the ceiling
    (flag bit 2, limited): a plain gain, no limiter, no compression.  A row without a loudness keeps the gain 1.  Returns (y, stats):
    y of wav's shape, zeros behind n[b]; stats = loudness's dict - the MEASURED values of wav, not of y - plus gain (float32).
    limiter: None - the above, nothing else runs.  True, or a dict of lookahead_ms / release_ms (limiter.limit_peaks), holds the
    ceiling with a look-ahead limiter instead, three library calls: t2_loudness with the ceiling lifted out of reach, so
    the gain is bounded by max_gain_db alone and `limited` is never set; t2_limit on that waveform with the ceiling; t2_loudness once
    more, measuring.  stats then also holds limit_peaks' in_peak, n_over, min_gain, peak_after, trim and its flags as limiter_flags,
    and output_lufs and output_true_peak, measured on y.  A row without a loudness keeps its bits through all three."""
    if limiter is None:
        y, gain, stats = _run("normalize_loudness", wav, n, sample_rate, target, ceiling, max_gain_db, True)
        return y, dict(stats, gain=gain)
    from . import limiter as lim
    fn = "normalize_loudness"
    if limiter is True:
        limiter = {}
    if not isinstance(limiter, dict) or set(limiter) - {"lookahead_ms", "release_ms"}:
        raise ValueError(f"{fn}: limiter must be None, True or a dict of lookahead_ms / release_ms, got {limiter!r}")
    lim.settings(fn, sample_rate, **limiter)                             # (checked in front of the first launch)
    g, gain, stats = _run(fn, wav, n, sample_rate, target, ceiling, max_gain_db, True, lift=True)
    y, more = lim.limit_peaks(g, n, sample_rate, ceiling=ceiling, **limiter)
    _, _, after = _run(fn, y, n, sample_rate, target, ceiling, max_gain_db, False)
    more["limiter_flags"] = more.pop("flags")
    return y, dict(stats, gain=gain, output_lufs=after["lufs"], output_true_peak=after["true_peak"], **more)
