"""Time stretching and pitch shifting of a padded batch of waveforms: WSOLA as one call into libtacotron2_amd.so (C-ABI
t2_stretch) on the current stream, and for the pitch a resampling (t2_resample) behind it.  analysis.time_stretch and
analysis.pitch_shift ARE this module's functions: they need no model, and their arguments are checked by _args before a pointer reaches
a kernel."""
from __future__ import annotations

import math

import torch

from . import _args
from ._lib import K, cached, call, make, stream

MAX_FRAME, MAX_TOLERANCE = K["STRETCH_MAX_N"], K["STRETCH_MAX_D"]
MAX_SAMPLES = 1 << 27                       # t2_stretch's n_max, and t2_psola's
TEMPO_RANGE = (0.25, 4.0)
RATIO_RANGE = (0.125, 8.0)                  # t2_stretch's P / Q: what a pitch shift may ask of the stretch (4 x 2 octaves is refused)
SEMITONE_RANGE = (-24.0, 24.0)              # of pitch_shift, and of pitch_shift_psola


def hann_table(N: int):
    """The periodic Hann window of N points, float32 from fp64: w[k] = 0.5 - 0.5 cos(2 pi k / N), so that w[k] + w[k + N / 2] = 1.
    A host (numpy) array; time_stretch uploads it once per length and device."""
    import numpy as np
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def tempo_ratio(fn: str, tempo):
    """The tempo as the rational (P, Q): a (P, Q) pair of positive integers as it is, a real rounded to 1/1000 (Q = 1000); either way
    0.25 <= P / Q <= 4."""
    if isinstance(tempo, (tuple, list)):
        if len(tempo) != 2:
            raise ValueError(f"{fn}: tempo must be a number or a (P, Q) pair of integers, got {tempo!r}")
        P, Q = _args.int_arg(fn, "tempo P", tempo[0], 1, 1 << 20), _args.int_arg(fn, "tempo Q", tempo[1], 1, 1 << 20)
    else:
        P, Q = int(round(_args.real_arg(fn, "tempo", tempo) * 1000.0)), 1000
    if P < TEMPO_RANGE[0] * Q or P > TEMPO_RANGE[1] * Q:
        raise ValueError(f"{fn}: tempo must lie in {TEMPO_RANGE[0]} .. {TEMPO_RANGE[1]}, got {tempo!r}")
    return P, Q


def out_len(n: int, P: int, Q: int) -> int:
    """ceil(n Q / P): the samples t2_stretch writes for n input samples."""
    return -((-int(n) * int(Q)) // int(P))


def window_args(fn: str, frame, tolerance):
    N = _args.int_arg(fn, "frame", frame, 4, MAX_FRAME)
    if N % 2:
        raise ValueError(f"{fn}: frame must be even, got {N}")
    return N, _args.int_arg(fn, "tolerance", tolerance, 0, MAX_TOLERANCE)


def time_stretch(wav, n, tempo, frame=1024, tolerance=256):
    """A padded batch played at `tempo` times its speed without a change of pitch (C-ABI t2_stretch): wav (B, ld) float32
    on the GPU (a strided view with a contiguous last dimension will do), n the B sample counts, 0 <= n[b] <= ld.  WSOLA with a
    periodic Hann window of `frame` samples (even, 4 .. 2048) at a hop of frame / 2; each frame is moved by at most `tolerance`
    samples (0 .. 1024) to where it best continues the frame before it, found by an integer correlation.  tempo: a real, rounded to
    1/1000, or a (P, Q) pair of integers, in 0.25 .. 4.
    Returns (y (B, ld') float32 with zeros behind each row, n_out = ceil(n[b] Q / P), pos (B, M') int32: the input sample at which
    output frame m starts, zeros behind a row's ceil(n_out / (frame / 2)) + 1 frames).  n as host integers keeps the call free of
    host reads and gives n_out as host integers; a tensor on the GPU is checked by the kernel and costs one read, that of n_out (a
    list): an entry out of range raises ValueError after the launch, nothing being read or written for it.
    A tempo of exactly 1 launches nothing: (wav, n, None) comes back, wav being the argument itself.  Needs no model."""
    fn = "time_stretch"
    _args.tensor_arg(fn, "wav", wav, 2, "(B, samples)")
    return _stretch(fn, wav, n, tempo_ratio(fn, tempo), frame, tolerance)


def _stretch(fn: str, wav, n, ratio, frame, tolerance):
    """time_stretch behind its tempo check, for the caller `fn`: ratio = (P, Q) within t2_stretch's range."""
    P, Q = ratio
    N, D = window_args(fn, frame, tolerance)
    B, ld, ldx = _args.wav_rows(fn, "wav", wav, MAX_SAMPLES)
    dev = wav.device
    n32, n_sum = _args.counts32(fn, "n", n, B, dev, hi=ld)
    _args.on_gpu(fn, "wav", wav)
    if P == Q:
        return wav, (n if n_sum is None else [int(v) for v in n]), None
    Hs = N // 2
    n_max = ld if n_sum is None else max(int(v) for v in n)
    top = out_len(n_max, P, Q)
    ldy, ldp = (top + 63) // 64 * 64, -(-top // Hs) + 1
    with torch.cuda.device(dev):
        w = cached(("hann", N, dev), lambda: torch.from_numpy(hann_table(N)).to(dev))
        y = torch.empty(B, ldy, dtype=torch.float32, device=dev)
        pos = torch.empty(B, ldp, dtype=torch.int32, device=dev)
        n_out = torch.empty(B, dtype=torch.int32, device=dev)
        a = make("T2Stretch", x=wav if ld > 0 else None, ldx=ldx, n=n32, w=w, B=B, n_max=n_max, N=N, D=D, P=P, Q=Q,
                 y=y if ldy > 0 else None, ldy=ldy, pos=pos, ldp=ldp, n_out=n_out)
        call("t2_stretch", a, stream())
        if n_sum is None:
            counts = n_out.tolist()
            if min(counts) < 0:
                raise ValueError(f"{fn}: an n[b] outside 0 .. {ld} (refused on the device; nothing was written for it)")
        else:
            counts = [out_len(v, P, Q) for v in n]
    return y, counts, pos


def pitch_plan(fn: str, semitones, sample_rate, tempo=1.0):
    """(sr_mid, effective tempo, stretch ratio (P, 1000)) of a pitch shift: f = 2^(semitones / 12); sr_mid = round(sample_rate f / 50)
    * 50 - a multiple of 50 keeps the resampler's ratio small: at most sample_rate / 50 phases, a pitch error of at most
    1200 log2(1 + 25 / sr_mid) cents -; the stretch runs at round(1000 tempo sample_rate / sr_mid) / 1000 and the resampling
    sr_mid -> sample_rate undoes the change of length, so the effective tempo is that ratio times sr_mid / sample_rate."""
    semitones = _args.real_arg(fn, "semitones", semitones)
    if not SEMITONE_RANGE[0] <= semitones <= SEMITONE_RANGE[1]:
        raise ValueError(f"{fn}: semitones must lie in {SEMITONE_RANGE[0]:g} .. {SEMITONE_RANGE[1]:g}, got {semitones!r}")
    sr = _args.int_arg(fn, "sample_rate", sample_rate, 1000)
    tempo = _args.real_arg(fn, "tempo", tempo)
    if not TEMPO_RANGE[0] <= tempo <= TEMPO_RANGE[1]:
        raise ValueError(f"{fn}: tempo must lie in {TEMPO_RANGE[0]} .. {TEMPO_RANGE[1]}, got {tempo!r}")
    sr_mid = int(round(sr * math.pow(2.0, semitones / 12.0) / 50.0)) * 50
    P = int(round(1000.0 * tempo * sr / sr_mid))
    if P < RATIO_RANGE[0] * 1000 or P > RATIO_RANGE[1] * 1000:
        raise ValueError(f"{fn}: {semitones:g} semitones at tempo {tempo:g} need a stretch by {P / 1000:g}, outside "
                         f"{RATIO_RANGE[0]} .. {RATIO_RANGE[1]}")
    return sr_mid, (P / 1000.0) * sr_mid / sr, (P, 1000)


def pitch_shift(wav, n, semitones, sample_rate, tempo=1.0, frame=1024, tolerance=256):
    """A padded batch raised by `semitones` (-24 .. 24) and played at `tempo` times its speed: time_stretch by the ratio of
    pitch_plan, then datasets.resample.Resampler(sample_rate).batch(.., sr_in=sr_mid) - the stretched signal read as one of sr_mid
    Hz and brought back to sample_rate.  Formants move with the pitch.  wav and n as time_stretch takes them (a device n is read
    back: the resampler wants host counts).  Returns (y (B, ld') float32, n_out host integers, the effective tempo, sr_mid); with
    semitones so small that sr_mid == sample_rate and a stretch ratio of 1 nothing is launched and wav itself comes back."""
    from . import voice
    plan = voice.plan_voice("pitch_shift", sample_rate, tempo, semitones, frame=frame, tolerance=tolerance)
    y, counts = voice.run_voice(plan, wav, n, fn="pitch_shift")
    return y, counts, plan.tempo, plan.sr_mid
