"""Per-character pitch and energy on the duration grid: one call into libtacotron2_amd.so (C-ABI t2_char_variance) on
the current stream.  analysis.char_variance IS this module's function: it needs no model, and its arguments are checked by _args
before a pointer reaches the kernel, as those of every other measurement of analysis are."""
from __future__ import annotations

import torch

from . import _args
from ._lib import K, call, make

VAR_MAX_T = K["VAR_MAX_T"]            # frames of one utterance (q and e as doubles in LDS)
VAR_MAX_L = K["VAR_MAX_L"]            # characters of one utterance
VAR_NSTAT = K["VAR_NSTAT"]
VAR_STATS = ["n_frames", "n_voiced", "sum_p", "sum_p2", "sum_q", "sum_q2", "sum_e", "sum_e2", "consistent", "chars_unvoiced"]


def char_variance(dur, chars_len, frames_len, f0, mel, log_pitch=True, interpolate=False, return_frames=False):
    """Pitch and energy per character from per-character durations: dur (B, L) int32 as Engine.durations gives them, chars_len and
    frames_len (B,) integers, f0 (B, T) float32 in Hz (yin's track or pitch_viterbi's, 0 = unvoiced) and the log-mel (B, T, M)
    float32 on the same grid, all on one GPU; f0, mel and dur may be strided views with a contiguous last dimension.  Character n
    of utterance b covers the frames [sum dur[b][:n], + dur[b][n]), clipped to frames_len[b].
    Returns (out, stats): out["pitch"] (B, L) float32 - log_pitch: of ln f0, else of Hz; interpolate False: the mean over the span's
    voiced frames, 0 without one (FastPitch); True: the mean over all its frames of the track interpolated linearly across the
    unvoiced stretches, the end values held (FastSpeech 2) -, out["energy"] (B, L) float32 = the mean of the frames' L2 norm of the
    mel magnitudes, out["voiced"] (B, L) int32 = the span's voiced frames; with return_frames also out["pitch_frames"] and
    out["energy_frames"] (B, T) float32, 0 behind frames_len.  stats (B, 10) float64, the columns VAR_STATS: the frames, the voiced
    frames, the sums of p and p^2 over the voiced frames, of the filled pitch q and q^2 and of the energy e and e^2 over all frames,
    consistent (the durations sum to frames_len) and the characters without a voiced frame.  Needs no model."""
    fn = "char_variance"
    # (types, shapes and strides first - they need no device -, then where the tensors live)
    _args.tensor_arg(fn, "f0", f0, 2, "(B, T)")
    _args.tensor_arg(fn, "mel", mel, 3, "(B, T, M)")
    _args.tensor_arg(fn, "dur", dur, 2, "(B, L)", torch.int32)
    B, T = f0.shape
    _args.batch_arg(fn, B)
    if T < 1 or T > VAR_MAX_T:
        raise ValueError(f"{fn}: {T} frames, outside 1 .. {VAR_MAX_T} (T2_VAR_MAX_T)")
    if mel.shape[0] != B or mel.shape[1] != T or mel.shape[2] < 1:
        raise ValueError(f"{fn}: mel of shape {tuple(mel.shape)}, f0 of shape {tuple(f0.shape)}: need ({B}, {T}, M >= 1)")
    L = dur.shape[1]
    if dur.shape[0] != B or L < 1 or L > VAR_MAX_L:
        raise ValueError(f"{fn}: dur of shape {tuple(dur.shape)}: need ({B}, L) with L in 1 .. {VAR_MAX_L} (T2_VAR_MAX_L)")
    _args.last_contiguous(fn, "f0", f0)
    _args.last_contiguous(fn, "dur", dur)
    ld_b, ld_t = _args.strided_3d(fn, "mel", mel)
    ld_f0 = f0.stride(0) if B > 1 else T
    ld_dur = dur.stride(0) if B > 1 else L
    if ld_f0 < T or ld_dur < L:
        raise ValueError(f"{fn}: overlapping rows of f0 or dur (row strides {ld_f0}, {ld_dur})")
    _args.on_gpu(fn, "f0", f0)
    _args.on_device(fn, "mel", mel, f0.device)
    _args.on_device(fn, "dur", dur, f0.device)
    clen = _args.lengths(fn, "chars_len", chars_len, B, f0.device).to(torch.int32).contiguous()
    flen = _args.lengths(fn, "frames_len", frames_len, B, f0.device).to(torch.int32).contiguous()
    dev = f0.device
    with torch.cuda.device(dev):
        pitch, energy = (torch.empty(B, L, dtype=torch.float32, device=dev) for _ in range(2))
        voiced = torch.empty(B, L, dtype=torch.int32, device=dev)
        stats = torch.empty(B, VAR_NSTAT, dtype=torch.float64, device=dev)
        fp = fe = None
        if return_frames:
            fp, fe = (torch.zeros(B, T, dtype=torch.float32, device=dev) for _ in range(2))
        a = make("T2CharVariance", f0=f0, ld_f0=ld_f0, mel=mel, ld_b=ld_b, ld_t=ld_t, dur=dur, ld_dur=ld_dur, B=B, T=T, L=L,
                 M=mel.shape[2], log_pitch=1 if log_pitch else 0, interpolate=1 if interpolate else 0, chars_len=clen, frames_len=flen,
                 char_pitch=pitch, char_energy=energy, char_voiced=voiced, frame_pitch=fp, frame_energy=fe, stats=stats)
        call("t2_char_variance", a, torch.cuda.current_stream().cuda_stream)
    out = dict(pitch=pitch, energy=energy, voiced=voiced)
    if return_frames:
        out.update(pitch_frames=fp, energy_frames=fe)
    return out, stats


def pooled(rows) -> dict:
    """Mean, standard deviation (population), minimum, maximum and count of the values behind per-utterance rows (count, sum, sum of
    squares, minimum, maximum), pooled on the host in float64; None where the count is 0."""
    import math
    n = sum(int(r[0]) for r in rows)
    if n == 0:
        return dict(count=0, mean=None, std=None, min=None, max=None)
    s, s2 = math.fsum(float(r[1]) for r in rows), math.fsum(float(r[2]) for r in rows)
    mean = s / n
    return dict(count=n, mean=mean, std=math.sqrt(max(s2 / n - mean * mean, 0.0)),
                min=min(float(r[3]) for r in rows if int(r[0]) > 0), max=max(float(r[4]) for r in rows if int(r[0]) > 0))
