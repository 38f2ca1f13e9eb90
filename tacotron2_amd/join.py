"""Joining a padded batch of synthesised pieces into one waveform: one call into libtacotron2_amd.so (C-ABI t2_join) on
the current stream.  analysis.join_audio IS this module's function: it needs no model, and its arguments are checked by _args before
a pointer reaches a kernel."""
from __future__ import annotations

import torch

from . import _args
from ._lib import cached, call, make, stream


def fade_table(fade: int):
    """The rising half of a Hann window at the centres of `fade` steps, float32 from fp64: w[k] = 0.5 - 0.5 cos(pi (k + 0.5) / fade).
    A host (numpy) array; join_audio uploads it once per length and device."""
    import numpy as np
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(fade, dtype=np.float64) + 0.5) / max(fade, 1))).astype(np.float32)


def join_audio(wav, n, pause, trim=True, top_db=60.0, frame_length=2048, hop_length=512, keep=0, fade=0, level=False, max_gain=2.0,
               ceiling=0.0):
    """A padded batch of pieces glued into one waveform (C-ABI t2_join): wav (B, ld) float32 on the GPU (a strided view
    with a contiguous last dimension will do), n the B sample counts, 0 <= n[b] <= ld, pause the B counts of zeros behind each piece.
    Each row is cut to its span - trim_silence's rule with top_db, frame_length, hop_length, widened by `keep` samples at both ends;
    the whole row with trim=False or n[b] < frame_length; nothing for a row without an active frame -, scaled (level=True: towards
    the document's RMS, by at most max_gain either way; ceiling > 0: all gains lowered together until no sample exceeds it), faded
    over `fade` samples at both ends (half a Hann window, shortened for a span below 2 fade) and written behind its predecessor.
    Returns (y (total,) float32, total, plan): plan = dict(off int64, s0 int32, len int32, gain float32), (B,) device tensors.
    n and pause as host integers keep the call at ONE host read, the total; a tensor on the GPU costs one more, the sum that bounds
    y, and its values are checked by the kernel: an entry out of range raises ValueError after the launch, nothing being read or
    written for it.  Needs no model."""
    fn = "join_audio"
    _args.tensor_arg(fn, "wav", wav, 2, "(B, samples)")
    _args.on_gpu(fn, "wav", wav)
    B, ld, ldx = _args.wav_rows(fn, "wav", wav)
    trim, level = _args.flag_arg(fn, "trim", trim), _args.flag_arg(fn, "level", level)
    F = _args.int_arg(fn, "frame_length", frame_length, 2)
    if F % 2:
        raise ValueError(f"{fn}: frame_length must be even, got {F}")
    H = _args.int_arg(fn, "hop_length", hop_length, 1)
    keep, fade = _args.int_arg(fn, "keep", keep, 0), _args.int_arg(fn, "fade", fade, 0)
    top_db = _args.real_arg(fn, "top_db", top_db, nonneg=True)
    max_gain = _args.real_arg(fn, "max_gain", max_gain)
    if max_gain < 1:
        raise ValueError(f"{fn}: max_gain must be >= 1, got {max_gain!r}")
    ceiling = _args.real_arg(fn, "ceiling", ceiling, nonneg=True)
    dev = wav.device
    n32, n_sum = _args.counts32(fn, "n", n, B, dev, hi=ld)
    p32, p_sum = _args.counts32(fn, "pause", pause, B, dev)
    with torch.cuda.device(dev):
        if n_sum is None or p_sum is None:                    # (device counts: their sum is the one extra read)
            cap = max(int(n32.clamp(0, ld).sum(dtype=torch.int64) + p32.clamp(min=0).sum(dtype=torch.int64)), 0)
        else:
            cap = n_sum + p_sum
        w = cached(("fade", fade, dev), lambda: torch.from_numpy(fade_table(fade)).to(dev)) if fade > 0 else None
        lde = ld // H + 1
        energy = torch.empty(B, lde, dtype=torch.float64, device=dev) if trim else None
        stat = torch.empty(B, 2, dtype=torch.float64, device=dev)
        off = torch.empty(B, dtype=torch.int64, device=dev)
        s0, length = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
        gain = torch.empty(B, dtype=torch.float32, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        y = torch.empty(cap, dtype=torch.float32, device=dev)
        a = make("T2Join", x=wav if ld > 0 else None, ldx=ldx, n=n32, pause=p32, w=w, B=B, n_max=ld, trim=trim, F=F, H=H, keep=keep,
                 fade=fade, level=level, top_db=top_db, max_gain=max_gain, ceiling=ceiling, energy=energy, lde=lde, stat=stat,
                 off=off, s0=s0, len=length, gain=gain, total=total, y=y if cap > 0 else None, cap=cap)
        call("t2_join", a, stream())
        t = int(total.item())
    if t < 0:
        raise ValueError(f"{fn}: an n[b] outside 0 .. {ld} or a negative pause[b] (refused on the device; nothing was written)")
    return y[:t], t, dict(off=off, s0=s0, len=length, gain=gain)
