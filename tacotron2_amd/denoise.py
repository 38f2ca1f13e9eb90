"""Spectral subtraction of a vocoder's stationary bias spectrum from a padded batch: one call into
libtacotron2_amd.so (C-ABI t2_denoise) on the current stream.  analysis.denoise, analysis.stft_magnitudes and analysis.vocoder_bias
ARE this module's functions.  denoise and stft_magnitudes need no model, and their arguments are checked by _args before a pointer
reaches the kernel."""
from __future__ import annotations

import numpy as np
import torch

from . import _args
from ._lib import cached, call, make, stream

NFFT, HOP, NSTAT = 1024, 256, 4              # the header's enum T2_DENOISE_NFFT, T2_DENOISE_HOP, T2_DENOISE_NSTAT (tests/test_denoise_ref_host.py)
BINS = NFFT // 2 + 1
FLAG_SHORT = 1
STRENGTH_LIMITS = (0.0, 1.0)                 # what `say --denoise` offers; the kernel itself takes any finite strength >= 0
BIAS_FRAMES = 88                             # the all-zero mel NVIDIA's denoiser vocodes


def _tables(dev):
    """(win [1024], tw [768][2]) on dev: the periodic Hann window and cos, sin of 2 pi k / 1024, made in float64, rounded once."""
    def build():
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT, dtype=np.float64) / NFFT)
        a = 2.0 * np.pi * np.arange(3 * NFFT // 4, dtype=np.float64) / NFFT
        tw = np.stack([np.cos(a), np.sin(a)], axis=1)
        return torch.from_numpy(win.astype(np.float32)).to(dev), torch.from_numpy(tw.astype(np.float32)).contiguous().to(dev)
    return cached(("denoise", dev), build)


def frames(n_max: int) -> int:
    """The frames of a row of n_max samples: 1 + n_max // 256 (none for a row of at most 512 samples, which is copied)."""
    return 1 + n_max // HOP


def _run(fn: str, wav, n, bias, strength, write: bool, want_mag: bool):
    B, ld, ldx = _args.wav_rows(fn, "wav", wav)
    dev = wav.device
    if write:
        strength = _args.real_arg(fn, "strength", strength, nonneg=True)
        if not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (BINS,):
            raise ValueError(f"{fn}: bias must be a float32 ({BINS},) tensor")
    n32, n_sum = _args.counts32(fn, "n", n, B, dev, hi=ld)
    _args.on_gpu(fn, "wav", wav)
    if write:
        _args.on_device(fn, "bias", bias, dev)
    with torch.cuda.device(dev):
        win, tw = _tables(dev)
        y = torch.empty(B, max(ld, 1), dtype=torch.float32, device=dev) if write else None
        F = frames(ld)
        mag = torch.zeros(B, F, BINS, dtype=torch.float32, device=dev) if want_mag else None
        gated = torch.empty(B, dtype=torch.int32, device=dev)
        stat = torch.empty(B, NSTAT, dtype=torch.float64, device=dev)
        arg = make("T2Denoise", x=wav if ld > 0 else None, ldx=ldx, n=n32, B=B, n_max=ld, win=win, tw=tw,
                   bias=bias.contiguous() if write else None, strength=strength if write else 0.0, y=y, ldy=ld, mag=mag, ldm=BINS,
                   f_max=F, gated=gated, stat=stat)
        call("t2_denoise", arg, stream())
        if n_sum is None and bool((stat[:, 2] < 0).any()):             # (device counts: the kernel's refusal is the one extra read)
            raise ValueError(f"{fn}: an n[b] outside 0 .. {ld} (refused on the device; nothing was written for it)")
    return y, mag, gated, stat


def denoise(wav, n, bias, strength):
    """A padded batch with `strength * bias` taken off every frame's magnitudes (C-ABI t2_denoise): wav (B, ld) float32
    on the GPU (a strided view with a contiguous last dimension will do), n the B sample counts, 0 <= n[b] <= ld - host integers, or
    an integer tensor on the GPU, whose values the kernel checks: an entry out of range raises ValueError after the launch -, bias a
    float32 (513,) tensor on wav's device (vocoder_bias), strength a finite number >= 0.  Frames of 1024 samples
    every 256, periodic Hann, rows reflect-padded at their own length; per bin the magnitude m becomes max(m - strength * bias, 0),
    the phase stays; the frames are overlap-added and divided by the window's own overlap, so the output has all n[b] samples and
    bias = 0 gives the input back to rounding.  A row of at most 512 samples is copied (flag bit 0, short).  strength == 0 launches
    nothing and returns wav itself.  Returns (y, stats): y of wav's shape, zeros behind n[b]; stats a dict of (B,) device tensors:
    frames (int64), gated (int64: the bins set to zero), gated_fraction (float64: gated / (frames * 513), 0 without a frame),
    flags (int64)."""
    fn = "denoise"
    if not isinstance(strength, bool) and isinstance(strength, (int, float)) and strength == 0:
        B, ld, _ = _args.wav_rows(fn, "wav", wav)
        n32, _ = _args.counts32(fn, "n", n, B, wav.device, hi=ld)
        _args.on_gpu(fn, "wav", wav)
        fr = torch.where(n32 > NFFT // 2, 1 + n32 // HOP, 0).to(torch.int64)
        zero = torch.zeros(B, dtype=torch.int64, device=wav.device)
        return wav, dict(frames=fr, gated=zero, gated_fraction=zero.double(), flags=(n32 <= NFFT // 2).to(torch.int64))
    y, _, gated, stat = _run(fn, wav, n, bias, strength, True, False)
    fr, g = stat[:, 0].to(torch.int64), gated.to(torch.int64)
    return y[:, :wav.shape[1]], dict(frames=fr, gated=g, gated_fraction=g.double() / (fr.clamp(min=1) * BINS).double(), flags=stat[:, 2].to(torch.int64))


def stft_magnitudes(wav, n):
    """The magnitudes denoise gates, without the gate (t2_denoise's analysis mode: no inverse transform, no waveform): wav and n as
    denoise takes them.  Returns (B, 1 + ld // 256, 513) float32 on the device; frame t of row b is defined for t < 1 + n[b] // 256
    when n[b] > 512, and zero elsewhere."""
    _, mag, _, _ = _run("stft_magnitudes", wav, n, None, 0.0, False, True)
    return mag


def vocoder_bias(generator, frames: int = BIAS_FRAMES):
    """The bias spectrum of a HiFi-GAN generator (hifigan.Generator), (513,) float32 on its device: an all-zero log-mel of `frames`
    frames is vocoded (88: NVIDIA's denoiser) and the float64 mean of stft_magnitudes over the INTERIOR frames is taken - those
    whose 1024 samples lie inside the waveform; frame 0, which NVIDIA's denoiser uses, is half reflection and holds the generator's
    start-up transient.  Cached on the generator per `frames`: the second call returns the same tensor."""
    fn = "vocoder_bias"
    frames = _args.int_arg(fn, "frames", frames, 1, 4096)
    store = generator.__dict__.setdefault("_denoise_bias", {})
    if frames not in store:
        wav = generator(torch.zeros(generator.conv_pre.Ci, frames, dtype=torch.float32, device=generator.dev))[:, 0]
        n = int(wav.shape[1])
        lo, hi = NFFT // 2 // HOP, (n - NFFT // 2) // HOP              # HOP t - 512 >= 0 and HOP t + 512 <= n
        if hi < lo:
            raise ValueError(f"{fn}: {frames} mel frames give {n} samples, too few for one whole frame of {NFFT}")
        mag = stft_magnitudes(wav.contiguous(), [n])
        store[frames] = mag[0, lo:hi + 1].double().mean(dim=0).float()
    return store[frames]
