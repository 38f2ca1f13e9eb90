"""What came out of a synthesis, measured on the GPU: pitch level and range, intensity, noisiness and speaking rate of a batch of
waveforms.  The YIN pitch tracker (engine.yin, C-ABI t2_yin) analyses frames on the mel grid - hop 256, frame t
centred on sample 256 t - and engine.prosody_stats (t2_prosody_stats) reduces every track to one row; this module only packs the
batch and names the fields.  No smoothing of the track, no jitter / shimmer, no parity with Praat's absolute values: the numbers
are for correlating with the requested controls (run/correlation.py)."""
from __future__ import annotations

import math
from typing import List, Sequence

import torch

from . import engine

MEASURES = ["pitch_mean_log", "pitch_range_log", "intensity_mean_db", "aperiodicity_mean", "rate"]


class ProsodyMeter:
    """measure() of a list of waveforms in one launch of each kernel.  The settings are engine.yin's (engine.YIN_DEFAULTS)."""

    def __init__(self, sample_rate: int = 22050, device=None, **yin_settings):
        unknown = set(yin_settings) - (set(engine.YIN_DEFAULTS) - {"sr"})
        if unknown:
            raise ValueError(f"ProsodyMeter: unknown YIN settings {sorted(unknown)}")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.settings = dict(engine.YIN_DEFAULTS, sr=int(sample_rate), **yin_settings)
        self.tau_min, self.tau_max = engine.yin_lags(self.settings["sr"], self.settings["fmin"], self.settings["fmax"])
        self.span = self.settings["W"] + self.tau_max

    def describe(self) -> dict:
        """The settings as they go into correlation.json."""
        return dict(self.settings, tau_min=self.tau_min, tau_max=self.tau_max)

    def measure(self, wavs: Sequence[torch.Tensor], n_chars: Sequence[int]) -> List[dict]:
        """One dict per waveform (1-D float32 tensors on the meter's device, any lengths, empty ones included): n_frames (valid
        analysis frames), n_voiced, and the MEASURES - pitch_mean_log = mean ln f0, pitch_range_log = ln p95 - ln p5,
        intensity_mean_db = mean 10 log10 of the frame power, aperiodicity_mean, all over the voiced frames, and rate = n_chars /
        seconds.  None where undefined: no voiced frame (the four track measures), an empty waveform (rate)."""
        if len(wavs) != len(n_chars):
            raise ValueError(f"measure: {len(wavs)} waveforms, {len(n_chars)} character counts")
        if not wavs:
            return []
        for w in wavs:
            if not torch.is_tensor(w) or w.dim() != 1 or w.dtype != torch.float32 or w.device != self.device:
                raise ValueError(f"measure: every waveform must be a 1-D float32 tensor on {self.device}")
        lens = [int(w.shape[0]) for w in wavs]
        n_max = max(lens)
        s = self.settings
        if 1 + n_max // s["hop"] > engine.PROSODY_MAX_T:
            raise ValueError(f"measure: a waveform of {n_max} samples has more than {engine.PROSODY_MAX_T} frames (T2_PROSODY_MAX_T)")
        batch = torch.zeros(len(wavs), max(n_max, 1), dtype=torch.float32, device=self.device)
        for k, w in enumerate(wavs):
            batch[k, :lens[k]] = w
        n = torch.tensor(lens, dtype=torch.int64, device=self.device)
        f0, aper, power = engine.yin(batch, n, n_max=n_max, **s)
        st = engine.prosody_stats(f0, aper, power, n, hop=s["hop"], span=self.span).cpu().tolist()
        out = []
        for k, row in enumerate(st):
            voiced = int(row[1]) > 0
            seconds = lens[k] / s["sr"]
            out.append(dict(
                n_frames=int(row[0]), n_voiced=int(row[1]),
                pitch_mean_log=row[2] if voiced else None,
                pitch_range_log=(math.log(row[4]) - math.log(row[3])) if voiced else None,
                intensity_mean_db=row[5] if voiced else None,
                aperiodicity_mean=row[6] if voiced else None,
                rate=(int(n_chars[k]) / seconds) if lens[k] > 0 else None))
        return out
