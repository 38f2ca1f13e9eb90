"""What came out of a synthesis, measured on the GPU: pitch level and range, intensity, noisiness and speaking rate of a batch of
waveforms.  The YIN pitch tracker (analysis.yin, C-ABI t2_yin) analyses frames on the mel grid - hop 256, frame t
centred on sample 256 t - and analysis.prosody_stats (t2_prosody_stats) reduces every track to one row; this module only packs the
batch and names the fields.  No parity with Praat's absolute values: the numbers are for correlating with the requested controls
(run/correlation.py).  ProsodyMeter.features adds jitter, shimmer and a noise-to-harmonics ratio by cycle matching
(analysis.voice_quality) and returns the reference's FEATURES_ALL columns: what `main.py prosody-export` writes.  ProsodyMeter(smooth=True) decodes the track with analysis.pitch_viterbi, and
f0_scores compares the tracks of two batches along a warping path (analysis.f0_path_stats): what `test --score --f0` reports."""
from __future__ import annotations

import math
from typing import List, Sequence

import torch

from . import analysis

MEASURES = ["pitch_mean_log", "pitch_range_log", "intensity_mean_db", "aperiodicity_mean", "rate"]
# the reference's feature columns (preprocessing/preprocessing_split/normalize.py: FEATURES_ALL), in its order
FEATURES = ["duration", "duration_vcd", "pitch_mean", "pitch_5", "pitch_95", "pitch_range", "pitch_mean_log", "pitch_5_log",
            "pitch_95_log", "pitch_range_log", "intensity_mean", "intensity_mean_vcd", "jitter", "shimmer", "nhr", "nhr_vcd", "rate",
            "rate_vcd"]


class ProsodyMeter:
    """measure() of a list of waveforms in one launch of each kernel.  The settings are analysis.yin's (analysis.YIN_DEFAULTS).
    smooth=True decodes the track with analysis.pitch_viterbi before the statistics: further settings are then
    analysis.VITERBI_DEFAULTS' (w, max_jump, u - default: this meter's vthr -, c_sw)."""

    def __init__(self, sample_rate: int = 22050, device=None, smooth: bool = False, **settings):
        yin_keys, vit_keys = set(analysis.YIN_DEFAULTS) - {"sr"}, set(analysis.VITERBI_DEFAULTS)
        unknown = set(settings) - yin_keys - (vit_keys if smooth else set())
        if unknown:
            raise ValueError(f"ProsodyMeter: unknown YIN settings {sorted(unknown)}")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.smooth = bool(smooth)
        self.settings = dict(analysis.YIN_DEFAULTS, sr=int(sample_rate), **{k: v for k, v in settings.items() if k in yin_keys})
        self.viterbi = None
        if self.smooth:
            self.viterbi = dict(analysis.VITERBI_DEFAULTS, u=self.settings["vthr"])
            self.viterbi.update({k: v for k, v in settings.items() if k in vit_keys})
        self.tau_min, self.tau_max = analysis.yin_lags(self.settings["sr"], self.settings["fmin"], self.settings["fmax"])
        self.span = self.settings["W"] + self.tau_max

    def describe(self) -> dict:
        """The settings as they go into correlation.json; with smooth also `smooth` and the Viterbi settings."""
        d = dict(self.settings, tau_min=self.tau_min, tau_max=self.tau_max)
        if self.smooth:
            d.update(smooth=True, **self.viterbi)
        return d

    def _pack(self, fn: str, wavs):
        for w in wavs:
            if not torch.is_tensor(w) or w.dim() != 1 or w.dtype != torch.float32 or w.device != self.device:
                raise ValueError(f"{fn}: every waveform must be a 1-D float32 tensor on {self.device}")
        lens = [int(w.shape[0]) for w in wavs]
        n_max = max(lens)
        s = self.settings
        if 1 + n_max // s["hop"] > analysis.PROSODY_MAX_T:
            raise ValueError(f"{fn}: a waveform of {n_max} samples has more than {analysis.PROSODY_MAX_T} frames (T2_PROSODY_MAX_T)")
        batch = torch.zeros(len(wavs), max(n_max, 1), dtype=torch.float32, device=self.device)
        for k, w in enumerate(wavs):
            batch[k, :lens[k]] = w
        return batch, lens, n_max, torch.tensor(lens, dtype=torch.int64, device=self.device)

    def _track(self, batch, n, n_max):
        """(f0, aper, power) of a packed batch: yin's own pick, or with smooth the Viterbi decode of its cmnd."""
        s = self.settings
        if not self.smooth:
            return analysis.yin(batch, n, n_max=n_max, **s)
        _, _, power, cmnd = analysis.yin(batch, n, n_max=n_max, return_cmnd=True, **s)
        f0, aper, _, _ = analysis.pitch_viterbi(cmnd, power, n, sr=s["sr"], hop=s["hop"], fmin=s["fmin"], fmax=s["fmax"],
                                              power_floor=s["power_floor"], **self.viterbi)
        return f0, aper, power

    def tracks(self, wavs: Sequence[torch.Tensor]):
        """(f0 (B, T) Hz, n (B,) int64 sample counts) of a batch of waveforms, padded to the longest: the track measure() reduces
        (0 = unvoiced or invalid frame; frame t is centred on sample t * hop)."""
        if not wavs:
            raise ValueError("tracks: no waveform")
        batch, _, n_max, n = self._pack("tracks", wavs)
        return self._track(batch, n, n_max)[0], n

    def measure(self, wavs: Sequence[torch.Tensor], n_chars: Sequence[int]) -> List[dict]:
        """One dict per waveform (1-D float32 tensors on the meter's device, any lengths, empty ones included): n_frames (valid
        analysis frames), n_voiced, and the MEASURES - pitch_mean_log = mean ln f0, pitch_range_log = ln p95 - ln p5,
        intensity_mean_db = mean 10 log10 of the frame power, aperiodicity_mean, all over the voiced frames, and rate = n_chars /
        seconds.  None where undefined: no voiced frame (the four track measures), an empty waveform (rate)."""
        if len(wavs) != len(n_chars):
            raise ValueError(f"measure: {len(wavs)} waveforms, {len(n_chars)} character counts")
        if not wavs:
            return []
        batch, lens, n_max, n = self._pack("measure", wavs)
        s = self.settings
        f0, aper, power = self._track(batch, n, n_max)
        st = analysis.prosody_stats(f0, aper, power, n, hop=s["hop"], span=self.span).cpu().tolist()
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

    def features(self, wavs: Sequence[torch.Tensor], n_chars: Sequence[int]) -> List[dict]:
        """One dict per waveform (as measure() takes them) with n_frames, n_voiced, n_measured and the FEATURES, from the meter's own
        track (smoothed or not, as the meter was built): duration = samples / sr and duration_vcd = n_voiced hop / sr in seconds;
        pitch_mean (Hz, over the voiced frames), pitch_5, pitch_95 (nearest-rank percentiles of the track), pitch_range = pitch_95 -
        pitch_5, and their _log twins - pitch_mean_log = mean ln f0 and pitch_range_log = ln p95 - ln p5, exactly measure()'s,
        pitch_5_log = ln p5, pitch_95_log = ln p95; intensity_mean = mean 10 log10 of the frame power over the loud frames (power >
        power_floor), intensity_mean_vcd over the voiced frames (measure()'s intensity_mean_db); jitter, shimmer, nhr = means over
        the measured frames (analysis.voice_quality); rate = n_chars / duration, rate_vcd = n_chars / duration_vcd.  nhr_vcd is a COPY
        of nhr: every period-based measure here is taken on voiced frames by construction, there is no other kind of nhr.  None where
        undefined: no voiced frame (pitch_*, intensity_mean_vcd, rate_vcd), no measured frame (jitter, shimmer, nhr, nhr_vcd), no loud
        frame (intensity_mean), an empty waveform (rate)."""
        if len(wavs) != len(n_chars):
            raise ValueError(f"features: {len(wavs)} waveforms, {len(n_chars)} character counts")
        if not wavs:
            return []
        batch, lens, n_max, n = self._pack("features", wavs)
        s = self.settings
        f0, aper, power = self._track(batch, n, n_max)
        st = analysis.prosody_stats(f0, aper, power, n, hop=s["hop"], span=self.span)
        vq = analysis.voice_quality(batch, n, f0, sr=s["sr"], hop=s["hop"], W=s["W"], fmin=s["fmin"], fmax=s["fmax"], n_max=n_max)
        cs = analysis.corpus_stats(f0, power, *vq, n, hop=s["hop"], span=self.span, power_floor=s["power_floor"])
        st, cs = st.cpu().tolist(), cs.cpu().tolist()
        out = []
        for k, (row, c) in enumerate(zip(st, cs)):
            n_voiced, n_measured, n_loud = int(row[1]), int(c[2]), int(c[3])
            voiced, measured = n_voiced > 0, n_measured > 0
            duration, duration_vcd = lens[k] / s["sr"], n_voiced * s["hop"] / s["sr"]
            nhr = c[7] if measured else None
            out.append(dict(
                n_frames=int(row[0]), n_voiced=n_voiced, n_measured=n_measured,
                duration=duration, duration_vcd=duration_vcd,
                pitch_mean=c[4] if voiced else None, pitch_5=row[3] if voiced else None, pitch_95=row[4] if voiced else None,
                pitch_range=(row[4] - row[3]) if voiced else None,
                pitch_mean_log=row[2] if voiced else None, pitch_5_log=math.log(row[3]) if voiced else None,
                pitch_95_log=math.log(row[4]) if voiced else None,
                pitch_range_log=(math.log(row[4]) - math.log(row[3])) if voiced else None,
                intensity_mean=c[9] if n_loud > 0 else None, intensity_mean_vcd=row[5] if voiced else None,
                jitter=c[5] if measured else None, shimmer=c[6] if measured else None, nhr=nhr, nhr_vcd=nhr,
                rate=(int(n_chars[k]) / duration) if lens[k] > 0 else None,
                rate_vcd=(int(n_chars[k]) / duration_vcd) if voiced else None))
        return out


def char_variances(meter: ProsodyMeter, wavs: Sequence[torch.Tensor], mel, mel_len, dur, chars_len, log_pitch: bool = True,
                   interpolate: bool = False, return_frames: bool = False):
    """Per-character pitch and energy targets of a batch (analysis.char_variance) from the meter's own track: wavs[k] the
    signal the log-mel mel[k] (B, T, M) came from (TTSDataset.load_audio), mel_len (B,) its frames, dur (B, L) int32 the durations
    of Engine.durations and chars_len (B,) the text lengths.  The track's frame t is centred on sample hop * t, as the mel frame is:
    the track of utterance k must have 1 + len(wavs[k]) // hop == mel_len[k] frames, anything else is a ValueError.  Returns
    analysis.char_variance's (out, stats)."""
    if not torch.is_tensor(mel) or mel.dim() != 3 or len(wavs) != mel.shape[0]:
        raise ValueError(f"char_variances: {len(wavs)} waveforms, mel must be a ({len(wavs)}, T, M) tensor")
    f0, n = meter.tracks(wavs)
    hop = meter.settings["hop"]
    frames = [1 + int(w.shape[0]) // hop for w in wavs]
    want = [int(v) for v in mel_len.reshape(-1).tolist()]
    if frames != want:
        k = next(i for i, (x, y) in enumerate(zip(frames, want)) if x != y) if len(frames) == len(want) else 0
        raise ValueError(f"char_variances: the track of utterance {k} has {frames[k]} frames (1 + {int(wavs[k].shape[0])} // {hop}), "
                         f"its mel {want[k] if k < len(want) else 'none'}: the waveforms are not the signals the mels came from")
    T = f0.shape[1]
    if mel.shape[1] < T:
        raise ValueError(f"char_variances: mel has {mel.shape[1]} frames, the longest utterance {T}")
    return analysis.char_variance(dur, chars_len, mel_len.reshape(-1).to(f0.device), f0, mel[:, :T], log_pitch=log_pitch,
                                  interpolate=interpolate, return_frames=return_frames)


F0_MEASURES = ["f0_rmse_cents", "f0_bias_cents", "f0_corr", "vuv_error"]


def f0_scores(meter: ProsodyMeter, syn_wavs: Sequence[torch.Tensor], ref_wavs: Sequence[torch.Tensor], path, path_len) -> List[dict]:
    """One dict per pair (analysis.f0_figures: n_pairs, n_voiced_both and the F0_MEASURES, None where undefined): the meter's tracks of
    syn_wavs[k] and ref_wavs[k] compared along the first path_len[k] cells (i = frame of the synthesis, j = frame of the recording)
    of path (B, P, 2) int32 - Tacotron2.score_decode(return_path=True) - whose frames lie on the meter's hop."""
    if len(syn_wavs) != len(ref_wavs):
        raise ValueError(f"f0_scores: {len(syn_wavs)} synthesised waveforms, {len(ref_wavs)} recordings")
    if not syn_wavs:
        return []
    f0_a, n_a = meter.tracks(syn_wavs)
    f0_b, n_b = meter.tracks(ref_wavs)
    st = analysis.f0_path_stats(path, path_len, f0_a, n_a, f0_b, n_b, hop=meter.settings["hop"], span=meter.span)
    return [analysis.f0_figures(row) for row in st.cpu().tolist()]
