"""do_duration_export: per-character durations of every utterance of the train and validation manifests, from the alignments of
a teacher-forced, eval-mode forward - the teacher export a duration-based model (FastSpeech) trains on, the sibling of
run/train_mel_export.py (no reference counterpart).

Per utterance `<results>/<wav name with / -> _>.dur.npy`: an int32 array (N,), N = the encoded text length (end token included),
mel frames per character, summing to the utterance's mel length.  One `durations.csv`, `|`-separated, with a header row:
wav|n_chars|n_frames|focus_rate|path_logp|feasible|argmax_agreement - the alignment-health figures such pipelines filter on.
mode "monotonic" (default): the best monotonic path through the log-alignments (Glow-TTS's alignment search, a HIP kernel:
include/tacotron2_amd.h, t2_align_durations); "argmax": each decoder step's peak.  An utterance with fewer decoder steps than
characters has no monotonic path: its file holds the argmax counts and its row says feasible = 0.

As in train_mel_export: `|`-separated manifests with QUOTE_NONE, no mel cache, batches of 64 in manifest order through
DevicePrefetcher, `training.forward_attention` honoured, check_persistent_kernels() before anything is written.

variances=True (`--variances`) adds the two further targets of FastSpeech 2 / FastPitch on the same character grid (DESIGN 5.15,
t2_char_variance): `<name>.pitch.npy` and `<name>.energy.npy`, float32 (N,), beside every `.dur.npy`, and with frame_level also
`<name>.pitch_frames.npy` and `<name>.energy_frames.npy`, float32 (F,).  The pitch is the ProsodyMeter's track (Viterbi-smoothed
unless smooth_pitch is False) of the signal the mel came from, in ln Hz (pitch_domain "log") or Hz: per character the mean over its
voiced frames, 0 for a character without one, or with interpolate_pitch the mean over all its frames of the track interpolated
across the unvoiced stretches.  The energy is the mean over the character's frames of the L2 norm of the mel magnitudes.  The
waveform comes with the item: the dataset is built with include_audio=True, an opt-in keyword of TTSDataset that hands
load_audio(i) along - one decode per utterance, in the loader thread, not a second one.  Also written: `variances.csv`
(wav|n_chars|n_frames|n_voiced|chars_unvoiced|pitch_mean|pitch_std|energy_mean|energy_std over the utterance's frames, empty where
undefined), `variance_stats.json` (the meter's settings, the options, and count, mean, standard deviation, minimum and maximum of
pitch and energy at character and at frame level over the TRAIN rows only: what a student normalises with) and
`variances_dropped.csv` (wav|reason: an utterance of more than T2_VAR_MAX_T frames gets its durations and no variances).  The
`.dur.npy` files and durations.csv are byte-identical with and without the option: the durations come from the same call."""
from __future__ import annotations

import csv
import datetime
import json
import math
import os
from typing import List, Optional

import numpy as np
import torch

from ..model.tts_model import TTSModel
from .common import model_kwargs, train_forward_attention_setting, use_ema_setting

MODES = ("monotonic", "argmax")
CSV_HEADER = ["wav", "n_chars", "n_frames", "focus_rate", "path_logp", "feasible", "argmax_agreement"]
PITCH_DOMAINS = ("log", "hz")
VAR_HEADER = ["wav", "n_chars", "n_frames", "n_voiced", "chars_unvoiced", "pitch_mean", "pitch_std", "energy_mean", "energy_std"]
VAR_DROPPED_HEADER = ["wav", "reason"]


def mean_std(n: float, s: float, s2: float):
    """("mean", "std") of n values with sum s and sum of squares s2 as text, empty where undefined (n = 0)."""
    if n <= 0:
        return "", ""
    m = s / n
    return f"{m:.6f}", f"{math.sqrt(max(s2 / n - m * m, 0.0)):.6f}"


def moments(x):
    """The pooled() row (count, sum, sum of squares, minimum, maximum) of a float32 array, in float64."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return [0, 0.0, 0.0, 0.0, 0.0]
    return [int(x.size), math.fsum(x), math.fsum(x * x), float(x.min()), float(x.max())]


class _Variances:
    """The --variances side of the export: measures each batch behind its durations, writes the per-utterance files and keeps the
    rows of variances.csv and the moments of the train rows."""

    def __init__(self, dev, sample_rate: int, hop: int, results_dir: str, pitch_domain: str, interpolate: bool, frame_level: bool,
                 smooth_pitch: bool):
        from ..prosody import ProsodyMeter
        from ..variance import VAR_MAX_T
        self.meter = ProsodyMeter(sample_rate, dev, smooth=smooth_pitch)
        if self.meter.settings["hop"] != hop:
            raise ValueError(f"duration-export: the meter's hop {self.meter.settings['hop']} is not the mel's {hop}")
        self.dev, self.dir, self.max_frames = dev, results_dir, VAR_MAX_T
        self.log_pitch, self.interpolate, self.frame_level = pitch_domain == "log", bool(interpolate), bool(frame_level)
        self.rows, self.dropped, self.written = [], [], []
        self.moments = {k: [] for k in ("pitch_char", "pitch_frame", "energy_char", "energy_frame")}
        self.counts = {}

    def batch(self, split: str, b: dict, dur):
        from ..prosody import char_variances
        names, audio = b["filename"], b["audio"]
        n_chars, n_frames = b["chars_idx_len"].cpu().tolist(), b["mel_spectrogram_len"].cpu().tolist()
        c = self.counts.setdefault(split, dict(utterances=0, measured=0, dropped=0))
        c["utterances"] += len(names)
        fit = [k for k, f in enumerate(n_frames) if int(f) <= self.max_frames]
        for k, f in enumerate(n_frames):
            if int(f) > self.max_frames:
                self.dropped.append([names[k], f"{int(f)} frames, above the limit of {self.max_frames}"])
        c["dropped"] += len(names) - len(fit)
        c["measured"] += len(fit)
        if not fit:
            return
        ld = max(1, max(len(audio[k]) for k in fit))
        host = torch.zeros(len(fit), ld, pin_memory=True)
        hv = host.numpy()
        for r, k in enumerate(fit):
            hv[r, :len(audio[k])] = audio[k]
        up = host.to(self.dev, non_blocking=True)
        wavs = [up[r, :len(audio[k])] for r, k in enumerate(fit)]
        whole = len(fit) == len(names)
        at = None if whole else torch.tensor(fit, device=self.dev)
        pick = (lambda x: x) if whole else (lambda x: x.index_select(0, at))
        flen = pick(b["mel_spectrogram_len"])
        T = int(flen.max())
        out, stats = char_variances(self.meter, wavs, pick(b["mel_spectrogram"])[:, :T], flen, pick(dur), pick(b["chars_idx_len"]),
                                    log_pitch=self.log_pitch, interpolate=self.interpolate, return_frames=True)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        stats = stats.cpu().numpy()
        dur_h = pick(dur).cpu().numpy()
        for r, k in enumerate(fit):
            N, F, st = int(n_chars[k]), int(n_frames[k]), stats[r]
            base = os.path.join(self.dir, names[k].replace("/", "_"))
            pitch, energy = out["pitch"][r, :N], out["energy"][r, :N]
            files = [(".pitch.npy", pitch), (".energy.npy", energy)]
            if self.frame_level:
                files += [(".pitch_frames.npy", out["pitch_frames"][r, :F]), (".energy_frames.npy", out["energy_frames"][r, :F])]
            for ext, x in files:
                np.save(base + ext, np.ascontiguousarray(x, dtype=np.float32))
                self.written.append(base + ext)
            nv = int(st[1])
            # the utterance's pitch figures are over the frames the option selects: the voiced ones, or with interpolation all of q
            pn, ps, ps2 = (st[0] if nv else 0, st[4], st[5]) if self.interpolate else (nv, st[2], st[3])
            self.rows.append([names[k], N, F, nv, int(st[9]), *mean_std(pn, ps, ps2), *mean_std(st[0], st[6], st[7])])
            if split != "train":
                continue
            # pitch is defined for a character with a voiced frame - interpolated: with a frame, in an utterance with a voiced one
            has_pitch = (dur_h[r, :N] > 0) & (nv > 0) if self.interpolate else out["voiced"][r, :N] > 0
            qf = out["pitch_frames"][r, :F]
            self.moments["pitch_char"].append(moments(pitch[has_pitch]))
            self.moments["energy_char"].append(moments(energy[dur_h[r, :N] > 0]))
            fsel = qf if self.interpolate else qf[qf != 0]
            self.moments["pitch_frame"].append([int(pn), float(ps), float(ps2), float(fsel.min()) if pn else 0.0,
                                                float(fsel.max()) if pn else 0.0])
            ef = out["energy_frames"][r, :F]
            self.moments["energy_frame"].append([F, float(st[6]), float(st[7]), float(ef.min()) if F else 0.0,
                                                 float(ef.max()) if F else 0.0])

    def finish(self, options: dict):
        from ..variance import pooled
        for name, header, rows in (("variances.csv", VAR_HEADER, self.rows), ("variances_dropped.csv", VAR_DROPPED_HEADER, self.dropped)):
            with open(os.path.join(self.dir, name), "w", newline="") as f:
                wr = csv.writer(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
                wr.writerow(header)
                wr.writerows(rows)
        m = self.moments
        with open(os.path.join(self.dir, "variance_stats.json"), "w") as f:
            json.dump(dict(meter=self.meter.describe(), options=options, statistics_from="train", counts=self.counts,
                           pitch=dict(char=pooled(m["pitch_char"]), frame=pooled(m["pitch_frame"])),
                           energy=dict(char=pooled(m["energy_char"]), frame=pooled(m["energy_frame"]))), f, indent=1)


def do_duration_export(dataset_config: dict, training_config: dict, model_config: dict, extensions_config: dict, device: int,
                       speech_dir: str, checkpoint: str, results_dir: Optional[str] = None, mode: str = "monotonic",
                       batch_size: int = 64, variances: bool = False, pitch_domain: str = "log", interpolate_pitch: bool = False,
                       frame_level: bool = False, smooth_pitch: bool = True) -> List[str]:
    import pandas as pd
    from ..datasets.tts_dataset import DevicePrefetcher, TTSDataLoader, TTSDataset
    from .train import _to_dev
    if mode not in MODES:
        raise ValueError(f"duration-export: mode must be one of {MODES}, got {mode!r}")
    if pitch_domain not in PITCH_DOMAINS:
        raise ValueError(f"duration-export: pitch_domain must be one of {PITCH_DOMAINS}, got {pitch_domain!r}")
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    cfg = dict(dataset=dataset_config, training=training_config, model=model_config, extensions=extensions_config)
    kw = model_kwargs(cfg)
    model = TTSModel.load_from_checkpoint(checkpoint, device=dev, use_ema=use_ema_setting(model_config), **kw)
    model.eval()
    # a model trained under forward attention (training.forward_attention) is aligned by the recursion: its alignments need it
    fwd_att = train_forward_attention_setting(training_config)
    if results_dir is None:
        results_dir = f"results_{training_config['name']}_duration_export {datetime.datetime.now()}"
    os.makedirs(results_dir, exist_ok=True)
    pre = dict(dataset_config["preprocessing"])
    pre["cache"] = False
    ctl = extensions_config.get("controls", {"active": False})
    written: List[str] = []
    rows = []
    var = None
    for split in ("train", "val"):
        df = pd.read_csv(dataset_config[split], delimiter="|", quoting=csv.QUOTE_NONE, engine="c")
        ds = TTSDataset(filenames=list(df.wav), texts=list(df.text), base_dir=speech_dir,
                        speaker_ids=list(df.speaker_id) if model.speaker_tokens else None,
                        features=df[ctl["features"]].values.tolist() if model.controls else None,
                        include_text=False, include_filename=True, device=dev, **(dict(pre, include_audio=True) if variances else pre))
        if variances and var is None:
            var = _Variances(dev, ds.sample_rate, ds.melspectrogram.hop, results_dir, pitch_domain, interpolate_pitch, frame_level,
                             smooth_pitch)
        loader = TTSDataLoader(ds, batch_size=batch_size, shuffle=False, drop_last=False)

        def to_dev(b, d):
            out = _to_dev(b, d)
            out["filename"] = b[2]["filename"]
            if "audio" in b[2]:
                out["audio"] = b[2]["audio"]
            return out
        for b in DevicePrefetcher(loader, to_dev, dev):
            args = {k: b[k] for k in ("speaker_id", "controls", "description_embeddings") if k in b}
            dur, stats, _ = model.durations(b["chars_idx"], b["chars_idx_len"], b["mel_spectrogram"], b["mel_spectrogram_len"],
                                            mode=mode, train_forward_attention=fwd_att, **args)
            dur_dev = dur
            dur, stats = dur.cpu().numpy(), stats.cpu().numpy()
            model.tacotron2._engine.check_persistent_kernels()     # (the copies above synchronised) never export a poisoned forward
            for d_b, s_b, nc, nf, fn in zip(dur, stats, b["chars_idx_len"].cpu().tolist(), b["mel_spectrogram_len"].cpu().tolist(),
                                            b["filename"]):
                path = os.path.join(results_dir, f"{fn.replace('/', '_')}.dur.npy")
                np.save(path, np.ascontiguousarray(d_b[:int(nc)], dtype=np.int32))
                written.append(path)
                rows.append([fn, int(nc), int(nf), f"{float(s_b[0]):.6f}", f"{float(s_b[1]):.6f}", int(s_b[2]), f"{float(s_b[3]):.6f}"])
            if var is not None:
                var.batch(split, b, dur_dev)
    with open(os.path.join(results_dir, "durations.csv"), "w", newline="") as f:
        wr = csv.writer(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
        wr.writerow(CSV_HEADER)
        wr.writerows(rows)
    if var is not None:
        var.finish(dict(mode=mode, pitch_domain=pitch_domain, interpolate_pitch=bool(interpolate_pitch), frame_level=bool(frame_level),
                        smooth_pitch=bool(smooth_pitch)))
        written += var.written
    return written
