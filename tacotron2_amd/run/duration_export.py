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
DevicePrefetcher, `training.forward_attention` honoured, check_persistent_kernels() before anything is written."""
from __future__ import annotations

import csv
import datetime
import os
from typing import List, Optional

import numpy as np
import torch

from ..model.tts_model import TTSModel
from .common import model_kwargs, train_forward_attention_setting

MODES = ("monotonic", "argmax")
CSV_HEADER = ["wav", "n_chars", "n_frames", "focus_rate", "path_logp", "feasible", "argmax_agreement"]


def do_duration_export(dataset_config: dict, training_config: dict, model_config: dict, extensions_config: dict, device: int,
                       speech_dir: str, checkpoint: str, results_dir: Optional[str] = None, mode: str = "monotonic",
                       batch_size: int = 64) -> List[str]:
    import pandas as pd
    from ..datasets.tts_dataset import DevicePrefetcher, TTSDataLoader, TTSDataset
    from .train import _to_dev
    if mode not in MODES:
        raise ValueError(f"duration-export: mode must be one of {MODES}, got {mode!r}")
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    cfg = dict(dataset=dataset_config, training=training_config, model=model_config, extensions=extensions_config)
    kw = model_kwargs(cfg)
    model = TTSModel.load_from_checkpoint(checkpoint, device=dev, **kw)
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
    for split in ("train", "val"):
        df = pd.read_csv(dataset_config[split], delimiter="|", quoting=csv.QUOTE_NONE, engine="c")
        ds = TTSDataset(filenames=list(df.wav), texts=list(df.text), base_dir=speech_dir,
                        speaker_ids=list(df.speaker_id) if model.speaker_tokens else None,
                        features=df[ctl["features"]].values.tolist() if model.controls else None,
                        include_text=False, include_filename=True, device=dev, **pre)
        loader = TTSDataLoader(ds, batch_size=batch_size, shuffle=False, drop_last=False)

        def to_dev(b, d):
            out = _to_dev(b, d)
            out["filename"] = b[2]["filename"]
            return out
        for b in DevicePrefetcher(loader, to_dev, dev):
            args = {k: b[k] for k in ("speaker_id", "controls", "description_embeddings") if k in b}
            dur, stats, _ = model.durations(b["chars_idx"], b["chars_idx_len"], b["mel_spectrogram"], b["mel_spectrogram_len"],
                                            mode=mode, train_forward_attention=fwd_att, **args)
            dur, stats = dur.cpu().numpy(), stats.cpu().numpy()
            model.tacotron2._engine.check_persistent_kernels()     # (the copies above synchronised) never export a poisoned forward
            for d_b, s_b, nc, nf, fn in zip(dur, stats, b["chars_idx_len"].cpu().tolist(), b["mel_spectrogram_len"].cpu().tolist(),
                                            b["filename"]):
                path = os.path.join(results_dir, f"{fn.replace('/', '_')}.dur.npy")
                np.save(path, np.ascontiguousarray(d_b[:int(nc)], dtype=np.int32))
                written.append(path)
                rows.append([fn, int(nc), int(nf), f"{float(s_b[0]):.6f}", f"{float(s_b[1]):.6f}", int(s_b[2]), f"{float(s_b[3]):.6f}"])
    with open(os.path.join(results_dir, "durations.csv"), "w", newline="") as f:
        wr = csv.writer(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
        wr.writerow(CSV_HEADER)
        wr.writerows(rows)
    return written
