"""`main.py prosody-export`: measure a corpus on the GPU and write the control manifests the configs name - what the
reference's `preprocess` command and its split scripts do with a Praat-based extractor (preprocessing/preprocessing_split/
normalize.py), here with the meter that also measures what the model synthesises (ProsodyMeter, `test-correlation --measure`): a
requested control and its measured value are then on one scale.

Every utterance of dataset.train / val / test is loaded through TTSDataset.load_audio (the trimmed, padded signal its mel comes from),
decoded by a small thread pool, batched by length and measured by one ProsodyMeter.features call per batch.  The manifests are written
to the results directory under their own base names: the original columns, the raw FEATURES, then <feature>_speaker_norm[_clip] and
<feature>_dataset_norm[_clip] with x_norm = (x - median) / (3 std), medians and sample standard deviations (ddof 1) of the TRAIN rows
only - per speaker (`speaker_id`; one speaker when the column is absent) and over the whole set - and _clip its clip to [-1, 1].
prosody_norm.json holds the meter's settings, those statistics and the counts; prosody_dropped.csv (manifest|wav|reason) lists the
utterances left out of the written manifests: a feature undefined (no voiced frame, no measured frame, ...) or more than
T2_PROSODY_MAX_T frames."""
from __future__ import annotations

import csv
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional

import numpy as np

from ..prosody import FEATURES
from .common import sample_rate

SPLITS = ("train", "val", "test")
DROPPED_HEADER = ["manifest", "wav", "reason"]


class ProsodyExportError(ValueError):
    pass


def host_threads(default: int = 4, cap: int = 16) -> int:
    """Decode threads: OMP_NUM_THREADS when it is a positive integer, else `default`; never above `cap`, never from the CPU count."""
    try:
        v = int(os.environ.get("OMP_NUM_THREADS", ""))
    except ValueError:
        v = 0
    return max(1, min(cap, v if v > 0 else default))


def drop_reason(n_samples: int, feats: Optional[dict], max_frames: int, hop: int) -> Optional[str]:
    """Why an utterance leaves the written manifest, or None when it stays: feats = its ProsodyMeter.features dict (None when it was
    never measured: more than max_frames frames)."""
    if feats is None:
        return f"{1 + n_samples // hop} frames, above the limit of {max_frames}"
    missing = [f for f in FEATURES if feats.get(f) is None]
    if not missing:
        return None
    if n_samples == 0:
        return "empty waveform"
    if feats["n_frames"] == 0:
        return "shorter than one analysis span"
    if feats["n_voiced"] == 0:
        return "no voiced frame"
    if feats["n_measured"] == 0:
        return "no measured frame"
    return "undefined: " + ",".join(missing)


def norm_statistics(train, speaker_col: Optional[str]) -> dict:
    """{"dataset": {"n", "median", "std"}, "speakers": {id: the same}} of the FEATURES columns of the train frame (std: ddof 1).  A
    speaker with fewer than 2 rows or a feature whose std is 0 (or not finite) raises ProsodyExportError naming the speaker."""
    def one(df, who):
        if len(df) < 2:
            raise ProsodyExportError(f"prosody-export: {who} has {len(df)} measured train utterance(s): a standard deviation needs 2")
        med, std = df[FEATURES].median(), df[FEATURES].std(ddof=1)
        bad = [f for f in FEATURES if not (np.isfinite(std[f]) and std[f] > 0 and np.isfinite(med[f]))]
        if bad:
            raise ProsodyExportError(f"prosody-export: {who}: the train standard deviation of {', '.join(bad)} is 0 or undefined")
        return dict(n=int(len(df)), median={f: float(med[f]) for f in FEATURES}, std={f: float(std[f]) for f in FEATURES})
    stats = dict(dataset=one(train, "the train set"), speakers={})
    if speaker_col is None:
        stats["speakers"]["0"] = dict(stats["dataset"])
    else:
        for spk, g in train.groupby(speaker_col, sort=True):
            stats["speakers"][str(spk)] = one(g, f"speaker {spk}")
    return stats


def add_norm_columns(df, stats: dict, speaker_col: Optional[str]):
    """df with <feature>_speaker_norm, _speaker_norm_clip, _dataset_norm, _dataset_norm_clip appended (in this order, each group in
    the order of FEATURES).  A speaker without train statistics raises ProsodyExportError naming it."""
    if speaker_col is not None and speaker_col not in df.columns:
        raise ProsodyExportError(f"prosody-export: the train manifest has a {speaker_col} column, another manifest has none")
    df = df.copy()
    x = df[FEATURES].to_numpy(dtype=np.float64)
    keys = ["0"] * len(df) if speaker_col is None else [str(s) for s in df[speaker_col]]
    unknown = sorted(set(keys) - set(stats["speakers"]))
    if unknown:
        raise ProsodyExportError(f"prosody-export: speaker {', '.join(unknown)} has no train utterance: nothing to normalise by")
    med = np.array([[stats["speakers"][k]["median"][f] for f in FEATURES] for k in keys], np.float64).reshape(len(df), len(FEATURES))
    std = np.array([[stats["speakers"][k]["std"][f] for f in FEATURES] for k in keys], np.float64).reshape(len(df), len(FEATURES))
    spk = (x - med) / (3.0 * std)
    dmed = np.array([stats["dataset"]["median"][f] for f in FEATURES])
    dstd = np.array([stats["dataset"]["std"][f] for f in FEATURES])
    dat = (x - dmed) / (3.0 * dstd)
    for suffix, z in (("_speaker_norm", spk), ("_speaker_norm_clip", np.clip(spk, -1.0, 1.0)),
                      ("_dataset_norm", dat), ("_dataset_norm_clip", np.clip(dat, -1.0, 1.0))):
        for j, f in enumerate(FEATURES):
            df[f + suffix] = z[:, j]
    return df


def assemble(frames: Dict[str, "object"], feats: Dict[str, List[Optional[dict]]], reasons: Dict[str, List[Optional[str]]]):
    """(written frames with the raw FEATURES appended, dropped rows [manifest, wav, reason]) from the manifests as read, the feature
    dicts and the drop reasons per row."""
    import pandas as pd
    out, dropped = {}, []
    for name, df in frames.items():
        keep = [i for i, r in enumerate(reasons[name]) if r is None]
        dropped += [[name, str(df.wav[i]), r] for i, r in enumerate(reasons[name]) if r is not None]
        kept = df.iloc[keep].reset_index(drop=True)
        raw = pd.DataFrame({f: [float(feats[name][i][f]) for i in keep] for f in FEATURES}, columns=FEATURES)
        clash = [c for c in kept.columns if c in FEATURES or any(c == f + s for f in FEATURES for s in (
            "_speaker_norm", "_speaker_norm_clip", "_dataset_norm", "_dataset_norm_clip"))]
        out[name] = pd.concat([kept.drop(columns=clash), raw], axis=1)       # (a manifest exported before: its columns are replaced)
    return out, dropped


def measure_manifest(ds, meter, n_chars: List[int], batch_size: int, pool: ThreadPoolExecutor, max_frames: int):
    """(features per utterance - None for one that was not measured -, sample counts) of the dataset's utterances: ordered by text
    length (it predicts the duration), decoded a batch ahead by the pool, one meter.features call per batch."""
    import torch
    hop, dev = meter.settings["hop"], meter.device
    order = sorted(range(len(ds)), key=lambda i: (n_chars[i], i))
    batches = [order[k:k + batch_size] for k in range(0, len(order), batch_size)]
    feats: List[Optional[dict]] = [None] * len(ds)
    n_samples = [0] * len(ds)
    pending = [pool.submit(ds.load_audio, i) for i in batches[0]] if batches else []
    for k, idxs in enumerate(batches):
        wavs = [f.result() for f in pending]
        pending = [pool.submit(ds.load_audio, i) for i in batches[k + 1]] if k + 1 < len(batches) else []
        for i, w in zip(idxs, wavs):
            n_samples[i] = len(w)
        fit = [(i, w) for i, w in zip(idxs, wavs) if 1 + len(w) // hop <= max_frames]
        if not fit:
            continue
        ld = max(1, max(len(w) for _, w in fit))
        host = torch.zeros(len(fit), ld, pin_memory=True)
        hv = host.numpy()
        for r, (_, w) in enumerate(fit):
            hv[r, :len(w)] = w
        up = host.to(dev, non_blocking=True)
        got = meter.features([up[r, :len(w)] for r, (_, w) in enumerate(fit)], [n_chars[i] for i, _ in fit])
        for (i, _), g in zip(fit, got):
            feats[i] = g
    return feats, n_samples


def do_prosody_export(dataset_config: dict, extensions_config: dict, device: int, speech_dir: str, results_dir: Optional[str] = None,
                      smooth_pitch: bool = True, batch_size: int = 64, name: str = "corpus"):
    import datetime

    import pandas as pd
    import torch

    from .. import analysis
    from ..datasets.tts_dataset import TTSDataset
    from ..prosody import ProsodyMeter
    paths = {k: dataset_config[k] for k in SPLITS if dataset_config.get(k)}
    if "train" not in paths:
        raise ProsodyExportError("prosody-export: the config names no dataset.train: the statistics come from the train manifest")
    bases = [os.path.basename(p) for p in paths.values()]
    if len(set(bases)) != len(bases):
        raise ProsodyExportError(f"prosody-export: the manifests {bases} share a base name: they would overwrite one another")
    for k, p in paths.items():
        if not os.path.exists(p):
            raise ProsodyExportError(f"prosody-export: dataset.{k} = {p!r} does not exist")
    if results_dir is None:
        results_dir = f"results_{name}_prosody_export {datetime.datetime.now()}"
    os.makedirs(results_dir, exist_ok=True)
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    pre = {k: v for k, v in dataset_config.get("preprocessing", {}).items() if k not in ("cache", "cache_dir")}
    sr = sample_rate(pre)
    meter = ProsodyMeter(sr, dev, smooth=smooth_pitch)
    pool = ThreadPoolExecutor(max_workers=host_threads())
    frames, feats, reasons, n_utts = {}, {}, {}, 0
    t0 = time.perf_counter()
    try:
        for k, p in paths.items():
            df = pd.read_csv(p, delimiter="|", quoting=csv.QUOTE_NONE, engine="c")
            ds = TTSDataset(filenames=list(df.wav), texts=list(df.text), base_dir=speech_dir, device=dev, **pre)
            n_chars = [len(i) for i in ds.ids]
            fs, ns = measure_manifest(ds, meter, n_chars, batch_size, pool, analysis.PROSODY_MAX_T)
            frames[k], feats[k] = df, fs
            reasons[k] = [drop_reason(n, f, analysis.PROSODY_MAX_T, meter.settings["hop"]) for n, f in zip(ns, fs)]
            n_utts += len(df)
    finally:
        pool.shutdown(wait=True)
    torch.cuda.synchronize(dev)
    seconds = time.perf_counter() - t0
    raw, dropped = assemble(frames, feats, reasons)
    speaker_col = "speaker_id" if "speaker_id" in raw["train"].columns else None
    stats = norm_statistics(raw["train"], speaker_col)
    counts = {}
    for k, df in raw.items():
        out = add_norm_columns(df, stats, speaker_col)
        out.to_csv(os.path.join(results_dir, os.path.basename(paths[k])), sep="|", index=False, quoting=csv.QUOTE_NONE)
        counts[k] = dict(manifest=os.path.basename(paths[k]), rows=int(len(frames[k])), written=int(len(out)),
                         dropped=int(len(frames[k]) - len(out)))
        raw[k] = out
    with open(os.path.join(results_dir, "prosody_dropped.csv"), "w", newline="") as f:
        wr = csv.writer(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
        wr.writerow(DROPPED_HEADER)
        wr.writerows([[os.path.basename(paths[m]), w, r] for m, w, r in dropped])
    with open(os.path.join(results_dir, "prosody_norm.json"), "w") as f:
        json.dump(dict(meter=meter.describe(), features=FEATURES, formula="x_norm = (x - median) / (3 * std); _clip: clipped to [-1, 1]",
                       speaker_column=speaker_col, dataset=stats["dataset"], speakers=stats["speakers"], counts=counts), f, indent=1)
    ctl = extensions_config.get("controls", {})
    if ctl.get("active"):
        missing = [c for c in ctl.get("features", []) if c not in raw["train"].columns]
        if missing:
            raise ProsodyExportError("prosody-export: the written train manifest lacks the control columns of extensions.controls."
                                     f"features: {', '.join(missing)}")
    print(f"prosody-export: {n_utts} utterances in {seconds:.2f} s = {n_utts / max(seconds, 1e-9):.1f} utterances/s, "
          f"{len(dropped)} dropped -> {results_dir}")
    return results_dir
