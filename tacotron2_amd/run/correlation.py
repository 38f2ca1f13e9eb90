"""The tables of `test-correlation --measure` and `measure-correlation`: how the measured prosody of the synthesised audio
(tacotron2_amd/prosody.py, `prosody.csv` of every override directory) follows the requested control vector.  Host only, float64
numpy, no scipy.

For control k the points are all (override, utterance) rows whose OTHER controls are 0 - the sweep of control k, the all-zero
override included; x is the requested value of control k and y a measure.  Per control against its own measure (FEATURE_MEASURES,
by the prefix of the config's feature name): n, n_dropped (rows without the measure: no voiced frame, no stop), Pearson r, Spearman
rho (average ranks on ties - x has 11 levels) and the least-squares slope; Pearson r also for the full control x measure matrix,
the leakage of one control into the others.  A degenerate column (fewer than 3 points or zero variance) gives None (JSON null)."""
from __future__ import annotations

import ast
import csv
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MEASURES = ["pitch_mean_log", "pitch_range_log", "intensity_mean_db", "aperiodicity_mean", "rate"]
FEATURE_MEASURES = [("pitch_mean", "pitch_mean_log"), ("pitch_range", "pitch_range_log"), ("intensity_mean", "intensity_mean_db"),
                    ("nhr", "aperiodicity_mean"), ("rate", "rate")]
PROSODY_HEADER = ["i", "wav", "n_chars", "seconds", "stopped", "n_frames", "n_voiced"] + MEASURES


def measure_of(feature: str) -> Optional[str]:
    """The measure a config feature name is compared with, by prefix (`pitch_mean_speaker_norm` -> pitch_mean_log); None for a
    feature that is not measured (jitter, shimmer, ...)."""
    for prefix, measure in FEATURE_MEASURES:
        if feature.startswith(prefix):
            return measure
    return None


def pearson(x, y) -> Optional[float]:
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if len(x) < 3 or not float(np.ptp(x)) > 0.0 or not float(np.ptp(y)) > 0.0:      # (a constant column, whatever its mean rounds to)
        return None
    dx, dy = x - x.mean(), y - y.mean()
    sxx, syy = float(dx @ dx), float(dy @ dy)
    if not (sxx > 0.0 and syy > 0.0):
        return None
    return float(min(1.0, max(-1.0, float(dx @ dy) / np.sqrt(sxx * syy))))


def average_ranks(v) -> np.ndarray:
    """Ranks 1 .. n of v, tied values sharing the average of their ranks."""
    v = np.asarray(v, dtype=np.float64)
    order = np.argsort(v, kind="stable")
    ranks = np.empty(len(v), dtype=np.float64)
    i = 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and v[order[j + 1]] == v[order[i]]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return ranks


def spearman(x, y) -> Optional[float]:
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if len(x) < 3:
        return None
    return pearson(average_ranks(x), average_ranks(y))


def slope(x, y) -> Optional[float]:
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if len(x) < 3:
        return None
    dx = x - x.mean()
    sxx = float(dx @ dx)
    if not sxx > 0.0 or not float(np.ptp(y)) > 0.0:
        return None
    return float(dx @ (y - y.mean())) / sxx


def parse_override_dir(name: str, n_features: int) -> Tuple[float, ...]:
    """`str(override)` of a results tree back to the tuple; anything else is a ValueError that names the directory."""
    try:
        v = ast.literal_eval(name)
    except (ValueError, SyntaxError):
        v = None
    if not isinstance(v, tuple) or len(v) != n_features or \
            not all(isinstance(c, (int, float)) and not isinstance(c, bool) for c in v):
        raise ValueError(f"{name!r} is not an override directory: expected a tuple of {n_features} numbers, e.g. "
                         f"{str(tuple([0.0] * n_features))!r}")
    return tuple(float(c) for c in v)


def write_prosody_csv(results_dir: str, rows: Sequence[dict]) -> None:
    """prosody.csv of one override directory (PROSODY_HEADER, `|`-separated); None is an empty field."""
    fmt = lambda v: "" if v is None else (f"{v:.6f}" if isinstance(v, float) else str(v))
    with open(os.path.join(results_dir, "prosody.csv"), "w", newline="") as f:
        wr = csv.writer(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
        wr.writerow(PROSODY_HEADER)
        for r in rows:
            wr.writerow([fmt(r.get(k)) for k in PROSODY_HEADER])


def read_prosody_csv(results_dir: str) -> List[dict]:
    """The MEASURES of every row of an override directory's prosody.csv; an empty field is None."""
    with open(os.path.join(results_dir, "prosody.csv"), newline="") as f:
        rd = csv.DictReader(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
        if rd.fieldnames != PROSODY_HEADER:
            raise ValueError(f"{results_dir}/prosody.csv: unexpected header {rd.fieldnames}")
        return [{m: (None if r[m] == "" else float(r[m])) for m in MEASURES} for r in rd]


def correlate_tree(base: str, features: Sequence[str], settings: dict) -> dict:
    """`main.py test-correlation --measure`, after the sweep: correlation.json from the prosody.csv that synthesize_manifest left in
    every override directory of `base` (the values as written there, six decimals)."""
    names = sorted(d for d in os.listdir(base) if os.path.isdir(os.path.join(base, d)))
    per_override = {parse_override_dir(d, len(features)): read_prosody_csv(os.path.join(base, d)) for d in names}
    return write_correlation(base, features, per_override, settings)


def correlation_tables(features: Sequence[str], per_override: Dict[Tuple[float, ...], List[dict]]) -> dict:
    """per_override: override tuple -> rows with the MEASURES (None = undefined).  The tables of the module docstring."""
    F = len(features)
    controls, leakage = [], {}
    for k, feat in enumerate(features):
        pts = [(ov[k], row) for ov, rows in per_override.items() if all(ov[j] == 0 for j in range(F) if j != k) for row in rows]
        col = {}
        for m in MEASURES:
            xy = [(x, row[m]) for x, row in pts if row.get(m) is not None]
            col[m] = ([p[0] for p in xy], [p[1] for p in xy])
        own = measure_of(feat)
        entry = {"feature": feat, "measure": own, "n": 0, "n_dropped": 0, "pearson": None, "spearman": None, "slope": None}
        if own is not None:
            x, y = col[own]
            entry.update(n=len(x), n_dropped=len(pts) - len(x), pearson=pearson(x, y), spearman=spearman(x, y), slope=slope(x, y))
        controls.append(entry)
        leakage[feat] = {m: pearson(*col[m]) for m in MEASURES}
    return {"features": list(features), "measures": MEASURES, "controls": controls, "pearson_matrix": leakage}


def write_correlation(base: str, features: Sequence[str], per_override, settings: dict) -> dict:
    """correlation.json in the base results directory; prints one line per control; returns the tables."""
    tables = correlation_tables(features, per_override)
    tables["yin"] = settings
    with open(os.path.join(base, "correlation.json"), "w") as f:
        json.dump(tables, f, indent=1)
    num = lambda v: "null" if v is None else f"{v:+.4f}"
    for c in tables["controls"]:
        if c["measure"] is None:
            print(f"{c['feature']}: not measured")
        else:
            print(f"{c['feature']} -> {c['measure']}: n {c['n']} (dropped {c['n_dropped']}), pearson {num(c['pearson'])}, "
                  f"spearman {num(c['spearman'])}, slope {num(c['slope'])}")
    return tables


def read_wav(path: str):
    """(float32 samples in [-1, 1), sample rate) of a PCM WAV written by vocoder.write_wav (16-bit mono), with the stdlib."""
    import wave
    with wave.open(path, "rb") as w:
        if w.getnchannels() != 1 or w.getsampwidth() != 2:
            raise ValueError(f"{path}: expected 16-bit mono PCM")
        sr, raw = w.getframerate(), w.readframes(w.getnframes())
    return np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0, sr


def do_measure_correlation(results_dir: str, features: Sequence[str], device: int = 0, batch_size: int = 8) -> dict:
    """`main.py measure-correlation`: the tables for a results tree that already exists.  Every sub-directory must be an override
    directory (parse_override_dir); its `<i>.wav` files are measured in numeric order and its prosody.csv is rewritten.  n_chars
    comes from an earlier prosody.csv of the directory when there is one (the WAVs do not carry the text), else it is 0 and `rate`
    measures nothing."""
    import torch
    from ..prosody import ProsodyMeter
    if not os.path.isdir(results_dir):
        raise ValueError(f"{results_dir!r} is not a directory")
    names = sorted(d for d in os.listdir(results_dir) if os.path.isdir(os.path.join(results_dir, d)))
    if not names:
        raise ValueError(f"{results_dir!r} holds no override directory")
    overrides = [parse_override_dir(d, len(features)) for d in names]          # every name is checked before any work
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    meter, per_override = None, {}
    for name, ov in zip(names, overrides):
        d = os.path.join(results_dir, name)
        idx = sorted(int(f[:-4]) for f in os.listdir(d) if f.endswith(".wav") and f[:-4].isdigit())
        chars = {}
        if os.path.exists(os.path.join(d, "prosody.csv")):
            with open(os.path.join(d, "prosody.csv"), newline="") as f:
                for r in csv.DictReader(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\"):
                    chars[int(r["i"])] = int(r["n_chars"])
        rows = []
        for b0 in range(0, len(idx), batch_size):
            sel = idx[b0:b0 + batch_size]
            wavs = []
            for i in sel:
                x, sr = read_wav(os.path.join(d, f"{i}.wav"))
                if meter is None:
                    meter = ProsodyMeter(sr, dev)
                elif sr != meter.settings["sr"]:
                    raise ValueError(f"{d}/{i}.wav: {sr} Hz, the tree started at {meter.settings['sr']} Hz")
                wavs.append(torch.from_numpy(x.copy()).to(dev))
            ms = meter.measure(wavs, [chars.get(i, 0) for i in sel])
            for i, w, m in zip(sel, wavs, ms):
                n = int(w.shape[0])
                if chars.get(i, 0) == 0:
                    m = dict(m, rate=None)
                rows.append(dict(m, i=i, wav=f"{i}.wav", n_chars=chars.get(i, 0), seconds=n / meter.settings["sr"],
                                 stopped=int(n > 0)))
        write_prosody_csv(d, rows)
        per_override[ov] = rows
    settings = meter.describe() if meter is not None else {}
    return write_correlation(results_dir, features, per_override, settings)
