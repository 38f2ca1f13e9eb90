"""Cost of the BS.1770 loudness measurement and normalisation (GPU box):

    python tools/time_loudness.py [--reps 7] [--warmup 2] [--json profiles/loudness_timing.json]

The two batches of tools/time_psola.py at 22 050 Hz - 64 rows of 4.6 s (the texts of one `say` call) and one row of 10 s (a joined
document) - of harmonic tones with a drifting pitch plus noise.  Timed between two device events, in ONE process and ALTERNATED
repetition by repetition, so that a drift of the machine meets all of them alike:
  measure      analysis.loudness (the allocations, the upload of the counts, three launches: filter, peaks, gates);
  normalize    analysis.normalize_loudness at -23 LUFS (the same and the scaling launch, one more buffer);
  resample_4x  analysis.resample to four times the rate, which WRITES the signal whose maximum the peak launch only keeps;
  join         analysis.join_audio of the same rows (trim, level, fade): the step that stands in front of it in a document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import tacotron2_amd  # noqa: F401
    from tacotron2_amd import analysis
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    sr = 22050
    rng = np.random.default_rng(1234)

    def voice(n):
        t = np.arange(n) / sr
        f0 = rng.uniform(90, 250) * (1.0 + 0.1 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0) * t))
        ph = 2 * np.pi * np.cumsum(f0) / sr
        return (0.3 * sum(np.sin(k * ph) / k for k in range(1, 6)) + 0.003 * rng.standard_normal(n)).astype(np.float32)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms):
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                    ms_all=[round(v, 4) for v in ms])

    out = dict(gpu=torch.cuda.get_device_name(0), sample_rate=sr, target_lufs=-23.0, reps=a.reps, warmup=a.warmup,
               method="device events; the four alternated repetition by repetition in one process", batches={})
    for name, B, seconds in (("64x4.6s", 64, 4.6), ("1x10s", 1, 10.0)):
        n = [int(round(seconds * sr))] * B
        x = torch.from_numpy(np.stack([voice(n[0]) for _ in range(B)])).to(dev)
        y, st = analysis.normalize_loudness(x, n, sr)
        again = analysis.loudness(y, n, sr)
        limited = int((st["flags"] & 4).ne(0).sum())
        assert bool(torch.isfinite(y).all()) and (limited or float((again["lufs"] + 23.0).abs().max()) < 1e-3)
        fns = dict(measure=lambda: analysis.loudness(x, n, sr), normalize=lambda: analysis.normalize_loudness(x, n, sr),
                   resample_4x=lambda: analysis.resample(x, n, sr, 4 * sr),
                   join=lambda: analysis.join_audio(x, n, [0] * B, level=True, ceiling=1.0, fade=110))
        ms = {k: [] for k in fns}
        for rep in range(a.warmup + a.reps):
            for k, fn in fns.items():
                t = timed(fn)
                if rep >= a.warmup:
                    ms[k].append(t)
        res = dict(rows=B, seconds_per_row=seconds, lufs_mean=round(float(st["lufs"].mean()), 3), gain_db_mean=round(float((20 * st["gain"].log10()).mean()), 3),
                   rows_limited=limited, **{k: stats(v) for k, v in ms.items()})
        res["measure_us_per_second_of_audio"] = round(res["measure"]["ms_median"] * 1e3 / (B * seconds), 3)
        out["batches"][name] = res
        print(name, json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
