"""Cost of the look-ahead true-peak limiter (GPU box):

    python tools/time_limiter.py [--reps 7] [--warmup 2] [--json profiles/limiter_timing.json]

The two batches of tools/time_loudness.py at 22 050 Hz - 64 rows of 4.6 s (the texts of one `say` call) and one row of 10 s (a joined
document) - of harmonic tones with a drifting pitch plus noise.  Timed between two device events, in ONE process and ALTERNATED
repetition by repetition, so that a drift of the machine meets all of them alike:
  measure            analysis.loudness of the rows: the figure to compare with (profiles/loudness_timing.json);
  limit_active       analysis.limit_peaks of the rows scaled until their sample peak is 1.2, under -1 dBTP: every row is limited - the
                     allocations, the upload of the counts, four launches (envelope, curve, apply and peak, trim);
  limit_idle         the same call on the rows at a sample peak of 0.5: no row passes the ceiling, the curve launch stops behind its
                     first read of the envelope and the apply launch copies;
  normalize_limiter  analysis.normalize_loudness(limiter=True) at -14 LUFS: t2_loudness, t2_limit, t2_loudness."""
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

    out = dict(gpu=torch.cuda.get_device_name(0), sample_rate=sr, ceiling_dbtp=-1.0, lookahead_ms=5.0, release_ms=50.0, reps=a.reps,
               warmup=a.warmup, method="device events; the four alternated repetition by repetition in one process", batches={})
    c = 10.0 ** (-1.0 / 20.0)
    for name, B, seconds in (("64x4.6s", 64, 4.6), ("1x10s", 1, 10.0)):
        n = [int(round(seconds * sr))] * B
        x = torch.from_numpy(np.stack([voice(n[0]) for _ in range(B)])).to(dev)
        top = x.abs().amax(dim=1, keepdim=True)
        loud, quiet = x * (1.2 / top), x * (0.5 / top)
        y, st = analysis.limit_peaks(loud, n, sr)
        again = analysis.loudness(y, n, sr)
        _, idle = analysis.limit_peaks(quiet, n, sr)
        assert bool(torch.isfinite(y).all()) and bool((st["flags"] & 1).ne(0).all()) and float(again["true_peak"].max()) <= c * (1.0 + 1e-5)
        assert not bool(idle["flags"].ne(0).any())
        yn, sn = analysis.normalize_loudness(x, n, sr, target=-14.0, limiter=True)
        fns = dict(measure=lambda: analysis.loudness(x, n, sr), limit_active=lambda: analysis.limit_peaks(loud, n, sr),
                   limit_idle=lambda: analysis.limit_peaks(quiet, n, sr),
                   normalize_limiter=lambda: analysis.normalize_loudness(x, n, sr, target=-14.0, limiter=True))
        ms = {k: [] for k in fns}
        for rep in range(a.warmup + a.reps):
            for k, fn in fns.items():
                t = timed(fn)
                if rep >= a.warmup:
                    ms[k].append(t)
        res = dict(rows=B, seconds_per_row=seconds, limited_samples_mean=round(float(st["n_over"].double().mean()), 1),
                   min_gain_mean=round(float(st["min_gain"].mean()), 4), rows_trimmed=int((st["flags"] & 2).ne(0).sum()),
                   normalize_rows_limited=int((sn["limiter_flags"] & 1).ne(0).sum()), output_lufs_mean=round(float(sn["output_lufs"].mean()), 3),
                   **{k: stats(v) for k, v in ms.items()})
        res["limit_active_us_per_second_of_audio"] = round(res["limit_active"]["ms_median"] * 1e3 / (B * seconds), 3)
        out["batches"][name] = res
        print(name, json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
