"""Cost of the TD-PSOLA pitch change (GPU box):

    python tools/time_psola.py [--reps 7] [--warmup 2] [--json profiles/psola_timing.json]

The two batches of tools/time_stretch.py at 22 050 Hz - 64 rows of 4.6 s (the piece buffer of a document) and one row of 10 s - of
harmonic tones with a drifting pitch plus noise.  Timed between two device events, in ONE process and ALTERNATED repetition by
repetition, so that a drift of the machine meets all of them alike:
  psola        analysis.psola alone (the allocation of the outputs, the upload of the counts, the t2_psola launch) on a track made
               once in front of the loop, at +3 semitones;
  track        the two pitch-tracking launches it needs: analysis.yin(return_cmnd=True) and analysis.pitch_viterbi;
  psola_shift  the whole analysis.pitch_shift_psola at +3 semitones, tempo 1 (track + pitch_ratio + psola);
  wsola_shift  the existing analysis.pitch_shift at +3 semitones (t2_stretch, then t2_resample), the path it stands beside."""
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
    ap.add_argument("--semitones", type=float, default=3.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import tacotron2_amd  # noqa: F401
    from tacotron2_amd import analysis
    from tacotron2_amd.psola import default_meter
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

    meter = default_meter(sr, dev)
    s = meter.settings
    out = dict(gpu=torch.cuda.get_device_name(0), sample_rate=sr, semitones=a.semitones, reps=a.reps, warmup=a.warmup,
               method="device events; the four alternated repetition by repetition in one process", batches={})
    for name, B, seconds in (("64x4.6s", 64, 4.6), ("1x10s", 1, 10.0)):
        n = [int(round(seconds * sr))] * B
        x = torch.from_numpy(np.stack([voice(n[0]) for _ in range(B)])).to(dev)
        n_dev = torch.tensor(n, dtype=torch.int64, device=dev)

        def track():
            _, _, power, cmnd = analysis.yin(x, n_dev, n_max=n[0], return_cmnd=True, **s)
            return analysis.pitch_viterbi(cmnd, power, n_dev, sr=sr, hop=s["hop"], fmin=s["fmin"], fmax=s["fmax"],
                                          power_floor=s["power_floor"], **meter.viterbi)[2]

        lag = track()
        rho = analysis.pitch_ratio(lag, n, a.semitones, 1.0, s["hop"])
        y, marks = analysis.psola(x, n, lag, rho, s["hop"])
        assert bool(torch.isfinite(y).all()) and int(marks["n_marks"].min()) > 0
        fns = dict(psola=lambda: analysis.psola(x, n, lag, rho, s["hop"]), track=track,
                   psola_shift=lambda: analysis.pitch_shift_psola(x, n, a.semitones, sr),
                   wsola_shift=lambda: analysis.pitch_shift(x, n, a.semitones, sr))
        ms = {k: [] for k in fns}
        for rep in range(a.warmup + a.reps):
            for k, fn in fns.items():
                t = timed(fn)
                if rep >= a.warmup:
                    ms[k].append(t)
        res = dict(rows=B, seconds_per_row=seconds, voiced_share=round(float((lag > 0).float().mean()), 3),
                   analysis_marks=int(marks["n_marks"].sum()), synthesis_marks=int(marks["n_syn"].sum()),
                   **{k: stats(v) for k, v in ms.items()})
        res["psola_share_of_psola_shift"] = round(res["psola"]["ms_median"] / res["psola_shift"]["ms_median"], 3)
        res["us_per_analysis_mark_of_a_row"] = round(res["psola"]["ms_median"] * 1e3 / (res["analysis_marks"] / B), 3)
        out["batches"][name] = res
        print(name, json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
