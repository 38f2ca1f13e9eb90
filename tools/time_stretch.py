"""Cost of the WSOLA time stretch (GPU box):

    python tools/time_stretch.py [--reps 5] [--warmup 1] [--json profiles/time_stretch_timing.json]

Two batches at 22 050 Hz - 64 rows of 4.6 s (the piece buffer of a document, the batch of profiles/say_document_timing.json) and one row
of 10 s - of harmonic tones with a drifting pitch plus noise, through analysis.time_stretch (the allocation of the outputs, the upload
of the counts, the t2_stretch launch) at tempo 0.8 and 1.25 with the product's window (1024) and tolerance (256), between two device
events; a pitch shift of +3 semitones (stretch, then t2_resample) beside it.  Multiply-adds = frames x (2 D + 1) offsets x N."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frame", type=int, default=1024)
    ap.add_argument("--tolerance", type=int, default=256)
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

    def series(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                    ms_all=[round(v, 4) for v in ms])

    out = dict(gpu=torch.cuda.get_device_name(0), sample_rate=sr, frame=a.frame, tolerance=a.tolerance, reps=a.reps, warmup=a.warmup,
               batches={})
    for name, B, seconds in (("64x4.6s", 64, 4.6), ("1x10s", 1, 10.0)):
        n = [int(round(seconds * sr))] * B
        x = torch.from_numpy(np.stack([voice(n[0]) for _ in range(B)])).to(dev)
        res = dict(rows=B, seconds_per_row=seconds)
        for tempo in (0.8, 1.25):
            y, n_out, pos = analysis.time_stretch(x, n, tempo, a.frame, a.tolerance)
            assert bool(torch.isfinite(y).all())
            r = series(lambda: analysis.time_stretch(x, n, tempo, a.frame, a.tolerance))
            frames = sum(-(-k // (a.frame // 2)) for k in n_out)
            r.update(samples_out=sum(n_out), frames=frames, multiply_adds=frames * (2 * a.tolerance + 1) * a.frame)
            r["gmac_per_s"] = round(r["multiply_adds"] / (r["ms_median"] * 1e-3) / 1e9, 1)
            r["us_per_frame_of_a_row"] = round(r["ms_median"] * 1e3 / (frames / B), 2)
            r["x_real_time_per_row"] = round(seconds * 1e3 / r["ms_median"], 1)
            res[f"tempo_{tempo}"] = r
            print(name, tempo, r, flush=True)
        r = series(lambda: analysis.pitch_shift(x, n, 3.0, sr, 1.0, a.frame, a.tolerance))
        res["pitch_shift_+3"] = r
        print(name, "pitch +3", r, flush=True)
        out["batches"][name] = res
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
