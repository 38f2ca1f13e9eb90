"""Cost of the sample-rate converter (GPU box):

    python tools/time_resample.py [--reps 30] [--warmup 5] [--batch 32] [--json profiles/resample_timing.json]

One batch of `batch` noise signals of LJSpeech-shaped lengths (tools/bench_frontend.py's length model, drawn at the model's rate and
stretched to the input rate) per input rate; Resampler.batch (the output allocation, the copy of the counts, the t2_resample launch)
between two device events, the batched log-mel pass on its output beside it in the same run.  Bytes = input + output floats once,
the table not counted (it stays in L2); multiply-adds = outputs x 2K."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rates", default="24000,16000,44100,48000,8000")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import tacotron2_amd  # noqa: F401
    from tacotron2_amd.datasets.logmel import TacotronMelSpectrogram
    from tacotron2_amd.datasets.resample import Resampler
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1234)
    ell = np.clip(np.round(rng.normal(101, 33.6, a.batch)), 13, 188)
    frames = np.clip(np.round(5.68 * ell + rng.normal(0, 54, a.batch)), 99, 872).astype(int)
    n22 = [(int(t) - 1) * 256 + 100 for t in frames]
    rs, fe = Resampler(22050, dev), TacotronMelSpectrogram(device=dev)

    def series(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))

    out = dict(gpu=torch.cuda.get_device_name(0), batch=a.batch, reps=a.reps, warmup=a.warmup, seconds_of_audio=round(sum(n22) / 22050, 1),
               rates={})
    for sr in [int(s) for s in a.rates.split(",")]:
        U, D, K, table = rs.plan(sr)
        n_in = [n * D // U for n in n22]
        x = torch.zeros(a.batch, (max(n_in) + 63) // 64 * 64)
        for b, n in enumerate(n_in):
            x[b, :n] = torch.from_numpy((rng.standard_normal(n) * 0.1).astype(np.float32))
        x = x.to(dev)
        y, n_out = rs.batch(x, n_in, sr)
        n_dev = torch.tensor(n_out, dtype=torch.int64, device=dev)
        r = series(lambda: rs.batch(x, n_in, sr))
        r.update(U=U, D=D, K=K, table_bytes=int(table.numel() * 4), samples_in=sum(n_in), samples_out=sum(n_out),
                 multiply_adds=sum(n_out) * 2 * K)
        r["gb_per_s"] = round((sum(n_in) + y.numel()) * 4 / (r["ms_median"] * 1e-3) / 1e9, 1)
        r["gmac_per_s"] = round(r["multiply_adds"] / (r["ms_median"] * 1e-3) / 1e9, 1)
        r["logmel_batch_ms_median"] = series(lambda: fe.batch(y, n_dev, max(n_out)))["ms_median"]
        out["rates"][str(sr)] = r
        print(sr, r, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
