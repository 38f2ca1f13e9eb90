"""Cost of the vocoder-bias denoiser (GPU box):

    python tools/time_denoise.py [--reps 7] [--warmup 2] [--out profiles/denoise_timing.txt]

The two batches of tools/time_limiter.py at 22 050 Hz - 64 rows of 4.6 s (the pieces of one `say --text-file` chunk) and one row of
10 s - of harmonic tones with a drifting pitch plus noise, and as the bias the interior-frame mean of a faint stationary buzz.  Timed
between two device events, in ONE process and ALTERNATED repetition by repetition, so that a drift of the machine meets all alike:
  denoise      analysis.denoise of the rows at strength 0.1: the allocations, the upload of the counts, two small memsets and ONE
               launch of t2_denoise;
  magnitudes   analysis.stft_magnitudes of the rows: t2_denoise's analysis mode, which writes the (B, F, 513) magnitudes;
  composition  what the parent commit could do with the pieces it had: per row vocoder.GriffinLim.stft (a dense 1024 x 1026 DFT GEMM),
               the same gate in torch, GriffinLim.istft (a GEMM and torch.nn.functional.fold).  It returns 256 (F - 1) samples per
               row where denoise returns all n; where both have samples they agree to float32 rounding, which is checked."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import tacotron2_amd  # noqa: F401
    from tacotron2_amd import analysis
    from tacotron2_amd.vocoder import GriffinLim
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    sr, strength = 22050, 0.1
    rng = np.random.default_rng(1234)
    gl = GriffinLim(sample_rate=sr, device=dev)

    def voice(n):
        t = np.arange(n) / sr
        f0 = rng.uniform(90, 250) * (1.0 + 0.1 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0) * t))
        ph = 2 * np.pi * np.cumsum(f0) / sr
        return (0.3 * sum(np.sin(k * ph) / k for k in range(1, 6)) + 0.003 * rng.standard_normal(n)).astype(np.float32)

    i = np.arange(22528)
    buzz = sum(amp * np.sin(2 * np.pi * h * i / 64.0 + ph) for h, amp, ph in ((1, 2e-3, 0.3), (2, 1e-3, 1.1), (4, 5e-4, 2.0))).astype(np.float32)
    m = analysis.stft_magnitudes(torch.from_numpy(buzz).to(dev)[None, :], [len(buzz)])[0]
    bias = m[2:len(buzz) // 256 - 1].double().mean(dim=0).float()

    def composed(x, n):
        out = []
        for b in range(x.shape[0]):
            spec = gl.stft(x[b, :n[b]])
            mag = torch.sqrt(spec[:, 0] * spec[:, 0] + spec[:, 1] * spec[:, 1])
            thr = strength * bias[None, :]
            g = torch.where(mag > thr, (mag - thr) / mag, torch.zeros_like(mag))
            out.append(gl.istft(spec * g[:, None, :]))
        return out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"# python tools/time_denoise.py --reps {a.reps} --warmup {a.warmup}; {torch.cuda.get_device_name(0)}; {sr} Hz, strength {strength}",
             "# device events; the three alternated repetition by repetition in one process; ms: median (min .. max)"]
    for name, B, seconds in (("64x4.6s", 64, 4.6), ("1x10s", 1, 10.0)):
        n = [int(round(seconds * sr))] * B
        x = torch.from_numpy(np.stack([voice(n[0]) for _ in range(B)])).to(dev)
        y, st = analysis.denoise(x, n, bias, strength)
        ref = composed(x, n)
        k = ref[0].numel()
        diff = max(float((y[b, 1024:k - 1024] - ref[b][1024:k - 1024]).abs().max()) for b in range(B))
        assert bool(torch.isfinite(y).all()) and diff <= 1e-4, diff
        fns = dict(denoise=lambda: analysis.denoise(x, n, bias, strength), magnitudes=lambda: analysis.stft_magnitudes(x, n),
                   composition=lambda: composed(x, n))
        ms = {k: [] for k in fns}
        for rep in range(a.warmup + a.reps):
            for k, fn in fns.items():
                t = timed(fn)
                if rep >= a.warmup:
                    ms[k].append(t)
        lines.append(f"{name}: {B} rows of {seconds} s, {int(st['frames'][0])} frames per row, {100.0 * float(st['gated_fraction'].mean()):.2f} % of bins gated, "
                     f"max |denoise - composition| in the interior {diff:.2e}")
        for k, v in ms.items():
            lines.append(f"  {k:12s} {statistics.median(v):9.4f} ms ({min(v):.4f} .. {max(v):.4f})")
        lines.append(f"  composition / denoise = {statistics.median(ms['composition']) / statistics.median(ms['denoise']):.1f}; "
                     f"denoise: {statistics.median(ms['denoise']) * 1e3 / (B * seconds):.3f} us per second of audio")
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
