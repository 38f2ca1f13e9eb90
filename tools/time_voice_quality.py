"""Cost of the corpus measurement (GPU box):

    python tools/time_voice_quality.py [--reps 20] [--warmup 5] [--batch 64] [--utterances 512] [--json profiles/voice_quality_timing.json]

Kernels: one batch of `batch` waveforms of LJSpeech-shaped lengths (tools/bench_frontend.py's length model; glides with harmonics, an
unvoiced and a silent stretch: tests/prosody_ref.py's generator) at the default settings.  t2_yin, t2_pitch_viterbi, t2_voice_quality,
t2_prosody_stats and t2_corpus_stats each sit between two device events, library calls only, on the same batch in the same run;
ProsodyMeter.features (packing, all launches, the copy of the rows to the host) beside them.

Command: `prosody-export`'s measuring loop (run/prosody_export.py: measure_manifest - decode by the thread pool, one features() call per
batch) in utterances/s on tools/bench_frontend.py's noise corpus, next to the loader alone (DeviceBatchLoader + DevicePrefetcher) on
the same files in the same run; then the same loop on the same lengths filled with voiced glides (noise is unvoiced: the voice-quality
kernel has nothing to match there)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import prosody_ref as R
    from bench_frontend import make_manifest
    from concurrent.futures import ThreadPoolExecutor
    from tacotron2_amd import _lib, analysis
    from tacotron2_amd.datasets.tts_dataset import DeviceBatchLoader, DevicePrefetcher, TTSDataset
    from tacotron2_amd.prosody import ProsodyMeter
    from tacotron2_amd.run.prosody_export import host_threads, measure_manifest
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sr, B = 22050, a.batch
    rng = np.random.default_rng(1234)
    ell = np.clip(np.rint(rng.normal(101, 33.6, size=B)), 13, 188)
    frames = np.clip(np.rint(5.68 * ell + rng.normal(0, 54, size=B)), 99, 872).astype(int)
    lens = [int((t - 1) * 256 + 100) for t in frames]
    signals = R.glides(seed=7, lengths=tuple(lens))
    n = max(lens)
    meter = ProsodyMeter(sr, dev, smooth=True)
    s = meter.settings
    wavs = [torch.from_numpy(x).to(dev) for x in signals]
    batch = torch.zeros(B, n, device=dev)
    for k, w in enumerate(wavs):
        batch[k, :lens[k]] = w
    nd = torch.tensor(lens, dtype=torch.int64, device=dev)
    T = 1 + n // 256
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def series(fn):
        for _ in range(a.warmup):
            timed(fn)
        ms, outs = zip(*[timed(fn) for _ in range(a.reps)])
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4)), outs[-1]

    out = dict(gpu=torch.cuda.get_device_name(0), B=B, frames=T, samples_total=int(sum(lens)), settings=meter.describe(), reps=a.reps,
               warmup=a.warmup)
    y_out = [torch.empty(B, T, device=dev) for _ in range(3)]
    y = _lib.make("T2Yin", wav=batch, ld_wav=n, n=nd, B=B, n_max=n, sr=sr, hop=s["hop"], W=s["W"], tau_min=meter.tau_min,
                  tau_max=meter.tau_max, thr=s["thr"], vthr=s["vthr"], power_floor=s["power_floor"], f0=y_out[0], aper=y_out[1],
                  power=y_out[2], cmnd=None)
    out["t2_yin"], _ = series(lambda: _lib.call("t2_yin", y, st))
    out["t2_yin_with_cmnd"], (_, _, power, cmnd) = series(lambda: analysis.yin(batch, nd, n_max=n, return_cmnd=True, **s))
    out["t2_pitch_viterbi"], (f0, aper, _, _) = series(lambda: analysis.pitch_viterbi(
        cmnd, power, nd, sr=sr, hop=s["hop"], fmin=s["fmin"], fmax=s["fmax"], power_floor=s["power_floor"], **meter.viterbi))
    outs = [torch.empty(B, T, device=dev) for _ in range(4)] + [torch.empty(B, T, dtype=torch.int32, device=dev)]
    v = _lib.make("T2VoiceQuality", wav=batch, ld_wav=n, n=nd, B=B, n_max=n, sr=sr, hop=s["hop"], W=s["W"], tau_min=meter.tau_min,
                  tau_max=meter.tau_max, f0=f0, jitter=outs[0], shimmer=outs[1], nhr=outs[2], hnr_db=outs[3], cycles=outs[4], cyc=None)
    out["t2_voice_quality"], _ = series(lambda: _lib.call("t2_voice_quality", v, st))
    out["measured_frames"] = int((outs[4] > 0).sum())
    out["cycles_matched"] = int(outs[4].sum())
    out["t2_prosody_stats"], _ = series(lambda: analysis.prosody_stats(f0, aper, power, nd, hop=s["hop"], span=meter.span))
    out["t2_corpus_stats"], _ = series(lambda: analysis.corpus_stats(f0, power, *outs, nd, hop=s["hop"], span=meter.span))
    out["meter_features"], rows = series(lambda: meter.features(wavs, [100] * B))
    out["meter_measure"], _ = series(lambda: meter.measure(wavs, [100] * B))
    out["voice_quality_over_yin"] = round(out["t2_voice_quality"]["ms_median"] / out["t2_yin"]["ms_median"], 4)
    out["row0"] = rows[0]
    print(json.dumps(out), flush=True)

    tmp = tempfile.mkdtemp(prefix="t2_vq_")
    try:
        root = os.path.join(tmp, "wavs")
        files, texts = make_manifest(root, a.utterances)
        ds = TTSDataset(filenames=files, texts=texts, base_dir=root, silence=512, trim=True, device=dev)
        threads = host_threads()
        ld = DeviceBatchLoader(ds, batch_size=32, shuffle=True, drop_last=True, seed=0, decode_threads=4)
        pf = DevicePrefetcher(ld, lambda b, d: b.to_device(d), dev, depth=2, limit=a.utterances // 32)
        torch.cuda.synchronize(); t0 = time.perf_counter(); nb = 0
        for _ in pf:
            nb += 1
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        cmd = dict(utterances=a.utterances, batch=B, decode_threads=threads, loader_alone_utt_per_s=round(nb * 32 / dt, 1),
                   loader_alone_decode_threads=4)
        n_chars = [len(i) for i in ds.ids]

        def export_rate(dataset):
            with ThreadPoolExecutor(max_workers=threads) as pool:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                feats, _ = measure_manifest(dataset, meter, n_chars, B, pool, analysis.PROSODY_MAX_T)
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
            return round(len(dataset) / dt, 1), sum(1 for f in feats if f is not None and f["n_measured"] > 0)

        export_rate(ds)                                       # warm-up: file cache, allocator
        cmd["export_noise_utt_per_s"], cmd["export_noise_measured_utts"] = export_rate(ds)
        for i, f in enumerate(files):                         # the same lengths, voiced
            with wave.open(os.path.join(root, f), "rb") as w:
                m = w.getnframes()
            x = R.glides(seed=i, lengths=(m,))[0]
            with wave.open(os.path.join(root, f), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes((x * 32767).astype("<i2").tobytes())
        export_rate(ds)
        cmd["export_voiced_utt_per_s"], cmd["export_voiced_measured_utts"] = export_rate(ds)
        out["command"] = cmd
        print(json.dumps(cmd), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
