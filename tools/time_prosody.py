"""Time of the prosody measurement next to the synthesis it measures (GPU box):

    python tools/time_prosody.py [--reps 20] [--warmup 5] [--batch 8] [--seconds 10] [--json profiles/prosody_timing.json]

B utterances of `seconds` of audio (glides with harmonics, an unvoiced and a silent stretch: tests/prosody_ref.py's generator) at the
default settings (W 1024, lags 44 .. 367, hop 256).  t2_yin and t2_prosody_stats each sit between two device events, library calls
only; ProsodyMeter.measure as `test-correlation --measure` calls it (packing, the two launches, the copy of the rows to the host)
beside them.  Beside them: what one `test-correlation` batch of 8 costs without the measurement - the free-running decode (vanilla
dimensions, seeded weights, 860 frames) and the HiFi-GAN generator (UNIVERSAL_V1 dimensions, seeded weights) on each of its rows."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--no-synthesis", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    import prosody_ref as R
    from tacotron2_amd import _lib, analysis
    from tacotron2_amd.prosody import ProsodyMeter
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sr, B, n = 22050, a.batch, int(a.seconds * 22050)
    meter = ProsodyMeter(sr, dev)
    wavs = [torch.from_numpy(s).to(dev) for s in R.glides(seed=7, lengths=(n,) * B)]
    batch = torch.stack(wavs)
    nd = torch.full((B,), n, dtype=torch.int64, device=dev)
    T = 1 + n // 256
    f0, aper, power = (torch.empty(B, T, device=dev) for _ in range(3))
    stats = torch.empty(B, analysis.PROSODY_NSTAT, device=dev)
    s = meter.settings
    y = _lib.make("T2Yin", wav=batch, ld_wav=n, n=nd, B=B, n_max=n, sr=sr, hop=s["hop"], W=s["W"], tau_min=meter.tau_min,
                  tau_max=meter.tau_max, thr=s["thr"], vthr=s["vthr"], power_floor=s["power_floor"], f0=f0, aper=aper, power=power,
                  cmnd=None)
    p = _lib.make("T2ProsodyStats", f0=f0, aper=aper, power=power, n=nd, B=B, T=T, hop=s["hop"], S=meter.span, out=stats)
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
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                    ms_all=[round(x, 4) for x in ms]), outs[-1]

    out = dict(gpu=torch.cuda.get_device_name(0), B=B, samples=n, frames=T, settings=meter.describe(), reps=a.reps, warmup=a.warmup,
               multiply_adds_per_frame=s["W"] * meter.tau_max)
    out["t2_yin"], _ = series(lambda: _lib.call("t2_yin", y, st))
    out["t2_prosody_stats"], _ = series(lambda: _lib.call("t2_prosody_stats", p, st))
    out["both_launches"], _ = series(lambda: (_lib.call("t2_yin", y, st), _lib.call("t2_prosody_stats", p, st)))
    out["gflops_yin"] = round(3e-9 * B * T * s["W"] * meter.tau_max / (out["t2_yin"]["ms_median"] * 1e-3), 1)     # sub, mul, add
    out["voiced_frames"] = [int(v) for v in stats[:, 1].tolist()]
    out["meter_measure"], rows = series(lambda: meter.measure(wavs, [100] * B))
    out["row0"] = rows[0]
    print(json.dumps(out), flush=True)

    if not a.no_synthesis:
        from bench import VANILLA
        from helpers import write_hifigan_checkpoint
        from tacotron2_amd.engine import Engine
        from tacotron2_amd.hifigan import Generator
        from tacotron2_amd.init import init_parameters
        from tacotron2_amd.params import ParamStore
        from tacotron2_amd.synthetic import ljspeech_batch
        ps = ParamStore(VANILLA, dev)
        init_parameters(ps, seed=0)
        eng = Engine(ps)
        eng.ensure_concurrent_streams()
        ib = ljspeech_batch(B, seed=4321, num_speakers=4)
        ci, cl, spk = ib["chars_idx"].to(dev), ib["chars_idx_len"].to(dev), ib["speaker_id"].to(dev)
        eng.infer(ci, cl, 32, speaker_id=spk, training=False, seed=1)           # warm-up
        torch.cuda.synchronize()
        ms_dec, _ = timed(lambda: eng.infer(ci, cl, 860, speaker_id=spk, training=False, seed=2, check_every=64))
        with tempfile.TemporaryDirectory() as tmp:
            gen = Generator.from_checkpoint(write_hifigan_checkpoint(tmp, n_mels=80, ch0=512), device=dev)
        mel = torch.randn(80, 860, device=dev) * 0.5 - 5.0
        gen(mel[:, :32].contiguous())                                             # warm-up
        torch.cuda.synchronize()
        ms_voc, _ = timed(lambda: [gen(mel) for _ in range(B)])
        eng.check_persistent_kernels()
        both = out["both_launches"]["ms_median"]
        out["synthesis"] = dict(decode_ms=round(ms_dec, 3), vocode_ms=round(ms_voc, 3), frames=860,
                                measure_share_of_decode=round(both / ms_dec, 5),
                                measure_share_of_decode_plus_vocode=round(both / (ms_dec + ms_voc), 5))
        print(json.dumps(out["synthesis"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
