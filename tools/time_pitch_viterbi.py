"""Time of the smoothed pitch track and the F0 path statistics next to the decode they score (GPU box):

    python tools/time_pitch_viterbi.py [--reps 20] [--warmup 5] [--json profiles/pitch_viterbi_timing.json]

Two batches at the default settings (W 1024, lags 44 .. 367, hop 256; 323 voiced states): B = 8 utterances of 10 s and B = 64 of 860
frames (glides with harmonics, an unvoiced and a silent stretch: tests/prosody_ref.py's generator).  t2_yin with cmnd,
t2_pitch_viterbi and t2_f0_path_stats (a diagonal path of T cells, the track against itself shifted by a semitone) each sit between
two device events, library calls only; ProsodyMeter.measure without and with smooth beside them, as the drivers call it.  Beside
them: the free-running decode of the same batch (vanilla dimensions, seeded weights, 860 frames)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-synthesis", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    import prosody_ref as R
    from tacotron2_amd import _lib, analysis
    from tacotron2_amd.prosody import ProsodyMeter
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream().cuda_stream
    sr = 22050

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

    raw, smooth = ProsodyMeter(sr, dev), ProsodyMeter(sr, dev, smooth=True)
    s, v = raw.settings, smooth.viterbi
    N = raw.tau_max - raw.tau_min
    out = dict(gpu=torch.cuda.get_device_name(0), settings=smooth.describe(), reps=a.reps, warmup=a.warmup, states=N + 1, cases=[])
    for B, n in ((8, 10 * sr), (64, 859 * 256)):
        T = 1 + n // 256
        base = R.glides(seed=7, lengths=(n,) * 8)
        wavs = [torch.from_numpy(base[k % 8]).to(dev) for k in range(B)]
        batch = torch.stack(wavs)
        nd = torch.full((B,), n, dtype=torch.int64, device=dev)
        f0, aper, power, f0v, aperv = (torch.empty(B, T, device=dev) for _ in range(5))
        cmnd = torch.empty(B, T, raw.tau_max + 1, device=dev)
        y = _lib.make("T2Yin", wav=batch, ld_wav=n, n=nd, B=B, n_max=n, sr=sr, hop=s["hop"], W=s["W"], tau_min=raw.tau_min,
                      tau_max=raw.tau_max, thr=s["thr"], vthr=s["vthr"], power_floor=s["power_floor"], f0=f0, aper=aper, power=power,
                      cmnd=cmnd)
        lw = (v["w"] * torch.log2(torch.arange(raw.tau_min, raw.tau_max, dtype=torch.float64))).to(dev)
        lag = torch.empty(B, T, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        back = torch.empty(B, T, N + 1, dtype=torch.int16, device=dev)
        p = _lib.make("T2PitchViterbi", cmnd=cmnd, ld_b=T * (raw.tau_max + 1), ld_t=raw.tau_max + 1, power=power,
                      len=torch.full((B,), T, dtype=torch.int32, device=dev), lw=lw, B=B, T=T, sr=sr, tau_min=raw.tau_min,
                      tau_max=raw.tau_max, power_floor=s["power_floor"], trans_max=v["w"] * v["max_jump"], u=v["u"], c_sw=v["c_sw"],
                      f0=f0v, aper=aperv, lag=lag, cost=cost, back=back)
        case = dict(B=B, samples=n, frames=T)
        case["t2_yin_with_cmnd"], _ = series(lambda: _lib.call("t2_yin", y, st))
        case["t2_pitch_viterbi"], _ = series(lambda: _lib.call("t2_pitch_viterbi", p, st))
        path = torch.arange(T, dtype=torch.int32, device=dev)[None, :, None].expand(B, T, 2).contiguous()
        stats = torch.empty(B, analysis.F0_NSTAT, dtype=torch.float64, device=dev)
        q = _lib.make("T2F0PathStats", path=path, path_len=torch.full((B,), T, dtype=torch.int32, device=dev), f0_a=f0v,
                      f0_b=(f0v * 2.0 ** (1 / 12)).contiguous(), n_a=nd, n_b=nd, B=B, P=T, Ta=T, Tb=T, hop=s["hop"], S=raw.span, out=stats)
        case["t2_f0_path_stats"], _ = series(lambda: _lib.call("t2_f0_path_stats", q, st))
        case["voiced_frames_raw"] = [int(x) for x in (f0 > 0).sum(dim=1).tolist()][:8]
        case["voiced_frames_smoothed"] = [int(x) for x in (f0v > 0).sum(dim=1).tolist()][:8]
        case["frames_where_the_voicing_differs"] = int(((f0 > 0) != (f0v > 0)).sum())
        case["stats_row0"] = stats[0].tolist()
        case["meter_measure"], r0 = series(lambda: raw.measure(wavs, [100] * B))
        case["meter_measure_smooth"], r1 = series(lambda: smooth.measure(wavs, [100] * B))
        case["row0"], case["row0_smooth"] = r0[0], r1[0]
        print(json.dumps(case), flush=True)

        if not a.no_synthesis:
            from bench import VANILLA
            from tacotron2_amd.engine import Engine
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
            eng.check_persistent_kernels()
            vit = case["t2_pitch_viterbi"]["ms_median"]
            case["decode_ms"] = round(ms_dec, 3)
            case["viterbi_share_of_decode"] = round(vit / ms_dec, 5)
            print(json.dumps(dict(B=B, decode_ms=case["decode_ms"], viterbi_share_of_decode=case["viterbi_share_of_decode"])), flush=True)
            del eng, ps
        out["cases"].append(case)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
