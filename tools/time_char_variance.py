"""Time of t2_char_variance next to what feeds it (GPU box):

    python tools/time_char_variance.py [--reps 20] [--warmup 5] [--json profiles/char_variance_timing.json]

B = 64 utterances of T = 872 frames (871 * 256 samples: glides with harmonics, an unvoiced and a silent stretch,
tests/prosody_ref.py's generator), L = 188 characters of random durations summing to T, M = 80 mel bins.  The one launch of
t2_char_variance sits between two device events, library calls only, in its four settings (log pitch; interpolation off / on; with
and without the two frame outputs); beside it t2_yin with cmnd and t2_pitch_viterbi of the same batch (the track it reads), and
one eval-mode teacher-forced forward of the batch at vanilla dimensions with seeded weights (the durations it reads)."""
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=872)
    ap.add_argument("--chars", type=int, default=188)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import prosody_ref as R
    from tacotron2_amd import _lib, analysis
    from tacotron2_amd.prosody import ProsodyMeter
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream().cuda_stream
    sr, B, T, L, M = 22050, a.batch, a.frames, a.chars, 80
    n = (T - 1) * 256

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def series(fn, reps=a.reps, warmup=a.warmup):
        for _ in range(warmup):
            timed(fn)
        ms, outs = zip(*[timed(fn) for _ in range(reps)])
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                    ms_all=[round(x, 4) for x in ms]), outs[-1]

    meter = ProsodyMeter(sr, dev, smooth=True)
    s, v = meter.settings, meter.viterbi
    N = meter.tau_max - meter.tau_min
    base = R.glides(seed=7, lengths=(n,) * 8)
    batch = torch.stack([torch.from_numpy(base[k % 8]).to(dev) for k in range(B)])
    nd = torch.full((B,), n, dtype=torch.int64, device=dev)
    f0, aper, power, f0v, aperv = (torch.empty(B, T, device=dev) for _ in range(5))
    cmnd = torch.empty(B, T, meter.tau_max + 1, device=dev)
    y = _lib.make("T2Yin", wav=batch, ld_wav=n, n=nd, B=B, n_max=n, sr=sr, hop=s["hop"], W=s["W"], tau_min=meter.tau_min,
                  tau_max=meter.tau_max, thr=s["thr"], vthr=s["vthr"], power_floor=s["power_floor"], f0=f0, aper=aper, power=power,
                  cmnd=cmnd)
    lw = (v["w"] * torch.log2(torch.arange(meter.tau_min, meter.tau_max, dtype=torch.float64))).to(dev)
    lag = torch.empty(B, T, dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    back = torch.empty(B, T, N + 1, dtype=torch.int16, device=dev)
    flen = torch.full((B,), T, dtype=torch.int32, device=dev)
    p = _lib.make("T2PitchViterbi", cmnd=cmnd, ld_b=T * (meter.tau_max + 1), ld_t=meter.tau_max + 1, power=power, len=flen, lw=lw, B=B,
                  T=T, sr=sr, tau_min=meter.tau_min, tau_max=meter.tau_max, power_floor=s["power_floor"],
                  trans_max=v["w"] * v["max_jump"], u=v["u"], c_sw=v["c_sw"], f0=f0v, aper=aperv, lag=lag, cost=cost, back=back)
    out = dict(gpu=torch.cuda.get_device_name(0), B=B, T=T, L=L, M=M, reps=a.reps, warmup=a.warmup, launches=1,
               lds_bytes=8 * 32 + 8 * 256 + 4 * 512 + 8 * ((T + 63) // 64) + 16 * T + 4 * (L + 1))
    out["t2_yin_with_cmnd"], _ = series(lambda: _lib.call("t2_yin", y, st))
    out["t2_pitch_viterbi"], _ = series(lambda: _lib.call("t2_pitch_viterbi", p, st))
    out["voiced_frames_mean"] = round(float((f0v > 0).sum(dim=1).float().mean()), 1)

    rng = np.random.default_rng(5)
    dur = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        cuts = np.sort(rng.integers(0, T + 1, L - 1))
        dur[b] = np.diff(np.concatenate([[0], cuts, [T]]))
    dur = torch.from_numpy(dur).to(dev)
    mel = (torch.randn(B, T, M, generator=torch.Generator().manual_seed(3)) * 2 - 4).to(dev)
    clen = torch.full((B,), L, dtype=torch.int32, device=dev)
    pitch, energy = (torch.empty(B, L, device=dev) for _ in range(2))
    voiced = torch.empty(B, L, dtype=torch.int32, device=dev)
    fq, fe = (torch.empty(B, T, device=dev) for _ in range(2))
    stats = torch.empty(B, analysis.VAR_NSTAT, dtype=torch.float64, device=dev)
    out["t2_char_variance"] = {}
    for interpolate in (0, 1):
        for frames in (False, True):
            c = _lib.make("T2CharVariance", f0=f0v, ld_f0=T, mel=mel, ld_b=T * M, ld_t=M, dur=dur, ld_dur=L, B=B, T=T, L=L, M=M,
                          log_pitch=1, interpolate=interpolate, chars_len=clen, frames_len=flen, char_pitch=pitch, char_energy=energy,
                          char_voiced=voiced, frame_pitch=fq if frames else None, frame_energy=fe if frames else None, stats=stats)
            key = f"interpolate={interpolate}{' frames' if frames else ''}"
            out["t2_char_variance"][key], _ = series(lambda: _lib.call("t2_char_variance", c, st))
            assert stats[:, 8].tolist() == [1.0] * B and stats[:, 0].tolist() == [float(T)] * B
    tracker = out["t2_yin_with_cmnd"]["ms_median"] + out["t2_pitch_viterbi"]["ms_median"]
    med = out["t2_char_variance"]["interpolate=0"]["ms_median"]
    out["tracker_ms"] = round(tracker, 4)
    out["share_of_tracker"] = round(med / tracker, 5)
    out["stats_row0"] = stats[0].tolist()
    print(json.dumps({k: out[k] for k in ("t2_yin_with_cmnd", "t2_pitch_viterbi", "t2_char_variance", "share_of_tracker")}), flush=True)

    if not a.no_forward:
        from bench import VANILLA
        from tacotron2_amd.engine import Engine
        from tacotron2_amd.init import init_parameters
        from tacotron2_amd.params import ParamStore
        ps = ParamStore(VANILLA, dev)
        init_parameters(ps, seed=0)
        eng = Engine(ps)
        eng.ensure_concurrent_streams()
        g = torch.Generator().manual_seed(1234)
        ci = torch.randint(1, 39, (B, L), generator=g).to(dev)
        lens = torch.full((B,), L, dtype=torch.int64, device=dev)
        tl = torch.full((B,), T, dtype=torch.int64, device=dev)
        spk = torch.zeros(B, dtype=torch.int32, device=dev)

        def fwd():
            masks = eng.make_masks(B, L, T, False, 0, 0)
            return eng.forward_tf(ci, lens, mel, tl, speaker_id=spk, training=False, masks=masks, save_for_backward=False)[0]
        out["forward_tf_eval"], _ = series(fwd, reps=5, warmup=1)
        eng.check_persistent_kernels()
        out["share_of_forward"] = round(med / out["forward_tf_eval"]["ms_median"], 5)
        print(json.dumps(dict(forward_tf_eval=out["forward_tf_eval"], share_of_forward=out["share_of_forward"])), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
