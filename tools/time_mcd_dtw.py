"""Time of the MCD-DTW scoring next to the decode it scores (GPU box):

    python tools/time_mcd_dtw.py [--reps 5] [--batch 64] [--ta 872] [--tb 860] [--json profiles/mcd_dtw_timing.json]

B pairs of full length: `ta` frames of "recording" against `tb` frames of "decode" (the bench horizon), smooth random log-mel
tracks and warped noisy copies (tests/mcd_dtw_ref.py's generator), 13 coefficients.  t2_mel_cepstra (both sides) and t2_dtw
(with and without the path) each sit between two device events, library calls only; Engine.mcd_dtw as callers see it (the checks,
the int32 copies of the lengths, the clones) beside them.  `reps` repeats after one warm-up call, all kept.  Beside them: the
decode of the same batch shape (vanilla dimensions, seeded weights, 64 utterances, 860 frames with the stop checks live - the
`decode` measurement of `bench.py --full`, unchanged) and the float64 restatement's time for ONE pair on the host."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ta", type=int, default=872)
    ap.add_argument("--tb", type=int, default=860)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import mcd_dtw_ref as R
    from bench import VANILLA
    from tacotron2_amd.synthetic import ljspeech_batch
    from tacotron2_amd import _lib
    from tacotron2_amd.engine import Engine
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    dev = torch.device("cuda:0")
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, seed=0)
    eng = Engine(ps)
    eng.ensure_concurrent_streams()
    B, Ta, Tb, K, M = a.batch, a.ta, a.tb, 13, 80
    rng = np.random.default_rng(1234)
    A = np.empty((B, Ta, M), dtype=np.float32)
    Bm = np.empty((B, Tb, M), dtype=np.float32)
    for i in range(B):
        A[i] = np.clip(-5.0 + 1.5 * R.trajectory(rng, Ta, M), np.log(1e-5), 2.0)
        Bm[i] = np.clip(R.warped_copy(rng, A[i], Tb, 0.2), np.log(1e-5), 2.0)
    Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev)
    la = torch.full((B,), Ta, dtype=torch.int32, device=dev)
    lb = torch.full((B,), Tb, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def series(fn):
        timed(fn)
        ms, outs = zip(*[timed(fn) for _ in range(a.reps)])
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                    ms_all=[round(x, 4) for x in ms]), outs[-1]

    st = torch.cuda.current_stream().cuda_stream
    basis = eng._ceps_basis(M, K)
    ca, cb = torch.zeros(B, Ta, K, device=dev), torch.zeros(B, Tb, K, device=dev)
    sa = _lib.make("T2MelCeps", mel=Ad, ld_b=Ta * M, ld_t=M, B=B, T=Ta, M=M, K=K, len=la, basis=basis, out=ca, ld_ob=Ta * K, ld_ot=K)
    sb = _lib.make("T2MelCeps", mel=Bd, ld_b=Tb * M, ld_t=M, B=B, T=Tb, M=M, K=K, len=lb, basis=basis, out=cb, ld_ob=Tb * K, ld_ot=K)
    cost = torch.zeros(B, dtype=torch.float64, device=dev)
    plen = torch.zeros(B, dtype=torch.int32, device=dev)
    back = torch.empty(B, Ta, Tb, dtype=torch.uint8, device=dev)
    path = torch.empty(B, Ta + Tb - 1, 2, dtype=torch.int32, device=dev)
    common = dict(a=ca, ld_ab=Ta * K, ld_at=K, b=cb, ld_bb=Tb * K, ld_bt=K, B=B, Ta=Ta, Tb=Tb, K=K, len_a=la, len_b=lb,
                  scale=eng.MCD_SCALE, cost=cost, path_len=plen)
    d0 = _lib.make("T2Dtw", back=None, path=None, **common)
    d1 = _lib.make("T2Dtw", back=back, path=path, **common)

    out = dict(gpu=torch.cuda.get_device_name(0), B=B, Ta=Ta, Tb=Tb, n_ceps=K, reps=a.reps, barriers_per_pair=Ta + Tb - 1)
    out["t2_mel_cepstra_both_sides"], _ = series(lambda: (_lib.call("t2_mel_cepstra", sa, st), _lib.call("t2_mel_cepstra", sb, st)))
    out["t2_dtw_score_only"], _ = series(lambda: _lib.call("t2_dtw", d0, st))
    c0, n0 = cost.clone(), plen.clone()
    out["t2_dtw_with_path"], _ = series(lambda: _lib.call("t2_dtw", d1, st))
    assert torch.equal(c0, cost) and torch.equal(n0, plen)
    out["back_workspace_bytes"] = B * Ta * Tb
    out["engine_mcd_dtw"], res = series(lambda: eng.mcd_dtw(Ad, la, Bd, lb, n_ceps=K))
    assert torch.equal(res[1], c0) and torch.equal(res[2], n0)
    out["mcd_mean_db"] = round(float(res[0].mean()), 4)
    out["path_len_mean"] = round(float(res[2].float().mean()), 1)
    t0 = time.perf_counter()
    ref = R.mcd_dtw(A[0], Bm[0], K)
    out["float64_restatement_one_pair_s"] = round(time.perf_counter() - t0, 4)
    out["pair0_mcd_db"] = dict(gpu=float(res[0][0]), float64=ref[0], path_len_gpu=int(res[2][0]), path_len_float64=ref[2])
    print(json.dumps({k: v for k, v in out.items()}), flush=True)

    if not a.no_decode:
        ib = ljspeech_batch(64, seed=4321, num_speakers=4)
        ci, cl, spk = ib["chars_idx"].to(dev), ib["chars_idx_len"].to(dev), ib["speaker_id"].to(dev)
        eng.infer(ci, cl, 32, speaker_id=spk, training=False, seed=1)           # warm-up
        torch.cuda.synchronize()
        ms, _ = timed(lambda: eng.infer(ci, cl, 860, speaker_id=spk, training=False, seed=2, check_every=64))
        out["decode_64x860_ms"] = round(ms, 3)
        out["dtw_share_of_decode"] = round(out["engine_mcd_dtw"]["ms_median"] / ms, 5)
        print(json.dumps({"decode_64x860_ms": out["decode_64x860_ms"], "dtw_share_of_decode": out["dtw_share_of_decode"]}), flush=True)
    eng.check_persistent_kernels()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
