"""Time of one Engine.durations call next to the forward it reads (GPU box):

    python tools/time_durations.py [--reps 5] [--batch 64] [--frames 872] [--text-lens 188,1000] [--json out]

Vanilla dimensions, seeded weights, B = 64 utterances of full length (every text L characters, every mel 872 frames: the
longest recurrence the batch shape allows).  Per text length: ONE eval-mode forward_tf of the batch (masks on, as make_masks gives
them in eval mode), then - in the same process, on its alignments - Engine.durations in both modes.  Every call sits between two
device events; `reps` repeats each after one warm-up call, all kept.  The durations call as timed includes what the engine does
around the kernel (the int32 copies of the lengths, the clones of the two results); the back workspace's size is reported."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=872)
    ap.add_argument("--text-lens", default="188,1000")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    from bench import VANILLA
    from tacotron2_amd.engine import Engine
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    dev = torch.device("cuda:0")
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, seed=0)
    eng = Engine(ps)
    eng.ensure_concurrent_streams()
    B, T = a.batch, a.frames
    g = torch.Generator().manual_seed(1234)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def summary(ms):
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                    ms_all=[round(x, 4) for x in ms])

    out = dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0), B=B, S=T, r=eng.r, reps=a.reps, cases={})
    for L in [int(x) for x in a.text_lens.split(",")]:
        ci = torch.randint(1, 39, (B, L), generator=g).to(dev)
        lens = torch.full((B,), L, dtype=torch.int64, device=dev)
        mel = (torch.randn(B, T, 80, generator=g) - 3).to(dev)
        tl = torch.full((B,), T, dtype=torch.int64, device=dev)
        spk = torch.zeros(B, dtype=torch.int32, device=dev)

        def fwd():
            masks = eng.make_masks(B, L, T, False, 0, 0)
            return eng.forward_tf(ci, lens, mel, tl, speaker_id=spk, training=False, masks=masks, save_for_backward=False)[0]
        timed(fwd)
        f_ms, outs = zip(*[timed(fwd) for _ in range(a.reps)])
        align = outs[-1][3]
        case = dict(L=L, forward_tf_eval=summary(f_ms))
        for mode in ("monotonic", "argmax"):
            run = lambda: eng.durations(align, lens, tl, mode=mode)
            timed(run)
            d_ms, res = zip(*[timed(run) for _ in range(a.reps)])
            dur, stats = res[-1]
            assert dur.sum(1).cpu().tolist() == [T] * B
            case[mode] = dict(summary(d_ms), ratio_to_forward=round(statistics.median(d_ms) / statistics.median(f_ms), 4),
                              focus_rate_mean=round(float(stats[:, 0].mean()), 4), feasible=int(stats[:, 2].sum()),
                              argmax_agreement_mean=round(float(stats[:, 3].mean()), 4))
        case["back_workspace_bytes"] = B * T * L
        eng.check_persistent_kernels()
        out["cases"][f"L={L}"] = case
        print(json.dumps({f"L={L}": case}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
