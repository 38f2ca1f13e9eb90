"""Training-step and decode-frame time with zoneout off and on (GPU box):

    python tools/time_zoneout.py [--steps N] [--warmup W] [--rate 0.1] [--frames F] [--json out]

Vanilla dimensions, seeded weights, the bench's synthetic batch of 32 padded to (L, T) = (188, 872).  ONE trainer runs the steps,
the option switched off / on from step to step (alternated: both see the same clocks and the same drift; Engine.zoneout is read by
make_masks at every step), each step between two device events, the engine's segment events on.  Reported per mode: median ms per
step, the forward and backward frame loops (`fwd.dec.attn_chain`, `bwd.dec.chains`) in us per frame, and the workspace the option
adds (four [T][B][H] mask tensors and the two dhz carries).  Then the decode loop, F frames at B = 1 and B = 64 with a stop logit that
never fires, off / on alternated call by call: us per frame."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ADDED = ("mask.att_zone_h", "mask.att_zone_c", "mask.dec_zone_h", "mask.dec_zone_c", "dhz_att", "dhz_dec")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed steps per mode")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per mode")
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--frames", type=int, default=400, help="decode frames per timed call")
    ap.add_argument("--calls", type=int, default=5, help="timed decode calls per mode and batch size")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    from bench import VANILLA
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.synthetic import ljspeech_batch
    from tacotron2_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, seed=0)
    tr = Trainer(ps, lr=1e-3, weight_decay=1e-6, scheduler_milestones=(50000, 75000))
    eng = tr.engine
    B, L, T = 32, 188, 872
    batch = Trainer.pad_to(ljspeech_batch(B, seed=1234, num_speakers=4), L, T)
    batch = {k: v.to(dev) for k, v in batch.items()}
    eng.ensure_concurrent_streams()
    setting = {"off": 0.0, "on": a.rate}
    modes = ("off", "on")

    def step(mode):
        eng.zoneout = setting[mode]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step(batch, padded=True)
        e1.record()
        return e0, e1, eng.marks
    for _ in range(a.warmup):
        for m in modes:
            step(m)
    torch.cuda.synchronize()
    eng.profile = True
    rec = {m: [] for m in modes}
    for _ in range(a.steps):
        for m in modes:
            rec[m].append(step(m))
    torch.cuda.synchronize()
    eng.profile = False
    eng.check_persistent_kernels()
    out = dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0), B=B, L=L, T=T, rate=a.rate, steps=a.steps,
               order="off, on alternated step by step in one process", train={}, decode={})
    for m in modes:
        ms = [e0.elapsed_time(e1) for e0, e1, _ in rec[m]]
        segs = {"fwd.dec.attn_chain": [], "bwd.dec.chains": []}
        for _, _, marks in rec[m]:
            seg = {n1: x0.elapsed_time(x1) for (_, x0), (n1, x1) in zip(marks[:-1], marks[1:])}
            for k in segs:
                segs[k].append(seg[k])
        out["train"][m] = dict(ms_per_step_median=round(statistics.median(ms), 3), ms_per_step_min=round(min(ms), 3),
                               ms_per_step_max=round(max(ms), 3),
                               fwd_chain_us_per_frame_median=round(statistics.median(segs["fwd.dec.attn_chain"]) * 1e3 / T, 3),
                               bwd_chain_us_per_frame_median=round(statistics.median(segs["bwd.dec.chains"]) * 1e3 / T, 3))
        print(json.dumps({"train " + m: out["train"][m]}), flush=True)
    added = {n: t.numel() * t.element_size() for n, t in eng._ws.items() if n in ADDED}
    out["workspace_bytes"] = dict(total=eng.workspace_report()["total_bytes"], added=added, added_total=sum(added.values()))
    print(json.dumps({"workspace_bytes": out["workspace_bytes"]}), flush=True)

    # decode: the stop logit never goes negative, so every call runs its F frames
    ps.P["decoder.gate.weight"].zero_()
    ps.P["decoder.gate.bias"].fill_(5.0)
    for Bd in (1, 64):
        b = ljspeech_batch(Bd, seed=77, num_speakers=4)
        ci, lens, spk = b["chars_idx"].to(dev), b["chars_idx_len"].to(dev), b["speaker_id"].to(dev)

        def decode(mode):
            eng.zoneout = setting[mode]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = eng.infer(ci, lens, a.frames, speaker_id=spk, check_every=a.frames)
            e1.record()
            torch.cuda.synchronize()
            assert o[0].shape[1] == a.frames
            return e0.elapsed_time(e1) * 1e3 / a.frames
        for m in modes:
            decode(m)
        us = {m: [] for m in modes}
        for _ in range(a.calls):
            for m in modes:
                us[m].append(decode(m))
        out["decode"][f"B{Bd}"] = {m: dict(us_per_frame_median=round(statistics.median(us[m]), 3), us_per_frame_min=round(min(us[m]), 3),
                                           us_per_frame_max=round(max(us[m]), 3)) for m in modes}
        print(json.dumps({f"decode B{Bd}": out["decode"][f"B{Bd}"]}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
