"""Training-step time with the guided-attention loss off and on (GPU box):

    python tools/time_guided_attention.py [--steps N] [--warmup W] [--guided 0.4,1.0] [--only on|off] [--json out]
    python tools/time_guided_attention.py --merge-kernel-stats kernel_stats.csv --json out      (no GPU work)

Vanilla dimensions, seeded weights, the bench's synthetic batch of 32 padded to (L, T) = (188, 872).  ONE trainer runs the steps,
the term switched off / on from step to step (alternated: both see the same clocks and the same drift), each step between two
device events, the engine's segment events on.  Reported per mode: median ms per step, the `bwd.dec.chains` segment (the backward
frame loop, where the new operand is read) in us per frame, and the workspace the term adds.  The guided kernel's own time comes from
a kernel trace of its own (`rocprofv3 --kernel-trace --stats ... -- python tools/time_guided_attention.py --only on --steps 5`),
merged into the same file with --merge-kernel-stats."""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def merge_kernel_stats(path, out):
    rows = [r for r in csv.DictReader(open(path)) if "guided_attn_kernel" in r["Name"]]
    assert len(rows) == 1, f"{path}: expected one guided_attn_kernel row, found {len(rows)}"
    r = rows[0]
    col = lambda *names: float(next(r[n] for n in names if n in r))       # (column names differ between rocprofv3 releases)
    d = json.load(open(out)) if os.path.exists(out) else {}
    d["guided_kernel"] = dict(calls=int(r["Calls"]), avg_us=round(col("AverageNs", "Average (Nsec)") / 1e3, 2),
                              min_us=round(col("MinNs", "Min (Nsec)") / 1e3, 2), max_us=round(col("MaxNs", "Max (Nsec)") / 1e3, 2))
    with open(out, "w") as f:
        json.dump(d, f, indent=1)
    print(json.dumps(d["guided_kernel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed steps per mode")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per mode")
    ap.add_argument("--guided", default="0.4,1.0")
    ap.add_argument("--only", choices=["on", "off"], default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--merge-kernel-stats", default=None)
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.json)

    import torch
    from bench import VANILLA
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.synthetic import ljspeech_batch
    from tacotron2_amd.trainer import Trainer
    guided = tuple(float(x) for x in a.guided.split(","))
    dev = torch.device("cuda:0")
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, seed=0)
    tr = Trainer(ps, lr=1e-3, weight_decay=1e-6, scheduler_milestones=(50000, 75000))
    B, L, T = 32, 188, 872
    batch = Trainer.pad_to(ljspeech_batch(B, seed=1234, num_speakers=4), L, T)
    batch = {k: v.to(dev) for k, v in batch.items()}
    assert batch["chars_idx"].shape == (B, L) and batch["mel_spectrogram"].shape[1] == T
    tr.engine.ensure_concurrent_streams()
    modes = [m for m in ("off", "on") if a.only in (None, m)]
    setting = {"off": None, "on": guided}

    def step(mode):
        tr.guided_attention = setting[mode]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step(batch, padded=True)
        e1.record()
        return e0, e1, tr.engine.marks
    for _ in range(a.warmup):
        for m in modes:
            step(m)
    torch.cuda.synchronize()
    ws_off = tr.engine.workspace_report()["total_bytes"] - sum(
        t.numel() * t.element_size() for n, t in tr.engine._ws.items() if n.startswith("guided."))
    tr.engine.profile = True
    rec = {m: [] for m in modes}
    for _ in range(a.steps):
        for m in modes:
            rec[m].append(step(m))
    torch.cuda.synchronize()
    tr.engine.profile = False
    tr.engine.check_persistent_kernels()
    out = dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0), B=B, L=L, T=T, guided=list(guided), steps=a.steps,
               order="off, on alternated step by step in one process" if len(modes) == 2 else modes[0], modes={})
    for m in modes:
        ms = [e0.elapsed_time(e1) for e0, e1, _ in rec[m]]
        chains = []
        for _, _, marks in rec[m]:
            seg = {n1: x0.elapsed_time(x1) for (_, x0), (n1, x1) in zip(marks[:-1], marks[1:])}
            chains.append(seg["bwd.dec.chains"])
        out["modes"][m] = dict(ms_per_step_median=round(statistics.median(ms), 3), ms_per_step_min=round(min(ms), 3),
                               ms_per_step_max=round(max(ms), 3),
                               bwd_chain_us_per_frame_median=round(statistics.median(chains) * 1e3 / T, 3),
                               bwd_chain_us_per_frame_min=round(min(chains) * 1e3 / T, 3),
                               bwd_chain_us_per_frame_max=round(max(chains) * 1e3 / T, 3))
        print(json.dumps({m: out["modes"][m]}), flush=True)
    if "on" in modes:
        gb = {n: t.numel() * t.element_size() for n, t in tr.engine._ws.items() if n.startswith("guided.")}
        out["workspace_bytes"] = dict(without_the_term=ws_off, added=gb)
        out["last_guided_loss"] = float(tr.last_guided_loss.cpu())
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        prev = json.load(open(a.json)) if os.path.exists(a.json) else {}
        out = dict(prev, **out)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
