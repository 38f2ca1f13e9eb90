"""Cost of the loss options and of the decode stop threshold (GPU box):

    python tools/time_loss_options.py [--steps N] [--warmup W] [--loss l1+l2,1,8] [--only on|off] [--cycle] [--json out]
    python tools/time_loss_options.py --decode [--frames N] [--json out]
    python tools/time_loss_options.py --merge-kernel-stats kernel_stats.csv --json out      (no GPU work)

Training: vanilla dimensions, seeded weights, the bench's synthetic batch of 32 padded to (L, T) = (188, 872).  ONE trainer runs the
steps, the options switched off / on from step to step (alternated: both see the same clocks and the same drift), each step between
two device events.  --cycle rotates the "on" steps through several option sets, so that a kernel trace of the run
(`rocprofv3 --kernel-trace --stats ... -- python tools/time_loss_options.py --cycle --steps 8`, no counters in that run) holds one
row per instantiation of the loss kernel; --merge-kernel-stats copies those rows into the same file.
Decoding (--decode): us per decoder frame at stop thresholds 0.5 and 0.4, alternated call by call, at B = 1 and B = 64: `frames` frames
of an untrained model whose gate bias is raised so that neither threshold stops it (both calls run the same number of frames)."""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CYCLE = [("l1", False, 1.0), ("l2", True, 1.0), ("l2", False, 8.0), ("l1+l2", True, 8.0)]


def merge_kernel_stats(path, out):
    rows = [r for r in csv.DictReader(open(path)) if "loss_kernel" in r["Name"]]
    assert rows, f"{path}: no loss kernel rows"
    col = lambda r, *names: float(next(r[n] for n in names if n in r))       # (column names differ between rocprofv3 releases)
    d = json.load(open(out)) if os.path.exists(out) else {}
    d["loss_kernels"] = {r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip():
                         dict(calls=int(r["Calls"]), avg_us=round(col(r, "AverageNs", "Average (Nsec)") / 1e3, 2),
                              min_us=round(col(r, "MinNs", "Min (Nsec)") / 1e3, 2), max_us=round(col(r, "MaxNs", "Max (Nsec)") / 1e3, 2))
                         for r in rows}
    with open(out, "w") as f:
        json.dump(d, f, indent=1)
    print(json.dumps(d["loss_kernels"]))


def save(path, out):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        prev = json.load(open(path)) if os.path.exists(path) else {}
        with open(path, "w") as f:
            json.dump(dict(prev, **out), f, indent=1)


def time_decode(a):
    import torch
    from bench import VANILLA
    from tacotron2_amd.engine import Engine
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    dev = torch.device("cuda:0")
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, seed=0)
    ps.P["decoder.gate.bias"].add_(20.0)          # neither threshold stops: every call runs `frames` frames
    eng = Engine(ps)
    res = {}
    for B in (1, 64):
        g = torch.Generator().manual_seed(B)
        L = 120
        ci = torch.randint(1, 40, (B, L), generator=g).to(dev)
        lens = torch.full((B,), L, dtype=torch.int64, device=dev)
        spk = torch.zeros(B, dtype=torch.int32, device=dev) if VANILLA.get("speaker_tokens") else None
        rec = {0.5: [], 0.4: []}
        for it in range(a.warmup + a.steps):
            for tau in (0.5, 0.4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                o = eng.infer(ci, lens, a.frames, speaker_id=spk, seed=it, stop_threshold=tau)
                e1.record()
                torch.cuda.synchronize()
                assert o[0].shape[1] == a.frames, (tau, o[0].shape)
                if it >= a.warmup:
                    rec[tau].append(e0.elapsed_time(e1) * 1e3 / a.frames)
        res[f"B{B}"] = {f"tau_{tau}": dict(us_per_frame_median=round(statistics.median(v), 3), us_per_frame_min=round(min(v), 3),
                                           us_per_frame_max=round(max(v), 3)) for tau, v in rec.items()}
        print(json.dumps({f"B{B}": res[f"B{B}"]}), flush=True)
    save(a.json, dict(decode=dict(frames=a.frames, calls_per_threshold=a.steps, L=120,
                                  note="whole Engine.infer call (encoder, loop, scan, post-net) over the frames run", **res)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed steps per mode (decode: timed calls per threshold)")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per mode")
    ap.add_argument("--loss", default="l1+l2,1,8", help="mel,masked,stop_weight of the `on` steps")
    ap.add_argument("--cycle", action="store_true", help="rotate the `on` steps through several option sets (kernel traces)")
    ap.add_argument("--only", choices=["on", "off"], default=None)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--json", default=None)
    ap.add_argument("--merge-kernel-stats", default=None)
    a = ap.parse_args()
    if a.merge_kernel_stats:
        if not a.json:
            ap.error("--merge-kernel-stats needs --json, the file the rows are merged into")
        return merge_kernel_stats(a.merge_kernel_stats, a.json)
    if a.decode:
        return time_decode(a)

    import torch
    from bench import VANILLA
    from tacotron2_amd.engine import check_loss_options
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.synthetic import ljspeech_batch
    from tacotron2_amd.trainer import Trainer
    mel, masked, w = a.loss.split(",")
    on = check_loss_options((mel, bool(int(masked)), float(w)))
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
    count = [0]

    def step(mode):
        if mode == "off":
            tr.loss_options = check_loss_options(None)
        else:
            tr.loss_options = check_loss_options(CYCLE[count[0] % len(CYCLE)]) if a.cycle else on
            count[0] += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss3, _ = tr.train_step(batch, padded=True)
        e1.record()
        return e0, e1, loss3.clone()
    for _ in range(a.warmup):
        for m in modes:
            step(m)
    torch.cuda.synchronize()
    rec = {m: [] for m in modes}
    for _ in range(a.steps):
        for m in modes:
            rec[m].append(step(m))
    torch.cuda.synchronize()
    tr.engine.check_persistent_kernels()
    out = dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0), B=B, L=L, T=T, steps=a.steps,
               on=[list(c) for c in CYCLE] if a.cycle else list(on),
               order="off, on alternated step by step in one process" if len(modes) == 2 else modes[0], modes={})
    for m in modes:
        ms = [e0.elapsed_time(e1) for e0, e1, _ in rec[m]]
        out["modes"][m] = dict(ms_per_step_median=round(statistics.median(ms), 3), ms_per_step_min=round(min(ms), 3),
                               ms_per_step_max=round(max(ms), 3), last_loss3=[round(float(x), 5) for x in rec[m][-1][2].cpu()])
        print(json.dumps({m: out["modes"][m]}), flush=True)
    save(a.json, out)


if __name__ == "__main__":
    main()
