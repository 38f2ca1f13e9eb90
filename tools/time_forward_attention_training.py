"""Training-step time with forward attention under teacher forcing off and on (GPU box):

    python tools/time_forward_attention_training.py [--steps N] [--warmup W] [--only on|off] [--json out]
    python tools/time_forward_attention_training.py --merge-bench this.jsonl parent.jsonl --json out      (no GPU work)

Vanilla dimensions, seeded weights, the bench's synthetic batch of 32 padded to (L, T) = (188, 872).  ONE trainer runs the steps,
the option switched off / on from step to step (alternated: both see the same clocks and the same drift), each step between two
device events, the engine's segment events on.  Reported per mode: median ms per step, the `fwd.dec.attn_chain` and `bwd.dec.chains`
segments (the two frame loops the option touches) in us per frame, and the workspace the option adds.
--merge-bench: the JSON result lines of `bench.py --gpus 1 --steps 20 --warmup 5` on this tree and on its parent, alternated in one
call (one file per tree, one line per run), go into the same file - the "off means off" record: the option-off step of this tree
must lie inside the parent's own run-to-run range."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def merge_bench(this, parent, out):
    def runs(path):
        rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
        key = next(k for k in ("ms_per_step", "step_ms", "ms_step") if k in rows[0])
        return key, [float(r[key]) for r in rows]
    key, a = runs(this)
    _, b = runs(parent)
    d = json.load(open(out)) if os.path.exists(out) else {}
    d["bench_off_means_off"] = dict(command="bench.py --gpus 1 --steps 20 --warmup 5", order="this tree, parent alternated in one call",
                                    field=key, this_tree=a, parent=b, parent_range=[min(b), max(b)],
                                    this_tree_inside_parent_range=bool(min(b) <= statistics.median(a) <= max(b)))
    with open(out, "w") as f:
        json.dump(d, f, indent=1)
    print(json.dumps(d["bench_off_means_off"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed steps per mode")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per mode")
    ap.add_argument("--only", choices=["on", "off"], default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--merge-bench", nargs=2, default=None, metavar=("THIS", "PARENT"))
    a = ap.parse_args()
    if a.merge_bench:
        return merge_bench(a.merge_bench[0], a.merge_bench[1], a.json)

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
    B, L, T = 32, 188, 872
    batch = Trainer.pad_to(ljspeech_batch(B, seed=1234, num_speakers=4), L, T)
    batch = {k: v.to(dev) for k, v in batch.items()}
    assert batch["chars_idx"].shape == (B, L) and batch["mel_spectrogram"].shape[1] == T
    tr.engine.ensure_concurrent_streams()
    modes = [m for m in ("off", "on") if a.only in (None, m)]

    def step(mode):
        tr.forward_attention = mode == "on"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step(batch, padded=True)
        e1.record()
        return e0, e1, tr.engine.marks
    for _ in range(a.warmup):
        for m in modes:
            step(m)
    torch.cuda.synchronize()
    tr.engine.profile = True
    rec = {m: [] for m in modes}
    for _ in range(a.steps):
        for m in modes:
            rec[m].append(step(m))
    torch.cuda.synchronize()
    tr.engine.profile = False
    tr.engine.check_persistent_kernels()
    out = dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0), B=B, L=L, T=T, steps=a.steps,
               order="off, on alternated step by step in one process" if len(modes) == 2 else modes[0], modes={})
    for m in modes:
        ms = [e0.elapsed_time(e1) for e0, e1, _ in rec[m]]
        seg = {"fwd.dec.attn_chain": [], "bwd.dec.chains": []}
        for _, _, marks in rec[m]:
            s = {n1: x0.elapsed_time(x1) for (_, x0), (n1, x1) in zip(marks[:-1], marks[1:])}
            for k in seg:
                seg[k].append(s[k])
        r = dict(ms_per_step_median=round(statistics.median(ms), 3), ms_per_step_min=round(min(ms), 3), ms_per_step_max=round(max(ms), 3))
        for k, tag in (("fwd.dec.attn_chain", "fwd_chain"), ("bwd.dec.chains", "bwd_chain")):
            r.update({f"{tag}_us_per_frame_median": round(statistics.median(seg[k]) * 1e3 / T, 3),
                      f"{tag}_us_per_frame_min": round(min(seg[k]) * 1e3 / T, 3), f"{tag}_us_per_frame_max": round(max(seg[k]) * 1e3 / T, 3)})
        out["modes"][m] = r
        print(json.dumps({m: r}), flush=True)
    if len(modes) == 2:
        d = lambda k: round(out["modes"]["on"][k] - out["modes"]["off"][k], 3)
        out["on_minus_off"] = {k: d(k) for k in ("ms_per_step_median", "fwd_chain_us_per_frame_median", "bwd_chain_us_per_frame_median")}
        print(json.dumps({"on_minus_off": out["on_minus_off"]}), flush=True)
    if "on" in modes:
        out["workspace_bytes_added"] = {n: t.numel() * t.element_size() for n, t in tr.engine._ws.items() if n == "dprior"}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        prev = json.load(open(a.json)) if os.path.exists(a.json) else {}
        out = dict(prev, **out)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
