"""Training-step and decode time against the reduction factor r (mel frames per decoder step; GPU box):

    python tools/time_reduction_factor.py [--steps N] [--warmup W] [--factors 1,2,3] [--decode-steps 200] [--reps R] [--json out]
    python tools/time_reduction_factor.py --merge-bench this.jsonl parent.jsonl --json out      (no GPU work)

Training: vanilla dimensions, seeded weights, the bench's synthetic batch of 32 padded to (L, T) = (188, 872).  ONE trainer per
factor (the factor changes `decoder.mel_out`, so each has its own parameters), stepped in turn - r = 1, 2, 3, 1, 2, 3, ... - in one
process, so that all see the same clocks and the same drift; each step between two device events, the engine's segment events on.
Reported per factor: ms per step (median, min, max), the `fwd.dec.attn_chain` and `bwd.dec.chains` segments - the two step loops -
in ms per step of training and in us per mel FRAME (segment / T) and per decoder STEP (segment / ceil(T / r)), and
Engine.workspace_report() after the steps.
Decode (tools/time_decode_forward.py's method): every text has the full length 188, the stop-logit bias is raised so that nothing
stops, `--decode-steps` decoder steps per run (r times as many frames), r = 1 and r = 2 alternated `--reps` times at B = 1 and B = 64;
the `inf.frame_loop` segment divided by the frames emitted.
--merge-bench [--bench-tag TAG --bench-order TEXT]: the JSON result lines of `bench.py --gpus 1 --steps 20 --warmup 5` on this tree and on its parent, alternated in one
call (one file per tree, one line per run), go into the same file - the "off means off" record: this tree's median must lie inside
the parent's own run-to-run range.  A repeated call goes in beside the first one under `bench_off_means_off_<TAG>`."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def merge_bench(this, parent, out, tag="", order="this tree, parent alternated in one call"):
    def runs(path):
        rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
        key = next(k for k in ("ms_per_step", "step_ms", "ms_step") if k in rows[0])
        return key, [float(r[key]) for r in rows]
    key, a = runs(this)
    _, b = runs(parent)
    d = json.load(open(out)) if os.path.exists(out) else {}
    key_out = "bench_off_means_off" + ("_" + tag if tag else "")          # (--bench-tag: a further call beside the first, not over it)
    d[key_out] = dict(command="bench.py --gpus 1 --steps 20 --warmup 5", order=order,
                                    field=key, this_tree=a, parent=b, this_tree_median=statistics.median(a),
                                    parent_range=[min(b), max(b)],
                                    this_tree_inside_parent_range=bool(min(b) <= statistics.median(a) <= max(b)))
    with open(out, "w") as f:
        json.dump(d, f, indent=1)
    print(json.dumps(d[key_out]))


def time_training(a, factors, dev):
    import torch
    from bench import VANILLA
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.synthetic import ljspeech_batch
    from tacotron2_amd.trainer import Trainer
    B, L, T = 32, 188, 872
    batch = Trainer.pad_to(ljspeech_batch(B, seed=1234, num_speakers=4), L, T)
    batch = {k: v.to(dev) for k, v in batch.items()}
    assert batch["chars_idx"].shape == (B, L) and batch["mel_spectrogram"].shape[1] == T
    trs = {}
    for r in factors:
        ps = ParamStore(dict(VANILLA, reduction_factor=r) if r != 1 else VANILLA, dev)
        init_parameters(ps, seed=0)
        trs[r] = Trainer(ps, lr=1e-3, weight_decay=1e-6, scheduler_milestones=(50000, 75000))
        trs[r].engine.ensure_concurrent_streams()

    def step(r):
        tr = trs[r]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step(batch, padded=True)
        e1.record()
        return e0, e1, tr.engine.marks
    for _ in range(a.warmup):
        for r in factors:
            step(r)
    torch.cuda.synchronize()
    for tr in trs.values():
        tr.engine.profile = True
    rec = {r: [] for r in factors}
    for _ in range(a.steps):
        for r in factors:
            rec[r].append(step(r))
    torch.cuda.synchronize()
    out = {}
    for r in factors:
        trs[r].engine.profile = False
        trs[r].engine.check_persistent_kernels()
        S = (T + r - 1) // r
        ms = [e0.elapsed_time(e1) for e0, e1, _ in rec[r]]
        seg = {"fwd.dec.attn_chain": [], "bwd.dec.chains": []}
        for _, _, marks in rec[r]:
            s = {n1: x0.elapsed_time(x1) for (_, x0), (n1, x1) in zip(marks[:-1], marks[1:])}
            for k in seg:
                seg[k].append(s[k])
        row = dict(decoder_steps=S, ms_per_step_median=round(statistics.median(ms), 3), ms_per_step_min=round(min(ms), 3),
                   ms_per_step_max=round(max(ms), 3))
        for k, tag in (("fwd.dec.attn_chain", "fwd_chain"), ("bwd.dec.chains", "bwd_chain")):
            med = statistics.median(seg[k])
            row.update({f"{tag}_ms_median": round(med, 3), f"{tag}_ms_min": round(min(seg[k]), 3), f"{tag}_ms_max": round(max(seg[k]), 3),
                        f"{tag}_us_per_frame": round(med * 1e3 / T, 3), f"{tag}_us_per_decoder_step": round(med * 1e3 / S, 3)})
        rep = trs[r].engine.workspace_report()
        row["workspace_total_bytes"] = rep["total_bytes"]; row["workspace_buffers"] = rep["buffers"]; row["workspace_largest"] = rep["largest"]
        out[str(r)] = row
        print(json.dumps({f"r={r}": row}), flush=True)
    if 1 in factors:
        base = out["1"]
        for r in factors:
            if r != 1:
                o = out[str(r)]
                o["below_r1_range"] = dict(ms_per_step=bool(o["ms_per_step_median"] < base["ms_per_step_min"]),
                                           fwd_chain=bool(o["fwd_chain_ms_median"] < base["fwd_chain_ms_min"]),
                                           bwd_chain=bool(o["bwd_chain_ms_median"] < base["bwd_chain_ms_min"]))
    return dict(B=B, L=L, T=T, steps=a.steps, order=", ".join(f"r={r}" for r in factors) + " in turn, step by step, one process",
                factors=out)


def time_decode(a, dev):
    import torch
    from bench import VANILLA
    from tacotron2_amd.engine import Engine
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    L, N = 188, a.decode_steps
    engs = {}
    for r in (1, 2):
        ps = ParamStore(dict(VANILLA, reduction_factor=r) if r != 1 else VANILLA, dev)
        init_parameters(ps, 0)
        with torch.no_grad():
            ps.P["decoder.gate.bias"].add_(10.0)       # no utterance stops: every run decodes exactly N decoder steps
        engs[r] = Engine(ps)
    rows = []
    for B in (1, 64):
        g = torch.Generator().manual_seed(1234 + L + B)
        ci = torch.randint(1, VANILLA["num_chars"], (B, L), generator=g).to(dev)
        cl = torch.full((B,), L, dtype=torch.int64, device=dev)
        spk = torch.randint(0, VANILLA.get("num_speakers", 1), (B,), generator=g).to(dev) if VANILLA.get("speaker_tokens") else None
        for r, eng in engs.items():
            eng.infer(ci, cl, 16 * r, speaker_id=spk, training=False, seed=1)
        torch.cuda.synchronize()
        us = {1: [], 2: []}
        for _ in range(a.reps):
            for r, eng in engs.items():
                eng.profile = True; eng.marks = []; eng.spans = []
                eng.mark("inf.start")
                out = eng.infer(ci, cl, N * r, speaker_id=spk, training=False, seed=2, check_every=64)
                torch.cuda.synchronize()
                eng.profile = False
                frames = int(out[0].shape[1])
                assert frames == N * r and out[3].shape[1] == N, (frames, out[3].shape)
                us[r].append(round(eng.segment_times_ms().get("inf.frame_loop", 0.0) * 1e3 / frames, 2))
        row = dict(B=B, L=L, decoder_steps=N, r1_us_per_frame=us[1], r2_us_per_frame=us[2],
                   r1_median=round(statistics.median(us[1]), 2), r2_median=round(statistics.median(us[2]), 2),
                   r1_spread=round(max(us[1]) - min(us[1]), 2))
        row["r2_us_per_decoder_step"] = round(2 * row["r2_median"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(reps=a.reps, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed training steps per factor")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per factor")
    ap.add_argument("--factors", default="1,2,3")
    ap.add_argument("--decode-steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", choices=["training", "decode"], default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--merge-bench", nargs=2, default=None, metavar=("THIS", "PARENT"))
    ap.add_argument("--bench-tag", default="", help="--merge-bench: write the entry as bench_off_means_off_<tag> (a repeated call)")
    ap.add_argument("--bench-order", default="this tree, parent alternated in one call", help="--merge-bench: how the runs were ordered")
    a = ap.parse_args()
    if a.merge_bench:
        return merge_bench(a.merge_bench[0], a.merge_bench[1], a.json, a.bench_tag, a.bench_order)
    import torch
    assert torch.cuda.is_available(), "this tool times the GPU: no device, no number"
    dev = torch.device("cuda:0")
    out = dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0))
    if a.skip != "training":
        out["training"] = time_training(a, [int(x) for x in a.factors.split(",")], dev)
    if a.skip != "decode":
        out["decode"] = time_decode(a, dev)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        prev = json.load(open(a.json)) if os.path.exists(a.json) else {}
        with open(a.json, "w") as f:
            json.dump(dict(prev, **out), f, indent=1)


if __name__ == "__main__":
    main()
