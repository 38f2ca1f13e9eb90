"""Cost of the optimiser options (GPU box): the `optimizer` segment of the bench batch's training step.

    python tools/time_optimizer_options.py [--steps N] [--warmup W] [--json out] [--label NAME]
    python tools/time_optimizer_options.py --baseline [--label NAME] ...     (also runs in a checkout of the parent commit)
    python tools/time_optimizer_options.py --summarize out                   (no GPU work)

Vanilla dimensions, seeded weights, the bench's synthetic batch of 32 padded to (L, T) = (188, 872), as tools/time_loss_options.py.  ONE
trainer runs the steps with the engine's segment marks on; the four combinations - off, ema (Adam + EMA), adamw, adamw+ema - are
switched from step to step (alternated: all see the same clocks and the same drift), and the time between the mark in front of the
update and the `optimizer` mark - t2_sumsq plus the Adam launch - is recorded per step.  --baseline builds the Trainer WITHOUT the
optimizer_options argument and times that one mode: copied into a checkout of the parent commit it measures the parent's segment.
Run the baseline twice in the session: the spread of the two medians is the noise figure.  Each run is stored under its --label in
the --json file; --summarize adds the comparison against the expectation: the EMA's segment at most 9/7 of the
parent's (36 against 28 bytes per element) plus the spread, the options-off segment within the spread of the parent's."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"off": {}, "ema": dict(ema_decay=0.999), "adamw": dict(decoupled_weight_decay=True),
         "adamw+ema": dict(decoupled_weight_decay=True, ema_decay=0.999)}


def save(path, out):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        prev = json.load(open(path)) if os.path.exists(path) else {}
        with open(path, "w") as f:
            json.dump(dict(prev, **out), f, indent=1)


def summarize(path):
    d = json.load(open(path))
    runs = d["runs"]
    base = sorted(k for k in runs if runs[k]["baseline"])
    new = [k for k in runs if not runs[k]["baseline"]]
    assert len(base) >= 2 and new, "need two baseline runs and one run of the options"
    meds = [runs[k]["modes"]["off"]["us_median"] for k in base]
    parent, spread = statistics.median(meds), max(meds) - min(meds)
    m = runs[new[-1]]["modes"]
    out = dict(parent_us=round(parent, 2), spread_us=round(spread, 2), parent_runs={k: runs[k]["modes"]["off"]["us_median"] for k in base},
               expectation=dict(ema_at_most_us=round(parent * 9 / 7 + spread, 2), off_within_us=round(spread, 2)),
               measured={k: v["us_median"] for k, v in m.items()},
               ema_over_parent={k: round(m[k]["us_median"] / parent, 4) for k in m},
               ema_within_expectation=all(m[k]["us_median"] <= parent * 9 / 7 + spread for k in m if "ema" in k),
               off_within_spread=abs(m["off"]["us_median"] - parent) <= spread)
    save(path, dict(summary=out))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="timed steps per mode")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per mode")
    ap.add_argument("--baseline", action="store_true", help="a Trainer without the optimizer_options argument, one mode")
    ap.add_argument("--label", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)

    import torch
    from bench import VANILLA
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.synthetic import ljspeech_batch
    from tacotron2_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, seed=0)
    kw = dict(lr=1e-3, weight_decay=1e-6, scheduler_milestones=(50000, 75000))
    if a.baseline:
        tr = Trainer(ps, **kw)
        modes = ["off"]
    else:
        from tacotron2_amd.options import check_optimizer_options
        tr = Trainer(ps, optimizer_options={}, **kw)
        modes = list(MODES)
        ps.init_ema()
    B, L, T = 32, 188, 872
    batch = Trainer.pad_to(ljspeech_batch(B, seed=1234, num_speakers=4), L, T)
    batch = {k: v.to(dev) for k, v in batch.items()}
    assert batch["chars_idx"].shape == (B, L) and batch["mel_spectrogram"].shape[1] == T
    tr.engine.ensure_concurrent_streams()
    tr.engine.profile = True

    def step(mode):
        if not a.baseline:
            tr.optimizer_options = check_optimizer_options(MODES[mode], lr=kw["lr"], milestones=kw["scheduler_milestones"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss3, _ = tr.train_step(batch, padded=True)
        e1.record()
        marks = list(tr.engine.marks)
        i = max(j for j, (name, _) in enumerate(marks) if name == "optimizer")
        return marks[i - 1][1], marks[i][1], e0, e1, loss3.clone()
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
    run = dict(baseline=bool(a.baseline), dims="VANILLA", numel=int(ps.numel), gpu=torch.cuda.get_device_name(0), B=B, L=L, T=T,
               steps=a.steps, order="modes alternated step by step in one process", modes={})
    for m in modes:
        us = [o0.elapsed_time(o1) * 1e3 for o0, o1, _, _, _ in rec[m]]
        ms = [e0.elapsed_time(e1) for _, _, e0, e1, _ in rec[m]]
        run["modes"][m] = dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2),
                               step_ms_median=round(statistics.median(ms), 3),
                               last_loss3=[round(float(x), 5) for x in rec[m][-1][4].cpu()])
        print(json.dumps({a.label or ("baseline" if a.baseline else "options"): {m: run["modes"][m]}}), flush=True)
    prev = json.load(open(a.json)).get("runs", {}) if a.json and os.path.exists(a.json) else {}
    save(a.json, dict(runs=dict(prev, **{a.label or ("baseline" if a.baseline else "options"): run})))


if __name__ == "__main__":
    main()
