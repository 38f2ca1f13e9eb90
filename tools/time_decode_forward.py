"""Frame-loop time of the autoregressive decode with forward attention off and on (GPU box):

    python tools/time_decode_forward.py [--frames N] [--batch 1,64] [--text-len 188,1000] [--reps R] [--json out]

Vanilla dimensions, seeded weights; every text of a batch has the full length L (seeded characters) and the stop-logit bias is
raised so that no utterance stops: each configuration decodes exactly N frames of the same inputs.  Off and on ALTERNATE, R times
each in one process, so that both see the same machine; every repeat is kept: the spread between the repeated "off" runs is what a
difference between "off" and "on" has to exceed to mean anything.  The number reported is the `inf.frame_loop` segment (device
events around the frame loop) divided by N."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import VANILLA  # noqa: E402
from tacotron2_amd.engine import Engine  # noqa: E402
from tacotron2_amd.init import init_parameters  # noqa: E402
from tacotron2_amd.params import ParamStore  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--batch", default="1,64")
    ap.add_argument("--text-len", default="188,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the GPU: no device, no number"
    dev = torch.device("cuda:0")
    ps = ParamStore(VANILLA, dev)
    init_parameters(ps, 0)
    with torch.no_grad():
        ps.P["decoder.gate.bias"].add_(10.0)       # no utterance stops: every run decodes exactly --frames frames
    eng = Engine(ps)
    rows = []
    for L in [int(x) for x in a.text_len.split(",")]:
        for B in [int(x) for x in a.batch.split(",")]:
            g = torch.Generator().manual_seed(1234 + L + B)
            ci = torch.randint(1, VANILLA["num_chars"], (B, L), generator=g).to(dev)
            cl = torch.full((B,), L, dtype=torch.int64, device=dev)
            spk = torch.randint(0, VANILLA.get("num_speakers", 1), (B,), generator=g).to(dev) \
                if VANILLA.get("speaker_tokens") else None
            for fa in (False, True):               # warm-up of both paths at this shape
                eng.infer(ci, cl, 16, speaker_id=spk, training=False, seed=1, forward_attention=fa)
            torch.cuda.synchronize()
            us = {False: [], True: []}
            for _ in range(a.reps):
                for fa in (False, True):
                    eng.profile = True; eng.marks = []; eng.spans = []
                    eng.mark("inf.start")
                    out = eng.infer(ci, cl, a.frames, speaker_id=spk, training=False, seed=2, check_every=64, forward_attention=fa)
                    torch.cuda.synchronize()
                    eng.profile = False
                    frames = int(out[0].shape[1])
                    assert frames == a.frames, (frames, a.frames)
                    us[fa].append(round(eng.segment_times_ms().get("inf.frame_loop", 0.0) * 1e3 / frames, 2))
            row = dict(B=B, L=L, frames=a.frames,
                       off_us_per_frame=us[False], on_us_per_frame=us[True],
                       off_median=round(statistics.median(us[False]), 2), on_median=round(statistics.median(us[True]), 2),
                       off_spread=round(max(us[False]) - min(us[False]), 2))
            row["on_minus_off"] = round(row["on_median"] - row["off_median"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
