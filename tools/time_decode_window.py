"""Frame-loop time of the autoregressive decode with the attention window off and on (GPU box):

    python tools/time_decode_window.py [--attention-window B,F] [--frames N] [--batch 1,64] [--text-len 188,1000] [--json out]

Vanilla dimensions, seeded weights; every text of a batch has the full length L (seeded characters) and the stop-logit bias is
raised so that no utterance stops: each configuration decodes exactly N frames of the same inputs, window off and on.  The
number reported is the `inf.frame_loop` segment (device events around the frame loop) divided by N."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import VANILLA  # noqa: E402
from tacotron2_amd.engine import Engine  # noqa: E402
from tacotron2_amd.init import init_parameters  # noqa: E402
from tacotron2_amd.params import ParamStore  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attention-window", default="1,3")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--batch", default="1,64")
    ap.add_argument("--text-len", default="188,1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-window", action="store_true", help="skip the window-off runs (kernel traces of the windowed kernels)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    win = tuple(int(x) for x in a.attention_window.split(","))
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
            for w in ([win] if a.only_window else [None, win]):
                eng.infer(ci, cl, 16, speaker_id=spk, training=False, seed=1, attention_window=w)    # warm-up
                torch.cuda.synchronize()
                best = None
                for _ in range(a.reps):
                    eng.profile = True; eng.marks = []; eng.spans = []
                    eng.mark("inf.start")
                    t0 = time.perf_counter()
                    out = eng.infer(ci, cl, a.frames, speaker_id=spk, training=False, seed=2, check_every=64,
                                    attention_window=w)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    eng.profile = False
                    seg = eng.segment_times_ms()
                    frames = int(out[0].shape[1])
                    us = seg.get("inf.frame_loop", 0.0) * 1e3 / max(frames, 1)
                    if best is None or us < best["us_per_frame"]:
                        best = dict(B=B, L=L, window=list(w) if w else None, frames=frames, us_per_frame=round(us, 2),
                                    call_ms=round(dt * 1e3, 1))
                rows.append(best)
                print(json.dumps(best), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(dims="VANILLA", gpu=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
