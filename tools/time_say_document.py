"""Time of `say --text-file`'s stages next to the parent's way of speaking the same pieces (GPU box):

    python tools/time_say_document.py [--reps 5] [--warmup 1] [--json profiles/say_document_timing.json]

A model at vanilla dimensions with seeded weights and a HiFi-GAN generator of V1 shapes (512 initial channels, synthetic weights in
the published layout, tests/helpers.py) speak 64 pieces of LJSpeech-shaped lengths (15 .. 190 characters), every decode cut at 400
frames (the stop gate's bias is set so that it never fires) so that nothing depends on stopping.  Between two device events each: the decode of the 64 pieces as one batch, the
vocoding of its padded batch in one generator call, analysis.join_audio (trim, fades, level; its four launches and its one host
read), and the parent's back end for the same mels - do_say's loop, one generator call and one .cpu() per piece.  Then the whole
document path (say_document) against the whole parent path (the same decode, post.cpu(), that loop), wall clock."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pieces", type=int, default=64)
    ap.add_argument("--max-len", type=int, default=400)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from helpers import write_hifigan_checkpoint
    from tacotron2_amd import analysis
    from tacotron2_amd.datasets.document import Piece
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.hifigan import Generator
    from tacotron2_amd.model.tts_model import TTSModel
    from tacotron2_amd.run.common import emitted_frames
    from tacotron2_amd.run.say import say_document
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sr, P = 22050, a.pieces
    enc = TextEncoder(ALLOWED, "^")
    model = TTSModel(lr=1e-3, weight_decay=1e-6, num_chars=enc.num_chars, device=dev)
    model.eval()
    model.tacotron2._seed = 3
    with torch.no_grad():                       # a stop gate that never fires: every piece runs into --max-len
        model.tacotron2.store.P["decoder.gate.bias"].fill_(30.0)
    with tempfile.TemporaryDirectory() as tmp:
        gen = Generator.from_checkpoint(write_hifigan_checkpoint(os.path.join(tmp, "hifi"), n_mels=80, ch0=512), device=dev)
    rng = np.random.default_rng(11)
    letters = list("abcdefghijklmnopqrstuvwxyz    ,")
    lengths = np.clip(rng.normal(100, 40, P).round().astype(int), 15, 190)                 # LJSpeech: 15 .. 190, about 100 on average
    texts = ["".join(rng.choice(letters, int(k) - 1)) + "." for k in lengths]
    brk = ["sentence", "clause", "paragraph"]
    pieces = [Piece(t, i // 8, brk[i % 3] if i < P - 1 else "end") for i, t in enumerate(texts)]
    ids = sorted((torch.tensor(enc.encode(t), dtype=torch.int64) for t in texts), key=len)
    chars = torch.nn.utils.rnn.pad_sequence(ids, batch_first=True).to(dev)
    lens = torch.tensor([len(i) for i in ids], dtype=torch.int64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    def series(fn):
        for _ in range(a.warmup):
            timed(fn)
        ms, wall, outs = zip(*[timed(fn) for _ in range(a.reps)])
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                    wall_ms_median=round(statistics.median(wall), 4), ms_all=[round(x, 4) for x in ms]), outs[-1]

    def decode():
        with torch.no_grad():
            return model(chars_idx=chars, chars_idx_len=lens, teacher_forcing=False, max_len_override=a.max_len)

    out = dict(gpu=torch.cuda.get_device_name(0), pieces=P, max_len=a.max_len, reps=a.reps, warmup=a.warmup,
               chars_mean=round(float(lengths.mean()), 1), generator="V1 shapes, synthetic weights")
    out["decode"], (_, post, gates, _) = series(decode)
    frames, _ = emitted_frames(gates, post.shape[1])
    assert frames == [a.max_len - 1] * P, frames
    out["frames"] = a.max_len - 1
    out["vocode_batched"], rows = series(lambda: gen(post.transpose(1, 2))[:, 0])
    n = [f * 256 for f in frames]
    buf = rows[:, :max(n)].contiguous()
    pause = [int(round(dict(sentence=0.25, clause=0.12, paragraph=0.6, end=0.0)[p.break_after] * sr)) for p in pieces]
    kw = dict(trim=True, top_db=60.0, frame_length=2048, hop_length=512, keep=441, fade=110)
    out["join_audio"], (y, total, _) = series(lambda: analysis.join_audio(buf, n, pause, **kw))
    out["join_audio_level"], _ = series(lambda: analysis.join_audio(buf, n, pause, level=True, ceiling=1.0, **kw))
    out["audio_seconds"] = round(total / sr, 2)
    mels = [post[k, :frames[k]].cpu().numpy() for k in range(P)]

    def parent_back_end():                     # do_say's HiFi-GAN branch: one generator call and one .cpu() per piece
        return [gen(torch.from_numpy(np.ascontiguousarray(m.T)).to(dev))[0, 0].cpu() for m in mels]
    out["vocode_per_piece_loop"], _ = series(parent_back_end)

    def parent_path():
        _, post, gates, _ = decode()
        host = post.cpu().numpy()
        valid = (gates.cpu().numpy()[:, :, 0] != -1000.0).sum(1)
        ms = [host[b, :max(min(int(valid[b]), host.shape[1] - 1), 1)] for b in range(P)]
        return [gen(torch.from_numpy(np.ascontiguousarray(m.T)).to(dev))[0, 0].cpu() for m in ms]
    out["parent_path"], _ = series(parent_path)
    out["document_path"], _ = series(lambda: say_document(model, pieces, enc, {}, gen, max_len=a.max_len)[0].cpu())
    med = lambda k: out[k]["ms_median"]
    out["join_us"] = round(med("join_audio") * 1e3, 1)
    out["join_share_of_vocoding"] = round(med("join_audio") / med("vocode_batched"), 5)
    out["document_over_parent_wall"] = round(out["document_path"]["wall_ms_median"] / out["parent_path"]["wall_ms_median"], 4)
    print(json.dumps(out), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
