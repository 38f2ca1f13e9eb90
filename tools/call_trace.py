"""Call trace of the engine: every library call that goes through tacotron2_amd.engine.call and every cross-stream edge
(Engine._record / Engine._wait), in enqueue order, per stream.  For host-side changes of the engine that must not move a launch:
run it in a checkout of the commit before the change and in one of the change, then `diff` the two files.

    python tools/call_trace.py --cases A,B,C,D,E,F --out trace.txt [--tree OTHER_CHECKOUT]

The tracer needs nothing but those three names, so the same file traces any checkout (--tree: the checkout whose package is
imported; default: the one this file sits in).  Logged per call: the stream (main = the stream current when tracing starts,
side = the engine's side stream, anything else s1, s2, ... in order of appearance) and
  t2_gemm                     M, N, K, splitk, accumulate, share_cu, batch
  t2_attn_seq_fwd / _bwd*     the frame range (t_begin / t_end, t_hi / t_lo); t2_attn_acc_bwd: its t_begin, t_end arguments
  t2_lstm_seq_*               cells and steps
  t2_zero_regions             regions and bytes
Events are numbered in the order they are recorded; a wait names the event (and the stream it was recorded on) or the stream.
Stdout: counts per (stream, call) and the edge / zero-list totals of every case; --out: the full per-stream sequences."""
import argparse
import collections
import contextlib
import os
import sys


class Tracer:
    def __init__(self, engine):
        self.engine = engine
        self.log = []              # (stream name, text) in enqueue order
        self.zero = [0, 0, 0]      # t2_zero_regions: launches, regions, bytes
        self._names = {}
        self._events = {}          # id(event) -> (event, number, stream name); the event is kept so that the id stays its own

    def name(self, handle):
        side = self.engine._side
        if side is not None and handle == side.cuda_stream:
            return "side"
        if handle not in self._names:
            self._names[handle] = f"s{len(self._names)}"
        return self._names[handle]

    def describe(self, name, args):
        a = args[0] if args else None
        if name == "t2_gemm":
            return (f"M={a.M} N={a.N} K={a.K} splitk={a.splitk} accumulate={a.accumulate} share_cu={a.share_cu} batch={a.batch}")
        if name == "t2_attn_seq_fwd":
            return f"t_begin={a.t_begin} t_end={a.t_end}"
        if name == "t2_attn_acc_bwd":
            return f"t_begin={args[3]} t_end={args[4]}"
        if name.startswith("t2_attn_seq_bwd"):
            return f"t_hi={a.t_hi} t_lo={a.t_lo}"
        if name.startswith("t2_lstm_seq_"):      # (the entries the engine calls: base, inc, n, S, ...)
            return f"n={args[2]} S={args[3]}"
        if name == "t2_zero_regions":
            nbytes = sum(a.row_bytes[i] * a.nrows[i] for i in range(a.n))
            self.zero[0] += 1; self.zero[1] += a.n; self.zero[2] += nbytes
            return f"regions={a.n} bytes={nbytes}"
        return ""

    @contextlib.contextmanager
    def tracing(self):
        import torch
        from tacotron2_amd import engine as E
        self._names = {torch.cuda.current_stream().cuda_stream: "main"}
        real_call, real_record, real_wait = E.call, E.Engine.__dict__["_record"], E.Engine.__dict__["_wait"]

        def call(name, *args):       # (every entry of include/tacotron2_amd.h takes its stream as the LAST argument)
            E.flush_zeros()        # what the hook in front of the real call would enqueue first is logged first
            self.log.append((self.name(args[-1]), f"{name} {self.describe(name, args)}".rstrip()))
            return real_call(name, *args)

        def record(stream):
            E.flush_zeros()
            ev = real_record.__func__(stream)
            s = self.name(stream.cuda_stream)
            self._events[id(ev)] = (ev, len(self._events), s)
            self.log.append((s, f"record ev{len(self._events) - 1}"))
            return ev

        def wait(stream, other):
            E.flush_zeros()
            if isinstance(other, torch.cuda.Event):
                _, n, s = self._events.get(id(other), (None, "?", "?"))
                what = f"ev{n}({s})"
            else:
                what = f"stream {self.name(other.cuda_stream)}"
            self.log.append((self.name(stream.cuda_stream), f"wait {what}"))
            return real_wait.__func__(stream, other)
        E.call, E.Engine._record, E.Engine._wait = call, staticmethod(record), staticmethod(wait)
        try:
            yield self
        finally:
            E.call, E.Engine._record, E.Engine._wait = real_call, real_record, real_wait

    def counts(self):
        return collections.Counter((s, text.split(" ")[0]) for s, text in self.log)

    def sequences(self):
        seqs = collections.OrderedDict()
        for s, text in self.log:
            seqs.setdefault(s, []).append(text)
        return seqs


# ---- the cases ---------------------------------------------------------------------------------------------------------------
BENCH = dict(num_chars=39, encoded_dim=512, encoder_kernel_size=5, num_mels=80, prenet_dim=256, att_rnn_dim=1024, att_dim=128,
             rnn_hidden_dim=1024, postnet_dim=512, dropout=0.5, speaker_tokens=True, num_speakers=4,
             description_embeddings=False, description_embeddings_dim=0)
SMALL = dict(num_chars=39, encoded_dim=64, encoder_kernel_size=5, num_mels=16, prenet_dim=32, att_rnn_dim=64, att_dim=32,
             rnn_hidden_dim=64, postnet_dim=64, dropout=0.5, speaker_tokens=False, num_speakers=1,
             description_embeddings=False, description_embeddings_dim=0)
CASES = collections.OrderedDict([
    ("A", dict(title="Trainer.train_step, bench dims, ljspeech_batch(32, seed=1234, num_speakers=4), third step", bench=True)),
    ("B", dict(title="small dims, B=5, L=17, T=23, chunk=8, chunk_bwd=5, dec_chain='steps'", B=5, L=17, T=23,
               engine=dict(chunk=8, chunk_bwd=5, dec_chain="steps"))),
    ("C", dict(title="small dims, B=5, L=17, T=150, chunk=chunk_bwd=16 (in-loop group flushes, the ramp)", B=5, L=17, T=150,
               engine=dict(chunk=16, chunk_bwd=16))),
    ("D", dict(title="small dims, B=3, L=300 (no stash), T=40, chunk_bwd=8", B=3, L=300, T=40, engine=dict(chunk_bwd=8))),
    ("E", dict(title="small dims, B=5, L=17, T=1", B=5, L=17, T=1)),
    ("F", dict(title="small dims, B=5, L=17, T=23, chunk_bwd=5, forward attention, controls, guided attention (0.4, 1.0)",
               B=5, L=17, T=23, engine=dict(chunk_bwd=5), dims=dict(controls=True, controls_dim=5),
               trainer=dict(forward_attention=True, guided_attention=(0.4, 1.0)))),
])


def small_batch(dims, B, L, T, seed=77):
    """Ragged lengths with the maxima present (the first text is L long, the last utterance T frames)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(min(max(3, L // 2), L), L + 1, (B,), generator=g); lens[0] = L
    tl = torch.randint(min(max(1, T // 2), T), T + 1, (B,), generator=g); tl[-1] = T
    M = dims["num_mels"]
    ci = torch.zeros(B, L, dtype=torch.int64); mel = torch.zeros(B, T, M); gate = torch.zeros(B, T, 1)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, dims["num_chars"] + 1, (int(lens[b]),), generator=g)
        mel[b, :tl[b]] = torch.randn(int(tl[b]), M, generator=g) * 1.5 - 3
        gate[b, :tl[b] - 1] = 1.0
    out = dict(chars_idx=ci, chars_idx_len=lens, mel_spectrogram=mel, mel_spectrogram_len=tl.to(torch.int32), gate=gate)
    if dims.get("controls"):
        out["controls"] = torch.randn(B, dims["controls_dim"], generator=g)
    return out


def run_case(key, steps=3):
    """`steps` optimisation steps of the case on a fresh trainer, the last one traced."""
    import torch
    from tacotron2_amd.init import init_parameters
    from tacotron2_amd.params import ParamStore
    from tacotron2_amd.synthetic import ljspeech_batch
    from tacotron2_amd.trainer import Trainer
    case = CASES[key]
    dev = torch.device("cuda", 0)
    dims = dict(BENCH if case.get("bench") else SMALL, **case.get("dims", {}))
    ps = ParamStore(dims, dev)
    init_parameters(ps, seed=0)
    tr = Trainer(ps, lr=1e-3, weight_decay=1e-6, **case.get("trainer", {}))
    for k, v in case.get("engine", {}).items():
        assert hasattr(tr.engine, k), k
        setattr(tr.engine, k, v)
    if case.get("bench"):
        batch = ljspeech_batch(32, seed=1234, num_speakers=4)
    else:
        batch = small_batch(dims, case["B"], case["L"], case["T"])
    batch = {k: v.to(dev) for k, v in batch.items()}
    for _ in range(steps - 1):
        tr.train_step(batch, padded=True)
    torch.cuda.synchronize()
    tracer = Tracer(tr.engine)
    with tracer.tracing():
        loss3, _ = tr.train_step(batch, padded=True)
    torch.cuda.synchronize()
    tr.engine.check_persistent_kernels()
    assert bool(torch.isfinite(loss3).all()), f"case {key}: loss {loss3.tolist()}"
    return tracer


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ",".join(CASES))
    ap.add_argument("--out", required=True, help="file for the full per-stream sequences")
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                    help="the checkout whose tacotron2_amd package is traced")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import tacotron2_amd  # noqa: F401  (first: the package pins the hardware-queue count before the HIP runtime starts)
    with open(args.out, "w") as f:
        for key in args.cases.split(","):
            tracer = run_case(key)
            title = f"## {key}  {CASES[key]['title']}"
            print(title)
            for (s, name), n in sorted(tracer.counts().items()):
                print(f"   {s:<6} {name:<34} {n:>6}")
            z = tracer.zero
            print(f"   total: {len(tracer.log)} entries; t2_zero_regions launches={z[0]} regions={z[1]} bytes={z[2]}", flush=True)
            f.write(title + "\n")
            for s, seq in tracer.sequences().items():
                f.write(f"# {key} stream {s}: {len(seq)} entries\n")
                f.writelines(f"{key} {s:<5} {text}\n" for text in seq)


if __name__ == "__main__":
    main()
