"""One sha256 per output tensor of fixed-seed cases through the 16 entries of the model-free measurement kernels (t2_align, t2_dtw,
t2_join, t2_limit, t2_loudness, t2_pitch, t2_prosody, t2_psola, t2_resample, t2_stretch, t2_variance), through the C ABI only (_lib.make and
_lib.call), so that the same file runs against two builds of the library (T2_LIB_PATH selects one) and their outputs can be compared
bit for bit.  Every entry runs on a ragged batch of 3 and on a single row, with every optional output requested; outputs start as
zeros, so what a kernel leaves unwritten is the same in both builds.  The tables come from the package's host-side helpers.

    python tools/measurement_digest.py [--save OUT.pt] [--against OTHER.pt]

--save keeps the output tensors; --against prints, for every tensor whose bytes differ from the saved ones of another build, the
maximum absolute difference."""
import argparse
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tacotron2_amd import _lib  # noqa: E402
from tacotron2_amd.datasets.resample import plan  # noqa: E402
from tacotron2_amd.join import fade_table  # noqa: E402
from tacotron2_amd.loudness import ABS_GATE, k_weighting  # noqa: E402
from tacotron2_amd.psola import grain_table  # noqa: E402
from tacotron2_amd.stretch import hann_table  # noqa: E402

DEV = torch.device("cuda:0")
OUT = {}
SR, HOP, W, TAU_MIN, TAU_MAX = 22050, 256, 1024, 44, 367
K = _lib.K


def stream():
    return torch.cuda.current_stream().cuda_stream


def record(case, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        OUT[f"{case}.{name}"] = t.detach().cpu().contiguous()


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def voices(g, n):
    """len(n) rows of a gliding harmonic tone with a silent lead-in, an unvoiced (noise) stretch and a little noise throughout."""
    ld = max(n)
    t = torch.arange(ld, dtype=torch.float64)
    rows = []
    for b, nb in enumerate(n):
        f = (110.0 + 45.0 * b) * (1.0 + 0.15 * torch.sin(2 * math.pi * t / (0.9 * ld)))
        ph = 2 * math.pi * torch.cumsum(f, 0) / SR
        x = sum(torch.sin(h * ph) / h for h in (1, 2, 3, 4))
        x = 0.3 * x + 0.01 * torch.randn(ld, generator=g, dtype=torch.float64)
        x[: 700 + 100 * b] = 0.0
        x[nb // 2: nb // 2 + 1500] = 0.05 * torch.randn(1500, generator=g, dtype=torch.float64)[: ld - nb // 2]
        rows.append(x)
    return torch.stack(rows).float().to(DEV)


def pitch_chain(case, g, n):
    """yin -> prosody_stats -> voice_quality -> corpus_stats -> pitch_viterbi -> f0_path_stats (along a dtw path) -> psola."""
    B, ld = len(n), max(n)
    wav = voices(g, n)
    T, S, NT = 1 + ld // HOP, W + TAU_MAX, TAU_MAX + 1
    n64 = i64(n)
    f0, aper, power, cmnd = zeros(B, T), zeros(B, T), zeros(B, T), zeros(B, T, NT)
    _lib.call("t2_yin", _lib.make("T2Yin", wav=wav, ld_wav=ld, n=n64, B=B, n_max=ld, sr=SR, hop=HOP, W=W, tau_min=TAU_MIN, tau_max=TAU_MAX,
                                  thr=0.1, vthr=0.3, power_floor=1e-10, f0=f0, aper=aper, power=power, cmnd=cmnd), stream())
    record(f"{case}.yin", f0=f0, aper=aper, power=power, cmnd=cmnd)
    out = zeros(B, K["PROSODY_NSTAT"])
    _lib.call("t2_prosody_stats", _lib.make("T2ProsodyStats", f0=f0, aper=aper, power=power, n=n64, B=B, T=T, hop=HOP, S=S, out=out), stream())
    record(f"{case}.prosody_stats", out=out)
    jitter, shimmer, nhr, hnr = (zeros(B, T) for _ in range(4))
    cycles, cyc = zeros(B, T, dtype=torch.int32), zeros(B, T, K["VQ_MAX_CYCLES"], 3)
    _lib.call("t2_voice_quality", _lib.make("T2VoiceQuality", wav=wav, ld_wav=ld, n=n64, B=B, n_max=ld, sr=SR, hop=HOP, W=W, tau_min=TAU_MIN,
                                            tau_max=TAU_MAX, f0=f0, jitter=jitter, shimmer=shimmer, nhr=nhr, hnr_db=hnr, cycles=cycles,
                                            cyc=cyc), stream())
    record(f"{case}.voice_quality", jitter=jitter, shimmer=shimmer, nhr=nhr, hnr_db=hnr, cycles=cycles, cyc=cyc)
    out = zeros(B, K["CORPUS_NSTAT"])
    _lib.call("t2_corpus_stats", _lib.make("T2CorpusStats", f0=f0, power=power, jitter=jitter, shimmer=shimmer, nhr=nhr, hnr_db=hnr,
                                           cycles=cycles, n=n64, B=B, T=T, hop=HOP, S=S, power_floor=1e-10, out=out), stream())
    record(f"{case}.corpus_stats", out=out)
    N = TAU_MAX - TAU_MIN
    frames = i32([min(T, 1 + v // HOP) for v in n])
    lw = torch.log2(torch.arange(TAU_MIN, TAU_MAX, dtype=torch.float64)).to(DEV)
    vf0, vap, lag, cost = zeros(B, T), zeros(B, T), zeros(B, T, dtype=torch.int32), zeros(B, dtype=torch.float64)
    back = zeros(B, T, N + 1, dtype=torch.int16)
    _lib.call("t2_pitch_viterbi", _lib.make("T2PitchViterbi", cmnd=cmnd, ld_b=T * NT, ld_t=NT, power=power, len=frames, lw=lw, B=B, T=T,
                                            sr=SR, tau_min=TAU_MIN, tau_max=TAU_MAX, power_floor=1e-10, trans_max=0.25, u=0.3, c_sw=0.15,
                                            f0=vf0, aper=vap, lag=lag, cost=cost, back=back), stream())
    record(f"{case}.pitch_viterbi", f0=vf0, aper=vap, lag=lag, cost=cost)
    # the two tracks (yin's, and the decoded one cut three frames short) along the dtw path of two feature sequences of their lengths
    Ta, Tb, Kc = T, T - 3, 13
    fa, fb = torch.randn(B, Ta, Kc, generator=g).to(DEV), torch.randn(B, Tb, Kc, generator=g).to(DEV)
    la, lb = frames, (frames - 3).clamp(min=1)
    dcost, plen = zeros(B, dtype=torch.float64), zeros(B, dtype=torch.int32)
    dback, path = zeros(B, Ta, Tb, dtype=torch.uint8), zeros(B, Ta + Tb - 1, 2, dtype=torch.int32)
    _lib.call("t2_dtw", _lib.make("T2Dtw", a=fa, ld_ab=Ta * Kc, ld_at=Kc, b=fb, ld_bb=Tb * Kc, ld_bt=Kc, B=B, Ta=Ta, Tb=Tb, K=Kc, len_a=la,
                                  len_b=lb, scale=10.0 * math.sqrt(2.0) / math.log(10.0), cost=dcost, path_len=plen, back=dback, path=path),
              stream())
    record(f"{case}.dtw", cost=dcost, path_len=plen, path=path)
    out = zeros(B, K["F0_NSTAT"], dtype=torch.float64)
    _lib.call("t2_f0_path_stats", _lib.make("T2F0PathStats", path=path, path_len=plen, f0_a=f0, f0_b=vf0[:, :Tb].contiguous(), n_a=n64,
                                            n_b=i64([max(v - 3 * HOP, 0) for v in n]), B=B, P=Ta + Tb - 1, Ta=Ta, Tb=Tb, hop=HOP, S=S,
                                            out=out), stream())
    record(f"{case}.f0_path_stats", out=out)
    rho = torch.full((B, T), 55000, dtype=torch.int32, device=DEV)
    rho[:, ::3] = 80000
    ldy, ldm, lds = (ld + 63) // 64 * 64, ld // 12 + 2, ld // 3 + K["PSOLA_SYN_TAIL"]
    w = torch.from_numpy(grain_table()).to(DEV)
    y, a, r, kmap = zeros(B, ldy), zeros(B, ldm, dtype=torch.int32), zeros(B, lds, dtype=torch.int32), zeros(B, lds, dtype=torch.int32)
    n_marks, n_syn = zeros(B, dtype=torch.int32), zeros(B, dtype=torch.int32)
    _lib.call("t2_psola", _lib.make("T2Psola", x=wav, ldx=ld, n=i32(n), lag=lag, rho=rho, ldt=T, w=w, B=B, n_max=ld, T=T, hop=HOP,
                                    U=HOP // 2, y=y, ldy=ldy, a=a, ldm=ldm, r=r, kmap=kmap, lds=lds, n_marks=n_marks, n_syn=n_syn), stream())
    record(f"{case}.psola", y=y, a=a, r=r, kmap=kmap, n_marks=n_marks, n_syn=n_syn)
    return wav


def audio_chain(case, wav, n):
    """stretch, join, loudness (with the normalised copy), the limiter on that copy and resample of the same rows."""
    B, ld = len(n), max(n)
    n32 = i32(n)
    N, D, P, Q = 512, 128, 1250, 1000
    top = -((-ld * Q) // P)
    ldy, ldp = (top + 63) // 64 * 64, -(-top // (N // 2)) + 1
    y, pos, n_out = zeros(B, ldy), zeros(B, ldp, dtype=torch.int32), zeros(B, dtype=torch.int32)
    _lib.call("t2_stretch", _lib.make("T2Stretch", x=wav, ldx=ld, n=n32, w=torch.from_numpy(hann_table(N)).to(DEV), B=B, n_max=ld, N=N, D=D,
                                      P=P, Q=Q, y=y, ldy=ldy, pos=pos, ldp=ldp, n_out=n_out), stream())
    record(f"{case}.stretch", y=y, pos=pos, n_out=n_out)
    pause = [300 + 50 * b for b in range(B)]
    cap, F, H, fade = sum(n) + sum(pause), 2048, 512, 64
    lde = ld // H + 1
    energy, stat = zeros(B, lde, dtype=torch.float64), zeros(B, 2, dtype=torch.float64)
    off, s0, length = zeros(B, dtype=torch.int64), zeros(B, dtype=torch.int32), zeros(B, dtype=torch.int32)
    gain, total, y = zeros(B), zeros(1, dtype=torch.int64), zeros(cap)
    _lib.call("t2_join", _lib.make("T2Join", x=wav, ldx=ld, n=n32, pause=i32(pause), w=torch.from_numpy(fade_table(fade)).to(DEV), B=B,
                                   n_max=ld, trim=1, F=F, H=H, keep=100, fade=fade, level=1, top_db=40.0, max_gain=2.0, ceiling=0.25,
                                   energy=energy, lde=lde, stat=stat, off=off, s0=s0, len=length, gain=gain, total=total, y=y, cap=cap),
              stream())
    record(f"{case}.join", energy=energy, stat=stat, off=off, s0=s0, len=length, gain=gain, total=total, y=y)
    b1, a1, b2, a2 = k_weighting(SR)
    H = int(round(SR / 10))
    _, _, Kt, table = plan(SR, 4 * SR)
    lde = max(ld // H, 1)
    E, stat, gain, y = zeros(B, lde, dtype=torch.float64), zeros(B, K["LOUD_NSTAT"], dtype=torch.float64), zeros(B), zeros(B, ld)
    _lib.call("t2_loudness", _lib.make("T2Loudness", x=wav, ldx=ld, n=n32, table=torch.from_numpy(table).to(DEV), K=Kt, B=B, n_max=ld, H=H,
                                       b1=b1, a1=a1, b2=b2, a2=a2, abs_gate=ABS_GATE, target=-23.0, max_gain=10.0 ** 1.5,
                                       ceiling=10.0 ** (-1.0 / 20.0), E=E, lde=lde, stat=stat, gain=gain, y=y, ldy=ld), stream())
    record(f"{case}.loudness", E=E, stat=stat, gain=gain, y=y)
    env, curve, out, stat = zeros(B, ld), zeros(B, ld), zeros(B, ld), zeros(B, 8, dtype=torch.float64)      # a ceiling the copy passes often
    _lib.call("t2_limit", _lib.make("T2Limit", x=y, ldx=ld, n=n32, table=torch.from_numpy(table).to(DEV), K=Kt, B=B, n_max=ld, L=110,
                                    a=math.exp(-1.0 / (0.05 * SR)), ceiling=0.1, env=env, lde=ld, curve=curve, ldc=ld, y=out, ldy=ld, stat=stat),
              stream())
    record(f"{case}.limit", env=env, curve=curve, y=out, stat=stat)
    U, D, Kt, table = plan(SR, 16000)
    n_out = [-((-v * U) // D) for v in n]
    ldy = (max(n_out) + 63) // 64 * 64
    y = zeros(B, ldy)
    _lib.call("t2_resample", _lib.make("T2Resample", x=wav, ldx=ld, n_in=i64(n), y=y, ldy=ldy, n_out_max=max(n_out),
                                       table=torch.from_numpy(table).to(DEV), U=U, D=D, K=Kt, B=B), stream())
    record(f"{case}.resample", y=y)


def text_chain(case, g, chars, frames):
    """align_durations in both modes, char_variance on the monotonic durations, mel_cepstra."""
    B, L, S, M = len(chars), max(chars), max(frames), 80
    align = torch.softmax(3.0 * torch.randn(B, S, L, generator=g), dim=-1).to(DEV)
    clen, flen = i32(chars), i32(frames)
    for mode, tag in ((0, "argmax"), (1, "monotonic")):
        dur, stats = zeros(B, L, dtype=torch.int32), zeros(B, 4)
        back = zeros(B, S, L, dtype=torch.uint8) if mode else None
        _lib.call("t2_align_durations", _lib.make("T2AlignDur", align=align, ld_b=S * L, ld_s=L, B=B, S=S, L=L, r=1, mode=mode, chars_len=clen,
                                                  frames_len=flen, dur=dur, ld_dur=L, stats=stats, back=back), stream())
        record(f"{case}.align_durations.{tag}", dur=dur, stats=stats)
    f0 = (100.0 + 200.0 * torch.rand(B, S, generator=g)) * (torch.rand(B, S, generator=g) > 0.3)
    f0, mel = f0.float().to(DEV), (torch.randn(B, S, M, generator=g) - 3.0).to(DEV)
    for interpolate in (0, 1):
        cp, ce, cv = zeros(B, L), zeros(B, L), zeros(B, L, dtype=torch.int32)
        fp, fe, stats = zeros(B, S), zeros(B, S), zeros(B, K["VAR_NSTAT"], dtype=torch.float64)
        _lib.call("t2_char_variance", _lib.make("T2CharVariance", f0=f0, ld_f0=S, mel=mel, ld_b=S * M, ld_t=M, dur=dur, ld_dur=L, B=B, T=S, L=L,
                                                M=M, log_pitch=1, interpolate=interpolate, chars_len=clen, frames_len=flen, char_pitch=cp,
                                                char_energy=ce, char_voiced=cv, frame_pitch=fp, frame_energy=fe, stats=stats), stream())
        record(f"{case}.char_variance.interpolate{interpolate}", char_pitch=cp, char_energy=ce, char_voiced=cv, frame_pitch=fp, frame_energy=fe,
               stats=stats)
    Kc = 13
    m = torch.arange(M, dtype=torch.float64).view(M, 1) + 0.5
    k = torch.arange(1, Kc + 1, dtype=torch.float64).view(1, Kc)
    basis = (math.sqrt(2.0 / M) * torch.cos(math.pi * k * m / M)).float().to(DEV)
    out = zeros(B, S, Kc)
    _lib.call("t2_mel_cepstra", _lib.make("T2MelCeps", mel=mel, ld_b=S * M, ld_t=M, B=B, T=S, M=M, K=Kc, len=flen, basis=basis, out=out,
                                          ld_ob=S * Kc, ld_ot=Kc), stream())
    record(f"{case}.mel_cepstra", out=out)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--save")
    ap.add_argument("--against")
    args = ap.parse_args()
    for case, n, chars, frames in (("batch3", [23000, 9000, 15500], [37, 130, 70], [300, 150, 211]), ("single", [11000], [41], [97])):
        g = torch.Generator().manual_seed(7000 + len(n))
        wav = pitch_chain(case, g, n)
        audio_chain(case, wav, n)
        text_chain(case, g, chars, frames)
    other = torch.load(args.against) if args.against else None
    differ = []
    for name, t in OUT.items():
        line = f"{hashlib.sha256(t.numpy().tobytes()).hexdigest()}  {name}  {str(t.dtype)[6:]}{tuple(t.shape)}  {int(t.count_nonzero())} non-zero"
        if other is not None and name in other and not same(other[name], t):      # (an entry the other build lacks is not compared)
            differ.append(name)
            line += f"  DIFFERS: max abs difference {float((other[name].double() - t.double()).abs().nan_to_num(nan=0.0).max()):.3e}"
        print(line)
    if other is not None:
        print("# tensors that differ from", os.path.basename(args.against), ":", differ or "none")
    if args.save:
        torch.save(OUT, args.save)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
