"""Pitch change of a padded batch of waveforms at their own length and with their own formants: TD-PSOLA as one call
into libtacotron2_amd.so (C-ABI t2_psola) on the current stream, the pitch marks placed from pitch_viterbi's integer lags.
analysis.psola, analysis.pitch_ratio and analysis.pitch_shift_psola ARE this module's functions: they need no model, and their
arguments are checked by _args before a pointer reaches a kernel."""
from __future__ import annotations

import contextlib
import math

import torch

from . import _args
from ._lib import K, cached, call, make, stream
from .stretch import MAX_SAMPLES, SEMITONE_RANGE

LAG_RANGE = (K["PSOLA_MIN_LAG"], K["PSOLA_MAX_LAG"])      # voiced lags, and the unvoiced spacing
RHO_ONE = 65536                             # Q16
RHO_RANGE = (K["PSOLA_MIN_RHO"], K["PSOLA_MAX_RHO"])      # 1/4 .. 4
SYN_TAIL = K["PSOLA_SYN_TAIL"]
PITCH_RANGE_RANGE = (0.0, 2.0)


def grain_table():
    """The rising half of a Hann window on 1025 points, float32 from fp64: W[u] = 0.5 - 0.5 cos(pi u / 1024), so that
    W[u] + W[1024 - u] = 1.  A host (numpy) array; psola uploads it once per device."""
    import numpy as np
    return (0.5 - 0.5 * np.cos(np.pi * np.arange(1025, dtype=np.float64) / 1024.0)).astype(np.float32)


def _rows(fn: str, name: str, x, B: int, T, dev):
    """x an int32 (B, T) tensor on dev with a contiguous last dimension and rows that do not overlap; (T, its row stride)."""
    _args.tensor_arg(fn, name, x, 2, "(B, T)", torch.int32)
    _args.on_device(fn, name, x, dev)
    if x.shape[0] != B or x.shape[1] < 1 or (T is not None and x.shape[1] != T):
        raise ValueError(f"{fn}: {name} must be ({B}, {'T >= 1' if T is None else T}), got {tuple(x.shape)}")
    return x.shape[1], _args.row_stride(fn, name, x, "frames")


def psola(wav, n, lag, rho, hop=256, unvoiced=None):
    """A padded batch with its pitch periods rescaled, frame by frame, at unchanged length (C-ABI t2_psola): wav (B, ld)
    float32 on the GPU (a strided view with a contiguous last dimension will do), n the B sample counts, 0 <= n[b] <= ld; lag (B, T)
    int32 the pitch period in samples at frame t, centred on sample t * hop, 0 = unvoiced, as pitch_viterbi gives it (16 .. 4096 where
    voiced); rho the output period over the input period in Q16 (65536 = unchanged, 16384 .. 262144 where voiced): a (B, T) int32
    tensor, or one Python integer for every frame.  hop >= 16; `unvoiced` (16 .. 4096, default hop // 2) is the spacing of the marks
    where there is no pitch.
    Returns (y (B, ld') float32 with zeros behind each row's n[b] samples, marks): marks = dict(a (B, M) int32 - the analysis marks,
    the last one n[b] -, r and kmap (B, S) int32 - the synthesis marks and the analysis mark each one copies -, n_marks and n_syn
    (B,) int32 - the entries of a, and of r and kmap; zeros behind them).  n as host integers keeps the call free of host reads; a
    tensor on the GPU is checked by the kernel.  A row with a count, a lag or a rho out of range is refused on the device: its
    n_marks is -1 and nothing else is written for it - with host counts nothing is read back, so look at n_marks when the lags are not
    pitch_viterbi's.  Needs no model."""
    fn = "psola"
    B, ld, ldx = _args.wav_rows(fn, "wav", wav, MAX_SAMPLES)
    dev = wav.device
    hop = _args.int_arg(fn, "hop", hop, 16, 1 << 20)
    U = _args.int_arg(fn, "unvoiced", hop // 2 if unvoiced is None else unvoiced, *LAG_RANGE)
    n32, n_sum = _args.counts32(fn, "n", n, B, dev, hi=ld)
    _args.on_gpu(fn, "wav", wav)
    T, ldt = _rows(fn, "lag", lag, B, None, dev)
    if torch.is_tensor(rho):
        _, ldr = _rows(fn, "rho", rho, B, T, dev)
        if ldr != ldt:
            rho, lag = rho.contiguous(), lag.contiguous()
            ldt = T
    else:
        q = _args.int_arg(fn, "rho", rho, *RHO_RANGE)
    n_max = ld if n_sum is None else max(int(v) for v in n)
    ldy, ldm, lds = (n_max + 63) // 64 * 64, n_max // 12 + 2, n_max // 3 + SYN_TAIL
    with torch.cuda.device(dev):
        if not torch.is_tensor(rho):
            rho = torch.full((B, ldt), q, dtype=torch.int32, device=dev)
        w = cached(("grain", dev), lambda: torch.from_numpy(grain_table()).to(dev))
        y = torch.empty(B, ldy, dtype=torch.float32, device=dev)
        a = torch.empty(B, ldm, dtype=torch.int32, device=dev)
        r, kmap = (torch.empty(B, lds, dtype=torch.int32, device=dev) for _ in range(2))
        n_marks, n_syn = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        args = make("T2Psola", x=wav if ld > 0 else None, ldx=ldx, n=n32, lag=lag, rho=rho, ldt=ldt, w=w, B=B, n_max=n_max, T=T, hop=hop,
                    U=U, y=y if ldy > 0 else None, ldy=ldy, a=a, ldm=ldm, r=r, kmap=kmap, lds=lds, n_marks=n_marks, n_syn=n_syn)
        call("t2_psola", args, stream())
    return y, dict(a=a, r=r, kmap=kmap, n_marks=n_marks, n_syn=n_syn)


def shift_args(fn: str, semitones, pitch_range):
    """(semitones, pitch_range) as floats: -24 .. 24 and 0 .. 2."""
    semitones, pitch_range = _args.real_arg(fn, "semitones", semitones), _args.real_arg(fn, "pitch_range", pitch_range)
    if not SEMITONE_RANGE[0] <= semitones <= SEMITONE_RANGE[1]:
        raise ValueError(f"{fn}: semitones must lie in {SEMITONE_RANGE[0]:g} .. {SEMITONE_RANGE[1]:g}, got {semitones!r}")
    if not PITCH_RANGE_RANGE[0] <= pitch_range <= PITCH_RANGE_RANGE[1]:
        raise ValueError(f"{fn}: pitch_range must lie in {PITCH_RANGE_RANGE[0]:g} .. {PITCH_RANGE_RANGE[1]:g}, got {pitch_range!r}")
    return semitones, pitch_range


def pitch_ratio(lag, n, semitones=0.0, pitch_range=1.0, hop=256):
    """The rho of psola for a shift by `semitones` (-24 .. 24) and an intonation range scaled by `pitch_range` (0 .. 2; 0 is a monotone
    voice at the row's mean pitch, 1 unchanged) about the row's mean log pitch: lag (B, T) int32 on the GPU as pitch_viterbi gives it,
    n the B sample counts (host integers or a tensor on lag's device) - the frames t < min(T, 1 + n[b] // hop) count.  With f = 1 /
    lag and m the mean of ln f over the row's voiced frames, rho = exp((1 - pitch_range) (ln f - m) - semitones ln 2 / 12) in float64
    on the device, rounded to Q16 and clipped to 16384 .. 262144; 65536 at unvoiced frames and behind the row's frames.  With
    pitch_range == 1 every voiced frame gets the ONE integer round(65536 * 2^(-semitones / 12)) formed by the host, so a plain shift
    is reproducible to the bit.  Returns (B, T) int32; nothing is read back.  Needs no model."""
    fn = "pitch_ratio"
    _args.tensor_arg(fn, "lag", lag, 2, "(B, T)", torch.int32)
    B, T = lag.shape
    _args.batch_arg(fn, B)
    if T < 1:
        raise ValueError(f"{fn}: lag must have at least one frame")
    semitones, pitch_range = shift_args(fn, semitones, pitch_range)
    hop = _args.int_arg(fn, "hop", hop, 1)
    dev = lag.device
    n32, _ = _args.counts32(fn, "n", n, B, dev)
    _args.on_gpu(fn, "lag", lag)
    with torch.cuda.device(dev):
        frames = (1 + torch.div(n32.to(torch.int64).clamp(min=0), hop, rounding_mode="floor")).clamp(max=T)
        voiced = (lag > 0) & (torch.arange(T, device=dev)[None, :] < frames[:, None])
        if pitch_range == 1.0:
            q = int(round(RHO_ONE * math.pow(2.0, -semitones / 12.0)))
            return torch.where(voiced, q, RHO_ONE).to(torch.int32)
        lf = torch.where(voiced, -torch.log(lag.clamp(min=1).to(torch.float64)), 0.0)
        m = lf.sum(1, keepdim=True) / voiced.sum(1, keepdim=True).clamp(min=1)
        rho = torch.exp((1.0 - pitch_range) * (lf - m) - semitones * math.log(2.0) / 12.0)
        q = torch.round(rho * RHO_ONE).clamp(*RHO_RANGE).to(torch.int32)
        return torch.where(voiced, q, RHO_ONE).to(torch.int32)


FOLD_MAX = 8                                # sub-multiples tried by fold_lags: tau_max / tau_min of the default meter is 8.3


def fold_lags(cmnd, lag, tau_min, thr=0.1):
    """pitch_viterbi's lags brought down to the pitch period itself.  The decode's local cost is yin's normalised difference alone,
    which on a steady voice is as small at two or three periods as at one - nothing in it prefers the shorter lag - and a mark every
    second period makes grains of two pulses.  So every voiced lag L takes the smallest of its sub-multiples that YIN's own threshold
    accepts: for m = 8 .. 2 in turn, c = (L + m // 2) // m, and the first m at which the smallest cmnd over the lags c - 1, c, c + 1
    inside [tau_min, tau_max) lies under `thr` takes that lag (the first of equal minima); L stays where no m does.  cmnd (B, T,
    tau_max + 1) float32 and lag (B, T) int32 as yin(return_cmnd=True) and pitch_viterbi give them.  Returns (B, T) int32; comparisons
    of stored floats and integer arithmetic only, so tests/psola_ref.py's fold_lags gives the same lags.  Needs no model."""
    fn = "fold_lags"
    _args.tensor_arg(fn, "cmnd", cmnd, 3, "(B, T, tau_max + 1)")
    B, T, NT = cmnd.shape
    _args.tensor_arg(fn, "lag", lag, 2, "(B, T)", torch.int32)
    if lag.shape != (B, T) or lag.device != cmnd.device:
        raise ValueError(f"{fn}: lag must be ({B}, {T}) on {cmnd.device}, got {tuple(lag.shape)} on {lag.device}")
    tau_min = _args.int_arg(fn, "tau_min", tau_min, 2, NT - 2)
    thr = _args.real_arg(fn, "thr", thr)
    tau_max = NT - 1
    with torch.cuda.device(cmnd.device) if cmnd.device.type == "cuda" else contextlib.nullcontext():
        L = lag.to(torch.int64)
        out, done = L.clone(), L <= 0
        big = torch.full((), float("inf"), dtype=cmnd.dtype, device=cmnd.device)
        for m in range(FOLD_MAX, 1, -1):
            c = torch.div(L + m // 2, m, rounding_mode="floor")
            cand = torch.stack([c - 1, c, c + 1], dim=-1)                                   # (B, T, 3)
            ok = (cand >= tau_min) & (cand < tau_max)
            v = torch.where(ok, torch.gather(cmnd, 2, cand.clamp(0, tau_max)), big)
            best = v.min(dim=-1).values
            first = (v == best[..., None]).to(torch.int64).argmax(dim=-1)                   # the first of equal minima
            take = ~done & (best < thr)
            out = torch.where(take, torch.gather(cand, 2, first[..., None])[..., 0], out)
            done = done | take
        return out.to(torch.int32)


def default_meter(sample_rate: int, dev):
    """The prosody.ProsodyMeter(sample_rate, dev, smooth=True) pitch_shift_psola tracks with, made once per rate and device."""
    from .prosody import ProsodyMeter
    return cached(("meter", int(sample_rate), dev), lambda: ProsodyMeter(int(sample_rate), dev, smooth=True))


def check_meter(fn: str, meter) -> None:
    """What psola needs of a meter: Viterbi smoothing (integer lags), a hop of at least 16, lags inside 16 .. 4096."""
    if not getattr(meter, "smooth", False):
        raise ValueError(f"{fn}: the meter must be a ProsodyMeter(smooth=True): the marks are placed from pitch_viterbi's integer lags")
    if meter.settings["hop"] < 16 or meter.tau_min < LAG_RANGE[0] or meter.tau_max - 1 > LAG_RANGE[1]:
        raise ValueError(f"{fn}: the meter's hop {meter.settings['hop']} and lags {meter.tau_min} .. {meter.tau_max - 1} must be a hop >= 16 "
                         f"and lags inside {LAG_RANGE[0]} .. {LAG_RANGE[1]}")


def check_rate(fn: str, sample_rate: int) -> None:
    """check_meter for the default meter at sample_rate, without making one."""
    from .analysis import YIN_DEFAULTS
    tau_min, tau_max = _args.lags(fn, int(sample_rate), YIN_DEFAULTS["fmin"], YIN_DEFAULTS["fmax"])
    if YIN_DEFAULTS["hop"] < 16 or tau_min < LAG_RANGE[0] or tau_max - 1 > LAG_RANGE[1]:
        raise ValueError(f"{fn}: at {sample_rate} Hz the pitch tracker's lags {tau_min} .. {tau_max - 1} leave {LAG_RANGE[0]} .. "
                         f"{LAG_RANGE[1]}, the periods a pitch mark can follow")


def track_lags(meter, wav, n_dev, n_max: int):
    """The integer pitch periods pitch_shift_psola places its marks from: the meter's yin(return_cmnd=True) and pitch_viterbi - the
    two pitch-tracking launches - and fold_lags under the meter's YIN threshold.  wav (B, ld) float32 on the GPU, n_dev the counts
    as an int64 tensor there.  (B, 1 + n_max // hop) int32, 0 = unvoiced."""
    from . import analysis
    s = meter.settings
    _, _, power, cmnd = analysis.yin(wav, n_dev, n_max=n_max, return_cmnd=True, **s)
    _, _, lag, _ = analysis.pitch_viterbi(cmnd, power, n_dev, sr=s["sr"], hop=s["hop"], fmin=s["fmin"], fmax=s["fmax"],
                                          power_floor=s["power_floor"], **meter.viterbi)
    return fold_lags(cmnd, lag, meter.tau_min, s["thr"])


def check_frames(fn: str, n_max: int, hop: int) -> None:
    from .analysis import PROSODY_MAX_T
    if 1 + n_max // hop > PROSODY_MAX_T:
        raise ValueError(f"{fn}: a row of {n_max} samples has more than {PROSODY_MAX_T} frames (T2_PROSODY_MAX_T)")


def pitch_shift_psola(wav, n, semitones, sample_rate, pitch_range=1.0, tempo=1.0, meter=None, frame=1024, tolerance=256):
    """A padded batch raised by `semitones` (-24 .. 24), its intonation range scaled by `pitch_range` (0 .. 2) and played at `tempo`
    times its speed (0.25 .. 4), the formants where they were: time_stretch if the tempo is not 1 (with `frame` and `tolerance`), then on
    the stretched signal track_lags - the meter's yin(return_cmnd=True) and pitch_viterbi, then fold_lags -, pitch_ratio and psola.
    Nothing is resampled, so the counts are the stretch's.  wav and n as time_stretch takes them; meter: a
    prosody.ProsodyMeter(smooth=True) at sample_rate (None: its defaults) - a row of more than T2_PROSODY_MAX_T frames is refused, as
    the meter refuses it.  The output's RMS is 0.66 .. 0.95 of the input's on synthetic vowels.
    Returns (y (B, ld') float32, n_out host integers, the effective tempo); with semitones == 0 and pitch_range == 1 nothing of the
    PSOLA path is launched and time_stretch's result comes back - at tempo 1, wav itself."""
    from . import voice
    plan = voice.plan_voice("pitch_shift_psola", sample_rate, tempo, semitones, pitch_range, True, frame, tolerance)
    y, counts = voice.run_voice(plan, wav, n, meter)
    return y, counts, plan.tempo
