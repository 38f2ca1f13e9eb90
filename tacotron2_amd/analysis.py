"""The audio measurements that need no model: pitch tracking, voice quality, their per-utterance
statistics, resampling, joining, time stretching, pitch change and loudness, each one call into libtacotron2_amd.so on the current stream.  The arguments are checked by _args before
a pointer reaches a kernel.  engine re-exports every public name of this module: engine.yin is analysis.yin."""
from __future__ import annotations

import math

import torch

from . import _args
from ._args import YIN_MAX_SPAN
from ._lib import K, cached, call, make, stream
# per-character pitch and energy on the duration grid: analysis.char_variance, written in variance.py
from .join import fade_table, join_audio  # noqa: F401  (pieces joined into one waveform, DESIGN 5.16: analysis.join_audio, in join.py)
from .stretch import hann_table, pitch_shift, time_stretch  # noqa: F401  (WSOLA tempo and pitch, DESIGN 5.17: in stretch.py)
from .psola import fold_lags, grain_table, pitch_ratio, pitch_shift_psola, psola  # noqa: F401  (TD-PSOLA pitch change, DESIGN 5.18: in psola.py)
from .loudness import k_weighting, loudness, normalize_loudness  # noqa: F401  (BS.1770 loudness and true peak, DESIGN 5.20: in loudness.py)
from .limiter import limit_peaks  # noqa: F401  (look-ahead true-peak limiter, DESIGN 5.21: in limiter.py)
from .denoise import denoise, stft_magnitudes, vocoder_bias  # noqa: F401  (vocoder-bias spectral subtraction, DESIGN 5.22: in denoise.py)
from .variance import VAR_MAX_L, VAR_MAX_T, VAR_NSTAT, VAR_STATS, char_variance  # noqa: F401

PROSODY_MAX_T = K["PROSODY_MAX_T"]        # frames of one utterance in t2_prosody_stats
PROSODY_NSTAT = K["PROSODY_NSTAT"]
YIN_DEFAULTS = dict(sr=22050, hop=256, W=1024, fmin=60.0, fmax=500.0, thr=0.1, vthr=0.3, power_floor=1e-10)


def _check_frames(fn: str, T: int) -> None:
    if T < 1 or T > PROSODY_MAX_T:
        raise ValueError(f"{fn}: {T} frames, outside 1 .. {PROSODY_MAX_T} (T2_PROSODY_MAX_T)")


def yin_lags(sr: int, fmin: float, fmax: float):
    """(tau_min, tau_max) of a pitch range in Hz: sr // fmax and sr // fmin (22050, 60, 500 -> 44, 367)."""
    return _args.lags("yin", sr, fmin, fmax)


def yin(wav, n, sr=22050, hop=256, W=1024, fmin=60.0, fmax=500.0, thr=0.1, vthr=0.3, power_floor=1e-10, n_max=None,
        return_cmnd=False):
    """The YIN pitch tracker on the mel grid (C-ABI t2_yin) of a padded batch wav (B, ld) float32 on the GPU with the
    sample counts n (B,) integers on the same device: (f0 Hz, aperiodicity, power), each (B, T) float32 with T = 1 + n_max // hop,
    and the normalised difference (B, T, tau_max + 1) with return_cmnd.  n_max (default: ld) is the largest count; nothing at or
    behind n[b] is read.  Frame t is centred on sample t * hop and needs W + tau_max samples around it: a frame whose span leaves
    [0, n[b]) is invalid and comes back as f0 0, aperiodicity 1, power 0; f0 is 0 for an unvoiced frame.  Needs no model."""
    B, ld_wav, n_max, n64, T, tau_min, tau_max = _args.padded_wav("yin", wav, n, n_max, sr, hop, W, fmin, fmax)
    thr, vthr, power_floor = (_args.real_arg("yin", k, v) for k, v in (("thr", thr), ("vthr", vthr), ("power_floor", power_floor)))
    with torch.cuda.device(wav.device):
        f0, aper, power = (torch.empty(B, T, dtype=torch.float32, device=wav.device) for _ in range(3))
        cmnd = torch.empty(B, T, tau_max + 1, dtype=torch.float32, device=wav.device) if return_cmnd else None
        a = make("T2Yin", wav=wav, ld_wav=ld_wav, n=n64, B=B, n_max=n_max, sr=sr, hop=hop, W=W, tau_min=tau_min, tau_max=tau_max,
                 thr=thr, vthr=vthr, power_floor=power_floor, f0=f0, aper=aper, power=power, cmnd=cmnd)
        call("t2_yin", a, stream())
    return (f0, aper, power, cmnd) if return_cmnd else (f0, aper, power)


def prosody_stats(f0, aper, power, n, hop=256, span=1024 + 367):
    """Per-utterance statistics (C-ABI t2_prosody_stats) of yin's (B, T) outputs, with n, hop and span = W + tau_max of that call:
    (B, 8) float32 rows [valid frames, voiced frames, mean ln f0, p5 Hz, p95 Hz, mean 10 log10 power, mean aperiodicity, 0], means
    and percentiles over the voiced frames (NaN without one); the percentiles are elements of the track, nearest rank."""
    B, T = _args.same_shape_2d("prosody_stats", (("f0", f0), ("aper", aper), ("power", power)))
    _args.batch_arg("prosody_stats", B)
    _check_frames("prosody_stats", T)
    _args.int_arg("prosody_stats", "hop", hop, 1)
    _args.int_arg("prosody_stats", "span", span, 1)
    n64 = _args.lengths("prosody_stats", "n", n, B, f0.device).to(torch.int64).contiguous()
    with torch.cuda.device(f0.device):
        out = torch.empty(B, PROSODY_NSTAT, dtype=torch.float32, device=f0.device)
        a = make("T2ProsodyStats", f0=f0, aper=aper, power=power, n=n64, B=B, T=T, hop=hop, S=span, out=out)
        call("t2_prosody_stats", a, stream())
    return out


VQ_MAX_CYCLES = K["VQ_MAX_CYCLES"]        # cycles matched per frame in t2_voice_quality
CORPUS_NSTAT = K["CORPUS_NSTAT"]


def voice_quality(wav, n, f0, sr=22050, hop=256, W=1024, fmin=60.0, fmax=500.0, n_max=None, return_cycles=False):
    """Jitter, shimmer and harmonicity per frame by cycle matching (C-ABI t2_voice_quality): wav (B, ld) float32, n (B,)
    and n_max as yin takes them, with the same sr, hop, W, fmin, fmax, and f0 (B, T) float32 - yin's track or pitch_viterbi's, 0 =
    unvoiced.  A valid frame (yin's rule) with f0 > 0 holds K = min((S - 2 L - d) // L + 1, 32) cycles of L = round(sr / f0) samples
    and is measured iff K >= 3.  (jitter, shimmer, nhr, hnr_db float32, cycles int32), each (B, T); every frame that is not measured
    has 0 in all five.  With return_cycles also (B, T, 32, 3) float32: period, correlation and RMS amplitude of every cycle, zeros
    behind the K-th.  Needs no model."""
    B, ld_wav, n_max, n64, T, tau_min, tau_max = _args.padded_wav("voice_quality", wav, n, n_max, sr, hop, W, fmin, fmax)
    _args.dense_arg("voice_quality", "f0", f0, (B, T), wav.device)
    with torch.cuda.device(wav.device):
        jitter, shimmer, nhr, hnr_db = (torch.empty(B, T, dtype=torch.float32, device=wav.device) for _ in range(4))
        cycles = torch.empty(B, T, dtype=torch.int32, device=wav.device)
        cyc = torch.empty(B, T, VQ_MAX_CYCLES, 3, dtype=torch.float32, device=wav.device) if return_cycles else None
        a = make("T2VoiceQuality", wav=wav, ld_wav=ld_wav, n=n64, B=B, n_max=n_max, sr=sr, hop=hop, W=W, tau_min=tau_min, tau_max=tau_max,
                 f0=f0, jitter=jitter, shimmer=shimmer, nhr=nhr, hnr_db=hnr_db, cycles=cycles, cyc=cyc)
        call("t2_voice_quality", a, stream())
    return (jitter, shimmer, nhr, hnr_db, cycles, cyc) if return_cycles else (jitter, shimmer, nhr, hnr_db, cycles)


def corpus_stats(f0, power, jitter, shimmer, nhr, hnr_db, cycles, n, hop=256, span=1024 + 367, power_floor=1e-10):
    """Per-utterance means (C-ABI t2_corpus_stats) of yin's f0 (or pitch_viterbi's) and power and of voice_quality's five (B, T) arrays,
    with n, hop and span = W + tau_max of those calls: (B, 12) float32 rows [valid, voiced, measured, loud frames, mean f0 Hz over the
    voiced frames, mean jitter, shimmer, nhr, hnr_db over the measured frames, mean 10 log10 power over the loud frames (valid and
    power > power_floor), 0, 0].  A mean over no frame is 0."""
    B, T = _args.same_shape_2d("corpus_stats", (("f0", f0), ("power", power), ("jitter", jitter), ("shimmer", shimmer), ("nhr", nhr),
                                                ("hnr_db", hnr_db), ("cycles", cycles)), dtypes=dict(cycles=torch.int32))
    if B < 1 or B > 65535 or T < 1:
        raise ValueError(f"corpus_stats: arrays of shape ({B}, {T}): need 1 .. 65535 utterances and T >= 1")
    _args.int_arg("corpus_stats", "hop", hop, 1)
    _args.int_arg("corpus_stats", "span", span, 1)
    power_floor = _args.real_arg("corpus_stats", "power_floor", power_floor)
    n64 = _args.lengths("corpus_stats", "n", n, B, f0.device).to(torch.int64).contiguous()
    with torch.cuda.device(f0.device):
        out = torch.empty(B, CORPUS_NSTAT, dtype=torch.float32, device=f0.device)
        a = make("T2CorpusStats", f0=f0, power=power, jitter=jitter, shimmer=shimmer, nhr=nhr, hnr_db=hnr_db, cycles=cycles, n=n64, B=B,
                 T=T, hop=hop, S=span, power_floor=power_floor, out=out)
        call("t2_corpus_stats", a, stream())
    return out


PITCH_MAX_STATES = K["PITCH_MAX_STATES"]  # voiced states (integer lags) of t2_pitch_viterbi
F0_NSTAT = K["F0_NSTAT"]
# w: transition cost per octave of lag change; max_jump: the largest allowed change in octaves per frame; u: local cost of the
# unvoiced state (YIN's voicing threshold: a frame whose best lag is worse than that is cheaper unvoiced); c_sw: a voicing switch
VITERBI_DEFAULTS = dict(w=1.0, max_jump=0.25, u=YIN_DEFAULTS["vthr"], c_sw=0.15)


def pitch_viterbi(cmnd, power, n, sr=22050, hop=256, fmin=60.0, fmax=500.0, power_floor=1e-10, w=1.0, max_jump=0.25,
                  u=VITERBI_DEFAULTS["u"], c_sw=0.15):
    """The cheapest lag sequence through yin's normalised difference (C-ABI t2_pitch_viterbi): cmnd (B, T, tau_max + 1)
    and power (B, T) as yin(return_cmnd=True) of the same sr, hop, fmin, fmax gives them, n (B,) the sample counts - the first
    min(T, 1 + n[b] // hop) frames are decoded.  States are the integer lags tau_min .. tau_max - 1 and one unvoiced state; a lag
    costs its cmnd (nothing voiced where power <= power_floor), the unvoiced state u, a lag change w * |log2 ratio| and at most
    max_jump octaves per frame, a voicing switch c_sw.  (f0 Hz, aperiodicity, lag int32, each (B, T); cost float64 (B,)): f0 and lag
    0, aperiodicity 1 for an unvoiced frame and behind the decoded frames.  Needs no model."""
    fn = "pitch_viterbi"
    _args.tensor_arg(fn, "cmnd", cmnd, 3, "(B, T, tau_max + 1)")
    _args.on_gpu(fn, "cmnd", cmnd)
    B, T, NT = cmnd.shape
    _args.batch_arg(fn, B)
    _check_frames(fn, T)
    _args.dense_arg(fn, "power", power, (B, T), cmnd.device)
    _args.int_arg(fn, "hop", hop, 1)
    tau_min, tau_max = _args.lags(fn, sr, fmin, fmax)
    _args.usable_lags(fn, tau_min, tau_max, sr, fmin, fmax)
    N = tau_max - tau_min
    if N > PITCH_MAX_STATES:
        raise ValueError(f"pitch_viterbi: {N} lags, above the limit of {PITCH_MAX_STATES} (T2_PITCH_MAX_STATES)")
    if NT != tau_max + 1:
        raise ValueError(f"pitch_viterbi: cmnd has {NT} lags per frame, {fmin} .. {fmax} Hz at {sr} Hz need tau_max + 1 = {tau_max + 1}")
    ld_b, ld_t = _args.strided_3d(fn, "cmnd", cmnd)
    w, max_jump, u, c_sw = (_args.real_arg(fn, k, v, nonneg=True) for k, v in (("w", w), ("max_jump", max_jump), ("u", u), ("c_sw", c_sw)))
    power_floor = _args.real_arg(fn, "power_floor", power_floor)
    n64 = _args.lengths(fn, "n", n, B, cmnd.device).to(torch.int64)
    with torch.cuda.device(cmnd.device):
        dev = cmnd.device
        frames = (1 + torch.div(n64.clamp(min=0), hop, rounding_mode="floor")).clamp(max=T).to(torch.int32)
        lw = (w * torch.log2(torch.arange(tau_min, tau_max, dtype=torch.float64))).to(dev)     # built on the host
        f0, aper = (torch.empty(B, T, dtype=torch.float32, device=dev) for _ in range(2))
        lag = torch.empty(B, T, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        back = torch.empty(B, T, N + 1, dtype=torch.int16, device=dev)       # (the kernel's uint16 workspace)
        a = make("T2PitchViterbi", cmnd=cmnd, ld_b=ld_b, ld_t=ld_t, power=power, len=frames, lw=lw, B=B, T=T, sr=sr, tau_min=tau_min,
                 tau_max=tau_max, power_floor=power_floor, trans_max=w * max_jump, u=u, c_sw=c_sw,
                 f0=f0, aper=aper, lag=lag, cost=cost, back=back)
        call("t2_pitch_viterbi", a, stream())
    return f0, aper, lag, cost


def f0_path_stats(path, path_len, f0_a, n_a, f0_b, n_b, hop=256, span=1024 + 367):
    """Two pitch tracks compared along a warping path (C-ABI t2_f0_path_stats): path (B, P, 2) int32 and path_len (B,) as
    Engine.dtw(return_path=True) gives them - cell (i, j) pairs frame i of f0_a (B, Ta) with frame j of f0_b (B, Tb), Hz, 0 =
    unvoiced -, n_a and n_b the sample counts, hop and span = W + tau_max of the yin call (the validity rule of prosody_stats; cells
    outside a track count as invalid).  (B, 12) float64 rows [scored cells, both voiced, only a voiced, only b voiced, sum d, sum d^2
    with d = 1200 (log2 fa - log2 fb) cents over the both-voiced cells, sum la, sum lb, sum la^2, sum lb^2, sum la lb with la =
    log2 fa, 0]; f0_figures turns a row into RMSE, bias, correlation and voicing error.  Sums in fp64 in a fixed order (per thread, a shuffle
    tree, the waves in order: t2m_sums_to_thread0 of csrc/t2_measure.hpp)."""
    fn = "f0_path_stats"
    if not torch.is_tensor(path) or path.dim() != 3 or path.shape[2] != 2 or path.dtype != torch.int32 or not path.is_contiguous():
        raise ValueError("f0_path_stats: path must be a contiguous int32 (B, P, 2) tensor")
    _args.on_gpu(fn, "path", path)
    B, P, _ = path.shape
    if B < 1 or B > 65535 or P < 1:
        raise ValueError(f"f0_path_stats: path of shape {tuple(path.shape)}: need 1 .. 65535 pairs and P >= 1")
    if not torch.is_tensor(path_len) or path_len.dtype != torch.int32 or path_len.device != path.device or path_len.shape != (B,):
        raise ValueError(f"f0_path_stats: path_len must be {B} int32 on {path.device}")
    _args.dense_arg(fn, "f0_a", f0_a, (B, None), path.device)
    _args.dense_arg(fn, "f0_b", f0_b, (B, None), path.device)
    _args.int_arg(fn, "hop", hop, 1)
    _args.int_arg(fn, "span", span, 1)
    na64 = _args.lengths(fn, "n", n_a, B, path.device).to(torch.int64).contiguous()      # (both counts are "n" in the message)
    nb64 = _args.lengths(fn, "n", n_b, B, path.device).to(torch.int64).contiguous()
    with torch.cuda.device(path.device):
        out = torch.empty(B, F0_NSTAT, dtype=torch.float64, device=path.device)
        a = make("T2F0PathStats", path=path, path_len=path_len.contiguous(), f0_a=f0_a, f0_b=f0_b, n_a=na64, n_b=nb64, B=B, P=P,
                 Ta=f0_a.shape[1], Tb=f0_b.shape[1], hop=hop, S=span, out=out)
        call("t2_f0_path_stats", a, stream())
    return out


def f0_figures(row) -> dict:
    """The figures of one f0_path_stats row (12 numbers): n_pairs, n_voiced_both, f0_rmse_cents, f0_bias_cents (a minus b), f0_corr
    (Pearson of log2 f0; None with fewer than 2 both-voiced cells or a column without variance), vuv_error = (only a + only b) /
    scored.  None where undefined."""
    n, nb = int(row[0]), int(row[1])
    out = dict(n_pairs=n, n_voiced_both=nb, f0_rmse_cents=None, f0_bias_cents=None, f0_corr=None, vuv_error=None)
    if n > 0:
        out["vuv_error"] = (row[2] + row[3]) / n
    if nb > 0:
        out["f0_rmse_cents"] = math.sqrt(max(row[5], 0.0) / nb)
        out["f0_bias_cents"] = row[4] / nb
    if nb >= 2:
        va, vb = row[8] - row[6] * row[6] / nb, row[9] - row[7] * row[7] / nb
        if va > 1e-12 * row[8] and vb > 1e-12 * row[9]:      # (a constant column leaves rounding noise, not variance)
            out["f0_corr"] = (row[10] - row[6] * row[7] / nb) / math.sqrt(va * vb)
    return out


_RESAMPLERS: dict = {}


def _resampler(sr_out: int, dev):
    """The datasets.resample.Resampler to sr_out on dev, made once: resample's, and voice.run_voice's for a pitch shift."""
    from .datasets.resample import Resampler
    return cached((int(sr_out), dev), lambda: Resampler(int(sr_out), dev), _RESAMPLERS)


def resample(wav, n, sr_in: int, sr_out: int):
    """A padded batch brought from sr_in to sr_out Hz (C-ABI t2_resample): wav (B, ld) float32 on the GPU, n the B sample
    counts (host integers, or an integer tensor, which is read back).  Returns (out (B, ld') float32, zeros behind each row, and the
    output counts ceil(n sr_out / sr_in) as host integers).  The Kaiser-windowed sinc of datasets/resample.py, designed once per
    rate pair; sr_in == sr_out returns the input.  Needs no model."""
    if not torch.is_tensor(wav) or wav.device.type != "cuda":
        raise ValueError("resample: wav must be a float32 (B, samples) tensor on the GPU")
    return _resampler(sr_out, wav.device).batch(wav, n.tolist() if torch.is_tensor(n) else n, int(sr_in))
