"""The voice chain behind the vocoder as ONE plan: plan_voice checks a tempo and a pitch change and says what
will run, run_voice runs it on a padded batch.  analysis.pitch_shift, analysis.pitch_shift_psola and `say` are these two functions
under their own names, limits and messages, so what `say` divides its times by is what the kernels ran at.  Importable without
torch or the library, as options.py is: what a plan needs of them is imported when one is made."""
from __future__ import annotations

from typing import NamedTuple, Tuple


class VoicePlan(NamedTuple):
    """sample_rate of the signal; requested_tempo, semitones and pitch_range as asked for; psola: the pitch is changed by TD-PSOLA
    behind a stretch by the tempo alone, else by a stretch and a resampling sr_mid -> sample_rate; ratio: the (P, Q) t2_stretch runs
    at; sr_mid == sample_rate when nothing is resampled; tempo: the EFFECTIVE tempo, what output times are divided by; frame and
    tolerance of the stretch; active: False when nothing would be launched."""
    sample_rate: int
    requested_tempo: object
    semitones: float
    pitch_range: float
    psola: bool
    ratio: Tuple[int, int]
    sr_mid: int
    tempo: float
    frame: int
    tolerance: int
    active: bool


def wav_target(output: str, hifi_gan_checkpoint) -> bool:
    """`say` writes audio - which the voice chain, the output rate and a document need - to a `.wav` target or with a HiFi-GAN
    checkpoint; anything else is a log-mel."""
    return hifi_gan_checkpoint is not None or output.endswith(".wav")


def plan_voice(fn: str, sample_rate, tempo=1.0, semitones=0.0, pitch_range=1.0, psola=False, frame=1024, tolerance=256, pitch=True) -> VoicePlan:
    """The plan of the caller `fn`, every refusal a ValueError(f"{fn}: ...").  psola: semitones -24 .. 24, pitch_range 0 .. 2, the
    tempo as time_stretch takes it.  Else the stretch and resampling of stretch.pitch_plan, at 0 semitones too, whose resampling
    table must exist - or with pitch=False a plain stretch by the tempo, semitones and pitch_range not being looked at."""
    from . import _args
    from .stretch import pitch_plan, tempo_ratio, window_args
    if psola:
        from .psola import shift_args
        semitones, pitch_range = shift_args(fn, semitones, pitch_range)
        sr = sr_mid = _args.int_arg(fn, "sample_rate", sample_rate, 1000)
    elif pitch:
        sr_mid, eff, ratio = pitch_plan(fn, semitones, sample_rate, tempo)
        sr, semitones, pitch_range = int(sample_rate), float(semitones), 1.0
    else:
        sr = sr_mid = int(sample_rate)
        semitones, pitch_range = 0.0, 1.0
    if psola or not pitch:
        ratio = tempo_ratio(fn, tempo)
        eff = ratio[0] / ratio[1]
    frame, tolerance = window_args(fn, frame, tolerance)
    if sr_mid != sr:
        from .datasets.resample import plan
        plan(sr_mid, sr)
    return VoicePlan(sr, tempo, semitones, pitch_range, bool(psola), ratio, sr_mid, eff, frame, tolerance,
                     bool(ratio[0] != ratio[1] or sr_mid != sr or (psola and (semitones != 0.0 or pitch_range != 1.0))))


def run_voice(plan: VoicePlan, wav, n, meter=None, fn=None):
    """wav (B, ld) float32 on the GPU and its counts n, as time_stretch takes them, through the plan: ONE t2_stretch launch for all
    rows (none at a ratio of 1), then with plan.psola psola.track_lags - the two pitch-tracking launches -, pitch_ratio and ONE
    t2_psola launch on the stretched signal, with `meter` (None: psola.default_meter) - nothing of them at 0 semitones and a range of
    1 -, else the resampling sr_mid -> sample_rate where the two differ.  (y (B, ld') float32, n_out host integers); refusals carry
    `fn` (None: the analysis function of the plan's path).  An inactive plan launches nothing: wav itself comes back."""
    import torch
    from . import _args, analysis, psola
    from .stretch import _stretch
    fn = fn or ("pitch_shift_psola" if plan.psola else "time_stretch" if plan.sr_mid == plan.sample_rate else "pitch_shift")
    if plan.psola:
        _args.tensor_arg(fn, "wav", wav, 2, "(B, samples)")
        _args.on_gpu(fn, "wav", wav)
        meter = psola.default_meter(plan.sample_rate, wav.device) if meter is None else meter
        psola.check_meter(fn, meter)
        if meter.settings["sr"] != plan.sample_rate or meter.device != wav.device:
            raise ValueError(f"{fn}: the meter is for {meter.settings['sr']} Hz on {meter.device}, the signal is {plan.sample_rate} Hz on "
                             f"{wav.device}")
    y, counts, _ = _stretch(fn, wav, n, plan.ratio, plan.frame, plan.tolerance)
    counts = [int(v) for v in (counts.tolist() if torch.is_tensor(counts) else counts)]
    if plan.sr_mid != plan.sample_rate:
        return analysis._resampler(plan.sample_rate, wav.device).batch(y, counts, plan.sr_mid)
    if not plan.psola or (plan.semitones == 0.0 and plan.pitch_range == 1.0) or y.numel() == 0:  # (t2_yin takes no batch without a column)
        return y, counts
    hop, n_max = meter.settings["hop"], max(counts)
    psola.check_frames(fn, n_max, hop)
    with torch.cuda.device(wav.device):
        lag = psola.track_lags(meter, y, torch.tensor(counts, dtype=torch.int64, device=wav.device), n_max)
        out, _ = psola.psola(y, counts, lag, psola.pitch_ratio(lag, counts, plan.semitones, plan.pitch_range, hop), hop)
    return out, counts
