#!/usr/bin/env python3
"""CLI with the reference's surface for the hot path (main.py:15-107,150-226 of mattm458/tacotron2):

    python main.py --config C --device N train --speech-dir S [--results-dir R] [--resume-ckpt K] [--finetune --finetune-steps n]
                                                  [--guided-attention SIGMA,ALPHA]
                                                  [--mel-loss l2|l1|l1+l2] [--masked-loss | --no-masked-loss] [--stop-weight W]
                                                  [--ema-decay D] [--decoupled-weight-decay] [--grad-clip NORM]
                                                  [--lr-schedule multistep|exponential|noam] [--lr-warmup STEPS]
                                                  [--lr-decay START,STEPS,MIN_LR]
    python main.py --config C --device N say --checkpoint K --text "..." [--out out.npy] [--random-seed s] [--speaker-id i]
    python main.py --config C --device N say --checkpoint K --text-file chapter.txt --out chapter.wav [--expand-numbers] [--level]
                                                  [--attention-window BACK,FWD | --forward-attention] [--durations-out PATH]
    python main.py --config C --device N test --speech-dir S --checkpoint K [--hifi-gan-checkpoint G] [--results-dir R]
                                                  [--attention-window BACK,FWD | --forward-attention] [--score [--no-audio | --f0]]
    python main.py --config C --device N test-correlation --speech-dir S --checkpoint K [--hifi-gan-checkpoint G] [--results-dir R]
                                                  [--attention-window BACK,FWD | --forward-attention] [--measure [--smooth-pitch]]
    python main.py --config C --device N measure-correlation --results-dir R [--features a,b,...]
    (say, test and test-correlation also take --stop-threshold P; they, train-mel-export and duration-export take --ema)
    python main.py --config C --device N train-mel-export --speech-dir S --checkpoint K [--results-dir R]
    python main.py --config C --device N duration-export --speech-dir S --checkpoint K [--results-dir R] [--mode monotonic|argmax]
                                                  [--variances [--pitch-domain log|hz] [--interpolate-pitch] [--frame-level]
                                                   [--no-smooth-pitch]]
    python main.py --config C --device N prosody-export --speech-dir S [--results-dir R] [--no-smooth-pitch] [--batch-size 64]

Other reference sub-commands (preprocess, server) are data preparation / demo tooling outside the hot-path scope
(SURVEY.md section 2); prosody-export writes what preprocess and the split scripts write for the controls, with this project's meter.  Multi-GPU training: `python -m torch.distributed.run --nproc-per-node N
main.py --config C train ...` (one process per GPU, RCCL gradient all-reduce)."""
import re

import click

from tacotron2_amd.run.common import load_config, sample_rate
from tacotron2_amd.voice import wav_target


def parse_attention_window(ctx, param, value):
    """--attention-window BACK,FWD -> (back, fwd): two integers >= 0, anything else a usage error."""
    if value is None:
        return None
    parts = [p.strip() for p in value.split(",")]
    if len(parts) != 2 or not all(re.fullmatch(r"[0-9]+", p) for p in parts):
        raise click.BadParameter(f"expected BACK,FWD (two integers >= 0, e.g. 1,3), got {value!r}")
    return int(parts[0]), int(parts[1])


def parse_guided_attention(ctx, param, value):
    """--guided-attention SIGMA,ALPHA -> (sigma, alpha): two numbers, sigma > 0 and alpha >= 0, anything else a usage error."""
    if value is None:
        return None
    from tacotron2_amd.options import check_guided_attention
    parts = [p.strip() for p in value.split(",")]
    try:
        if len(parts) != 2:
            raise ValueError
        return check_guided_attention((float(parts[0]), float(parts[1])))
    except ValueError:
        raise click.BadParameter(f"expected SIGMA,ALPHA (two numbers, sigma > 0 and alpha >= 0, e.g. 0.4,1.0), got {value!r}") \
            from None


attention_window_option = click.option(
    "--attention-window", required=False, type=str, default=None, callback=parse_attention_window, metavar="BACK,FWD",
    help="Windowed (monotonic) attention: each decoder frame attends only to the text positions from BACK before to FWD after "
         "the previous frame's attention peak (ESPnet's attention constraint; 1,3 is the usual value). Default: off, the whole "
         "text.")


forward_attention_option = click.option(
    "--forward-attention", is_flag=True, default=False,
    help="Forward attention (Zhang et al. 2018; Mozilla TTS's use_forward_attn): each decoder frame's attention stays where it is or "
         "advances one text position; no skipping ahead, no jumping back. The config's model.forward_attention sets the default; "
         "the flag wins. Not together with --attention-window. Default: off.")


def parse_stop_threshold(ctx, param, value):
    """--stop-threshold P -> a float with 0 < P < 1, anything else a usage error."""
    if value is None:
        return None
    from tacotron2_amd.options import check_stop_threshold
    try:
        return check_stop_threshold(float(value))
    except ValueError:
        raise click.BadParameter(f"expected a number with 0 < P < 1 (e.g. 0.4), got {value!r}") from None


stop_threshold_option = click.option(
    "--stop-threshold", required=False, type=str, default=None, callback=parse_stop_threshold, metavar="P",
    help="Stop probability below which an utterance ends (NVIDIA's gate_threshold): lower decodes longer, higher stops earlier. "
         "Wins over model.stop_threshold of the config. Default: 0.5, the reference's rule.")


def decode_options(f):
    """--attention-window, --forward-attention and --stop-threshold, in this order: the decode settings that say, test and
    test-correlation share."""
    for option in (stop_threshold_option, forward_attention_option, attention_window_option):
        f = option(f)
    return f


def parse_stop_weight(ctx, param, value):
    """--stop-weight W -> a finite float > 0, anything else a usage error."""
    if value is None:
        return None
    from tacotron2_amd.options import check_loss_options
    try:
        return check_loss_options({"stop_weight": float(value)})[2]
    except ValueError:
        raise click.BadParameter(f"expected a finite number > 0 (e.g. 8), got {value!r}") from None


def parse_ema_decay(ctx, param, value):
    """--ema-decay D -> a float with 0 <= D < 1, anything else a usage error."""
    if value is None:
        return None
    from tacotron2_amd.options import check_optimizer_options
    try:
        return check_optimizer_options({"ema_decay": float(value)}).ema_decay
    except ValueError:
        raise click.BadParameter(f"expected a number with 0 <= D < 1 (e.g. 0.999), got {value!r}") from None


def parse_grad_clip(ctx, param, value):
    """--grad-clip NORM -> a finite float >= 0 (0: no clip), anything else a usage error."""
    if value is None:
        return None
    from tacotron2_amd.options import check_optimizer_options
    try:
        return check_optimizer_options({"grad_clip": float(value)}).grad_clip
    except ValueError:
        raise click.BadParameter(f"expected a finite number >= 0 (0 switches the clip off, e.g. 1.0), got {value!r}") from None


def parse_lr_warmup(ctx, param, value):
    """--lr-warmup STEPS -> an integer >= 0, anything else a usage error."""
    if value is None:
        return None
    if not re.fullmatch(r"[0-9]+", value.strip()):
        raise click.BadParameter(f"expected a number of steps >= 0 (e.g. 4000), got {value!r}")
    return int(value)


def parse_lr_decay(ctx, param, value):
    """--lr-decay START,STEPS,MIN_LR -> (start, steps, min_lr): two integers, start >= 0 and steps >= 1, and a finite number > 0;
    anything else a usage error."""
    if value is None:
        return None
    parts = [p.strip() for p in value.split(",")]
    try:
        if len(parts) != 3 or not all(re.fullmatch(r"[0-9]+", p) for p in parts[:2]):
            raise ValueError
        start, steps, min_lr = int(parts[0]), int(parts[1]), float(parts[2])
        if steps < 1 or not 0.0 < min_lr < float("inf"):
            raise ValueError
        return start, steps, min_lr
    except ValueError:
        raise click.BadParameter("expected START,STEPS,MIN_LR (two integers, START >= 0 and STEPS >= 1, and a number > 0, "
                                 f"e.g. 50000,50000,1e-5), got {value!r}") from None


ema_option = click.option(
    "--ema", is_flag=True, default=False,
    help="Load the checkpoint's EMA weights (written by `train --ema-decay`) instead of the live ones; a checkpoint without them "
         "is an error. Wins over model.use_ema of the config. Default: off.")


def with_ema(cfg: dict, ema: bool) -> dict:
    """The drivers' arguments with model.use_ema set for the --ema flag (the loaders read it there); unchanged without the flag."""
    return dict(cfg, model_config=dict(cfg["model_config"], use_ema=True)) if ema else cfg


def forward_attention_arg(forward_attention, attention_window):
    """The drivers' forward_attention argument: True for the flag, None (= the config's model.forward_attention) without it; the
    flag together with --attention-window is a usage error."""
    if forward_attention and attention_window is not None:
        raise click.UsageError("--forward-attention and --attention-window do not combine: use one of the two")
    return True if forward_attention else None


def config_args(ctx, missing: str) -> dict:
    """The four sections of --config and --device as the drivers' keyword arguments; without --config an Exception saying `missing`."""
    c = ctx.obj["config"]
    if c is None:
        raise Exception(missing)
    return dict(dataset_config=c["dataset"], training_config=c["training"], model_config=c["model"],
                extensions_config=c["extensions"], device=ctx.obj["device"])


@click.group()
@click.pass_context
@click.option("--config", type=str, required=False, default=None, help="A Tacotron hyperparameter config file")
@click.option("--device", type=int, required=False, default=0, help="The GPU to use for training or inference. Default 0.")
def main(ctx, config, device):
    ctx.ensure_object(dict)
    ctx.obj["config"] = load_config(config) if config is not None else None
    ctx.obj["device"] = device


@main.command()
@click.pass_context
@click.option("--speech-dir", required=True, type=str, help="A directory containing audio files from the dataset.")
@click.option("--results-dir", required=False, type=str, help="The directory to save results.")
@click.option("--resume-ckpt", required=False, type=str, help="Resume training from the given checkpoint.")
@click.option("--prosody-model-checkpoint", required=False, type=str, help="(accepted for CLI compatibility; unused)")
@click.option("--finetune", is_flag=True, default=False, help="Fine-tune a model. If specified, --resume-ckpt is required.")
@click.option("--finetune-steps", required=False, type=int, help="Steps to fine-tune. Required if --finetune is given.")
@click.option("--max-steps", required=False, type=int, default=None, help="Override training.args.max_steps (smoke runs).")
@click.option("--synthetic", is_flag=True, default=False, help="Train on synthetic LJSpeech-shaped batches (no dataset needed).")
@click.option("--guided-attention", required=False, type=str, default=None, callback=parse_guided_attention, metavar="SIGMA,ALPHA",
              help="Guided-attention loss: adds ALPHA times the mean of the attention weights under the off-diagonal mask "
                   "1 - exp(-(l/N - t/T)^2 / (2 SIGMA^2)) to the training and validation loss, so that the alignment forms early "
                   "(0.4,1.0 is the usual value). Wins over training.guided_attention of the config. Default: off.")
@click.option("--forward-attention", is_flag=True, default=False,
              help="Train under forward attention (Zhang et al. 2018): every teacher-forced frame's weights are the softmax times the "
                   "prior 0.5 a[t-1][n] + 0.5 a[t-1][n-1], renormalised, forward and backward. Decode such a model with "
                   "--forward-attention. Wins over training.forward_attention of the config. Default: off.")
@click.option("--mel-loss", required=False, type=click.Choice(["l2", "l1", "l1+l2"]), default=None,
              help="The two mel terms: l2 = mean squared error (the reference), l1 = mean absolute error, l1+l2 = their sum (ESPnet's "
                   "default). Wins over training.loss.mel of the config. Default: l2.")
@click.option("--masked-loss/--no-masked-loss", default=None,
              help="Average the three loss terms over the valid frames of the batch only, not over its padding (ESPnet's use_masking); "
                   "--no-masked-loss is the plain mean. Either wins over training.loss.masked of the config. Default: the config's "
                   "value, else the plain mean.")
@click.option("--stop-weight", required=False, type=str, default=None, callback=parse_stop_weight, metavar="W",
              help="Weight of the stop class (the one last frame of an utterance) in the stop-token loss; 5 to 20 is customary "
                   "(ESPnet's bce_pos_weight, on the class that is rare here). Wins over training.loss.stop_weight. Default: 1.")
@click.option("--ema-decay", required=False, type=str, default=None, callback=parse_ema_decay, metavar="D",
              help="Keep an exponential moving average of the weights, ema += (1 - D) (p - ema) after every step (0.999 to 0.9999 is "
                   "customary; the first updates run under min(D, (1 + k) / (10 + k))). Checkpoints carry it as ema_state_dict, "
                   "validation also reports validation_loss_ema, and say / test / the exports decode from it with --ema. Wins over "
                   "training.optimizer.ema_decay. Default: 0, off.")
@click.option("--decoupled-weight-decay/--no-decoupled-weight-decay", default=None,
              help="AdamW: the weight decay multiplies the weights by 1 - lr * weight_decay in front of the step instead of joining "
                   "the gradient. Either wins over training.optimizer.decoupled_weight_decay. Default: the config's value, else "
                   "L2 in the gradient (the reference).")
@click.option("--grad-clip", required=False, type=str, default=None, callback=parse_grad_clip, metavar="NORM",
              help="Clip the global gradient norm at NORM; 0 switches the clip off. Wins over training.optimizer.grad_clip. Default: 1.0.")
@click.option("--lr-schedule", required=False, type=click.Choice(["multistep", "exponential", "noam"]), default=None,
              help="multistep: a tenth at each of model.scheduler_milestones (the reference); exponential: from lr to MIN_LR over "
                   "--lr-decay (the Tacotron 2 paper); noam: linear warm-up over --lr-warmup steps to lr, then lr * sqrt(W / step). "
                   "Wins over training.optimizer.schedule. Default: multistep.")
@click.option("--lr-warmup", required=False, type=str, default=None, callback=parse_lr_warmup, metavar="STEPS",
              help="Linear warm-up: the first STEPS steps run at lr * step / STEPS (multistep, exponential); noam's W. Wins over "
                   "training.optimizer.warmup_steps. Default: 0, none.")
@click.option("--lr-decay", required=False, type=str, default=None, callback=parse_lr_decay, metavar="START,STEPS,MIN_LR",
              help="With --lr-schedule exponential: lr until step START, then a geometric decay that reaches MIN_LR after STEPS more "
                   "steps and stays there (50000,50000,1e-5 is the paper's). Wins over training.optimizer.decay_start / decay_steps / "
                   "min_lr.")
def train(ctx, speech_dir, results_dir=None, resume_ckpt=None, prosody_model_checkpoint=None, finetune=False,
          finetune_steps=None, max_steps=None, synthetic=False, guided_attention=None, forward_attention=False, mel_loss=None,
          masked_loss=None, stop_weight=None, ema_decay=None, decoupled_weight_decay=None, grad_clip=None, lr_schedule=None,
          lr_warmup=None, lr_decay=None):
    cfg = config_args(ctx, "Configuration required for training!")
    if finetune and finetune_steps is None:
        raise Exception("If finetuning, --finetune-steps is required!")
    optimizer = dict(ema_decay=ema_decay, decoupled_weight_decay=decoupled_weight_decay, grad_clip=grad_clip, schedule=lr_schedule,
                     warmup_steps=lr_warmup)
    if lr_decay is not None:
        optimizer.update(decay_start=lr_decay[0], decay_steps=lr_decay[1], min_lr=lr_decay[2])
    from tacotron2_amd.options import optimizer_options_setting
    try:        # the combinations the options refuse are usage errors, before torch or the library is loaded
        tc, mc = cfg["training_config"], cfg["model_config"]
        optimizer_options_setting(tc, lr=(tc["lr"] / 10 if finetune else tc["lr"]) if "lr" in tc else None,
                                  milestones=mc.get("scheduler_milestones", []), **optimizer)
    except ValueError as e:
        raise click.UsageError(str(e)) from None
    from tacotron2_amd.run.train import do_train
    do_train(**cfg, speech_dir=speech_dir, results_dir=results_dir, resume_ckpt=resume_ckpt, finetune=finetune,
             finetune_steps=finetune_steps, max_steps_override=max_steps, synthetic=synthetic, guided_attention=guided_attention,
             forward_attention=True if forward_attention else None, mel_loss=mel_loss, masked_loss=masked_loss, stop_weight=stop_weight,
             optimizer=optimizer)


@main.command()
@click.pass_context
@click.option("--checkpoint", required=True, type=str, help="A trained Tacotron model checkpoint")
@click.option("--text", required=False, type=str, default=None, help="Text to speak (or --text-file)")
@click.option("--text-file", required=False, type=click.Path(exists=True, dir_okay=False), default=None, metavar="PATH",
              help="A document to read: split into sentences of at most --max-chars characters, decoded side by side in chunks of "
                   "--batch-size, trimmed, faded and joined on the GPU with --pause between them, written as ONE .wav. Exclusive "
                   "with --text; needs a .wav target or a HiFi-GAN checkpoint.")
@click.option("--max-chars", required=False, type=click.IntRange(min=1), default=None, metavar="N",
              help="With --text-file: the longest piece, in characters of the cleaned text; a longer sentence is cut at its last "
                   "';', ':' or ',', else at a space. Default: 190.")
@click.option("--expand-numbers", is_flag=True, default=False,
              help="With --text-file: English number words for integers, decimals, ordinals, -5 and 50%% before the text is cleaned "
                   "(which deletes every digit). No years, currency, times or Roman numerals.")
@click.option("--pause", required=False, type=str, default=None, metavar="SENT,CLAUSE,PARA",
              help="With --text-file: seconds of silence behind a sentence, a cut inside a sentence and a paragraph. Default: 0.25,0.12,0.60.")
@click.option("--no-trim", is_flag=True, default=False,
              help="With --text-file: keep each piece's leading and trailing silence (default: trimmed by the dataset's rule, "
                   "preprocessing.trim_top_db over trim_frame_length, 20 ms kept).")
@click.option("--level", is_flag=True, default=False,
              help="With --text-file: bring every piece towards the document's RMS (by at most 6 dB either way) and keep the peak at or below 1.")
@click.option("--fade-ms", required=False, type=click.FloatRange(min=0), default=None, metavar="X",
              help="With --text-file: half-Hann fade at both ends of every piece, in ms. Default: 5.")
@click.option("--batch-size", required=False, type=click.IntRange(min=1, max=64), default=None, metavar="N",
              help="With --text-file: pieces decoded together, 1 to 64. Default: 64.")
@click.option("--max-len", required=False, type=click.IntRange(min=1), default=5000, metavar="FRAMES",
              help="The decode stops a text that has not stopped by itself after FRAMES mel frames. Default: 5000.")
@click.option("--out", required=False, type=str, default="out.npy", help="Output file (log-mel .npy). Default: out.npy")
@click.option("--hifi-gan-checkpoint", required=False, type=str, default=None, help="HiFi-GAN generator checkpoint (config.json next to it, UNIVERSAL_V1 values when absent)")
@click.option("--random-seed", required=False, type=int, default=None, help="A random seed to use in generation.")
@click.option("--speaker-id", required=False, type=int, default=None, help="Speaker ID for a multi-speaker model")
@click.option("--controls", required=False, type=str, default=None, help="If controls are enabled, a comma-separated list of values to pass into the model. Defaults to all 0 values.")
@click.option("--description", required=False, type=str, default=None, help="Path of a precomputed description embedding (.pt / .npy, pooler_output of bert-base-uncased); raw text needs the BERT weights (unavailable offline)")
@decode_options
@ema_option
@click.option("--durations-out", required=False, type=str, default=None, metavar="PATH",
              help="Write character timestamps as JSON: per text the encoded symbols, the mel frames each one lasts (the best "
                   "monotonic path through the decode's own alignments), start_s / end_s, focus_rate and feasible. Default: off.")
@click.option("--out-sample-rate", required=False, type=click.IntRange(min=1), default=None, metavar="R",
              help="Write the audio at R Hz (48000, 44100, 16000, 8000, ...) instead of the model's rate: the vocoded waveform is "
                   "resampled on the GPU. Needs a .wav target; --durations-out times stay in model frames. Default: the model's rate.")
@click.option("--tempo", required=False, type=float, default=None, metavar="T",
              help="Speak T times as fast, 0.5 to 2.0, at the same pitch: the vocoded waveform is time-stretched on the GPU (WSOLA), the "
                   "model's output stays as decoded. Needs a .wav target; --durations-out times and --text-file pauses are divided by "
                   "the tempo. Default: off.")
@click.option("--pitch-shift", required=False, type=float, default=None, metavar="SEMITONES",
              help="Raise the voice by SEMITONES, -12 to 12, at the same tempo: a time stretch and a resampling on the GPU (formants "
                   "move with the pitch). Needs a .wav target. Default: off.")
@click.option("--preserve-formants", is_flag=True, default=False,
              help="With --pitch-shift or --pitch-range: change the pitch by TD-PSOLA on the GPU instead - pitch-synchronous grains are "
                   "re-spaced, so the formants stay where they are and the length is the tempo's alone. The level falls by up to a "
                   "third. Default: off.")
@click.option("--pitch-range", required=False, type=float, default=None, metavar="K",
              help="Scale the intonation range about the voice's mean pitch by K, 0 to 2: 0 is a monotone voice, 1 unchanged, 2 twice "
                   "the excursions. Works with any checkpoint; always by TD-PSOLA, so it implies --preserve-formants. Needs a .wav "
                   "target. Default: off.")
@click.option("--loudness", required=False, type=float, default=None, metavar="LUFS",
              help="Write the file at this programme loudness, -40 to -5 LUFS (EBU R128: -23, podcasts: -16): measured by ITU-R "
                   "BS.1770-4 on the GPU on the samples as they are written - behind --tempo, --pitch-shift and --out-sample-rate -, "
                   "then ONE gain per file, lowered where --true-peak asks for it; no limiter, no compression. With --text-file the "
                   "loudness is the whole document's. Needs a .wav target. Default: off.")
@click.option("--true-peak", required=False, type=float, default=None, metavar="DBTP",
              help="With --loudness: the true peak (4x oversampled) the file may reach, -9 to 0 dBTP; the gain is lowered until it "
                   "holds. Default: -1.")
@click.option("--limiter", is_flag=True, default=False,
              help="With --loudness: hold --true-peak with a look-ahead true-peak limiter on the GPU (5 ms look-ahead, 50 ms release) "
                   "instead of a lower gain for the whole file, so a file with a few tall peaks comes out at the loudness asked for; "
                   "the line tells the limited samples, the largest reduction and the loudness reached. Default: off.")
@click.option("--denoise", required=False, type=float, default=None, metavar="STRENGTH",
              help="Take the HiFi-GAN generator's own stationary buzz off the waveform, 0 to 1: the spectrum of a vocoded all-zero mel, "
                   "times STRENGTH, is subtracted from every frame's magnitudes on the GPU - the first step behind the vocoder, in "
                   "front of --tempo, --pitch-shift, --out-sample-rate and --loudness. NVIDIA's defaults are 0.01 for HiFi-GAN and 0.1 "
                   "for WaveGlow. Needs --hifi-gan-checkpoint and a .wav target. Default: off.")
def say(ctx, checkpoint, text, out, speaker_id, hifi_gan_checkpoint, random_seed, controls, description, attention_window,
        forward_attention, durations_out=None, stop_threshold=None, out_sample_rate=None, text_file=None, max_chars=None,
        expand_numbers=False, pause=None, no_trim=False, level=False, fade_ms=None, batch_size=None, max_len=5000, tempo=None,
        pitch_shift=None, preserve_formants=False, pitch_range=None, ema=False, loudness=None, true_peak=None, limiter=False, denoise=None):
    if (text is None) == (text_file is None):
        raise click.UsageError("say needs exactly one of --text and --text-file" + (", got both" if text is not None else ""))
    limiter = True if limiter else None
    if loudness is not None or true_peak is not None or limiter:
        from tacotron2_amd.run.say import limiter_settings, loudness_settings
        try:
            loudness_settings(loudness, true_peak, wav_target(out, hifi_gan_checkpoint))
            limiter_settings(limiter, loudness)
        except ValueError as e:
            raise click.UsageError(str(e))
    if denoise is not None:
        from tacotron2_amd.run.say import denoise_settings
        try:
            denoise_settings(denoise, hifi_gan_checkpoint, out)
        except ValueError as e:
            raise click.UsageError(str(e))
    if text_file is None:
        given = [name for name, v in (("--max-chars", max_chars), ("--expand-numbers", expand_numbers or None), ("--pause", pause),
                                      ("--no-trim", no_trim or None), ("--level", level or None), ("--fade-ms", fade_ms),
                                      ("--batch-size", batch_size)) if v is not None]
        if given:
            raise click.UsageError(f"{', '.join(given)} only with --text-file")
    elif not wav_target(out, hifi_gan_checkpoint):
        raise click.UsageError(f"--text-file needs a .wav target (--out) or --hifi-gan-checkpoint, got --out {out}: a document has no single log-mel")
    preserve_formants = True if preserve_formants else None
    if tempo is not None or pitch_shift is not None or preserve_formants or pitch_range is not None:
        from tacotron2_amd.run.say import voice_settings
        try:
            voice_settings(tempo, pitch_shift, sample_rate(config_args(ctx, "Configuration required for speech!")["dataset_config"]["preprocessing"]),
                           wav_target(out, hifi_gan_checkpoint), preserve_formants, pitch_range)
        except ValueError as e:
            raise click.UsageError(str(e))
    forward_attention = forward_attention_arg(forward_attention, attention_window)
    common = dict(with_ema(config_args(ctx, "Configuration required for speech!"), ema), checkpoint=checkpoint, output=out, speaker_id=speaker_id,
                  hifi_gan_checkpoint=hifi_gan_checkpoint, random_seed=random_seed, controls=controls,
                  description=description, attention_window=attention_window, forward_attention=forward_attention,
                  durations_out=durations_out, stop_threshold=stop_threshold, out_sample_rate=out_sample_rate, max_len=max_len,
                  tempo=tempo, pitch_shift=pitch_shift, preserve_formants=preserve_formants, pitch_range=pitch_range,
                  loudness=loudness, true_peak=true_peak, limiter=limiter, denoise=denoise)
    if text_file is None:
        from tacotron2_amd.run.say import do_say
        do_say(text=text, **common)
        return
    from tacotron2_amd.run.say import do_say_document, parse_pauses
    try:
        parse_pauses(pause)
    except ValueError as e:
        raise click.UsageError(str(e))
    do_say_document(text_file=text_file, max_chars=190 if max_chars is None else max_chars, expand_numbers=expand_numbers, pause=pause,
                    trim=not no_trim, level=level, fade_ms=5.0 if fade_ms is None else fade_ms,
                    batch_size=64 if batch_size is None else batch_size, **common)


@main.command()
@click.pass_context
@click.option("--speech-dir", required=True, type=str, help="A directory containing audio files from the dataset.")
@click.option("--checkpoint", required=True, type=str, help="A trained Tacotron model checkpoint")
@click.option("--hifi-gan-checkpoint", required=False, type=str, default=None, help="A HiFi-GAN generator checkpoint. If not given, Griffin-Lim is used.")
@click.option("--results-dir", required=False, type=str, default=None, help="The directory to save results.")
@click.option("--batch-size", required=False, type=int, default=8, help="Utterances decoded together (reference: 8; up to 64 per decode group).")
@click.option("--max-len", required=False, type=int, default=5000, help="Frame cap per utterance (reference: 5000).")
@click.option("--limit", required=False, type=int, default=None, help="Only the first n utterances of the test manifest.")
@decode_options
@ema_option
@click.option("--score", is_flag=True, default=False,
              help="Also score every decode against its recording (the manifest's wav column under --speech-dir): mel-cepstral "
                   "distortion under dynamic time warping (MCD-DTW, 13 coefficients, dB), duration ratio, stop failures and "
                   "focus rate, as scores.csv and scores.json in the results directory. Default: off.")
@click.option("--no-audio", is_flag=True, default=False,
              help="With --score: skip vocoding and the WAV files, write the scores only.")
@click.option("--f0", is_flag=True, default=False,
              help="With --score: also compare intonation. Every synthesised waveform and its recording are pitch-tracked on the GPU "
                   "(YIN with Viterbi smoothing) and compared along the MCD warping path: F0 RMSE and bias in cents, log-F0 "
                   "correlation and voicing-decision error, as f0_scores.csv and four means in scores.json. Default: off.")
def test(ctx, speech_dir, checkpoint, hifi_gan_checkpoint, results_dir, batch_size, max_len, limit, attention_window,
         forward_attention, stop_threshold=None, score=False, no_audio=False, f0=False, ema=False):
    """Synthesise the test manifest (run/test.py of the reference): one wav per utterance + failures.csv."""
    forward_attention = forward_attention_arg(forward_attention, attention_window)
    if no_audio and not score:
        raise click.UsageError("--no-audio needs --score: without either there would be nothing to write")
    if f0 and not score:
        raise click.UsageError("--f0 needs --score: the tracks are compared along the path of the MCD score")
    if f0 and no_audio:
        raise click.UsageError("--f0 cannot go with --no-audio: there would be no waveform to track")
    cfg = with_ema(config_args(ctx, "Configuration required for testing!"), ema)
    from tacotron2_amd.run.test import do_test
    do_test(**cfg, speech_dir=speech_dir, checkpoint=checkpoint, hifi_gan_checkpoint=hifi_gan_checkpoint, results_dir=results_dir,
            batch_size=batch_size, max_len=max_len, limit=limit, attention_window=attention_window,
            forward_attention=forward_attention, stop_threshold=stop_threshold, score=score, audio=not no_audio, **({"f0": True} if f0 else {}))


@main.command()
@click.pass_context
@click.option("--speech-dir", required=True, type=str, help="A directory containing audio files from the dataset.")
@click.option("--checkpoint", required=True, type=str, help="A trained Tacotron model checkpoint")
@click.option("--hifi-gan-checkpoint", required=False, type=str, default=None, help="A trained HiFi-GAN model checkpoint")
@click.option("--results-dir", required=False, type=str, default=None, help="The directory to save results.")
@click.option("--samples-per-speaker", required=False, type=int, default=200, help="Utterances drawn per speaker (reference: 200).")
@click.option("--max-len", required=False, type=int, default=5000, help="Frame cap per utterance (reference: 5000).")
@click.option("--limit-overrides", required=False, type=int, default=None, help="Only the first n of the 51 control overrides.")
@decode_options
@ema_option
@click.option("--measure", is_flag=True, default=False,
              help="Also measure what comes out, on the GPU: pitch level and range (YIN), intensity, aperiodicity and speaking rate "
                   "of every waveform as prosody.csv in each override directory, and the correlation of every requested control "
                   "with its measure (Pearson, Spearman, slope, and the control x measure leakage matrix) as correlation.json in the "
                   "results directory. Default: off.")
@click.option("--smooth-pitch", is_flag=True, default=False,
              help="With --measure: decode every pitch track with the Viterbi smoother before its statistics (no octave jumps in "
                   "the pitch range). Default: off.")
def test_correlation(ctx, speech_dir, checkpoint, hifi_gan_checkpoint, results_dir, samples_per_speaker, max_len, limit_overrides,
                     attention_window, forward_attention, stop_threshold=None, measure=False, smooth_pitch=False, ema=False):
    """The test manifest under 51 control-vector overrides (run/test_correlation.py of the reference)."""
    forward_attention = forward_attention_arg(forward_attention, attention_window)
    if smooth_pitch and not measure:
        raise click.UsageError("--smooth-pitch needs --measure: without it no pitch is tracked")
    cfg = with_ema(config_args(ctx, "Configuration required for testing!"), ema)
    from tacotron2_amd.run.test_correlation import do_test_correlation
    given = dict(attention_window=None if attention_window is None else list(attention_window), forward_attention=forward_attention,
                 stop_threshold=stop_threshold)
    model_config = dict(cfg["model_config"], **{k: v for k, v in given.items() if v is not None})      # load_test_model reads them there
    if measure:                # the meter travels with the model (load_test_model), the tables need the directory's name afterwards
        import datetime
        model_config = dict(model_config, measure_prosody=True, **({"smooth_pitch": True} if smooth_pitch else {}))
        if results_dir is None:
            results_dir = f"results_{cfg['training_config']['name']}_test_correlation {datetime.datetime.now()}"
    do_test_correlation(**dict(cfg, model_config=model_config), speech_dir=speech_dir, checkpoint=checkpoint,
                        hifi_gan_checkpoint=hifi_gan_checkpoint, results_dir=results_dir, samples_per_speaker=samples_per_speaker,
                        max_len=max_len, limit_overrides=limit_overrides)
    if measure:
        from tacotron2_amd.prosody import ProsodyMeter
        from tacotron2_amd.run.correlation import correlate_tree
        meter = ProsodyMeter(sample_rate(cfg["dataset_config"].get("preprocessing", {})), f"cuda:{cfg['device']}", smooth=smooth_pitch)
        correlate_tree(results_dir, cfg["extensions_config"]["controls"]["features"], meter.describe())


@main.command()
@click.pass_context
@click.option("--results-dir", required=True, type=str, help="A results tree of test-correlation: one directory per override.")
@click.option("--features", required=False, type=str, default=None, metavar="a,b,...",
              help="The control names in the order of the override tuples. Default: extensions.controls.features of --config.")
def measure_correlation(ctx, results_dir, features=None):
    """Measure the WAVs of an existing test-correlation tree: rewrites prosody.csv per override and correlation.json."""
    if features is not None:
        names = [f.strip() for f in features.split(",")]
        if not all(names):
            raise click.UsageError(f"--features: expected a comma-separated list of names, got {features!r}")
    elif ctx.obj["config"] is not None and ctx.obj["config"].get("extensions", {}).get("controls", {}).get("features"):
        names = list(ctx.obj["config"]["extensions"]["controls"]["features"])
    else:
        raise click.UsageError("measure-correlation needs the control names: --features a,b,... or a --config with "
                               "extensions.controls.features")
    from tacotron2_amd.run.correlation import do_measure_correlation
    try:
        do_measure_correlation(results_dir, names, device=ctx.obj["device"])
    except ValueError as e:
        raise click.UsageError(str(e)) from None


@main.command()
@click.pass_context
@click.option("--speech-dir", required=True, type=str, help="A directory containing audio files from the dataset.")
@click.option("--checkpoint", required=True, type=str, help="A trained Tacotron model checkpoint")
@click.option("--results-dir", required=False, type=str, default=None, help="The directory to save results. Defaults to the model configuration name with a timestamp.")
@ema_option
def train_mel_export(ctx, speech_dir, checkpoint, results_dir=None, ema=False):
    """Teacher-forced post-net mels of the train + val manifests (run/train_mel_export.py of the reference)."""
    cfg = with_ema(config_args(ctx, "Configuration required!"), ema)
    from tacotron2_amd.run.train_mel_export import do_train_mel_export
    do_train_mel_export(**cfg, speech_dir=speech_dir, checkpoint=checkpoint, results_dir=results_dir)


@main.command()
@click.pass_context
@click.option("--speech-dir", required=True, type=str, help="A directory containing audio files from the dataset.")
@click.option("--checkpoint", required=True, type=str, help="A trained Tacotron model checkpoint")
@click.option("--results-dir", required=False, type=str, default=None, help="The directory to save results. Defaults to the model configuration name with a timestamp.")
@click.option("--mode", required=False, type=click.Choice(["monotonic", "argmax"]), default="monotonic",
              help="monotonic: the best monotonic path through the alignment (first character to last, stay or advance by one per "
                   "decoder step); argmax: each decoder step's attention peak. Default: monotonic.")
@click.option("--variances", is_flag=True, default=False,
              help="Also write per-character pitch and energy targets (<name>.pitch.npy, <name>.energy.npy) beside every .dur.npy, "
                   "with variances.csv, variance_stats.json (the train set's normalisation constants) and variances_dropped.csv. "
                   "Default: off.")
@click.option("--pitch-domain", required=False, type=click.Choice(["log", "hz"]), default=None,
              help="With --variances: the pitch in ln Hz or in Hz. Default: log.")
@click.option("--interpolate-pitch", is_flag=True, default=False,
              help="With --variances: interpolate the pitch across the unvoiced frames and average over all frames of a character "
                   "(FastSpeech 2). Default: the mean over its voiced frames, 0 without one (FastPitch).")
@click.option("--frame-level", is_flag=True, default=False,
              help="With --variances: also write <name>.pitch_frames.npy and <name>.energy_frames.npy, one value per mel frame.")
@click.option("--no-smooth-pitch", is_flag=True, default=False,
              help="With --variances: the raw YIN track instead of the Viterbi-smoothed one. Default: smoothed.")
@ema_option
def duration_export(ctx, speech_dir, checkpoint, results_dir=None, mode="monotonic", variances=False, pitch_domain=None,
                    interpolate_pitch=False, frame_level=False, no_smooth_pitch=False, ema=False):
    """Per-character durations (mel frames) of the train + val manifests from teacher-forced alignments, plus durations.csv; with
    --variances also per-character pitch and energy."""
    if not variances:
        given = [flag for flag, on in (("--pitch-domain", pitch_domain is not None), ("--interpolate-pitch", interpolate_pitch),
                                       ("--frame-level", frame_level), ("--no-smooth-pitch", no_smooth_pitch)) if on]
        if given:
            raise click.UsageError(f"{', '.join(given)} need{'s' if len(given) == 1 else ''} --variances")
    cfg = with_ema(config_args(ctx, "Configuration required!"), ema)
    from tacotron2_amd.run.duration_export import do_duration_export
    do_duration_export(**cfg, speech_dir=speech_dir, checkpoint=checkpoint, results_dir=results_dir, mode=mode, variances=variances, pitch_domain=pitch_domain or "log",
                       interpolate_pitch=interpolate_pitch, frame_level=frame_level, smooth_pitch=not no_smooth_pitch)


@main.command()
@click.pass_context
@click.option("--speech-dir", required=True, type=str, help="A directory containing audio files from the dataset.")
@click.option("--results-dir", required=False, type=str, default=None, help="The directory to save results. Defaults to the configuration name with a timestamp.")
@click.option("--no-smooth-pitch", is_flag=True, default=False,
              help="Measure on the raw YIN track instead of the Viterbi-smoothed one. Default: smoothed.")
@click.option("--batch-size", required=False, type=click.IntRange(1, 65535), default=64, help="Utterances measured together. Default 64.")
def prosody_export(ctx, speech_dir, results_dir=None, no_smooth_pitch=False, batch_size=64):
    """Measure the train / val / test manifests on the GPU (pitch, intensity, jitter, shimmer, noise-to-harmonics ratio, rate) and
    write them with the raw and the speaker- and dataset-normalised control columns, plus prosody_norm.json and
    prosody_dropped.csv.  Needs no checkpoint."""
    c = ctx.obj["config"]
    if c is None:
        raise click.UsageError("prosody-export needs --config: it names the manifests (dataset.train / val / test)")
    if not isinstance(c.get("dataset"), dict) or not c["dataset"].get("train"):
        raise click.UsageError("prosody-export: the config names no dataset.train: the statistics come from the train manifest")
    from tacotron2_amd.run.prosody_export import ProsodyExportError, do_prosody_export
    try:
        do_prosody_export(dataset_config=c["dataset"], extensions_config=c["extensions"], device=ctx.obj["device"],
                          speech_dir=speech_dir, results_dir=results_dir, smooth_pitch=not no_smooth_pitch, batch_size=batch_size,
                          name=c.get("training", {}).get("name", "corpus"))
    except ProsodyExportError as e:
        raise click.ClickException(str(e)) from None


if __name__ == "__main__":
    main(obj={})
