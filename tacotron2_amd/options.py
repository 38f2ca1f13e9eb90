"""The option checks of the Python layer and the settings resolved from them, each rule written once and importable without torch
or the library: a usage error of the command line costs no more than this module.  check_* return a value's checked form or raise
ValueError; *_setting resolve "the option wins, else the config's key, else the default"; DecodeSettings is what a free-running
decode is configured by.  engine and run.common serve every name as before: engine.check_stop_threshold is options.check_stop_threshold."""
from __future__ import annotations

import ctypes
import math
import numbers
from typing import NamedTuple, Optional, Tuple


def check_attention_window(window):
    """None, or (back, fwd) as two integers >= 0 -> the same as a tuple of ints; anything else raises ValueError."""
    if window is None:
        return None
    try:
        back, fwd = window
    except (TypeError, ValueError):
        raise ValueError(f"attention_window must be (back, fwd), got {window!r}") from None
    for v in (back, fwd):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
            raise ValueError(f"attention_window must be two integers >= 0, got {window!r}")
    return int(back), int(fwd)


def check_forward_attention(forward, window=None):
    """True or False -> the same; anything else, or True together with an attention window, raises ValueError."""
    if not isinstance(forward, bool):
        raise ValueError(f"forward_attention must be True or False, got {forward!r}")
    if forward and window is not None:
        raise ValueError("forward_attention does not compose with attention_window: use one of the two")
    return forward


def check_rate(p, name: str, closed: bool = False) -> float:
    """A probability in [0, 1) - or [0, 1] with closed=True - as a float; anything else is a ValueError that names the option."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= float(p) < 1.0 or (closed and float(p) == 1.0)):
        raise ValueError(f"{name} must be a number in [0, 1{']' if closed else ')'}, got {p!r}")
    return float(p)


def check_guided_attention(guided):
    """None, or (sigma, alpha) of the guided-attention loss as two real numbers, sigma > 0 and alpha >= 0 -> a tuple of floats;
    anything else raises ValueError."""
    if guided is None:
        return None
    try:
        sigma, alpha = guided
    except (TypeError, ValueError):
        raise ValueError(f"guided_attention must be (sigma, alpha), got {guided!r}") from None
    for v in (sigma, alpha):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != v or abs(v) == float("inf"):
            raise ValueError(f"guided_attention must be two finite numbers (sigma, alpha), got {guided!r}")
    if sigma <= 0 or alpha < 0:
        raise ValueError(f"guided_attention needs sigma > 0 and alpha >= 0, got {guided!r}")
    return float(sigma), float(alpha)


MEL_LOSSES = ("l2", "l1", "l1+l2")       # T2LossOpts.mel_loss = the index
LOSS_DEFAULTS = ("l2", False, 1.0)


def check_loss_options(loss):
    """None, a dict with any of the keys "mel" / "masked" / "stop_weight", or a 3-tuple (mel, masked, stop_weight) -> the tuple
    (mel in MEL_LOSSES, masked bool, stop_weight float > 0), missing keys at their defaults ("l2", False, 1.0: the reference's loss);
    anything else raises ValueError naming the offending value."""
    if loss is None:
        return LOSS_DEFAULTS
    if isinstance(loss, dict):
        unknown = sorted(set(loss) - {"mel", "masked", "stop_weight"})
        if unknown:
            raise ValueError(f"loss options: unknown key {unknown[0]!r} (known: mel, masked, stop_weight)")
        mel, masked, w = (loss.get(k, dflt) for k, dflt in zip(("mel", "masked", "stop_weight"), LOSS_DEFAULTS))
    else:
        try:
            mel, masked, w = loss
        except (TypeError, ValueError):
            raise ValueError(f"loss options must be a dict or (mel, masked, stop_weight), got {loss!r}") from None
    if not isinstance(mel, str) or mel not in MEL_LOSSES:
        raise ValueError(f"loss options: mel must be one of {', '.join(MEL_LOSSES)}, got {mel!r}")
    if not isinstance(masked, bool):
        raise ValueError(f"loss options: masked must be True or False, got {masked!r}")
    if isinstance(w, bool) or not isinstance(w, numbers.Real) or w != w or abs(w) == float("inf") or w <= 0:
        raise ValueError(f"loss options: stop_weight must be a finite number > 0, got {w!r}")
    if not 0.0 < float(ctypes.c_float(float(w)).value) < float("inf"):
        raise ValueError(f"loss options: stop_weight must be a finite float32 > 0, got {w!r}")
    return mel, masked, float(w)


def check_stop_threshold(tau) -> float:
    """A stop threshold 0 < tau < 1 as a float (0.5: the reference's rule); anything else raises ValueError."""
    if isinstance(tau, bool) or not isinstance(tau, numbers.Real) or not 0.0 < float(tau) < 1.0:
        raise ValueError(f"stop_threshold must be a number with 0 < threshold < 1, got {tau!r}")
    return float(tau)


def stop_logit(tau: float) -> float:
    """logit(tau) = log(tau / (1 - tau)) formed in double and rounded to float32: the ONE value the decode loop's flags, the scan
    and the drivers' length rule compare against.  0.5 gives 0.0, the reference's comparison."""
    v = float(ctypes.c_float(math.log(tau / (1.0 - tau))).value)
    if v != v or abs(v) == float("inf"):
        raise ValueError(f"stop_threshold {tau!r} has no finite float32 logit")
    return v


def train_forward_attention_setting(training_config: dict, override=None) -> bool:
    """Forward attention under teacher forcing (training, validation, train-mel-export): `override` (True for the
    `--forward-attention` flag of `main.py train`, None without it) wins over `"training": {"forward_attention": true}`; default off.
    A value that is not a bool raises ValueError."""
    return check_forward_attention(override if override is not None else training_config.get("forward_attention", False))


def loss_options_setting(training_config: dict, mel=None, masked=None, stop_weight=None):
    """(mel, masked, stop_weight) of the training loss (check_loss_options): each of `mel` (--mel-loss), `masked` (True / False for
    --masked-loss / --no-masked-loss) and `stop_weight` (--stop-weight) wins, when it is not None, over its key of
    `"training": {"loss": {"mel": "l1+l2", "masked": true, "stop_weight": 8.0}}`; any key may be left out ("l2", false, 1.0: the
    reference's loss).  A section of another form or a bad value raises ValueError naming it."""
    sec = training_config.get("loss")
    if sec is None:
        sec = {}
    if not isinstance(sec, dict):
        raise ValueError('training.loss must be an object with the keys "mel", "masked" and "stop_weight" '
                         f'(e.g. {{"mel": "l1+l2", "masked": true, "stop_weight": 8.0}}), got {sec!r}')
    sec = dict(sec)
    for key, v in (("mel", mel), ("masked", masked), ("stop_weight", stop_weight)):
        if v is not None:
            sec[key] = v
    return check_loss_options(sec)


def stop_threshold_setting(model_config: dict, override=None) -> float:
    """The decode stop threshold 0 < tau < 1: `override` (the --stop-threshold option) wins over `"model": {"stop_threshold": 0.4}`;
    default 0.5, the reference's rule.  Anything else raises ValueError."""
    return check_stop_threshold(override if override is not None else model_config.get("stop_threshold", 0.5))


def guided_attention_setting(training_config: dict, override=None):
    """(sigma, alpha) of the guided-attention loss, or None when it is off: `override` (the --guided-attention option) wins over
    `"training": {"guided_attention": {"sigma": 0.4, "alpha": 1.0}}` (either key may be left out: 0.4 and 1.0).  A section of
    another form, sigma <= 0 or alpha < 0 raises ValueError."""
    if override is not None:
        return check_guided_attention(override)
    sec = training_config.get("guided_attention")
    if sec is None or sec is False:
        return None
    if not isinstance(sec, dict) or set(sec) - {"sigma", "alpha"}:
        raise ValueError('training.guided_attention must be an object with the keys "sigma" and "alpha" '
                         f'(e.g. {{"sigma": 0.4, "alpha": 1.0}}), got {sec!r}')
    return check_guided_attention((sec.get("sigma", 0.4), sec.get("alpha", 1.0)))


class DecodeSettings(NamedTuple):
    """What a free-running decode is configured by; the defaults are the reference's decode (the whole text, no forward attention,
    stop below 0.5) and are written here only."""
    attention_window: Optional[Tuple[int, int]] = None
    forward_attention: bool = False
    stop_threshold: float = 0.5

    def kwargs(self) -> dict:
        """The three keyword arguments of Tacotron2.forward."""
        return self._asdict()


def decode_settings(model_config: dict, attention_window=None, forward_attention=None, stop_threshold=None) -> DecodeSettings:
    """Each argument (the command line's option; None without it) wins over its key of the config's `model` section
    (`attention_window`: [back, fwd]; `forward_attention`: a bool; `stop_threshold`: 0 < tau < 1), which wins over the default.
    Checked in this order: the window, forward attention against the window, the threshold; a bad value raises ValueError."""
    window = check_attention_window(attention_window if attention_window is not None else model_config.get("attention_window"))
    forward = forward_attention if forward_attention is not None else model_config.get("forward_attention", False)
    return DecodeSettings(window, check_forward_attention(forward, window), stop_threshold_setting(model_config, stop_threshold))


def decode_settings_of(model) -> DecodeSettings:
    """The settings that are on a model (TTSModel's three attributes; load_decode_model puts them there); an object that lacks one
    decodes with its default."""
    return DecodeSettings(*(getattr(model, name, default) for name, default in DecodeSettings()._asdict().items()))


LR_SCHEDULES = ("multistep", "exponential", "noam")


class OptimizerOptions(NamedTuple):
    """The options of the update (Trainer(optimizer_options=...)); the defaults are the reference's optimiser - Adam with
    L2 in the gradient, clip at 1.0, MultiStepLR, no EMA - and are written here only.  ema_decay 0 switches the EMA off; grad_clip 0
    the clip."""
    decoupled_weight_decay: bool = False
    ema_decay: float = 0.0
    grad_clip: float = 1.0
    schedule: str = "multistep"
    warmup_steps: int = 0
    decay_start: int = 0
    decay_steps: int = 0
    min_lr: float = 0.0


def _opt_number(v, key: str, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != v or abs(v) == float("inf"):
        raise ValueError(f"optimizer options: {key} must be {what}, got {v!r}")
    return float(v)


def _opt_count(v, key: str) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
        raise ValueError(f"optimizer options: {key} must be an integer >= 0, got {v!r}")
    return int(v)


def check_optimizer_options(opts=None, lr: Optional[float] = None, milestones=()) -> OptimizerOptions:
    """None, a dict with any of OptimizerOptions' keys, or an OptimizerOptions -> the checked tuple, missing keys at their defaults.
    `lr` is the base learning rate the `exponential` schedule's min_lr is held against (None: that comparison is left out) and
    `milestones` the MultiStepLR milestones, which `noam` does not combine with.  Each refusal is a ValueError that names the key."""
    if opts is None:
        opts = {}
    if isinstance(opts, OptimizerOptions):
        opts = opts._asdict()
    if not isinstance(opts, dict):
        raise ValueError(f"optimizer options must be a dict or OptimizerOptions, got {opts!r}")
    unknown = sorted(set(opts) - set(OptimizerOptions._fields))
    if unknown:
        raise ValueError(f"optimizer options: unknown key {unknown[0]!r} (known: {', '.join(OptimizerOptions._fields)})")
    o = dict(OptimizerOptions()._asdict(), **opts)
    if not isinstance(o["decoupled_weight_decay"], bool):
        raise ValueError(f"optimizer options: decoupled_weight_decay must be True or False, got {o['decoupled_weight_decay']!r}")
    ema = _opt_number(o["ema_decay"], "ema_decay", "a number in [0, 1)")
    if not 0.0 <= ema < 1.0 or not float(ctypes.c_float(ema).value) < 1.0:
        raise ValueError(f"optimizer options: ema_decay must be a number in [0, 1) (as a float32 too), got {o['ema_decay']!r}")
    clip = _opt_number(o["grad_clip"], "grad_clip", "a finite number >= 0")
    if clip < 0:
        raise ValueError(f"optimizer options: grad_clip must be >= 0 (0 switches the clip off), got {o['grad_clip']!r}")
    schedule = o["schedule"]
    if not isinstance(schedule, str) or schedule not in LR_SCHEDULES:
        raise ValueError(f"optimizer options: schedule must be one of {', '.join(LR_SCHEDULES)}, got {schedule!r}")
    warmup, start, steps = (_opt_count(o[k], k) for k in ("warmup_steps", "decay_start", "decay_steps"))
    min_lr = _opt_number(o["min_lr"], "min_lr", "a finite number >= 0")
    if min_lr < 0:
        raise ValueError(f"optimizer options: min_lr must be >= 0, got {o['min_lr']!r}")
    if schedule == "exponential":
        if steps < 1:
            raise ValueError(f"optimizer options: the exponential schedule needs decay_steps >= 1, got {steps!r}")
        if not min_lr > 0 or (lr is not None and min_lr > float(lr)):
            raise ValueError(f"optimizer options: the exponential schedule needs 0 < min_lr <= lr"
                             f"{'' if lr is None else f' = {lr!r}'}, got min_lr {o['min_lr']!r}")
    if schedule == "noam":
        if warmup < 1:
            raise ValueError(f"optimizer options: the noam schedule needs warmup_steps >= 1, got {warmup!r}")
        if len(list(milestones)) > 0:
            raise ValueError("optimizer options: the noam schedule does not combine with scheduler milestones "
                             f"(schedule 'noam', milestones {list(milestones)!r})")
    return OptimizerOptions(o["decoupled_weight_decay"], ema, clip, schedule, warmup, start, steps, min_lr)


def optimizer_options_setting(training_config: dict, lr: Optional[float] = None, milestones=(), **overrides) -> OptimizerOptions:
    """The options of the update: each keyword of `overrides` that is not None (the command line: --ema-decay, --decoupled-weight-decay /
    --no-decoupled-weight-decay, --grad-clip, --lr-schedule, --lr-warmup, --lr-decay) wins over its key of
    `"training": {"optimizer": {"ema_decay": 0.999, "decoupled_weight_decay": true, ...}}`, which wins over the default.  A section of
    another form or a bad value raises ValueError naming it (check_optimizer_options)."""
    sec = training_config.get("optimizer")
    if sec is None:
        sec = {}
    if not isinstance(sec, dict):
        raise ValueError(f"training.optimizer must be an object with keys among {', '.join(OptimizerOptions._fields)}, got {sec!r}")
    sec = dict(sec)
    for key, v in overrides.items():
        if key not in OptimizerOptions._fields:
            raise ValueError(f"optimizer options: unknown key {key!r}")
        if v is not None:
            sec[key] = v
    return check_optimizer_options(sec, lr=lr, milestones=milestones)


def lr_at(base_lr: float, milestones, opts: OptimizerOptions, t: int) -> float:
    """The learning rate of the 0-based scheduler step t, in Python floats (Trainer.lr_at):
    multistep base * 0.1^(milestones passed); exponential base until decay_start, then base * (min_lr / base)^min(1, (t - start) / steps);
    both times min(1, (t + 1) / warmup_steps) under a warm-up; noam base * min((t + 1) / W, sqrt(W / (t + 1))), base the peak at step W."""
    if opts.schedule == "noam":
        W = opts.warmup_steps
        return base_lr * min((t + 1) / W, math.sqrt(W / (t + 1)))
    if opts.schedule == "exponential":
        lr = base_lr if t < opts.decay_start else \
            base_lr * (opts.min_lr / base_lr) ** min(1.0, (t - opts.decay_start) / opts.decay_steps)
    else:
        lr = base_lr * (0.1 ** sum(1 for m in milestones if t >= m))
    if opts.warmup_steps > 0:
        lr = lr * min(1.0, (t + 1) / opts.warmup_steps)
    return lr


def ema_decay_at(decay: float, k: int) -> float:
    """The effective decay of the k-th EMA update, k = 1, 2, ...: min(D, (1 + k) / (10 + k)), TensorFlow's num_updates rule - without
    it a D of 0.9999 holds the random initial weights for 10 000 steps."""
    return min(float(decay), (1.0 + k) / (10.0 + k))
