"""Config handling shared by train/say: the reference's four-section JSON (main.py:95-99) with the staleness rules of
SURVEY.md section 5: `char_embedding_dim` is an alias of `encoded_dim`; missing `extensions.*` sections are inactive."""
from __future__ import annotations

import json


def load_config(path: str) -> dict:
    with open(path) as f:
        cfg = json.load(f)
    cfg.setdefault("extensions", {})
    ext = cfg["extensions"]
    ext.setdefault("speaker_tokens", {"active": False})
    ext.setdefault("controls", {"active": False})
    ext.setdefault("descriptions", {"bert_embeddings": False, "finetuneable": False})
    return cfg


def model_kwargs(cfg: dict) -> dict:
    """kwargs for TTSModel from (dataset, training, model, extensions), as run/train.py:176-227 derives them."""
    ds, tr, md, ext = cfg["dataset"], cfg["training"], cfg["model"], cfg["extensions"]
    pre = ds["preprocessing"]
    args = dict(md.get("args", {}))
    if "char_embedding_dim" in args:
        args["encoded_dim"] = args.pop("char_embedding_dim")
    ctl = bool(ext["controls"].get("active"))          # run/train.py:176-180: one control per listed feature column
    args.update(controls=ctl, controls_dim=len(ext["controls"].get("features", [])) if ctl else 0)
    spk = ext["speaker_tokens"].get("active", False)
    max_steps = tr.get("args", {}).get("max_steps", 100000)
    return dict(lr=tr["lr"], weight_decay=tr["weight_decay"],
                num_chars=len(pre["allowed_chars"]) + (pre.get("end_token") is not None),
                num_mels=pre.get("num_mels", 80), speaker_tokens=spk,
                num_speakers=ext["speaker_tokens"].get("num_speakers", 1) if spk else 1,
                scheduler_milestones=[int(x * max_steps) for x in md.get("scheduler_milestones", [])], **args)


def train_forward_attention_setting(training_config: dict, override=None) -> bool:
    """Forward attention under teacher forcing (training, validation, train-mel-export): `override` (True for the
    `--forward-attention` flag of `main.py train`, None without it) wins over `"training": {"forward_attention": true}`; default off.
    A value that is not a bool raises ValueError."""
    from ..engine import check_forward_attention
    if override is not None:
        return check_forward_attention(override)
    return check_forward_attention(training_config.get("forward_attention", False))


def loss_options_setting(training_config: dict, mel=None, masked=None, stop_weight=None):
    """(mel, masked, stop_weight) of the training loss (engine.check_loss_options): each of `mel` (--mel-loss), `masked` (True / False for
    --masked-loss / --no-masked-loss) and `stop_weight` (--stop-weight) wins, when it is not None, over its key of
    `"training": {"loss": {"mel": "l1+l2", "masked": true, "stop_weight": 8.0}}`; any key may be left out ("l2", false, 1.0: the
    reference's loss).  A section of another form or a bad value raises ValueError naming it."""
    from ..engine import check_loss_options
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
    from ..engine import check_stop_threshold
    return check_stop_threshold(override if override is not None else model_config.get("stop_threshold", 0.5))


def guided_attention_setting(training_config: dict, override=None):
    """(sigma, alpha) of the guided-attention loss, or None when it is off: `override` (the --guided-attention option) wins over
    `"training": {"guided_attention": {"sigma": 0.4, "alpha": 1.0}}` (either key may be left out: 0.4 and 1.0).  A section of
    another form, sigma <= 0 or alpha < 0 raises ValueError."""
    from ..engine import check_guided_attention
    if override is not None:
        return check_guided_attention(override)
    sec = training_config.get("guided_attention")
    if sec is None or sec is False:
        return None
    if not isinstance(sec, dict) or set(sec) - {"sigma", "alpha"}:
        raise ValueError('training.guided_attention must be an object with the keys "sigma" and "alpha" '
                         f'(e.g. {{"sigma": 0.4, "alpha": 1.0}}), got {sec!r}')
    return check_guided_attention((sec.get("sigma", 0.4), sec.get("alpha", 1.0)))
