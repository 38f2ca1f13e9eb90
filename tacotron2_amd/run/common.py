"""Config handling shared by the drivers: the reference's four-section JSON (main.py:95-99) with the staleness rules of
SURVEY.md section 5: `char_embedding_dim` is an alias of `encoded_dim`; missing `extensions.*` sections are inactive.  And what
the decoding drivers (say, test, test-correlation) share: the loader, the text encoding, the free-running call, `say`'s frame rule."""
from __future__ import annotations

import json

# the resolvers of an option against its config key live in options; run.common.<name> is the same object
from ..options import (decode_settings, decode_settings_of, guided_attention_setting, loss_options_setting,  # noqa: F401
                       optimizer_options_setting, stop_threshold_setting, train_forward_attention_setting)


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


# (torch is imported where it is used: main.py imports this module, and a usage error must not wait for it)
def sample_rate(pre: dict) -> int:
    """The sample rate of a `dataset.preprocessing` section."""
    return int(pre.get("sample_rate", 22050))


def use_ema_setting(model_config: dict, override=None) -> bool:
    """Decode from the EMA weights of the checkpoint: `override` (True for the --ema flag, None without it) wins over
    `"model": {"use_ema": true}`; default off.  A value that is not a bool raises ValueError."""
    v = override if override is not None else model_config.get("use_ema", False)
    if not isinstance(v, bool):
        raise ValueError(f"model.use_ema must be true or false, got {v!r}")
    return v


def load_decode_model(dataset_config: dict, training_config: dict, model_config: dict, extensions_config: dict, checkpoint: str, dev,
                      random_seed=None, attention_window=None, forward_attention=None, stop_threshold=None, ema=None, **model_overrides):
    """The checkpoint as a TTSModel in eval mode, built with model_kwargs of the config (model_overrides on top), seeded with
    random_seed if there is one, and with decode_settings of the three options on the three attributes free_run reads them from.
    ema (use_ema_setting): the weights are the checkpoint's EMA weights; a file without them is an error that names it."""
    from ..model.tts_model import TTSModel
    cfg = dict(dataset=dataset_config, training=training_config, model=model_config, extensions=extensions_config)
    model = TTSModel.load_from_checkpoint(checkpoint, device=dev, use_ema=use_ema_setting(model_config, ema),
                                          **dict(model_kwargs(cfg), **model_overrides))
    model.eval()
    if random_seed is not None:
        model.tacotron2._seed = int(random_seed)
    model.attention_window, model.forward_attention, model.stop_threshold = decode_settings(
        model_config, attention_window, forward_attention, stop_threshold)
    return model


def pad_ids(ids: list, dev):
    """Encoded texts -> (chars (B, longest) int64, zero-padded; lens (B,) int64), both on dev."""
    import torch
    return torch.nn.utils.rnn.pad_sequence(ids, batch_first=True).to(dev), torch.tensor([len(i) for i in ids], dtype=torch.int64, device=dev)


def encode_texts(enc, texts, dev=None):
    """(ids - one int64 host tensor per text, enc.encode of it -, chars, lens): pad_ids of all of them as one batch, or None and
    None without a device, for a driver that pads batch by batch."""
    import torch
    ids = [torch.tensor(enc.encode(t), dtype=torch.int64) for t in texts]
    return (ids, *(pad_ids(ids, dev) if dev is not None else (None, None)))


def free_run(model, chars, lens, max_len: int, **conditioning):
    """The free-running decode of a padded batch under the settings that are on the model -> (post, gates, align)."""
    import torch
    with torch.no_grad():
        return model(chars_idx=chars, chars_idx_len=lens, teacher_forcing=False, max_len_override=max_len,
                     **decode_settings_of(model).kwargs(), **conditioning)[1:]


def emitted_frames(gates, n_emitted: int):
    """(frames: List[int], stopped: List[bool]): `say`'s frames per utterance of a decode with n_emitted frames, and whether it stopped.
    run/say.py:155,161 keeps mel_spectrogram_post[:, :-1]: all emitted frames but the last.  The stop frame itself is already
    masked (gate -1000 from `lengths` on), so an utterance that stopped keeps its `lengths` = n - 1 frames; one that ran into
    max_len without stopping has n unmasked frames and loses the last one, as in the reference.  (A stop threshold changes
    `lengths`, not this rule: it reads the mask, never a logit's sign.)  Counted where gates (B, n, 1) lives; one vector is read."""
    valid = (gates[:, :, 0] != -1000.0).sum(1).cpu().tolist()
    return [max(min(v, n_emitted - 1), 1) for v in valid], [v < n_emitted for v in valid]
