"""do_say (run/say.py:25-179): text -> ids -> checkpoint -> forward(teacher_forcing=False, max_len_override=5000) ON THE GPU
(the reference runs this on CPU at batch 1; here any number of texts is decoded as one batch, up to 64 per group) ->
log-mel written as .npy, or - when the output name ends in .wav - Griffin-Lim audio (tacotron2_amd/vocoder.py, the branch
run/say.py:161-171 takes without a HiFi-GAN checkpoint), or HiFi-GAN audio with --hifi-gan-checkpoint (tacotron2_amd/hifigan.py,
run/say.py:66-86,153-159)."""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from ..datasets.text import TextEncoder
from ..engine import check_attention_window, check_forward_attention
from ..model.tts_model import TTSModel
from .common import model_kwargs, stop_threshold_setting


def load_description(description: Optional[str], dim: int, n: int, dev) -> torch.Tensor:
    """--description of `say`.  The reference encodes the description TEXT with google-bert/bert-base-uncased (run/say.py:93-116:
    tokenizer + BertModel -> pooler_output, (1, 768)) - remote weights, unavailable offline.  What the model consumes is only that
    vector, and the dataset path already feeds it from precomputed files (datasets/tts_dataset.py:277-287: torch.load of a `.pt`
    per utterance, zeros when absent).  So: a PATH to a precomputed embedding - `.pt` (weights-only load) or `.npy`, (dim,) or
    (1, dim) - is used as the dataset uses it; no description = zeros; raw text still needs BERT and is refused with that message."""
    import os
    if description is None:
        return torch.zeros(n, dim, device=dev)
    if not (os.path.isfile(description) and description.endswith((".pt", ".npy"))):
        raise NotImplementedError("--description with raw text needs the remote google-bert/bert-base-uncased weights (unavailable "
                                  "offline); pass the path of a precomputed pooler_output embedding (.pt or .npy, shape "
                                  f"({dim},)) instead, as the dataset manifests do")
    if description.endswith(".npy"):
        v = torch.from_numpy(np.load(description, allow_pickle=False))
    else:
        v = torch.load(description, map_location="cpu", weights_only=True)
    v = torch.as_tensor(v).float().reshape(-1)
    assert v.numel() == dim, f"--description embedding has {v.numel()} values, the model expects {dim}"
    return v.to(dev).unsqueeze(0).repeat(n, 1).contiguous()


def duration_records(model, enc: TextEncoder, texts: List[str], align: torch.Tensor, lens: torch.Tensor, frames: List[int],
                     sample_rate: int, hop: int = 256) -> list:
    """One dict per text: the monotonic path through the decode's alignments (one row per decoder step; r frames per step with a
    reduction factor) over the text's written frames -> per-symbol frame counts and times."""
    flen = torch.tensor(frames, dtype=torch.int32, device=align.device)
    dur, stats = model.tacotron2._engine.durations(align, lens, flen, mode="monotonic")
    dur, stats = dur.cpu().numpy(), stats.cpu().numpy()
    out = []
    for b, t in enumerate(texts):
        sym = list(enc.clean(t))
        fr = [int(x) for x in dur[b, :len(sym)]]
        ends = np.cumsum(fr)
        out.append(dict(symbols=sym, frames=fr, start_s=[float((e - f) * hop / sample_rate) for e, f in zip(ends, fr)],
                        end_s=[float(e * hop / sample_rate) for e in ends], focus_rate=float(stats[b, 0]),
                        feasible=bool(stats[b, 2] != 0)))
    return out


def write_durations(path: str, model, enc: TextEncoder, texts: List[str], align: torch.Tensor, lens: torch.Tensor,
                    frames: List[int], sample_rate: int, hop: int = 256) -> list:
    """`say --durations-out`: duration_records of the decode, as a JSON list."""
    import json
    out = duration_records(model, enc, texts, align, lens, frames, sample_rate, hop)
    with open(path, "w") as f:
        json.dump(out, f)
    return out


def load_say_model(dataset_config: dict, training_config: dict, model_config: dict, extensions_config: dict, dev, checkpoint: str,
                   random_seed: Optional[int], attention_window, forward_attention: Optional[bool], stop_threshold: Optional[float]):
    """The checkpoint in eval mode with the decode settings of `say` on it (seed, attention window, forward attention, stop
    threshold; None takes the config's): what do_say and do_say_document share."""
    cfg = dict(dataset=dataset_config, training=training_config, model=model_config, extensions=extensions_config)
    model = TTSModel.load_from_checkpoint(checkpoint, device=dev, **model_kwargs(cfg))
    model.eval()
    if random_seed is not None:
        model.tacotron2._seed = int(random_seed)
    if attention_window is None:       # the config's model.attention_window, if any (as load_test_model does)
        attention_window = model_config.get("attention_window")
    model.attention_window = check_attention_window(attention_window)
    if forward_attention is None:      # likewise the config's model.forward_attention (a bool)
        forward_attention = model_config.get("forward_attention", False)
    model.forward_attention = check_forward_attention(forward_attention, model.attention_window)
    model.stop_threshold = stop_threshold_setting(model_config, stop_threshold)
    return model


def conditioning(model, n: int, dev, speaker_id: Optional[int], controls: Optional[str], description: Optional[str]) -> dict:
    """The speaker, description and control inputs of n texts, as the model's keyword arguments."""
    kw = {}
    if model.speaker_tokens:
        kw["speaker_id"] = torch.full((n,), int(speaker_id or 0), dtype=torch.int32, device=dev)
    if model.description_embeddings:
        dim = model.hparams["description_embeddings_dim"]
        kw["description_embeddings"] = load_description(description, dim, n, dev)
    if model.controls:      # run/say.py:113-118: comma-separated values; the CLI help promises zeros by default
        n_ctl = int(model.hparams["controls_dim"])
        vals = [float(x) for x in controls.split(",")] if controls else [0.0] * n_ctl
        assert len(vals) == n_ctl, f"--controls needs {n_ctl} comma-separated values"
        kw["controls"] = torch.tensor([vals] * n, dtype=torch.float32, device=dev)
    return kw


def do_say(dataset_config: dict, training_config: dict, model_config: dict, extensions_config: dict, device: int,
           checkpoint: str, text: Union[str, List[str]], output: str, hifi_gan_checkpoint: Optional[str] = None,
           random_seed: Optional[int] = None, speaker_id: Optional[int] = None, controls: Optional[str] = None,
           description: Optional[str] = None, max_len: int = 5000, attention_window: Optional[Tuple[int, int]] = None,
           forward_attention: Optional[bool] = None, durations_out: Optional[str] = None,
           stop_threshold: Optional[float] = None, out_sample_rate: Optional[int] = None):
    """out_sample_rate: R Hz - with a `.wav` target (HiFi-GAN or Griffin-Lim) the vocoded waveform is resampled from the model's
    rate to R on the device (datasets/resample.py) before it is written, and the header carries R; `durations_out`
    times stay in model frames.  None: the model's rate, nothing changes.
    stop_threshold: 0 < tau < 1, the stop probability below which an utterance ends (Tacotron2.forward); None takes the config's
    `model.stop_threshold` if there is one, else 0.5, the reference's rule.
    durations_out: a path - character timestamps of the decode are written there as a JSON list with one object per text:
    `symbols` (the encoded sequence, end token included), `frames` per symbol (the monotonic path through the decode's own
    alignments, Engine.durations; they sum to the frames of the mel that is written), `start_s` / `end_s` per symbol (hop of 256
    samples at the dataset's sample rate), `focus_rate` and `feasible`.  None: nothing of this runs."""
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    pre = dataset_config["preprocessing"]
    to_rate = None
    if out_sample_rate is not None:
        if hifi_gan_checkpoint is None and not output.endswith(".wav"):
            raise ValueError(f"--out-sample-rate needs a .wav target or a HiFi-GAN checkpoint, got {output!r}: a log-mel has no rate")
        from ..datasets.resample import Resampler, plan
        plan(int(pre.get("sample_rate", 22050)), int(out_sample_rate))      # (refuses a bad rate before anything is decoded)
        resampler = Resampler(int(out_sample_rate), dev)
        to_rate = lambda wav, sr: torch.from_numpy(resampler.one(wav.detach().float().cpu().numpy(), sr))
    enc = TextEncoder(pre["allowed_chars"], pre.get("end_token"), expand_abbrev=False)   # run/say.py: no abbreviations
    texts = [text] if isinstance(text, str) else list(text)
    ids = [torch.tensor(enc.encode(t), dtype=torch.int64) for t in texts]
    chars = torch.nn.utils.rnn.pad_sequence(ids, batch_first=True).to(dev)
    lens = torch.tensor([len(i) for i in ids], dtype=torch.int64, device=dev)
    model = load_say_model(dataset_config, training_config, model_config, extensions_config, dev, checkpoint, random_seed,
                           attention_window, forward_attention, stop_threshold)
    kw = conditioning(model, len(texts), dev, speaker_id, controls, description)
    with torch.no_grad():
        _, post, gates, align = model(chars_idx=chars, chars_idx_len=lens, teacher_forcing=False, max_len_override=max_len,
                                      attention_window=model.attention_window, forward_attention=model.forward_attention,
                                      stop_threshold=model.stop_threshold, **kw)
    post = post.cpu().numpy()
    # run/say.py:155,161 keeps mel_spectrogram_post[:, :-1]: all emitted frames but the last.  The stop frame itself is already
    # masked (gate -1000 from `lengths` on), so an utterance that stopped keeps its `lengths` = n - 1 frames; one that ran into
    # max_len without stopping has n unmasked frames and loses the last one, as in the reference.  (A stop threshold changes
    # `lengths`, not this rule: it reads the mask, never a logit's sign.)
    valid = (gates.cpu().numpy()[:, :, 0] != -1000.0).sum(1)
    n_emitted = post.shape[1]
    mels = [post[b, :max(min(int(valid[b]), n_emitted - 1), 1)] for b in range(len(texts))]
    if durations_out is not None:
        write_durations(durations_out, model, enc, texts, align, lens, [len(m) for m in mels], int(pre.get("sample_rate", 22050)))
    if hifi_gan_checkpoint is not None:
        # run/say.py:66-86,153-159: generator(mel_post[:, :-1].swapaxes(1, 2)) -> waveform, written as audio whatever the name
        from ..hifigan import Generator
        from ..vocoder import write_wav
        sr = int(pre.get("sample_rate", 22050))
        gen = Generator.from_checkpoint(hifi_gan_checkpoint, device=dev)
        for i, m in enumerate(mels):
            wav = gen(torch.from_numpy(np.ascontiguousarray(m.T)).to(dev))[0, 0].cpu()
            name = output if isinstance(text, str) else f"{output.rsplit('.', 1)[0]}_{i}.wav"
            if to_rate is not None:
                write_wav(name, to_rate(wav, sr), int(out_sample_rate))
            else:
                write_wav(name, wav, sr)
        return mels
    if output.endswith(".wav"):
        from ..vocoder import GriffinLim, write_wav
        sr = int(pre.get("sample_rate", 22050))
        gl = GriffinLim(n_mels=post.shape[2], sample_rate=sr, device=dev)
        for i, m in enumerate(mels):
            name = output if isinstance(text, str) else f"{output[:-4]}_{i}.wav"
            wav = gl.mel_to_audio(torch.from_numpy(m), seed=int(random_seed or 0))
            if to_rate is not None:
                write_wav(name, to_rate(wav, sr), int(out_sample_rate))
            else:
                write_wav(name, wav, sr)
        return mels
    np.save(output, mels[0] if isinstance(text, str) else np.array(mels, dtype=object), allow_pickle=not isinstance(text, str))
    return mels


# ---- say --text-file: a document split into pieces, decoded side by side, joined on the device ----------------------------
PAUSES = dict(sentence=0.25, clause=0.12, paragraph=0.60, end=0.0)      # seconds behind a piece; product defaults, not measurements
KEEP_S = 0.020                                                          # audio kept in front of and behind a piece's trimmed span


def say_document(model, pieces, enc: TextEncoder, pre: dict, vocoder, max_len: int = 5000, batch_size: int = 64, pauses: dict = PAUSES,
                 trim: bool = True, level: bool = False, fade_ms: float = 5.0, speaker_id: Optional[int] = None,
                 controls: Optional[str] = None, description: Optional[str] = None, random_seed: Optional[int] = None,
                 durations: bool = False):
    """Pieces (datasets.document.Piece, or a text, which is split at the defaults) -> one waveform on the model's device.
    The pieces are sorted by encoded length and decoded in chunks of batch_size through the model's free-running forward, with the
    decode settings that are on the model (attention_window, forward_attention, stop_threshold; none, off and 0.5 where it has
    none).  `vocoder` is a loaded
    hifigan.Generator - each chunk's PADDED batch is vocoded in one call and cut at frames * 256, as `test` does, so a row's last
    samples see the padding inside the generator's receptive field, which `say --text` of one piece does not - or a
    vocoder.GriffinLim, which runs per piece.  The rows go back into document order in one padded buffer, and one
    analysis.join_audio call trims (dataset.preprocessing's trim_top_db and trim_frame_length, the hop a quarter of it, 20 ms kept
    at both ends), levels, fades and joins them, with pauses[break_after] seconds behind each piece.
    A piece that ran into max_len without stopping is kept, cut there, and marked stopped=False.
    Returns (y (total,) float32, plan - join_audio's, device tensors -, info): info = dict(pieces, frames, stopped, n, pause,
    waveforms - the per-piece device tensors that went into the join -, chunks, join - the keyword arguments of the join_audio
    call -, durations - duration_records per piece, or None)."""
    from .. import analysis
    from ..datasets.document import split_document
    from ..hifigan import Generator
    if isinstance(pieces, str):
        pieces = split_document(pieces, clean=lambda t: enc.clean(t)[:len(enc.clean(t)) - len(enc.end_token or "")])
    pieces = list(pieces)
    if not pieces:
        raise ValueError("say_document: nothing to say - the text has no piece that survives cleaning")
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or not 1 <= batch_size <= 64:
        raise ValueError(f"say_document: batch_size must be an integer in 1 .. 64, got {batch_size!r}")
    dev = next(model.parameters()).device
    sr = int(pre.get("sample_rate", 22050))
    texts = [p.text for p in pieces]
    ids = [torch.tensor(enc.encode(t), dtype=torch.int64) for t in texts]
    order = sorted(range(len(ids)), key=lambda i: (len(ids[i]), i))
    chunks = [order[k:k + batch_size] for k in range(0, len(order), batch_size)]
    P = len(pieces)
    waves, frames, stopped, records = [None] * P, [0] * P, [False] * P, [None] * P
    for ch in chunks:
        chars = torch.nn.utils.rnn.pad_sequence([ids[i] for i in ch], batch_first=True).to(dev)
        lens = torch.tensor([len(ids[i]) for i in ch], dtype=torch.int64, device=dev)
        kw = conditioning(model, len(ch), dev, speaker_id, controls, description)
        with torch.no_grad():
            _, post, gates, align = model(chars_idx=chars, chars_idx_len=lens, teacher_forcing=False, max_len_override=max_len,
                                          attention_window=getattr(model, "attention_window", None),
                                          forward_attention=getattr(model, "forward_attention", False),
                                          stop_threshold=getattr(model, "stop_threshold", 0.5), **kw)
        n_emitted = post.shape[1]
        valid = (gates[:, :, 0] != -1000.0).sum(1).cpu().tolist()             # (do_say's rule: all emitted frames but the last)
        fr = [max(min(int(v), n_emitted - 1), 1) for v in valid]
        if durations:
            for i, rec in zip(ch, duration_records(model, enc, [texts[i] for i in ch], align, lens, fr, sr)):
                records[i] = rec
        if isinstance(vocoder, Generator):
            rows = vocoder(post.transpose(1, 2))[:, 0]                        # the padded batch in one call
            out = [rows[k, :fr[k] * 256] for k in range(len(ch))]
        else:
            out = [torch.as_tensor(vocoder.mel_to_audio(post[k, :fr[k]], seed=int(random_seed or 0))).float().reshape(-1).to(dev)
                   for k in range(len(ch))]
        for k, i in enumerate(ch):
            waves[i], frames[i], stopped[i] = out[k], fr[k], valid[k] < n_emitted
    n = [int(w.numel()) for w in waves]
    buf = torch.zeros(P, max(max(n), 1), dtype=torch.float32, device=dev)
    for i, w in enumerate(waves):
        buf[i, :n[i]] = w
    pause = [int(round(float(pauses[p.break_after]) * sr)) for p in pieces]
    F = int(pre.get("trim_frame_length", 2048))
    join = dict(trim=bool(trim), top_db=float(pre.get("trim_top_db", 60)), frame_length=F, hop_length=max(F // 4, 1),
                keep=int(round(KEEP_S * sr)), fade=int(round(float(fade_ms) * sr / 1000.0)), level=bool(level),
                ceiling=1.0 if level else 0.0)
    y, _, plan = analysis.join_audio(buf, n, pause, **join)
    return y, plan, dict(pieces=pieces, frames=frames, stopped=stopped, n=n, pause=pause, waveforms=waves, chunks=len(chunks),
                         join=join, durations=records if durations else None)


def document_records(info: dict, plan: dict, sample_rate: int) -> list:
    """`say --text-file --durations-out`: one object per piece in document order - piece, paragraph, text; symbols, frames,
    focus_rate, feasible as duration_records gives them; stopped; offset_s, trim_start_s, length_s, pause_s and gain of the join's
    plan; start_s / end_s per symbol in DOCUMENT time: a piece-local time t lies at offset_s + clip(t - trim_start_s, 0, length_s),
    still at the model's rate and its hop of 256."""
    off, s0, length, gain = (plan[k].cpu().tolist() for k in ("off", "s0", "len", "gain"))
    out = []
    for i, (p, rec) in enumerate(zip(info["pieces"], info["durations"])):
        o, t0, ln = off[i] / sample_rate, s0[i] / sample_rate, length[i] / sample_rate
        doc = lambda t: o + min(max(t - t0, 0.0), ln)
        out.append(dict(piece=i, paragraph=p.paragraph_index, text=p.text, symbols=rec["symbols"], frames=rec["frames"],
                        focus_rate=rec["focus_rate"], feasible=rec["feasible"], stopped=bool(info["stopped"][i]), offset_s=o,
                        trim_start_s=t0, length_s=ln, pause_s=info["pause"][i] / sample_rate, gain=float(gain[i]),
                        start_s=[doc(t) for t in rec["start_s"]], end_s=[doc(t) for t in rec["end_s"]]))
    return out


def parse_pauses(spec) -> dict:
    """`--pause SENT,CLAUSE,PARA` in seconds -> the pauses of say_document (the last piece gets 0)."""
    if spec is None:
        return dict(PAUSES)
    try:
        sent, clause, para = (float(x) for x in str(spec).split(","))
        if not all(0.0 <= v < 3600.0 for v in (sent, clause, para)):
            raise ValueError
    except ValueError:
        raise ValueError(f"--pause needs three comma-separated times in seconds (SENT,CLAUSE,PARA), each >= 0, got {spec!r}") from None
    return dict(sentence=sent, clause=clause, paragraph=para, end=0.0)


def do_say_document(dataset_config: dict, training_config: dict, model_config: dict, extensions_config: dict, device: int,
                    checkpoint: str, text_file: str, output: str, hifi_gan_checkpoint: Optional[str] = None,
                    random_seed: Optional[int] = None, speaker_id: Optional[int] = None, controls: Optional[str] = None,
                    description: Optional[str] = None, max_len: int = 5000, attention_window: Optional[Tuple[int, int]] = None,
                    forward_attention: Optional[bool] = None, durations_out: Optional[str] = None,
                    stop_threshold: Optional[float] = None, out_sample_rate: Optional[int] = None, max_chars: int = 190,
                    expand_numbers: bool = False, pause=None, trim: bool = True, level: bool = False, fade_ms: float = 5.0,
                    batch_size: int = 64):
    """`say --text-file`: the file is read, its numbers expanded if asked, split (datasets/document.py) and spoken by say_document;
    the joined waveform is resampled to out_sample_rate if given (one Resampler call) and written by ONE write_wav call.
    durations_out: document_records as a JSON list.  A piece that did not stop is reported on stderr; the exit status stays 0.
    Returns say_document's (y, plan, info), y as written (after resampling)."""
    import json
    import sys
    import time
    from .. import vocoder as V
    from ..datasets.document import expand_numbers as expand, split_document
    from .test import make_vocoders
    if hifi_gan_checkpoint is None and not output.endswith(".wav"):
        raise ValueError(f"--text-file needs a .wav target or a HiFi-GAN checkpoint, got {output!r}: a document has no single log-mel")
    if fade_ms < 0:
        raise ValueError(f"--fade-ms must be >= 0, got {fade_ms!r}")
    pauses = parse_pauses(pause)
    t_start = time.perf_counter()
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    pre = dataset_config["preprocessing"]
    sr = int(pre.get("sample_rate", 22050))
    resampler = None
    if out_sample_rate is not None:
        from ..datasets.resample import Resampler, plan
        plan(sr, int(out_sample_rate))                                      # (refuses a bad rate before anything is decoded)
        resampler = Resampler(int(out_sample_rate), dev)
    enc = TextEncoder(pre["allowed_chars"], pre.get("end_token"), expand_abbrev=False)
    with open(text_file, encoding="utf-8") as f:
        text = f.read()
    if expand_numbers:
        text = expand(text)
    n_end = len(pre.get("end_token") or "")
    pieces = split_document(text, max_chars=max_chars, clean=lambda t: enc.clean(t)[:len(enc.clean(t)) - n_end])
    if not pieces:
        raise ValueError(f"--text-file {text_file!r}: nothing to say - no piece of the text survives cleaning")
    model = load_say_model(dataset_config, training_config, model_config, extensions_config, dev, checkpoint, random_seed,
                           attention_window, forward_attention, stop_threshold)
    gen, gl, _ = make_vocoders(hifi_gan_checkpoint, dict(pre, num_mels=int(model.hparams.get("num_mels", pre.get("num_mels", 80)))), dev)
    y, plan_, info = say_document(model, pieces, enc, pre, gen if gen is not None else gl, max_len=max_len, batch_size=batch_size,
                                  pauses=pauses, trim=trim, level=level, fade_ms=fade_ms, speaker_id=speaker_id, controls=controls,
                                  description=description, random_seed=random_seed, durations=durations_out is not None)
    for i, ok in enumerate(info["stopped"]):
        if not ok:
            print(f"say: piece {i} did not stop within --max-len {max_len} frames and is cut there: {pieces[i].text[:40]!r}", file=sys.stderr)
    if durations_out is not None:
        with open(durations_out, "w") as f:
            json.dump(document_records(info, plan_, sr), f)
    seconds = y.numel() / sr
    if resampler is not None and y.numel() > 0:
        out, n_out = resampler.batch(y[None, :], [int(y.numel())], sr)
        y = out[0, :n_out[0]]
    V.write_wav(output, y, int(out_sample_rate) if out_sample_rate is not None else sr)
    torch.cuda.synchronize(dev)
    print(f"say: {len(pieces)} pieces in {info['chunks']} chunks, {seconds:.2f} s of audio in {time.perf_counter() - t_start:.2f} s")
    return y, plan_, info
