"""do_test (run/test.py:29-227): synthesise every utterance of the test manifest and write `<i>.wav` files.

The reference runs `trainer.predict` over a batch-8 loader (which also decodes every test wav although the prediction only
reads the text), vocodes each batch with HiFi-GAN (`generator(mel_post.swapaxes(1, 2))`, wav cut at `mel_lengths * 256`) or
with librosa's Griffin-Lim (`mel_post[:mel_length]`), and logs utterances without a stop to `failures.csv`.  Here the texts
go straight from the manifest through the batched decode path (`Tacotron2.forward(teacher_forcing=False)` on the GPU, any
batch size up to 64 per decode group), and the vocoders are the GEMM-kernel ones of this package (hifigan.py, vocoder.py).

Rules kept from the reference: `|`-separated manifest with QUOTE_NONE (:76-78), the `force_speaker` filter and its two
consistency checks (:81-100), controls from the manifest's feature columns (:102-106), `max_len_override` = 5000 (:147),
`mel_lengths = (gate < 0).argmax` - the first masked frame, 0 when the utterance never stopped (:172,205) -, numbering from
1 in manifest order, `failures.csv` rows `i|text` (:187-193,223-227), 22050 Hz output; see synthesize_manifest for the
vocoding details.  `main.py test-correlation` (run/test_correlation.py) runs the same loop under 51 control-vector overrides.

`test --score` (no reference counterpart) also scores every decode against its recording: the manifest's wav column
under --speech-dir goes through the dataset's item path (TTSDataset: the same trim, silence pad and device log-mel as training),
and the post-net mels cut at `mel_lengths` are compared with it by mel-cepstral distortion under dynamic time warping on the
device (Tacotron2.score_decode).  `scores.csv`, `|`-separated with the header SCORE_HEADER, one row per utterance in manifest
order (`i` as in the WAV names; an utterance that never stopped has an empty mcd_dtw and dur_ratio), and `scores.json` with
the aggregates.  `--no-audio` skips vocoding and the WAVs.

`test --score --f0` also compares intonation: every waveform as it goes to write_wav and the recording's waveform
(TTSDataset.load_audio - the trimmed, padded signal the reference mel came from, frame t centred on sample 256 t as the mel frame
is) are pitch-tracked with prosody.ProsodyMeter(smooth=True), and the two tracks are compared along the MCD path
(prosody.f0_scores).  `f0_scores.csv`, `|`-separated with the header F0_HEADER, one row per utterance in manifest order, empty
where undefined (every measure of an utterance that never stopped), and four means plus `settings.f0` in scores.json.
"""
from __future__ import annotations

import csv
import datetime
import json
import math
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..datasets.text import TextEncoder
from ..model.tts_model import TTSModel      # noqa: F401  (load_decode_model's class, under the name it always had here)
from ..options import decode_settings_of, stop_logit
from .common import encode_texts, free_run, load_decode_model, pad_ids, sample_rate


def load_test_model(dataset_config, training_config, model_config, extensions_config, checkpoint, dev, random_seed=None,
                    attention_window=None, forward_attention=None, stop_threshold=None):
    """TTSModel.load_from_checkpoint as run/test.py:116-130 calls it (max_len_override 5000, no scheduler), in eval mode
    (load_decode_model).  attention_window (back, fwd), forward_attention (a bool) and stop_threshold (0 < tau < 1) are what the
    model decodes with (TTSModel's attributes of these names); None takes the config's `model.<name>` if there is one (`main.py`
    puts its options there for test-correlation), else off, off and 0.5 (options.decode_settings).  Forward attention together
    with a window is refused.
    The config's `model.measure_prosody` (a bool; `main.py test-correlation --measure` puts it there, as it does the settings above)
    gives the model a prosody.ProsodyMeter as `model.prosody_meter`, which synthesize_manifest then measures with; the config's
    `model.smooth_pitch` (`--smooth-pitch`) builds it with smooth=True."""
    model = load_decode_model(dataset_config, training_config, model_config, extensions_config, checkpoint, dev, random_seed,
                              attention_window, forward_attention, stop_threshold, scheduler_milestones=[])
    if model_config.get("measure_prosody", False):
        from ..prosody import ProsodyMeter
        model.prosody_meter = ProsodyMeter(sample_rate(dataset_config["preprocessing"]), dev, smooth=bool(model_config.get("smooth_pitch", False)))
    return model


def check_force_speaker(extensions_config: dict):
    """run/test.py:81-100 / run/test_correlation.py:93-110."""
    spk_cfg, ctl_cfg = extensions_config["speaker_tokens"], extensions_config.get("controls", {"active": False})
    if "force_speaker" in spk_cfg:
        if spk_cfg["active"]:
            raise Exception("Cannot use speaker tokens with force_speaker parameter!")
        if ctl_cfg.get("active") and not all("speaker_norm" in x for x in ctl_cfg["features"]):
            raise Exception("If force_speaker, all controls must be for speaker-normalized values!")
        return True
    return False


def make_vocoders(hifi_gan_checkpoint, pre, dev):
    """(HiFi-GAN generator or None, Griffin-Lim or None, sample rate)."""
    from ..vocoder import GriffinLim
    sr = sample_rate(pre)
    if hifi_gan_checkpoint is not None:
        from ..hifigan import Generator
        return Generator.from_checkpoint(hifi_gan_checkpoint, device=dev), None, sr
    return None, GriffinLim(n_mels=int(pre.get("num_mels", 80)), sample_rate=sr, device=dev), sr


def mel_lengths_of(gate: torch.Tensor, stop_threshold: float = 0.5) -> torch.Tensor:
    """run/test.py:172,205 `(gate < 0).argmax` against the decode's own stop threshold: the first frame of (B, n, 1) gates below
    logit(threshold) - the first masked frame (-1000) of an utterance that stopped -, 0 when there is none.  0.5 compares with 0."""
    return (gate[:, :, 0] < stop_logit(stop_threshold)).to(torch.int64).argmax(dim=-1)


SCORE_HEADER = ["i", "wav", "n_chars", "ref_frames", "syn_frames", "stopped", "mcd_dtw", "path_len", "dur_ratio", "focus_rate"]


F0_HEADER = ["i", "wav", "stopped", "n_pairs", "n_voiced_both", "f0_rmse_cents", "f0_bias_cents", "f0_corr", "vuv_error"]


def check_recordings(df, speech_dir) -> None:
    """`test --score` reads every recording of the manifest: a missing one is an error that names the file, before any decoding."""
    if "wav" not in df.columns:
        raise ValueError("test --score: the test manifest has no `wav` column")
    for wav in df.wav:
        path = os.path.join(str(speech_dir), str(wav))
        if not os.path.isfile(path):
            raise FileNotFoundError(f"test --score: recording not found: {path}")


def write_f0_scores(results_dir: str, rows: List[dict]) -> dict:
    """f0_scores.csv (F0_HEADER) of `test --score --f0`; returns the means that go into scores.json, each over the stopped
    utterances where it is defined."""
    from ..prosody import F0_MEASURES
    with open(os.path.join(results_dir, "f0_scores.csv"), "w", newline="") as f:
        wr = csv.writer(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
        wr.writerow(F0_HEADER)
        for r in rows:
            ok = r["stopped"]
            wr.writerow([r["i"], r["wav"], int(ok), r["n_pairs"] if ok else "", r["n_voiced_both"] if ok else ""]
                        + [f"{r[m]:.6f}" if ok and r[m] is not None else "" for m in F0_MEASURES])
    out = {}
    for m in F0_MEASURES:
        v = [r[m] for r in rows if r["stopped"] and r[m] is not None]
        out[f"{m}_mean"] = (sum(v) / len(v)) if v else None
    return out


def write_scores(results_dir: str, rows: List[dict], settings: dict, f0_means: Optional[dict] = None) -> dict:
    """scores.csv (SCORE_HEADER) and scores.json of `test --score`; returns the aggregates.  f0_means (write_f0_scores, with --f0
    only) are added to scores.json in front of `settings`."""
    with open(os.path.join(results_dir, "scores.csv"), "w", newline="") as f:
        wr = csv.writer(f, delimiter="|", quoting=csv.QUOTE_NONE, escapechar="\\")
        wr.writerow(SCORE_HEADER)
        for r in rows:
            ok = r["stopped"]
            wr.writerow([r["i"], r["wav"], r["n_chars"], r["ref_frames"], r["syn_frames"], int(ok),
                         f"{r['mcd']:.6f}" if ok else "", r["path_len"], f"{r['dur_ratio']:.6f}" if ok else "",
                         f"{r['focus_rate']:.6f}"])
    ok = [r for r in rows if r["stopped"]]
    mcds = sorted(r["mcd"] for r in ok)
    mean = lambda v: (sum(v) / len(v)) if v else None
    median = (mcds[len(mcds) // 2] if len(mcds) % 2 else 0.5 * (mcds[len(mcds) // 2 - 1] + mcds[len(mcds) // 2])) if mcds else None
    agg = {"n": len(rows), "n_stopped": len(ok), "failure_rate": (1.0 - len(ok) / len(rows)) if rows else None,
           "mcd_dtw_mean": mean(mcds), "mcd_dtw_median": median,
           "abs_log_dur_ratio_mean": mean([abs(math.log(r["dur_ratio"])) for r in ok if r["dur_ratio"] > 0]),
           "focus_rate_mean": mean([r["focus_rate"] for r in rows]), **(f0_means or {}), "settings": settings}
    with open(os.path.join(results_dir, "scores.json"), "w") as f:
        json.dump(agg, f, indent=1)
    return agg


def measure_batch(meter, pending, n_chars, sr, dev) -> List[dict]:
    """The prosody.csv rows of one batch: pending = (i, manifest index, mel length, waveform as it went to write_wav)."""
    wavs = [torch.as_tensor(w, dtype=torch.float32).reshape(-1).to(dev) if n > 0 else torch.zeros(0, device=dev)
            for _, _, n, w in pending]
    rows = []
    for (i, _, n, written), c, m in zip(pending, n_chars, meter.measure(wavs, n_chars)):
        if n == 0:               # never stopped: whatever was written is not an utterance, and an empty waveform measures nothing
            m = dict(m, rate=None)
        rows.append(dict(m, i=i, wav=f"{i}.wav", n_chars=c, seconds=int(torch.as_tensor(written).numel()) / sr, stopped=int(n > 0)))
    return rows


def synthesize_manifest(model, df, pre, speech_dir, results_dir, gen, gl, sr, feats, batch_size=8, max_len=5000,
                        random_seed=None, zero_length="test", score=False, audio=True, n_ceps=13, meter=None,
                        f0=False) -> List[str]:
    """The prediction + "Saving WAVs" loops of run/test.py:132-227 and run/test_correlation.py:171-250 over one manifest:
    batches of `batch_size` texts through the batched decode path, `mel_lengths = (gate < 0).argmax` (:172,205), numbering from
    1 in manifest order, `failures.csv` rows `i|text`.

    HiFi-GAN: the generator runs on the whole PADDED row of the batch (masked frames are zeros) and the waveform is cut at
    mel_length * 256, as `generator(mel_post.swapaxes(1, 2))` + `wav[:wav_length]` do in the reference - the generator's
    receptive field spans many frames, so the last samples of an utterance depend on what follows it.
    zero_length: what is written for an utterance that never stopped (mel_length 0): "test" = run/test.py:176-193 (wav_length
    becomes -1 and is applied twice: the row minus its last two samples); "correlation" = run/test_correlation.py:196-209 (an
    empty file).  Both log the utterance.  Griffin-Lim (librosa raises on an empty spectrogram): logged, nothing written.
    The decode uses the model's attention window (TTSModel.attention_window, set by load_test_model; None = off) or its forward
    attention (TTSModel.forward_attention; False = off), and its stop threshold (TTSModel.stop_threshold): `mel_lengths` is then the
    first frame with gate < logit(threshold) - under a threshold below 0.5 a kept frame may have a logit in [logit(threshold), 0) -,
    which at 0.5 is the reference's `gate < 0`.
    score: also compare every decode with its recording (module docstring) and write scores.csv / scores.json.  audio False
    (`--no-audio`, with score only): no vocoding, no WAVs; failures.csv is still written.
    meter: a prosody.ProsodyMeter (None: the model's `prosody_meter`, if load_test_model gave it one) measures every waveform as it
    goes to write_wav (before quantisation; one measure() call per batch) and the rows go to `prosody.csv` of results_dir
    (run/correlation.py: PROSODY_HEADER); an utterance that never stopped has stopped = 0 and empty measures.  Without a meter
    nothing of this happens.
    f0 (`--f0`; needs score and audio): also f0_scores.csv and the F0 means in scores.json (module docstring)."""
    from ..vocoder import write_wav
    if f0 and not (score and audio):
        raise ValueError("test: f0=True (--f0) needs score=True (--score) and audio (no --no-audio): it tracks the waveforms")
    dev = model.tacotron2.store.device
    s = decode_settings_of(model)
    enc = TextEncoder(pre["allowed_chars"], pre.get("end_token"), bool(pre.get("expand_abbreviations", False)))
    texts = [enc.clean(t) for t in df.text]
    ids, _, _ = encode_texts(enc, df.text)
    desc_paths = None
    if model.description_embeddings:
        desc_paths = [None if isinstance(x, float) else x for x in df.description_embedding] \
            if "description_embedding" in df.columns else [None] * len(df)
    os.makedirs(results_dir, exist_ok=True)
    speaker_ids = list(df.speaker_id) if model.speaker_tokens else None
    written: List[str] = []
    recordings, score_rows, prosody_rows, f0_rows, f0_meter = None, [], [], [], None
    if meter is None and hasattr(model, "prosody_meter"):
        meter = model.prosody_meter
    if score:
        from ..datasets.tts_dataset import TTSDataset
        check_recordings(df, speech_dir)
        recordings = TTSDataset(filenames=[str(w) for w in df.wav], texts=list(df.text), base_dir=speech_dir, device=dev,
                                **dict(pre, cache=False))
        if f0:
            from ..prosody import ProsodyMeter, f0_scores
            f0_meter = ProsodyMeter(sr, dev, smooth=True)

    def fail(i, text):
        print(f"Error: {i}: {text}")
        with open(os.path.join(results_dir, "failures.csv"), "a") as f:
            f.write(f"{i}|{text}\n")

    i = 0
    for b0 in range(0, len(df), batch_size):
        sel = list(range(b0, min(len(df), b0 + batch_size)))
        chars, lens = pad_ids([ids[j] for j in sel], dev)
        args = {}
        if speaker_ids is not None:
            args["speaker_id"] = torch.tensor([int(speaker_ids[j]) for j in sel], dtype=torch.int32, device=dev)
        if feats is not None:
            args["controls"] = torch.tensor([feats[j] for j in sel], dtype=torch.float32, device=dev)
        if desc_paths is not None:
            dim = int(model.hparams["description_embeddings_dim"])
            rows = [torch.load(os.path.join(speech_dir, desc_paths[j]), map_location="cpu", weights_only=True).reshape(-1)
                    if desc_paths[j] is not None else torch.zeros(dim) for j in sel]
            args["description_embeddings"] = torch.stack(rows).to(dev)
        post, gate, align = free_run(model, chars, lens, max_len, **args)
        mel_lengths = mel_lengths_of(gate, s.stop_threshold).cpu().tolist()
        if score:
            refs = [recordings[j][0]["mel_spectrogram"] for j in sel]
            sc = model.tacotron2.score_decode(post, gate, align, lens, torch.nn.utils.rnn.pad_sequence(refs, batch_first=True),
                                              torch.tensor([len(m) for m in refs], dtype=torch.int64, device=dev),
                                              stop_threshold=s.stop_threshold, n_ceps=n_ceps, return_path=f0)
            warp = (sc.pop("path"), sc["path_len"]) if f0 else None
            sc = {k: v.cpu().tolist() for k, v in sc.items()}
            assert sc["syn_frames"] == [int(n) for n in mel_lengths]
            for k, j in enumerate(sel):
                score_rows.append(dict(i=i + k + 1, wav=str(df.wav[j]), n_chars=len(ids[j]), ref_frames=sc["ref_frames"][k],
                                       syn_frames=sc["syn_frames"][k], stopped=bool(sc["stopped"][k]), mcd=sc["mcd"][k],
                                       path_len=sc["path_len"][k], focus_rate=sc["focus_rate"][k],
                                       dur_ratio=sc["syn_frames"][k] / max(sc["ref_frames"][k], 1)))
        pending = []              # (i, j, n, waveform as written) of this batch, for the meter
        voc = {}                  # k -> the waveform as written, of the utterances that stopped: for f0
        for k, j in enumerate(sel):
            i += 1
            n = int(mel_lengths[k])
            name = os.path.join(results_dir, f"{i}.wav")
            if not audio:
                if n == 0:
                    fail(i, texts[j])
            elif gen is not None:
                row = gen(post[k].t().contiguous())[0, 0]          # the padded row, as the reference vocodes it
                if n == 0:
                    fail(i, texts[j])
                    wav = row[:-1][:-1] if zero_length == "test" else row[:0]
                else:
                    wav = row[:n * 256]
                write_wav(name, wav.cpu(), sr)
                written.append(name)
                if n > 0:
                    voc[k] = wav
                if meter is not None:
                    pending.append((i, j, n, wav))
            else:
                if n == 0:
                    fail(i, texts[j])
                    if meter is not None:
                        pending.append((i, j, 0, torch.zeros(0)))
                    continue
                wav = gl.mel_to_audio(post[k, :n], seed=int(random_seed or 0))
                write_wav(name, wav, sr)
                written.append(name)
                voc[k] = wav
                if meter is not None:
                    pending.append((i, j, n, wav))
        if f0:                    # an utterance that never stopped has path_len 0 and goes in as an empty waveform: nothing scored
            as_dev = lambda x: torch.as_tensor(x, dtype=torch.float32).reshape(-1).to(dev)
            syn_w = [as_dev(voc[k]) if k in voc else torch.zeros(0, device=dev) for k in range(len(sel))]
            ref_w = [as_dev(recordings.load_audio(j)) for j in sel]
            for k, (j, fig) in enumerate(zip(sel, f0_scores(f0_meter, syn_w, ref_w, warp[0], warp[1]))):
                f0_rows.append(dict(fig, i=i - len(sel) + k + 1, wav=str(df.wav[j]), stopped=int(mel_lengths[k]) > 0))
        if meter is not None and pending:
            prosody_rows += measure_batch(meter, pending, [len(ids[j]) for _, j, _, _ in pending], sr, dev)
    if meter is not None:
        from .correlation import write_prosody_csv
        write_prosody_csv(results_dir, prosody_rows)
    if score:
        f0_means = write_f0_scores(results_dir, f0_rows) if f0 else None
        write_scores(results_dir, score_rows, {
            **({"f0": f0_meter.describe()} if f0 else {}), "n_ceps": n_ceps,
            "attention_window": list(s.attention_window) if s.attention_window is not None else None,
            "forward_attention": bool(s.forward_attention), "stop_threshold": float(s.stop_threshold),
            "r": int(model.tacotron2.reduction_factor), "max_len": int(max_len)}, f0_means)
    return written


def do_test(dataset_config: dict, training_config: dict, model_config: dict, extensions_config: dict, device: int,
            speech_dir: Optional[str], checkpoint: str, hifi_gan_checkpoint: Optional[str] = None,
            results_dir: Optional[str] = None, batch_size: int = 8, max_len: int = 5000, limit: Optional[int] = None,
            random_seed: Optional[int] = None, attention_window: Optional[Tuple[int, int]] = None,
            forward_attention: Optional[bool] = None, stop_threshold: Optional[float] = None, score: bool = False,
            audio: bool = True, n_ceps: int = 13, f0: bool = False) -> List[str]:
    import pandas as pd
    if not audio and not score:
        raise ValueError("test: audio=False (--no-audio) needs score=True (--score)")
    if f0 and not (score and audio):
        raise ValueError("test: f0=True (--f0) needs score=True (--score) and audio (no --no-audio): it tracks the waveforms")
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    pre = dataset_config["preprocessing"]
    df = pd.read_csv(dataset_config["test"], delimiter="|", quoting=csv.QUOTE_NONE, engine="c")
    if check_force_speaker(extensions_config):
        df = df[df.speaker_id == extensions_config["speaker_tokens"]["force_speaker"]].reset_index(drop=True)
    if limit is not None:
        df = df.iloc[:int(limit)].reset_index(drop=True)
    if score:
        check_recordings(df, speech_dir)
    model = load_test_model(dataset_config, training_config, model_config, extensions_config, checkpoint, dev, random_seed,
                            attention_window, forward_attention, stop_threshold)
    ctl_cfg = extensions_config.get("controls", {"active": False})
    feats = df[ctl_cfg["features"]].values.tolist() if model.controls else None
    if results_dir is None:
        results_dir = f"results_{training_config['name']}_test {datetime.datetime.now()}"
    gen, gl, sr = make_vocoders(hifi_gan_checkpoint, pre, dev) if audio else (None, None, sample_rate(pre))
    return synthesize_manifest(model, df, pre, speech_dir, results_dir, gen, gl, sr, feats, batch_size=batch_size,
                               max_len=max_len, random_seed=random_seed, zero_length="test", score=score, audio=audio,
                               n_ceps=n_ceps, f0=f0)
