"""TTSModel: the reference's training shell (model/tts_model.py) without Lightning: same constructor kwargs, the
`.tacotron2` attribute (state_dict keys `tacotron2.<...>`), forward() delegation (:93-115), the 3-term loss (:197-201),
Adam + MultiStepLR (:78-91).  run/train.py drives the fused HIP step (tacotron2_amd.trainer.Trainer); training_step /
validation_step keep the reference's batch format for external loops."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor, nn

from .._lib import call
from ..engine import LOSS_DEFAULTS, check_guided_attention, check_loss_options, loss_opts_struct
from ..params import check_reduction_factor
from .tacotron2 import Tacotron2


def check_loss_inputs(mel, post, gate, mel_tgt, gate_tgt, mel_len) -> None:
    """The loss kernel reads raw pointers with the strides of `mel`: a target of another shape would be read with the wrong stride
    or past its end, a tensor on another device would be a foreign pointer inside the kernel.  Raises ValueError instead."""
    if mel.dim() != 3:
        raise ValueError(f"loss: mels must be (B, T, M), got shape {tuple(mel.shape)}")
    B, T, M = mel.shape
    if tuple(post.shape) != (B, T, M) or gate.numel() != B * T:
        raise ValueError(f"loss: mels_post {tuple(post.shape)} and gates {tuple(gate.shape)} do not match mels {(B, T, M)}")
    if tuple(mel_tgt.shape) != (B, T, M):
        raise ValueError(f"loss: the mel target has shape {tuple(mel_tgt.shape)}, the model output {(B, T, M)}")
    if gate_tgt.numel() != B * T:
        raise ValueError(f"loss: the gate target has {gate_tgt.numel()} elements, the output has B * T = {B * T}")
    if mel_len.numel() != B:
        raise ValueError(f"loss: {mel_len.numel()} mel lengths for a batch of {B}")
    for name, t in (("mels_post", post), ("gates", gate), ("mel target", mel_tgt), ("gate target", gate_tgt), ("mel lengths", mel_len)):
        if t.device != mel.device:
            raise ValueError(f"loss: the {name} is on {t.device}, the mels on {mel.device}")


class _LossTermsFn(torch.autograd.Function):
    """(gate BCE-with-logits, mel MSE, post MSE) of model/tts_model.py:197-199 - plain means over the padded tensors - as ONE
    device kernel (t2_loss_terms); with autograd on, the same launch also writes the three dense gradients, which backward scales
    by the upstream gradient of each term.  `loss`: checked loss options (engine.check_loss_options); anything but the defaults goes
    through t2_loss_terms_opt - l1 / l1+l2 mel terms, the mean over valid frames, the stop-class weight."""

    @staticmethod
    def forward(ctx, mel, post, gate, mel_tgt, gate_tgt, mel_len, *options):
        check_loss_inputs(mel, post, gate, mel_tgt, gate_tgt, mel_len)
        loss = check_loss_options(options[0] if options else None)     # (an optional seventh argument: callers without it are served as before)
        ctx.n_options = len(options)
        B, T, M = mel.shape
        need = any(ctx.needs_input_grad[:3])
        mel, post, gate = mel.contiguous().float(), post.contiguous().float(), gate.contiguous().float()
        loss3 = torch.empty(3, dtype=torch.float64, device=mel.device)
        grads = [torch.empty_like(t) if need else None for t in (mel, post, gate)]
        if loss == LOSS_DEFAULTS:
            call("t2_loss_terms", mel, post, gate, mel_tgt.contiguous().float(), gate_tgt.contiguous().float(),
                 mel_len.to(torch.int32), B, T, M, loss3, grads[0], grads[1], grads[2], 1.0, torch.cuda.current_stream().cuda_stream)
        else:
            call("t2_loss_terms_opt", mel, post, gate, mel_tgt.contiguous().float(), gate_tgt.contiguous().float(),
                 mel_len.to(torch.int32), B, T, M, loss3, grads[0], grads[1], grads[2], 1.0, loss_opts_struct(loss),
                 torch.cuda.current_stream().cuda_stream)
        ctx.grads = grads
        return loss3.float()

    @staticmethod
    def backward(ctx, g3):
        d_mel, d_post, d_gate = ctx.grads
        return (d_mel * g3[1] if d_mel is not None else None, d_post * g3[2] if d_post is not None else None,
                d_gate * g3[0] if d_gate is not None else None, None, None, None) + (None,) * ctx.n_options


class _GuidedAttnFn(torch.autograd.Function):
    """Guided-attention loss on the alignments (t2_guided_attn, include/tacotron2_amd.h): value and - with autograd on - the dense
    gradient from ONE launch; backward scales it by the upstream gradient of the term."""

    @staticmethod
    def forward(ctx, alignment, chars_len, mel_len, sigma, alpha):
        if alignment.dim() != 3 or chars_len.numel() != alignment.shape[0] or mel_len.numel() != alignment.shape[0]:
            raise ValueError(f"guided attention: alignments {tuple(alignment.shape)} must be (B, T, L) with B text and mel lengths, "
                             f"got {chars_len.numel()} and {mel_len.numel()}")
        for name, t in (("text lengths", chars_len), ("mel lengths", mel_len)):
            if t.device != alignment.device:
                raise ValueError(f"guided attention: the {name} are on {t.device}, the alignments on {alignment.device}")
        B, T, L = alignment.shape
        alignment = alignment.contiguous().float()
        loss = torch.empty(1, dtype=torch.float64, device=alignment.device)
        ctx.grad = torch.empty_like(alignment) if ctx.needs_input_grad[0] else None
        call("t2_guided_attn", alignment, chars_len.to(torch.int32), mel_len.to(torch.int32), B, T, L, float(sigma), float(alpha),
             loss, ctx.grad, 1.0, torch.cuda.current_stream().cuda_stream)
        return loss.float()[0]

    @staticmethod
    def backward(ctx, g):
        return (ctx.grad * g if ctx.grad is not None else None, None, None, None, None)


class TTSModel(nn.Module):
    def __init__(self, lr: float, weight_decay: float, num_chars: int, encoded_dim: int = 512, encoder_kernel_size: int = 5,
                 num_mels: int = 80, prenet_dim: int = 256, att_rnn_dim: int = 1024, att_dim: int = 128,
                 rnn_hidden_dim: int = 1024, postnet_dim: int = 512, dropout: float = 0.5,
                 scheduler_milestones: List[int] = (), speaker_tokens: bool = False, num_speakers: int = 1,
                 controls: bool = False, controls_dim: int = 0, max_len_override: Optional[int] = None,
                 description_embeddings: bool = False, description_embeddings_dim: int = 0,
                 char_embedding_dim: Optional[int] = None, device=None, reduction_factor: int = 1,
                 zoneout: float = 0.0, cell_dropout: float = 0.1):
        super().__init__()
        reduction_factor = check_reduction_factor(reduction_factor)    # mel frames per decoder step (Tacotron2)
        if char_embedding_dim is not None:     # stale configs name encoded_dim `char_embedding_dim`
            encoded_dim = char_embedding_dim
        self.hparams = dict(lr=lr, weight_decay=weight_decay, num_chars=num_chars, encoded_dim=encoded_dim,
                            encoder_kernel_size=encoder_kernel_size, num_mels=num_mels, prenet_dim=prenet_dim,
                            att_rnn_dim=att_rnn_dim, att_dim=att_dim, rnn_hidden_dim=rnn_hidden_dim,
                            postnet_dim=postnet_dim, dropout=dropout, scheduler_milestones=list(scheduler_milestones),
                            speaker_tokens=speaker_tokens, num_speakers=num_speakers, controls=controls,
                            controls_dim=controls_dim, max_len_override=max_len_override,
                            description_embeddings=description_embeddings,
                            description_embeddings_dim=description_embeddings_dim, reduction_factor=reduction_factor,
                            zoneout=float(zoneout), cell_dropout=float(cell_dropout))
        self.lr, self.weight_decay = lr, weight_decay
        self.scheduler_milestones = list(scheduler_milestones)
        self.speaker_tokens, self.controls = speaker_tokens, controls
        self.max_len_override, self.description_embeddings = max_len_override, description_embeddings
        # (back, fwd) windowed attention of predict_step and the run drivers' decoding (run/test.py); None = the whole text
        self.attention_window: Optional[Tuple[int, int]] = None
        # forward attention of predict_step and the run drivers' decoding (Tacotron2.forward); False = the plain softmax weights
        self.forward_attention: bool = False
        # (sigma, alpha) of the guided-attention loss that training_step / validation_step add to the three terms; None = off.  Set by
        # the driver (run/train.py), not a constructor argument: checkpoint hyper_parameters stay as the reference writes them
        self.guided_attention: Optional[Tuple[float, float]] = None
        # forward attention under teacher forcing in training_step / validation_step (Tacotron2.forward(train_forward_attention=True)).
        # Set by the driver like guided_attention: not a constructor argument, not in hparams
        self.train_forward_attention: bool = False
        # loss options of training_step / validation_step: None, a dict or (mel, masked, stop_weight) - engine.check_loss_options:
        # "l1" / "l1+l2" mel terms, the mean over valid frames only, a weight on the stop class.  Training settings that change no
        # parameter: set by the driver like guided_attention, not a constructor argument, not in hparams.  None = the reference's loss
        self.loss_options = None
        # stop threshold of predict_step and the run drivers' decoding (Tacotron2.forward(stop_threshold=...)); 0.5 = the reference
        self.stop_threshold: float = 0.5
        self.tacotron2 = Tacotron2(num_chars=num_chars, encoded_dim=encoded_dim, encoder_kernel_size=encoder_kernel_size,
                                   num_mels=num_mels, prenet_dim=prenet_dim, att_rnn_dim=att_rnn_dim, att_dim=att_dim,
                                   rnn_hidden_dim=rnn_hidden_dim, postnet_dim=postnet_dim, dropout=dropout,
                                   speaker_tokens=speaker_tokens, num_speakers=num_speakers, controls=controls,
                                   controls_dim=controls_dim, description_embeddings=description_embeddings,
                                   description_embeddings_dim=description_embeddings_dim, device=device,
                                   reduction_factor=reduction_factor, zoneout=zoneout, cell_dropout=cell_dropout)

    def configure_optimizers(self):
        optimizer = torch.optim.Adam(self.tacotron2.parameters(), lr=self.lr, weight_decay=self.weight_decay)
        cfg = {"optimizer": optimizer}
        if len(self.scheduler_milestones) > 0:
            sched = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=self.scheduler_milestones, gamma=0.1)
            cfg["lr_scheduler"] = {"scheduler": sched, "interval": "step"}
        return cfg

    def forward(self, chars_idx: Tensor, chars_idx_len: Tensor, teacher_forcing: bool = True,
                mel_spectrogram: Optional[Tensor] = None, mel_spectrogram_len: Optional[Tensor] = None,
                speaker_id: Optional[Tensor] = None, controls: Optional[Tensor] = None,
                max_len_override: Optional[int] = None, description_embeddings: Optional[Tensor] = None,
                attention_window: Optional[Tuple[int, int]] = None, forward_attention: bool = False,
                train_forward_attention: bool = False, stop_threshold: float = 0.5):
        return self.tacotron2(chars_idx=chars_idx, chars_idx_len=chars_idx_len, teacher_forcing=teacher_forcing,
                              mel_spectrogram=mel_spectrogram, mel_spectrogram_len=mel_spectrogram_len,
                              speaker_id=speaker_id, controls=controls, max_len_override=max_len_override,
                              description_embeddings=description_embeddings, attention_window=attention_window,
                              forward_attention=forward_attention, train_forward_attention=train_forward_attention,
                              stop_threshold=stop_threshold)

    def durations(self, chars_idx: Tensor, chars_idx_len: Tensor, mel_spectrogram: Tensor, mel_spectrogram_len: Tensor,
                  mode: str = "monotonic", speaker_id: Optional[Tensor] = None, controls: Optional[Tensor] = None,
                  max_len_override: Optional[int] = None, description_embeddings: Optional[Tensor] = None,
                  train_forward_attention: bool = False):
        """(durations, stats, alignments) of an eval-mode teacher-forced forward: Tacotron2.durations."""
        return self.tacotron2.durations(chars_idx, chars_idx_len, mel_spectrogram, mel_spectrogram_len, mode=mode,
                                        speaker_id=speaker_id, controls=controls, max_len_override=max_len_override,
                                        description_embeddings=description_embeddings,
                                        train_forward_attention=train_forward_attention)

    def variances(self, chars_idx: Tensor, chars_idx_len: Tensor, mel_spectrogram: Tensor, mel_spectrogram_len: Tensor, wavs, meter,
                  mode: str = "monotonic", log_pitch: bool = True, interpolate: bool = False, return_frames: bool = False,
                  speaker_id: Optional[Tensor] = None, controls: Optional[Tensor] = None, max_len_override: Optional[int] = None,
                  description_embeddings: Optional[Tensor] = None, train_forward_attention: bool = False):
        """(durations, variances, stats) - per-character durations, pitch and energy - of an eval-mode teacher-forced forward and the
        meter's pitch track of `wavs`: Tacotron2.variances."""
        return self.tacotron2.variances(chars_idx, chars_idx_len, mel_spectrogram, mel_spectrogram_len, wavs, meter, mode=mode,
                                        log_pitch=log_pitch, interpolate=interpolate, return_frames=return_frames,
                                        speaker_id=speaker_id, controls=controls, max_len_override=max_len_override,
                                        description_embeddings=description_embeddings,
                                        train_forward_attention=train_forward_attention)

    def score(self, chars_idx: Tensor, chars_idx_len: Tensor, mel_spectrogram: Tensor, mel_spectrogram_len: Tensor,
              max_len_override: Optional[int] = None, n_ceps: int = 13, speaker_id: Optional[Tensor] = None,
              controls: Optional[Tensor] = None, description_embeddings: Optional[Tensor] = None,
              attention_window: Optional[Tuple[int, int]] = None, forward_attention: bool = False, stop_threshold: float = 0.5):
        """(mels_post, scores) of an eval-mode free-running decode scored against the recording by MCD-DTW: Tacotron2.score.
        max_len_override None takes the model's (else 5000), as predict_step does."""
        return self.tacotron2.score(chars_idx, chars_idx_len, mel_spectrogram, mel_spectrogram_len,
                                    max_len_override=max_len_override or self.max_len_override or 5000, n_ceps=n_ceps,
                                    speaker_id=speaker_id, controls=controls, description_embeddings=description_embeddings,
                                    attention_window=attention_window, forward_attention=forward_attention,
                                    stop_threshold=stop_threshold)

    def say_document(self, pieces, encoder, preprocessing: Optional[dict] = None, vocoder=None, **options):
        """A document spoken as one waveform: run.say.say_document on this model - pieces (datasets.document.Piece, or a text, which
        is split), the TextEncoder of the model's alphabet, the dataset's `preprocessing` settings (sample_rate, trim_top_db,
        trim_frame_length; None: the defaults) and a loaded vocoder object (hifigan.Generator or vocoder.GriffinLim; None: a
        Griffin-Lim for this model's mel bands).  Among the options: tempo=T (0.5 .. 2.0) and pitch_shift=SEMITONES (-12 .. 12), a
        WSOLA stretch of all pieces in one launch in front of the join; preserve_formants=True and pitch_range=K (0 .. 2) change the
        pitch by TD-PSOLA instead, one launch of each kernel for all pieces; loudness=LUFS (-40 .. -5)
        and true_peak=DBTP (-9 .. 0, default -1) bring the joined waveform to that BS.1770 programme loudness as the last step
        (DESIGN 5.20), and limiter=True holds that ceiling with the look-ahead true-peak limiter; denoise=STRENGTH (0 .. 1, with a
        hifigan.Generator) takes that generator's own bias spectrum off each chunk as the first step behind it.  Loads no checkpoint.  Returns (waveform, plan, per-piece
        dict)."""
        from ..run.say import say_document
        pre = dict(preprocessing or {})
        if vocoder is None:
            from ..vocoder import GriffinLim
            vocoder = GriffinLim(n_mels=int(self.hparams["num_mels"]), sample_rate=int(pre.get("sample_rate", 22050)),
                                 device=next(self.parameters()).device)
        return say_document(self, pieces, encoder, pre, vocoder, **options)

    def _args(self, meta):
        args = {}
        if self.speaker_tokens:
            args["speaker_id"] = meta["speaker_id"]
        if self.description_embeddings:
            args["description_embeddings"] = meta["description_embeddings"]
        if self.controls:
            args["controls"] = meta["features"]           # model/tts_model.py:125,173,304
        return args

    def _loss(self, batch):
        data, meta = batch[0], batch[1]
        guided = check_guided_attention(self.guided_attention)
        loss_options = check_loss_options(self.loss_options)
        mel, post, gate, alignment = self(chars_idx=data["chars_idx"], chars_idx_len=meta["chars_idx_len"],
                                          teacher_forcing=True, mel_spectrogram=data["mel_spectrogram"],
                                          mel_spectrogram_len=meta["mel_spectrogram_len"],
                                          train_forward_attention=self.train_forward_attention, **self._args(meta))
        # the three terms of model/tts_model.py:197-199 from the library's loss kernel (no ATen arithmetic on this path)
        l3 = _LossTermsFn.apply(mel, post, gate, data["mel_spectrogram"], data["gate"], meta["mel_spectrogram_len"], loss_options)
        gate_loss, mel_loss, post_loss = l3[0], l3[1], l3[2]
        loss = l3.sum()
        if guided is not None:
            r = self.tacotron2.reduction_factor      # the alignments have one row per decoder step: ceil(mel_len / r) of them count
            steps = meta["mel_spectrogram_len"] if r == 1 else \
                torch.div(meta["mel_spectrogram_len"] + (r - 1), r, rounding_mode="floor")
            loss = loss + _GuidedAttnFn.apply(alignment, meta["chars_idx_len"], steps, *guided)
        return loss, (gate_loss, mel_loss, post_loss), (mel, post, gate, alignment)

    def training_step(self, batch, batch_idx=0):
        return self._loss(batch)[0]

    def validation_step(self, batch, batch_idx=0):
        with torch.no_grad():
            loss, _, (mel, post, gate, alignment) = self._loss(batch)
        data, meta = batch[0], batch[1]
        ml, cl, r = meta["mel_spectrogram_len"], meta["chars_idx_len"], self.tacotron2.reduction_factor
        return {"mel_spectrogram_pred": post[0, :ml[0]], "mel_spectrogram": data["mel_spectrogram"][0, :ml[0]],
                "alignment": alignment[0, :(ml[0] + r - 1) // r, :cl[0]], "gate": data["gate"][0], "gate_pred": gate[0], "loss": loss}

    def predict_step(self, batch, batch_idx=0, dataloader_idx=0):
        data, meta = batch[0], batch[1]
        with torch.no_grad():
            return self(chars_idx=data["chars_idx"], chars_idx_len=meta["chars_idx_len"], teacher_forcing=False,
                        max_len_override=self.max_len_override or 5000, attention_window=self.attention_window,
                        forward_attention=self.forward_attention, stop_threshold=self.stop_threshold,
                        **self._args(meta))

    # Lightning-style checkpoint exchange: {"state_dict": {"tacotron2.<name>": tensor}, "hyper_parameters": {...}}
    def checkpoint(self, extra: Optional[dict] = None) -> dict:
        ck = {"state_dict": {k: v.cpu() for k, v in self.tacotron2.state_dict(prefix="tacotron2.").items()},
              "hyper_parameters": dict(self.hparams)}
        ck.update(extra or {})
        return ck

    def load_checkpoint_dict(self, ck: dict, strict: bool = True, use_ema: bool = False, path: Optional[str] = None):
        """use_ema=True loads the shadow weights a training run with an EMA wrote beside the live ones (`ema_state_dict`: same keys,
        same shapes); a checkpoint without them is a KeyError that names `path`."""
        key = "ema_state_dict" if use_ema else "state_dict"
        if use_ema and not ck.get(key):
            raise KeyError(f"{path or 'the checkpoint'} holds no EMA weights (ema_state_dict): it was trained without --ema-decay; "
                           "load it without use_ema / --ema")
        sd = {k[len("tacotron2."):]: v for k, v in ck[key].items() if k.startswith("tacotron2.")}
        return self.tacotron2.load_state_dict(sd, strict=strict)

    @classmethod
    def load_from_checkpoint(cls, path: str, map_location=None, device=None, use_ema: bool = False, **overrides):
        ck = torch.load(path, map_location="cpu", weights_only=True)
        hp = dict(ck.get("hyper_parameters", {}))
        # zoneout / cell_dropout change no parameter, so the configured value always loads; a file that recorded another one says so
        for k in ("zoneout", "cell_dropout"):
            if k in overrides and k in hp and float(hp[k]) != float(overrides[k]):
                print(f"warning: checkpoint {path} was written with {k} = {hp[k]}, the configuration says {overrides[k]}: using {overrides[k]}")
        hp.update({k: v for k, v in overrides.items()
                   if k in hp or k in ("lr", "weight_decay", "num_chars", "reduction_factor", "zoneout", "cell_dropout")})
        hp = {k: v for k, v in hp.items() if k in cls.__init__.__code__.co_varnames}
        model = cls(device=device, **hp)
        model.load_checkpoint_dict(ck, use_ema=use_ema, path=path)
        return model
