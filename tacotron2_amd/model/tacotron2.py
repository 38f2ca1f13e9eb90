"""Tacotron2: drop-in for the reference's model.tacotron2.Tacotron2 (constructor kwargs model/tacotron2.py:15-34,
forward signature and 4-tuple return :155-166,347, state_dict keys SURVEY.md Appendix A) on the gfx950 HIP engine.

All learnable tensors are views into ONE flat fp32 device buffer (tacotron2_amd.params.ParamStore); they are exposed as
ordinary nn.Parameters under the reference's module paths, so state_dict()/load_state_dict()/optimizers work unchanged.
forward(teacher_forcing=True) is differentiable in all four outputs (the alignments included: a loss on the attention
weights trains the model): autograd receives the hand-written backward through one torch.autograd.Function.
forward(teacher_forcing=False, max_len_override=N) is the autoregressive path.
There is no CPU fallback: the module can be constructed and (de)serialised anywhere, but forward needs the GPU library.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from .._lib import call
from ..engine import check_rate, Engine, _stream, check_attention_window, check_forward_attention, check_stop_threshold
from ..init import init_parameters
from ..params import ParamStore, check_reduction_factor


class _Node(nn.Module):
    """Bare container used to reproduce the reference's module paths (encoder.convolutions.0.weight, ...)."""


def _attach(root: nn.Module, dotted: str, value, buffer: bool = False):
    import weakref
    from .submodules import CLASSES
    parts = dotted.split(".")
    mod = root
    for i, part in enumerate(parts[:-1]):
        if part not in mod._modules:
            cls = CLASSES.get(".".join(parts[:i + 1]), _Node)
            child = cls()
            child.__dict__["_t2_root"] = weakref.ref(root)      # not a registered sub-module: no reference cycle in state
            mod.add_module(part, child)
        mod = mod._modules[part]
    if buffer:
        mod.register_buffer(parts[-1], value)
    else:
        mod.register_parameter(parts[-1], value)


class _TacotronFn(torch.autograd.Function):
    """Teacher-forced forward / backward of the whole model as one autograd node."""

    @staticmethod
    def forward(ctx, model, batch, *params):
        eng: Engine = model._engine
        masks = batch.get("masks")
        if masks is None:
            B, L = batch["chars_idx"].shape
            masks = eng.make_masks(B, L, batch["mel"].shape[1], model.training, model._seed, model._calls)
        model._calls += 1
        outs, ectx = eng.forward_tf(batch["chars_idx"], batch["chars_len"], batch["mel"], batch["mel_len"],
                                    speaker_id=batch.get("speaker_id"),
                                    description_embeddings=batch.get("description_embeddings"),
                                    training=model.training, masks=masks, save_for_backward=batch["need_grad"],
                                    controls=batch.get("controls"), forward_attention=batch.get("forward_attention", False))
        ctx.model, ctx.ectx = model, ectx
        # an output the loss does not touch arrives in backward as None, not as a tensor of zeros: the alignments are
        # differentiable, but a loss on the mels alone allocates no (B,T,L) gradient and runs the attention backward without one
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, d_mels, d_post, d_gates, d_align):
        model, ectx = ctx.model, ctx.ectx
        eng: Engine = model._engine
        ps = model.store
        B, T, M = ectx["B"], ectx["T"], model.num_mels
        f = lambda g: g.contiguous().float() if g is not None else None
        r, S = ectx["r"], ectx["S"]
        d_post_m = eng.buf("ag.d_post", B, T, M)
        dproj = eng.buf("ag.dproj", S, B, r * M + 1)
        # grouped layout [S][B][r*M+1]; a step's stop-logit gradient is the sum over its frames
        call("t2_outgrad_pack_r", f(d_mels), f(d_post), f(d_gates), ectx["mlen32"], d_post_m, dproj, B, T, M, r, _stream())
        ps.grad.zero_()
        eng.backward_tf(ectx, d_post_m, dproj, d_align=f(d_align))
        grads = tuple(ps.G[name] for name in model._param_names)
        return (None, None) + grads


class Tacotron2(nn.Module):
    def __init__(self, num_chars: int, encoded_dim: int, encoder_kernel_size: int, num_mels: int, prenet_dim: int,
                 att_rnn_dim: int, att_dim: int, rnn_hidden_dim: int, postnet_dim: int, dropout: float,
                 speaker_tokens: bool = False, speaker_tokens_dim: Optional[int] = 128, num_speakers: int = 1,
                 controls: bool = False, controls_dim: int = 0, description_embeddings: bool = False,
                 description_embeddings_dim: int = 0, device=None, seed: int = 0, reduction_factor: int = 1,
                 zoneout: float = 0.0, cell_dropout: float = 0.1):
        """zoneout z in [0, 1] (Krueger et al. 2017; ESPnet's `zoneout_rate`, customary 0.1): in training every unit of the two decoder
        LSTM cells keeps its previous h / c with probability z per step (independent 0/1 masks for h and c, no rescaling); in eval and
        decoding the carried state is z * previous + (1 - z) * new.  0 (default): the reference's cells.  cell_dropout in [0, 1): the
        rate of the dropout on the two cells' outputs (the reference's hard-coded nn.Dropout(0.1)); 0 = none - the paper's setting
        is zoneout=0.1, cell_dropout=0.  Neither changes a parameter.
        reduction_factor r >= 1: every decoder step emits r consecutive mel frames (`decoder.mel_out` has r * num_mels rows), so
        the recurrences run ceil(T / r) times for T frames.  mels, mels_post and gates keep frame resolution (a step's stop logit
        is repeated over its frames); `alignments` has one row per step, (B, ceil(T / r), L).  1: the reference's model."""
        super().__init__()
        reduction_factor = check_reduction_factor(reduction_factor)
        self.reduction_factor = reduction_factor
        self.zoneout, self.cell_dropout = check_rate(zoneout, "zoneout", closed=True), check_rate(cell_dropout, "cell_dropout")
        assert not speaker_tokens or num_speakers is not None, "If speaker tokens are enabled, you must give a num_speakers!"
        assert encoder_kernel_size == 5, "the conv-as-GEMM kernels are specialised for the reference's k=5"
        self.embedding_dim = self.char_embedding_dim = encoded_dim
        self.num_mels, self.att_rnn_dim, self.rnn_hidden_dim = num_mels, att_rnn_dim, rnn_hidden_dim
        self.controls, self.controls_dim = controls, controls_dim
        self.speaker_tokens, self.description_embeddings = speaker_tokens, description_embeddings
        self.encoded_full_dim = encoded_dim + (128 if description_embeddings else 0)
        self.dims = dict(num_chars=num_chars, encoded_dim=encoded_dim, encoder_kernel_size=encoder_kernel_size,
                         num_mels=num_mels, prenet_dim=prenet_dim, att_rnn_dim=att_rnn_dim, att_dim=att_dim,
                         rnn_hidden_dim=rnn_hidden_dim, postnet_dim=postnet_dim, dropout=dropout,
                         speaker_tokens=speaker_tokens, num_speakers=num_speakers,
                         description_embeddings=description_embeddings,
                         description_embeddings_dim=description_embeddings_dim,
                         controls=bool(controls), controls_dim=int(controls_dim) if controls else 0)
        if reduction_factor != 1:     # (a missing key means 1: the dims of an r = 1 model are what they always were)
            self.dims["reduction_factor"] = reduction_factor
        if self.zoneout != 0.0:       # (likewise: missing keys mean zoneout 0 and cell_dropout 0.1)
            self.dims["zoneout"] = self.zoneout
        if self.cell_dropout != 0.1:
            self.dims["cell_dropout"] = self.cell_dropout
        if device is None:
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        self._seed, self._calls = seed, 0
        self._install(ParamStore(self.dims, device))
        init_parameters(self.store, seed)

    # ---- parameter plumbing -------------------------------------------------------------------------
    def _install(self, store: ParamStore):
        for name in list(self._modules):
            del self._modules[name]
        self.store = store
        self._engine = Engine(store)
        self._param_names = list(store.P)
        for name, view in store.P.items():
            _attach(self, name, nn.Parameter(view, requires_grad=True))
        for name, view in store.Bf.items():
            _attach(self, name, view, buffer=True)
        for name, val in store.num_batches_tracked.items():
            _attach(self, name, torch.tensor(val, dtype=torch.int64), buffer=True)

    def _apply(self, fn, recurse=True):
        """.to()/.cuda()/.cpu(): move the flat buffers and rebuild the views (the aliasing is the point)."""
        probe = fn(torch.empty(0, dtype=torch.float32, device=self.store.device))
        if probe.device != self.store.device:
            new = ParamStore(self.dims, probe.device)
            new.flat.copy_(self.store.flat)
            new.buf_flat.copy_(self.store.buf_flat)
            new.num_batches_tracked = dict(self.store.num_batches_tracked)
            self._install(new)
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        missing = self.store.load_state_dict(state_dict, strict=False)
        unexpected = [k for k in state_dict if k not in self.store.P and k not in self.store.Bf
                      and k not in self.store.num_batches_tracked]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:4]} unexpected {unexpected[:4]}")
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def state_dict(self, *args, destination=None, prefix: str = "", keep_vars: bool = False):
        sd = self.store.state_dict(prefix)
        if destination is not None:
            destination.update(sd)
            return destination
        return sd

    # ---- forward ------------------------------------------------------------------------------------
    def init_hidden(self, encoded_len: int, batch_size: int, device):
        """model/tacotron2.py:126-153 (zero states; the engine keeps its own, this is for API parity)."""
        z = lambda *s: torch.zeros(*s, device=device)
        return ((z(batch_size, self.att_rnn_dim), z(batch_size, self.att_rnn_dim)), z(batch_size, self.encoded_full_dim),
                z(batch_size, encoded_len), z(batch_size, encoded_len),
                (z(batch_size, self.rnn_hidden_dim), z(batch_size, self.rnn_hidden_dim)))

    def forward(self, chars_idx: Tensor, chars_idx_len: Tensor, teacher_forcing: bool,
                mel_spectrogram: Optional[Tensor] = None, mel_spectrogram_len: Optional[Tensor] = None,
                speaker_id: Optional[Tensor] = None, controls: Optional[Tensor] = None,
                max_len_override: Optional[int] = None, description_embeddings: Optional[Tensor] = None,
                dropout_masks: Optional[dict] = None, attention_window: Optional[Tuple[int, int]] = None,
                forward_attention: bool = False, train_forward_attention: bool = False, stop_threshold: float = 0.5):
        """attention_window (autoregressive decoding only): (back, fwd) integers >= 0 - each frame attends only to the positions
        max(0, m - back) .. min(len - 1, m + fwd) around the previous frame's attention peak m (ESPnet's `use_att_constraint`);
        None attends to the whole text, as the reference does.
        forward_attention (autoregressive decoding only, not together with attention_window): True decodes with forward
        attention (Zhang et al. 2018; Mozilla TTS's `use_forward_attn` without a transition agent) - the weights of a frame are
        the softmax times the prior 0.5 alpha_{t-1}(n) + 0.5 alpha_{t-1}(n-1) + 1e-8, renormalised (Engine.infer).
        train_forward_attention (teacher forcing only): True runs the teacher-forced attention chain under the same prior, forward
        and backward (Engine.forward_tf(forward_attention=True)) - training-time forward attention; such a model is decoded with
        forward_attention=True.
        stop_threshold (autoregressive decoding only): 0 < tau < 1 - an utterance stops at the first step whose stop probability
        sigmoid(logit) falls below tau (NVIDIA's `gate_threshold`; Engine.infer).  0.5 is the reference's rule, `gate < 0`; a lower
        value decodes longer, a higher one stops earlier."""
        if check_stop_threshold(stop_threshold) != 0.5 and teacher_forcing:
            raise ValueError("stop_threshold applies to autoregressive decoding only (teacher_forcing=False)")
        if check_forward_attention(train_forward_attention) and not teacher_forcing:
            raise ValueError("train_forward_attention applies to teacher forcing only (teacher_forcing=True); decode with "
                             "forward_attention=True")
        if attention_window is not None:
            if teacher_forcing:
                raise ValueError("attention_window applies to autoregressive decoding only (teacher_forcing=False)")
            attention_window = check_attention_window(attention_window)
        if check_forward_attention(forward_attention, attention_window) and teacher_forcing:
            raise ValueError("forward_attention applies to autoregressive decoding only (teacher_forcing=False)")
        if teacher_forcing:
            assert mel_spectrogram is not None, "Ground-truth Mel spectrogram is required for teacher forcing"
            assert mel_spectrogram_len is not None, "Ground-truth Mel spectrogram lengths are required for teacher forcing"
        assert not self.speaker_tokens or speaker_id is not None, "speaker_id tensor required when speaker tokens are active!"
        assert not self.description_embeddings or description_embeddings is not None, \
            "description tensor required when description tokens are active!"
        assert not self.controls or controls is not None, "Controls are enabled, but no control vector was passed to the model!"
        assert self.controls or controls is None, "Controls are disabled, but a control vector was passed to the model!"
        if max_len_override is None and mel_spectrogram is None:
            raise Exception("If Mel spectrogram is not given, max_len_override is required!")
        if not chars_idx.is_cuda:
            raise RuntimeError("Tacotron2.forward needs CUDA/HIP tensors: the product path has no CPU fallback")
        if teacher_forcing:
            T = mel_spectrogram.shape[1] if max_len_override is None else max_len_override
            mel = mel_spectrogram[:, :T].contiguous().float()
            batch = dict(chars_idx=chars_idx.contiguous(), chars_len=chars_idx_len, mel=mel, mel_len=mel_spectrogram_len,
                         speaker_id=speaker_id,
                         description_embeddings=description_embeddings.contiguous().float()
                         if description_embeddings is not None else None, masks=dropout_masks,
                         controls=controls, need_grad=torch.is_grad_enabled(), forward_attention=train_forward_attention)
            named = dict(self.named_parameters())
            params = [named[n] for n in self._param_names]      # store order = order of the returned gradients
            return _TacotronFn.apply(self, batch, *params)
        with torch.no_grad():     # ONE loop over the whole batch (groups of 64 in lock-step inside the engine)
            pm = dropout_masks.get("prenet_drop") if dropout_masks else None
            o = self._engine.infer(chars_idx.contiguous(), chars_idx_len, int(max_len_override), speaker_id=speaker_id,
                                   description_embeddings=description_embeddings.contiguous().float()
                                   if description_embeddings is not None else None,
                                   training=self.training, prenet_masks=pm, seed=self._seed + self._calls, controls=controls,
                                   attention_window=attention_window, forward_attention=forward_attention,
                                   stop_threshold=stop_threshold)
            self._calls += 1
        return o[:4]

    def durations(self, chars_idx: Tensor, chars_idx_len: Tensor, mel_spectrogram: Tensor, mel_spectrogram_len: Tensor,
                  mode: str = "monotonic", **kw):
        """Per-character durations of a batch from its teacher-forced alignments: an EVAL-mode forward(teacher_forcing=True, ...)
        with the same arguments (speaker_id, controls, description_embeddings, max_len_override, dropout_masks,
        train_forward_attention), no gradients, then Engine.durations on its alignments.  Returns (durations, stats, alignments):
        int32 (B, L) mel frames per character (each row sums to the utterance's mel length, 0 behind its text), float32 (B, 4) =
        (focus rate, mean log-weight on the path, feasible, agreement with the argmax) and the (B, S, L) alignments.  mode:
        "monotonic" (the best monotonic path, Glow-TTS's alignment search) or "argmax".  The module's train/eval state is kept."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                align = self.forward(chars_idx, chars_idx_len, True, mel_spectrogram=mel_spectrogram,
                                     mel_spectrogram_len=mel_spectrogram_len, **kw)[3]
                T = mel_spectrogram.shape[1] if kw.get("max_len_override") is None else min(int(kw["max_len_override"]),
                                                                                            mel_spectrogram.shape[1])
                frames = mel_spectrogram_len.to(align.device).clamp(max=T)
                dur, stats = self._engine.durations(align, chars_idx_len.to(align.device), frames, mode=mode)
        finally:
            self.train(was_training)
        return dur, stats, align

    def variances(self, chars_idx: Tensor, chars_idx_len: Tensor, mel_spectrogram: Tensor, mel_spectrogram_len: Tensor, wavs, meter,
                  mode: str = "monotonic", log_pitch: bool = True, interpolate: bool = False, return_frames: bool = False, **kw):
        """Per-character durations, pitch and energy of a batch - the three targets of a duration-based student: durations(...) with
        the same arguments, then prosody.char_variances on its durations with `wavs` (the signals the mels came from, 1-D float32 on
        the meter's device) and `meter` (a ProsodyMeter; its track is the pitch).  Returns (durations, variances, stats): int32
        (B, L); the dict of analysis.char_variance - pitch, energy float32 (B, L), voiced int32 (B, L), with return_frames also
        pitch_frames and energy_frames (B, T) - plus alignment_stats = durations' float32 (B, 4); and its float64 (B, 10) sums
        (analysis.VAR_STATS).  The energy is taken on `mel_spectrogram`, the recording's log-mel."""
        from .. import prosody
        dur, dstats, _ = self.durations(chars_idx, chars_idx_len, mel_spectrogram, mel_spectrogram_len, mode=mode, **kw)
        dev = dur.device
        out, stats = prosody.char_variances(meter, wavs, mel_spectrogram.to(dev).float(), mel_spectrogram_len.to(dev), dur,
                                            chars_idx_len.to(dev), log_pitch=log_pitch, interpolate=interpolate,
                                            return_frames=return_frames)
        out["alignment_stats"] = dstats
        return dur, out, stats

    def score(self, chars_idx: Tensor, chars_idx_len: Tensor, mel_spectrogram: Tensor, mel_spectrogram_len: Tensor,
              max_len_override: int = 5000, n_ceps: int = 13, **kw):
        """Objective score of a free-running decode against the recording: an EVAL-mode forward(teacher_forcing=False, ...) with the
        same arguments (speaker_id, controls, description_embeddings, dropout_masks, attention_window, forward_attention,
        stop_threshold; the reduction factor is the model's), then score_decode on its outputs.  Returns (mels_post, scores).  The
        module's train / eval state is kept."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                _, post, gates, align = self.forward(chars_idx, chars_idx_len, False, max_len_override=max_len_override, **kw)
                scores = self.score_decode(post, gates, align, chars_idx_len, mel_spectrogram, mel_spectrogram_len,
                                           stop_threshold=kw.get("stop_threshold", 0.5), n_ceps=n_ceps)
        finally:
            self.train(was_training)
        return post, scores

    def score_decode(self, post: Tensor, gates: Tensor, align: Tensor, chars_idx_len: Tensor, mel_spectrogram: Tensor,
                     mel_spectrogram_len: Tensor, stop_threshold: float = 0.5, n_ceps: int = 13, return_path: bool = False) -> dict:
        """MCD-DTW (Engine.mcd_dtw) between the post-net mels of a decode - (mels_post, gates, alignments) as
        forward(teacher_forcing=False) returns them - cut at the decode's own lengths, and the recordings `mel_spectrogram`
        (B, T, num_mels) cut at `mel_spectrogram_len`.  A dict of per-utterance tensors:
          mcd         float64 dB, the mean distance over the warped frame pairs; NaN for an utterance that never stopped
          path_len    int32 warped pairs (0 when it never stopped)
          syn_frames  int64 - the first frame whose stop logit is below logit(stop_threshold), 0 when there is none (the rule of
                      run/test.py's mel_lengths_of)
          ref_frames  int64, mel_spectrogram_len cut at T
          stopped     bool, syn_frames > 0
          focus_rate  float32, the mean over the decoder steps of the largest attention weight (Engine.durations, mode "argmax",
                      over the syn_frames of a stopped utterance, over the whole decode of one that never stopped)
        return_path adds  path  int32 (B, P, 2): the first path_len[b] rows are the warped pairs (frame of the decode, frame of
                      the recording) in forward order (Engine.dtw), the rest -1"""
        from ..engine import stop_logit
        B = post.shape[0]
        if not torch.is_tensor(mel_spectrogram) or mel_spectrogram.dim() != 3 or mel_spectrogram.shape[0] != B \
                or mel_spectrogram.shape[2] != self.num_mels:
            raise ValueError(f"score: mel_spectrogram must be ({B}, T, {self.num_mels}), got "
                             f"{tuple(mel_spectrogram.shape) if torch.is_tensor(mel_spectrogram) else type(mel_spectrogram)}")
        if not torch.is_tensor(mel_spectrogram_len) or mel_spectrogram_len.numel() != B or mel_spectrogram_len.is_floating_point():
            raise ValueError(f"score: mel_spectrogram_len must be {B} integers")
        tau = check_stop_threshold(stop_threshold)
        with torch.no_grad():
            dev = post.device
            syn = (gates[:, :, 0] < stop_logit(tau)).to(torch.int64).argmax(dim=-1)
            stopped = syn > 0
            ref = mel_spectrogram_len.reshape(B).to(dev).to(torch.int64).clamp(min=0, max=mel_spectrogram.shape[1])
            # (cut at the longest utterance of each side: a decode that ran into max_len is longer than the warping's cap, its
            # stopped utterances are not)
            ta, tb = max(int(syn.max()), 1), max(int(ref.max()), 1)
            mcd, _, path_len, *path = self._engine.mcd_dtw(post[:, :ta], syn, mel_spectrogram.to(dev).float()[:, :tb], ref,
                                                           n_ceps=n_ceps, return_path=return_path)
            frames = torch.where(stopped, syn, torch.full_like(syn, post.shape[1]))
            stats = self._engine.durations(align, chars_idx_len.to(dev), frames, mode="argmax")[1]
        out = dict(mcd=mcd, path_len=path_len, syn_frames=syn, ref_frames=ref, stopped=stopped, focus_rate=stats[:, 0].clone())
        if return_path:
            out["path"] = path[0]
        return out

    def inference(self, chars_idx, chars_idx_len, max_len: int = 5000, **kw):
        """Alias of forward(teacher_forcing=False, max_len_override=max_len) (north_star's "inference() surface")."""
        return self.forward(chars_idx, chars_idx_len, False, max_len_override=max_len, **kw)
