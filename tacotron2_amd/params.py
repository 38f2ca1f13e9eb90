"""Flat fp32 parameter / gradient storage with reference-named views.

All learnable parameters of the reference ``Tacotron2`` (state_dict names and shapes) live
in ONE contiguous fp32 device buffer, each tensor 16-byte aligned, so that
  * the optimizer is one fused kernel over the buffer (t2_adam_step) and the gradient norm one reduction,
  * data-parallel training all-reduces ONE buffer over RCCL (112.5 MB for vanilla dims),
  * tensor pairs that the kernels consume as one matrix are adjacent: [mel_out.weight ; gate.weight] is the
    (M+1, D+Ef) projection, the forward/reverse encoder-LSTM input weights are one (8H, E) matrix, etc.
"""
from __future__ import annotations

import numbers
from collections import OrderedDict
from typing import Dict, Optional

import torch

from . import guard as _guard


def check_reduction_factor(r) -> int:
    """The reduction factor (mel frames per decoder step) as an int >= 1; anything else - a bool, a float, a string, 0 - raises
    ValueError."""
    if isinstance(r, bool) or not isinstance(r, numbers.Integral) or r < 1:
        raise ValueError(f"reduction_factor must be an integer >= 1, got {r!r}")
    return int(r)


def reduction_factor(d: dict) -> int:
    """`reduction_factor` of a dims dict; a missing key means 1."""
    return check_reduction_factor(d.get("reduction_factor", 1))


def param_manifest(d: dict) -> "OrderedDict[str, tuple]":
    """name -> shape in flat-buffer order (learnable parameters only)."""
    r = reduction_factor(d)
    E, k = d["encoded_dim"], d["encoder_kernel_size"]
    Ef = E + (128 if d.get("description_embeddings") else 0)
    P, A, D = d["prenet_dim"], d["att_rnn_dim"], d["rnn_hidden_dim"]
    M, Pn, Ad = d["num_mels"], d["postnet_dim"], d["att_dim"]
    F, Kl = d.get("loc_filters", 32), d.get("loc_kernel", 31)
    s: "OrderedDict[str, tuple]" = OrderedDict()
    s["encoder.embedding.weight"] = (d["num_chars"] + 1, E)
    for i in (0, 4, 8):
        s[f"encoder.convolutions.{i}.weight"] = (E, E, k)
        s[f"encoder.convolutions.{i}.bias"] = (E,)
        s[f"encoder.convolutions.{i + 1}.weight"] = (E,)
        s[f"encoder.convolutions.{i + 1}.bias"] = (E,)
    # adjacent pairs (forward, reverse) -> single (8H, E) / (8H,) operands
    s["encoder.lstm.weight_ih_l0"] = (2 * E, E)
    s["encoder.lstm.weight_ih_l0_reverse"] = (2 * E, E)
    s["encoder.lstm.bias_ih_l0"] = (2 * E,)
    s["encoder.lstm.bias_ih_l0_reverse"] = (2 * E,)
    s["encoder.lstm.bias_hh_l0"] = (2 * E,)
    s["encoder.lstm.bias_hh_l0_reverse"] = (2 * E,)
    s["encoder.lstm.weight_hh_l0"] = (2 * E, E // 2)
    s["encoder.lstm.weight_hh_l0_reverse"] = (2 * E, E // 2)
    if d.get("speaker_tokens"):
        s["speaker_embedding.weight"] = (d["num_speakers"], E)
    if d.get("description_embeddings"):
        s["description_embeddings_linear.0.weight"] = (128, d["description_embeddings_dim"])
        s["description_embeddings_linear.0.bias"] = (128,)
    s["prenet.0.weight"] = (P, M)
    s["prenet.3.weight"] = (P, P)
    s["att_encoder.weight"] = (Ad, Ef)
    s["decoder.att_rnn.weight_ih"] = (4 * A, P + Ef)
    s["decoder.att_rnn.weight_hh"] = (4 * A, A)
    s["decoder.att_rnn.bias_ih"] = (4 * A,)
    s["decoder.att_rnn.bias_hh"] = (4 * A,)
    s["decoder.attention.query_layer.weight"] = (Ad, A)
    s["decoder.attention.v.weight"] = (1, Ad)
    s["decoder.attention.location_conv.weight"] = (F, 2, Kl)
    s["decoder.attention.location_dense.weight"] = (Ad, F)
    s["decoder.lstm.weight_ih"] = (4 * D, A + Ef)
    s["decoder.lstm.weight_hh"] = (4 * D, D)
    s["decoder.lstm.bias_ih"] = (4 * D,)
    s["decoder.lstm.bias_hh"] = (4 * D,)
    # adjacent: (r*M+1, D+Ef) projection and (r*M+1,) bias; with a reduction factor r row j*M + m is mel bin m of a step's j-th frame
    s["decoder.mel_out.weight"] = (r * M, D + Ef)
    s["decoder.gate.weight"] = (1, D + Ef)
    s["decoder.mel_out.bias"] = (r * M,)
    s["decoder.gate.bias"] = (1,)
    chans = [M, Pn, Pn, Pn, Pn, M]
    for li in range(5):
        s[f"postnet.postnet.{4 * li}.weight"] = (chans[li + 1], chans[li], 5)
        s[f"postnet.postnet.{4 * li + 1}.weight"] = (chans[li + 1],)
        s[f"postnet.postnet.{4 * li + 1}.bias"] = (chans[li + 1],)
    # prosody-controls extension (model/decoder.py:40-48): the reference appends controls_dim input columns to the decoder
    # LSTM's weight_ih and to mel_out.weight.  They are stored as separate blocks so that [att_h | ctx] stays one K segment
    # and [mel_out ; gate] stays one (M+1, D+Ef) matrix; state_dict exchange splits / concatenates (CONTROL_SPLITS).
    C = d.get("controls_dim", 0) if d.get("controls") else 0
    if C:
        s["decoder.lstm.weight_ih#controls"] = (4 * D, C)
        s["decoder.mel_out.weight#controls"] = (r * M, C)
    return s


CONTROL_SPLITS = ("decoder.lstm.weight_ih", "decoder.mel_out.weight")


# pairs that must be contiguous without padding between them
_GLUED = {
    "encoder.lstm.weight_ih_l0", "encoder.lstm.bias_ih_l0", "encoder.lstm.bias_hh_l0", "encoder.lstm.weight_hh_l0",
    "decoder.mel_out.weight", "decoder.mel_out.bias",
}


def buffer_manifest(d: dict) -> "OrderedDict[str, tuple]":
    """BatchNorm buffers (running stats) - kept outside the learnable flat buffer."""
    E, M, Pn = d["encoded_dim"], d["num_mels"], d["postnet_dim"]
    s: "OrderedDict[str, tuple]" = OrderedDict()
    for i in (1, 5, 9):
        s[f"encoder.convolutions.{i}.running_mean"] = (E,)
        s[f"encoder.convolutions.{i}.running_var"] = (E,)
    chans = [Pn, Pn, Pn, Pn, M]
    for li in range(5):
        s[f"postnet.postnet.{4 * li + 1}.running_mean"] = (chans[li],)
        s[f"postnet.postnet.{4 * li + 1}.running_var"] = (chans[li],)
    return s


def _numel(shape) -> int:
    n = 1
    for x in shape:
        n *= x
    return n


class ParamStore:
    """Owns the flat parameter, gradient and Adam-moment buffers and the name -> view tables."""

    def __init__(self, d: dict, device, with_grad: bool = True, guard_bytes: Optional[int] = None):
        """guard_bytes (tests; default T2_GUARD_BYTES, else 0): guard bands of that many bytes at both ends of flat, grad,
        exp_avg, exp_avg_sq and buf_flat (tacotron2_amd/guard.py) - the views and offsets between parameters do not change."""
        self.dims = dict(d)
        self.device = torch.device(device)
        self.guard_bytes = _guard.DEFAULT_BYTES if guard_bytes is None else int(guard_bytes)
        self._guards: Dict[str, tuple] = {}
        man = param_manifest(d)
        offs, off = OrderedDict(), 0
        for name, shp in man.items():
            offs[name] = off
            n = _numel(shp)
            off += n if name in _GLUED else (n + 3) // 4 * 4
        self.numel = (off + 3) // 4 * 4
        self.offsets, self.shapes = offs, man
        self.flat = self._zeros("flat", self.numel)
        self.grad = self._zeros("grad", self.numel) if with_grad else None
        self.exp_avg = None
        self.exp_avg_sq = None
        self.ema = None
        self.P: Dict[str, torch.Tensor] = {}
        self.G: Dict[str, torch.Tensor] = {}
        for name, shp in man.items():
            n = _numel(shp)
            self.P[name] = self.flat[offs[name]:offs[name] + n].view(shp)
            if with_grad:
                self.G[name] = self.grad[offs[name]:offs[name] + n].view(shp)
        bman = buffer_manifest(d)
        nb = sum((_numel(s) + 3) // 4 * 4 for s in bman.values())
        self.buf_flat = self._zeros("buf_flat", nb)
        self.Bf: Dict[str, torch.Tensor] = {}
        o = 0
        for name, shp in bman.items():
            n = _numel(shp)
            self.Bf[name] = self.buf_flat[o:o + n].view(shp)
            if name.endswith("running_var"):
                self.Bf[name].fill_(1.0)
            o += (n + 3) // 4 * 4
        self.num_batches_tracked = {k.replace("running_mean", "num_batches_tracked"): 0
                                    for k in bman if k.endswith("running_mean")}

    # --- concatenated operands -------------------------------------------------------------------
    def cat_view(self, first: str, rows: int, cols: int, grad: bool = False) -> torch.Tensor:
        o = self.offsets[first]
        buf = self.grad if grad else self.flat
        return buf[o:o + rows * cols].view(rows, cols) if cols > 0 else buf[o:o + rows]

    def reference_layout(self, table: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
        """Copies of `table` (self.P or self.G) under the reference's names and shapes (controls columns appended)."""
        out = OrderedDict()
        for name, v in table.items():
            if name.endswith("#controls"):
                continue
            c = table.get(name + "#controls")
            out[name] = torch.cat([v, c], 1) if c is not None else v.detach().clone()
        return out

    def init_adam(self):
        if self.exp_avg is None:
            self.exp_avg = self._zeros("exp_avg", self.numel)
            self.exp_avg_sq = self._zeros("exp_avg_sq", self.numel)

    # --- EMA of the parameters --------------------------------------------------------
    def init_ema(self):
        """The shadow buffer `ema`, a copy of `flat` (padding included, so that it stays bit-equal there); a second call keeps it."""
        if self.ema is None:
            self.ema = self._zeros("ema", self.numel)
            self.ema.copy_(self.flat)

    def swap_ema(self):
        """Exchange the contents of `flat` and `ema` in place: every pointer and view stays valid, the model then runs on the shadow
        weights until the next call.  Three elementwise copies through a temporary; not on the step path."""
        if self.ema is None:
            raise RuntimeError("ParamStore.swap_ema: no EMA buffer (init_ema)")
        tmp = self.flat.clone()
        self.flat.copy_(self.ema)
        self.ema.copy_(tmp)

    def ema_state_dict(self, prefix: str = "") -> "OrderedDict[str, torch.Tensor]":
        """state_dict() with the shadow weights in place of the parameters: same keys, same reference shapes (controls columns
        re-joined); the BatchNorm buffers are the live ones."""
        if self.ema is None:
            raise RuntimeError("ParamStore.ema_state_dict: no EMA buffer (init_ema)")
        table = {}
        for name, shp in self.shapes.items():
            o = self.offsets[name]
            table[name] = self.ema[o:o + _numel(shp)].view(shp)
        out = OrderedDict()
        for name, v in self.reference_layout(table).items():
            out[prefix + name] = v
        for name, v in self.Bf.items():
            out[prefix + name] = v.detach().clone()
        for name, v in self.num_batches_tracked.items():
            out[prefix + name] = torch.tensor(v, dtype=torch.int64)
        return out

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = ""):
        """The shadow weights of an ema_state_dict into `ema` (allocated if need be); keys that are no parameter are ignored."""
        self.init_ema()
        ctrl = any(n.endswith("#controls") for n in self.P)
        for name, shp in self.shapes.items():
            if name.endswith("#controls"):
                continue
            if prefix + name not in sd:
                raise KeyError(f"missing key in ema_state_dict: {prefix + name}")
            t = torch.as_tensor(sd[prefix + name]).to(torch.float32)
            if ctrl and name in CONTROL_SPLITS:
                k0 = shp[1]
                oc = self.offsets[name + "#controls"]
                self.ema[oc:oc + t[:, k0:].numel()].copy_(t[:, k0:].reshape(-1))
                t = t[:, :k0]
            o = self.offsets[name]
            self.ema[o:o + _numel(shp)].copy_(t.reshape(-1))

    # --- guard bands (tests) ------------------------------------------------------------------------
    def _zeros(self, name: str, n: int) -> torch.Tensor:
        if self.guard_bytes <= 0:
            return torch.zeros(n, dtype=torch.float32, device=self.device)
        backing, v, g = _guard.alloc(n, torch.float32, self.device, self.guard_bytes)
        self._guards[name] = (backing, g, n)
        return v.zero_()

    def guard_check(self) -> list:
        """Band hits of the flat buffers (the caller synchronises): [(name, side, offset, count, first values)]."""
        hits = []
        for name, (backing, g, n) in self._guards.items():
            hits += _guard.scan("ps." + name, backing, g, n)
        return hits

    # --- state_dict exchange (reference layout) -----------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = "", strict: bool = True):
        missing = []
        ctrl = any(n.endswith("#controls") for n in self.P)
        for name in self.P:
            if name.endswith("#controls"):
                continue                     # filled together with its base tensor below
            key = prefix + name
            if key in sd:
                t = torch.as_tensor(sd[key]).to(torch.float32)
                if name in ("decoder.mel_out.weight", "decoder.mel_out.bias") and t.shape[0] != self.shapes[name][0]:
                    M, r = self.dims["num_mels"], reduction_factor(self.dims)
                    theirs = t.shape[0] // M if t.shape[0] % M == 0 else f"{t.shape[0]}/{M}"
                    raise ValueError(f"{key} has {t.shape[0]} rows: the checkpoint was written with reduction_factor = {theirs}, this "
                                     f"model is configured with reduction_factor = {r} ({r} x {M} = {r * M} rows)")
                if ctrl and name in CONTROL_SPLITS:       # reference layout: [main columns | controls columns]
                    k0 = self.shapes[name][1]
                    self.P[name + "#controls"].copy_(t[:, k0:])
                    t = t[:, :k0]
                self.P[name].copy_(t.reshape(self.shapes[name]))
            else:
                missing.append(key)
        for name in self.Bf:
            key = prefix + name
            if key in sd:
                self.Bf[name].copy_(torch.as_tensor(sd[key]).to(torch.float32))
            else:
                missing.append(key)
        for name in self.num_batches_tracked:
            if prefix + name in sd:
                self.num_batches_tracked[name] = int(sd[prefix + name])
        if strict and missing:
            raise KeyError(f"missing keys in state_dict: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        return missing

    def state_dict(self, prefix: str = "") -> "OrderedDict[str, torch.Tensor]":
        out = OrderedDict()
        for name, v in self.reference_layout(self.P).items():
            out[prefix + name] = v
        for name, v in self.Bf.items():
            out[prefix + name] = v.detach().clone()
        for name, v in self.num_batches_tracked.items():
            out[prefix + name] = torch.tensor(v, dtype=torch.int64)
        return out
