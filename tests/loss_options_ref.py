"""Float64 restatement of the loss options and of the stop threshold, for tests.  CPU only, plain torch.

With len_b the utterance's mel length a frame (b, t) is VALID when t < min(len_b, T); n_f = the number of valid frames.
  mel_loss  "l2": e^2, "l1": |e| (gradient sign(e), sign(0) = 0), "l1+l2": the sum of the two means; for mels and mels_post alike
  masked    the sums run over the valid frames only; the gate term is divided by n_f, the mel terms by n_f * M; n_f = 0: zeros.
            Not masked: the sums run over all B*T frames (padding included, as the reference's mean) and are divided by B*T, B*T*M
  stop_weight w: per frame y softplus(-x) + w (1 - y) softplus(x), gradient sigmoid(x) (y + w (1 - y)) - y; the divisor is the count
Gradients are with respect to the tensors BEFORE masking: positions at or beyond len_b are constants, their gradient is 0 in either
mode.  `loss_terms` is differentiable (autograd on it gives `loss_grads` at the valid positions); `loss_grads` is the closed form.

Stop threshold tau: a step stops when logit < logit(tau) = log(tau / (1 - tau)), formed in double and rounded to float32; the count
rule counts logit >= logit(tau) among the steps the loop ran."""
import math

import numpy as np
import torch

MEL_LOSSES = ("l2", "l1", "l1+l2")


def valid_mask(lens, T):
    """(B, T) bool: t < min(len_b, T)."""
    return torch.arange(T)[None, :] < torch.as_tensor(lens).to(torch.int64)[:, None]


def _mel_term(e, kind):
    if kind == "l2":
        return e * e
    if kind == "l1":
        return e.abs()
    return e.abs() + e * e


def _mel_grad(e, kind):
    if kind == "l2":
        return 2 * e
    if kind == "l1":
        return torch.sign(e)
    return torch.sign(e) + 2 * e


def _softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def loss_terms(mels, post, gates, mel_tgt, gate_tgt, lens, mel_loss="l2", masked=False, stop_weight=1.0):
    """(gate, mel, post) as 0-d tensors of the inputs' dtype; mels/post/mel_tgt (B,T,M), gates/gate_tgt (B,T,1).  In masked mode the
    invalid positions are indexed away, not multiplied by 0: NaN there reaches nothing."""
    assert mel_loss in MEL_LOSSES
    B, T, M = mels.shape
    x, y = gates.reshape(B, T), gate_tgt.reshape(B, T)
    if masked:
        v = valid_mask(lens, T)
        n_f = int(v.sum())
        if n_f == 0:
            z = torch.zeros((), dtype=mels.dtype)
            return z, z.clone(), z.clone()
        x, y = x[v], y[v]
        e1, e2 = mels[v] - mel_tgt[v], post[v] - mel_tgt[v]
        dg, dm = n_f, n_f * M
    else:
        e1, e2 = mels - mel_tgt, post - mel_tgt
        dg, dm = B * T, B * T * M
    gate = (y * _softplus(-x) + stop_weight * (1 - y) * _softplus(x)).sum() / dg
    return gate, _mel_term(e1, mel_loss).sum() / dm, _mel_term(e2, mel_loss).sum() / dm


def loss_grads(mels, post, gates, mel_tgt, gate_tgt, lens, mel_loss="l2", masked=False, stop_weight=1.0, grad_scale=1.0):
    """(d_mels, d_post, d_gates) of gate + mel + post in closed form, float64, exactly 0 at the invalid positions."""
    B, T, M = mels.shape
    v = valid_mask(lens, T)
    n_f = int(v.sum())
    dg, dm = (n_f, n_f * M) if masked else (B * T, B * T * M)
    zm, zg = torch.zeros(B, T, M, dtype=torch.float64), torch.zeros(B, T, 1, dtype=torch.float64)
    if n_f == 0:
        return zm, zm.clone(), zg
    c = lambda t: torch.where(v.reshape(B, T, *([1] * (t.dim() - 2))), t.double(), torch.zeros((), dtype=torch.float64))
    tg = c(mel_tgt)
    d_mels = torch.where(v[:, :, None], _mel_grad(c(mels) - tg, mel_loss) / dm, zm) * grad_scale
    d_post = torch.where(v[:, :, None], _mel_grad(c(post) - tg, mel_loss) / dm, zm) * grad_scale
    x, y = c(gates), c(gate_tgt)
    d_gates = torch.where(v[:, :, None], (torch.sigmoid(x) * (y + stop_weight * (1 - y)) - y) / dg, zg) * grad_scale
    return d_mels, d_post, d_gates


def pack_dproj(d_mels, d_post, d_gates, r):
    """The packed projection gradient [S][B][r*M + 1] of a reduction factor r: column j*M + m = (d_mels + d_post) of frame s*r + j
    (zero for frames >= T), column r*M = the sum of d_gates over the step's frames."""
    B, T, M = d_mels.shape
    S = (T + r - 1) // r
    out = torch.zeros(S, B, r * M + 1, dtype=d_mels.dtype)
    for t in range(T):
        out[t // r, :, (t % r) * M:(t % r + 1) * M] = (d_mels + d_post)[:, t]
        out[t // r, :, r * M] += d_gates[:, t, 0]
    return out


def stop_logit(tau):
    """logit(tau) formed in double and rounded to float32 (returned as a Python float holding that float32); 0.5 -> 0.0."""
    return float(np.float32(math.log(tau / (1.0 - tau))))


def stop_count(logits, thr=0.0, r=1, max_len=None):
    """The count rule on stored stop logits [N][B] (N steps of r frames) against the threshold logit `thr`:
    first_b = the first step with logit < thr (N - 1 if none), the loop ends after step n* = max_b first_b, counted_b = the steps
    <= n* with logit >= thr.  Returns (lengths [B] in frames, frames emitted, steps emitted); max_len (frames) cuts the first two."""
    logits = torch.as_tensor(logits, dtype=torch.float32)
    N, B = logits.shape
    thr32 = torch.tensor(thr, dtype=torch.float32)
    below = logits < thr32
    first = [int(torch.nonzero(below[:, b])[0]) if bool(below[:, b].any()) else N - 1 for b in range(B)]
    n = max(first) + 1
    counted = (logits[:n] >= thr32).sum(0).to(torch.int64) * r
    frames = n * r
    if max_len is not None:
        counted, frames = torch.clamp(counted, max=max_len), min(frames, max_len)
    return counted, frames, n
