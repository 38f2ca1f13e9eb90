"""Sample-rate conversion on the device (C-ABI t2_resample): what the reference's offline preprocessing does with librosa
and pydub (preprocessing/hifi_tts.py:73-78), as one launch in front of the batched log-mel pass and behind the vocoder in `say`.

The filter is designed here, on the host, in float64, once per rate pair: a Kaiser-windowed sinc with ZEROS zero crossings on each side,
cut at ROLLOFF of the lower of the two Nyquist rates, as a polyphase table of U rows (one per output phase) of 2K taps; the kernel takes
any such table.  tests/resample_ref.py restates the design and the kernel's rule in float64."""
from __future__ import annotations

import math
import threading
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .._lib import call, make

ZEROS, ROLLOFF, BETA = 16, 0.90, 9.0
TABLE_LIMIT = 1 << 20          # U * 2K floats: t2_resample's limit


def ratio(sr_in: int, sr_out: int) -> Tuple[int, int]:
    """(U, D) of sr_out / sr_in in lowest terms."""
    for name, v in (("sr_in", sr_in), ("sr_out", sr_out)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"resample: {name} must be an integer >= 1, got {v!r}")
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def out_len(n_in: int, U: int, D: int) -> int:
    """ceil(n_in * U / D): the samples t2_resample writes for n_in input samples."""
    return -((-int(n_in) * U) // D)


_PLANS: Dict[Tuple[int, int], tuple] = {}
_PLANS_LOCK = threading.Lock()


def plan(sr_in: int, sr_out: int):
    """(U, D, K, table) of one rate pair, cached: table (U, 2K) float32, row p = the taps k = -K+1 .. K of output phase p,
    h_p[k] = fc sinc(fc d) I0(beta sqrt(1 - (d / W)^2)) / I0(beta) for |d| < W, d = k - p / U, fc = ROLLOFF * s, W = ZEROS / s input
    samples, s = min(1, U / D), K = ceil(W); every row is normalised to sum 1 in float64, then rounded.  A pair whose table would
    hold more than 2^20 floats is an error."""
    U, D = ratio(sr_in, sr_out)
    key = (int(sr_in), int(sr_out))
    with _PLANS_LOCK:
        got = _PLANS.get(key)
    if got is not None:
        return got
    s = min(1.0, U / D)
    W = ZEROS / s
    K = int(math.ceil(W))
    if U * 2 * K > TABLE_LIMIT:
        raise ValueError(f"resample: {sr_in} Hz -> {sr_out} Hz is the ratio {U} / {D}: a table of {U} phases x {2 * K} taps = "
                         f"{U * 2 * K} floats, above the limit of {TABLE_LIMIT}")
    fc = ROLLOFF * s
    k = np.arange(-K + 1, K + 1, dtype=np.float64)[None, :]
    d = k - (np.arange(U, dtype=np.float64) / U)[:, None]
    inside = np.abs(d) < W
    win = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - (d / W) ** 2, 0.0))) / np.i0(BETA)
    h = np.where(inside, fc * np.sinc(fc * d) * win, 0.0)
    h /= h.sum(1, keepdims=True)
    h /= h.sum(1, keepdims=True)
    got = (U, D, K, np.ascontiguousarray(h.astype(np.float32)))
    with _PLANS_LOCK:
        _PLANS.setdefault(key, got)
    return got


def resample(wav: torch.Tensor, n, table: torch.Tensor, U: int, D: int, K: int, out: torch.Tensor = None, ldy: int = None):
    """t2_resample on a padded batch: wav (B, ldx) float32 on the GPU, n the B sample counts (a sequence of host integers), table (U, 2K)
    float32 on the same device.  Returns (out, n_out): out (B, ldy) float32 with row b = the ceil(n[b] U / D) resampled samples and
    zeros behind them (ldy: default the longest row rounded up to 64; `out`, when given, is written instead and sets ldy), n_out the
    host integers.  Enqueued on the current stream; nothing is read back."""
    if not torch.is_tensor(wav) or wav.dim() != 2 or wav.dtype != torch.float32 or wav.device.type != "cuda":
        raise ValueError("resample: wav must be a float32 (B, samples) tensor on the GPU")
    B, ldx = wav.shape
    if B < 1 or B > 65535:
        raise ValueError(f"resample: batch of {B}, outside 1 .. 65535")
    if ldx > 1 and wav.stride(1) != 1:
        raise ValueError("resample: the last dimension of wav must be contiguous")
    n = [int(v) for v in n]
    if len(n) != B or any(v < 0 or v > ldx for v in n):
        raise ValueError(f"resample: n must be {B} sample counts in 0 .. {ldx}")
    if (not torch.is_tensor(table) or table.device != wav.device or table.dtype != torch.float32 or not table.is_contiguous()
            or tuple(table.shape) != (U, 2 * K)):
        raise ValueError(f"resample: table must be a contiguous float32 ({U}, {2 * K}) tensor on {wav.device}")
    n_out = [out_len(v, U, D) for v in n]
    if out is None:
        ldy = (max(n_out) + 63) // 64 * 64 if ldy is None else int(ldy)
        if ldy < max(n_out):
            raise ValueError(f"resample: ldy = {ldy} below the longest output, {max(n_out)} samples")
        with torch.cuda.device(wav.device):
            out = torch.empty(B, ldy, dtype=torch.float32, device=wav.device)
    else:
        if (not torch.is_tensor(out) or out.device != wav.device or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B
                or not out.is_contiguous() or out.shape[1] < max(n_out)):
            raise ValueError(f"resample: out must be a contiguous float32 ({B}, >= {max(n_out)}) tensor on {wav.device}")
        ldy = out.shape[1]
    if ldy == 0:
        return out, n_out
    with torch.cuda.device(wav.device):
        n_dev = torch.tensor(n, dtype=torch.int64).to(wav.device, non_blocking=True)
        a = make("T2Resample", x=wav, ldx=wav.stride(0) if B > 1 else max(ldx, 1), n_in=n_dev, y=out, ldy=ldy, n_out_max=max(n_out),
                 table=table, U=U, D=D, K=K, B=B)
        call("t2_resample", a, torch.cuda.current_stream().cuda_stream)
    return out, n_out


class Resampler:
    """Signals of any rate brought to `sr_out` on `device`.  Plans are cached per input rate, with their tables on the device."""

    def __init__(self, sr_out: int, device="cuda:0"):
        self.sr_out, self.device = int(sr_out), torch.device(device)
        self._tables: Dict[int, tuple] = {}
        self._lock = threading.Lock()

    def plan(self, sr_in: int):
        """(U, D, K, table on the device) of one input rate."""
        with self._lock:
            got = self._tables.get(int(sr_in))
            if got is None:
                U, D, K, table = plan(int(sr_in), self.sr_out)
                got = (U, D, K, torch.from_numpy(table).to(self.device))
                self._tables[int(sr_in)] = got
        return got

    def out_len(self, n_in: int, sr_in: int) -> int:
        U, D = ratio(sr_in, self.sr_out)
        return out_len(n_in, U, D)

    def batch(self, wavs_dev: torch.Tensor, n_in: Sequence[int], sr_in: int, ldy: int = None):
        """wavs_dev (B, ldx) float32 on the device, rows of n_in[b] samples at sr_in -> (out_dev (B, ldy), n_out): see resample().
        sr_in == sr_out: the input itself comes back."""
        if int(sr_in) == self.sr_out:
            return wavs_dev, [int(v) for v in n_in]
        U, D, K, table = self.plan(sr_in)
        return resample(wavs_dev, n_in, table, U, D, K, ldy=ldy)

    def one(self, wav_np: np.ndarray, sr_in: int) -> np.ndarray:
        """One host signal -> its resampled float32 host array (up, one launch, down)."""
        x = np.ascontiguousarray(wav_np, dtype=np.float32).reshape(-1)
        if int(sr_in) == self.sr_out:
            return x
        if len(x) == 0:
            plan(int(sr_in), self.sr_out)          # (a pair beyond the table limit is refused whatever the length)
            return x
        with torch.cuda.device(self.device):
            out, n_out = self.batch(torch.from_numpy(x).to(self.device)[None, :], [len(x)], sr_in)
            return np.ascontiguousarray(out[0, :n_out[0]].cpu().numpy())
