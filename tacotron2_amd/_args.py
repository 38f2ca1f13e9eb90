"""The argument checks of the Python layer, each rule written once.  The kernels index raw pointers and take strides and counts on
trust: what these functions let through is what reaches them.  Every check takes the caller's name `fn` and the argument's name,
raises ValueError(f"{fn}: ...") and returns what the caller needs; the order of a caller's checks is the order of its calls."""
from __future__ import annotations

import math
import numbers

import torch

from ._lib import K

YIN_MAX_SPAN = K["YIN_MAX_SPAN"]         # W + tau_max floats of one frame's span in LDS


def int_arg(fn: str, name: str, v, lo=None, hi=None) -> int:
    """v a Python integer (no bool), >= lo, <= hi."""
    want = "an integer" if lo is None else f"an integer >= {lo}" if hi is None else f"an integer in {lo} .. {hi}"
    if isinstance(v, bool) or not isinstance(v, int) or (lo is not None and v < lo) or (hi is not None and v > hi):
        raise ValueError(f"{fn}: {name} must be {want}, got {v!r}")
    return v


def real_arg(fn: str, name: str, v, nonneg: bool = False) -> float:
    """v a finite real number (no bool), >= 0 with nonneg."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or (nonneg and v < 0):
        raise ValueError(f"{fn}: {name} must be a finite number{' >= 0' if nonneg else ''}, got {v!r}")
    return float(v)


def batch_arg(fn: str, B: int) -> None:
    """B utterances as one grid dimension."""
    if B < 1 or B > 65535:
        raise ValueError(f"{fn}: batch of {B}, outside 1 .. 65535")


def tensor_arg(fn: str, name: str, x, rank: int, shape: str, dtype=torch.float32) -> None:
    """x a tensor of that rank and dtype; `shape` names the dimensions in the message."""
    if not torch.is_tensor(x) or x.dim() != rank or x.dtype != dtype:
        raise ValueError(f"{fn}: {name} must be a {str(dtype)[6:]} {shape} tensor")


def on_gpu(fn: str, name: str, x) -> None:
    if x.device.type != "cuda":
        raise ValueError(f"{fn}: {name} must be on the GPU, got {x.device}")


def on_device(fn: str, name: str, x, dev, engine: bool = False) -> None:
    """x a tensor on dev: the device of the signals, or with `engine` the engine's."""
    if not torch.is_tensor(x) or x.device != dev:
        where = f"the engine's device {dev}" if engine else f"the device of the signals, {dev}"
        raise ValueError(f"{fn}: {name} must be a tensor on {where}")


def int_vector(fn: str, name: str, n, B: int) -> None:
    if n.dim() != 1 or n.shape[0] != B or n.is_floating_point() or n.dtype == torch.bool:
        raise ValueError(f"{fn}: {name} must be {B} integers")


def lengths(fn: str, name: str, n, B: int, dev, engine: bool = False):
    """n the B integer lengths as a tensor on dev.  Returns n: the caller converts it to the kernel's integer type."""
    on_device(fn, name, n, dev, engine)
    int_vector(fn, name, n, B)
    return n


def lags(fn: str, sr, fmin, fmax):
    """(tau_min, tau_max) of a pitch range in Hz: sr // fmax and sr // fmin."""
    int_arg(fn, "sr", sr, 1)
    if not (math.isfinite(fmin) and math.isfinite(fmax) and 0 < fmin < fmax):
        raise ValueError(f"{fn}: need 0 < fmin < fmax, got fmin = {fmin!r}, fmax = {fmax!r}")
    return int(sr // fmax), int(sr // fmin)


def usable_lags(fn: str, tau_min: int, tau_max: int, sr, fmin, fmax) -> None:
    """What the pitch kernels need of lags(): no lag below 2 and at least two lags."""
    if tau_min < 2 or tau_max <= tau_min + 1:
        raise ValueError(f"{fn}: lags {tau_min} .. {tau_max} of {fmin} .. {fmax} Hz at {sr} Hz: need tau_min >= 2 and "
                         "tau_max > tau_min + 1")


def last_contiguous(fn: str, name: str, x) -> None:
    if x.shape[-1] > 1 and x.stride(-1) != 1:
        raise ValueError(f"{fn}: the last dimension of {name} must be contiguous")


def row_stride(fn: str, name: str, x, unit: str = "samples") -> int:
    """The row stride in elements of a (B, ld) view with a contiguous last dimension whose rows do not overlap - a contiguous
    tensor, or a cut such as big[:, :ld].  One row takes the stride of the contiguous layout, at least 1."""
    last_contiguous(fn, name, x)
    B, ld = x.shape
    ldx = x.stride(0) if B > 1 else max(ld, 1)
    if ldx < ld:
        raise ValueError(f"{fn}: overlapping rows of {name} (row stride {ldx}, {ld} {unit})")
    return ldx


def wav_rows(fn: str, name: str, x, max_samples=None):
    """The front of time_stretch, psola and join_audio: a padded batch x (B, ld) float32 of 1 .. 65535 rows of at most max_samples
    samples, row_stride's layout.  Returns (B, ld, ldx); the counts and the device are the caller's to check, in its own order."""
    tensor_arg(fn, name, x, 2, "(B, samples)")
    B, ld = x.shape
    batch_arg(fn, B)
    if max_samples is not None and ld > max_samples:
        raise ValueError(f"{fn}: rows of {ld} samples, above the limit of {max_samples}")
    return B, ld, row_stride(fn, name, x)


def padded_wav(fn: str, wav, n, n_max, sr, hop, W, fmin, fmax):
    """The front of yin and voice_quality: a padded batch wav (B, ld) float32 on the GPU, its counts n, the largest count n_max
    (None: ld) and the frame geometry.  Returns (B, ld_wav, n_max, n as int64, T = 1 + n_max // hop, tau_min, tau_max)."""
    tensor_arg(fn, "wav", wav, 2, "(B, samples)")
    on_gpu(fn, "wav", wav)
    B, ld = wav.shape
    batch_arg(fn, B)
    last_contiguous(fn, "wav", wav)
    n_max = ld if n_max is None else int(n_max)
    ld_wav = wav.stride(0) if B > 1 else max(ld, 1)
    if not 0 <= n_max <= ld or (B > 1 and ld_wav < n_max):
        raise ValueError(f"{fn}: n_max = {n_max} outside 0 .. {ld}, the row length of wav (row stride {ld_wav})")
    n64 = lengths(fn, "n", n, B, wav.device).to(torch.int64).contiguous()
    int_arg(fn, "hop", hop)
    int_arg(fn, "W", W)
    tau_min, tau_max = lags(fn, sr, fmin, fmax)
    if hop < 1 or W < 16:
        raise ValueError(f"{fn}: need hop >= 1 and W >= 16, got hop = {hop}, W = {W}")
    usable_lags(fn, tau_min, tau_max, sr, fmin, fmax)
    if W + tau_max > YIN_MAX_SPAN:
        raise ValueError(f"{fn}: W + tau_max = {W + tau_max} samples per frame, above the limit of {YIN_MAX_SPAN} (T2_YIN_MAX_SPAN)")
    return B, ld_wav, n_max, n64, 1 + n_max // hop, tau_min, tau_max


def same_shape_2d(fn: str, arrays, dtypes=None):
    """arrays: (name, x) pairs, the first the reference: contiguous (B, T) tensors of one shape on one GPU, float32 unless dtypes
    names another type for a name.  Returns (B, T)."""
    ref_name, ref = arrays[0]
    for name, x in arrays:
        tensor_arg(fn, name, x, 2, "(B, T)", (dtypes or {}).get(name, torch.float32))
        if x.device.type != "cuda" or x.device != ref.device:
            raise ValueError(f"{fn}: {name} must be on the GPU, all on one device")
        if x.shape != ref.shape or not x.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous and of the shape of {ref_name} {tuple(ref.shape)}")
    return tuple(ref.shape)


def dense_arg(fn: str, name: str, x, shape, dev, dtype=torch.float32) -> None:
    """x a contiguous tensor of that shape and dtype on dev; None in shape is any size >= 1."""
    if not torch.is_tensor(x) or x.dtype != dtype or x.device != dev or x.dim() != len(shape) or not x.is_contiguous() \
            or any(have < 1 if want is None else have != want for have, want in zip(x.shape, shape)):
        dims = ", ".join("T >= 1" if want is None else str(want) for want in shape)
        raise ValueError(f"{fn}: {name} must be a contiguous {str(dtype)[6:]} ({dims}) tensor on {dev}")


def strided_3d(fn: str, name: str, x):
    """The strides (ld_b, ld_t) in elements of a (B, T, C) view with a contiguous last dimension whose rows and batch items do not
    overlap - a contiguous tensor, or a cut such as x[:, :T, :C] of a larger one.  The kernels multiply ld_b by the batch index
    and ld_t by the frame index only, so a dimension of size 1 takes the stride of the contiguous layout."""
    last_contiguous(fn, name, x)
    B, T, C = x.shape
    ld_t = x.stride(1) if T > 1 else C
    ld_b = x.stride(0) if B > 1 else T * ld_t
    if ld_t < C or (B > 1 and ld_b < (T - 1) * ld_t + C):
        raise ValueError(f"{fn}: overlapping rows of {name} (strides {tuple(x.stride())})")
    return ld_b, ld_t


def flag_arg(fn: str, name: str, v) -> int:
    """v a bool, or the integer 0 or 1."""
    if not isinstance(v, (bool, int)) or v not in (0, 1):
        raise ValueError(f"{fn}: {name} must be a flag (a bool, 0 or 1), got {v!r}")
    return int(v)


def counts32(fn: str, name: str, v, B: int, dev, hi=None):
    """B integer counts for a kernel that takes them as int32 on dev.  Host integers (a sequence, a numpy array, a CPU tensor) are
    checked here, 0 <= v[b] <= hi, and their sum is known without a read; a tensor on dev is checked for type and shape alone
    (int_vector) - its values are the kernel's to refuse.  Returns (the int32 tensor on dev, the host's sum or None)."""
    if torch.is_tensor(v) and v.device.type == "cuda":
        lengths(fn, name, v, B, dev)
        return v.to(torch.int32).contiguous(), None
    try:
        t = torch.as_tensor(v)
    except Exception:
        raise ValueError(f"{fn}: {name} must be {B} integers") from None
    int_vector(fn, name, t, B)
    t = t.to(torch.int64)
    if int(t.min()) < 0 or (hi is not None and int(t.max()) > hi):
        raise ValueError(f"{fn}: {name} must lie in 0 .. {'' if hi is None else hi}, got {int(t.min())} .. {int(t.max())}")
    return t.to(torch.int32).to(dev), int(t.sum())
