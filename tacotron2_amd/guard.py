"""Guard bands around device allocations (test-only, off by default: Engine.guard_bytes, ParamStore(guard_bytes=...)).

An allocation of n elements becomes [band | n | band]: the view in the middle is handed out, both bands hold a fixed pattern
written once, and `scan` finds every band element that no longer holds it - a kernel that wrote past either end of the view.
Float bands hold one quiet-NaN bit pattern: a write is seen by its bits, a read past the end when the NaN reaches a compared output
or gradient.  Integer bands hold 0: integer workspaces are read by kernels as indices, row counts and addresses (win_peak,
inf.lengths, done, state), and a band must never hold a value that could send a kernel out of range - so they only detect writes.
The band size is a multiple of 512 bytes, so every view keeps the caching allocator's alignment (kernels use 16-byte accesses).

T2_GUARD_BYTES (read once, like T2_LIB_PATH): the default band size of every Engine and ParamStore of the process - the whole GPU
suite can be run guarded by hand."""
from __future__ import annotations

import os

import torch

DEFAULT_BYTES = int(os.environ.get("T2_GUARD_BYTES", "0"))
FLOAT_BITS = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5)}


def _words(t: torch.Tensor) -> torch.Tensor:
    """`t` as integers of its own width (bitwise comparison), or `t` itself for an integer dtype."""
    iv = FLOAT_BITS.get(t.dtype)
    return t.view(iv[0]) if iv is not None else t


def pattern(dtype) -> int:
    return FLOAT_BITS[dtype][1] if dtype in FLOAT_BITS else 0


def alloc(n: int, dtype, device, guard_bytes: int, short: int = 0):
    """(backing, view, g): n + 2g elements, g = guard_bytes / element size, the view [g, g + n) and both bands filled.  `short` > 0
    (test hook) starts the after-band that many elements BEFORE the view's end: the last `short` elements of the view are then
    checked as band - writes there stay inside the allocation."""
    es = torch.empty(0, dtype=dtype).element_size()
    assert guard_bytes > 0 and guard_bytes % 512 == 0, f"guard bands: a positive multiple of 512 bytes, got {guard_bytes}"
    assert 0 <= short <= n
    g = guard_bytes // es
    backing = torch.empty(n + 2 * g, dtype=dtype, device=device)
    w = _words(backing)
    w[:g].fill_(pattern(dtype))
    w[g + n - short:].fill_(pattern(dtype))
    return backing, backing[g:g + n], g


def scan(name: str, backing: torch.Tensor, g: int, n: int, short: int = 0) -> list:
    """Band hits of one allocation: [(name, "before" | "after", offset of the first bad element from the view's first element,
    number of bad elements, first values)]."""
    w = _words(backing)
    fill = pattern(backing.dtype)
    hits = []
    for side, lo, hi in (("before", 0, g), ("after", g + n - short, n + 2 * g)):
        bad = (w[lo:hi] != fill).nonzero().flatten()
        if bad.numel():
            i0 = lo + int(bad[0])
            hits.append((name, side, i0 - g, int(bad.numel()), backing[i0:i0 + 4].tolist()))
    return hits


def describe(hits: list) -> str:
    return "; ".join(f"{n} {side} (offset {o}, {c} elements, {v})" for n, side, o, c, v in hits)
