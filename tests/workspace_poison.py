"""Poisoned workspaces for tests that reuse ONE engine over many calls ("Workspace poison").

Engine.buf hands out `t[:n]` of whatever larger tensor an earlier call left under the name, and what has to be zero goes through
need_zero / clear_ahead / prezero / zero_later and one t2_zero_regions launch.  A test that builds a fresh engine per case cannot see
a missing clear: a fresh torch.empty from the caching allocator is very often zero, and a second step of nearly the same shape
leaves nearly the same numbers behind.  poison() makes the interior of every floating-point workspace implausible between two
calls instead, and dirty_allocator() does the same for the memory that the next torch.empty of Engine.out and of the engine's
temporaries gets back from the caching allocator.  A read of something the call did not write or clear is then wrong by orders of
magnitude, and the caller's comparison with its reference sees it.

Rules (part of the design):
  * finite values only: two runs use +P and -Q, about 1e4 in magnitude - far above any activation of these models, squares finite in
    float32.  No NaN: the engine legitimately multiplies never-written pad rows and masked positions by exact zeros.
  * integer workspaces (win_peak, inf*.lengths, done, state, ...) are never touched: kernels read them as indices and row counts.
    Stale integers come from the SEQUENCE of calls instead (other B, N, stop frames).
  * Engine._persist_sync (arrival counters, timeout flag of the persistent launches) is not a named workspace and is never touched.
  * SKIP: float workspaces whose VALUES a kernel turns into an index or a trip count would go here, each with the file and line as
    its reason - at most MAX_SKIP names, none of NEVER_SKIPPED.  The kernels the engine's training step, eval forward and decode run
    (csrc/t2_gemm.hip, t2_lstm.hip, t2_attention.hip, t2_elementwise.hip, t2_infer.hip) were read for such conversions: every integer
    cast there is of an index expression, and the attention window's peak is computed and kept as an integer (win_peak).  So the
    list is empty.

skip_clear() is the harness's own proof: one named float region stays uncleared, and the comparison must notice under poison.

Imported like the other helpers of this directory; tests/test_workspace_poison_host.py drives it on a CPU-device engine,
tests/test_gpu_engine_reuse.py on the device."""
import fnmatch
import math

import torch

P_POS = 1.0e4                  # +P
Q_NEG = -1.3e4                 # -Q
MAX_SKIP = 5
SKIP = {}                      # workspace name -> "file:line: what converts its value to an index or a trip count"
# never on the skip list: the time-major stashes, the split-K and gradient accumulators, bn.sums, pack.*, proj, mel_tm
NEVER_SKIPPED = ("xdec", "xdec_t", "dech_t", "att_c", "cum", "xproj", "dec_c", "enc.h", "enc.c", "enc.ht", "enc.gates", "gates_att",
                 "gates_dec", "th", "dgd", "dgd_t", "Zatt", "Zatt_t", "dp2", "enc.dgt", "de_stash", "p1", "p2", "pre_att", "pre_dec",
                 "*.dwp", "*.raw", "*.dx", "enc.dx3", "enc.dpre", "enc.dc", "dpmT", "dv_part", "dU_part", "dU", "dc_dec", "dc_att",
                 "dhz_dec", "dhz_att", "db_dec", "db_att", "ctl.*", "ddesc", "bn.sums", "*.sums", "pack.*", "proj", "mel_tm")


def check_skip_list(skip) -> None:
    assert len(skip) <= MAX_SKIP, f"the skip list holds {len(skip)} names, at most {MAX_SKIP} are allowed"
    for name, reason in skip.items():
        assert not any(fnmatch.fnmatchcase(name, pat) for pat in NEVER_SKIPPED), f"{name} must never be skipped"
        assert isinstance(reason, str) and ":" in reason, f"{name}: the reason names the file and line of the conversion"


def _sync(dev) -> None:
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize(dev)


def poison(eng, value: float, skip=None):
    """Fill every floating-point entry of eng._ws with `value`, over its whole allocation: (poisoned names, skipped names).  Without
    guard bands the entry IS the backing tensor - the largest one any call asked for, not the last view handed out; with guard bands
    it is the exact-size view between the bands, which stay as they are.  Skipped: the integer workspaces and the names on `skip`."""
    skip = SKIP if skip is None else skip
    check_skip_list(skip)
    value = float(value)
    assert math.isfinite(value) and value * value < torch.finfo(torch.float32).max, f"poison must be finite, and its square too: {value}"
    _sync(eng.dev)
    poisoned, skipped = [], []
    for name, t in eng._ws.items():
        if not t.is_floating_point() or name in skip:
            skipped.append(name)
            continue
        t.fill_(value)
        poisoned.append(name)
    _sync(eng.dev)
    return poisoned, skipped


def dirty_allocator(dev, sizes, value: float) -> list:
    """Allocate one tensor per byte size in `sizes`, fill it with `value`, free them all: the caching allocator hands such a block to
    the next torch.empty of a fitting size on the same stream (stream order puts the fill in front of that tensor's first use).
    Returns the addresses, for a test that wants to see one come back."""
    value = float(value)
    assert math.isfinite(value)
    blocks = [torch.empty(max(1, (int(n) + 3) // 4), dtype=torch.float32, device=dev).fill_(value) for n in sizes]
    ptrs = [b.data_ptr() for b in blocks]
    del blocks
    return ptrs


# ---- the harness's own proof ---------------------------------------------------------------------------------------------------
CLEAR_SKIPPABLE = ("pre_dec", "dpmT", "dv_part", "dU_part", "dc_dec", "dc_att", "*.dwp")      # split-K / gradient accumulators


def skip_clear(monkeypatch, engine_cls, name: str) -> list:
    """Engine.need_zero - and clear_ahead, the prologue half of the same contract - hand out every region inside the float workspace
    `name` WITHOUT clearing it.  Never a counter, a flag or an integer buffer: asserted.  Returns the list the skipped regions
    (address, bytes) are appended to."""
    assert any(fnmatch.fnmatchcase(name, pat) for pat in CLEAR_SKIPPABLE), name
    real_need, real_ahead = engine_cls.need_zero, engine_cls.clear_ahead
    skipped = []

    def inside(eng, v):
        t = eng._ws.get(name)
        if t is None or not (t.data_ptr() <= v.data_ptr() < t.data_ptr() + t.numel() * t.element_size()):
            return False
        assert t.is_floating_point() and v.is_floating_point(), f"{name}: only float regions may stay uncleared"
        skipped.append((v.data_ptr(), v.numel() * v.element_size()))
        return True

    def need_zero(self, v):
        if inside(self, v):
            self._cleared.pop((v.data_ptr(), v.numel() * v.element_size()), None)
            return v
        return real_need(self, v)

    def clear_ahead(self, v, nm=""):
        return v if inside(self, v) else real_ahead(self, v, nm)

    monkeypatch.setattr(engine_cls, "need_zero", need_zero)
    monkeypatch.setattr(engine_cls, "clear_ahead", clear_ahead)
    return skipped
