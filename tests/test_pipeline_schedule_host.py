"""The two frame-loop pipelines as values (engine.forward_schedule / engine.backward_schedule): no GPU, no torch tensors.
The backward schedule is held against a literal restatement of the bookkeeping that Engine.backward_tf did inline before the
schedule became a function (three mutable lists, `ci >= 4`, `len(att_done) >= 2`, and a tail that repeats the loop)."""
import itertools

import pytest

from tacotron2_amd.engine import _chunk_sizes, backward_schedule, chunk_ranges, chunk_splits, forward_schedule

TS = (1, 2, 3, 5, 15, 16, 17, 23, 63, 64, 65, 128, 150, 872, 936)
CHS = (1, 3, 5, 8, 16, 64, 80)
WGS = (1, 2, 4, 7)
DEFERRED = (0, 1, 6)
GRID = list(itertools.product(TS, CHS, WGS, DEFERRED, (True, False), (True, False)))     # T, CH, WG, n_deferred, stash, ramp


def inline_loop_restated(T, CH, WG, n_deferred, stash, ramp):
    """The former loop of backward_tf with every launch replaced by the tuple (kind, share_cu, hi, lo, k) it stands for; an event
    is the index of the chunk it was recorded behind.  share_cu is a field of the GEMM operand block only: the accumulate launch
    and the event record have none, wherever they stand, and carry False.  Returns (per-chunk (hi, lo, ops), tail ops)."""
    chunks, hi = [], T
    for n in reversed(_chunk_sizes(T, CH, ramp_at_end=ramp)):
        chunks.append((hi, hi - n)); hi -= n
    post_wgrads = list(range(n_deferred))
    dec_grp, att_done, att_grp = None, [], None        # [hi, lo, n]; [(hi, lo, event)]; [hi, lo, n, event]
    ops = None

    def att_acc(hi, lo, ev):
        if not stash:
            return
        ops.append(("att_acc", False, hi, lo, ev))
    out = []
    for ci_, (hi, lo) in enumerate(chunks):
        ops = []
        # with share_cu(...):
        dec_grp = [hi, lo, 1] if dec_grp is None else [dec_grp[0], lo, dec_grp[2] + 1]
        if dec_grp[2] >= WG:
            ops.append(("dec_wgrads", True, dec_grp[0], dec_grp[1], -1)); dec_grp = None
        if post_wgrads and ci_ >= 4:
            post_wgrads.pop(0); ops.append(("deferred", True, 0, 0, -1))
        if len(att_done) >= 2:
            h2, l2, e2 = att_done.pop(0)
            att_acc(h2, l2, e2)
            att_grp = [h2, l2, 1, e2] if att_grp is None else [att_grp[0], l2, att_grp[2] + 1, e2]
            if att_grp[2] >= WG:
                ops.append(("att_wgrads", True, att_grp[0], att_grp[1], att_grp[3])); att_grp = None
        att_done.append((hi, lo, ci_))
        out.append((hi, lo, tuple(ops)))
    ops = []
    for h2, l2, e2 in att_done[:-1]:
        att_acc(h2, l2, e2)
    while post_wgrads:
        post_wgrads.pop(0); ops.append(("deferred", False, 0, 0, -1))
    # with share_cu(...):
    if dec_grp is not None:
        ops.append(("dec_wgrads", True, dec_grp[0], dec_grp[1], -1))
    att_acc(*att_done[-1])
    ops.append(("acc_done", False, 0, 0, -1))
    for h2, l2, e2 in att_done:
        att_grp = [h2, l2, 1, e2] if att_grp is None else [att_grp[0], l2, att_grp[2] + 1, e2]
    if att_grp is not None:
        ops.append(("att_wgrads", True, att_grp[0], att_grp[1], att_grp[3]))
    return tuple(out), tuple(ops)


def test_backward_schedule_equals_the_inline_loop_it_replaced():
    for case in GRID:
        sched = backward_schedule(*case)
        got = tuple((hi, lo, tuple(tuple(op) for op in ops)) for hi, lo, ops in sched.chunks), tuple(tuple(op) for op in sched.tail)
        assert got == inline_loop_restated(*case), case


def _tiles_descending(ranges, T):
    """contiguous, descending, [0, T) exactly once"""
    edge = T
    for hi, lo in ranges:
        if hi != edge or not lo < hi:
            return False
        edge = lo
    return edge == 0


def test_backward_schedule_invariants():
    for case in GRID:
        T, CH, WG, n_deferred, stash, ramp = case
        sched = backward_schedule(*case)
        chunks = [(hi, lo) for hi, lo, _ in sched.chunks]
        assert chunks == chunk_ranges(T, CH, ramp, descending=True), case
        # (position, op): position ci = behind chunk ci's side-stream event, i.e. in front of chunk ci's main-stream step;
        # len(chunks) = the tail, behind every main-stream step
        flat = [(ci, op) for ci, (_, _, ops) in enumerate(sched.chunks) for op in ops] + [(len(chunks), op) for op in sched.tail]
        of = lambda kind: [(op.hi, op.lo) for _, op in flat if op.kind == kind]
        index_of_hi = {hi: ci for ci, (hi, _) in enumerate(chunks)}
        assert _tiles_descending(of("dec_wgrads"), T), case
        assert _tiles_descending(of("att_wgrads"), T), case
        if stash:
            assert _tiles_descending(of("att_acc"), T), case
            assert of("att_acc") == chunks, case           # one launch per chunk
        else:
            assert of("att_acc") == [], case
        for pos, op in flat:
            if op.kind in ("att_acc", "att_wgrads"):
                assert 0 <= op.k < pos, case               # chunk k's main-stream step is enqueued before the operation
                assert chunks[op.k][1] == op.lo, case      # ... and k is the newest (lowest) chunk the range covers
                assert index_of_hi[op.hi] <= op.k, case   # ... of whole chunks, none later than k
            else:
                assert op.k == -1, case
            if op.kind == "dec_wgrads":                    # its own stream's output: the chunks up to this one
                assert op.lo >= (chunks[pos][1] if pos < len(chunks) else 0), case
        deferred = [pos for pos, op in flat if op.kind == "deferred"]
        assert len(deferred) == n_deferred and all(pos >= 4 for pos in deferred if pos < len(chunks)), case
        kinds = [op.kind for op in sched.tail]
        assert kinds.count("acc_done") == 1 and all(op.kind != "acc_done" for _, _, ops in sched.chunks for op in ops), case
        assert "att_acc" not in kinds[kinds.index("acc_done"):], case
        gemms = ("dec_wgrads", "deferred", "att_wgrads")
        assert all(op.share == (op.kind in gemms) for _, _, ops in sched.chunks for op in ops), case      # the loop: all inside
        assert all(op.share == (op.kind in gemms and op.kind != "deferred") for op in sched.tail), case     # the tail's deferred: outside


def test_backward_schedule_at_the_judged_shape():
    sched = backward_schedule(872, 64, 4, 6, True)
    assert len(sched.chunks) == 17 and sched.chunks[0][:2] == (872, 864)
    every = [op for _, _, ops in sched.chunks for op in ops] + list(sched.tail)
    of = lambda kind: [(op.hi, op.lo) for op in every if op.kind == kind]
    assert of("dec_wgrads") == [(872, 808), (808, 576), (576, 320), (320, 64), (64, 0)]
    assert of("att_wgrads") == [(872, 808), (808, 576), (576, 320), (320, 0)]     # the last group: what the loop left + the tail's two
    assert [op.kind for op in sched.tail] == ["att_acc", "dec_wgrads", "att_acc", "acc_done", "att_wgrads"]
    assert [op.share for op in sched.tail] == [False, True, False, False, True]      # GEMM operations only: both weight-gradient groups
    one = backward_schedule(1, 64, 4, 6, True)
    assert one.chunks == ((1, 0, ()),)
    assert [tuple(op) for op in one.tail] == [("deferred", False, 0, 0, -1)] * 6 + [
        ("dec_wgrads", True, 1, 0, -1), ("att_acc", False, 1, 0, 0), ("acc_done", False, 0, 0, -1), ("att_wgrads", True, 1, 0, 0)]


def test_forward_schedule():
    s = forward_schedule(872, 64, 32, 1024)
    assert [(c1 - c0, sk) for c0, c1, sk, _ in s] == [(64, 1)] * 12 + [(40, 1), (32, 1), (16, 2), (8, 4), (8, 4)]
    assert [cleared for *_, cleared in s] == [sk > 1 for _, _, sk, _ in s]
    assert not any(cleared for *_, cleared in forward_schedule(872, 64, 32, 1024, controls=True))
    assert [sk for _, _, sk, _ in forward_schedule(872, 64, 32, 1024, controls=True)] == [sk for _, _, sk, _ in s]
    assert all(sk == 1 and not cleared for _, _, sk, cleared in forward_schedule(872, 64, 32, 1024, splitk_small=False))
    for T, CH, ramp in itertools.product(TS, CHS, (True, False)):
        for B, D in ((32, 1024), (5, 64)):
            s = forward_schedule(T, CH, B, D, ramp)
            assert [(c0, c1) for c0, c1, _, _ in s] == chunk_ranges(T, CH, ramp)
            assert all(sk == chunk_splits(c1 - c0, B, D) for c0, c1, sk, _ in s)


@pytest.mark.parametrize("ramp", [True, False])
def test_chunk_ranges_tile_the_frames_both_ways(ramp):
    for T, CH in itertools.product(TS, CHS):
        asc = chunk_ranges(T, CH, ramp)
        assert [c1 - c0 for c0, c1 in asc] == _chunk_sizes(T, CH, ramp_at_end=ramp)
        assert asc[0][0] == 0 and asc[-1][1] == T and all(a[1] == b[0] for a, b in zip(asc, asc[1:]))
        assert chunk_ranges(T, CH, ramp, descending=True) == [(c1, c0) for c0, c1 in reversed(asc)]
