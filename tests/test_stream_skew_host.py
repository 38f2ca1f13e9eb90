"""tests/stream_skew.py itself, with a fake `call` and fake stream handles (no GPU), and the schedule-coverage claims that
tests/test_gpu_stream_skew.py rests on, asserted from engine.forward_schedule / engine.backward_schedule for every shape it uses."""
import pytest

import stream_skew as SK
from tacotron2_amd import _lib, engine as E

MAIN, SIDE, THIRD = 0, 0x5151, 0x7777


class FakeStream:
    def __init__(self, handle, log):
        self.cuda_stream, self.log = handle, log

    def record_event(self):
        self.log.append(("hip.record", self.cuda_stream))
        return ("event", self.cuda_stream)

    def wait_stream(self, other):
        self.log.append(("hip.wait", self.cuda_stream, other.cuda_stream))

    wait_event = wait_stream


class FakeEngine:
    dev = "cpu"

    def __init__(self, log):
        self.side = FakeStream(SIDE, log)

    def side_stream(self):
        return self.side


@pytest.fixture
def rig(monkeypatch):
    """(log, engine, main stream): `call` replaced by a fake that runs the PRE_CALL hooks like the real one and logs (name, stream)."""
    log = []

    def fake_call(name, *args):
        for hook in list(_lib.PRE_CALL):
            hook()
        log.append((name, args[-1]) if name != SK.PROBE else (name, args[-1], args[1], args[0]))
    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(E, "call", fake_call)
    monkeypatch.setattr(E._TLS, "pending", {}, raising=False)
    return log, FakeEngine(log), FakeStream(MAIN, log)


def install(monkeypatch, rig, policy, delay=700):
    log, eng, main = rig
    return SK.skew(monkeypatch, eng, policy, delay, main=MAIN, word=0x1000)


def pend(handle, ptr=0x4000):
    """One region on the zero list of stream `handle`, as engine.zero_later leaves it."""
    E._pending().setdefault(handle, []).append(((ptr, 64, 1, 64), None))


def test_both_names_are_patched_and_restored(monkeypatch, rig):
    with monkeypatch.context() as mp:
        before = (_lib.call, E.call, E.Engine._wait, E.Engine._record)
        SK.skew(mp, rig[1], SK.slow("side"), 100, main=MAIN, word=0)
        assert _lib.call is E.call and _lib.call is not before[0]
        assert E.Engine._wait is not before[2] and E.Engine._record is not before[3]
    assert (_lib.call, E.call, E.Engine._wait, E.Engine._record) == before


def test_slow_delays_one_stream_on_that_stream(monkeypatch, rig):
    log = rig[0]
    sk = install(monkeypatch, rig, SK.slow("side"))
    E.call("t2_a", 1, MAIN)
    E.call("t2_b", 2, SIDE)
    _lib.call("t2_c", 3, SIDE)
    assert log == [("t2_a", MAIN), (SK.PROBE, SIDE, 700, 0x1000 + 8), ("t2_b", SIDE), (SK.PROBE, SIDE, 700, 0x1000 + 8), ("t2_c", SIDE)]
    assert sk.trace == [(0, "main", "t2_a", False), (1, "side", "t2_b", True), (2, "side", "t2_c", True)]
    assert sk.counts() == {"main": (1, 0), "side": (2, 2)}
    log.clear()
    sk.policy = SK.slow("main")
    E.call("t2_a", 1, MAIN)
    E.call("t2_b", 2, SIDE)
    assert log == [(SK.PROBE, MAIN, 700, 0x1000), ("t2_a", MAIN), ("t2_b", SIDE)]


def test_the_probe_is_never_delayed_or_counted(monkeypatch, rig):
    log = rig[0]
    sk = install(monkeypatch, rig, lambda o, n, l: True)
    E.call(SK.PROBE, 0x2000, 3000, SIDE)                # the engine's own probe (stream_concurrency_check)
    assert log == [(SK.PROBE, SIDE, 3000, 0x2000)] and sk.trace == [] and sk.ordinal == 0
    E.call("t2_x", SIDE)
    assert [e[0] for e in log] == [SK.PROBE, SK.PROBE, "t2_x"] and sk.ordinal == 1


def test_unknown_stream_is_other(monkeypatch, rig):
    sk = install(monkeypatch, rig, SK.slow("side"))
    E.call("t2_x", 1, THIRD)
    E.call("t2_y", 1, None)
    E.call("t2_z", 1, "text")
    assert [e[1] for e in sk.trace] == ["other"] * 3 and not any(e[3] for e in sk.trace)
    assert SK.seeded(1, p=1.0)(0, "t2_x", "other") is False
    # a side stream that ensure_concurrent_streams replaced is followed
    rig[1].side = FakeStream(THIRD, rig[0])
    E.call("t2_x", 1, THIRD)
    assert sk.trace[-1][1:] == ("side", "t2_x", True)


def test_reentry_through_pre_call_keeps_flush_spin_call(monkeypatch, rig):
    """A pending zero list: the delayed call X comes out as [spin, zero] (the flush, delayed itself), [spin, X]; the hooks that the
    original `call` runs again find an empty list, so the re-entry ends."""
    log = rig[0]
    monkeypatch.setattr(_lib, "PRE_CALL", [E.flush_zeros])
    sk = install(monkeypatch, rig, SK.slow("side"))
    pend(SIDE)
    pend(MAIN)
    E.call("t2_x", 1, SIDE)
    assert [(e[0], e[1]) for e in log] == [(SK.PROBE, SIDE), ("t2_zero_regions", SIDE), ("t2_zero_regions", MAIN),
                                          (SK.PROBE, SIDE), ("t2_x", SIDE)]
    assert [(e[0], e[1], e[2], e[3]) for e in sk.trace] == [(0, "side", "t2_zero_regions", True), (1, "main", "t2_zero_regions", False),
                                                          (2, "side", "t2_x", True)]
    assert E._pending() == {}


def test_policies_are_pure_functions_of_seed_and_ordinal():
    a, b = SK.seeded(3), SK.seeded(3)
    fwd = [a(i, "n", "main") for i in range(400)]
    back = [b(i, "x", "side") for i in reversed(range(400))][::-1]        # asked in another order, other names and labels
    assert fwd == back and fwd == [a(i, "n", "side") for i in range(400)]
    assert fwd != [SK.seeded(4)(i, "n", "main") for i in range(400)]
    assert 60 <= sum(fwd) <= 140                                          # p = 0.25 of 400 (+- 4.6 sigma)
    assert sum(SK.seeded(3, p=0.0)(i, "n", "main") for i in range(100)) == 0
    assert all(SK.seeded(3, p=1.0)(i, "n", "main") for i in range(100))


def test_window_limits_by_ordinal(monkeypatch, rig):
    sk = install(monkeypatch, rig, SK.window(SK.slow("side"), 2, 4))
    for i in range(6):
        E.call("t2_x", i, SIDE if i != 3 else MAIN)
    assert [e[3] for e in sk.trace] == [False, False, True, False, False, False]
    w = SK.window(lambda o, n, l: True, 5, 7)
    assert [w(i, "n", "main") for i in range(4, 8)] == [False, True, True, False]


def test_edges_are_traced_and_unchanged(monkeypatch, rig):
    log, eng, main = rig
    monkeypatch.setattr(_lib, "PRE_CALL", [E.flush_zeros])
    sk = install(monkeypatch, rig, SK.slow("side"))
    pend(MAIN)
    ev = E.Engine._record(main)                     # flushes first, as before
    E.Engine._wait(eng.side, main)
    E.Engine._wait(main, eng.side)
    E.Engine._record(eng.side)
    E.Engine._wait(FakeStream(THIRD, log), main)
    assert ev == ("event", MAIN)
    assert log == [("t2_zero_regions", MAIN), ("hip.record", MAIN), ("hip.wait", SIDE, MAIN), ("hip.wait", MAIN, SIDE), ("hip.record", SIDE),
                   ("hip.wait", THIRD, MAIN)]
    assert sk.edges() == [("record", "main"), ("wait", "side", "stream"), ("wait", "main", "stream"), ("record", "side"),
                          ("wait", "other", "stream")]
    assert sk.edge_string() == "RsMr?" and sk.wait_ordinals() == [1, 2, 4]
    assert "before launch 1: record main" in sk.report()


def test_drop_wait_still_flushes(monkeypatch, rig):
    log, eng, main = rig
    monkeypatch.setattr(_lib, "PRE_CALL", [E.flush_zeros])
    sk = install(monkeypatch, rig, SK.slow("side"))
    st = SK.drop_wait(monkeypatch, 1)
    E.Engine._wait(eng.side, main)
    pend(SIDE)
    E.Engine._wait(main, eng.side)                  # the dropped one: the flush (delayed: side stream) but no wait
    E.Engine._wait(main, eng.side)
    assert log == [("hip.wait", SIDE, MAIN), (SK.PROBE, SIDE, 700, 0x1000 + 8), ("t2_zero_regions", SIDE), ("hip.wait", MAIN, SIDE)]
    assert st == dict(seen=3, dropped=[1]) and sk.dropped == [1]
    assert sk.edge_string() == "sMM"                # the dropped wait keeps its place in the pattern


def test_delay_is_held_to_the_probes_limit(monkeypatch, rig):
    assert SK.PROBE_MAX_US == 50000
    with pytest.raises(AssertionError):
        install(monkeypatch, rig, SK.slow("side"), delay=50001)
    with pytest.raises(AssertionError):
        install(monkeypatch, rig, SK.slow("side"), delay=0)


# ---- the schedules that tests/test_gpu_stream_skew.py runs: every kind of edge is reached ----------------------------------------
# (T in decoder steps, chunk, chunk_bwd, wgrad_group, batch): the base shape, the three shapes of the multi-step case (T = 9: odd),
# B = 35, and zoneout with r = 2 at T = 24 frames = 12 steps.  N_DEFERRED is read off the engine in the GPU test and asserted there.
GPU_SHAPES = [(12, 2, 2, 2, 5), (9, 2, 2, 2, 5), (12, 2, 2, 2, 35)]
N_DEFERRED = 6                                      # five postnet weight gradients and the projection's


def kinds_in_loop(s):
    return {op.kind for _, _, ops in s.chunks for op in ops}


@pytest.mark.parametrize("T,chunk,chunk_bwd,wg,B", GPU_SHAPES)
def test_schedules_of_the_gpu_cases_reach_every_kind_of_edge(T, chunk, chunk_bwd, wg, B):
    s = E.backward_schedule(T, chunk_bwd, wg, N_DEFERRED, True)
    assert kinds_in_loop(s) == {"dec_wgrads", "deferred", "att_acc", "att_wgrads"}
    assert len(s.chunks) >= 5
    tail = [op.kind for op in s.tail]
    assert tail[-3:] == ["att_acc", "acc_done", "att_wgrads"] and tail[0] == "att_acc" and "deferred" in tail
    f = E.forward_schedule(T, chunk, B, 64)
    assert len(f) == len(s.chunks) and all(sk > 1 and cleared for _, _, sk, cleared in f)
    assert not any(cleared for _, _, _, cleared in E.forward_schedule(T, chunk, B, 64, controls=True))   # the cterm copy instead


def test_base_schedule_is_the_one_the_sensitivity_ordinals_were_read_from():
    s = E.backward_schedule(12, 2, 2, N_DEFERRED, True)
    assert len(s.chunks) == 6
    assert [[op.kind for op in ops] for _, _, ops in s.chunks] == [
        [], ["dec_wgrads"], ["att_acc"], ["dec_wgrads", "att_acc", "att_wgrads"], ["deferred", "att_acc"],
        ["dec_wgrads", "deferred", "att_acc", "att_wgrads"]]
    assert [op.kind for op in s.tail] == ["att_acc"] + ["deferred"] * 4 + ["att_acc", "acc_done", "att_wgrads"]
    assert [(c0, c1) for c0, c1, _, _ in E.forward_schedule(12, 2, 5, 64)] == [(i, i + 2) for i in range(0, 12, 2)]
