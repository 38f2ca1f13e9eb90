"""Deterministic stream skew for the engine's two-stream schedules ("Stream skew").

Engine.forward_tf / backward_tf order their two HIP streams with hand-placed Engine._record / Engine._wait edges.  At the shapes the
suite can afford, every kernel finishes in microseconds and a missing edge almost never shows.  skew() makes ONE stream arbitrarily
slow instead: in front of the library calls a policy selects, an idle wave (t2_stream_probe_spin) holds the call's own stream for
`delay_us`.  The other stream then runs as far ahead as the declared edges allow, and a missing or misplaced edge is a stale or
premature read on every run, which the caller's comparison with its float64 reference sees.

What it orders is LAUNCHES: the harness knows nothing about byte ranges, and torch operations on a stream (copy_, fill_) are not
library calls - they are not delayed, but stay ordered behind the delayed kernels of their stream.  Product code is not touched:
everything is a monkeypatch of tacotron2_amd._lib.call / tacotron2_amd.engine.call (engine imports `call` by name) and of the two
edge helpers, which only gain a trace entry.

Imported like the other helpers of this directory (`import stream_skew`); tests/test_stream_skew_host.py drives it with a fake
`call` and fake stream handles, tests/test_gpu_stream_skew.py on the device."""
import random

PROBE = "t2_stream_probe_spin"
PROBE_MAX_US = 50000           # the probe's limit (include/tacotron2_amd.h)


# ---- policies: (ordinal, name, label) -> delay this launch? ----------------------------------------------------------------------
def slow(which):
    """Every launch on the stream labelled `which` ("main" | "side")."""
    assert which in ("main", "side")
    return lambda ordinal, name, label: label == which


def seeded(seed, p=0.25):
    """Each launch on either engine stream with probability p: launch `ordinal` takes the ordinal-th draw of random.Random(seed), so a
    decision is a pure function of (seed, ordinal) - not of the order in which the policy is asked."""
    rng, draws = random.Random(seed), []

    def policy(ordinal, name, label):
        while len(draws) <= ordinal:
            draws.append(rng.random())
        return label in ("main", "side") and draws[ordinal] < p
    return policy


def window(policy, lo, hi):
    """`policy` restricted to the launches with ordinals in [lo, hi): narrows a failing case by hand."""
    return lambda ordinal, name, label: lo <= ordinal < hi and policy(ordinal, name, label)


# ---- the harness ---------------------------------------------------------------------------------------------------------------
class Skew:
    """State of one skew() installation.  trace: launches (ordinal, label, name, delayed) and edges ("record", label) /
    ("wait", waiting label, "event" | "stream"), in host order."""

    def __init__(self, engine, policy, delay_us, main, word):
        self.engine, self.policy, self.delay_us, self.main, self.word = engine, policy, int(delay_us), main, word
        self.trace = []
        self.dropped = []          # indices (into edges()) of waits that drop_wait skipped
        self.ordinal = 0

    def label(self, handle):
        if isinstance(handle, bool) or not isinstance(handle, int):
            return "other"
        if handle == self.main:
            return "main"
        return "side" if handle == self.engine.side_stream().cuda_stream else "other"

    def launches(self, label=None):
        return [e for e in self.trace if len(e) == 4 and (label is None or e[1] == label)]

    def edges(self):
        return [e for e in self.trace if e[0] in ("record", "wait")]

    def counts(self):
        out = {}
        for _, label, _, delayed in self.launches():
            n, k = out.get(label, (0, 0))
            out[label] = (n + 1, k + int(bool(delayed)))
        return out                 # label -> (launches, delayed launches)

    def edge_string(self):
        """One letter per edge: r / R a record on the side / main stream; waits: e / s the SIDE stream waits for an event / for the
        other stream, E / M the MAIN stream does; ? anything on another stream."""
        out = []
        for e in self.edges():
            if e[1] not in ("main", "side"):
                out.append("?")
            elif e[0] == "record":
                out.append("R" if e[1] == "main" else "r")
            else:
                c = "e" if e[2] == "event" else ("m" if e[1] == "main" else "s")
                out.append(c.upper() if e[1] == "main" else c)
        return "".join(out)

    def wait_ordinals(self):
        """Positions in edge_string() of the waits, in order: wait_ordinals()[n] is the n of drop_wait(monkeypatch, n)."""
        return [i for i, e in enumerate(self.edges()) if e[0] == "wait"]

    def report(self):
        lines = [f"stream skew: delay {self.delay_us} us; launches per stream (all, delayed): {self.counts()}",
                 f"edges: {self.edge_string()}  (dropped waits at {self.dropped})"]
        pos = 0
        for e in self.trace:       # every edge with the launch ordinal it stands in front of
            if len(e) == 4:
                pos = e[0] + 1
            else:
                lines.append(f"  before launch {pos}: {' '.join(str(x) for x in e)}")
        return "\n".join(lines)


def skew(monkeypatch, engine, policy, delay_us, main=None, word=None):
    """Install the skew for `engine` until monkeypatch undoes it; returns the Skew (its trace fills as the engine runs).
    main: handle of the main stream - torch's current stream NOW (inside the engine's `with torch.cuda.stream(side)` blocks the
    current stream is the side stream, so it is resolved once, here); the side stream is engine.side_stream() at every call
    (ensure_concurrent_streams may replace it).  word: where the idle wave leaves its poll count, an int32 tensor of the harness's
    own on the engine's device (8 words; one per label, so spins on both streams never share one)."""
    from tacotron2_amd import _lib, engine as E
    assert 0 < int(delay_us) <= PROBE_MAX_US, f"delay {delay_us} us: the probe takes 1..{PROBE_MAX_US}"
    if main is None or word is None:
        import torch
        main = torch.cuda.current_stream().cuda_stream if main is None else main
        word = torch.zeros(8, dtype=torch.int32, device=engine.dev) if word is None else word
    sk = Skew(engine, policy, delay_us, main, word)
    orig = _lib.call
    slot = {"main": 0, "side": 2, "other": 4}

    def call(name, *args):
        if name == PROBE:                              # never delayed, never counted: the harness's own launches, and the engine's
            return orig(name, *args)
        # what `orig` does first, done here so that the trace is in launch order: the hooks (flush_zeros) come back through
        # engine.call - this wrapper - and their t2_zero_regions launches are delayed like any other.  They empty the zero list
        # before they launch, so the re-entry ends: the hooks that `orig` runs again below find nothing
        for hook in list(_lib.PRE_CALL):
            hook()
        handle = args[-1] if args else None
        label = sk.label(handle)
        ordinal, sk.ordinal = sk.ordinal, sk.ordinal + 1
        delayed = bool(sk.policy(ordinal, name, label))
        sk.trace.append((ordinal, label, name, delayed))
        if delayed:
            w = sk.word
            orig(PROBE, (w.data_ptr() if hasattr(w, "data_ptr") else w) + 4 * slot[label], sk.delay_us, handle)
        return orig(name, *args)

    rec0, wait0 = E.Engine._record, E.Engine._wait

    # (the edge helpers flush the zero list first; done here already, so that an edge's entry stands behind that flush's launches)
    def _record(stream):
        E.flush_zeros()
        sk.trace.append(("record", sk.label(stream.cuda_stream)))
        return rec0(stream)

    def log_wait(stream, other):
        import torch
        sk.trace.append(("wait", sk.label(stream.cuda_stream), "event" if isinstance(other, torch.cuda.Event) else "stream"))

    def _wait(stream, other):
        E.flush_zeros()
        log_wait(stream, other)
        return wait0(stream, other)
    _wait.log = log_wait
    _wait.skew = sk
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(E, "call", call)
    monkeypatch.setattr(E.Engine, "_record", staticmethod(_record))
    monkeypatch.setattr(E.Engine, "_wait", staticmethod(_wait))
    return sk


def drop_wait(monkeypatch, n):
    """Sensitivity check only: the n-th Engine._wait from now on (0-based) still flushes the zero list but skips the stream wait.
    Install it behind skew(): the dropped wait then keeps its trace entry and is listed in Skew.dropped.
    Returns {"seen": waits so far, "dropped": [n] once it happened}."""
    from tacotron2_amd import engine as E
    prev = E.Engine._wait
    state = dict(seen=0, dropped=[])

    def _wait(stream, other):
        i, state["seen"] = state["seen"], state["seen"] + 1
        if i != n:
            return prev(stream, other)
        sk = getattr(prev, "skew", None)
        E.flush_zeros()
        if sk is not None:                             # (`prev` is not called, so its trace entry is made here)
            prev.log(stream, other)
            sk.dropped.append(len(sk.edges()) - 1)
        state["dropped"].append(i)
    monkeypatch.setattr(E.Engine, "_wait", staticmethod(_wait))
    return state
