"""Host side of the guard-band mode (tacotron2_amd/guard.py: Engine.guard_bytes, ParamStore(guard_bytes=...)), the persistent
launches' counter ring, and the shape / device checks in front of the loss kernel - all on CPU tensors, nothing is launched."""
import pytest
import torch

from oracle import tacotron2_ref as R
from tacotron2_amd import engine as E
from tacotron2_amd import guard
from tacotron2_amd.params import ParamStore
from tests.helpers import SMALL

CPU = torch.device("cpu")


@pytest.fixture
def no_zero_list(monkeypatch):
    """zero_later records regions for a device launch (current HIP stream): on the CPU they are only collected here."""
    regions = []
    monkeypatch.setattr(E, "zero_later", lambda t: regions.append(t) or t)
    return regions


def _engine(guard_bytes, ps_guard=0):
    eng = E.Engine(ParamStore(R.default_dims(**SMALL), CPU, guard_bytes=ps_guard))
    eng.guard_bytes = guard_bytes
    return eng


@pytest.mark.parametrize("dtype,bits", [(torch.float32, 0x7FC5A5A5), (torch.float64, 0x7FF8A5A5A5A5A5A5), (torch.int32, 0),
                                        (torch.int64, 0)])
def test_guard_bands_sit_on_both_sides_of_an_exact_size_aligned_view(dtype, bits):
    eng = _engine(4096)
    v = eng.buf("x", 7, 3, dtype=dtype)
    backing, g, n, short = eng._guards["x"]
    es = v.element_size()
    assert v.shape == (7, 3) and n == 21 and short == 0 and g * es == 4096 and backing.numel() == 21 + 2 * g
    assert v.data_ptr() - backing.data_ptr() == 4096                      # the view starts right behind the before-band ...
    assert (v.data_ptr() - backing.data_ptr()) % 512 == 0                  # ... at the allocator's alignment
    w = guard._words(backing)
    assert bool((w[:g] == bits).all()) and bool((w[g + n:] == bits).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(backing[:g]).all()) and bool(torch.isnan(backing[g + n:]).all())
    assert eng.guard_check() == []


def test_guard_bytes_must_keep_the_alignment():
    eng = _engine(1000)
    with pytest.raises(AssertionError, match="multiple of 512"):
        eng.buf("x", 4)


def test_guarded_workspace_is_reallocated_when_count_or_dtype_change():
    eng = _engine(512)
    a = eng.buf("x", 10)
    assert eng.buf("x", 2, 5).data_ptr() == a.data_ptr()                   # same count: the same allocation
    b = eng.buf("x", 6)                                                    # smaller: a new one, its band right behind 6
    assert eng._guards["x"][2] == 6 and b.data_ptr() != a.data_ptr()
    c = eng.buf("x", 12)
    assert eng._guards["x"][2] == 12 and eng._guards["x"][0].numel() == 12 + 2 * 128
    d = eng.buf("x", 12, dtype=torch.int32)
    assert d.dtype == torch.int32 and eng._guards["x"][0].dtype == torch.int32 and c.data_ptr() != d.data_ptr()


def test_unguarded_workspaces_keep_the_product_rule():
    eng = _engine(0)
    assert eng.buf("x", 0).numel() == 0 and eng._ws["x"].numel() == 1     # max(n, 1) elements
    a = eng.buf("x", 10)
    b = eng.buf("x", 5)
    assert eng._ws["x"].numel() == 10 and b.data_ptr() == a.data_ptr()   # a larger earlier tensor is reused
    assert eng.buf("x", 3, dtype=torch.float64).dtype == torch.float64 and eng._ws["x"].numel() == 3
    assert eng._guards == {} and eng.guard_check() == []
    o = eng.out("mels", 2, 3)
    assert o.shape == (2, 3) and o.untyped_storage().nbytes() == 24 and "out.mels" not in eng._guards


@pytest.mark.parametrize("side,where", [("after", 0), ("after", 37), ("before", -1), ("before", -128)])
def test_a_band_write_is_reported_with_name_side_and_offset(side, where):
    eng = _engine(512)
    v = eng.buf("ws.proj", 4, 5)
    backing, g, n, _ = eng._guards["ws.proj"]
    off = n + where if side == "after" else where                          # offset from the view's first element
    backing[g + off] = 1.5
    hits = eng.guard_check()
    assert len(hits) == 1 and hits[0][:4] == ("ws.proj", side, off, 1) and hits[0][4][0] == 1.5
    v.fill_(3.0)                                                           # writes inside the view are not band hits
    assert len(eng.guard_check()) == 1
    with pytest.raises(E._lib.T2Error, match=f"ws.proj {side}"):
        eng.check_persistent_kernels()


def test_integer_band_write_is_reported():
    eng = _engine(512)
    eng.buf("inf0.done", 5, dtype=torch.int32)
    backing, g, n, _ = eng._guards["inf0.done"]
    backing[g + n + 3] = 7
    assert eng.guard_check() == [("inf0.done", "after", n + 3, 1, [7, 0, 0, 0])]


def test_short_after_band_hook_checks_the_end_of_the_view():
    eng = _engine(512)
    eng._guard_short["proj"] = 6
    v = eng.buf("proj", 3, 2, 3)                   # 18 elements, the last 6 are checked as band
    assert eng.guard_check() == []
    v[-1].fill_(0.25)                              # the last "frame" written: 6 elements
    assert eng.guard_check() == [("proj", "after", 12, 6, [0.25] * 4)]


def test_prezero_then_buf_of_another_size_asserts_in_guard_mode(no_zero_list):
    eng = _engine(512)
    eng.prezero("post.conv0.dwp", 4, 10)
    assert eng.buf("post.conv0.dwp", 4, 10, zero=True).shape == (4, 10)     # the same size: a plain lookup
    eng.prezero("post.conv1.dwp", 4, 10)
    with pytest.raises(AssertionError, match="prezero"):
        eng.buf("post.conv1.dwp", 4, 11, zero=True)


# ---- marks of regions cleared ahead (Engine.clear_ahead / need_zero) ---------------------------------------------------------------
def _region(t):
    return t.data_ptr(), t.numel() * t.element_size()


def test_buf_of_another_size_after_prezero_is_cleared_in_product_mode(no_zero_list):
    eng = _engine(0)
    eng.prezero("x", 4, 10)
    no_zero_list.clear()
    v = eng.buf("x", 4, 11, zero=True)             # a new, larger allocation: the mark is for another region
    assert len(no_zero_list) == 1 and _region(no_zero_list[0]) == _region(v) and v.shape == (4, 11)


def test_a_mark_does_not_outlive_begin_phase(no_zero_list):
    eng = _engine(0)
    eng.prezero("y", 4, 10)
    eng.begin_phase(backward=True)                 # (the phase that set the mark was abandoned)
    no_zero_list.clear()
    v = eng.buf("y", 4, 10, zero=True)
    assert len(no_zero_list) == 1 and _region(no_zero_list[0]) == _region(v)


def test_a_fill_gemm_mark_stays_with_its_engine_and_its_phase(no_zero_list, monkeypatch):
    gemms = []
    monkeypatch.setattr(E, "gemm", lambda *a, **k: gemms.append(k))
    eng, other = _engine(0), _engine(0)
    C = torch.empty(128, 128)
    assert E.fill_splits(128, 128, 1024)
    eng.fill_ahead(C, 128, 128, 1024, 128)         # the encoder's prologue: clear now and remember
    assert len(no_zero_list) == 1 and eng._cleared
    for e in (eng, other):
        e.begin_phase(backward=False)
        no_zero_list.clear()
        e.gemm_fill(None, None, C, 128, 128, 1024, 1024, 1024, 128)
        assert len(no_zero_list) == 1 and _region(no_zero_list[0]) == _region(C)
        assert gemms[-1]["accumulate"] == 2 and gemms[-1]["splitk"] == 2
    # within one phase of one engine the consumer finds the mark, once
    eng.fill_ahead(C, 128, 128, 1024, 128)
    no_zero_list.clear()
    eng.gemm_fill(None, None, C, 128, 128, 1024, 1024, 1024, 128)
    assert no_zero_list == [] and not eng._cleared
    eng.gemm_fill(None, None, C, 128, 128, 1024, 1024, 1024, 128)
    assert len(no_zero_list) == 1


def test_a_mark_is_consumed_once(no_zero_list):
    eng = _engine(0)
    eng.prezero("z", 4, 10)
    no_zero_list.clear()
    eng.buf("z", 4, 10, zero=True)
    assert no_zero_list == []                      # the first user finds the region cleared ahead ...
    v = eng.buf("z", 4, 10, zero=True)
    assert len(no_zero_list) == 1 and _region(no_zero_list[0]) == _region(v)     # ... the second one in the phase clears it


def test_share_cu_request_is_restored_when_the_body_raises(monkeypatch):
    seen = []
    monkeypatch.setattr(E, "make", lambda name, **kw: seen.append(kw["share_cu"]))
    monkeypatch.setattr(E, "call", lambda *a: None)
    monkeypatch.setattr(E, "_stream", lambda: 0)
    g = lambda: E.gemm(None, None, None, 1, 1, 1, 1, 1, 1)
    g()
    with pytest.raises(RuntimeError, match="boom"):
        with E.share_cu(1):
            g()
            with E.share_cu(0):
                g()
            g()
            raise RuntimeError("boom")
    g()
    assert seen == [0, 1, 0, 1, 0]


def test_guarded_outputs_are_fresh_and_checked():
    eng = _engine(512)
    a = eng.out("mels", 2, 3)
    z = eng.out("align", 2, 4, zero=True)
    assert a.shape == (2, 3) and bool((z == 0).all())
    b = eng.out("mels", 2, 3)
    assert b.data_ptr() != a.data_ptr()                                   # the caller keeps its tensor
    backing, g, n, _ = eng._guards["out.mels"]
    backing[g - 1] = 0.0
    assert [h[:4] for h in eng.guard_check()] == [("out.mels", "before", -1, 1)]


def test_paramstore_bands_leave_the_views_and_offsets_alone():
    d = R.default_dims(**SMALL)
    ps0 = ParamStore(d, CPU, guard_bytes=0)
    ps = ParamStore(d, CPU, guard_bytes=1024)
    assert ps.offsets == ps0.offsets and ps.numel == ps0.numel and ps.flat.numel() == ps0.flat.numel()
    ps.init_adam()
    for name in ("flat", "grad", "exp_avg", "exp_avg_sq", "buf_flat"):
        backing, g, n = ps._guards[name]
        view = getattr(ps, name)
        assert g == 256 and view.data_ptr() - backing.data_ptr() == 1024 and view.numel() == n
        assert bool((guard._words(backing[:g]) == 0x7FC5A5A5).all()) and bool((guard._words(backing[g + n:]) == 0x7FC5A5A5).all())
    for k in ps.P:
        assert ps.P[k].data_ptr() - ps.flat.data_ptr() == ps0.P[k].data_ptr() - ps0.flat.data_ptr()
        assert ps.G[k].data_ptr() - ps.grad.data_ptr() == 4 * ps.offsets[k]
    assert float(ps.flat.abs().sum()) == 0.0 and float(ps.buf_flat.sum()) == float(ps0.buf_flat.sum())
    assert ps.guard_check() == []
    ps._guards["grad"][0][ps._guards["grad"][1] + ps.numel] = 0.0        # one element past the gradient buffer
    eng = E.Engine(ps)
    assert [h[:4] for h in eng.guard_check()] == [("ps.grad", "after", ps.numel, 1)]
    with pytest.raises(E._lib.T2Error, match="ps.grad"):
        eng.check_persistent_kernels()


# ---- the persistent launches' counter ring -----------------------------------------------------------------------------------
def test_counter_ring_starts_over_instead_of_running_out(no_zero_list):
    """Engine.persist_counters hands out blocks of the ring in order; a phase (or a caller without one - model/submodules.py) that
    needs more than the ring holds starts it over, and the ring is put on the zero list again in front of that launch."""
    eng = _engine(0)
    ring = eng.persist_sync()
    base = ring.data_ptr() + 4 * eng.PERSIST_RING0
    eng.begin_phase(backward=False)
    no_zero_list.clear()
    addrs = [eng.persist_counters(2) for _ in range(eng.PERSIST_RING // 2)]
    assert addrs == [base + 4 * 256 * 2 * i for i in range(eng.PERSIST_RING // 2)] and no_zero_list == []
    assert eng.persist_counters(2) == base                                 # the 49th launch of two blocks: start over ...
    assert len(no_zero_list) == 1 and no_zero_list[0].data_ptr() == base  # ... behind a clear of the whole ring
    assert no_zero_list[0].numel() == 256 * eng.PERSIST_RING
    # without any phase (the Encoder sub-module): 120 launches, never an assertion, every block cleared since its last use
    eng2 = _engine(0)
    used = {}
    for i in range(120):
        before = len(no_zero_list)
        a = eng2.persist_counters(1)
        if len(no_zero_list) > before:
            used.clear()
        assert a not in used
        used[a] = i
    assert int(ring[256]) == 0


# ---- loss inputs ---------------------------------------------------------------------------------------------------------------
def _loss_inputs(B=3, T=5, M=4, dev=CPU):
    g = torch.Generator().manual_seed(0)
    mel = torch.randn(B, T, M, generator=g).to(dev)
    return dict(mel=mel, post=mel + 0.1, gate=torch.randn(B, T, 1, generator=g).to(dev), mel_tgt=mel * 0.5,
                gate_tgt=torch.ones(B, T, 1).to(dev), mel_len=torch.tensor([5, 3, 1][:B], dtype=torch.int32).to(dev))


def _kernel_must_not_run(*a, **k):
    raise AssertionError("the loss kernel was reached with invalid inputs")


@pytest.mark.parametrize("bad", ["mel_tgt_T", "mel_tgt_M", "mel_tgt_B", "gate_tgt", "mel_len_short", "mel_len_long"])
def test_loss_rejects_mismatched_targets_before_the_kernel(monkeypatch, bad):
    from tacotron2_amd.model import tts_model
    monkeypatch.setattr(tts_model, "call", _kernel_must_not_run)
    x = _loss_inputs()
    B, T, M = x["mel"].shape
    if bad == "mel_tgt_T":
        x["mel_tgt"] = torch.zeros(B, T + 1, M)            # longer target: would be read with the wrong stride
    elif bad == "mel_tgt_M":
        x["mel_tgt"] = torch.zeros(B, T, M - 1)
    elif bad == "mel_tgt_B":
        x["mel_tgt"] = torch.zeros(B - 1, T, M)            # shorter: read past its end
    elif bad == "gate_tgt":
        x["gate_tgt"] = torch.zeros(B, T - 1, 1)
    elif bad == "mel_len_short":
        x["mel_len"] = x["mel_len"][:2]
    else:
        x["mel_len"] = torch.tensor([5, 3, 1, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="loss"):
        tts_model._LossTermsFn.apply(x["mel"], x["post"], x["gate"], x["mel_tgt"], x["gate_tgt"], x["mel_len"])
