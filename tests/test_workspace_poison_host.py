"""Host side of tests/workspace_poison.py on a CPU-device engine (as tests/test_guard_host.py): nothing is launched."""
import pytest
import torch

import workspace_poison as WP
from oracle import tacotron2_ref as R
from tacotron2_amd import engine as E
from tacotron2_amd.params import ParamStore
from tests.helpers import SMALL

CPU = torch.device("cpu")


def _engine(guard_bytes=0):
    eng = E.Engine(ParamStore(R.default_dims(**SMALL), CPU, guard_bytes=0))
    eng.guard_bytes = guard_bytes
    return eng


def test_poison_values_are_finite_with_finite_squares_and_differ():
    f32 = torch.tensor([WP.P_POS, WP.Q_NEG], dtype=torch.float32)
    assert bool(torch.isfinite(f32 * f32).all()) and WP.P_POS > 0 > WP.Q_NEG and abs(WP.P_POS) != abs(WP.Q_NEG)
    assert 5e3 <= float(f32.abs().min()) and float(f32.abs().max()) <= 2e4
    eng = _engine()
    eng.buf("x", 4)
    for bad in (float("nan"), float("inf"), 1e30):
        with pytest.raises(AssertionError, match="finite"):
            WP.poison(eng, bad)


def test_floats_are_filled_to_the_end_of_the_backing_tensor_and_integers_stay_bit_identical():
    eng = _engine()
    f = eng.buf("xdec", 3, 5).fill_(0.25)
    h = eng.buf("bn.sums", 4, dtype=torch.float64).fill_(1.0)
    i32 = eng.buf("inf0.win_peak", 2, 3, dtype=torch.int32).copy_(torch.arange(6, dtype=torch.int32).view(2, 3))
    i64 = eng.buf("inf.lengths", 3, dtype=torch.int64).copy_(torch.tensor([7, -1, 2 ** 40]))
    u8 = eng.buf("dur.back", 5, dtype=torch.uint8).fill_(200)
    before = {k: eng._ws[k].clone() for k in ("inf0.win_peak", "inf.lengths", "dur.back")}
    poisoned, skipped = WP.poison(eng, WP.P_POS)
    assert poisoned == ["xdec", "bn.sums"] and skipped == ["inf0.win_peak", "inf.lengths", "dur.back"]
    assert bool((eng._ws["xdec"] == WP.P_POS).all()) and bool((f == WP.P_POS).all())
    assert h.dtype == torch.float64 and bool((eng._ws["bn.sums"] == WP.P_POS).all())
    for k, t in before.items():
        assert eng._ws[k].dtype == t.dtype and torch.equal(eng._ws[k], t), k
    assert i32[1, 2] == 5 and i64[2] == 2 ** 40 and u8[0] == 200


def test_a_smaller_view_of_a_larger_tensor_is_poisoned_over_the_larger_tensor():
    eng = _engine()
    big = eng.buf("cum", 4, 10).zero_()
    small = eng.buf("cum", 2, 3)                       # Engine.buf: t[:n] of the larger earlier tensor
    assert small.data_ptr() == big.data_ptr() and eng._ws["cum"].numel() == 40
    WP.poison(eng, WP.Q_NEG)
    assert bool((big == WP.Q_NEG).all()) and bool((eng._ws["cum"] == WP.Q_NEG).all())
    assert eng._ws["cum"].untyped_storage().nbytes() == 160      # the entry is the whole allocation: nothing lies behind it


def test_guard_bands_survive_the_poison():
    eng = _engine(512)
    v = eng.buf("proj", 3, 7)
    WP.poison(eng, WP.P_POS)
    assert bool((v == WP.P_POS).all()) and eng.guard_check() == []


def test_the_skip_list_is_honoured_and_capped():
    assert len(WP.SKIP) <= WP.MAX_SKIP == 5
    WP.check_skip_list(WP.SKIP)
    eng = _engine()
    a, b = eng.buf("some.table", 4).zero_(), eng.buf("other", 4).zero_()
    poisoned, skipped = WP.poison(eng, WP.P_POS, skip={"some.table": "csrc/x.hip:1: index"})
    assert poisoned == ["other"] and skipped == ["some.table"] and float(a.abs().max()) == 0.0 and bool((b == WP.P_POS).all())
    with pytest.raises(AssertionError, match="at most 5"):
        WP.poison(eng, WP.P_POS, skip={f"t{i}": "f.hip:1: x" for i in range(6)})
    for never in ("xdec", "dgd_t", "enc.conv1.dwp", "post.conv4.dwp", "dpmT", "bn.sums", "pack.att", "pack.enc.whh0", "proj", "mel_tm"):
        with pytest.raises(AssertionError, match="never"):
            WP.poison(eng, WP.P_POS, skip={never: "f.hip:1: x"})
    with pytest.raises(AssertionError, match="file and line"):
        WP.poison(eng, WP.P_POS, skip={"some.table": "because"})
    assert float(a.abs().max()) == 0.0                  # a refused list poisons nothing


def test_persist_sync_is_untouched():
    eng = _engine()
    ring = eng.persist_sync()
    ring[3], ring[256], ring[eng.PERSIST_RING0 + 5] = 11, 1, 7
    before = ring.clone()
    eng.buf("enc.ht", 8)
    poisoned, skipped = WP.poison(eng, WP.P_POS)
    assert poisoned == ["enc.ht"] and skipped == []
    assert eng._persist_sync is ring and torch.equal(ring, before)
    assert all(t.data_ptr() != ring.data_ptr() for t in eng._ws.values())


def test_dirty_allocator_fills_and_frees():
    ptrs = WP.dirty_allocator(CPU, [1, 512, 4096], WP.P_POS)
    assert len(ptrs) == 3 and all(p % 4 == 0 for p in ptrs)
    with pytest.raises(AssertionError):
        WP.dirty_allocator(CPU, [16], float("nan"))


def test_skip_clear_leaves_one_named_float_region_uncleared(monkeypatch):
    regions = []
    monkeypatch.setattr(E, "zero_later", lambda t: regions.append(t.data_ptr()) or t)
    eng = _engine()
    skipped = WP.skip_clear(monkeypatch, E.Engine, "dpmT")
    d = eng.buf("dpmT", 2, 3, zero=True)
    o = eng.buf("dv_part", 2, 3, zero=True)
    assert regions == [o.data_ptr()] and skipped == [(d.data_ptr(), 24)]
    # a region cleared ahead (the split-K blocks of pre_dec): neither half of the pair clears it, and no mark is left behind
    WP.skip_clear(monkeypatch, E.Engine, "pre_dec")
    pre = eng.buf("pre_dec", 4, 6)
    eng.clear_ahead(pre[1:3])
    eng.need_zero(pre[1:3])
    assert regions == [o.data_ptr()] and not eng._cleared
    with pytest.raises(AssertionError):
        WP.skip_clear(monkeypatch, E.Engine, "inf0.done")        # never a counter, a flag or an integer buffer
