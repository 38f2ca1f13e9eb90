"""t2_stretch / analysis.time_stretch / analysis.pitch_shift on the GPU against tests/stretch_ref.py.

pos must be EQUAL on every frame: the search runs on integers whose int32 sums are exact (|q| <= 1023, N <= 2048), so the kernel and
numpy see the same scores and the same ties.  y = w0 * x0 + w1 * x1 is two float32 products and one sum, each within 2^-24 of its
result and every result at most peak in magnitude (w0 + w1 = 1 up to the table's rounding): 2^-22 * peak in all; the tests allow
2^-21 * peak against the float64 overlap-add.  The rows are NaN behind n[b] and in the padding up to ldx, so a read past n[b] shows in
pos or in y."""
import ctypes as C

import numpy as np
import pytest
import torch

import stretch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TEMPI = (500, 800, 1001, 1250, 2000)
SENTINEL = -7


def _noise(n, seed, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _device_rows(rows, extra=5, strided=False):
    """The device's copy of ragged rows: NaN behind every n[b] and in `extra` columns of padding, returned as the (B, n_max) view;
    with `strided` the rows are every second row of a buffer twice as tall, the others NaN."""
    n = [len(r) for r in rows]
    ld = max(max(n), 1)
    big = np.full((len(rows) * (2 if strided else 1), ld + extra), np.nan, np.float32)
    for b, r in enumerate(rows):
        big[b * (2 if strided else 1), :n[b]] = r
    t = torch.from_numpy(big).to(DEV)
    return (t[::2] if strided else t)[:, :ld], n


def _abi(wav, n_dev, n_max, P, Q, N, D, ldy=None, ldp=None):
    """One t2_stretch call through the C ABI.  (rc, y, pos, n_out) with y, pos, n_out prefilled with SENTINEL."""
    from tacotron2_amd import _lib
    from tacotron2_amd.stretch import hann_table
    B = wav.shape[0]
    top = R.cdiv(max(n_max, 0) * Q, max(P, 1))
    ldy = top + 3 if ldy is None else ldy
    ldp = R.cdiv(top, N // 2) + 1 + 2 if ldp is None else ldp
    y = torch.full((B, max(ldy, 1)), float(SENTINEL), dtype=torch.float32, device=DEV)
    pos = torch.full((B, max(ldp, 1)), SENTINEL, dtype=torch.int32, device=DEV)
    n_out = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    w = torch.from_numpy(hann_table(N)).to(DEV)
    a = _lib.make("T2Stretch", x=wav, ldx=wav.stride(0) if B > 1 else max(wav.shape[1], 1), n=n_dev, w=w, B=B, n_max=n_max, N=N, D=D,
                  P=P, Q=Q, y=y, ldy=ldy, pos=pos, ldp=ldp, n_out=n_out)
    rc = _lib.lib().t2_stretch(C.addressof(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, y.cpu().numpy(), pos.cpu().numpy(), n_out.cpu().numpy()


_REF = {}


def _ref(key, x, P, Q, N, D):
    """The reference of one row, computed once per (key, P, Q, N, D) and shared."""
    k = (key, P, Q, N, D)
    if k not in _REF:
        _REF[k] = R.stretch(x, P, Q, N, D)
    return _REF[k]


def check(rows, keys, P, N, D, Q=1000, strided=False):
    wav, n = _device_rows(rows, strided=strided)
    n_dev = torch.tensor(n, dtype=torch.int32, device=DEV)
    rc, y, pos, n_out = _abi(wav, n_dev, max(n), P, Q, N, D)
    assert rc == 0
    for b, x in enumerate(rows):
        want_y, want_pos = _ref(keys[b], x, P, Q, N, D)
        M = len(want_pos)
        assert n_out[b] == len(want_y) == R.cdiv(n[b] * Q, P)
        assert np.array_equal(pos[b, :M], want_pos), (b, n[b], P, np.nonzero(pos[b, :M] != want_pos)[0][:5])      # EVERY frame
        assert not pos[b, M:].any()
        got = y[b, :n_out[b]].astype(np.float64)
        assert not np.isnan(y[b]).any()
        peak = float(np.abs(x).max()) if len(x) else 0.0
        assert np.abs(got - want_y).max(initial=0.0) <= 2.0 ** -21 * peak, (b, n[b], P, np.abs(got - want_y).max())
        assert not y[b, n_out[b]:].view(np.uint32).any()                       # exactly +0.0 behind n_out up to ldy
    return y, pos, n_out


@pytest.mark.parametrize("P", TEMPI)
def test_smallest_window_and_edge_lengths(P):
    sizes = (0, 1, 7, 8, 17, 997)
    check([_noise(n, 100 + n) for n in sizes], [("noise", n) for n in sizes], P, 16, 4)


@pytest.fixture(scope="module")
def voiced():
    return R.tone(140.0, 22050, 1.0, seed=3)


@pytest.mark.parametrize("P", TEMPI)
def test_default_window_ragged_and_strided(voiced, P):
    sizes = (1023, 5000, 22050)
    check([voiced[:n] for n in sizes], [("voiced", n) for n in sizes], P, 1024, 256, strided=True)


@pytest.mark.parametrize("D", [0, 600])
def test_largest_window(voiced, D):
    for P in TEMPI:
        y, pos, _ = check([voiced[:9000], -voiced[500:7001]], [("voiced", 9000), ("voiced-", 6501)], P, 2048, D)
        if D == 0:                                                             # no search: every frame at its nominal centre
            M = R.lengths(9000, P, 1000, 2048)[1]
            assert np.array_equal(pos[0, :M], R.centres(M, P, 1000, 2048))


def test_full_scale_square_wave_meets_the_int32_bound():
    x = np.where((np.arange(3 * 2048) // 64) % 2 == 0, 1.0, -1.0).astype(np.float32)
    check([x], [("square", len(x))], 1000, 2048, 128, Q=999)


@pytest.mark.parametrize("N,D", [(64, 16), (1024, 256)])
def test_silent_constant_and_impulse_rows(N, D):
    n = 6 * N + 13
    impulse = np.zeros(n, np.float32)
    impulse[n // 2] = -0.7
    rows = [np.zeros(n, np.float32), np.full(n, 0.25, np.float32), impulse]
    for P in (800, 1250):
        y, pos, _ = check(rows, [("zero", n), ("const", n), ("impulse", n)], P, N, D)
        M = R.lengths(n, P, 1000, N)[1]
        assert np.array_equal(pos[0, :M], R.centres(M, P, 1000, N))           # silence: delta = 0 throughout


def test_two_calls_are_bit_identical_and_rows_do_not_depend_on_the_batch(voiced):
    rows = [voiced[:5000], _noise(3001, 9), voiced[2000:9000]]
    wav, n = _device_rows(rows)
    n_dev = torch.tensor(n, dtype=torch.int32, device=DEV)
    first = _abi(wav, n_dev, max(n), 800, 1000, 1024, 256)
    again = _abi(wav, n_dev, max(n), 800, 1000, 1024, 256)
    for a, b in zip(first[1:], again[1:]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    one, n1 = _device_rows(rows[1:2], extra=11)
    alone = _abi(one, n_dev[1:2].contiguous(), n1[0], 800, 1000, 1024, 256)
    k = alone[3][0]
    assert k == first[3][1] and np.array_equal(alone[1][0, :k].view(np.uint32), first[1][1, :k].view(np.uint32))
    M = R.lengths(n1[0], 800, 1000, 1024)[1]
    assert np.array_equal(alone[2][0, :M], first[2][1, :M])


def test_python_layer_matches_the_abi_and_tempo_one_is_the_input(voiced, monkeypatch):
    from tacotron2_amd import analysis, stretch
    rows = [voiced[:5000], voiced[100:3100]]
    wav, n = _device_rows(rows, strided=True)
    y, n_out, pos = analysis.time_stretch(wav, n, 0.8)
    assert n_out == [6250, 3750] and y.shape[1] % 64 == 0 and pos.dtype == torch.int32
    _, y2, pos2, _ = _abi(wav, torch.tensor(n, dtype=torch.int32, device=DEV), max(n), 800, 1000, 1024, 256)
    for b in range(2):
        assert np.array_equal(y[b, :n_out[b]].cpu().numpy().view(np.uint32), y2[b, :n_out[b]].view(np.uint32))
        assert not y[b, n_out[b]:].any()
        M = R.lengths(n[b], 800, 1000, 1024)[1]
        assert np.array_equal(pos[b, :M].cpu().numpy(), pos2[b, :M])
    y3, n3, _ = analysis.time_stretch(wav, torch.tensor(n, device=DEV), (4, 5))           # device counts, a (P, Q) pair
    assert n3 == n_out and torch.equal(y3[:, :max(n3)], y[:, :max(n3)])
    with pytest.raises(ValueError, match="refused on the device"):
        analysis.time_stretch(wav, torch.tensor([5001, 3], device=DEV), 0.8)
    y0, n0, pos0 = analysis.time_stretch(torch.zeros(1, 0, device=DEV), [0], 0.8)          # (a batch without a column)
    assert n0 == [0] and y0.shape == (1, 0) and pos0.tolist() == [[0]]
    monkeypatch.setattr(stretch, "call", lambda *a: pytest.fail("tempo 1 must launch nothing"))
    for tempo in (1, 1.0, 1.0004, (7, 7)):
        same, n_same, none = analysis.time_stretch(wav, n, tempo)
        assert same is wav and n_same == n and none is None


def test_pitch_shift_is_stretch_then_resample(voiced):
    from tacotron2_amd import analysis
    from tacotron2_amd.stretch import pitch_plan
    rows = [voiced[:6000], voiced[300:4300]]
    wav, n = _device_rows(rows)
    for semitones, tempo in ((3, 1.0), (-5, 1.25)):
        y, n_out, eff, sr_mid = analysis.pitch_shift(wav, n, semitones, 22050, tempo)
        plan = pitch_plan("pitch_shift", semitones, 22050, tempo)
        assert (sr_mid, eff) == plan[:2] and abs(eff - tempo) <= 1e-3 * tempo
        s, ns, _ = analysis.time_stretch(wav, n, plan[2])
        want, nw = analysis.resample(s, ns, sr_mid, 22050)
        assert n_out == nw and torch.equal(y, want) and not torch.isnan(y).any()
        for b in range(2):
            assert abs(n_out[b] - n[b] / eff) <= 2e-3 * n[b] / eff + 1
    same, n_same, eff, sr_mid = analysis.pitch_shift(wav, n, 0, 22050)
    assert same is wav and n_same == n and eff == 1.0 and sr_mid == 22050


def test_a_count_out_of_range_is_refused_with_nothing_written():
    rows = [_noise(300, 1), _noise(200, 2), _noise(250, 3)]
    wav, n = _device_rows(rows)
    for bad in (301, -1, 2 ** 31 - 1):
        n_dev = torch.tensor([n[0], bad, n[2]], dtype=torch.int32, device=DEV)
        rc, y, pos, n_out = _abi(wav, n_dev, 300, 800, 1000, 16, 4)
        assert rc == 0 and n_out.tolist() == [375, -1, 313]
        assert (y[1] == SENTINEL).all() and (pos[1] == SENTINEL).all()        # nothing written for the refused row
        for b in (0, 2):
            want_y, want_pos = _ref(("noise-r", b), rows[b], 800, 1000, 16, 4)
            assert np.array_equal(pos[b, :len(want_pos)], want_pos) and np.abs(y[b, :n_out[b]] - want_y).max() <= 2.0 ** -21 * np.abs(rows[b]).max()


def test_rows_beside_a_refused_count_keep_their_bits():
    rows = [_noise(300, 1), _noise(200, 2), _noise(250, 3)]
    wav, n = _device_rows(rows)
    _, y0, pos0, n_out0 = _abi(wav, torch.tensor(n, dtype=torch.int32, device=DEV), 300, 800, 1000, 16, 4)
    for bad in (-1, 301):                                   # one below 0, one above n_max
        rc, y, pos, n_out = _abi(wav, torch.tensor([n[0], bad, n[2]], dtype=torch.int32, device=DEV), 300, 800, 1000, 16, 4)
        assert rc == 0 and n_out[1] == -1 and (y[1] == SENTINEL).all() and (pos[1] == SENTINEL).all()
        for b in (0, 2):
            assert n_out[b] == n_out0[b] and np.array_equal(pos[b], pos0[b]) and np.array_equal(y[b].view(np.uint32), y0[b].view(np.uint32))


def test_bad_operand_blocks_return_an_error_before_any_launch():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    wav, n = _device_rows([_noise(100, 1)])
    n_dev = torch.tensor(n, dtype=torch.int32, device=DEV)
    assert _abi(wav, n_dev, 100, 800, 1000, 16, 4)[0] == 0
    bad = [dict(N=2), dict(N=15), dict(N=2050), dict(D=-1), dict(D=1025), dict(P=0), dict(Q=0), dict(P=100, Q=1000), dict(P=9, Q=1),
           dict(P=(1 << 20) + 1, Q=1 << 20), dict(n_max=-1), dict(n_max=101), dict(ldy=124), dict(ldp=16)]
    for kw in bad:
        args = dict(wav=wav, n_dev=n_dev, n_max=100, P=800, Q=1000, N=16, D=4)
        args.update(kw)
        rc, y, pos, n_out = _abi(**args)
        assert rc == 1 and b"t2_stretch" in lib.t2_last_error(), kw
        assert (y == SENTINEL).all() and (pos == SENTINEL).all() and (n_out == SENTINEL).all(), kw
    assert _abi(wav, n_dev, 100, 800, 1000, 16, 4, ldy=125, ldp=17)[0] == 0               # the smallest that will do
