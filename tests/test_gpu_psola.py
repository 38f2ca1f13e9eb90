"""t2_psola / analysis.psola / pitch_ratio / pitch_shift_psola on the GPU against tests/psola_ref.py.

a, r, kmap, n_marks and n_syn must be EQUAL: the analysis chain compares input floats and everything else is integer arithmetic, so
the kernel and numpy place every mark on the same sample, ties included.  y = (sum_j w_j x_j) / max(sum_j w_j, 1) over at most G
grains is G float32 products, 2 (G - 1) sums and one division, each within 2^-24 of its result, and no partial result exceeds G * peak:
the tests allow 4 (G + 2) * 2^-24 * peak against the float64 overlap-add, G being the largest number of grains over one sample that the
reference met in that row.  The rows are NaN behind n[b] and in the padding up to ldx, so a read past n[b] shows in the marks or in y."""
import ctypes as C

import numpy as np
import pytest
import torch

import psola_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7
HOP = 256
Q = {0.25: 16384, 0.5: 32768, 0.794: 52016, 1.335: 87491, 2: 131072, 4: 262144}


def _voice(n, period=100, seed=0):
    """A synthetic vowel with a little noise on it, so that no two samples of a search window are equal by construction."""
    x = R.vowel(period, 1000.0, 200.0, n=max(n, 1))[:n]
    return (x + 1e-4 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _frames(n, extra=0):
    return 1 + n // HOP + extra


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


def _tracks(lags, rhos, T):
    """(lag, rho) int32 (B, T) on the device from per-row arrays (a scalar fills the row); -1 behind a row's own frames."""
    lag, rho = np.full((len(lags), T), -1, np.int32), np.full((len(lags), T), -1, np.int32)
    for b, (l, q) in enumerate(zip(lags, rhos)):
        l = np.asarray(l, np.int32)
        lag[b, :len(l)] = l
        rho[b, :len(l)] = q
    return torch.from_numpy(lag).to(DEV), torch.from_numpy(rho).to(DEV)


def _abi(wav, n_dev, n_max, lag, rho, hop=HOP, U=None, ldy=None, ldm=None, lds=None, T=None):
    """One t2_psola call through the C ABI.  (rc, dict of numpy outputs), every output prefilled with SENTINEL."""
    from tacotron2_amd import _lib
    from tacotron2_amd.psola import grain_table
    B = wav.shape[0]
    ldy = n_max + 3 if ldy is None else ldy
    ldm = max(n_max, 0) // 12 + 2 + 2 if ldm is None else ldm
    lds = max(n_max, 0) // 3 + 10256 + 2 if lds is None else lds
    y = torch.full((B, max(ldy, 1)), float(SENTINEL), dtype=torch.float32, device=DEV)
    a = torch.full((B, max(ldm, 1)), SENTINEL, dtype=torch.int32, device=DEV)
    r, kmap = (torch.full((B, max(lds, 1)), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    n_marks, n_syn = (torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    w = torch.from_numpy(grain_table()).to(DEV)
    s = _lib.make("T2Psola", x=wav, ldx=wav.stride(0) if B > 1 else max(wav.shape[1], 1), n=n_dev, lag=lag, rho=rho, ldt=lag.shape[1], w=w,
                  B=B, n_max=n_max, T=lag.shape[1] if T is None else T, hop=hop, U=hop // 2 if U is None else U, y=y, ldy=ldy, a=a, ldm=ldm,
                  r=r, kmap=kmap, lds=lds, n_marks=n_marks, n_syn=n_syn)
    rc = _lib.lib().t2_psola(C.addressof(s), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in dict(y=y, a=a, r=r, kmap=kmap, n_marks=n_marks, n_syn=n_syn).items()}


def _row_ok(out, b, x, lag, rho, hop=HOP, U=None):
    """Row b of `out` against the reference of (x, lag, rho); returns the reference."""
    n = len(x)
    want, a, r, km, G = R.psola(x, lag, rho, hop, U)
    K1, J1 = len(a), len(r)
    assert (out["n_marks"][b], out["n_syn"][b]) == (K1, J1), (b, n, out["n_marks"][b], out["n_syn"][b], K1, J1)
    assert np.array_equal(out["a"][b, :K1], a), (b, n, np.nonzero(out["a"][b, :K1] != a)[0][:5])               # EVERY mark
    assert np.array_equal(out["r"][b, :J1], r), (b, n, np.nonzero(out["r"][b, :J1] != r)[0][:5])
    assert np.array_equal(out["kmap"][b, :J1], km)
    assert not out["a"][b, K1:].any() and not out["r"][b, J1:].any() and not out["kmap"][b, J1:].any()
    y = out["y"][b]
    assert not np.isnan(y).any()
    peak = float(np.abs(x).max()) if n else 0.0
    err = np.abs(y[:n].astype(np.float64) - want).max(initial=0.0)
    print(f"row {b}: n {n}, marks {K1}, grains {J1}, G {G}, error {err / max(peak, 1e-30) / 2.0 ** -24:.2f} * 2^-24 * peak, allowed {4 * (G + 2)}")
    assert err <= 4 * (G + 2) * 2.0 ** -24 * peak, (b, n, G, err, peak)
    assert not y[n:].view(np.uint32).any()                                 # exactly +0.0 behind n up to ldy
    return want, a, r, km, G


def check(rows, lags, rhos, U=None, strided=False, extra_frames=0):
    wav, n = _device_rows(rows, strided=strided)
    lag, rho = _tracks(lags, rhos, _frames(max(n), extra_frames))
    rc, out = _abi(wav, torch.tensor(n, dtype=torch.int32, device=DEV), max(n), lag, rho, U=U)
    assert rc == 0
    return out, [_row_ok(out, b, x, lag[b].cpu().numpy(), rho[b].cpu().numpy(), U=U) for b, x in enumerate(rows)]


@pytest.fixture(scope="module")
def voiced():
    return _voice(12000)


def test_identity(voiced):
    _, ((want, a, r, km, G),) = check([voiced], [np.full(_frames(12000), 100)], [R.ONE])
    assert np.array_equal(a, r) and G == 2
    assert np.abs(want - voiced).max() <= 4 * 2.0 ** -24 * np.abs(voiced).max()


@pytest.mark.parametrize("ratio", sorted(Q))
def test_constant_ratios(voiced, ratio):
    check([voiced[:9000]], [np.full(_frames(9000), 100)], [Q[ratio]])


def test_ratio_ramp_and_a_length_that_is_no_multiple_of_the_hop(voiced):
    n = 11111
    T = _frames(n)
    check([voiced[:n]], [np.full(T, 100)], [np.linspace(0.5 * R.ONE, 2.0 * R.ONE, T).astype(np.int32)])
    check([voiced[:n]], [np.full(T, 100)], [Q[0.794]], extra_frames=3)               # (frames behind the row's own are not read)


def test_unvoiced_gaps_at_the_start_in_the_middle_and_at_the_end(voiced):
    n = 10000
    lag = np.full(_frames(n), 100)
    lag[:5], lag[17:23], lag[-6:] = 0, 0, 0
    for q, U in ((Q[0.794], None), (Q[1.335], 100), (Q[0.5], 16)):
        check([voiced[:n]], [lag], [q], U=U)


def test_rows_of_0_1_and_about_U_samples(voiced):
    U = HOP // 2
    sizes = (0, 1, U - 1, U, U + 1)
    for l0 in (0, 100):
        check([voiced[:n] for n in sizes], [np.full(_frames(n), l0) for n in sizes], [Q[0.794]] * len(sizes))


def test_adjacent_frames_of_lags_44_and_367_and_unvoiced_to_367():
    x = _voice(9000, period=147, seed=2)
    T = _frames(9000)
    alt = np.where(np.arange(T) % 2 == 0, 44, 367)
    uv = np.where(np.arange(T) % 2 == 0, 0, 367)
    for q in (R.ONE, Q[0.5], Q[2]):
        check([x, x], [alt, uv], [q, q])


def test_plateau_and_all_zero_rows_take_the_first_of_equal_maxima():
    n = 4000
    plateau = np.zeros(n, np.float32)
    plateau[500:3000] = 0.5
    _, refs = check([np.zeros(n, np.float32), plateau], [np.full(_frames(n), 80)] * 2, [Q[0.794]] * 2)
    a = refs[0][1]
    assert np.array_equal(a[:-1], 60 * np.arange(len(a) - 1)) and a[-1] == n           # 0, 60, 120, ...: c - d on every mark


def test_a_row_longer_than_a_staged_piece_with_more_marks_than_threads():
    n = 40000
    x = _voice(n, period=33, seed=5)
    lag = 30 + (np.arange(_frames(n)) % 7)
    _, ((_, a, r, _, _),) = check([x], [lag], [Q[0.794]])
    assert len(a) > 1024 and len(r) > 1024


def test_a_mixed_batch_as_a_strided_view_reads_nothing_behind_a_row(voiced):
    rows = [voiced[:7001], voiced[300:1500], voiced[1000:11500]]
    lags = [np.full(_frames(len(r)), l) for r, l in zip(rows, (100, 101, 99))]
    check(rows, lags, [Q[0.794], Q[2], Q[0.5]], strided=True)


def test_refused_rows_keep_their_prefill_and_the_others_are_right(voiced):
    rows = [voiced[:3000], voiced[:2500], voiced[:2800], voiced[:2000]]
    wav, n = _device_rows(rows)
    T = _frames(3000)
    lags = [np.full(_frames(k), 100) for k in n]
    lags[2] = lags[2].copy()
    lags[2][4] = 5                                                         # a lag of 5
    rhos = [Q[0.794], Q[0.794], Q[0.794], 1000]                            # a rho of 1000
    lag, rho = _tracks(lags, rhos, T)
    n_dev = torch.tensor([n[0], 3001, n[2], n[3]], dtype=torch.int32, device=DEV)          # a count past n_max
    rc, out = _abi(wav, n_dev, 3000, lag, rho)
    assert rc == 0 and out["n_marks"].tolist()[1:] == [-1, -1, -1]
    for b in (1, 2, 3):
        assert all((out[k][b] == SENTINEL).all() for k in ("y", "a", "r", "kmap")) and out["n_syn"][b] == SENTINEL
    _row_ok(out, 0, rows[0], lag[0].cpu().numpy(), rho[0].cpu().numpy())
    lag[3, 2] = 0                                                          # an unvoiced frame's rho is not looked at ...
    rho2 = rho.clone()
    rho2[3, :] = R.ONE
    rho2[3, 2] = 1000
    rc, out = _abi(wav, torch.tensor(n, dtype=torch.int32, device=DEV), 3000, lag, rho2)
    assert rc == 0 and out["n_marks"][3] > 0 and out["n_marks"][2] == -1
    _row_ok(out, 3, rows[3], lag[3].cpu().numpy(), rho2[3].cpu().numpy())


def test_rows_beside_a_refused_count_keep_their_bits(voiced):
    rows = [voiced[:3000], voiced[:2500], voiced[:2800]]
    wav, n = _device_rows(rows)
    lag, rho = _tracks([np.full(_frames(k), 100) for k in n], [Q[0.794]] * 3, _frames(3000))
    _, good = _abi(wav, torch.tensor(n, dtype=torch.int32, device=DEV), 3000, lag, rho)
    for bad in (-1, 3001):                                  # one below 0, one above n_max
        rc, out = _abi(wav, torch.tensor([n[0], bad, n[2]], dtype=torch.int32, device=DEV), 3000, lag, rho)
        assert rc == 0 and out["n_marks"][1] == -1 and out["n_syn"][1] == SENTINEL
        assert all((out[k][1] == SENTINEL).all() for k in ("y", "a", "r", "kmap"))
        for b in (0, 2):
            for k in out:
                assert out[k][b].tobytes() == good[k][b].tobytes(), (bad, b, k)


def test_two_calls_are_bit_identical_and_rows_do_not_depend_on_the_batch(voiced):
    rows = [voiced[:5000], voiced[200:3201]]
    wav, n = _device_rows(rows)
    lag, rho = _tracks([np.full(_frames(k), 100) for k in n], [Q[0.794], Q[1.335]], _frames(5000))
    n_dev = torch.tensor(n, dtype=torch.int32, device=DEV)
    first, again = _abi(wav, n_dev, 5000, lag, rho)[1], _abi(wav, n_dev, 5000, lag, rho)[1]
    for k in first:
        assert np.array_equal(first[k].view(np.uint32) if first[k].dtype == np.float32 else first[k],
                              again[k].view(np.uint32) if again[k].dtype == np.float32 else again[k]), k
    one, n1 = _device_rows(rows[1:2], extra=11)
    alone = _abi(one, n_dev[1:2].contiguous(), n1[0], lag[1:2, :_frames(n1[0])].contiguous(), rho[1:2, :_frames(n1[0])].contiguous())[1]
    assert np.array_equal(alone["y"][0, :n1[0]].view(np.uint32), first["y"][1, :n1[0]].view(np.uint32))
    J1 = alone["n_syn"][0]
    assert J1 == first["n_syn"][1] and np.array_equal(alone["r"][0, :J1], first["r"][1, :J1])


def test_python_layer_matches_the_abi(voiced):
    from tacotron2_amd import analysis
    rows = [voiced[:5000], voiced[100:3100]]
    wav, n = _device_rows(rows, strided=True)
    T = _frames(5000)
    lag, rho = _tracks([np.full(T, 100), np.full(T, 101)], [Q[0.794], Q[0.794]], T)
    y, marks = analysis.psola(wav, n, lag, Q[0.794])
    assert y.shape[1] % 64 == 0 and marks["a"].dtype == torch.int32 and marks["n_marks"].min() > 0
    _, out = _abi(wav, torch.tensor(n, dtype=torch.int32, device=DEV), max(n), lag, rho)
    for b in range(2):
        assert np.array_equal(y[b, :n[b]].cpu().numpy().view(np.uint32), out["y"][b, :n[b]].view(np.uint32)) and not y[b, n[b]:].any()
        K1, J1 = int(marks["n_marks"][b]), int(marks["n_syn"][b])
        assert (K1, J1) == (out["n_marks"][b], out["n_syn"][b])
        assert np.array_equal(marks["a"][b, :K1].cpu().numpy(), out["a"][b, :K1])
        assert np.array_equal(marks["r"][b, :J1].cpu().numpy(), out["r"][b, :J1])
    y2, marks2 = analysis.psola(wav, torch.tensor(n, device=DEV), lag, rho)                 # device counts, a tensor rho
    assert torch.equal(y2[:, :max(n)], y[:, :max(n)]) and torch.equal(marks2["n_syn"], marks["n_syn"])
    _, bad = analysis.psola(wav, torch.tensor([5001, 3], device=DEV), lag, rho)
    assert bad["n_marks"].tolist()[0] == -1 and bad["n_marks"].tolist()[1] > 0


def test_pitch_ratio_on_the_device():
    from tacotron2_amd import analysis
    rng = np.random.default_rng(4)
    lag = rng.integers(44, 367, size=(3, 40)).astype(np.int32)
    lag[0, 5:9], lag[2, :] = 0, 0
    n = [39 * HOP, 20 * HOP + 7, 30 * HOP]
    dev = torch.from_numpy(lag).to(DEV)
    for st, k in ((0.0, 0.0), (3.0, 0.5), (-7.0, 2.0), (12.0, 1.5)):
        got = analysis.pitch_ratio(dev, n, st, k, HOP).cpu().numpy()
        for b in range(3):
            assert np.abs(got[b] - R.pitch_ratio(lag[b], n[b], st, k, HOP)).max() <= 1, (st, k, b)
    for st in (4.0, -12.0, 0.0):
        got = analysis.pitch_ratio(dev, torch.tensor(n, device=DEV), st, 1.0, HOP).cpu().numpy()
        for b in range(3):
            assert np.array_equal(got[b], R.pitch_ratio(lag[b], n[b], st, 1.0, HOP))


@pytest.fixture(scope="module")
def shifted():
    """pitch_shift_psola of a 1 s steady vowel of lag 100 at +4 semitones: (x, wav, y, n_out, eff)."""
    from tacotron2_amd import analysis
    x = R.vowel(100, 1000.0, 200.0, n=22050)
    wav = torch.from_numpy(x).to(DEV)[None, :]
    return (x, wav) + tuple(analysis.pitch_shift_psola(wav, [22050], 4.0, 22050))


def test_pitch_shift_psola_keeps_the_formant_and_the_sample_count(shifted, monkeypatch):
    from tacotron2_amd import analysis, psola
    x, wav, y, n_out, eff = shifted
    n = len(x)
    assert n_out == [n] and eff == 1.0 and y.shape[1] >= n and not torch.isnan(y).any()
    out = y[0, :n].cpu().numpy()
    f0, width = R.fundamental(out[1000:21000])
    print("fundamental of the output:", f0, "Hz, wanted", 22050 / (100 * Q[0.794] / R.ONE))
    assert abs(f0 - 22050 / (100 * Q[0.794] / R.ONE)) <= width
    c0, c1 = R.centroid(x), R.centroid(out)
    c2 = R.centroid(R.resampled(R.vowel(100, 1000.0, 200.0, n=int(n / 0.7937) + 200), 0.7937))
    print("centroid: input", c0, "psola", c1, "resampled", c2, "share", abs(c1 - c0) / abs(c2 - c0))
    assert abs(c1 - c0) <= 0.25 * abs(c2 - c0)
    # no shift and an unchanged range: nothing of the PSOLA path is launched, the argument comes back
    monkeypatch.setattr(psola, "call", lambda *a: pytest.fail("semitones 0 with pitch_range 1 must launch nothing"))
    monkeypatch.setattr(analysis, "call", lambda *a: pytest.fail("semitones 0 with pitch_range 1 must track nothing"))
    same, n_same, eff = analysis.pitch_shift_psola(wav, [n], 0.0, 22050, 1.0)
    assert same is wav and n_same == [n] and eff == 1.0
    with pytest.raises(ValueError, match="T2_PROSODY_MAX_T"):
        analysis.pitch_shift_psola(torch.zeros(1, 4096 * 256, device=DEV), [4096 * 256], 2.0, 22050)


def test_pitch_shift_psola_output_lag_read_by_the_same_tracker(shifted):
    """The median voiced lag of the output is round(100 * 0.7937) = 79 +- 1, one lag being the tracker's resolution, when it is read
    as pitch_shift_psola read its input: psola.track_lags, the smoothed meter's yin and pitch_viterbi with fold_lags behind them.
    The meter's own decode does not read it so, nor the input: measured on an MI355X, pitch_viterbi alone gives the steady input vowel
    the lag 200 and the output 159, and tests/pitch_ref.py in float32 gives 200 and 238.  Its local cost is yin's normalised
    difference alone, which on a steady voice is as small at every multiple of the period (float64 reference output: 0.0112 at lag 79,
    0.0097 at 159, 0.0027 at 238; the true period is 79.37 and the marks are whole samples), and nothing in it prefers the shorter
    lag.  Marks two periods apart shifted the vowel to 138 Hz, not 278 Hz; fold_lags is what was added against that."""
    from tacotron2_amd import analysis, psola
    from tacotron2_amd.prosody import ProsodyMeter
    x, wav, y, n_out, eff = shifted
    n = len(x)
    meter = ProsodyMeter(22050, DEV, smooth=True)
    nd = torch.tensor([n], device=DEV)
    lag_in = psola.track_lags(meter, wav, nd, n)[0].cpu().numpy()
    lag = psola.track_lags(meter, y, nd, n)[0].cpu().numpy()
    s = meter.settings
    _, _, power, cmnd = analysis.yin(y, nd, n_max=n, return_cmnd=True, **s)
    raw = analysis.pitch_viterbi(cmnd, power, nd, sr=22050, hop=s["hop"], fmin=s["fmin"], fmax=s["fmax"], power_floor=s["power_floor"],
                                 **meter.viterbi)[2]
    assert np.array_equal(lag, R.fold_lags(cmnd[0].cpu().numpy(), raw[0].cpu().numpy(), meter.tau_min, s["thr"]))     # the fold, to the lag
    med, med_in = int(np.median(lag[lag > 0])), int(np.median(lag_in[lag_in > 0]))
    print("median voiced lag: input", med_in, "output", med, "voiced frames", int((lag > 0).sum()), "pitch_viterbi alone on the output",
          int(np.median(raw[0].cpu().numpy()[raw[0].cpu().numpy() > 0])))
    assert med_in == 100 and (lag > 0).sum() > 40 and abs(med - round(100 * 0.7937)) <= 1


def test_fold_lags_matches_the_reference():
    from tacotron2_amd import analysis
    rng = np.random.default_rng(0)
    cm = rng.uniform(0.0, 0.4, size=(3, 50, 368)).astype(np.float32)
    cm[:, :, 100], cm[1, :, 50], cm[2, :, 99] = 0.05, 0.05, 0.05
    cm[2, :, 101] = cm[2, :, 99]                                           # equal minima: the first one
    lag = rng.integers(44, 367, size=(3, 50)).astype(np.int32)
    lag[0, :10], lag[:, 20:30], lag[:, 30:40] = 0, 200, 300
    got = analysis.fold_lags(torch.from_numpy(cm).to(DEV), torch.from_numpy(lag).to(DEV), 44, 0.1).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, np.stack([R.fold_lags(cm[b], lag[b], 44, 0.1) for b in range(3)]))
    assert (got[0, :10] == 0).all() and (got[:, 20:40] <= 101).all()


def test_bad_operand_blocks_return_an_error_before_any_launch(voiced):
    from tacotron2_amd import _lib
    lib = _lib.lib()
    wav, n = _device_rows([voiced[:1200]])
    n_dev = torch.tensor(n, dtype=torch.int32, device=DEV)
    lag, rho = _tracks([np.full(_frames(1200), 100)], [R.ONE], _frames(1200))
    assert _abi(wav, n_dev, 1200, lag, rho)[0] == 0
    for kw in (dict(hop=15), dict(U=15), dict(U=4097), dict(n_max=-1), dict(n_max=1201), dict(ldy=1199), dict(ldm=101), dict(lds=10655),
               dict(T=0), dict(T=_frames(1200) + 1)):
        args = dict(wav=wav, n_dev=n_dev, n_max=1200, lag=lag, rho=rho)
        args.update(kw)
        rc, out = _abi(**args)
        assert rc == 1 and b"t2_psola" in lib.t2_last_error(), kw
        assert all((v == SENTINEL).all() for v in out.values()), kw
    assert _abi(wav, n_dev, 1200, lag, rho, ldy=1200, ldm=102, lds=10656)[0] == 0         # the smallest that will do
