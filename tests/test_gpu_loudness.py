"""t2_loudness / analysis.loudness / analysis.normalize_loudness on the GPU against tests/loudness_ref.py.

Every case draws its inputs with a fixed seed and asserts IN THE REFERENCE, before the device is touched, that every block is further
than 1e-6 LU from both gates: the hop energies are fp64 sums of at most H squares of a filter output that itself carries rounding of
the order of 2^-53 per step, about 4 H 2^-53 times the filter's gain or 1e-11 relative, so no order of summation can move a block
across a gate and n_blocks, n_below_abs, n_below_rel and flags must be EQUAL; E is held to 1e-9 relative and the loudness to 1e-8 dB.
The true peak is t2_resample's arithmetic and must have the bits of max |engine.resample(x, n, sr, 4 sr)|; against the float64
reference it is 32 float32 taps at 2^-24 each, 1e-5 relative.  The gain - one rounding to float32 of an fp64 value - is held to one
float32 ulp of the reference's, which bounds a limited gain with that float32 true peak; y is x * gain in numpy float32 from the
device's own gain, bit for bit.  The rows are NaN behind n[b] and in the padding up to ldx."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 8000
H, N = 800, 3200
STAT = ("lufs", "gain", "true_peak", "sample_peak", "n_blocks", "n_below_abs", "n_below_rel", "rel_gate_lufs", "momentary_max_lufs", "flags")


def _voice(seed, n, amp, sr=SR):
    """n samples of a 180 Hz tone with four harmonics under a slow swell, plus a little noise: float32, RMS about amp."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = sum(np.sin(2 * np.pi * 180.0 * k * t + k) / k for k in range(1, 5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.9 * t + 1.0))
    return (amp * (x / 0.8 + 0.05 * rng.standard_normal(n))).astype(np.float32)


def _pad(rows, n_max=None):
    n = [len(r) for r in rows]
    x = np.zeros((len(rows), max(max(n), 1) if n_max is None else n_max), np.float32)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


def _poison(x, n, extra=5):
    """The device's copy: NaN behind every n[b] and in `extra` columns of padding; returned as the (B, n_max) view of it."""
    big = np.full((x.shape[0], x.shape[1] + extra), np.nan, np.float32)
    for b in range(len(n)):
        big[b, :n[b]] = x[b, :n[b]]
    return torch.from_numpy(big).to(DEV)[:, :x.shape[1]]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _raw(wav, n, sr, target=-23.0, ceiling=-1.0, max_gain_db=30.0, write=True, lde=None):
    """The C entry itself, with E in reach: dict(E, stat, gain, y) as numpy arrays."""
    from tacotron2_amd import _lib, loudness
    from tacotron2_amd.datasets.resample import plan
    B, ld = wav.shape
    b1, a1, b2, a2 = loudness.k_weighting(sr)
    hop = loudness.hop(sr)
    _, _, K, table = plan(sr, 4 * sr)
    lde = max(ld // hop, 1) if lde is None else lde
    E = torch.full((B, lde), float("nan"), dtype=torch.float64, device=DEV)
    stat = torch.full((B, 10), float("nan"), dtype=torch.float64, device=DEV)
    gain = torch.full((B,), float("nan"), device=DEV)
    y = torch.full((B, ld), float("nan"), device=DEV) if write else None
    a = _lib.make("T2Loudness", x=wav, ldx=wav.stride(0) if B > 1 else max(ld, 1), n=torch.as_tensor(n, dtype=torch.int32).to(DEV),
                  table=torch.from_numpy(table).to(DEV), K=K, B=B, n_max=ld, H=hop, b1=b1, a1=a1, b2=b2, a2=a2, abs_gate=R.ABS_GATE,
                  target=target, max_gain=10.0 ** (max_gain_db / 20.0), ceiling=10.0 ** (ceiling / 20.0), E=E, lde=lde, stat=stat,
                  gain=gain, y=y, ldy=ld)
    _lib.call("t2_loudness", a, _lib.stream())
    torch.cuda.synchronize()
    return dict(E=E.cpu().numpy(), stat=stat.cpu().numpy(), gain=gain.cpu().numpy(), y=None if y is None else y.cpu().numpy())


def _resample_peak(wav, n, sr):
    """max |engine.resample(x, n, sr, 4 sr)| over each row's first 4 n outputs: float32."""
    from tacotron2_amd import engine
    if max(n) == 0:
        return np.zeros(len(n), np.float32)
    out, n_out = engine.resample(wav, n, sr, 4 * sr)
    assert n_out == [4 * v for v in n]
    out = out.cpu().numpy()
    return np.array([np.abs(out[b, :4 * n[b]]).max() if n[b] else 0.0 for b in range(len(n))], np.float32)


def check(rows, sr=SR, target=-23.0, ceiling=-1.0, max_gain_db=30.0, extra=5, n_max=None):
    """Reference first, then the C entry (E) and the Python layer on a poisoned, strided copy.  Returns (refs, stats, y, raw)."""
    from tacotron2_amd import analysis
    x, n = _pad(rows, n_max)
    refs = [R.measure(x[b, :n[b]], sr) for b in range(len(n))]
    assert all(r["margin_lu"] > 1e-6 for r in refs), [r["margin_lu"] for r in refs]       # (before the device is touched)
    wav = _poison(x, n, extra)
    hop = int(round(sr / 10))
    raw = _raw(wav, n, sr, target, ceiling, max_gain_db)
    y, stats = analysis.normalize_loudness(wav, n, sr, target=target, ceiling=ceiling, max_gain_db=max_gain_db)
    assert y.shape == wav.shape and y.dtype == torch.float32 and set(stats) == set(STAT)
    y, stats = y.cpu().numpy(), {k: v.cpu().numpy() for k, v in stats.items()}
    peak = _resample_peak(wav, n, sr)
    for k in ("lufs", "true_peak", "sample_peak", "rel_gate_lufs", "momentary_max_lufs"):               # the layer returns the entry's numbers
        assert np.array_equal(_bits64(stats[k]), _bits64(raw["stat"][:, STAT.index(k)])), k
    assert np.array_equal(_bits(stats["gain"]), _bits(raw["gain"])) and np.array_equal(_bits(y), _bits(raw["y"]))
    for b, ref in enumerate(refs):
        E = raw["E"][b, :n[b] // hop]
        assert len(E) == len(ref["E"]) and (np.abs(E - ref["E"]) <= 1e-9 * ref["E"]).all(), (b, np.abs(E / ref["E"] - 1).max())
        for k in ("n_blocks", "n_below_abs", "n_below_rel"):
            assert stats[k].dtype == np.int64 and stats[k][b] == ref[k], (b, k, stats[k][b], ref[k])
        g_ref, more = R.gain(ref["lufs"], float(peak[b]), target, ceiling, max_gain_db) if not ref["flags"] & R.UNDEFINED else (1.0, 0)
        assert stats["flags"][b] == ref["flags"] | more, (b, stats["flags"][b], ref["flags"], more)
        for k in ("lufs", "rel_gate_lufs", "momentary_max_lufs"):
            got, want = float(stats[k][b]), ref[k]
            assert (math.isnan(got) and math.isnan(want)) or got == want or abs(got - want) <= 1e-8, (b, k, got, want)
        assert stats["true_peak"][b] == float(peak[b]) and stats["true_peak"][b].dtype == np.float64          # t2_resample's bits
        assert abs(stats["true_peak"][b] - ref["true_peak"]) <= 1e-5 * ref["true_peak"]
        assert stats["sample_peak"][b] == ref["sample_peak"]
        g = stats["gain"][b]
        assert g.dtype == np.float32 and abs(float(g) - g_ref) <= np.spacing(np.float32(g_ref)), (b, g, g_ref)
        assert abs(raw["stat"][b, 1] - g_ref) <= 1e-9 * g_ref
        assert np.array_equal(_bits(y[b, :n[b]]), _bits(x[b, :n[b]] * g)) and not _bits(y[b, n[b]:]).any()
    return refs, stats, y, raw


def test_rows_of_0_1_n_minus_1_n_and_n_plus_h_samples_in_one_strided_batch():
    lengths = [0, 1, N - 1, N, N + H - 1, N + H, 2 * 8192 + 77]         # the last: two passes of the filter and a part of a third
    refs, stats, _, _ = check([_voice(10 + i, n, 0.1) for i, n in enumerate(lengths)], extra=7)
    assert [r["n_blocks"] for r in refs] == [0, 1, 1, 1, 1, 2, 17]
    assert [r["flags"] for r in refs] == [R.UNDEFINED, R.SHORT, R.SHORT, 0, 0, 0, 0]
    assert np.isnan(stats["lufs"][0]) and stats["gain"][0] == 1.0 and all(np.isfinite(stats["lufs"][1:]))


@pytest.mark.parametrize("sr", [8000, 22050])
def test_the_gate_signal(sr):
    refs, stats, _, _ = check([R.gate_signal(sr)], sr=sr)
    assert (stats["n_blocks"][0], stats["n_below_abs"][0], stats["n_below_rel"][0]) == (37, 7, 10)
    assert abs(stats["lufs"][0] - (-26.24 if sr == 8000 else -26.39)) <= 0.005
    assert stats["lufs"][0] - refs[0]["ungated_lufs"] > 2.0                                     # gating matters


def test_48_khz_and_the_standards_sine():
    refs, stats, _, _ = check([R.sine(48000, 997.0, 1.0), _voice(3, 30011, 0.05, 48000)], sr=48000, target=-30.0)
    assert abs(stats["lufs"][0] + 3.01) <= 0.01


def test_silence_a_limited_row_and_a_capped_row():
    rows = [np.zeros(5000, np.float32), R.sine(SR, SR / 4.0, 0.5, 0.9, math.pi / 4.0), _voice(5, 6000, 1e-3), _voice(6, 7001, 0.1)]
    refs, stats, y, raw = check(rows, target=-3.0, ceiling=-6.0)
    x, n = _pad(rows)
    assert stats["flags"].tolist() == [R.UNDEFINED, R.LIMITED, R.CAPPED, R.LIMITED] and stats["gain"][0] == 1.0
    assert np.array_equal(_bits(y[0]), _bits(x[0]))                                              # silence: y == x bit for bit
    assert stats["true_peak"][1] > 1.2 * stats["sample_peak"][1]                                 # the peak lies between the samples
    assert stats["gain"][2] == np.float32(10.0 ** 1.5)
    # the ceiling holds for what was written: the true peak of y, measured again
    from tacotron2_amd import analysis
    again = analysis.loudness(torch.from_numpy(y).to(DEV), n, SR)["true_peak"].cpu().numpy()
    c = 10.0 ** (-6.0 / 20.0)
    assert (again[[1, 3]] <= c * (1.0 + 1e-5)).all() and (again[[1, 3]] >= c * (1.0 - 1e-5)).all() and again[2] < c


def test_measuring_writes_no_waveform(monkeypatch):
    from tacotron2_amd import analysis, loudness
    seen = []
    make = loudness.make
    monkeypatch.setattr(loudness, "make", lambda name, **kw: (seen.append(kw), make(name, **kw))[1])
    x, n = _pad([_voice(7, 5000, 0.1), _voice(8, 300, 0.5)])
    stats = analysis.loudness(_poison(x, n), n, SR)
    assert len(seen) == 1 and seen[0]["y"] is None and "gain" not in stats and set(stats) == set(STAT) - {"gain"}
    raw = _raw(_poison(x, n), n, SR, target=-5.0, write=False)           # a target that would be limited: measuring sets no gain flag
    assert raw["gain"].tolist() == [1.0, 1.0] and raw["stat"][:, 9].tolist() == [0.0, 1.0] and raw["stat"][:, 1].tolist() == [1.0, 1.0]
    for b in range(2):
        ref = R.measure(x[b, :n[b]], SR)
        assert abs(float(stats["lufs"][b]) - ref["lufs"]) <= 1e-8 and int(stats["flags"][b]) == ref["flags"]
    y, full = analysis.normalize_loudness(_poison(x, n), n, SR)
    assert torch.equal(full["lufs"], stats["lufs"]) and torch.equal(full["true_peak"], stats["true_peak"])


def test_two_calls_give_identical_bits_and_a_row_does_not_depend_on_the_batch():
    rows = [_voice(20 + i, n, a) for i, (n, a) in enumerate([(9000, 0.1), (2 * 8192 + 77, 0.03), (2500, 0.2), (0, 0.0), (12345, 1e-3)])]
    x, n = _pad(rows)
    a, b = _raw(_poison(x, n), n, SR), _raw(_poison(x, n), n, SR)
    hops = [v // H for v in n]
    for k in ("stat", "E"):
        for r in range(5):
            cols = slice(0, hops[r]) if k == "E" else slice(None)
            assert np.array_equal(_bits64(a[k][r, cols]), _bits64(b[k][r, cols])), (k, r)
    assert np.array_equal(_bits(a["gain"]), _bits(b["gain"])) and np.array_equal(_bits(a["y"]), _bits(b["y"]))
    for r in (0, 1, 4):                                                  # alone, with another leading dimension
        xr, nr = _pad([rows[r]], n_max=n[r] + 3)
        one = _raw(_poison(xr, nr, extra=11), nr, SR)
        assert np.array_equal(_bits64(one["stat"][0]), _bits64(a["stat"][r])) and np.array_equal(_bits(one["gain"]), _bits(a["gain"][r:r + 1]))
        assert np.array_equal(_bits64(one["E"][0, :hops[r]]), _bits64(a["E"][r, :hops[r]]))
        assert np.array_equal(_bits(one["y"][0, :n[r]]), _bits(a["y"][r, :n[r]]))


def test_normalise_then_measure_reads_the_target():
    from tacotron2_amd import analysis
    rows = [_voice(30, 12000, 0.05), _voice(31, 2 * 8192 + 77, 0.2), _voice(32, 2000, 0.02), R.gate_signal(SR)[:16000]]
    x, n = _pad(rows)
    for r in rows:                                                        # every block 1 LU from the absolute gate, before and after the gain
        m = R.measure(r, SR)
        before = R.lufs(m["z"][m["z"] > 0]) + 70.0
        after = before + (-23.0 - m["lufs"])
        assert (np.sign(before) == np.sign(after)).all() and min(np.abs(before).min(), np.abs(after).min()) > 1.0
    y, stats = analysis.normalize_loudness(_poison(x, n), n, SR, target=-23.0, ceiling=0.0)
    assert not (stats["flags"].cpu().numpy() & (R.LIMITED | R.CAPPED)).any()
    again = analysis.loudness(y, n, SR)
    assert (again["lufs"] + 23.0).abs().max().item() <= 1e-4
    assert torch.equal(again["n_blocks"], stats["n_blocks"]) and torch.equal(again["n_below_rel"], stats["n_below_rel"])


def test_a_device_count_out_of_range_is_refused_on_the_device():
    from tacotron2_amd import analysis
    x, n = _pad([_voice(40, 5000, 0.1), _voice(41, 4000, 0.1), _voice(42, 3000, 0.1)])
    wav = _poison(x, n)
    for bad in ([5000, 5001, 3000], [5000, -1, 3000]):
        with pytest.raises(ValueError, match="refused on the device"):
            analysis.normalize_loudness(wav, torch.tensor(bad, device=DEV), SR)
        raw = _raw(wav, bad, SR)
        assert raw["stat"][1, 9] == -1.0 and np.isnan(raw["stat"][1, :9]).all() and np.isnan(raw["gain"][1]) and np.isnan(raw["y"][1]).all()
        assert np.isnan(raw["E"][1]).all()                                # nothing was written for the row ...
        good = _raw(wav, n, SR)
        for r in (0, 2):                                                  # ... and its neighbours are what they are without it
            assert np.array_equal(_bits64(raw["stat"][r]), _bits64(good["stat"][r])) and np.array_equal(_bits(raw["y"][r]), _bits(good["y"][r]))
    y, stats = analysis.normalize_loudness(wav, torch.tensor(n, device=DEV), SR)                  # device counts in range
    y2, stats2 = analysis.normalize_loudness(wav, n, SR)
    assert torch.equal(y, y2) and torch.equal(stats["gain"], stats2["gain"])
    empty, st = analysis.normalize_loudness(torch.zeros(2, 0, device=DEV), [0, 0], SR)           # (a batch without a column)
    assert empty.shape == (2, 0) and st["flags"].tolist() == [2, 2] and st["gain"].tolist() == [1.0, 1.0]


def test_err_arg_before_any_launch():
    from tacotron2_amd import _lib, loudness
    from tacotron2_amd.datasets.resample import plan
    b1, a1, b2, a2 = loudness.k_weighting(SR)
    _, _, K, table = plan(SR, 4 * SR)
    x = torch.zeros(2, 4000, device=DEV)
    ok = dict(x=x, ldx=4000, n=torch.tensor([4000, 10], dtype=torch.int32, device=DEV), table=torch.from_numpy(table).to(DEV), K=K, B=2,
              n_max=4000, H=H, b1=b1, a1=a1, b2=b2, a2=a2, abs_gate=R.ABS_GATE, target=-23.0, max_gain=10.0, ceiling=0.9,
              E=torch.zeros(2, 5, dtype=torch.float64, device=DEV), lde=5, stat=torch.zeros(2, 10, dtype=torch.float64, device=DEV),
              gain=torch.zeros(2, device=DEV), y=torch.zeros(2, 4000, device=DEV), ldy=4000)
    _lib.call("t2_loudness", _lib.make("T2Loudness", **ok), _lib.stream())
    marker = torch.full((2, 10), -7.0, dtype=torch.float64, device=DEV)
    for change, msg in ((dict(x=None), "null"), (dict(B=0), "B outside"), (dict(B=65536), "B outside"), (dict(H=0), "H < 1"),
                        (dict(lde=4), "lde < n_max / H"), (dict(ldx=3999), "ldx < n_max"), (dict(table=None), "null"), (dict(K=0), "K outside"),
                        (dict(n=None), "null"), (dict(E=None), "null"), (dict(stat=None), "null"), (dict(gain=None), "null"),
                        (dict(ldy=3999), "ldy < n_max"), (dict(n_max=-1), "n_max < 0"), (dict(a1=(1.0, float("nan"), 0.5)), "not finite"),
                        (dict(ceiling=0.0), "ceiling"), (dict(max_gain=float("inf")), "max_gain"), (dict(target=float("nan")), "target")):
        kw = dict(ok, stat=marker)
        kw.update(change)
        with pytest.raises(_lib.T2Error, match=msg):
            _lib.call("t2_loudness", _lib.make("T2Loudness", **kw), _lib.stream())
    torch.cuda.synchronize()
    assert (marker == -7.0).all()                                         # refused before any launch
    _lib.call("t2_loudness", _lib.make("T2Loudness", **dict(ok, x=None, n_max=0, ldx=0, ldy=0, y=None, n=torch.zeros(2, dtype=torch.int32, device=DEV))),
              _lib.stream())                                              # (a null x is fine without a sample)
