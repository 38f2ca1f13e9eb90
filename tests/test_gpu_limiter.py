"""t2_limit / analysis.limit_peaks / analysis.normalize_loudness(limiter=) on the GPU against tests/limiter_ref.py.

What is EXACT: env has the bits of the maxima formed from engine.resample(x, n, sr, 4 sr) and |x| - the kernel's taps are t2_resample's
-, in_peak is max(true_peak, sample_peak) of analysis.loudness, and everything the rule decides from env's bits follows without a
tolerance: n_over, r and its sliding minimum h (seen through a release so short that e == h: the box mean of float32 values is exact
in fp64 whatever the order, so curve has the reference's bits), peak_after as the same maxima of x * curve, the trim as the largest
float32 under the ceiling, y as float32(float32(x * curve) * trim) from the device's own curve and trim, zeros behind n[b].
What is HELD TO A BOUND: the release runs chunked on the device and meets the sequential recurrence to tau / e * 2^-53
(tests/test_limiter_ref_host.py), the box sum adds L + 1 <= 2049 values of at most 1 in another order, 2049 * 2^-53 - both far inside
a float32 ulp, 6e-8, so curve is within ONE float32 ulp of the reference's and min_gain within 1e-9.
The promise: the true peak of y, measured again by t2_loudness, is at most ceiling * (1 + 1e-5), that module's figure for 32 float32
taps.  The rows are NaN behind n[b] and in the padding up to ldx; the outputs are NaN-filled with leading dimensions of their own."""
import numpy as np
import pytest
import torch

import limiter_ref as M
import loudness_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 8000
C_DB = -1.0
C = 10.0 ** (C_DB / 20.0)
STAT = ("in_peak", "n_over", "min_gain", "peak_after", "trim", "flags")


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


def _table(sr):
    from tacotron2_amd.datasets.resample import plan
    _, _, K, table = plan(sr, 4 * sr)
    return K, torch.from_numpy(table).to(DEV)


def _raw(wav, n, L, a, c=C, sr=SR, pads=(3, 1, 2)):
    """The C entry itself on NaN-filled outputs whose rows are ld + pads apart: dict(env, curve, y, stat) as numpy arrays."""
    from tacotron2_amd import _lib
    B, ld = wav.shape
    K, table = _table(sr)
    env, curve, y = (torch.full((B, ld + p), float("nan"), device=DEV) for p in pads)
    stat = torch.full((B, 8), float("nan"), dtype=torch.float64, device=DEV)
    arg = _lib.make("T2Limit", x=wav, ldx=wav.stride(0) if B > 1 else max(ld, 1), n=torch.as_tensor(n, dtype=torch.int32).to(DEV), table=table, K=K,
                    B=B, n_max=ld, L=L, a=a, ceiling=c, env=env, lde=ld + pads[0], curve=curve, ldc=ld + pads[1], y=y, ldy=ld + pads[2], stat=stat)
    _lib.call("t2_limit", arg, _lib.stream())
    torch.cuda.synchronize()
    return dict(env=env.cpu().numpy(), curve=curve.cpu().numpy(), y=y.cpu().numpy(), stat=stat.cpu().numpy())


def _peaks(x, n, sr=SR):
    """P of every row - max(|x[i]|, |u[4i]|, .., |u[4i+3]|), u = engine.resample(x, n, sr, 4 sr) - as float32 arrays."""
    from tacotron2_amd import engine
    wav = _poison(x, n)
    if max(n) == 0:
        return [np.zeros(0, np.float32) for _ in n]
    out, n_out = engine.resample(wav, n, sr, 4 * sr)
    assert n_out == [4 * v for v in n]
    out = out.cpu().numpy()
    return [np.maximum(np.abs(out[b, :4 * n[b]]).reshape(n[b], 4).max(axis=1), np.abs(x[b, :n[b]])) for b in range(len(n))]


def check(rows, L, a, c=C, extra=5):
    """The C entry on a poisoned, strided copy against the reference built from the device's own env.  Returns (refs, raw)."""
    from tacotron2_amd import analysis
    x, n = _pad(rows)
    wav = _poison(x, n, extra)
    raw = _raw(wav, n, L, a, c)
    P = _peaks(x, n)
    loud = {k: v.cpu().numpy() for k, v in analysis.loudness(wav, n, SR).items()}
    w = np.zeros_like(x)
    refs = []
    for b in range(len(n)):
        env, curve, st = raw["env"][b, :n[b]], raw["curve"][b, :n[b]], raw["stat"][b]
        assert np.array_equal(_bits(env), _bits(M.envelope(P[b]))), b                            # t2_resample's bits
        assert np.isnan(raw["env"][b, n[b]:]).all() and np.isnan(raw["curve"][b, n[b]:]).all()
        assert st[0] == (float(env.max()) if n[b] else 0.0) == max(loud["true_peak"][b], loud["sample_peak"][b]), (b, st[0])
        ref = M.gain_curve(env, c, L, a)
        assert st[1] == ref["n_over"], (b, st[1], ref["n_over"])
        assert (np.abs(curve.astype(np.float64) - ref["curve"]) <= np.spacing(ref["curve"])).all(), \
            (b, np.abs(curve.astype(np.float64) - ref["curve"]).max())
        assert abs(st[2] - ref["min_gain"]) <= 1e-9 and (curve <= ref["r"]).all(), (b, st[2], ref["min_gain"])
        if ref["n_over"] == 0:
            assert (curve == 1.0).all() and st[2] == 1.0
        w[b, :n[b]] = x[b, :n[b]] * curve
        refs.append(ref)
    Pw = _peaks(w, n)
    for b in range(len(n)):
        st, y = raw["stat"][b], raw["y"][b]
        assert st[3] == (float(Pw[b].max()) if n[b] else 0.0), (b, st[3])                          # peak_after: the same taps on x * curve
        t = M.trim(st[3], c)
        assert st[4] == float(t) and st[5] == (1 if refs[b]["n_over"] else 0) + (2 if st[3] > c else 0) and st[6] == st[7] == 0.0, (b, st)
        assert (st[4] < 1.0) == (st[3] > c) == bool(int(st[5]) & 2)
        print(f"row {b}: n {n[b]}, n_over {int(st[1])}, min_gain {st[2]:.6f}, peak_after / c - 1 = {st[3] / c - 1.0:+.2e}, trim {st[4]:.8f}, "
              f"max |curve - ref| = {np.abs(raw['curve'][b, :n[b]].astype(np.float64) - refs[b]['s']).max() if n[b] else 0.0:.2e}")
        assert np.array_equal(_bits(y[:n[b]]), _bits(w[b, :n[b]] * np.float32(st[4]))) and not _bits(y[n[b]:]).any(), b
    ld = x.shape[1]
    again = analysis.loudness(torch.from_numpy(np.ascontiguousarray(raw["y"][:, :ld])).to(DEV), n, SR)["true_peak"].cpu().numpy()
    assert (again <= c * (1.0 + 1e-5)).all(), (again / c).max()                                    # the promise
    return refs, raw


@pytest.mark.parametrize("L,release_ms", [(40, 50.0), (1, 5.0), (2048, 2000.0)])
def test_rows_of_every_length_and_peaks_at_every_pass_boundary_in_one_strided_batch(L, release_ms):
    from tacotron2_amd import limiter
    P = limiter.PASS
    rows = M.rows(P, L, SR)
    names = [name for name, _ in rows]
    assert [len(r) for _, r in rows][:8] == [0, 1, L, L + 1, P - 1, P, P + L + 1, 2 * P + 77]
    refs, raw = check([r for _, r in rows], L, M.coefficient(release_ms, SR), extra=7)
    x, n = _pad([r for _, r in rows])
    below, above = names.index("below"), names.index("above")
    assert raw["stat"][below, 1] == 0 and raw["stat"][below, 5] == 0 and np.array_equal(_bits(raw["y"][below, :n[below]]), _bits(x[below, :n[below]]))
    assert raw["stat"][above, 1] == n[above] and raw["stat"][0].tolist() == [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert all(raw["stat"][b, 1] > 0 for b in range(1, 9)) and raw["stat"][names.index("2P+77"), 1] > 20


def test_the_sliding_minimum_is_exact_seen_through_a_release_that_is_gone_in_one_sample():
    from tacotron2_amd import limiter
    P, a = limiter.PASS, 1e-30                                           # a e + (1 - a) == 1 in fp64: e == h
    for L in (40, 1, 2047, 2048):
        rows = [r for name, r in M.rows(P, L, SR) if name in ("P+L+1", "2P+77", "L+1")]
        x, n = _pad(rows)
        raw = _raw(_poison(x, n), n, L, a)
        for b in range(len(n)):
            env = raw["env"][b, :n[b]]
            ref = M.gain_curve(env, C, L, a)
            assert np.array_equal(ref["e"], ref["h"].astype(np.float64))
            assert np.array_equal(_bits(raw["curve"][b, :n[b]]), _bits(ref["curve"])), (L, b)
            assert raw["stat"][b, 2] == ref["min_gain"]


def test_the_python_layer_returns_the_entrys_numbers():
    from tacotron2_amd import analysis, limiter
    rows = [r for name, r in M.rows(limiter.PASS, 40, SR) if name in ("P", "2P+77", "below", "empty")]
    x, n = _pad(rows)
    wav = _poison(x, n)
    raw = _raw(wav, n, 40, M.coefficient(50.0, SR))
    y, stats = analysis.limit_peaks(wav, n, SR, return_curve=True)
    assert y.shape == wav.shape and y.dtype == torch.float32 and set(stats) == set(STAT) | {"env", "curve"}
    assert stats["n_over"].dtype == stats["flags"].dtype == torch.int64 and stats["env"].shape == stats["curve"].shape == wav.shape
    for i, k in enumerate(STAT):
        assert np.array_equal(_bits64(stats[k].cpu().numpy().astype(np.float64)), _bits64(raw["stat"][:, i])), k
    for b in range(len(n)):
        for k in ("env", "curve"):
            assert np.array_equal(_bits(stats[k][b, :n[b]].cpu().numpy()), _bits(raw[k][b, :n[b]])), (k, b)
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(raw["y"][:, :x.shape[1]]))
    y2, plain = analysis.limit_peaks(wav, torch.tensor(n, device=DEV), SR, ceiling=C_DB, lookahead_ms=5.0, release_ms=50.0)      # device counts in range
    assert torch.equal(y, y2) and set(plain) == set(STAT) and torch.equal(plain["min_gain"], stats["min_gain"])
    empty, st = analysis.limit_peaks(torch.zeros(2, 0, device=DEV), [0, 0], SR)                  # (a batch without a column)
    assert empty.shape == (2, 0) and st["flags"].tolist() == [0, 0] and st["trim"].tolist() == [1.0, 1.0]


def test_the_limited_voice_is_closer_to_the_target_than_the_plain_gain(monkeypatch):
    from tacotron2_amd import analysis, limiter, loudness
    target = -10.0
    voice = M.voice(1, 3 * SR, 0.1, SR)
    m = R.measure(voice, SR)                                             # in the reference first, before the device is touched
    g_plain, flags = R.gain(m["lufs"], m["true_peak"], target, C_DB)
    ref = M.limit(voice * np.float32(10.0 ** ((target - m["lufs"]) / 20.0)), SR, C, M.lookahead_samples(5.0, SR), M.coefficient(50.0, SR))
    ref_plain, ref_lim = R.measure(voice * np.float32(g_plain), SR)["lufs"], R.measure(ref["y"], SR)["lufs"]
    assert flags & R.LIMITED and abs(ref_lim - target) < abs(ref_plain - target) - 0.5
    x, n = _pad([voice, np.zeros(5000, np.float32), R.sine(SR, 440.0, 1.0, 0.05)])      # the sine reaches the target at 0.45 of full scale
    wav = _poison(x, n)
    seen = []
    for mod in (loudness, limiter):
        call = mod.call
        monkeypatch.setattr(mod, "call", lambda name, *a, _call=call: (seen.append(name), _call(name, *a))[1])
    yp, sp = analysis.normalize_loudness(wav, n, SR, target=target, ceiling=C_DB)
    assert seen == ["t2_loudness"] and sp["flags"].tolist() == [R.LIMITED, R.UNDEFINED, 0]      # None: today's path
    del seen[:]
    y, st = analysis.normalize_loudness(wav, n, SR, target=target, ceiling=C_DB, limiter=True)
    assert seen == ["t2_loudness", "t2_limit", "t2_loudness"]
    assert set(st) == set(sp) | {"in_peak", "n_over", "min_gain", "peak_after", "trim", "limiter_flags", "output_lufs", "output_true_peak"}
    assert st["flags"].tolist() == [0, R.UNDEFINED, 0] and st["limiter_flags"][1:].tolist() == [0, 0] and st["limiter_flags"][0].item() & 1
    assert torch.equal(st["lufs"][[0, 2]], sp["lufs"][[0, 2]]) and torch.equal(st["gain"][1:], sp["gain"][1:]) and st["gain"][0] > sp["gain"][0]
    plain_lufs = analysis.loudness(yp, n, SR)["lufs"][0].item()
    out = st["output_lufs"][0].item()
    print(f"plain {plain_lufs:.3f} LUFS (reference {ref_plain:.3f}), limiter {out:.3f} LUFS (reference {ref_lim:.3f}), target {target}")
    assert abs(out - target) < abs(plain_lufs - target) and abs(out - ref_lim) <= 1e-3 and abs(plain_lufs - ref_plain) <= 1e-3
    again = analysis.loudness(y, n, SR)
    assert torch.equal(again["lufs"][[0, 2]], st["output_lufs"][[0, 2]]) and torch.equal(again["true_peak"], st["output_true_peak"])
    assert (st["output_true_peak"] <= C * (1.0 + 1e-5)).all() and abs(st["n_over"][0].item() - ref["n_over"]) <= 2 and ref["n_over"] > 100
    assert torch.equal(y[1], wav[1].nan_to_num(0.0)) and not y[1].abs().max() > 0               # a row without a loudness keeps its bits
    assert torch.equal(y[2, :n[2]], yp[2, :n[2]]) and st["n_over"][2].item() == 0               # a row under the ceiling: the plain gain's bits
    y3, st3 = analysis.normalize_loudness(wav, n, SR, target=target, ceiling=C_DB, limiter=dict(lookahead_ms=2.0, release_ms=200.0))
    assert not torch.equal(y3[0], y[0]) and (st3["output_true_peak"] <= C * (1.0 + 1e-5)).all()


def test_two_calls_give_identical_bits_and_a_row_does_not_depend_on_the_batch():
    from tacotron2_amd import limiter
    rows = [r for name, r in M.rows(limiter.PASS, 40, SR) if name in ("P+L+1", "2P+77", "above", "below", "empty")]
    x, n = _pad(rows)
    a = M.coefficient(50.0, SR)
    one, two = _raw(_poison(x, n), n, 40, a), _raw(_poison(x, n), n, 40, a)
    assert np.array_equal(_bits64(one["stat"]), _bits64(two["stat"]))
    for k in ("env", "curve", "y"):
        for b in range(len(n)):
            assert np.array_equal(_bits(one[k][b, :n[b]]), _bits(two[k][b, :n[b]])), (k, b)
    for b in (1, 2, 3):                                                  # alone, with other leading dimensions
        xr, nr = _pad([rows[b]], n_max=n[b] + 3)
        alone = _raw(_poison(xr, nr, extra=11), nr, 40, a, pads=(0, 5, 9))
        assert np.array_equal(_bits64(alone["stat"][0]), _bits64(one["stat"][b]))
        for k in ("env", "curve", "y"):
            assert np.array_equal(_bits(alone[k][0, :n[b]]), _bits(one[k][b, :n[b]])), (k, b)


def test_a_device_count_out_of_range_is_refused_on_the_device():
    from tacotron2_amd import analysis
    x, n = _pad([M.pulses(40, 5000, [100, 4090], SR), M.pulses(41, 4000, [5], SR), M.pulses(42, 3000, [2999], SR)])
    wav = _poison(x, n)
    a = M.coefficient(50.0, SR)
    good = _raw(wav, n, 40, a)
    for bad in ([5000, 5001, 3000], [5000, -1, 3000]):
        with pytest.raises(ValueError, match="^limit_peaks: .*refused on the device"):
            analysis.limit_peaks(wav, torch.tensor(bad, device=DEV), SR)
        with pytest.raises(ValueError, match="^normalize_loudness: .*refused on the device"):
            analysis.normalize_loudness(wav, torch.tensor(bad, device=DEV), SR, limiter=True)
        raw = _raw(wav, bad, 40, a)
        assert raw["stat"][1, 5] == -1.0 and np.isnan(np.delete(raw["stat"][1], 5)).all()        # nothing else was written for the row ...
        assert np.isnan(raw["env"][1]).all() and np.isnan(raw["curve"][1]).all() and np.isnan(raw["y"][1]).all()
        for r in (0, 2):                                                  # ... and its neighbours are what they are without it
            assert np.array_equal(_bits64(raw["stat"][r]), _bits64(good["stat"][r])) and np.array_equal(_bits(raw["y"][r]), _bits(good["y"][r]))


def test_err_arg_before_any_launch():
    from tacotron2_amd import _lib
    K, table = _table(SR)
    x = torch.zeros(2, 4000, device=DEV)
    ok = dict(x=x, ldx=4000, n=torch.tensor([4000, 10], dtype=torch.int32, device=DEV), table=table, K=K, B=2, n_max=4000, L=40, a=0.99,
              ceiling=0.9, env=torch.zeros(2, 4000, device=DEV), lde=4000, curve=torch.zeros(2, 4000, device=DEV), ldc=4000,
              y=torch.zeros(2, 4000, device=DEV), ldy=4000, stat=torch.zeros(2, 8, dtype=torch.float64, device=DEV))
    _lib.call("t2_limit", _lib.make("T2Limit", **ok), _lib.stream())
    marker = torch.full((2, 8), -7.0, dtype=torch.float64, device=DEV)
    nan, inf = float("nan"), float("inf")
    for change, msg in ((dict(x=None), "null"), (dict(n=None), "null"), (dict(table=None), "null"), (dict(env=None), "null"),
                        (dict(curve=None), "null"), (dict(y=None), "null"), (dict(stat=None), "null"), (dict(B=0), "B outside"),
                        (dict(B=65536), "B outside"), (dict(n_max=-1), "n_max < 0"), (dict(ldx=3999), "ldx < n_max"),
                        (dict(lde=3999), "lde, ldc or ldy < n_max"), (dict(ldc=3999), "ldc"), (dict(ldy=3999), "ldy"), (dict(K=0), "K outside"),
                        (dict(K=4097), "K outside"), (dict(L=0), "L outside 1 .. 2048"), (dict(L=2049), "L outside"), (dict(a=0.0), "a not in"),
                        (dict(a=1.0), "a not in"), (dict(a=nan), "a not in"), (dict(a=-0.5), "a not in"), (dict(ceiling=0.0), "ceiling"),
                        (dict(ceiling=inf), "ceiling"), (dict(ceiling=nan), "ceiling"), (dict(ceiling=-1.0), "ceiling")):
        kw = dict(ok, stat=marker)
        kw.update(change)
        with pytest.raises(_lib.T2Error, match=r"t2_limit failed \(rc=1\): t2_limit: .*" + msg):
            _lib.call("t2_limit", _lib.make("T2Limit", **kw), _lib.stream())
        assert _lib.lib().t2_last_error().decode().startswith("t2_limit: ")
    torch.cuda.synchronize()
    assert (marker == -7.0).all()                                         # refused before any launch
    _lib.call("t2_limit", _lib.make("T2Limit", **dict(ok, x=None, n_max=0, ldx=0, n=torch.zeros(2, dtype=torch.int32, device=DEV))),
              _lib.stream())                                              # (a null x is fine without a sample)
    torch.cuda.synchronize()
    assert ok["stat"].cpu().numpy().tolist() == [[0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]] * 2
