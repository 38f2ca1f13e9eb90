"""t2_voice_quality and t2_corpus_stats on the GPU through the C ABI against the float64 restatement tests/voice_quality_ref.py, then
engine.voice_quality / engine.corpus_stats and ProsodyMeter.features.

The cycle counts and the zero outputs of every frame that is not measured are compared exactly.  The pick tau* of a cycle (recovered
from T_i, which lies within one lag of it) is compared exactly on the STABLE cycles - those whose float64 margin between the best and
the second-best ncc exceeds 16 x the largest ncc deviation of the two float32 restatements (numpy pairwise, strictly sequential) from
float64 on the same inputs - and the unstable ones may be at most 5 % of all cycles.  T_i, r_i, A_i and the frame values are compared
within 8 x the larger deviation of the two restatements from float64, computed here: the factor covers a third summation order, the
kernel's (products left to right per pair, window energies as a running sum from tau = L outwards).  The measured tolerances and GPU
deviations are printed and quoted in DESIGN 5.12."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import voice_quality_ref as V

pytestmark = pytest.mark.gpu
DEFAULT = dict(V.DEFAULTS)
SMALL = dict(sr=8000, hop=64, W=80, tau_min=10, tau_max=100)        # S = 180; period 37.3 -> L = 37, d = 5, K = 3: the measured edge
OUTS = ("jitter", "shimmer", "nhr", "hnr_db")


def _struct(wav, n, cfg, n_max, f0, outs, cyc, ld_wav=None):
    from tacotron2_amd import _lib
    return _lib.make("T2VoiceQuality", wav=wav, ld_wav=wav.stride(0) if ld_wav is None else ld_wav, n=n, B=wav.shape[0], n_max=n_max,
                     sr=cfg["sr"], hop=cfg["hop"], W=cfg["W"], tau_min=cfg["tau_min"], tau_max=cfg["tau_max"], f0=f0,
                     jitter=outs[0], shimmer=outs[1], nhr=outs[2], hnr_db=outs[3], cycles=outs[4], cyc=cyc)


def run_vq(signals, f0, cfg, with_cyc=True, pad=37):
    """One t2_voice_quality call: row stride n_max + pad, NaN behind every n[b], outputs pre-filled with NaN (cycles: -7)."""
    from tacotron2_amd import _lib
    dev = torch.device("cuda:0")
    B, n_max = len(signals), max(len(s) for s in signals)
    T = 1 + n_max // cfg["hop"]
    wav = torch.full((B, n_max + pad), float("nan"), dtype=torch.float32)
    for b, s in enumerate(signals):
        wav[b, :len(s)] = torch.from_numpy(s)
    wav = wav.to(dev)
    n = torch.tensor([len(s) for s in signals], dtype=torch.int64, device=dev)
    outs = [torch.full((B, T), float("nan"), device=dev) for _ in range(4)] + [torch.full((B, T), -7, dtype=torch.int32, device=dev)]
    cyc = torch.full((B, T, V.MAX_CYCLES, 3), float("nan"), device=dev) if with_cyc else None
    _lib.call("t2_voice_quality", _struct(wav, n, cfg, n_max, torch.from_numpy(f0).to(dev), outs, cyc),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs] + [cyc.cpu().numpy() if cyc is not None else None]


def _valid(T, n, hop, S):
    s0 = np.arange(T) * hop - S // 2
    return (s0 >= 0) & (s0 + S <= n)


def inputs(name):
    """(signals, f0 track float32 (B, T), cfg).  Invalid frames of the track hold NaN: they are not read."""
    if name == "small":
        rng = np.random.default_rng(5)
        t = np.arange(4001)
        x = 0.3 * np.sin(2 * np.pi * t / 37.3) + 0.1 * np.sin(4 * np.pi * t / 37.3) + 0.003 * rng.normal(size=4001)
        x[600:800] = 0.05 * rng.normal(size=200)
        x[800:920] = 0.0                                      # (cycles that lie in it have ncc = 0 at every lag: a tie, never stable)
        signals, cfg = [x.astype(np.float32)], SMALL
        f0 = np.full((1, 1 + 4001 // 64), 8000 / 37.3, np.float32)
        f0[0, 20] = 0.0                                       # unvoiced
        f0[0, 22] = 8000 / 38.0                               # L = 38: K = (180 - 76 - 5) // 38 + 1 = 3, still measured
        f0[0, 24] = 8000 / 45.0                               # L = 45, d = 6: K = 84 // 45 + 1 = 2, not measured
        f0[0, 26] = 8000 / 12.0                               # L = 12, d = 2: K = 13
        f0[0, 28] = 0.0
    else:
        a, _ = V.voice(90.0, 15999, jitter=0.01, shimmer=0.03, noise=0.02, amp=0.2, seed=1)
        b1, _ = V.voice(120.0, 7000, jitter=0.005, shimmer=0.03, noise=0.10, amp=0.3, seed=2)
        b2, _ = V.voice(210.0, 6001, jitter=0.02, shimmer=0.05, noise=0.01, amp=0.1, seed=3)
        c, _ = V.voice(120.0, 1300, seed=4)                   # shorter than one span of 1391: no valid frame
        signals, cfg = [a, np.concatenate([b1, b2]), c], DEFAULT
        T = 1 + 15999 // 256
        f0 = np.zeros((3, T), np.float32)
        f0[0] = 90.0
        f0[1, :27] = 120.0                                    # (frame 27 = sample 6912: its span straddles the change of voice)
        f0[1, 27:] = 210.0
        f0[2] = 120.0
        rng = np.random.default_rng(9)
        f0 *= (1.0 + 0.02 * rng.uniform(-1, 1, size=f0.shape)).astype(np.float32)          # L varies by a few samples
        f0[0, 10:13] = 0.0                                    # unvoiced frames
        f0[1, 40] = 0.0
        f0[0, 30] = 61.0                                      # L = 361, d = 46: 1391 - 722 - 46 = 623 -> K = 2, not measured
        f0[0, 31] = -50.0                                     # not > 0: unvoiced
    S = cfg["W"] + cfg["tau_max"]
    for b_, s in enumerate(signals):
        f0[b_, ~_valid(f0.shape[1], len(s), cfg["hop"], S)] = np.nan
    return signals, f0, cfg


@functools.lru_cache(maxsize=None)
def case(name):
    """(signals, f0, cfg, float64 reference, tolerances, stable, dev_ncc, GPU outputs) - computed once per configuration."""
    signals, f0, cfg = inputs(name)
    ref, tol, stable, dev_ncc = V.tolerances(signals, f0, **cfg)
    return signals, f0, cfg, ref, tol, stable, dev_ncc, run_vq(signals, f0, cfg)


@pytest.mark.parametrize("name", ["small", "default"])
def test_voice_quality_against_the_float64_reference(name):
    signals, f0, cfg, ref, tol, stable, dev_ncc, got = case(name)
    jit, shi, nhr, hnr, cycles, cyc = got
    print(f"{name}: tolerances {tol}, largest float32 ncc deviation {dev_ncc:.3e}")
    for a in (jit, shi, nhr, hnr, cyc):
        assert np.isfinite(a).all()                           # everything written, nothing read at or behind n[b] (NaN there)
    # counts and zeros, exactly
    assert (cycles == ref["cycles"]).all()
    me = ref["cycles"] > 0
    assert me.sum() >= 10 and (ref["valid"] & ~me).sum() >= 3 and (~ref["valid"]).sum() >= 3
    if name == "small":
        assert set(ref["cycles"][0][[20, 22, 24, 26]].tolist()) == {0, 3, 13} and ref["frames"][(0, 21)]["L"] == 37
        assert (ref["cycles"][0, 10:16] == 3).all()          # frames in the stretch of noise and of exact zeros are measured too
        assert sum(int((fr["r"] == 0).sum()) for fr in ref["frames"].values()) >= 3         # ... some cycles wholly in the zeros
    else:
        assert not ref["valid"][2].any() and ref["cycles"][0, 30] == 0 and ref["valid"][0, 30]
        assert {ref["frames"][k]["L"] for k in ref["frames"]} >= {245, 184, 105}
    for a in (jit, shi, nhr, hnr):
        assert (a[~me] == 0).all()
    assert (cyc[~me] == 0).all()
    for (b, t), fr in ref["frames"].items():
        assert (cyc[b, t, fr["K"]:] == 0).all()               # the rows behind K are zeros
    # the picks on the stable cycles, and the stability cap
    n_cyc = sum(fr["K"] for fr in ref["frames"].values())
    n_unstable = sum(int((~st).sum()) for st in stable.values())
    print(f"{name}: {me.sum()} measured frames, {n_cyc} cycles, {n_unstable} unstable, "
          f"{tol['n_differing_picks']} picks differ in a float32 restatement")
    assert n_unstable <= 0.05 * n_cyc
    dev = dict(T=0.0, r=0.0, A=0.0, jitter=0.0, shimmer=0.0, nhr=0.0, hnr_db=0.0)
    n_frames_cmp = 0
    for (b, t), fr in ref["frames"].items():
        K, st = fr["K"], stable[(b, t)]
        g = cyc[b, t, :K]
        tau_ref = fr["L"] - fr["d"] + fr["k"]
        assert (np.abs(np.rint(g[:, 0]) - tau_ref)[st] <= 1).all(), (b, t)
        assert (np.abs(g[:, 0] - tau_ref)[st] <= 1).all(), (b, t)
        if st.any():
            dev["T"] = max(dev["T"], float(np.max(np.abs(g[:, 0] - fr["T"])[st])))
            dev["r"] = max(dev["r"], float(np.max(np.abs(g[:, 1] - fr["r"])[st])))
            nz = st & (fr["A"] > 0)
            assert (g[:, 2][st & (fr["A"] == 0)] == 0).all()
            if nz.any():
                dev["A"] = max(dev["A"], float(np.max((np.abs(g[:, 2] - fr["A"]) / np.where(fr["A"] > 0, fr["A"], 1))[nz])))
        if st.all():                                          # frame values: only where every cycle's pick is settled
            n_frames_cmp += 1
            dev["jitter"] = max(dev["jitter"], abs(float(jit[b, t]) - float(fr["jitter"])))
            dev["shimmer"] = max(dev["shimmer"], abs(float(shi[b, t]) - float(fr["shimmer"])))
            dev["hnr_db"] = max(dev["hnr_db"], abs(float(hnr[b, t]) - float(fr["hnr_db"])))
            dev["nhr"] = max(dev["nhr"], abs(float(nhr[b, t]) - float(fr["nhr"])) / float(fr["nhr"]))
    print(f"{name}: GPU deviations {dev} ({n_frames_cmp} frames with all cycles stable)")
    assert n_frames_cmp >= 10
    for q, v in dev.items():
        assert v <= tol[q], (q, v, tol[q])


@pytest.mark.parametrize("name", ["small", "default"])
def test_voice_quality_is_reproducible_and_cyc_is_optional(name):
    signals, f0, cfg, *_, first = case(name)
    again = run_vq(signals, f0, cfg)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    *outs, cyc = run_vq(signals, f0, cfg, with_cyc=False, pad=0)                # ld_wav == n_max, no cyc
    assert cyc is None
    for a, b in zip(first[:5], outs):
        assert a.tobytes() == b.tobytes()


def test_voice_quality_bad_arguments_return_the_code_without_a_launch():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wav = torch.zeros(2, 3000, device=dev)
    n = torch.tensor([3000, 2000], dtype=torch.int64, device=dev)
    T = 1 + 3000 // 256
    f0 = torch.full((2, T), 150.0, device=dev)
    outs = [torch.full((2, T), -7.0, device=dev) for _ in range(4)] + [torch.full((2, T), -7, dtype=torch.int32, device=dev)]
    cyc = torch.full((2, T, 32, 3), -7.0, device=dev)

    def rc(n_max=3000, **over):
        s = _struct(wav, n, DEFAULT, n_max, f0, outs, cyc, ld_wav=over.pop("ld_wav", None))
        for k, v in over.items():
            setattr(s, k, v)
        return lib.t2_voice_quality(C.addressof(s), None)

    for field in ("wav", "n", "f0", "jitter", "shimmer", "nhr", "hnr_db", "cycles"):
        assert rc(**{field: None}) == 1, field
        assert b"t2_voice_quality" in lib.t2_last_error()
    assert rc(B=0) == 1 and rc(B=-1) == 1 and rc(B=65536) == 1
    assert rc(hop=0) == 1 and rc(sr=0) == 1 and rc(n_max=-1) == 1
    assert rc(W=15) == 1
    assert rc(tau_min=1) == 1
    assert rc(tau_min=44, tau_max=45) == 1 and rc(tau_min=44, tau_max=44) == 1
    assert rc(W=4096 - 367 + 1) == 1                        # S = T2_YIN_MAX_SPAN + 1
    assert rc(ld_wav=2999) == 1
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs + [cyc])        # nothing ran
    assert rc() == 0 and rc(cyc=None) == 0                  # the same block, unchanged, is accepted
    torch.cuda.synchronize()
    assert all(bool((o != -7).all()) for o in outs + [cyc])


# --------------------------------------------------------------------------------------------------------------------------------
# t2_corpus_stats
# --------------------------------------------------------------------------------------------------------------------------------
def run_corpus(f0, power, vq, n, hop, S, power_floor=1e-10):
    from tacotron2_amd import _lib
    dev = torch.device("cuda:0")
    B, T = f0.shape
    out = torch.full((B, 12), -7.0, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s = _lib.make("T2CorpusStats", f0=up(f0), power=up(power), jitter=up(vq["jitter"]), shimmer=up(vq["shimmer"]), nhr=up(vq["nhr"]),
                  hnr_db=up(vq["hnr_db"]), cycles=up(vq["cycles"]), n=torch.tensor(n, dtype=torch.int64, device=dev), B=B, T=T,
                  hop=hop, S=S, power_floor=power_floor, out=out)
    _lib.call("t2_corpus_stats", s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_corpus_stats_on_the_kernels_own_outputs():
    """The rows of the default case from the GPU's own per-frame outputs against float64 means of the same arrays - the third
    utterance has no valid frame: a row of zeros; the invalid frames of the inputs hold NaN and are not read.  A float32 row of fp64
    means: within 1e-6 relative."""
    signals, f0, cfg, ref, *_, got = case("default")
    jit, shi, nhr, hnr, cycles, _ = got
    S = cfg["W"] + cfg["tau_max"]
    rng = np.random.default_rng(3)
    power = (10.0 ** rng.uniform(-12, -1, size=f0.shape)).astype(np.float32)            # some frames under the floor of 1e-10
    inv = ~ref["valid"]
    vq = dict(jitter=jit.copy(), shimmer=shi.copy(), nhr=nhr.copy(), hnr_db=hnr.copy(), cycles=cycles.copy())
    power[inv] = np.nan
    for q in OUTS:
        vq[q][inv] = np.nan
    vq["cycles"][inv] = 9
    n = [len(s) for s in signals]
    out = run_corpus(f0, power, vq, n, cfg["hop"], S)
    print(out)
    for b in range(3):
        want = V.corpus_stats(f0[b], power[b], {k: v[b] for k, v in vq.items()}, ref["valid"][b])
        assert out[b, :4].tolist() == want[:4] and out[b, 10] == 0 and out[b, 11] == 0, (b, out[b], want)
        for k in range(4, 10):
            assert abs(out[b, k] - want[k]) <= 1e-6 * abs(want[k]), (b, k, out[b, k], want[k])
    assert out[0, 0] > out[0, 1] > out[0, 2] > 10 and 0 < out[0, 3] < out[0, 0]
    assert (out[2] == 0).all()                                # the all-empty utterance


@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257])
def test_corpus_stats_at_the_wave_and_block_edges(T):
    """The lengths at which a lane, a wave or the second round of the 256-thread block is empty or holds one frame.  B = 2, hop = S = 1
    (every frame inside n is valid): all T frames of the first utterance, none of the second (n = 0, NaN in its inputs).  Counts
    exact, means within 1e-6 relative, as on the kernel's own outputs."""
    rng = np.random.default_rng(200 + T)
    f0 = rng.choice(np.array([0, 98.5, 131.25, 220, 402.7], np.float32), size=(2, T))
    power = (10.0 ** rng.uniform(-12, -1, size=(2, T))).astype(np.float32)              # some frames under the floor of 1e-10
    vq = {q: rng.uniform(0.001, 0.2, size=(2, T)).astype(np.float32) for q in OUTS}
    vq["cycles"] = rng.integers(0, 4, size=(2, T)).astype(np.int32)
    f0[0, T - 1], power[0, T - 1], vq["cycles"][0, T - 1] = 220.0, 1e-3, 3             # the last frame counts everywhere
    f0[1], power[1], vq["cycles"][1] = np.nan, np.nan, 9
    for q in OUTS:
        vq[q][1] = np.nan
    out = run_corpus(f0, power, vq, [T, 0], 1, 1)
    for b, n in enumerate([T, 0]):
        want = V.corpus_stats(f0[b], power[b], {k: v[b] for k, v in vq.items()}, np.arange(T) < n)
        assert out[b, :4].tolist() == want[:4] and out[b, 10] == 0 and out[b, 11] == 0, (b, out[b], want)
        for k in range(4, 10):
            assert abs(out[b, k] - want[k]) <= 1e-6 * abs(want[k]), (b, k, out[b, k], want[k])
    assert out[0, 0] == T and out[0, 1] >= 1 and out[0, 2] >= 1 and out[0, 3] >= 1 and (out[1] == 0).all()


def test_corpus_stats_bad_arguments():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    x = torch.zeros(1, 8, device=dev)
    ci = torch.zeros(1, 8, dtype=torch.int32, device=dev)
    n = torch.tensor([8], dtype=torch.int64, device=dev)
    out = torch.full((1, 12), -7.0, device=dev)
    base = dict(f0=x, power=x, jitter=x, shimmer=x, nhr=x, hnr_db=x, cycles=ci, n=n, B=1, T=8, hop=1, S=1, power_floor=1e-10, out=out)
    for over in [dict(f0=None), dict(power=None), dict(jitter=None), dict(shimmer=None), dict(nhr=None), dict(hnr_db=None),
                 dict(cycles=None), dict(n=None), dict(out=None), dict(B=0), dict(B=65536), dict(T=0), dict(hop=0), dict(S=0),
                 dict(power_floor=float("nan"))]:
        s = _lib.make("T2CorpusStats", **dict(base, **over))
        assert lib.t2_corpus_stats(C.addressof(s), None) == 1, over
        assert b"t2_corpus_stats" in lib.t2_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    s = _lib.make("T2CorpusStats", **base)
    assert lib.t2_corpus_stats(C.addressof(s), None) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[8.0] + [0.0] * 11]        # valid frames only: silence is neither voiced, measured nor loud


# --------------------------------------------------------------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------------------------------------------------------------
def test_engine_voice_quality_and_corpus_stats_check_their_arguments():
    from tacotron2_amd import engine
    dev = torch.device("cuda:0")
    wav = torch.zeros(2, 3000, device=dev)
    n = torch.tensor([3000, 10], device=dev)
    f0 = torch.full((2, 12), 150.0, device=dev)
    got = engine.voice_quality(wav, n, f0)
    assert len(got) == 5 and all(g.shape == (2, 12) for g in got) and got[4].dtype == torch.int32
    assert int(got[4][0, 3]) == 8 and not got[4][1].any()   # L = 147, d = 19: (1391 - 294 - 19) // 147 + 1 = 8 cycles of silence
    assert abs(float(got[2][0, 3]) - 999.0) < 1e-2           # ... whose correlation 0 is clamped to 1e-3: nhr = 999
    assert engine.voice_quality(wav, n, f0, return_cycles=True)[5].shape == (2, 12, 32, 3)
    for bad in [dict(wav=wav.cpu()), dict(wav=wav.double()), dict(wav=wav[0]), dict(n=n.cpu()), dict(n=n.float()), dict(n=n[:1]),
                dict(W=8), dict(W=4000), dict(hop=0), dict(fmin=600.0), dict(n_max=3001), dict(wav=wav[:, ::2]), dict(f0=None),
                dict(f0=f0.cpu()), dict(f0=f0[:, :11]), dict(f0=f0.double())]:
        kw = dict(dict(wav=wav, n=n, f0=f0), **bad)
        with pytest.raises(ValueError) as e:
            engine.voice_quality(**kw)
        assert str(e.value).startswith("voice_quality"), bad
    z = torch.zeros(2, 12, device=dev)
    row = engine.corpus_stats(f0, z, *got, n)
    assert row.shape == (2, 12) and row[0, :4].tolist() == [7.0, 7.0, 7.0, 0.0] and float(row[0, 4]) == 150.0
    for bad in [dict(power=z.cpu()), dict(cycles=got[4].float()), dict(nhr=z[:, :5]), dict(hop=0), dict(span=0),
                dict(power_floor=float("nan")), dict(n=n.cpu())]:
        kw = dict(dict(f0=f0, power=z, jitter=got[0], shimmer=got[1], nhr=got[2], hnr_db=got[3], cycles=got[4], n=n), **bad)
        with pytest.raises(ValueError, match="corpus_stats:"):
            engine.corpus_stats(**kw)


def test_prosody_meter_features_on_generator_voices():
    """Three voices that differ in pitch, loudness, jitter and noise: the features order them, the _log twins and intensity_mean_vcd
    are measure()'s numbers, and the derived columns follow their definitions.  Silence and an empty waveform are undefined."""
    from tacotron2_amd.prosody import FEATURES, ProsodyMeter
    dev = torch.device("cuda:0")
    spec = [(100.0, 0.05, 0.003, 0.005, 20), (150.0, 0.1, 0.01, 0.03, 40), (220.0, 0.3, 0.02, 0.10, 60)]
    signals = [V.voice(f, 9000, jitter=j, shimmer=0.03, noise=nu, amp=a, seed=k)[0] for k, (f, a, j, nu, _) in enumerate(spec)]
    signals += [np.zeros(5000, np.float32), np.zeros(0, np.float32)]
    chars = [c for *_, c in spec] + [5, 7]
    wavs = [torch.from_numpy(s).to(dev) for s in signals]
    for smooth in (False, True):
        meter = ProsodyMeter(22050, dev, smooth=smooth)
        got, old = meter.features(wavs, chars), meter.measure(wavs, chars)
        assert meter.features([], []) == []
        print(got[:3])
        for g, m, s, c in zip(got, old, signals, chars):
            assert list(g) == ["n_frames", "n_voiced", "n_measured"] + FEATURES
            assert g["n_frames"] == m["n_frames"] and g["n_voiced"] == m["n_voiced"] and g["n_measured"] <= g["n_voiced"]
            assert g["pitch_mean_log"] == m["pitch_mean_log"] and g["pitch_range_log"] == m["pitch_range_log"]
            assert g["intensity_mean_vcd"] == m["intensity_mean_db"] and g["rate"] == m["rate"]
            assert g["nhr_vcd"] == g["nhr"] and g["duration"] == len(s) / 22050 and g["duration_vcd"] == g["n_voiced"] * 256 / 22050
        for k, (f, a, j, nu, c) in enumerate(spec):
            g = got[k]
            assert all(g[q] is not None for q in FEATURES) and g["n_measured"] >= 20
            # (the raw track of a jittered voice holds a few octave errors: the mean may lie under pitch_5, the percentiles stay)
            assert abs(g["pitch_mean"] / f - 1) < 0.1 and 0.97 * g["pitch_5"] <= f <= 1.03 * g["pitch_95"] and g["pitch_5"] <= g["pitch_95"]
            assert g["pitch_range"] == g["pitch_95"] - g["pitch_5"]
            assert abs(g["pitch_5_log"] - np.log(g["pitch_5"])) < 1e-12 and abs(g["pitch_95_log"] - np.log(g["pitch_95"])) < 1e-12
            assert abs(g["pitch_95_log"] - g["pitch_5_log"] - g["pitch_range_log"]) < 1e-12
            assert abs(g["intensity_mean"] - g["intensity_mean_vcd"]) < 1.0        # steady voices: all frames equally loud
            assert g["rate_vcd"] == c / g["duration_vcd"]
        for key in ("pitch_mean", "pitch_mean_log", "intensity_mean", "jitter", "nhr", "rate"):
            assert got[0][key] < got[1][key] < got[2][key], key
        assert got[3]["n_frames"] > 0 and got[3]["n_voiced"] == 0 and got[3]["duration_vcd"] == 0
        assert all(got[3][q] is None for q in FEATURES if q not in ("duration", "duration_vcd", "rate"))
        assert got[4]["rate"] is None and got[4]["duration"] == 0 and got[4]["n_frames"] == 0
