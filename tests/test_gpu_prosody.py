"""t2_yin and t2_prosody_stats on the GPU through the C ABI against the float64 restatement tests/prosody_ref.py, then
tacotron2_amd.prosody.ProsodyMeter.

Lags and voiced flags are compared exactly on the STABLE frames - those where the float64 reference itself picks the same lag and flag
with thr and vthr scaled by 0.98 and by 1.02 - and the unstable ones may be at most 5 % of the valid frames.  cmnd, aper, power and f0
are compared within 8 x the larger deviation of the two float32 restatements (numpy pairwise, strictly sequential) from float64 on the
same inputs, computed here: the factor covers a third summation order, the kernel's (four contiguous quarters of j, sequential
within each).  The measured tolerances and GPU deviations are printed and quoted in DESIGN 5.10."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import prosody_ref as R

pytestmark = pytest.mark.gpu
DEFAULT = dict(R.DEFAULTS)
SMALL = dict(sr=8000, hop=64, W=80, tau_min=10, tau_max=100, thr=0.1, vthr=0.3, power_floor=1e-10)     # W no multiple of 64, B = 1


def _yin_struct(wav, n, cfg, n_max, outs, ld_wav=None):
    from tacotron2_amd import _lib
    f0, aper, power, cmnd = outs
    return _lib.make("T2Yin", wav=wav, ld_wav=wav.stride(0) if ld_wav is None else ld_wav, n=n, B=wav.shape[0], n_max=n_max,
                     sr=cfg["sr"], hop=cfg["hop"], W=cfg["W"], tau_min=cfg["tau_min"], tau_max=cfg["tau_max"], thr=cfg["thr"],
                     vthr=cfg["vthr"], power_floor=cfg["power_floor"], f0=f0, aper=aper, power=power, cmnd=cmnd)


def run_yin(signals, cfg, with_cmnd=True, pad=37):
    """One t2_yin call on the padded batch: row stride n_max + pad, NaN behind every n[b], outputs pre-filled with NaN."""
    from tacotron2_amd import _lib
    dev = torch.device("cuda:0")
    B, n_max = len(signals), max(len(s) for s in signals)
    T = 1 + n_max // cfg["hop"]
    wav = torch.full((B, n_max + pad), float("nan"), dtype=torch.float32)
    for b, s in enumerate(signals):
        wav[b, :len(s)] = torch.from_numpy(s)
    wav = wav.to(dev)
    n = torch.tensor([len(s) for s in signals], dtype=torch.int64, device=dev)
    outs = [torch.full((B, T), float("nan"), device=dev) for _ in range(3)]
    outs.append(torch.full((B, T, cfg["tau_max"] + 1), float("nan"), device=dev) if with_cmnd else None)
    _lib.call("t2_yin", _yin_struct(wav, n, cfg, n_max, outs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() if o is not None else None for o in outs]


@functools.lru_cache(maxsize=None)
def case(name):
    """(signals, cfg, float64 reference, tolerances, stable mask, GPU outputs) - computed once per configuration."""
    if name == "glides":
        signals, cfg = R.glides(), DEFAULT
    else:
        rng = np.random.default_rng(5)
        t = np.arange(2500)
        x = 0.3 * np.sin(2 * np.pi * t / 37.3) + 0.1 * np.sin(4 * np.pi * t / 37.3) + 0.003 * rng.normal(size=2500)
        x[600:800] = 0.05 * rng.normal(size=200)
        x[800:1000] = 0.0
        signals, cfg = [x.astype(np.float32)], SMALL
    ref, tol = R.tolerances(signals, **cfg)
    return signals, cfg, ref, tol, R.stable_frames(ref, **cfg), run_yin(signals, cfg)


@pytest.mark.parametrize("name", ["glides", "small"])
def test_yin_against_the_float64_reference(name):
    signals, cfg, ref, tol, stable, (f0, aper, power, cm) = case(name)
    va, inv = ref["valid"], ~ref["valid"]
    print(f"{name}: tolerances {tol}")
    for a in (f0, aper, power, cm):
        assert np.isfinite(a).all()                         # everything written, nothing read at or behind n[b] (NaN there)
    # invalid frames, exactly - every t >= 1 + n[b] / hop among them
    assert va.sum() > 0 and inv.sum() > 0
    assert (f0[inv] == 0).all() and (aper[inv] == 1).all() and (power[inv] == 0).all() and (cm[inv] == 1).all()
    assert (power[va & (ref["power"] > 0)] > 0).all() and (power[va & (ref["power"] == 0)] == 0).all()
    # the stability cap
    n_unstable = int((va & ~stable).sum())
    print(f"{name}: {va.sum()} valid frames, {n_unstable} unstable, {ref['voiced'].sum()} voiced")
    assert n_unstable <= 0.05 * va.sum()
    # the kernel's pick, recovered from its own cmnd by the rule: aper is that entry bit for bit, f0 lies within one lag of it
    tau = np.zeros(va.shape, np.int64)
    for b, t in zip(*np.nonzero(va)):
        tau[b, t] = R.pick(cm[b, t], cfg["tau_min"], cfg["tau_max"], cfg["thr"])
        assert aper[b, t] == cm[b, t, tau[b, t]]
        if f0[b, t] > 0:
            assert abs(cfg["sr"] / f0[b, t] - tau[b, t]) <= 1 + 1e-4
            assert aper[b, t] < np.float32(cfg["vthr"]) and power[b, t] > np.float32(cfg["power_floor"])
    st = va & stable
    assert (tau[st] == ref["tau"][st]).all()
    assert ((f0 > 0)[st] == ref["voiced"][st]).all()
    # values
    dev_cm = np.max(np.abs(cm[va] - ref["cm"][va]))
    dev_ap = np.max(np.abs(aper[st] - ref["aper"][st]))
    pw = va & (ref["power"] > 0)
    dev_pw = np.max(np.abs(power[pw] - ref["power"][pw]) / ref["power"][pw])
    v = st & ref["voiced"]
    dev_f0 = np.max(np.abs(f0[v] - ref["f0"][v]) / ref["f0"][v])
    print(f"{name}: GPU deviations cm {dev_cm:.3e} aper {dev_ap:.3e} power {dev_pw:.3e} f0 {dev_f0:.3e} ({v.sum()} voiced stable)")
    assert v.sum() >= 10
    assert dev_cm <= tol["cm"] and dev_ap <= tol["aper"] and dev_pw <= tol["power"] and dev_f0 <= tol["f0"]


@pytest.mark.parametrize("name", ["glides", "small"])
def test_yin_is_reproducible_and_cmnd_is_optional(name):
    signals, cfg, _, _, _, first = case(name)
    again = run_yin(signals, cfg)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    f0, aper, power, cm = run_yin(signals, cfg, with_cmnd=False, pad=0)         # ld_wav == n_max, no cmnd
    assert cm is None
    for a, b in zip(first[:3], (f0, aper, power)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("thr", [0.1, 0.0])
def test_yin_pulse_train_exact_ties_across_lanes_and_waves(thr):
    """One valid frame of a pulse train of exact period 100 at the default geometry (lags 44 .. 366 searched): the difference function,
    and so cmnd, is exactly 0 at lags 100, 200 and 300 - candidates of wave 0, of wave 2 and of wave 0's second round of the 256-thread
    pick.  thr = 0.1 takes the "first under the threshold" path, thr = 0 the argmin path: both must give the lowest, lag 100."""
    x = np.zeros(1500, np.float32)                          # frames 0 .. 5; only t = 3 (samples 73 .. 1463) lies inside the row
    x[::100] = 0.5
    cfg = dict(DEFAULT, thr=thr)
    ref, tol = R.tolerances([x], **cfg)
    f0, aper, power, cm = run_yin([x], cfg)
    assert ref["valid"][0].tolist() == [False, False, False, True, False, False] and ref["tau"][0, 3] == 100 and ref["voiced"][0, 3]
    assert [c for c in range(44, 367) if cm[0, 3, c] == 0] == [100, 200, 300] and (cm[0, 3, 44:367] >= 0).all()
    assert R.pick(cm[0, 3], 44, 367, thr) == 100 and aper[0, 3] == 0
    print(f"thr {thr}: f0 {f0[0, 3]!r}, reference {ref['f0'][0, 3]!r}, tolerance {tol['f0']:.3e}")
    assert abs(f0[0, 3] - ref["f0"][0, 3]) <= tol["f0"] * ref["f0"][0, 3]
    assert abs(cfg["sr"] / f0[0, 3] - 100) <= 1 + 1e-4
    inv = ~ref["valid"][0]
    assert (f0[0, inv] == 0).all() and (aper[0, inv] == 1).all() and (power[0, inv] == 0).all()


def test_yin_bad_arguments_return_the_code_without_a_launch():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wav = torch.zeros(2, 3000, device=dev)
    n = torch.tensor([3000, 2000], dtype=torch.int64, device=dev)
    T = 1 + 3000 // 256
    outs = [torch.full((2, T), -7.0, device=dev) for _ in range(3)] + [torch.full((2, T, 368), -7.0, device=dev)]

    def rc(cfg=DEFAULT, n_max=3000, **over):
        s = _yin_struct(wav, n, dict(cfg), n_max, outs, ld_wav=over.pop("ld_wav", None))
        for k, v in over.items():
            setattr(s, k, v)
        return lib.t2_yin(C.addressof(s), None)

    for field in ("wav", "n", "f0", "aper", "power"):
        assert rc(**{field: None}) == 1, field
        assert b"t2_yin" in lib.t2_last_error()
    assert rc(B=0) == 1 and rc(B=-1) == 1 and rc(B=65536) == 1
    assert rc(hop=0) == 1 and rc(sr=0) == 1 and rc(n_max=-1) == 1
    assert rc(W=15) == 1
    assert rc(tau_min=1) == 1
    assert rc(tau_min=44, tau_max=45) == 1 and rc(tau_min=44, tau_max=44) == 1
    assert rc(W=4096 - 367 + 1) == 1                        # S = T2_YIN_MAX_SPAN + 1
    assert rc(ld_wav=2999) == 1
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)      # nothing ran
    assert rc() == 0 and rc(cmnd=None) == 0                # the same block, unchanged, is accepted
    torch.cuda.synchronize()
    assert all(bool((o != -7.0).all()) for o in outs)


# --------------------------------------------------------------------------------------------------------------------------------
# t2_prosody_stats
# --------------------------------------------------------------------------------------------------------------------------------
def run_stats(f0, aper, power, n, hop, S):
    from tacotron2_amd import _lib
    dev = torch.device("cuda:0")
    B, T = f0.shape
    out = torch.full((B, 8), -7.0, device=dev)
    s = _lib.make("T2ProsodyStats", f0=torch.from_numpy(f0).to(dev), aper=torch.from_numpy(aper).to(dev),
                  power=torch.from_numpy(power).to(dev), n=torch.tensor(n, dtype=torch.int64, device=dev), B=B, T=T, hop=hop, S=S, out=out)
    _lib.call("t2_prosody_stats", s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _valid(T, n, hop, S):
    s0 = np.arange(T) * hop - S // 2
    return (s0 >= 0) & (s0 + S <= n)


def _check_stats(got, f0, aper, power, n, hop, S):
    for b in range(f0.shape[0]):
        want = R.stats(f0[b], aper[b], power[b], _valid(f0.shape[1], n[b], hop, S))
        assert got[b, 0] == want[0] and got[b, 1] == want[1] and got[b, 7] == 0, (b, got[b], want)
        if want[1] == 0:
            assert np.isnan(got[b, 2:7]).all(), (b, got[b])
            continue
        assert got[b, 3] == np.float32(want[3]) and got[b, 4] == np.float32(want[4]), (b, got[b], want)
        for k in (2, 5, 6):
            assert abs(got[b, k] - want[k]) <= 1e-6 * abs(want[k]), (b, k, got[b, k], want[k])


def test_prosody_stats_hand_made_tracks():
    """T = 4096 (the cap), four utterances in one launch: many ties, one voiced frame, none, and a short one whose invalid frames hold
    NaN and large values that must not count."""
    rng = np.random.default_rng(11)
    T, hop, S = 4096, 256, 1391
    f0 = rng.choice(np.array([0, 0, 90.5, 120.25, 120.25, 200, 333.3, 410], np.float32), size=(4, T))
    aper = rng.uniform(0.01, 0.3, size=(4, T)).astype(np.float32)
    power = (10.0 ** rng.uniform(-4, -1, size=(4, T))).astype(np.float32)
    n = [4095 * hop + 700, 3000 * hop, 2000 * hop, 40 * hop]
    f0[1] = 0
    f0[1, 1234] = 151.0                                     # one voiced frame: both percentiles are it
    f0[2] = 0                                               # none
    inv3 = ~_valid(T, n[3], hop, S)
    f0[3, inv3] = np.where(rng.random(inv3.sum()) < 0.5, np.nan, 9999.0).astype(np.float32)
    aper[3, inv3] = np.nan
    power[3, inv3] = np.nan
    got = run_stats(f0, aper, power, n, hop, S)
    print(got)
    _check_stats(got, np.nan_to_num(f0, nan=0.0), aper, power, n, hop, S)
    assert got[0, 0] == _valid(T, n[0], hop, S).sum() > 4000 and got[1, 1] == 1 and got[1, 3] == got[1, 4] == 151.0
    assert got[3, 0] == 35 and 0 < got[3, 1] <= 35 and got[3, 4] <= 410


def test_prosody_stats_small_and_ties_by_index():
    """T = 7, all frames valid (S = 1): the track (100, 100, 100, 200, 300) plus unvoiced frames - p5 is index 0 and p95 index 4 of
    the sorted voiced values, whichever of the equal 100s ranks first."""
    f0 = np.array([[0, 100, 300, 100, 0, 200, 100]], np.float32)
    aper = np.full((1, 7), 0.125, np.float32)
    power = np.full((1, 7), 1e-2, np.float32)
    got = run_stats(f0, aper, power, [7], 1, 1)
    _check_stats(got, f0, aper, power, [7], 1, 1)
    assert got[0].tolist()[:2] == [7.0, 5.0] and got[0, 3] == 100 and got[0, 4] == 300 and got[0, 6] == 0.125
    assert abs(got[0, 5] + 20.0) < 1e-5


EDGE_LENGTHS = [1, 63, 64, 65, 255, 256, 257]       # a lane, a wave or the block's second round is empty or holds one frame


@pytest.mark.parametrize("T", EDGE_LENGTHS)
def test_prosody_stats_at_the_wave_and_block_edges(T):
    """B = 2, hop = S = 1 (every frame inside n is valid): the first utterance has all T frames, the second n = 0 - no valid frame,
    NaN in its inputs.  Counts exact, sums within the bound of the hand-made tracks."""
    rng = np.random.default_rng(100 + T)
    f0 = rng.choice(np.array([0, 90.5, 120.25, 200, 333.3, 410], np.float32), size=(2, T))
    f0[0, T - 1] = 151.0                                    # the last frame is voiced: a sum that drops it is wrong
    aper = rng.uniform(0.01, 0.3, size=(2, T)).astype(np.float32)
    power = (10.0 ** rng.uniform(-4, -1, size=(2, T))).astype(np.float32)
    f0[1], aper[1], power[1] = np.nan, np.nan, np.nan
    got = run_stats(f0, aper, power, [T, 0], 1, 1)
    _check_stats(got, np.nan_to_num(f0, nan=0.0), aper, power, [T, 0], 1, 1)
    assert got[0, 0] == T and 1 <= got[0, 1] <= T and got[1, 0] == 0 and got[1, 1] == 0


def test_prosody_stats_bad_arguments():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    x = torch.zeros(1, 8, device=dev)
    n = torch.tensor([8], dtype=torch.int64, device=dev)
    out = torch.full((1, 8), -7.0, device=dev)
    base = dict(f0=x, aper=x, power=x, n=n, B=1, T=8, hop=1, S=1, out=out)
    for over in [dict(f0=None), dict(aper=None), dict(power=None), dict(n=None), dict(out=None), dict(B=0), dict(T=0), dict(T=4097),
                 dict(hop=0), dict(S=0)]:
        s = _lib.make("T2ProsodyStats", **dict(base, **over))
        assert lib.t2_prosody_stats(C.addressof(s), None) == 1, over
        assert b"t2_prosody_stats" in lib.t2_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# --------------------------------------------------------------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------------------------------------------------------------
def test_engine_yin_checks_its_arguments():
    from tacotron2_amd import engine
    dev = torch.device("cuda:0")
    wav = torch.zeros(2, 3000, device=dev)
    n = torch.tensor([3000, 10], device=dev)
    f0, aper, power = engine.yin(wav, n)
    assert f0.shape == aper.shape == power.shape == (2, 12) and not f0.any() and bool((aper == 1).all())       # silence: unvoiced
    for bad in [dict(wav=wav.cpu()), dict(wav=wav.double()), dict(wav=wav[0]), dict(n=n.cpu()), dict(n=n.float()), dict(n=n[:1]),
                dict(W=8), dict(W=4000), dict(hop=0), dict(fmin=600.0), dict(fmax=22050.0), dict(n_max=3001), dict(thr=float("nan")),
                dict(wav=wav[:, ::2])]:
        kw = dict(dict(wav=wav, n=n), **bad)
        with pytest.raises(ValueError) as e:
            engine.yin(**kw)
        assert str(e.value).startswith("yin:"), bad
    with pytest.raises(ValueError, match="T2_YIN_MAX_SPAN"):
        engine.yin(wav, n, W=4000)
    with pytest.raises(ValueError, match="T2_PROSODY_MAX_T"):
        engine.prosody_stats(torch.zeros(1, 4097, device=dev), torch.zeros(1, 4097, device=dev), torch.zeros(1, 4097, device=dev),
                             torch.tensor([5], device=dev))
    with pytest.raises(ValueError, match="prosody_stats:"):
        engine.prosody_stats(f0, aper.cpu(), power, n)


def test_prosody_meter_on_tones():
    """Pitch and amplitude set per utterance: the measures order the utterances, and match the float64 reference through the tolerances
    of these inputs (a relative f0 tolerance is an absolute one on ln f0, a relative power tolerance 10 / ln 10 times that in dB; plus the
    rounding of the kernel's float32 output row).  An empty waveform and one shorter than a span measure nothing."""
    from tacotron2_amd.prosody import MEASURES, ProsodyMeter
    dev = torch.device("cuda:0")
    spec = [(110.0, 0.1, 8000, 10), (180.0, 0.2, 12000, 30), (260.0, 0.4, 6000, 50)]
    signals = [R.tone(f, n, amp=a) for f, a, n, _ in spec] + [np.zeros(0, np.float32), R.tone(200.0, 1000)]
    chars = [c for *_, c in spec] + [5, 7]
    meter = ProsodyMeter(22050, dev)
    assert meter.describe() == dict(sr=22050, hop=256, W=1024, fmin=60.0, fmax=500.0, thr=0.1, vthr=0.3, power_floor=1e-10, tau_min=44,
                                    tau_max=367)
    got = meter.measure([torch.from_numpy(s).to(dev) for s in signals], chars)
    assert meter.measure([], []) == []
    ref, tol = R.tolerances(signals, **DEFAULT)
    print("tolerances", tol, "\n", got)
    eps = 2.0 ** -23
    for k, (f, a, n, c) in enumerate(spec):
        want = R.stats(ref["f0"][k], ref["aper"][k], ref["power"][k], ref["valid"][k])
        g = got[k]
        assert set(g) == {"n_frames", "n_voiced"} | set(MEASURES)
        assert g["n_frames"] == want[0] == ref["valid"][k].sum() and g["n_voiced"] == want[1] == g["n_frames"]
        assert abs(g["pitch_mean_log"] - want[2]) <= tol["f0"] + eps * abs(want[2])
        assert abs(g["pitch_mean_log"] - math.log(f)) < 5e-4
        assert abs(g["pitch_range_log"] - (math.log(want[4]) - math.log(want[3]))) <= 2 * tol["f0"] + 2 * eps
        assert abs(g["intensity_mean_db"] - want[5]) <= 10 / math.log(10) * tol["power"] + eps * abs(want[5])
        assert abs(g["aperiodicity_mean"] - want[6]) <= tol["aper"] + eps
        assert g["rate"] == c / (n / 22050)
    for key in ("pitch_mean_log", "intensity_mean_db", "rate"):
        assert got[0][key] < got[1][key] < got[2][key], key
    assert got[3] == dict(n_frames=0, n_voiced=0, pitch_mean_log=None, pitch_range_log=None, intensity_mean_db=None,
                          aperiodicity_mean=None, rate=None)
    assert got[4]["n_frames"] == 0 and got[4]["pitch_mean_log"] is None and got[4]["rate"] == 7 / (1000 / 22050)
    with pytest.raises(ValueError):
        meter.measure([torch.zeros(10)], [1])               # a host tensor
    with pytest.raises(ValueError):
        ProsodyMeter(22050, dev, window=3)
