"""t2_pitch_viterbi and t2_f0_path_stats on the GPU through the C ABI against the float64 restatement tests/pitch_ref.py ON IDENTICAL
float32 INPUTS (the test hands the cmnd to the kernel, so nothing depends on t2_yin's rounding), then the engine functions.

Viterbi: lag equal everywhere; cost and aper bit-identical (the recurrence has additions only, in the header's association); f0 within
8 x the deviation of the float32 restatement of the interpolation formula from the float64 one on the test's own input (the scheme of
prosody_ref.tolerances).  Path statistics: counts equal, every sum within 4 (P + 8) 2^-52 sum |term| - the bound of an fp64 sum of P
terms in any order, plus the device log2's last bits.  The measured deviations are printed and quoted in DESIGN 5.11."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pitch_ref as P
import prosody_ref as R

pytestmark = pytest.mark.gpu
DEFAULT = dict(R.DEFAULTS)
SMALL = dict(sr=8000, hop=64, W=80, tau_min=10, tau_max=100, thr=0.1, vthr=0.3, power_floor=1e-10)     # 90 lags + U: no multiple of 64
VIT = dict(P.DEFAULTS)


def _struct(cm, power, lens, lw, cfg, vit, outs, back, over=None):
    from tacotron2_amd import _lib
    f0, aper, lag, cost = outs
    kw = dict(cmnd=cm, ld_b=cm.stride(0), ld_t=cm.stride(1), power=power, len=lens, lw=lw, B=cm.shape[0], T=cm.shape[1], sr=cfg["sr"],
              tau_min=cfg["tau_min"], tau_max=cfg["tau_max"], power_floor=cfg["power_floor"], trans_max=vit["w"] * vit["max_jump"],
              u=vit["u"], c_sw=vit["c_sw"], f0=f0, aper=aper, lag=lag, cost=cost, back=back)
    kw.update(over or {})
    return _lib.make("T2PitchViterbi", **kw)


def run_viterbi(cm, power, lens, cfg, vit, pad_t=0, pad_b=0):
    """One t2_pitch_viterbi call; outputs pre-filled with NaN / -7.  pad_t, pad_b: extra floats behind every row / utterance of cmnd
    (a strided view into a larger NaN-filled buffer)."""
    from tacotron2_amd import _lib
    dev = torch.device("cuda:0")
    B, T, NT = cm.shape
    N = cfg["tau_max"] - cfg["tau_min"]
    if pad_t or pad_b:
        ld_t = NT + pad_t
        ld_b = T * ld_t + pad_b
        buf = torch.full((B * ld_b,), float("nan"), dtype=torch.float32)
        view = buf.as_strided((B, T, NT), (ld_b, ld_t, 1))
        view.copy_(torch.from_numpy(cm))
        cm_d = buf.to(dev).as_strided((B, T, NT), (ld_b, ld_t, 1))
    else:
        cm_d = torch.from_numpy(cm).to(dev)
    lw = torch.from_numpy(P.lag_weights(cfg["tau_min"], cfg["tau_max"], vit["w"])).to(dev)
    outs = [torch.full((B, T), float("nan"), device=dev), torch.full((B, T), float("nan"), device=dev),
            torch.full((B, T), -7, dtype=torch.int32, device=dev), torch.full((B,), float("nan"), dtype=torch.float64, device=dev)]
    back = torch.zeros(B, T, N + 1, dtype=torch.int16, device=dev)
    s = _struct(cm_d, torch.from_numpy(power).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), lw, cfg, vit, outs, back)
    _lib.call("t2_pitch_viterbi", s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def reference(cm, power, lens, cfg, vit):
    T = cm.shape[1]
    lw = P.lag_weights(cfg["tau_min"], cfg["tau_max"], vit["w"])
    clean = np.nan_to_num(cm, nan=7.0)                   # (the reference is never to read behind len either; NaN would hide a slip)
    return [P.viterbi_fast(clean[b], np.nan_to_num(power[b], nan=7.0), min(max(int(lens[b]), 0), T), cfg["tau_min"], cfg["tau_max"], lw,
                           vit["w"] * vit["max_jump"], vit["u"], vit["c_sw"], cfg["power_floor"], cfg["sr"]) for b in range(cm.shape[0])]


def check(name, got, want, min_voiced=0):
    f0, aper, lag, cost = got
    assert np.isfinite(f0).all() and np.isfinite(aper).all() and np.isfinite(cost).all() and (lag >= 0).all()       # all written
    dev_f0, tol_f0, voiced = 0.0, 0.0, 0
    for b, w in enumerate(want):
        assert np.array_equal(lag[b], w["lag"]), (name, b, lag[b], w["lag"])
        assert cost[b].tobytes() == np.float64(w["cost"]).tobytes(), (name, b, cost[b], w["cost"])
        assert aper[b].tobytes() == w["aper"].tobytes(), (name, b)
        v = w["lag"] > 0
        assert (f0[b][~v] == 0).all() and (aper[b][~v] == 1).all()
        if v.any():
            voiced += int(v.sum())
            tol_f0 = max(tol_f0, 8.0 * float(np.max(np.abs(w["f0_32"][v] - w["f0"][v]) / w["f0"][v])))
            dev_f0 = max(dev_f0, float(np.max(np.abs(f0[b][v] - w["f0"][v]) / w["f0"][v])))
    print(f"[pitch_viterbi] {name}: {voiced} voiced frames, f0 deviation {dev_f0:.3e} (tolerance {tol_f0:.3e}), costs {cost.tolist()}")
    assert voiced >= min_voiced and dev_f0 <= tol_f0
    return voiced


def random_case(seed, B, T, tau_min, tau_max, quant=None):
    rng = np.random.default_rng(seed)
    cm = rng.random((B, T, tau_max + 1)).astype(np.float32)
    if quant:
        cm = (rng.integers(0, quant + 1, size=cm.shape) / quant).astype(np.float32)
    cm[:, :, 0] = 1.0
    return cm, np.ones((B, T), np.float32), dict(sr=22050, tau_min=tau_min, tau_max=tau_max, power_floor=1e-10)


@functools.lru_cache(maxsize=None)
def signal_case(name):
    """(cmnd float32, power float32, len) from the float64 YIN reference of the test signals, computed once."""
    if name == "small":
        rng = np.random.default_rng(5)
        t = np.arange(2500)
        x = 0.3 * np.sin(2 * np.pi * t / 37.3) + 0.1 * np.sin(4 * np.pi * t / 37.3) + 0.003 * rng.normal(size=2500)
        x[600:800] = 0.05 * rng.normal(size=200)
        x[800:1000] = 0.0
        signals, cfg = [x.astype(np.float32)], SMALL
    else:
        signals, cfg = [P.octave_signal(), R.glides()[4]], DEFAULT       # 16000 samples each: 63 frames
    ref = R.yin(signals, **cfg)
    cm, power = ref["cm"].astype(np.float32), ref["power"].astype(np.float32)
    lens = [1 + len(s) // cfg["hop"] for s in signals]
    if name != "small":
        lens[1] = 50                                     # the glide is decoded up to frame 50 only
    for b, n in enumerate(lens):                         # NaN behind every len[b]: nothing there may be read
        cm[b, n:] = np.nan
        power[b, n:] = np.nan
    return cm, power, lens, cfg, ref


def test_small_configuration_91_states():
    cm, power, lens, cfg, _ = signal_case("small")
    assert cm.shape == (1, 40, 101)
    want = reference(cm, power, lens, cfg, VIT)
    check("small", run_viterbi(cm, power, lens, cfg, VIT), want, min_voiced=10)
    assert (want[0]["lag"] == 0).any()                   # the noise and the silence are unvoiced


def test_defaults_octave_signal_and_glide_with_different_lengths():
    cm, power, lens, cfg, ref = signal_case("default")
    assert cm.shape == (2, 63, 368) and lens == [63, 50] and np.isnan(cm[1, 50:]).all() and np.isnan(power[1, 50:]).all()
    assert (power[1, :50] == 0).any()                    # the glide's digital silence: frames of exactly zero power
    want = reference(cm, power, lens, cfg, VIT)
    got = run_viterbi(cm, power, lens, cfg, VIT)
    check("defaults", got, want, min_voiced=70)
    f0 = got[0]
    v = f0[0] > 0
    raw = ref["f0"][0]
    off = lambda f: np.abs(np.log2(f / 110.0)) > 0.5
    assert v.sum() == 57 and off(f0[0][v]).sum() == 0 and off(raw[ref["voiced"][0]]).sum() >= 3       # the octave errors are gone
    assert (f0[1, 50:] == 0).all() and (got[1][1, 50:] == 1).all() and (got[2][1, 50:] == 0).all()


@pytest.mark.parametrize("N", [512, 513, 600, 4096])
def test_random_cmnd_on_both_kernel_instances(N):
    """N = 512 is the last size of the two-targets-per-thread instance, 513 the first of the other; 4096 is T2_PITCH_MAX_STATES (98 320
    bytes of LDS, behind the 64 KB a kernel gets without asking)."""
    T = 8 if N <= 600 else 3
    cm, power, cfg = random_case(N, 1, T, 20, 20 + N)
    vit = dict(VIT, u=0.05, c_sw=0.02)                   # random cmnd: cheap enough that voiced and unvoiced stretches both occur
    want = reference(cm, power, [T], cfg, vit)
    check(f"random N={N}", run_viterbi(cm, power, [T], cfg, vit), want, min_voiced=1)


def test_ties_only_the_order_rule_decides():
    """w = 0 and cmnd in eighths: every transition is free and allowed, sums are exact, whole families of paths tie."""
    cm, power, cfg = random_case(4, 2, 12, 44, 367, quant=8)
    cm[1] = 0.25                                          # one utterance where EVERYTHING ties: lag 44 throughout
    vit = dict(w=0.0, max_jump=0.25, u=0.25, c_sw=0.125)
    want = reference(cm, power, [12, 12], cfg, vit)
    got = run_viterbi(cm, power, [12, 12], cfg, vit)
    check("ties", got, want, min_voiced=12)
    assert (got[2][1] == 44).all() and got[3][1] == 3.0
    vit = dict(w=0.0, max_jump=0.25, u=0.125, c_sw=0.0)   # U ties with the best voiced state wherever that is 1/8
    check("ties with U", run_viterbi(cm, power, [12, 12], cfg, vit), reference(cm, power, [12, 12], cfg, vit))


def test_one_frame_silence_and_empty_utterances():
    cm, power, cfg = random_case(6, 4, 5, 44, 367)
    cm[:, :, 44:367] *= 0.2
    check("T=1", run_viterbi(cm[:, :1].copy(), power[:, :1].copy(), [1, 1, 1, 1], cfg, VIT),
          reference(cm[:, :1], power[:, :1], [1, 1, 1, 1], cfg, VIT), min_voiced=4)
    power[1] = 0.0                                        # an all-silent utterance
    power[2, 2] = 1e-10                                   # at the floor: not above it
    lens = [5, 5, 5, 0]
    cm[3], power[3] = np.nan, np.nan                      # len = 0: nothing is read
    want = reference(cm, power, lens, cfg, VIT)
    got = run_viterbi(cm, power, lens, cfg, VIT)
    check("silence", got, want, min_voiced=9)
    assert (got[2][1] == 0).all() and got[3][1] == 5 * VIT["u"] and got[2][2, 2] == 0
    assert (got[2][3] == 0).all() and got[3][3] == 0.0 and (got[1][3] == 1).all()
    lens = [7, -3, 2, 5]                                  # clipped to 0 .. T
    cm[3], power[3] = cm[0], power[0]
    got = run_viterbi(cm, power, lens, cfg, VIT)
    check("clipped len", got, reference(cm, power, lens, cfg, VIT))
    assert np.array_equal(got[2][3], got[2][0]) and (got[2][1] == 0).all() and (got[2][2, 2:] == 0).all()


def test_strided_cmnd_and_reproducibility():
    cm, power, lens, cfg, _ = signal_case("default")
    first = run_viterbi(cm, power, lens, cfg, VIT)
    again = run_viterbi(cm, power, lens, cfg, VIT)
    strided = run_viterbi(cm, power, lens, cfg, VIT, pad_t=5, pad_b=11)
    for a, b, c in zip(first, again, strided):
        assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes()


def test_viterbi_bad_arguments_return_the_code_without_a_launch():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    cfg = dict(sr=22050, tau_min=44, tau_max=367, power_floor=1e-10)
    B, T, NT = 2, 6, 368
    cm = torch.full((B, T, NT), 0.5, device=dev)
    power = torch.ones(B, T, device=dev)
    lens = torch.tensor([6, 4], dtype=torch.int32, device=dev)
    lw = torch.from_numpy(P.lag_weights(44, 367, 1.0)).to(dev)
    outs = [torch.full((B, T), -7.0, device=dev), torch.full((B, T), -7.0, device=dev),
            torch.full((B, T), -7, dtype=torch.int32, device=dev), torch.full((B,), -7.0, dtype=torch.float64, device=dev)]
    back = torch.zeros(B, T, 324, dtype=torch.int16, device=dev)

    def rc(**over):
        s = _struct(cm, power, lens, lw, cfg, VIT, outs, back, over)
        return lib.t2_pitch_viterbi(C.addressof(s), None)

    for field in ("cmnd", "power", "len", "lw", "f0", "aper", "lag", "cost", "back"):
        assert rc(**{field: None}) == 1, field
        assert b"t2_pitch_viterbi" in lib.t2_last_error()
    assert rc(B=0) == 1 and rc(B=65536) == 1 and rc(T=0) == 1 and rc(T=4097) == 1 and rc(sr=0) == 1
    assert rc(tau_min=1) == 1 and rc(tau_max=45) == 1 and rc(tau_max=44) == 1
    assert rc(tau_min=2, tau_max=4099, ld_t=5000, ld_b=50000) == 1                      # 4097 lags: above T2_PITCH_MAX_STATES
    assert rc(ld_t=367) == 1 and rc(ld_b=5 * 368 + 367) == 1
    nan, inf = float("nan"), float("inf")
    for field in ("trans_max", "u", "c_sw"):
        assert rc(**{field: nan}) == 1 and rc(**{field: inf}) == 1 and rc(**{field: -0.5}) == 1, field
    assert rc(power_floor=nan) == 1
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs)       # nothing ran
    assert rc() == 0                                      # the same block, unchanged, is accepted
    torch.cuda.synchronize()
    assert all(bool((o != -7).all()) for o in outs)


# --------------------------------------------------------------------------------------------------------------------------------
# t2_f0_path_stats
# --------------------------------------------------------------------------------------------------------------------------------
def run_stats(path, path_len, f0_a, n_a, f0_b, n_b, hop, S):
    from tacotron2_amd import _lib
    dev = torch.device("cuda:0")
    B, Pn, _ = path.shape
    out = torch.full((B, 12), -7.0, dtype=torch.float64, device=dev)
    s = _lib.make("T2F0PathStats", path=torch.from_numpy(path).to(dev), path_len=torch.tensor(path_len, dtype=torch.int32, device=dev),
                  f0_a=torch.from_numpy(f0_a).to(dev), f0_b=torch.from_numpy(f0_b).to(dev),
                  n_a=torch.tensor(n_a, dtype=torch.int64, device=dev), n_b=torch.tensor(n_b, dtype=torch.int64, device=dev), B=B, P=Pn,
                  Ta=f0_a.shape[1], Tb=f0_b.shape[1], hop=hop, S=S, out=out)
    _lib.call("t2_f0_path_stats", s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_stats(name, got, path, path_len, f0_a, n_a, f0_b, n_b, hop, S):
    worst = 0.0
    for b in range(path.shape[0]):
        n = min(max(int(path_len[b]), 0), path.shape[1])
        row, mag = P.f0_path_stats(path[b], n, np.nan_to_num(f0_a[b], nan=0.0), n_a[b], np.nan_to_num(f0_b[b], nan=0.0), n_b[b], hop, S)
        assert got[b, :4].tolist() == row[:4].tolist() and got[b, 11] == 0, (name, b, got[b], row)
        bound = 4 * (path.shape[1] + 8) * 2.0 ** -52 * mag[4:11]
        err = np.abs(got[b, 4:11] - row[4:11])
        assert (err <= bound).all(), (name, b, err, bound)
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"[f0_path_stats] {name}: worst error / bound = {worst:.3e}")


def test_stats_along_a_path_of_the_dtw_kernel():
    from tacotron2_amd.model import Tacotron2
    dev = torch.device("cuda:0")
    eng = Tacotron2(num_chars=39, encoded_dim=64, encoder_kernel_size=5, num_mels=80, prenet_dim=32, att_rnn_dim=64, att_dim=32,
                    rnn_hidden_dim=64, postnet_dim=64, dropout=0.5, device=dev, seed=11)._engine
    rng = np.random.default_rng(8)
    a, b = rng.normal(size=(1, 9, 3)).astype(np.float32), rng.normal(size=(1, 7, 3)).astype(np.float32)
    _, plen, path = eng.dtw(torch.from_numpy(a).to(dev), torch.tensor([9], device=dev), torch.from_numpy(b).to(dev),
                            torch.tensor([7], device=dev), return_path=True)
    path, plen = path.cpu().numpy(), plen.cpu().tolist()
    assert path.shape == (1, 15, 2) and 9 <= plen[0] <= 15
    f0_a = rng.choice(np.array([98.5, 131.25, 220, 402.7], np.float32), size=(1, 9))
    f0_b = rng.choice(np.array([101.5, 120.25, 233, 390.1], np.float32), size=(1, 7))
    f0_a[0, 1], f0_b[0, 5] = 0.0, 0.0                    # one unvoiced frame on each side
    got = run_stats(path, plen, f0_a, [9], f0_b, [7], 1, 1)          # hop = S = 1: every frame inside n is valid
    print(got)
    check_stats("dtw path", got, path, plen, f0_a, [9], f0_b, [7], 1, 1)
    assert got[0, 0] == plen[0] and got[0, 1] >= 1 and got[0, 2] + got[0, 3] >= 1


def test_stats_hand_made_paths_batch_of_three():
    """B = 3: cells outside the tracks and at invalid edges (NaN in the tracks there: they are not read), a long path that more than
    one pass of the block strides over, and path_len = 0."""
    rng = np.random.default_rng(12)
    hop, S, Ta, Tb, Pn = 4, 6, 40, 30, 700
    n_a, n_b = [4 * 35 + 3, 4 * 39 + 3, 50], [4 * 29 + 3, 4 * 20, 50]
    f0_a = rng.uniform(70, 450, size=(3, Ta)).astype(np.float32)
    f0_b = rng.uniform(70, 450, size=(3, Tb)).astype(np.float32)
    f0_a[rng.random((3, Ta)) < 0.3] = 0
    f0_b[rng.random((3, Tb)) < 0.3] = 0
    for b in range(3):                                    # NaN at every invalid frame
        for t in range(Ta):
            if not P.frame_valid(t, n_a[b], hop, S, Ta):
                f0_a[b, t] = np.nan
        for t in range(Tb):
            if not P.frame_valid(t, n_b[b], hop, S, Tb):
                f0_b[b, t] = np.nan
    path = np.stack([rng.integers(-2, Ta + 3, size=(3, Pn)), rng.integers(-2, Tb + 3, size=(3, Pn))], axis=-1).astype(np.int32)
    path_len = [Pn, 300, 0]
    path[2] = 2 ** 30                                     # path_len = 0: nothing is read
    got = run_stats(path, path_len, f0_a, n_a, f0_b, n_b, hop, S)
    check_stats("hand-made", got, path, path_len, f0_a, n_a, f0_b, n_b, hop, S)
    assert got[0, 0] > 256 and got[0, 1] > 50 and got[0, 2] > 0 and got[0, 3] > 0 and 0 < got[0, 0] < Pn
    assert not got[2].any()
    got = run_stats(path[:2], [Pn + 50, -4], f0_a[:2], n_a[:2], f0_b[:2], n_b[:2], hop, S)          # clipped to 0 .. P
    check_stats("clipped", got, path[:2], [Pn, 0], f0_a[:2], n_a[:2], f0_b[:2], n_b[:2], hop, S)


@pytest.mark.parametrize("Pn", [1, 63, 64, 65, 255, 256, 257])
def test_stats_at_the_wave_and_block_edges(Pn):
    """Path lengths at which a lane, a wave or the second round of the 256-thread block is empty or holds one cell.  B = 2, hop = S = 1
    (every frame inside n is valid): the first pair scores all Pn cells, the second has n = 0 on both sides - no valid frame, NaN in
    its tracks - and scores none."""
    rng = np.random.default_rng(300 + Pn)
    Ta, Tb = 40, 30
    f0_a = rng.choice(np.array([0, 98.5, 131.25, 220, 402.7], np.float32), size=(2, Ta))
    f0_b = rng.choice(np.array([0, 101.5, 120.25, 233, 390.1], np.float32), size=(2, Tb))
    path = np.stack([rng.integers(0, Ta, size=(2, Pn)), rng.integers(0, Tb, size=(2, Pn))], axis=-1).astype(np.int32)
    f0_a[0, path[0, Pn - 1, 0]], f0_b[0, path[0, Pn - 1, 1]] = 220.0, 233.0            # the last cell is voiced on both sides
    f0_a[1], f0_b[1] = np.nan, np.nan
    got = run_stats(path, [Pn, Pn], f0_a, [Ta, 0], f0_b, [Tb, 0], 1, 1)
    check_stats(f"edge P={Pn}", got, path, [Pn, Pn], f0_a, [Ta, 0], f0_b, [Tb, 0], 1, 1)
    assert got[0, 0] == Pn and got[0, 1] >= 1 and not got[1].any()


def test_stats_bad_arguments():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    path = torch.zeros(1, 4, 2, dtype=torch.int32, device=dev)
    pl = torch.tensor([4], dtype=torch.int32, device=dev)
    f = torch.ones(1, 5, device=dev)
    n = torch.tensor([5], dtype=torch.int64, device=dev)
    out = torch.full((1, 12), -7.0, dtype=torch.float64, device=dev)
    base = dict(path=path, path_len=pl, f0_a=f, f0_b=f, n_a=n, n_b=n, B=1, P=4, Ta=5, Tb=5, hop=1, S=1, out=out)
    for over in [dict(path=None), dict(path_len=None), dict(f0_a=None), dict(f0_b=None), dict(n_a=None), dict(n_b=None), dict(out=None),
                 dict(B=0), dict(B=65536), dict(P=0), dict(Ta=0), dict(Tb=0), dict(hop=0), dict(S=0)]:
        s = _lib.make("T2F0PathStats", **dict(base, **over))
        assert lib.t2_f0_path_stats(C.addressof(s), None) == 1, over
        assert b"t2_f0_path_stats" in lib.t2_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# --------------------------------------------------------------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------------------------------------------------------------
def test_engine_functions_and_their_argument_checks():
    from tacotron2_amd import engine
    dev = torch.device("cuda:0")
    cm, power, lens, cfg, _ = signal_case("default")
    n = torch.tensor([16000, 50 * 256 - 1], device=dev)   # the engine decodes 1 + n // hop frames: 63 and 50
    cm_d, pw_d = torch.from_numpy(np.nan_to_num(cm, nan=1.0)).to(dev), torch.from_numpy(np.nan_to_num(power, nan=0.0)).to(dev)
    f0, aper, lag, cost = engine.pitch_viterbi(cm_d, pw_d, n)
    want = reference(cm, power, lens, cfg, VIT)
    assert f0.shape == aper.shape == lag.shape == (2, 63) and lag.dtype == torch.int32 and cost.dtype == torch.float64
    for b in range(2):                                    # (the engine builds lw with torch.log2: the lags are robust to its last bit)
        assert np.array_equal(lag[b].cpu().numpy(), want[b]["lag"])
        assert abs(float(cost[b]) - want[b]["cost"]) <= 1e-12 * want[b]["cost"]
    for bad in [dict(cmnd=cm_d.cpu()), dict(cmnd=cm_d.double()), dict(cmnd=cm_d[0]), dict(cmnd=cm_d[:, :, :300]), dict(power=pw_d.cpu()),
                dict(power=pw_d[:, :5]), dict(n=n.cpu()), dict(n=n.float()), dict(n=n[:1]), dict(hop=0), dict(fmin=600.0), dict(w=-1.0),
                dict(max_jump=float("nan")), dict(u=float("inf")), dict(c_sw=-0.1), dict(power_floor=float("nan")),
                dict(cmnd=cm_d[:, :, ::2]), dict(fmin=1.0, cmnd=torch.zeros(1, 2, 22051, device=dev), power=pw_d[:1, :2], n=n[:1])]:
        kw = dict(dict(cmnd=cm_d, power=pw_d, n=n), **bad)
        with pytest.raises(ValueError) as e:
            engine.pitch_viterbi(**kw)
        assert str(e.value).startswith("pitch_viterbi:"), (bad, str(e.value))
    path = torch.tensor([[[1, 1], [2, 1], [2, 2], [9, 9]]], dtype=torch.int32, device=dev)
    pl = torch.tensor([4], dtype=torch.int32, device=dev)
    fa, fb = torch.tensor([[0.0, 100.0, 200.0]], device=dev), torch.tensor([[0.0, 200.0, 0.0]], device=dev)
    n3 = torch.tensor([3], device=dev)
    st = engine.f0_path_stats(path, pl, fa, n3, fb, n3, hop=1, span=1)
    assert st.shape == (1, 12) and st.dtype == torch.float64 and st[0, :6].tolist() == [3.0, 2.0, 1.0, 0.0, -1200.0, 1200.0 ** 2]
    fig = engine.f0_figures(st[0].tolist())
    assert fig["f0_rmse_cents"] == pytest.approx(1200.0 / 2 ** 0.5) and fig["f0_corr"] is None and fig["vuv_error"] == 1 / 3
    for bad in [dict(path=path.cpu()), dict(path=path.long()), dict(path=path[0]), dict(path_len=pl.long()), dict(path_len=pl.cpu()),
                dict(f0_a=fa.double()), dict(f0_b=fb[0]), dict(f0_a=fa.cpu()), dict(n_a=n3.float()), dict(n_b=n3.cpu()), dict(hop=0),
                dict(span=0)]:
        kw = dict(dict(path=path, path_len=pl, f0_a=fa, n_a=n3, f0_b=fb, n_b=n3, hop=1, span=1), **bad)
        with pytest.raises(ValueError) as e:
            engine.f0_path_stats(**kw)
        assert str(e.value).startswith("f0_path_stats:"), (bad, str(e.value))


def test_engine_pitch_viterbi_of_a_cut_of_a_larger_allocation():
    """The accepted strided path of the shared check: cmnd as a view (2, 63, tau_max + 1) into a (2, 70, tau_max + 6) buffer - rows
    and utterances further apart than the view is wide, NaN between them - decodes to what the contiguous tensor gives, bit for bit."""
    from tacotron2_amd import engine
    dev = torch.device("cuda:0")
    cm, power, _, cfg, _ = signal_case("default")
    NT = cfg["tau_max"] + 1
    n = torch.tensor([16000, 50 * 256 - 1], device=dev)   # 63 and 50 frames
    cm_d, pw_d = torch.from_numpy(np.nan_to_num(cm, nan=1.0)).to(dev), torch.from_numpy(np.nan_to_num(power, nan=0.0)).to(dev)
    big = torch.full((2, 70, NT + 5), float("nan"), device=dev)
    view = big[:, :63, :NT]
    view.copy_(cm_d)
    assert not view.is_contiguous() and view.stride() == (70 * (NT + 5), NT + 5, 1)
    dense = engine.pitch_viterbi(cm_d, pw_d, n)
    assert int((dense[2] > 0).sum()) > 50                  # (voiced frames: the comparison is not one of zeros)
    for got, want in zip(engine.pitch_viterbi(view, pw_d, n), dense):
        assert torch.equal(got, want)
