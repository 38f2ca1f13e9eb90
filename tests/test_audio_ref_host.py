"""tests/audio_ref.py checked on the CPU: the float64 references against independent routes (torch.stft, a direct O(N^2) DFT,
oracle/logmel_ref.py, torch.nn.functional convolutions, the exact round trips), the tolerance constants against the float32
restatement they are derived from, the conditions the GPU comparisons rest on (coverage of the per-element log comparison, silent
frames, empty filters), and each metric against the mistake it exists for - a mutation of the restatement, never of product code."""
import math

import numpy as np
import pytest
import torch

from tests import audio_ref as A

F64 = torch.float64


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# -----------------------------------------------------------------------------------------------------------------
# The references against independent routes
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(A.GEOMETRIES))
def test_stft_against_torch_stft(geom):
    g = A.GEOMETRIES[geom]
    n_fft, hop = g["n_fft"], g["hop"]
    for n in A.lengths(geom):
        y = A.signal(geom, n).double()
        ref = torch.stft(y, n_fft, hop, n_fft, torch.hann_window(n_fft, periodic=True, dtype=F64), center=True, pad_mode="reflect",
                         return_complex=True).T                                          # (frames, nb), frames = 1 + n // hop
        got = A.stft_ri(y, n_fft, hop)
        assert got.shape == (1 + n // hop, 2 * (n_fft // 2 + 1))
        assert _rel(got, torch.cat([ref.real, ref.imag], 1)) < 1e-12, (geom, n)
        assert _rel(A.magnitude(got), ref.abs()) < 1e-12


def test_stft_against_a_direct_dft():
    n_fft, hop, n = 64, 16, 145
    y = A.signal("small", n).double().numpy()
    pad = np.concatenate([y[1:n_fft // 2 + 1][::-1], y, y[-n_fft // 2 - 1:-1][::-1]])
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    got = A.stft_ri(torch.from_numpy(y), n_fft, hop).numpy()
    assert np.array_equal(A.reflect_pad(torch.from_numpy(y), n_fft // 2).numpy(), pad)
    for f in range(1 + n // hop):
        for k in range(n_fft // 2 + 1):
            X = sum(pad[f * hop + i] * win[i] * np.exp(-2j * np.pi * k * i / n_fft) for i in range(n_fft))
            assert abs(got[f, k] - X.real) < 1e-11 and abs(got[f, n_fft // 2 + 1 + k] - X.imag) < 1e-11, (f, k)


def test_log_mel_against_the_oracle_restatement():
    from oracle.logmel_ref import logmel, mel_filterbank
    g = A.GEOMETRIES["default"]
    fb = A.mel_filterbank(g["sr"], g["n_fft"], g["n_mels"], g["f_min"], g["f_max"])
    assert float((fb - torch.from_numpy(mel_filterbank())).abs().max()) < 1e-12
    for n in A.lengths("default"):
        ref = torch.from_numpy(logmel(A.signal("default", n).double().numpy()))
        r = A.log_mel_case("default", n)
        # the oracle computes its spectrum with an FFT: the floor's neighbourhood (a magnitude of 1e-13 against zero) is left out
        live = ~r["silent"]
        assert float((r["out"] - ref)[live].abs().max()) < 1e-9, n
        assert float((r["out"] - ref)[~live].abs().max()) == 0.0 if bool((~live).any()) else True


def test_batch_layout():
    outs = [torch.full((3, 4), 1.5), torch.full((1, 4), 2.5), torch.full((5, 4), -3.0)]
    mel, gate, mel_len = A.batch_layout(outs, 6)
    assert mel.shape == (3, 6, 4) and mel_len.tolist() == [3, 1, 5]
    assert gate.tolist() == [[1, 1, 0, 0, 0, 0], [0] * 6, [1, 1, 1, 1, 0, 0]]
    assert bool((mel[0, :3] == 1.5).all()) and bool((mel[0, 3:] == 0).all()) and bool((mel[1, 1:] == 0).all()) and bool((mel[2, :5] == -3).all())


@pytest.mark.parametrize("case", A.CONV_CASES, ids=str)
def test_conv1d_against_torch_functional(case):
    Ci, Co, k, d = case
    for L in A.CONV_LENGTHS:
        i = A.conv_inputs(case, L)
        ref = torch.nn.functional.conv1d(i["x"].double().t()[None], i["w"].double(), i["b"].double(), padding=d * (k - 1) // 2, dilation=d)[0].t()
        assert _rel(A.conv1d(i["x"], i["w"], i["b"], d), ref) < 1e-12
        assert _rel(A.conv1d(i["x"], i["w"], i["b"], d, i["res"]), ref + i["res"].double()) < 1e-12


@pytest.mark.parametrize("case", A.UP_CASES, ids=str)
def test_conv_transpose1d_against_torch_functional(case):
    Ci, Co, u = case
    for L in A.UP_LENGTHS:
        i = A.up_inputs(case, L)
        ref = torch.nn.functional.conv_transpose1d(i["x"].double().t()[None], i["w"].double(), i["b"].double(), stride=u, padding=u // 2)[0].t()
        got = A.conv_transpose1d(i["x"], i["w"], i["b"], u)
        assert got.shape == (L * u, Co) and _rel(got, ref) < 1e-12


def test_margin_layouts():
    x = torch.ones(3, 2)
    buf = A.margin_input(x, 5)
    assert buf.shape == (3 + 2 * A.PAD, 2) and bool(torch.isnan(buf[:A.PAD - 5]).all()) and bool(torch.isnan(buf[A.PAD + 3 + 5:]).all())
    assert bool((buf[A.PAD - 5:A.PAD] == 0).all()) and bool((buf[A.PAD + 3:A.PAD + 8] == 0).all()) and bool((buf[A.PAD:A.PAD + 3] == 1).all())
    exp = A.margin_expected(x, A.SENTINEL)
    assert bool((exp[:A.PAD] == A.SENTINEL).all()) and bool((exp[A.PAD + 3:] == A.SENTINEL).all()) and bool((exp[A.PAD:A.PAD + 3] == 1).all())


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_istft_inverts_the_stft(geom):
    g = A.GEOMETRIES[geom]
    n_fft, hop = g["n_fft"], g["hop"]
    for n in (9 * hop, 140 * hop):
        y = A.signal(geom, n).double()
        back = A.istft(A.stft3(y, n_fft, hop), n_fft, hop)
        assert back.shape == y.shape and _rel(back, y) < 1e-12


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_pseudo_inverse_and_clamp(geom):
    g = A.GEOMETRIES[geom]
    fb = A.mel_filterbank(g["sr"], g["n_fft"], g["n_mels"], g["f_min"], g["f_max"])
    pinv = torch.linalg.pinv(fb)
    assert _rel(fb @ pinv @ fb, fb) < 1e-10
    m = A.random_mel(geom)
    lin = A.mel_to_linear(m, fb)
    raw = m.double() @ pinv.t()
    assert float(raw.min()) < -1e-3 * float(raw.abs().max())                      # the clamp has work
    assert float(lin.min()) == 0.0 and torch.equal(lin, raw.clamp(min=0))


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_griffin_lim_from_the_true_phases_returns_the_signal(geom):
    g = A.GEOMETRIES[geom]
    n_fft, hop = g["n_fft"], g["hop"]
    y = A.signal(geom, hop * (A.GL_FRAMES - 1), False).double()
    spec = A.stft3(y, n_fft, hop)
    S, ph = A.magnitude(spec.reshape(spec.shape[0], -1)), torch.atan2(spec[:, 1], spec[:, 0])
    for it in (1, 2):
        assert _rel(A.griffin_lim(S, ph, it, A.MOMENTUM, n_fft, hop), y) < 1e-9, it


# -----------------------------------------------------------------------------------------------------------------
# The constants
# -----------------------------------------------------------------------------------------------------------------
def test_tolerances_are_anchored_to_the_float32_restatement():
    """F32_ERR is what the float32 run of each reference differs from its float64 run by over the committed case lists: no case
    exceeds its stored constant, no stored constant is more than twice the measured worst, TOL = 16 x F32_ERR."""
    worst = A.measure_f32_err()
    print("output          float32 restatement   F32_ERR    TOL (x 16)")
    for k, (e, name) in worst.items():
        print(f"{k:15s} {e:.2e} ({name})   {A.F32_ERR[k]:.1e}   {A.TOL[k]:.2e}")
    assert set(worst) == set(A.F32_ERR) == set(A.TOL)
    for k, (e, name) in worst.items():
        assert e <= A.F32_ERR[k] <= 2.0 * e, (k, e, name, A.F32_ERR[k])
        assert A.TOL[k] == 16.0 * A.F32_ERR[k]
    assert A.FLOOR_TOL == 2e-6 and 2 * float(np.spacing(np.float32(abs(math.log(1e-5))))) < A.FLOOR_TOL < 3e-6
    assert A.COVER == 10 * A.FLOOR


# -----------------------------------------------------------------------------------------------------------------
# The conditions
# -----------------------------------------------------------------------------------------------------------------
def test_case_tables_are_the_ones_the_kernels_need():
    G = A.GEOMETRIES
    assert list(G) == ["default", "small", "narrow", "sr16k", "oddhop"] and A.BATCH_GEOMETRIES == ["default", "small", "narrow", "sr16k"]
    assert (G["default"]["n_fft"] // 2 + 1, G["small"]["n_fft"] // 2 + 1) == (513, 33) and G["small"]["f_max"] == G["small"]["sr"] / 2
    assert G["oddhop"]["n_fft"] % G["oddhop"]["hop"] != 0 and all(G[g]["n_fft"] % G[g]["hop"] == 0 for g in A.BATCH_GEOMETRIES)
    for geom, g in G.items():
        P, hop = g["n_fft"] // 2, g["hop"]
        ns = A.lengths(geom)
        assert ns[:5] == [P + 1, g["n_fft"], 9 * hop, 9 * hop - 1, 9 * hop + 1] and 128 < 1 + ns[5] // hop <= 144
    assert A.lengths("default")[5] < 36500
    assert A.CONV_CASES == [(80, 32, 7, 1), (32, 32, 11, 5), (64, 64, 7, 3), (16, 16, 3, 3), (8, 8, 11, 5), (8, 1, 7, 1)]
    assert max(d * (k - 1) // 2 for _, _, k, d in A.CONV_CASES) == 25 <= A.PAD
    assert A.CONV_LENGTHS == (1, 2, 33, 130) and A.UP_CASES == [(32, 16, 8), (16, 8, 2), (64, 32, 4)] and A.UP_LENGTHS == (1, 3, 40)


@pytest.mark.parametrize("geom", list(A.GEOMETRIES))
def test_coverage_silence_and_empty_filters(geom):
    """The per-element log comparison covers >= 75 % of the elements of non-silent frames in non-empty filters of EVERY utterance;
    every utterance that can hold the block of 2 * n_fft zeros has at least two digitally silent frames (the three shortest
    lengths are shorter than the block), so every geometry's list and every batch has them; `narrow` has empty filters."""
    g = A.GEOMETRIES[geom]
    with_block = 0
    for n in A.lengths(geom):
        r = A.log_mel_case(geom, n)
        assert A.coverage(r) >= 0.75, (geom, n, A.coverage(r))
        assert int((~r["silent"]).sum()) >= 2
        if n >= 2 * g["n_fft"] + g["hop"] // 2:
            with_block += 1
            assert int(r["silent"].sum()) >= 2, (geom, n)
            s = r["silent"]
            assert bool((r["lin"][s] == 0).all()) and bool((r["out"][s] == math.log(A.FLOOR)).all())
        assert bool((r["lin"][:, r["empty"]] == 0).all())
    assert with_block == 4
    n_empty = int(A.log_mel_case(geom, A.lengths(geom)[0])["empty"].sum())
    assert n_empty == (4 if geom == "narrow" else 0)


# -----------------------------------------------------------------------------------------------------------------
# The metrics see the mistakes they exist for
# -----------------------------------------------------------------------------------------------------------------
def _mutant(geom, n, fault):
    return A.log_mel(A.signal(geom, n), geom, torch.float32, fault)


@pytest.mark.parametrize("geom", list(A.GEOMETRIES))
def test_log_mel_metrics_see_their_mutations(geom):
    n = A.lengths(geom)[4]
    ref = A.log_mel_case(geom, n)
    clean = A.log_mel(A.signal(geom, n), geom, torch.float32)
    assert torch.equal(clean["padded"], ref["padded"])
    assert A.rel(clean["spec"], ref["spec"]) <= A.F32_ERR["spec"] and A.mel_figures(clean["out"], ref)["floor"] <= A.FLOOR_TOL

    bad = _mutant(geom, n, "pad_off_by_one")
    assert not torch.equal(bad["padded"], ref["padded"]) and A.rel(bad["spec"], ref["spec"]) > A.TOL["spec"]
    bad = _mutant(geom, n, "symmetric_hann")
    assert A.rel(bad["spec"], ref["spec"]) > A.TOL["spec"] and A.mel_figures(bad["out"], ref)["mel_lin"] > A.TOL["mel_lin"]
    bad = _mutant(geom, n, "nyquist_dropped")
    assert A.rel(bad["mag"], ref["mag"]) > A.TOL["mag"]
    bad = _mutant(geom, n, "floor")
    assert A.mel_figures(bad["out"], ref)["floor"] > A.FLOOR_TOL
    bad = _mutant(geom, n, "filter_norm")
    assert A.mel_figures(bad["out"], ref)["mel_log"] > A.TOL["mel_log"] and A.rel(bad["lin"], ref["lin"]) > A.TOL["tmp"]


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_vocoder_metrics_see_their_mutations(geom):
    g = A.GEOMETRIES[geom]
    n_fft, hop = g["n_fft"], g["hop"]
    for frames in A.ISTFT_FRAMES:
        s = A.random_spec(geom, frames)
        ref = A.istft(s, n_fft, hop)
        assert A.rel(A.istft(s, n_fft, hop, torch.float32), ref) <= A.F32_ERR["istft"]
        assert A.rel(A.istft(s, n_fft, hop, torch.float32, "herm_dc"), ref) > A.TOL["istft"]
        assert A.rel(A.istft(s, n_fft, hop, torch.float32, "env_sum_win"), ref) > A.TOL["istft"]
    S, ph = A.gl_input(geom)
    ref = A.griffin_lim(S, ph, 2, A.MOMENTUM, n_fft, hop)
    assert A.rel_l2(A.griffin_lim(S, ph, 2, A.MOMENTUM, n_fft, hop, torch.float32, "alpha"), ref) > A.TOL["gl2"]
    ref1 = A.griffin_lim(S, ph, 1, A.MOMENTUM, n_fft, hop)
    assert A.rel_l2(ref, ref1) > A.TOL["gl1"]                                      # the second iteration moves the waveform


def test_layer_metrics_see_their_mutations():
    for case in A.UP_CASES:
        for L in A.UP_LENGTHS:
            i = A.up_inputs(case, L)
            ref = A.conv_transpose1d(i["x"], i["w"], i["b"], case[2])
            assert A.rel(A.conv_transpose1d(i["x"], i["w"], i["b"], case[2], torch.float32, "taps_swapped"), ref) > A.TOL["up"]
    for case in A.CONV_CASES:
        if case[3] == 1:
            continue
        for L in (L for L in A.CONV_LENGTHS if L > case[3]):                      # at L <= d - 1 only the centre tap meets data
            i = A.conv_inputs(case, L)
            ref = A.conv1d(i["x"], i["w"], i["b"], case[3])
            assert A.rel(A.conv1d(i["x"], i["w"], i["b"], case[3], None, torch.float32, "dilation"), ref) > A.TOL["conv"]
            assert A.rel(A.conv1d(i["x"], i["w"], i["b"], case[3], i["res"], torch.float32, "dilation"),
                         A.conv1d(i["x"], i["w"], i["b"], case[3], i["res"])) > A.TOL["conv_acc"]
