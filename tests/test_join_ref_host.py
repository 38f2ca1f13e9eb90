"""The numpy restatement of t2_join (tests/join_ref.py) on the CPU: its spans against trim_silence, hand-computed plans, the fades.
No GPU: what the kernel is compared with in tests/test_gpu_join.py is checked here on its own."""
import numpy as np
import pytest

import join_ref as R
from tacotron2_amd.datasets.tts_dataset import trim_silence

F, H = 2048, 512


def _burst(n, a, b, seed, amp=0.1):
    """n samples of exact zeros with noise of RMS amp in [a, b)."""
    x = np.zeros(n, np.float32)
    x[a:b] = (amp * np.random.default_rng(seed).standard_normal(b - a)).astype(np.float32)
    return x


SIGNALS = [("burst in silence", 20000, 6000, 13000), ("active from sample 0", 20000, 0, 9000), ("active to the last sample", 20000, 7000, 20000),
           ("n not a multiple of H", 5000, 1300, 3100), ("all active", 7777, 0, 7777), ("n == F", 2048, 600, 1500)]


@pytest.mark.parametrize("name,n,a,b", SIGNALS, ids=[s[0] for s in SIGNALS])
@pytest.mark.parametrize("top_db", [60.0, 30.0])
def test_span_is_what_trim_silence_keeps(name, n, a, b, top_db):
    x = _burst(n, a, b, seed=n + a)
    s0, s1, margin = R.span_ref(x, top_db, F, H, keep=0)
    assert margin > 1e-9
    kept = trim_silence(x, top_db, F, H)
    pad = F // 2                                                   # trim_silence's own frames, to find where its slice starts
    cs = np.concatenate([[0.0], np.cumsum(np.square(np.pad(x, pad).astype(np.float64)))])
    e = cs[H * np.arange(1 + n // H) + F] - cs[H * np.arange(1 + n // H)]
    nz = np.nonzero(e > e.max() * 10 ** (-top_db / 10))[0]
    assert (s0, s1) == (nz[0] * H, min(n, (nz[-1] + 1) * H))
    assert len(kept) == s1 - s0 and np.array_equal(kept, x[s0:s1])


def test_a_quiet_tail_below_top_db_is_cut_and_above_it_is_kept():
    x = _burst(20000, 4096, 8192, 1, amp=0.1)
    x[12288:16384] = _burst(4096, 0, 4096, 2, amp=0.1 * 10 ** (-70 / 20))          # 70 dB down
    assert R.span_ref(x, 60.0, F, H)[:2] == (4096 - H, 8192 + 2 * H) == trim_silence_span(x, 60.0)
    assert R.span_ref(x, 80.0, F, H)[:2] == (4096 - H, 16384 + 2 * H) == trim_silence_span(x, 80.0)


def trim_silence_span(x, top_db):
    kept = trim_silence(x, top_db, F, H)
    start = next(i for i in range(0, len(x), H) if np.array_equal(x[i:i + len(kept)], kept))
    return start, start + len(kept)


def test_the_silent_row_is_empty_and_short_rows_are_whole():
    # NOT trim_silence's answer: its 1e-10 floors put every frame of an all-zero signal at 0 dB of the peak, so it keeps the
    # signal whole; a synthesised piece of pure silence contributes its pause alone.
    z = np.zeros(5000, np.float32)
    assert R.span_ref(z, 60.0, F, H)[:2] == (0, 0) and len(trim_silence(z, 60, F, H)) == 5000
    x = _burst(F - 1, 100, 300, 3)
    assert R.span_ref(x, 60.0, F, H)[:2] == (0, F - 1) and len(trim_silence(x, 60, F, H)) == F - 1
    assert R.span_ref(_burst(9000, 3000, 4000, 4), 60.0, F, H, trim=False)[:2] == (0, 9000)
    assert R.span_ref(np.zeros(0, np.float32))[:2] == (0, 0)


def test_keep_widens_the_span_and_is_clamped_to_the_row():
    x = _burst(20000, 6000, 13000, 5)
    s0, s1, _ = R.span_ref(x, 60.0, F, H, keep=0)
    assert R.span_ref(x, 60.0, F, H, keep=441)[:2] == (s0 - 441, s1 + 441)
    x = _burst(5000, 100, 4950, 6)                                  # active inside the first and the last `keep` samples
    assert R.span_ref(x, 60.0, F, H, keep=441)[:2] == (0, 5000)


def _const_rows(levels, n=100):
    x = np.zeros((len(levels), n), np.float32)
    for b, v in enumerate(levels):
        x[b, :] = v
        x[b, 1::2] *= -1
    return x


def test_plan_level_off_offsets_and_total():
    x = _const_rows([0.5, 0.25, 0.125])
    r = R.join_ref(x, [100, 60, 0], [0, 7, 3], trim=False)
    assert r["gain"].tolist() == [1.0, 1.0, 1.0] and r["len"].tolist() == [100, 60, 0] and r["s0"].tolist() == [0, 0, 0]
    assert r["off"].tolist() == [0, 100, 167] and r["total"] == 170
    assert np.array_equal(r["y"][:100], x[0]) and np.array_equal(r["y"][100:160], x[1, :60]) and not r["y"][160:].any()
    r = R.join_ref(x, [100, 60, 10], [0, 0, 0], trim=False)
    assert r["off"].tolist() == [0, 100, 160] and r["total"] == 170


def test_plan_level_on_clamps_both_ways_and_skips_the_silent_piece():
    # rows of constant magnitude: rms = the magnitude.  rms_doc^2 = (1 + 1 + 1/64 + 16) / 4 over the four live rows of equal length
    x = _const_rows([1.0, 1.0, 0.125, 4.0, 0.0])
    r = R.join_ref(x, [100] * 5, [0] * 5, trim=False, level=True, max_gain=2.0)
    rms_doc = np.sqrt((1 + 1 + 1 / 64 + 16) * 100 / 500)            # the silent row's 100 samples count in sum len
    assert r["gain64"].tolist() == [rms_doc, rms_doc, 2.0, 0.5, 1.0] and 1.0 < rms_doc < 2.0
    z = np.zeros((1, 50), np.float32)
    assert R.join_ref(z, [50], [0], trim=False, level=True)["gain"].tolist() == [1.0]
    r = R.join_ref(z, [50], [9], trim=True, level=True, F=16, H=4)   # trimmed away: only the pause is left
    assert (r["len"].tolist(), r["total"], r["gain"].tolist()) == ([0], 9, [1.0]) and not r["y"].any()


def test_plan_ceiling_engages_only_above_it():
    x = _const_rows([0.9, 0.3])
    r = R.join_ref(x, [100, 100], [0, 0], trim=False, level=True, max_gain=2.0, ceiling=1.0)
    a, b = np.float64(np.float32(0.9)), np.float64(np.float32(0.3))
    rms_doc = np.sqrt((a * a * 100 + b * b * 100) / 200)
    g = np.array([rms_doc / a, 2.0])                                 # (0.745; 2.236 clamped)
    pk = max(g[0] * a, g[1] * b)
    assert pk < 1.0 and np.allclose(r["gain64"], g, rtol=1e-12)      # the ceiling does not engage
    x = _const_rows([0.9, 0.2])
    r = R.join_ref(x, [100, 100], [0, 0], trim=False, ceiling=0.5)
    assert np.allclose(r["gain64"], [0.5 / np.float64(np.float32(0.9))] * 2, rtol=1e-15)      # level off: every gain lowered alike
    assert np.abs(r["y"]).max() <= np.float32(0.5) * (1 + 2.0 ** -23)
    assert R.join_ref(x, [100, 100], [0, 0], trim=False, ceiling=0.9)["gain"].tolist() == [1.0, 1.0]   # a peak AT the ceiling


FADE = 8


@pytest.mark.parametrize("length", [0, 1, 2, 2 * FADE - 1, 2 * FADE, 2 * FADE + 1, 100])
def test_fades(length):
    w = R.fade_table(FADE)
    assert np.array_equal(w, (0.5 - 0.5 * np.cos(np.pi * (np.arange(FADE) + 0.5) / FADE)).astype(np.float32)) and np.all(np.diff(w) > 0)
    x = np.ones((1, 120), np.float32)
    y = R.join_ref(x, [length], [0], trim=False, fade=FADE)["y"]
    fl = min(FADE, length // 2)
    assert len(y) == length and np.array_equal(y, y[::-1])          # a symmetric input gives a symmetric output
    if length == 1:
        assert y.tolist() == [1.0]                                  # fl = 0: no fade
    elif length >= 2:
        first = w[FADE // (2 * fl)]                                 # i = 0: index (2 * 0 + 1) * fade // (2 fl)
        assert y[0] == first == y[-1]
        if fl == FADE:
            assert first == w[0] and np.array_equal(y[:FADE], w) and np.all(y[FADE:length - FADE] == 1.0)
        if length == 2:
            assert first == w[FADE // 2]                            # one step: the middle of the table
        if length % 2:
            assert y[length // 2] == 1.0 or fl == FADE
    assert np.array_equal(R.envelope(length, 0, R.fade_table(0)), np.ones(length, np.float32))


def test_the_shortened_fade_samples_the_same_table():
    w = R.fade_table(110)
    e = R.envelope(219, 110, w)                                     # fl = 109
    assert np.array_equal(e[:109], w[((2 * np.arange(109) + 1) * 110) // 218]) and e[109] == 1.0
    assert np.array_equal(e[110:], e[:109][::-1])
    assert np.array_equal(R.envelope(220, 110, w), np.concatenate([w, w[::-1]]))
