"""CPU-only checks of the per-character durations: the float64 reference (tests/durations_ref.py) against brute-force enumeration
of every monotonic path, the pinned edge rules (ties stay, infeasible falls back to the argmax, the last step's frames with a
reduction factor), the ABI entry and the two CLI options.  The kernel itself is compared with this reference on the GPU
(tests/test_gpu_durations.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import durations_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _softmax_rows(rng, S, N, sharpen=0.0):
    z = rng.normal(size=(S, N))
    if sharpen:
        z[np.arange(S), np.minimum(np.arange(S) * N // S, N - 1)] += sharpen
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("S,N", [(7, 4), (6, 6), (5, 1), (1, 1), (8, 3)])
def test_reference_against_brute_force_over_all_monotonic_paths(S, N):
    rng = np.random.default_rng(100 * S + N)
    for sharpen in (0.0, 3.0):
        a = _softmax_rows(rng, S, N, sharpen)
        la = R.log_align(a)
        pos, score, margin = R.monotonic_path(la)
        bpos, bscore = R.brute_force(la)
        assert np.array_equal(pos, bpos), (pos, bpos)
        assert abs(score - bscore) <= 1e-12 * max(1.0, abs(bscore))
        assert pos[0] == 0 and pos[-1] == N - 1 and set(np.diff(pos)) <= {0, 1}
        dur, stats, m2 = R.durations(a, N, S, 1, "monotonic")
        assert np.array_equal(dur, np.bincount(bpos, minlength=N)) and dur.min() >= 1 and dur.sum() == S
        assert stats[2] == 1.0 and abs(stats[1] - bscore / S) <= 1e-12 * max(1.0, abs(bscore)) and m2 == margin


def test_a_tie_stays_on_the_character():
    a = np.full((4, 2), 0.5, dtype=np.float32)
    dur, stats, margin = R.durations(a, 2, 4, 1, "monotonic")
    # backtracking from the last character, a tie keeps it: the path stays on character 1 down to step 1, the only step whose
    # other predecessor is unreachable - character 0 keeps its one mandatory step.  The decisions at steps 2 and 3 are exact ties
    assert dur.tolist() == [1, 3] and margin == 0.0
    assert stats[2] == 1.0 and abs(stats[0] - 0.5) < 1e-12 and abs(stats[1] - np.log(np.float64(np.float32(0.5)))) < 1e-12


def test_infeasible_utterance_gets_the_argmax_counts():
    rng = np.random.default_rng(7)
    a = _softmax_rows(rng, 3, 5)
    dur, stats, _ = R.durations(a, 5, 3, 1, "monotonic")
    dur0, stats0, _ = R.durations(a, 5, 3, 1, "argmax")
    assert stats[2] == 0.0 and stats0[2] == 0.0 and stats[3] == 1.0
    assert np.array_equal(dur, np.bincount(a.argmax(axis=1), minlength=5)) and np.array_equal(dur, dur0) and dur.sum() == 3
    assert np.array_equal(stats, stats0)


def test_reduction_factor_last_step_carries_the_remainder():
    assert R.step_weights(10, 3).tolist() == [3, 3, 3, 1]
    assert R.step_weights(9, 3).tolist() == [3, 3, 3] and R.step_weights(1, 3).tolist() == [1] and R.step_weights(0, 3).tolist() == []
    rng = np.random.default_rng(3)
    a = _softmax_rows(rng, 6, 3, 3.0)                         # 6 step rows given, 4 used
    a[4:] = np.nan
    for mode in ("monotonic", "argmax"):
        dur, stats, _ = R.durations(a, 3, 10, 3, mode)
        assert dur.sum() == 10 and np.isfinite(stats).all()
    dur, _, _ = R.durations(a, 3, 10, 3, "monotonic")
    pos, _, _ = R.monotonic_path(R.log_align(a[:4, :3]))
    assert dur[pos[-1]] % 3 == 1 and pos[-1] == 2            # the last character holds the one-frame step


def test_empty_text_or_no_frames_is_all_zero():
    a = np.full((4, 3), np.nan, dtype=np.float32)
    for N, F in ((0, 4), (3, 0)):
        dur, stats, _ = R.durations(a, N, F, 1, "monotonic")
        assert not dur.any() and not stats.any()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tacotron2_amd import _lib, build
    build.build(verbose=False)                  # cross-compiles for gfx950 without a GPU
    return _lib.lib()


def test_abi_entry_is_declared_exported_and_sized(lib):
    from tacotron2_amd import _lib
    assert "t2_align_durations" in _lib.DECLARED_SYMBOLS and hasattr(lib, "t2_align_durations")
    assert lib.t2_sizeof(b"T2AlignDur") == C.sizeof(_lib.S["T2AlignDur"]) > 0
    assert [f[0] for f in _lib._structs["T2AlignDur"]] == ["align", "ld_b", "ld_s", "B", "S", "L", "r", "mode", "chars_len",
                                                           "frames_len", "dur", "ld_dur", "stats", "back"]


def test_argument_errors_are_codes_before_any_launch(lib):
    from tacotron2_amd import _lib
    ok = dict(align=1 << 20, ld_b=64, ld_s=8, B=1, S=8, L=8, r=1, mode=1, chars_len=1 << 20, frames_len=1 << 20, dur=1 << 20,
              ld_dur=8, stats=1 << 20, back=1 << 20)         # (never dereferenced: every call below fails its argument check)
    for bad, word in ((dict(L=4097, ld_s=4097, ld_dur=4097), b"T2_ALIGN_MAX_L"), (dict(mode=2), b"mode"), (dict(back=None), b"back"),
                      (dict(r=0), b"r >= 1"), (dict(ld_dur=7), b"ld_dur")):
        a = _lib.make("T2AlignDur", **dict(ok, **bad))
        assert lib.t2_align_durations(C.addressof(a), None) == 1, bad
        assert b"t2_align_durations" in lib.t2_last_error() and word in lib.t2_last_error(), (bad, lib.t2_last_error())


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
def _main(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + list(args), cwd=ROOT, capture_output=True, text=True,
                          timeout=300)


def test_cli_help_lists_the_new_command_and_options():
    r = _main("duration-export", "--help")
    assert r.returncode == 0 and all(w in r.stdout for w in ("--speech-dir", "--checkpoint", "--results-dir", "--mode", "monotonic",
                                                             "argmax"))
    r = _main("say", "--help")
    assert r.returncode == 0 and "--durations-out" in r.stdout
    assert "duration-export" in _main("--help").stdout


def test_cli_bad_mode_is_a_usage_error():
    r = _main("duration-export", "--speech-dir", "s", "--checkpoint", "k", "--mode", "viterbi")
    assert r.returncode == 2 and "--mode" in r.stderr
