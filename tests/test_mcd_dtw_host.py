"""CPU-only checks of the MCD-DTW scoring: the float64 restatement's own properties (tests/mcd_dtw_ref.py), the two
ABI entries (symbols, struct layouts, argument errors as codes before any launch) and the two options of `main.py test`.  The
kernels themselves are checked on the GPU (tests/test_gpu_mcd_dtw.py)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import mcd_dtw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(80, 13), (80, 32), (16, 13), (7, 1)])
def test_basis_has_orthonormal_columns_without_the_constant(M, K):
    w = R.basis(M, K)
    assert w.shape == (M, K)
    assert np.abs(w.T @ w - np.eye(K)).max() < 1e-13
    assert np.abs(w.sum(axis=0)).max() < 1e-13            # c[0], the frame energy, is dropped: a constant row maps to zero
    assert abs(w[3, K - 1] - np.sqrt(2.0 / M) * np.cos(np.pi * K * 3.5 / M)) < 1e-15


def test_identical_sequences_cost_nothing_on_the_diagonal():
    a = R.trajectory(np.random.default_rng(0), 37, 13)
    cost, n, path = R.dtw(a, a, R.MCD_SCALE)
    assert cost == 0.0 and n == 37 and np.array_equal(path, np.stack([np.arange(37)] * 2, axis=1))


def test_repeating_every_frame_costs_nothing_and_doubles_the_path():
    a = R.trajectory(np.random.default_rng(1), 23, 5)
    cost, n, path = R.dtw(np.repeat(a, 2, axis=0), a)
    assert cost == 0.0 and n == 46
    R.check_path(path, 46, 23)
    assert np.array_equal(path[:, 0] // 2, path[:, 1])


def test_cost_is_symmetric():
    rng = np.random.default_rng(2)
    a = R.trajectory(rng, 41, 13)
    b = R.warped_copy(rng, a, 57, 0.1)
    c1, n1, p1 = R.dtw(a, b)
    c2, n2, p2 = R.dtw(b, a)
    assert abs(c1 - c2) <= 1e-12 * c1 and c1 > 0
    R.check_path(p1, 41, 57)
    R.check_path(p2, 57, 41)


def test_hand_computed_three_by_four():
    # d = |a_i - b_j| = [[0,1,2,4],[2,1,0,2],[3,2,1,1]];  D = [[0,1,3,7],[2,1,1,3],[5,3,2,2]].  D[1][2] and D[2][2] are ties between
    # the diagonal and another predecessor: the diagonal is taken
    a, b = np.array([[0.0], [2.0], [3.0]]), np.array([[0.0], [1.0], [2.0], [4.0]])
    cost, n, path = R.dtw(a, b)
    assert cost == 2.0 and n == 4 and path.tolist() == [[0, 0], [0, 1], [1, 2], [2, 3]]
    assert R.dtw(a, b, 2.5)[0] == 5.0
    assert R.dtw(a[:0], b)[:2] == (0.0, 0) and R.dtw(a, b[:0])[:2] == (0.0, 0) and len(R.dtw(a, b[:0])[2]) == 0


def test_ties_prefer_the_diagonal_then_the_first_index():
    d = np.zeros((3, 3))
    assert R.dtw_matrix(d)[1].tolist() == [[0, 0], [1, 1], [2, 2]]
    d = np.zeros((3, 1))
    assert R.dtw_matrix(d)[1].tolist() == [[0, 0], [1, 0], [2, 0]]
    # (2, 2) is reached at equal cost over (1, 2) and over (2, 1) while the diagonal (1, 1) costs more: (i-1, j) wins; (1, 2) in turn
    # ties between its diagonal (0, 1) and its (i-1, j) = (0, 2): the diagonal wins
    d = np.array([[0.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, 1.0]])
    cost, path = R.dtw_matrix(d)
    assert cost == 1.0 and path.tolist() == [[0, 0], [0, 1], [1, 2], [2, 2]]
    # brute force over all paths of a 4 x 5 case
    rng = np.random.default_rng(3)
    d = rng.uniform(0.1, 1.0, size=(4, 5))

    def paths(i, j):
        if i == 0 and j == 0:
            return [[(0, 0)]]
        out = []
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i - di >= 0 and j - dj >= 0:
                out += [p + [(i, j)] for p in paths(i - di, j - dj)]
        return out
    best = min(sum(d[i, j] for i, j in p) for p in paths(3, 4))
    cost, path = R.dtw_matrix(d)
    assert abs(cost - best) < 1e-12 and abs(R.path_cost(d, path) - cost) < 1e-12


def test_score_is_the_mean_over_the_warped_pairs_and_the_reference_is_quick():
    rng = np.random.default_rng(4)
    mel_a = rng.uniform(np.log(1e-5), 2.0, size=(300, 80))
    mel_b = rng.uniform(np.log(1e-5), 2.0, size=(520, 80))
    t0 = time.perf_counter()
    mcd, cost, n, path = R.mcd_dtw(mel_a, mel_b)
    dt = time.perf_counter() - t0
    assert dt < 1.0, dt
    R.check_path(path, 300, 520)
    assert 520 <= n <= 819 and abs(mcd - cost / n) < 1e-12
    d = R.distances(R.cepstra(mel_a), R.cepstra(mel_b), R.MCD_SCALE)
    assert abs(R.path_cost(d, path) - cost) <= 1e-10 * cost
    # the distance in closed form: (10 / ln 10) sqrt(2 sum_k (.)^2)
    ca, cb = R.cepstra(mel_a[:1]), R.cepstra(mel_b[:1])
    assert abs(d[0, 0] - 10.0 / np.log(10.0) * np.sqrt(2.0 * ((ca - cb) ** 2).sum())) < 1e-10
    assert np.isnan(R.mcd_dtw(mel_a[:0], mel_b)[0])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tacotron2_amd import _lib, build
    build.build(verbose=False)                  # cross-compiles for gfx950 without a GPU
    return _lib.lib()


def test_abi_entries_are_declared_exported_and_sized(lib):
    from tacotron2_amd import _lib
    for sym in ("t2_mel_cepstra", "t2_dtw"):
        assert sym in _lib.DECLARED_SYMBOLS and hasattr(lib, sym)
    for st in ("T2MelCeps", "T2Dtw"):
        assert lib.t2_sizeof(st.encode()) == C.sizeof(_lib.S[st]) > 0
    assert [f[0] for f in _lib._structs["T2MelCeps"]] == ["mel", "ld_b", "ld_t", "B", "T", "M", "K", "len", "basis", "out", "ld_ob",
                                                          "ld_ot"]
    assert [f[0] for f in _lib._structs["T2Dtw"]] == ["a", "ld_ab", "ld_at", "b", "ld_bb", "ld_bt", "B", "Ta", "Tb", "K", "len_a",
                                                      "len_b", "scale", "cost", "path_len", "back", "path"]
    hdr = open(os.path.join(ROOT, "include", "tacotron2_amd.h")).read()
    assert "#define T2_DTW_MAX_T 4096" in hdr and "#define T2_DTW_MAX_K 32" in hdr
    # the LDS budget stated in the header: three fp64 rows and three int32 rows at the cap, inside 160 KB
    assert 3 * 4096 * (8 + 4) == 147456 <= 160 * 1024


def test_dtw_argument_errors_are_codes_before_any_launch(lib):
    from tacotron2_amd import _lib
    p = 1 << 20                                  # (never dereferenced: every call below fails its argument check)
    ok = dict(a=p, ld_ab=8 * 13, ld_at=13, b=p, ld_bb=9 * 13, ld_bt=13, B=2, Ta=8, Tb=9, K=13, len_a=p, len_b=p, scale=1.0, cost=p,
              path_len=p, back=p, path=p)
    cases = [(dict(Ta=4097, ld_ab=4097 * 13), b"T2_DTW_MAX_T"), (dict(Tb=4097, ld_bb=4097 * 13), b"T2_DTW_MAX_T"),
             (dict(K=0), b"T2_DTW_MAX_K"), (dict(K=33, ld_at=33, ld_bt=33, ld_ab=8 * 33, ld_bb=9 * 33), b"T2_DTW_MAX_K"),
             (dict(back=None), b"back"), (dict(ld_at=12), b"strides of a"), (dict(ld_ab=7 * 13 + 12), b"strides of a"),
             (dict(ld_bt=12), b"strides of b"), (dict(ld_bb=8 * 13 + 12), b"strides of b"), (dict(scale=float("inf")), b"scale"),
             (dict(B=0), b"B, Ta, Tb >= 1")]
    cases += [({k: None}, b"null") for k in ("a", "b", "len_a", "len_b", "cost", "path_len")]
    for bad, word in cases:
        s = _lib.make("T2Dtw", **dict(ok, **bad))
        assert lib.t2_dtw(C.addressof(s), None) == 1, bad
        assert b"t2_dtw" in lib.t2_last_error() and word in lib.t2_last_error(), (bad, lib.t2_last_error())
    assert lib.t2_dtw(None, None) == 1 and b"t2_dtw" in lib.t2_last_error()


def test_mel_cepstra_argument_errors_are_codes_before_any_launch(lib):
    from tacotron2_amd import _lib
    p = 1 << 20
    ok = dict(mel=p, ld_b=5 * 80, ld_t=80, B=2, T=5, M=80, K=13, len=p, basis=p, out=p, ld_ob=5 * 13, ld_ot=13)
    cases = [(dict(K=0), b"T2_DTW_MAX_K"), (dict(K=33, ld_ot=33, ld_ob=5 * 33), b"T2_DTW_MAX_K"), (dict(M=1025, ld_t=1025), b"T2_CEPS_MAX_M"),
             (dict(ld_t=79), b"strides of mel"), (dict(ld_b=4 * 80 + 79), b"strides of mel"), (dict(ld_ot=12), b"strides of out"),
             (dict(ld_ob=4 * 13 + 12), b"strides of out"), (dict(T=0), b"B, T, M >= 1")]
    cases += [({k: None}, b"null") for k in ("mel", "len", "basis", "out")]
    for bad, word in cases:
        s = _lib.make("T2MelCeps", **dict(ok, **bad))
        assert lib.t2_mel_cepstra(C.addressof(s), None) == 1, bad
        assert b"t2_mel_cepstra" in lib.t2_last_error() and word in lib.t2_last_error(), (bad, lib.t2_last_error())
    assert lib.t2_mel_cepstra(None, None) == 1 and b"t2_mel_cepstra" in lib.t2_last_error()


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
def _main(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + list(args), cwd=ROOT, capture_output=True, text=True,
                          timeout=300)


def test_cli_help_lists_both_flags():
    r = _main("test", "--help")
    assert r.returncode == 0 and "--score" in r.stdout and "--no-audio" in r.stdout


def test_cli_no_audio_without_score_is_a_usage_error():
    r = _main("test", "--speech-dir", "s", "--checkpoint", "k", "--no-audio")
    assert r.returncode == 2 and "--no-audio" in r.stderr and "--score" in r.stderr
