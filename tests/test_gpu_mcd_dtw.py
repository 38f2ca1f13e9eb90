"""MCD-DTW scoring on the GPU: t2_dtw and t2_mel_cepstra (csrc/t2_dtw.hip) against the float64 restatement of
tests/mcd_dtw_ref.py, then Engine.mcd_dtw and TTSModel.score.

Criteria for t2_dtw.  The kernel forms d(i, j) in fp32 and runs the recurrence in fp64; the reference does both in float64.  A path
is therefore not compared cell by cell (a near-tie may legitimately resolve the other way) but by properties.  With u = 2^-24 and
eps = (K + 8) u - the roundings of the difference (1), the square and the K-term FMA sum (K + 1), sqrtf (1), the scale and its own
float32 rounding (2), with margin - every fp32 distance is within eps relative of the float64 one, so
  1. the returned path is a warping path of path_len cells, and path_len is the same with and without the `back` workspace;
  2. |cost - sum_path d64| <= eps * sum_path d64 (the kernel's cost is the sum of ITS distances along ITS path, in fp64);
  3. sum_path d64 - opt64 <= 2.5 eps * opt64: the path is optimal under distances within eps relative, so under the float64 ones
     it loses at most (1 + eps) / (1 - eps) - 1 < 2.5 eps against the float64 optimum;
  4. a pair with an empty side returns (0, 0) and nothing of its rows is read (they are NaN).
Shapes: the smallest at which the wavefront can go wrong - single rows and columns, the wave edge (64, 63), the block edge in both
orientations (255 / 256 / 257), and (300, 520) / (520, 300) where a thread owns several cells of a diagonal and the diagonals
shorten over long tails."""
import functools

import numpy as np
import pytest
import torch

import mcd_dtw_ref as R

pytestmark = pytest.mark.gpu
U = R.U


def _dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def _eps(K):
    return (K + 8) * U


def _dtw(a, la, b, lb, scale, dev, with_path=True):
    """One t2_dtw call on device tensors (any strides with a contiguous last dimension) -> (cost, path_len, path | None) numpy."""
    from tacotron2_amd import _lib
    B, Ta, K = a.shape
    Tb = b.shape[1]
    cost = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    plen = torch.full((B,), -7, dtype=torch.int32, device=dev)
    back = torch.empty(B * Ta * Tb, dtype=torch.uint8, device=dev) if with_path else None
    path = torch.full((B, Ta + Tb - 1, 2), -7, dtype=torch.int32, device=dev) if with_path else None
    s = _lib.make("T2Dtw", a=a, ld_ab=a.stride(0), ld_at=a.stride(1), b=b, ld_bb=b.stride(0), ld_bt=b.stride(1), B=B, Ta=Ta, Tb=Tb, K=K,
                  len_a=torch.as_tensor(la, dtype=torch.int32).to(dev), len_b=torch.as_tensor(lb, dtype=torch.int32).to(dev),
                  scale=float(scale), cost=cost, path_len=plen, back=back, path=path)
    _lib.call("t2_dtw", s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return cost.cpu().numpy(), plen.cpu().numpy(), (path.cpu().numpy() if with_path else None)


@functools.lru_cache(maxsize=None)
def _pair(Ta, Tb, K):
    """(a, b, d64, opt64): a smooth random trajectory, a warped noisy copy of it, their float64 distances and the float64 optimum -
    computed once per shape and shared by the tests that use it."""
    rng = np.random.default_rng(100000 * K + 1000 * Ta + Tb)
    a = R.trajectory(rng, Ta, K)
    b = R.warped_copy(rng, a, Tb, 0.05)
    d = R.distances(a, b, R.MCD_SCALE)
    return a, b, d, R.dtw_matrix(d)[0]


def _check_properties(label, K, d64, opt64, cost, n, path, n_noback, la, lb):
    eps = _eps(K)
    p = path[:n]
    R.check_path(p, la, lb)                                                       # 1
    assert n == n_noback and (path[n:] == -7).all(), (label, n, n_noback)
    on_path = R.path_cost(d64, p)
    e2 = abs(cost - on_path) / on_path
    e3 = (on_path - opt64) / opt64
    print(f"[dtw] {label}: cost {cost:.6f} path_len {n} |cost - sum_path d64| / sum = {e2:.3e} /{eps:.3e}, "
          f"(sum_path d64 - opt64) / opt64 = {e3:.3e} /{2.5 * eps:.3e}")
    assert e2 <= eps, (label, e2, eps)                                            # 2
    assert -1e-12 <= e3 <= 2.5 * eps, (label, e3, 2.5 * eps)                      # 3
    return e2, e3


CASES = [(1, 1, 13), (1, 7, 13), (7, 1, 13), (5, 9, 13), (64, 63, 13), (255, 257, 13), (257, 255, 13), (256, 256, 13),
         (300, 520, 13), (520, 300, 13), (37, 41, 1), (37, 41, 32)]


@pytest.mark.parametrize("Ta,Tb,K", CASES)
def test_dtw_kernel_properties(Ta, Tb, K):
    dev = _dev()
    a, b, d64, opt64 = _pair(Ta, Tb, K)
    ad, bd = torch.from_numpy(a).to(dev)[None], torch.from_numpy(b).to(dev)[None]
    cost, n, path = _dtw(ad, [Ta], bd, [Tb], R.MCD_SCALE, dev)
    cost0, n0, _ = _dtw(ad, [Ta], bd, [Tb], R.MCD_SCALE, dev, with_path=False)
    assert cost0[0] == cost[0]
    _check_properties(f"({Ta},{Tb}) K={K}", K, d64, opt64, float(cost[0]), int(n[0]), path[0], int(n0[0]), Ta, Tb)


def test_dtw_plain_scale_and_exact_ties():
    """scale = 1 is the plain Euclidean DTW; on integer features every distance is exact, so the kernel must reproduce the reference's
    path cell by cell - ties included (the diagonal first, then (i-1, j))."""
    dev = _dev()
    a = np.array([[0.0], [2.0], [3.0]], dtype=np.float32)
    b = np.array([[0.0], [1.0], [2.0], [4.0]], dtype=np.float32)
    cost, n, path = _dtw(torch.from_numpy(a).to(dev)[None], [3], torch.from_numpy(b).to(dev)[None], [4], 1.0, dev)
    assert cost[0] == 2.0 and n[0] == 4 and path[0, :4].tolist() == [[0, 0], [0, 1], [1, 2], [2, 3]]
    rng = np.random.default_rng(9)
    a = rng.integers(0, 3, size=(70, 1)).astype(np.float32)          # many exact ties
    b = rng.integers(0, 3, size=(90, 1)).astype(np.float32)
    rc, rn, rp = R.dtw(a, b)
    cost, n, path = _dtw(torch.from_numpy(a).to(dev)[None], [70], torch.from_numpy(b).to(dev)[None], [90], 1.0, dev)
    assert cost[0] == rc and n[0] == rn and np.array_equal(path[0, :rn], rp)
    z = torch.zeros(1, 5, 3, device=dev)                             # every cell a three-way tie
    cost, n, path = _dtw(z, [5], z[:, :3], [3], 1.0, dev)
    rp = R.dtw_matrix(np.zeros((5, 3)))[1]
    assert cost[0] == 0.0 and n[0] == len(rp) == 5 and np.array_equal(path[0, :5], rp)


def test_dtw_ragged_batch_reads_nothing_behind_the_lengths():
    """B = 6 inside padded Ta = Tb = 520: mixed lengths, one pair with len_b = 0 (all of its rows NaN), NaN behind every length and
    in the gaps of a strided view."""
    dev = _dev()
    K, T, gap = 13, 520, 29
    lens = [(1, 7), (64, 63), (255, 257), (300, 520), (520, 300), (5, 0)]
    B = len(lens)
    fa = torch.full((B, T * K + gap), float("nan"), device=dev)
    fb = torch.full((B, T * (K + 3) + gap), float("nan"), device=dev)
    ad = fa.as_strided((B, T, K), (T * K + gap, K, 1))
    bd = fb.as_strided((B, T, K), (T * (K + 3) + gap, K + 3, 1))       # rows of b further apart than K as well
    for i, (la, lb) in enumerate(lens):
        if la and lb:
            a, b, _, _ = _pair(la, lb, K)
            ad[i, :la] = torch.from_numpy(a).to(dev)
            bd[i, :lb] = torch.from_numpy(b).to(dev)
    la_, lb_ = [x for x, _ in lens], [y for _, y in lens]
    cost, n, path = _dtw(ad, la_, bd, lb_, R.MCD_SCALE, dev)
    cost0, n0, _ = _dtw(ad, la_, bd, lb_, R.MCD_SCALE, dev, with_path=False)
    assert np.isfinite(cost).all() and np.array_equal(cost, cost0)
    for i, (la, lb) in enumerate(lens):
        if la and lb:
            _, _, d64, opt64 = _pair(la, lb, K)
            _check_properties(f"ragged[{i}] ({la},{lb})", K, d64, opt64, float(cost[i]), int(n[i]), path[i], int(n0[i]), la, lb)
    assert cost[5] == 0.0 and n[5] == 0 and n0[5] == 0 and (path[5] == -7).all()          # 4
    # lengths above the padded shape are clipped to it, negative ones to 0
    c2, n2, _ = _dtw(ad[1:2, :64], [99], bd[1:2, :63], [1000], R.MCD_SCALE, dev, with_path=False)
    assert c2[0] == cost[1] and n2[0] == n[1]
    c3, n3, _ = _dtw(ad[1:2], [-3], bd[1:2], [63], R.MCD_SCALE, dev, with_path=False)
    assert c3[0] == 0.0 and n3[0] == 0


# ---- t2_mel_cepstra ---------------------------------------------------------------------------------------------------------------
def _mel(rng, *shape):
    return rng.uniform(np.log(1e-5), 2.0, size=shape).astype(np.float32)       # the front-end's range: ln of a magnitude floored at 1e-5


@pytest.mark.parametrize("T", [1, 63, 257])
@pytest.mark.parametrize("K", [13, 32])
def test_mel_cepstra_kernel_against_float64(T, K):
    from tacotron2_amd import _lib
    dev = _dev()
    M, B = 80, 2
    lens = [T, T // 2]
    rng = np.random.default_rng(10 * T + K)
    x = _mel(rng, B, T + 2, M)
    for b in range(B):
        x[b, lens[b]:] = np.nan
    xd = torch.from_numpy(x).to(dev)[:, :T]                          # a strided view: two more rows per utterance
    w64 = R.basis(M, K)
    wd = torch.from_numpy(w64.astype(np.float32)).to(dev)
    out = torch.full((B, T, K + 1), -7.0, device=dev)                # rows K + 1 apart: the kernel must keep to its K columns
    s = _lib.make("T2MelCeps", mel=xd, ld_b=xd.stride(0), ld_t=xd.stride(1), B=B, T=T, M=M, K=K,
                  len=torch.tensor(lens, dtype=torch.int32, device=dev), basis=wd, out=out, ld_ob=out.stride(0), ld_ot=out.stride(1))
    _lib.call("t2_mel_cepstra", s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(B):
        n = lens[b]
        assert (got[b, n:] == -7.0).all() and (got[b, :, K] == -7.0).all()             # rows behind len and the gap: untouched
        if n:
            xb = x[b, :n].astype(np.float64)
            bound = (M + 2) * U * (np.abs(xb) @ np.abs(w64))                           # the standard dot-product bound
            err = np.abs(got[b, :n, :K] - xb @ w64)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (b, float((err / bound).max()))
    print(f"[mel_cepstra] T={T} K={K}: worst error / bound = {worst:.3e}")


# ---- Engine.mcd_dtw ------------------------------------------------------------------------------------------------------------------
TINY = dict(num_chars=39, encoded_dim=64, encoder_kernel_size=5, num_mels=80, prenet_dim=32, att_rnn_dim=64, att_dim=32,
            rnn_hidden_dim=64, postnet_dim=64, dropout=0.5)
GUARD = 4096


def _engine(dev):
    from tacotron2_amd.model import Tacotron2
    m = Tacotron2(**TINY, device=dev, seed=11)
    m._engine.guard_bytes = GUARD
    m.eval()
    return m._engine


def _log_mels(seed=21):
    """(mel_a, len_a, mel_b, len_b): smooth log-mel-like tracks in the front-end's range and warped noisy copies, B = 3, ragged."""
    rng = np.random.default_rng(seed)
    la, lb = [120, 61, 0], [97, 150, 40]
    A = np.full((3, 130, 80), np.nan, dtype=np.float32)
    Bm = np.full((3, 150, 80), np.nan, dtype=np.float32)
    for i in range(3):
        full = np.clip(-5.0 + 1.5 * R.trajectory(rng, max(la[i], 1), 80), np.log(1e-5), 2.0).astype(np.float32)
        A[i, :la[i]] = full[:la[i]]
        Bm[i, :lb[i]] = np.clip(R.warped_copy(rng, full, lb[i], 0.2), np.log(1e-5), 2.0)
    return A, la, Bm, lb


def test_engine_mcd_dtw_against_the_float64_restatement():
    """Engine.mcd_dtw from log-mels against tests/mcd_dtw_ref.py from the same log-mels.  The bound composes the two above, written
    out from the inputs.  With e_a[i][k] = (M + 2) u sum_m |x_a[i][m]| |w[m][k]| the cepstral error bound of frame i (e_b alike), a
    float64 distance d moves by at most Delta[i][j] = scale (||e_a[i]|| + ||e_b[j]||) (triangle inequality), and the fp32 distance is
    within eps relative of the moved one: along ANY path P, |cost_kernel(P) - cost64(P)| <= E(P) = sum_P (eps (d + Delta) + Delta).
    The kernel's path Pk is optimal under its distances and the reference's P* under the float64 ones, so
        -E(Pk) <= cost_kernel - opt64 <= E(P*)        (cost_kernel <= cost_kernel(P*) <= opt64 + E(P*); opt64 <= cost64(Pk))."""
    dev = _dev()
    eng = _engine(dev)
    K, M = 13, 80
    A, la, Bm, lb = _log_mels()
    Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev)
    la_d, lb_d = torch.tensor(la, device=dev), torch.tensor(lb, device=dev)
    mcd, cost, n, path = eng.mcd_dtw(Ad, la_d, Bd, lb_d, n_ceps=K, return_path=True)
    mcd0, cost0, n0 = eng.mcd_dtw(Ad, la_d, Bd, lb_d, n_ceps=K)
    assert mcd.dtype == torch.float64 and n.dtype == torch.int32 and path.shape == (3, 130 + 150 - 1, 2)
    assert torch.equal(cost, cost0) and torch.equal(n, n0) and torch.equal(mcd.isnan(), mcd0.isnan())
    mcd, cost, n, path = mcd.cpu().numpy(), cost.cpu().numpy(), n.cpu().numpy(), path.cpu().numpy()
    w = R.basis(M, K)
    eps, worst = _eps(K), 0.0
    for i in range(2):
        xa, xb = A[i, :la[i]].astype(np.float64), Bm[i, :lb[i]].astype(np.float64)
        d = R.distances(xa @ w, xb @ w, R.MCD_SCALE)
        opt64, pstar = R.dtw_matrix(d)
        ea = np.linalg.norm((M + 2) * U * (np.abs(xa) @ np.abs(w)), axis=1)
        eb = np.linalg.norm((M + 2) * U * (np.abs(xb) @ np.abs(w)), axis=1)
        delta = R.MCD_SCALE * (ea[:, None] + eb[None, :])
        E = eps * (d + delta) + delta
        pk = path[i, :n[i]]
        R.check_path(pk, la[i], lb[i])
        assert (path[i, n[i]:] == -1).all()
        lo, hi = -R.path_cost(E, pk), R.path_cost(E, pstar)
        diff = cost[i] - opt64
        worst = max(worst, abs(diff) / opt64)
        print(f"[mcd_dtw] pair {i}: mcd {mcd[i]:.6f} dB (float64 {opt64 / len(pstar):.6f}), cost - opt64 = {diff:.3e} in [{lo:.3e}, {hi:.3e}], "
              f"relative {abs(diff) / opt64:.3e}")
        assert lo <= diff <= hi, (i, lo, diff, hi)
        assert mcd[i] == cost[i] / n[i]
    print(f"[mcd_dtw] worst relative cost error {worst:.3e}")
    assert np.isnan(mcd[2]) and cost[2] == 0.0 and n[2] == 0 and (path[2] == -1).all()
    eng.check_persistent_kernels()
    assert eng.guard_check() == [] and {"mcd.ceps_a", "mcd.ceps_b", "dtw.cost", "dtw.path_len", "dtw.back", "dtw.path"} <= set(eng._guards)
    # the public pieces give the same numbers: mel_cepstra (zeros behind the lengths), then dtw under the MCD scale
    ca, cb = eng.mel_cepstra(Ad, la_d, K), eng.mel_cepstra(Bd, lb_d, K)
    assert ca.shape == (3, 130, K) and not ca[0, 120:].any() and not ca[2].any() and bool(torch.isfinite(ca).all())
    c2, n2 = eng.dtw(ca, la_d, cb, lb_d, scale=eng.MCD_SCALE)
    assert np.array_equal(c2.cpu().numpy(), cost) and np.array_equal(n2.cpu().numpy(), n)


def test_engine_mcd_dtw_does_not_depend_on_the_matmul_precision():
    from tacotron2_amd import engine as E
    dev = _dev()
    eng = _engine(dev)
    A, la, Bm, lb = _log_mels(22)
    args = (torch.from_numpy(A).to(dev), torch.tensor(la, device=dev), torch.from_numpy(Bm).to(dev), torch.tensor(lb, device=dev))
    was = E.GEMM_PRECISION[0]
    try:
        E.set_float32_matmul_precision("highest")
        hi = eng.mcd_dtw(*args, return_path=True)
        E.set_float32_matmul_precision("high")
        lo = eng.mcd_dtw(*args, return_path=True)
    finally:
        E.GEMM_PRECISION[0] = was
    for x, y in zip(hi[1:], lo[1:]):
        assert torch.equal(x, y)
    assert torch.equal(hi[0][:2], lo[0][:2])


def test_engine_groups_keep_the_back_workspace_bounded():
    dev = _dev()
    eng = _engine(dev)
    a, b, _, _ = _pair(64, 63, 13)
    ad, bd = torch.from_numpy(a).to(dev)[None].repeat(5, 1, 1), torch.from_numpy(b).to(dev)[None].repeat(5, 1, 1)
    la, lb = torch.tensor([64, 30, 64, 1, 0], device=dev), torch.tensor([63, 63, 20, 63, 63], device=dev)
    whole = eng.dtw(ad, la, bd, lb, return_path=True)
    eng.DTW_BACK_BYTES = 2 * 64 * 63 + 5                # (an instance attribute: room for groups of two pairs)
    grouped = eng.dtw(ad, la, bd, lb, return_path=True)
    assert eng._ws["dtw.back"].numel() == 2 * 64 * 63
    for x, y in zip(whole, grouped):
        assert torch.equal(x, y)
    assert whole[1].tolist()[3:] == [63, 0]


def test_engine_refuses_what_the_kernels_cannot_take():
    dev = _dev()
    eng = _engine(dev)
    one = torch.ones(2, dtype=torch.int32, device=dev)
    a = torch.zeros(2, 5, 13, device=dev)
    mel = torch.zeros(2, 5, 80, device=dev)
    for bad, word in ((lambda: eng.dtw(torch.zeros(2, 4097, 2, device=dev), one, a[:, :, :2], one), "4096"),
                      (lambda: eng.dtw(a, one, torch.zeros(2, 4097, 13, device=dev), one), "b has 4097"),
                      (lambda: eng.dtw(a.double(), one, a, one), "a must be a float32"),
                      (lambda: eng.dtw(a, one, torch.zeros(2, 5, 7, device=dev), one), "agree"),
                      (lambda: eng.dtw(a.transpose(1, 2).contiguous().transpose(1, 2), one, a, one), "contiguous"),
                      (lambda: eng.dtw(a.cpu(), one, a, one), "a must be a tensor on"),
                      (lambda: eng.dtw(a, one.cpu(), a, one), "len_a must be a tensor on"),
                      (lambda: eng.dtw(a, one, a, one.float()), "len_b must be 2 integers"),
                      (lambda: eng.dtw(a, one, a, one[:1]), "len_b must be 2 integers"),
                      (lambda: eng.dtw(a, one, a, one, scale=float("nan")), "scale"),
                      (lambda: eng.dtw(torch.zeros(2, 5, 33, device=dev), one, torch.zeros(2, 5, 33, device=dev), one), "T2_DTW_MAX_K"),
                      (lambda: eng.dtw(a[:, :, None, 0].expand(2, 5, 13), one, a, one), "contiguous"),
                      (lambda: eng.mel_cepstra(mel, one, 0), "n_ceps"),
                      (lambda: eng.mel_cepstra(mel, one, 33), "n_ceps"),
                      (lambda: eng.mel_cepstra(mel, one, 80), "n_ceps"),
                      (lambda: eng.mel_cepstra(mel.double(), one), "mel must be a float32"),
                      (lambda: eng.mel_cepstra(mel, one.cpu()), "lens must be a tensor on"),
                      (lambda: eng.mcd_dtw(mel, one, mel[:, :, :40], one), "one batch"),
                      (lambda: eng.mcd_dtw(mel, one, mel.cpu(), one), "mel_b must be a tensor on")):
        with pytest.raises(ValueError, match=word):
            bad()


# ---- TTSModel.score ---------------------------------------------------------------------------------------------------------------
def test_model_score_on_the_infer_fixture_weights():
    """TTSModel.score on the weights of the reference-generated `infer` fixture (small dims; utterances stop within a few frames):
    the decode is the one forward(teacher_forcing=False) gives, syn_frames is run/test.py's mel_lengths_of, the scores are
    Engine.mcd_dtw's, and a decode scored against ITSELF has mcd = 0 and path_len = syn_frames."""
    from tests.helpers import SMALL, load_golden, params_from
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.model import TTSModel
    from tacotron2_amd.run.test import mel_lengths_of
    dev = _dev()
    tm = TTSModel(lr=1e-3, weight_decay=1e-6, device=dev, dropout=0.5, **SMALL)
    tm.load_checkpoint_dict({"state_dict": {"tacotron2." + k: v for k, v in params_from(load_golden("infer")).items()}})
    tm.train()                                                        # score() must decode in eval mode and put this back
    enc = TextEncoder("!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz", "^", True)
    ids = [torch.tensor(enc.encode(t)) for t in ("Hi there.", "A somewhat longer sentence, Dr. Who!", "Testing: one; two? three.")]
    chars = torch.nn.utils.rnn.pad_sequence(ids, batch_first=True).to(dev)
    lens = torch.tensor([len(i) for i in ids], device=dev)
    rng = np.random.default_rng(5)
    ref_len = torch.tensor([30, 12, 21], device=dev)
    ref = torch.from_numpy(_mel(rng, 3, 30, 16)).to(dev)
    for kw in (dict(), dict(stop_threshold=0.3), dict(attention_window=(1, 3)), dict(forward_attention=True)):
        tm.eval()
        tm.tacotron2._calls = 0
        with torch.no_grad():
            _, post, gates, align = tm(chars, lens, teacher_forcing=False, max_len_override=40, **kw)
        tm.train()
        tm.tacotron2._calls = 0
        post2, sc = tm.score(chars, lens, ref, ref_len, max_len_override=40, **kw)
        assert tm.training and torch.equal(post2, post)
        syn = mel_lengths_of(gates, kw.get("stop_threshold", 0.5))
        assert torch.equal(sc["syn_frames"], syn) and torch.equal(sc["stopped"], syn > 0) and torch.equal(sc["ref_frames"], ref_len)
        print(f"[score] {kw}: syn_frames {syn.tolist()} mcd {sc['mcd'].tolist()} focus {sc['focus_rate'].tolist()}")
        assert kw or bool(sc["stopped"].any())
        eng = tm.tacotron2._engine
        mcd, cost, n = eng.mcd_dtw(post[:, :max(int(syn.max()), 1)], syn, ref, ref_len)
        assert torch.equal(sc["path_len"], n) and torch.equal(sc["mcd"][sc["stopped"]], mcd[sc["stopped"]])
        assert bool(sc["mcd"][~sc["stopped"]].isnan().all()) and bool((sc["mcd"][sc["stopped"]] > 0).all())
        assert bool(((sc["focus_rate"] > 0) & (sc["focus_rate"] <= 1)).all())
        own = tm.tacotron2.score_decode(post, gates, align, lens, post, syn, stop_threshold=kw.get("stop_threshold", 0.5))
        assert torch.equal(own["path_len"].to(torch.int64), syn)
        assert bool((own["mcd"][sc["stopped"]] == 0).all()) and bool(own["mcd"][~sc["stopped"]].isnan().all())
    with pytest.raises(ValueError, match="mel_spectrogram must be"):
        tm.score(chars, lens, ref[:, :, :8], ref_len, max_len_override=40)
    with pytest.raises(ValueError, match="mel_spectrogram_len"):
        tm.score(chars, lens, ref, ref_len[:2], max_len_override=40)
