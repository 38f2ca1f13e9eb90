"""Kernel-level parity on the GPU: every call goes through the C ABI (tacotron2_amd._lib) and is compared with a
plain fp32/fp64 torch restatement of the same op on CPU.  Tolerances are fp32 re-association level."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tacotron2_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.fixture(params=["split_bf16x3", "native_f32"])
def gemm_kernel(request):
    """Both GEMM kernels behind t2_gemm: the default (fp32 by error-free 3 x bf16 operand splitting on the bf16 matrix pipe)
    and the f32-input MFMA kernel, held to the SAME fp32 tolerance against float64."""
    from tacotron2_amd import engine
    old = engine.GEMM_NATIVE_FP32[0]
    engine.GEMM_NATIVE_FP32[0] = 1 if request.param == "native_f32" else 0
    yield request.param
    engine.GEMM_NATIVE_FP32[0] = old


@pytest.mark.parametrize("layout", ["nt", "nn", "tn"])
def test_gemm_matmul_precision_levels(dev, layout):
    """T2Gemm.precision = the reference's float32_matmul_precision (run/train.py:170): "highest" keeps all six bf16 partial
    products (fp32-exact operands), "high" three (torch's bf16x3: ~16 significand bits), "medium" one (bf16 operands).  Each
    level is held to its own error class against float64, and the levels must be ordered."""
    from tacotron2_amd import engine
    from tacotron2_amd.engine import gemm
    M, N, K = 300, 260, 1000
    g = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(K, N, generator=g)
    ref = (A.double() @ B.double())
    a_k, b_k = {"nt": (1, 1), "nn": (1, 0), "tn": (0, 0)}[layout]
    Ad = (A if a_k else A.t().contiguous()).to(dev)
    Bd = (B.t().contiguous() if b_k else B).to(dev)
    errs = {}
    try:
        for name in ("highest", "high", "medium"):
            engine.set_float32_matmul_precision(name)
            C = torch.full((M, N), float("nan"), device=dev)
            gemm(Ad, Bd, C, M, N, K, Ad.shape[1], Bd.shape[1], N, a_k=a_k, b_k=b_k)
            torch.cuda.synchronize()
            errs[name] = _rel(C, ref)
    finally:
        engine.set_float32_matmul_precision("highest")
    assert errs["highest"] < 2e-6 and errs["high"] < 5e-5 and errs["medium"] < 2e-2, errs
    assert errs["highest"] < errs["high"] < errs["medium"], errs
    with pytest.raises(ValueError):
        engine.set_float32_matmul_precision("lowest")


@pytest.mark.parametrize("layout", ["nt", "nn", "tn"])
@pytest.mark.parametrize("shape", [(128, 128, 32), (200, 150, 72), (37, 300, 70), (1000, 81, 1536), (260, 4096, 96), (5, 3, 7)])
def test_gemm_layouts(dev, gemm_kernel, layout, shape):
    from tacotron2_amd.engine import gemm
    M, N, K = shape
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(K, N, generator=g)
    ref = (A.double() @ B.double())
    a_k, b_k = {"nt": (1, 1), "nn": (1, 0), "tn": (0, 0)}[layout]
    Ad = (A if a_k else A.t().contiguous()).to(dev)
    Bd = (B.t().contiguous() if b_k else B).to(dev)
    C = torch.full((M, N), float("nan"), device=dev)
    gemm(Ad, Bd, C, M, N, K, Ad.shape[1], Bd.shape[1], N, a_k=a_k, b_k=b_k)
    torch.cuda.synchronize()
    assert _rel(C, ref) < 2e-6


def test_gemm_epilogues(dev, gemm_kernel):
    from tacotron2_amd.engine import gemm
    M, N, K = 300, 200, 256
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    b1, b2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    mask = (torch.rand(M, N, generator=g) > 0.5).float() * 2
    C0 = torch.randn(M, N, generator=g)
    ref = A.double() @ B.double().t()
    Ad, Bd = A.to(dev), B.to(dev)
    # bias + relu + mask
    C = torch.empty(M, N, device=dev)
    gemm(Ad, Bd, C, M, N, K, K, K, N, bias=b1.to(dev), bias2=b2.to(dev), relu=1, mulmask=mask.to(dev), ldmask=N)
    want = torch.relu(ref + b1.double() + b2.double()) * mask.double()
    assert _rel(C, want) < 2e-6
    # plain accumulate with alpha
    C = C0.to(dev).clone()
    gemm(Ad, Bd, C, M, N, K, K, K, N, alpha=0.5, accumulate=1)
    assert _rel(C, C0.double() + 0.5 * ref) < 2e-6
    # split-K atomic accumulate (+ bias counted once)
    C = C0.to(dev).clone()
    gemm(Ad, Bd, C, M, N, K, K, K, N, accumulate=2, splitk=4, bias=b1.to(dev))
    assert _rel(C, C0.double() + ref + b1.double()) < 2e-6
    # batched, strided C
    Bt = 3
    A3 = torch.randn(Bt, 40, 64, generator=g); B3 = torch.randn(Bt, 50, 64, generator=g)
    C3 = torch.empty(Bt, 40, 50, device=dev)
    gemm(A3.to(dev), B3.to(dev), C3, 40, 50, 64, 64, 64, 50, batch=Bt, sA=40 * 64, sB=50 * 64, sC=40 * 50)
    assert _rel(C3, torch.einsum("bmk,bnk->bmn", A3.double(), B3.double())) < 2e-6


def test_gemm_overlapping_rows_is_conv1d(dev, gemm_kernel):
    """lda < K: A rows overlap -> a k=5 'same' Conv1d on the padded channel-last layout."""
    from tacotron2_amd._lib import call
    from tacotron2_amd.engine import gemm
    B, L, Ci, Co = 3, 21, 16, 24
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, L, Ci, generator=g); w = torch.randn(Co, Ci, 5, generator=g); bias = torch.randn(Co, generator=g)
    ref = R.conv1d_cl(x.double(), w.double(), bias.double())
    xp = torch.zeros(B, L + 4, Ci); xp[:, 2:L + 2] = x
    xd, wd = xp.to(dev), w.to(dev)
    wp = torch.empty(Co, 5 * Ci, device=dev)
    call("t2_pack_conv_weight", wd, wp, Co, Ci, 5, 0, torch.cuda.current_stream().cuda_stream)
    raw = torch.zeros(B * (L + 4), Co, device=dev)
    gemm(xd, wp, raw, B * (L + 4) - 4, Co, 5 * Ci, Ci, 5 * Ci, Co, bias=bias.to(dev))
    got = raw.view(B, L + 4, Co)[:, :L]
    assert _rel(got, ref) < 2e-6


@pytest.mark.parametrize("Ci,k,d", [(32, 3, 3), (64, 7, 5), (32, 11, 2)])
def test_gemm_tap_strided_rows_is_dilated_conv1d(dev, gemm_kernel, Ci, k, d):
    """T2Gemm.a_tap_len / a_tap_stride: the K axis of an A row is k blocks of Ci channels that lie d rows apart -> a dilated
    'same' Conv1d (model/hifi_gan.py:60-87) as ONE GEMM, with and without accumulation into the output."""
    from tacotron2_amd.engine import gemm
    L, Co = 137, 40
    g = torch.Generator().manual_seed(d)
    x = torch.randn(L, Ci, generator=g); w = torch.randn(Co, Ci, k, generator=g) / (Ci * k) ** 0.5; bias = torch.randn(Co, generator=g)
    p = (k * d - d) // 2
    xp = torch.zeros(L + 2 * p, Ci, dtype=torch.float64); xp[p:p + L] = x.double()
    ref = bias.double()[None, :].expand(L, -1).clone()
    for j in range(k):
        ref += xp[j * d:j * d + L] @ w[:, :, j].double().t()
    xd = xp.float().to(dev).contiguous()
    wp = w.permute(0, 2, 1).reshape(Co, k * Ci).contiguous().to(dev)
    y = torch.zeros(L, Co, device=dev)
    gemm(xd, wp, y, L, Co, k * Ci, Ci, k * Ci, Co, bias=bias.to(dev), a_tap_len=Ci, a_tap_stride=d * Ci)
    assert _rel(y, ref) < 2e-6
    base = torch.randn(L, Co, generator=g)
    y2 = base.to(dev).clone()
    gemm(xd, wp, y2, L, Co, k * Ci, Ci, k * Ci, Co, bias=bias.to(dev), accumulate=1, a_tap_len=Ci, a_tap_stride=d * Ci)
    assert _rel(y2, ref + base.double()) < 2e-6


@pytest.mark.parametrize("layout", ["nt", "nn", "tn"])
def test_split_gemm_is_as_accurate_as_f32_mfma(dev, layout):
    """The bf16x3-split kernel against the f32-input MFMA kernel on a long reduction (K = 4096) with operands spanning many
    binades and a large common offset (cancellation): both errors are measured against float64, per element relative to
    sum_k |a||b| (the fp32 dot-product error scale); the split kernel must be within 2x of the native one (it is ~10x better) and both far
    below what ANY dropped significand bits would give (bf16x1 ~ 4e-3, bf16x2 ~ 1.5e-5)."""
    from tacotron2_amd import engine
    from tacotron2_amd.engine import gemm
    M, N, K = 256, 384, 4096
    g = torch.Generator().manual_seed(17)
    A = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-12, 12, (M, K), generator=g).float()) + 3.0
    B = torch.randn(K, N, generator=g) * torch.exp2(torch.randint(-12, 12, (K, N), generator=g).float()) - 1.5
    ref = A.double() @ B.double()
    scale = A.double().abs() @ B.double().abs()
    a_k, b_k = {"nt": (1, 1), "nn": (1, 0), "tn": (0, 0)}[layout]
    Ad = (A if a_k else A.t().contiguous()).to(dev)
    Bd = (B.t().contiguous() if b_k else B).to(dev)
    errs = {}
    old = engine.GEMM_NATIVE_FP32[0]
    try:
        for name, native in (("split", 0), ("native", 1)):
            engine.GEMM_NATIVE_FP32[0] = native
            C = torch.empty(M, N, device=dev)
            gemm(Ad, Bd, C, M, N, K, Ad.shape[1], Bd.shape[1], N, a_k=a_k, b_k=b_k)
            torch.cuda.synchronize()
            e = (C.double().cpu() - ref).abs() / scale
            errs[name] = (float(e.max()), float(e.mean()))
    finally:
        engine.GEMM_NATIVE_FP32[0] = old
    # measured: split 6.7e-7 max / 5.6e-8 mean, f32 MFMA 1.2e-5 max / 5.6e-7 mean - the two-accumulator split kernel is the
    # MORE accurate of the two (exact products, small terms kept apart from the large partial sums)
    assert errs["split"][0] < 2e-6 and errs["native"][0] < 5e-5, errs
    assert errs["split"][0] < 2.0 * errs["native"][0] + 1e-8 and errs["split"][1] < 2.0 * errs["native"][1] + 1e-9, errs
    # special values propagate like fp32 arithmetic: zeros stay exact zeros, a NaN / Inf operand poisons its row
    A2 = torch.zeros(64, 64); B2 = torch.randn(64, 64, generator=g); A2[3, 5] = float("inf"); A2[7, 1] = float("nan")
    C2 = torch.empty(64, 64, device=dev)
    gemm(A2.to(dev), B2.t().contiguous().to(dev), C2, 64, 64, 64, 64, 64, 64)
    C2 = C2.cpu()
    assert bool(torch.isnan(C2[7]).all()) and not bool(torch.isfinite(C2[3]).any()) and float(C2[0].abs().max()) == 0.0


@pytest.mark.parametrize("B,H,Ks", [(3, 32, (16, 32)), (32, 1024, (512, 1024)), (64, 256, (256,)), (17, 64, (16, 32, 64))])
def test_lstm_step_fwd(dev, B, H, Ks):
    """The generic (segment-walking) kernel with every epilogue operand: two biases, dropout mask, lengths (rows past theirs
    give exact zeros in h, c and the four stashed gates) and the second h copy with its own leading dimension."""
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(B + H)
    xs = [torch.randn(B, K, generator=g) for K in Ks]
    Ws = [torch.randn(4 * H, K, generator=g) / (K ** 0.5) for K in Ks]
    pre = torch.randn(B, 4 * H, generator=g); b1 = torch.randn(4 * H, generator=g)
    c0 = torch.randn(B, H, generator=g); drop = (torch.rand(B, H, generator=g) > 0.1).float() / 0.9
    b2 = torch.randn(4 * H, generator=g)
    lens = torch.tensor([3 if i % 4 == 1 else 9 for i in range(B)], dtype=torch.int32)
    t = 5
    act = (t < lens)[:, None]
    assert bool(act.any()) and not bool(act.all())
    gates = pre.double() + b1.double() + b2.double()
    for x, W in zip(xs, Ws):
        gates = gates + x.double() @ W.double().t()
    h_ref, c_ref = R.lstm_cell(gates, c0.double())
    h_ref = h_ref * drop.double() * act; c_ref = c_ref * act
    xd = [x.to(dev) for x in xs]; Wd = [W.to(dev) for W in Ws]
    h = torch.empty(B, H, device=dev); c = torch.empty(B, H, device=dev); gs = torch.empty(B, 4 * H, device=dev)
    h2 = torch.full((B, H + 8), -7.0, device=dev)
    st = _lib.make("T2LstmStep", B=B, H=H, nseg=len(Ks), pre=pre.to(dev), ldpre=4 * H, bias1=b1.to(dev), bias2=b2.to(dev),
                   c_prev=c0.to(dev), ldc_prev=H, drop=drop.to(dev), lddrop=H, h_out=h, ldh=H, h_out2=h2, ldh2=H + 8,
                   c_out=c, ldc_out=H, gates_out=gs, ldg=4 * H, len=lens.to(dev), t=t)
    keep = [st.pre, st.bias1]
    for i, (x, W) in enumerate(zip(xd, Wd)):
        st.seg[i].x = x.data_ptr(); st.seg[i].ldx = x.shape[1]; st.seg[i].w = W.data_ptr(); st.seg[i].ldw = W.shape[1]
        st.seg[i].K = x.shape[1]
    _lib.call("t2_lstm_step_fwd", st, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _rel(h, h_ref) < 5e-6 and _rel(c, c_ref) < 5e-6
    i_ref = 1 / (1 + torch.exp(-gates[:, :H])) * act
    assert _rel(gs.view(B, H, 4)[:, :, 0], i_ref) < 5e-6      # gate-interleaved stash [b][u][4] = (i, f, g, o)
    off = ~act[:, 0]
    assert float(h.cpu()[off].abs().max()) == 0.0 and float(c.cpu()[off].abs().max()) == 0.0
    assert float(gs.cpu()[off].abs().max()) == 0.0            # all four gates of the rows past their length
    assert torch.equal(h2[:, :H], h) and float((h2[:, H:] + 7.0).abs().max()) == 0.0


def _tile16(x, Bp):
    """(B, K) -> x16 layout [K/16][Bp][16] (include/tacotron2_amd.h, T2LstmStep.xt)."""
    B, K = x.shape
    out = torch.zeros(K // 16, Bp, 16, dtype=x.dtype)
    out[:, :B] = x.reshape(B, K // 16, 16).permute(1, 0, 2)
    return out


def _untile16(xt, B):
    nch, Bp, _ = xt.shape
    return xt[:, :B].permute(1, 0, 2).reshape(B, nch * 16)


@pytest.mark.parametrize("B,H,Ks,col0", [(32, 1024, (1024, 512), 0), (5, 64, (48,), 16), (64, 128, (128, 64), 0), (19, 32, (32,), 32),
                                          (35, 64, (64,), 0)])
def test_lstm_step_fwd_packed_tiled(dev, B, H, Ks, col0):
    """Packed weight stream + x16-tiled activations in / tiled h out (the product path of the frame loop) against float64;
    the tiled input holds NaN in the rows >= B, which must not leak into any output row.  Every epilogue operand and output is
    in: dropout mask, lengths, gate stash, second h copy.  (64, 128) takes the square-tile kernel, and so does (35, 64), whose
    last row block (rows 32..34) has no fourth tile."""
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(B * 7 + H)
    K = sum(Ks)
    x = torch.randn(B, K, generator=g)
    Ws = [torch.randn(4 * H, k, generator=g) / (K ** 0.5) for k in Ks]
    pre = torch.randn(B, 4 * H, generator=g); b1 = torch.randn(4 * H, generator=g); b2 = torch.randn(4 * H, generator=g)
    c0 = torch.randn(B, H, generator=g)
    drop = (torch.rand(B, H, generator=g) > 0.1).float() / 0.9
    lens = torch.tensor([3 if i % 4 == 1 else 9 for i in range(B)], dtype=torch.int32)
    t = 5
    gates = pre.double() + b1.double() + b2.double() + x.double() @ torch.cat(Ws, 1).double().t()
    h_ref, c_ref = R.lstm_cell(gates, c0.double())
    act = (t < lens)[:, None]
    h_ref = h_ref * drop.double() * act; c_ref = c_ref * act
    gi, gf, gg, go = [gates[:, i * H:(i + 1) * H] for i in range(4)]
    gs_ref = torch.stack([torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)], 2) * act[:, :, None]
    st_ = torch.cuda.current_stream().cuda_stream
    Wd = [W.to(dev) for W in Ws]
    segs = (_lib.S["T2Seg"] * len(Ks))()
    for i, W in enumerate(Wd):
        segs[i].w = W.data_ptr(); segs[i].ldw = W.shape[1]; segs[i].K = W.shape[1]
    ntpad = (K // 16 + 15) // 16 * 16
    wp = torch.empty(H // 4 * ntpad * 256, device=dev)
    _lib.call("t2_lstm_pack_fwd", segs, len(Ks), H, wp, st_)
    Bp = (B + 15) // 16 * 16
    xt = _tile16(x, Bp)
    xt[:, B:] = float("nan")                                   # rows >= B are never read into a valid output row
    xt = xt.to(dev)
    Ht = (col0 + H + 15) // 16 * 16
    ht = torch.full((Ht // 16, Bp, 16), -7.0, device=dev)
    h = torch.empty(B, H, device=dev); c = torch.empty(B, H, device=dev); xd = x.to(dev)
    gs = torch.empty(B, 4 * H, device=dev); hc = torch.full((B, H + 8), -7.0, device=dev)
    keep = [pre.to(dev), b1.to(dev), b2.to(dev), c0.to(dev), lens.to(dev), drop.to(dev)]
    st = _lib.make("T2LstmStep", B=B, H=H, nseg=1, wpacked=wp, pre=keep[0], ldpre=4 * H, bias1=keep[1], bias2=keep[2],
                   c_prev=keep[3], ldc_prev=H, drop=keep[5], lddrop=H, h_out=h, ldh=H, h_out2=hc, ldh2=H + 8, c_out=c, ldc_out=H,
                   gates_out=gs, ldg=4 * H, len=keep[4], t=t, xt=xt, ht_out=ht, ht_col0=col0)
    st.seg[0].x = xd.data_ptr(); st.seg[0].ldx = K; st.seg[0].K = K
    _lib.call("t2_lstm_step_fwd", st, 1, st_)
    torch.cuda.synchronize()
    assert _rel(h, h_ref) < 5e-6 and _rel(c, c_ref) < 5e-6
    assert _rel(gs.view(B, H, 4), gs_ref) < 5e-6               # gate-interleaved stash [b][u][4] = (i, f, g, o)
    assert torch.equal(hc[:, :H], h) and float((hc[:, H:] + 7.0).abs().max()) == 0.0
    got_t = _untile16(ht.cpu(), B)
    assert torch.equal(got_t[:, col0:col0 + H], h.cpu())       # the tiled copy holds the same values
    if col0:
        assert float((got_t[:, :col0] + 7.0).abs().max()) == 0.0   # other columns untouched
    # row-major activations through the same packed kernel give the same result (different load pattern only)
    h2 = torch.empty(B, H, device=dev); c2 = torch.empty(B, H, device=dev); gs2 = torch.empty(B, 4 * H, device=dev)
    st.xt = None; st.ht_out = None; st.h_out = h2.data_ptr(); st.c_out = c2.data_ptr(); st.gates_out = gs2.data_ptr()
    _lib.call("t2_lstm_step_fwd", st, 1, st_)
    torch.cuda.synchronize()
    assert _rel(h2, h_ref) < 5e-6 and _rel(c2, c_ref) < 5e-6 and _rel(gs2.view(B, H, 4), gs_ref) < 5e-6
    assert torch.equal(hc[:, :H], h2)
    if B <= 32:
        assert torch.equal(h2, h)
    else:      # 33..64 rows: the tiled input takes the 32 x 32-tile kernel, row-major input the 64 x 16 one - same sums, two kernels
        assert _rel(h2, h.double().cpu()) < 1e-6


def test_lstm_step_fwd_two_cells_mixed_paths_write_the_tiled_copy(dev):
    """Two cells in one launch, one packed with a tiled h copy and one with plain weights: the launch takes the generic kernel
    for both, and the first cell's tiled copy is written all the same (it shares the stores of the packed kernels)."""
    from tacotron2_amd import _lib
    B, H, K, col0 = 19, 32, 32, 16
    g = torch.Generator().manual_seed(77)
    st_ = torch.cuda.current_stream().cuda_stream
    Bp = (B + 15) // 16 * 16
    steps = (_lib.S["T2LstmStep"] * 2)()
    keep, hs, refs = [], [], []
    ht = torch.full(((col0 + H) // 16, Bp, 16), -7.0, device=dev)
    for i in range(2):
        x = torch.randn(B, K, generator=g); W = torch.randn(4 * H, K, generator=g) / (K ** 0.5)
        pre = torch.randn(B, 4 * H, generator=g); c0 = torch.randn(B, H, generator=g)
        h_ref, _ = R.lstm_cell(pre.double() + x.double() @ W.double().t(), c0.double())
        xd, Wd, pd, cd = x.to(dev), W.to(dev), pre.to(dev), c0.to(dev)
        h = torch.empty(B, H, device=dev)
        wp = None
        if i == 0:
            seg = (_lib.S["T2Seg"] * 1)()
            seg[0].w = Wd.data_ptr(); seg[0].ldw = K; seg[0].K = K
            wp = torch.empty(H // 4 * 16 * 256, device=dev)
            _lib.call("t2_lstm_pack_fwd", seg, 1, H, wp, st_)
        st = _lib.make("T2LstmStep", B=B, H=H, nseg=1, wpacked=wp, pre=pd, ldpre=4 * H, c_prev=cd, ldc_prev=H, h_out=h, ldh=H,
                       xt=_tile16(x, Bp).to(dev) if i == 0 else None, ht_out=ht if i == 0 else None, ht_col0=col0)
        st.seg[0].x = xd.data_ptr(); st.seg[0].ldx = K; st.seg[0].w = Wd.data_ptr(); st.seg[0].ldw = K; st.seg[0].K = K
        keep += [xd, Wd, pd, cd, wp, st]
        steps[i] = st
        hs.append(h); refs.append(h_ref)
    _lib.call("t2_lstm_step_fwd", steps, 2, st_)
    torch.cuda.synchronize()
    for h, h_ref in zip(hs, refs):
        assert _rel(h, h_ref) < 5e-6
    got_t = _untile16(ht.cpu(), B)
    assert torch.equal(got_t[:, col0:col0 + H], hs[0].cpu()) and float((got_t[:, :col0] + 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("B,H,S", [(32, 1024, 9), (5, 64, 6), (17, 128, 4), (64, 1024, 5), (35, 128, 4)])
def test_lstm_seq_fwd_persistent_matches_step_launches(dev, B, H, S):
    """t2_lstm_seq_fwd_persist (ONE weight-stationary launch, workgroups exchanging h through the tiled stash) against the same
    S steps as dependent launches (t2_lstm_seq_fwd) and against float64; the timeout flag must stay clear.  Above 32 rows the
    call runs one launch per block of 32 rows (B = 64: two full blocks; B = 35: a 32-row and a 3-row block)."""
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(B + H + S)
    Bp = (B + 15) // 16 * 16
    W = torch.randn(4 * H, H, generator=g) / (H ** 0.5)
    pre = torch.randn(S, B, 4 * H, generator=g)
    drop = (torch.rand(S, B, H, generator=g) > 0.1).float() / 0.9
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g) * 0.5
    # float64 reference
    h, c = h0.double(), c0.double()
    hs_ref = []
    for s in range(S):
        h, c = R.lstm_cell(pre[s].double() + h @ W.double().t(), c)
        h = h * drop[s].double()
        hs_ref.append(h)
    st = torch.cuda.current_stream().cuda_stream
    Wd = W.to(dev)
    seg = (_lib.S["T2Seg"] * 1)()
    seg[0].w = Wd.data_ptr(); seg[0].ldw = H; seg[0].K = H
    ntpad = (H // 16 + 15) // 16 * 16
    wp = torch.empty(H // 4 * ntpad * 256, device=dev)
    _lib.call("t2_lstm_pack_fwd", seg, 1, H, wp, st)
    outs = {}
    for mode in ("launches", "persistent"):
        ht = torch.zeros(S + 1, H // 16, Bp, 16, device=dev)
        ht[0] = _tile16(h0, Bp).to(dev)
        hrow = torch.zeros(S + 1, B, H, device=dev); hrow[0] = h0.to(dev)
        cs = torch.zeros(S + 1, B, H, device=dev); cs[0] = c0.to(dev)
        gs = torch.zeros(S, B, 4 * H, device=dev)
        pd, dd = pre.to(dev), drop.to(dev)
        stp = _lib.make("T2LstmStep", B=B, H=H, nseg=1, wpacked=wp, pre=pd, ldpre=4 * H, c_prev=cs, ldc_prev=H, drop=dd, lddrop=H,
                        h_out=hrow[1], ldh=H, c_out=cs[1], ldc_out=H, gates_out=gs, ldg=4 * H, xt=ht, ht_out=ht[1], ht_col0=0)
        stp.seg[0].x = hrow.data_ptr(); stp.seg[0].ldx = H; stp.seg[0].w = Wd.data_ptr(); stp.seg[0].ldw = H; stp.seg[0].K = H
        inc = _lib.make("T2LstmStride", pre=B * 4 * H, c_prev=B * H, drop=B * H, h_out=B * H, c_out=B * H, gates_out=B * 4 * H,
                        dt=0, xt=H * Bp, ht_out=H * Bp)
        inc.seg_x[0] = B * H
        if mode == "launches":
            _lib.call("t2_lstm_seq_fwd", stp, inc, 1, S, st)
        else:
            sync = torch.full((320,), 7, dtype=torch.int32, device=dev)         # the call must zero what it polls ...
            sync[256:272] = 0                                                   # ... the sticky timeout flag is the caller's
            _lib.call("t2_lstm_seq_fwd_persist", stp, inc, S, sync, st)
            torch.cuda.synchronize()
            assert int(sync[256]) == 0, "an inter-workgroup wait timed out"
        torch.cuda.synchronize()
        outs[mode] = (hrow.clone(), cs.clone(), gs.clone(), ht.clone())
    for a, b in zip(outs["launches"], outs["persistent"]):
        assert _rel(a, b) < 2e-6
    for s in range(S):
        assert _rel(outs["persistent"][0][s + 1], hs_ref[s]) < 2e-5
        assert _rel(_untile16(outs["persistent"][3][s + 1].cpu(), B), hs_ref[s]) < 2e-5


def _cell_bwd_ref(dh, gates, cp, cc, dc0, H):
    """float64 pointwise cell backward: gates [B, 4H] gate-major (i, f, g, o) activations -> (dgates [B, 4H], dc_prev)."""
    gi, gf, gg, go = [gates[:, i * H:(i + 1) * H].double() for i in range(4)]
    tc = torch.tanh(cc.double())
    dcv = dc0.double() + dh * go * (1 - tc * tc)
    return torch.cat([dcv * gg * gi * (1 - gi), dcv * cp.double() * gf * (1 - gf), dcv * gi * (1 - gg * gg), dh * tc * go * (1 - go)], 1), dcv * gf


@pytest.mark.parametrize("B,H,N4", [(32, 1024, 4096), (7, 48, 192), (33, 64, 256), (17, 528, 64)])
def test_lstm_step_bwd_packed_tiled(dev, B, H, N4):
    """dx = dgates . W + pointwise cell backward on the packed path with x16-tiled gradients in and out, against the same
    step with row-major operands (bit-identical) and float64; with a dropout mask, lengths (rows past theirs give exact zeros
    in the four gate gradients and in dc) and the second gradient copy.  (7, 48) and (33, 64) run the 8-wave kernel; (17, 528)
    is 33 x 2 = 66 workgroups, above the 64-workgroup switch: the 4-wave kernel, as (32, 1024).  Then the plain-store
    products (epi = 0) of two descriptors of different widths in one call."""
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(B + N4)
    W = torch.randn(N4, H, generator=g) / (N4 ** 0.5)
    dg = torch.randn(B, N4, generator=g)
    ext = torch.randn(B, H, generator=g)
    gates = torch.rand(B, 4 * H, generator=g) * 0.8 + 0.1
    cp = torch.randn(B, H, generator=g); cc = torch.randn(B, H, generator=g); dc0 = torch.randn(B, H, generator=g)
    drop = (torch.rand(B, H, generator=g) > 0.1).float() / 0.9
    lens = torch.tensor([3 if i % 4 == 1 else 9 for i in range(B)], dtype=torch.int32)
    t = 5
    act = (t < lens)[:, None]
    assert bool(act.any()) and not bool(act.all())
    st_ = torch.cuda.current_stream().cuda_stream
    Wd = W.to(dev)
    nchpad = (N4 // 16 + 31) // 32 * 32
    wtp = torch.empty((H + 15) // 16 * nchpad * 256, device=dev)
    _lib.call("t2_lstm_pack_bwd", Wd, H, N4, None, 0, 0, H, wtp, st_)
    Bp = (B + 15) // 16 * 16
    dgt = _tile16(dg, Bp); dgt[:, B:] = float("nan"); dgt = dgt.to(dev)
    res = []
    for tiled in (False, True):
        dc = dc0.clone().to(dev)
        dgo = torch.empty(B, 4 * H, device=dev)
        dgo2 = torch.full((B, 2 * 4 * H), -7.0, device=dev)
        dgo_t = torch.zeros(4 * H // 16, Bp, 16, device=dev) if tiled else None
        keep = [dg.to(dev), ext.to(dev), gates.view(B, 4, H).transpose(1, 2).contiguous().view(B, 4 * H).to(dev), cp.to(dev), cc.to(dev),
                drop.to(dev), lens.to(dev)]
        s = _lib.make("T2LstmBwdStep", B=B, H=H, N4=N4, dg_next=keep[0], lddg=N4, W=Wd, ldw=H, wtpacked=wtp, ncols=H, epi=1,
                      ext1=keep[1], ldx1=H, drop=keep[5], lddrop=H, gates=keep[2], ldgs=4 * H, c_prev=keep[3], ldcp=H,
                      c_cur=keep[4], ldcc=H, dc=dc, lddc=H, dg_out=dgo, ldgo=4 * H, dg_out2=dgo2, ldgo2=2 * 4 * H,
                      len=keep[6], t=t, dgt_next=dgt if tiled else None, dgt_out=dgo_t)
        _lib.call("t2_lstm_step_bwd", s, 1, st_)
        torch.cuda.synchronize()
        assert torch.equal(dgo2[:, :4 * H], dgo) and float((dgo2[:, 4 * H:] + 7.0).abs().max()) == 0.0
        res.append((dgo.cpu(), dc.cpu(), None if dgo_t is None else _untile16(dgo_t.cpu(), B)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[1][2], res[1][0])
    dh = (dg.double() @ W.double() + ext.double()) * drop.double()
    ref, dcp_ref = _cell_bwd_ref(dh, gates, cp, cc, dc0, H)
    assert _rel(res[1][0], ref * act) < 5e-6 and _rel(res[1][1], dcp_ref * act) < 5e-6
    off = ~act[:, 0]
    assert float(res[1][0][off].abs().max()) == 0.0 and float(res[1][1][off].abs().max()) == 0.0
    # epi = 0: two descriptors of different widths in ONE call (the workgroups past the narrower one's columns exit), each
    # with both external addends
    widths = (40, 64)
    steps = (_lib.S["T2LstmBwdStep"] * 2)()
    keep2, outs = [dg.to(dev)], []
    for i, nc in enumerate(widths):
        Wn = torch.randn(N4, nc, generator=g) / (N4 ** 0.5)
        e1 = torch.randn(B, nc, generator=g); e2 = torch.randn(B, nc, generator=g)
        Wnd, e1d, e2d = Wn.to(dev), e1.to(dev), e2.to(dev)
        wtn = torch.empty((nc + 15) // 16 * nchpad * 256, device=dev)
        _lib.call("t2_lstm_pack_bwd", Wnd, nc, N4, None, 0, 0, nc, wtn, st_)
        dx = torch.full((B, nc + 8), -7.0, device=dev)
        steps[i] = _lib.make("T2LstmBwdStep", B=B, H=H, N4=N4, dg_next=keep2[0], lddg=N4, W=Wnd, ldw=nc, wtpacked=wtn, ncols=nc,
                             epi=0, ext1=e1d, ldx1=nc, ext2=e2d, ldx2=nc, dx_out=dx, lddx=nc + 8)
        keep2 += [Wnd, wtn, e1d, e2d]          # (the array holds a copy of the struct, not its operand tensors)
        outs.append((dx, dg.double() @ Wn.double() + e1.double() + e2.double()))
    _lib.call("t2_lstm_step_bwd", steps, 2, st_)
    torch.cuda.synchronize()
    for (dx, dx_ref), nc in zip(outs, widths):
        assert _rel(dx[:, :nc], dx_ref) < 5e-6 and float((dx[:, nc:] + 7.0).abs().max()) == 0.0


def test_lstm_step_bwd_generic_matches_packed(dev):
    """The generic (unpacked-weights) backward kernel and the packed one share the pointwise cell: the same inputs through
    both - two external addends (summed before the K shares of the waves in both), dropout mask, lengths, second gradient
    copy - against float64 at the bound of the packed test, with and without the recurrent product, and as plain products."""
    from tacotron2_amd import _lib
    B, H, N4 = 19, 48, 192
    g = torch.Generator().manual_seed(B + N4 + 1)
    W = torch.randn(N4, H, generator=g) / (N4 ** 0.5)
    dg = torch.randn(B, N4, generator=g)
    e1 = torch.randn(B, H, generator=g); e2 = torch.randn(B, H, generator=g)
    gates = torch.rand(B, 4 * H, generator=g) * 0.8 + 0.1
    cp = torch.randn(B, H, generator=g); cc = torch.randn(B, H, generator=g); dc0 = torch.randn(B, H, generator=g)
    drop = (torch.rand(B, H, generator=g) > 0.1).float() / 0.9
    lens = torch.tensor([3 if i % 4 == 1 else 9 for i in range(B)], dtype=torch.int32)
    t = 5
    act = (t < lens)[:, None]
    st_ = torch.cuda.current_stream().cuda_stream
    Wd = W.to(dev)
    wtp = torch.empty((H + 15) // 16 * ((N4 // 16 + 31) // 32 * 32) * 256, device=dev)
    _lib.call("t2_lstm_pack_bwd", Wd, H, N4, None, 0, 0, H, wtp, st_)
    keep = [dg.to(dev), e1.to(dev), e2.to(dev), gates.view(B, 4, H).transpose(1, 2).contiguous().view(B, 4 * H).to(dev), cp.to(dev),
            cc.to(dev), drop.to(dev), lens.to(dev)]

    def run(packed, epi, recurrent=True):
        dc = dc0.clone().to(dev)
        dgo = torch.empty(B, 4 * H, device=dev); dgo2 = torch.full((B, 2 * 4 * H), -7.0, device=dev); dx = torch.empty(B, H, device=dev)
        s = _lib.make("T2LstmBwdStep", B=B, H=H, N4=N4, dg_next=keep[0] if recurrent else None, lddg=N4, W=Wd, ldw=H,
                      wtpacked=wtp if packed else None, ncols=H, epi=epi, ext1=keep[1], ldx1=H, ext2=keep[2], ldx2=H,
                      dx_out=dx, lddx=H, drop=keep[6], lddrop=H, gates=keep[3], ldgs=4 * H, c_prev=keep[4], ldcp=H,
                      c_cur=keep[5], ldcc=H, dc=dc, lddc=H, dg_out=dgo, ldgo=4 * H, dg_out2=dgo2, ldgo2=2 * 4 * H, len=keep[7], t=t)
        _lib.call("t2_lstm_step_bwd", s, 1, st_)
        torch.cuda.synchronize()
        if epi == 0:
            return dx.cpu()
        assert torch.equal(dgo2[:, :4 * H], dgo) and float((dgo2[:, 4 * H:] + 7.0).abs().max()) == 0.0
        return dgo.cpu(), dc.cpu()

    ext = e1.double() + e2.double()
    dx_ref = dg.double() @ W.double() + ext
    off = ~act[:, 0]
    for packed in (False, True):
        assert _rel(run(packed, 0), dx_ref) < 5e-6
        dgo, dc = run(packed, 1)
        ref, dcp_ref = _cell_bwd_ref(dx_ref * drop.double(), gates, cp, cc, dc0, H)
        assert _rel(dgo, ref * act) < 5e-6 and _rel(dc, dcp_ref * act) < 5e-6
        assert float(dgo[off].abs().max()) == 0.0 and float(dc[off].abs().max()) == 0.0
    # no recurrent product (the last step of a sequence): only the generic kernel takes a step without dg_next
    dgo, dc = run(False, 1, recurrent=False)
    ref, dcp_ref = _cell_bwd_ref(ext * drop.double(), gates, cp, cc, dc0, H)
    assert _rel(dgo, ref * act) < 5e-6 and _rel(dc, dcp_ref * act) < 5e-6


def test_lstm_step_bwd_matches_autograd(dev):
    from tacotron2_amd import _lib
    B, H = 19, 48
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(4 * H, H, generator=g) / 7).double().requires_grad_(True)
    pre = torch.randn(B, 4 * H, generator=g).double().requires_grad_(True)
    h0 = torch.randn(B, H, generator=g).double().requires_grad_(True)
    c0 = torch.randn(B, H, generator=g).double().requires_grad_(True)
    drop = (torch.rand(B, H, generator=g) > 0.1).double() / 0.9
    gates = pre + h0 @ W.t()
    h1, c1 = R.lstm_cell(gates, c0)
    h1 = h1 * drop
    dh1 = torch.randn(B, H, generator=g).double(); dc1 = torch.randn(B, H, generator=g).double()
    gpre, gh0, gc0 = torch.autograd.grad((h1 * dh1).sum() + (c1 * dc1).sum(), [pre, h0, c0])
    Hh = H
    acts = torch.cat([torch.sigmoid(gates[:, :Hh]), torch.sigmoid(gates[:, Hh:2 * Hh]), torch.tanh(gates[:, 2 * Hh:3 * Hh]),
                      torch.sigmoid(gates[:, 3 * Hh:])], 1).detach()
    f = lambda t: t.detach().float().to(dev).contiguous()
    dc = f(dc1); dg = torch.empty(B, 4 * H, device=dev)
    s = _lib.make("T2LstmBwdStep", B=B, H=H, N4=4 * H, ncols=H, epi=1, ext1=f(dh1), ldx1=H, drop=f(drop), lddrop=H,
                  gates=f(acts.view(B, 4, H).transpose(1, 2).contiguous().view(B, 4 * H)), ldgs=4 * H, c_prev=f(c0), ldcp=H, c_cur=f(c1), ldcc=H, dc=dc, lddc=H, dg_out=dg, ldgo=4 * H)
    _lib.call("t2_lstm_step_bwd", s, 1, torch.cuda.current_stream().cuda_stream)
    assert _rel(dg, gpre) < 1e-5 and _rel(dc, gc0) < 1e-5
    # recurrent hop: dh0 = dg @ W  (epi=0)
    dx = torch.empty(B, H, device=dev)
    Wd = f(W)
    s2 = _lib.make("T2LstmBwdStep", B=B, H=H, N4=4 * H, dg_next=dg, lddg=4 * H, W=Wd, ldw=H, ncols=H, epi=0, dx_out=dx, lddx=H)
    _lib.call("t2_lstm_step_bwd", s2, 1, torch.cuda.current_stream().cuda_stream)
    assert _rel(dx, gh0) < 1e-5


@pytest.mark.parametrize("B,L,A,Ad,Ef", [(3, 17, 32, 16, 32), (4, 160, 1024, 128, 512), (2, 61, 64, 32, 160)])
def test_attention_step_fwd(dev, B, L, A, Ad, Ef):
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(L)
    P = {"decoder.attention.query_layer.weight": torch.randn(Ad, A, generator=g) / A ** 0.5,
         "decoder.attention.v.weight": torch.randn(1, Ad, generator=g),
         "decoder.attention.location_conv.weight": torch.randn(32, 2, 31, generator=g) / 8,
         "decoder.attention.location_dense.weight": torch.randn(Ad, 32, generator=g) / 6}
    att_h = torch.randn(B, A, generator=g); mem = torch.randn(B, L, Ef, generator=g); pm = torch.randn(B, L, Ad, generator=g)
    w = torch.softmax(torch.randn(B, L, generator=g), 1); cum = w * 2.5
    lens = torch.tensor([L - 3 * i for i in range(B)])
    mask = torch.arange(L)[None] >= lens[:, None]
    Pd_ = {k: v.double() for k, v in P.items()}
    ctx_ref, w_ref = R.attention_fwd(Pd_, att_h.double(), mem.double(), pm.double(), torch.stack([w, cum], 1).double(), mask)
    st = torch.cuda.current_stream().cuda_stream
    f = lambda t: t.float().to(dev).contiguous()
    U = torch.empty(Ad, 2, 31, device=dev)
    Wd, Wc = f(P["decoder.attention.location_dense.weight"]), f(P["decoder.attention.location_conv.weight"])
    _lib.call("t2_attn_fold_location", Wd, Wc, U, Ad, 32, 31, st)
    e_part = torch.empty(B, Ad // 16, L, device=dev); th = torch.empty(B, Ad, (L + 3) // 4 * 4, device=dev)
    w_out = torch.empty(B, L, device=dev); cum_out = torch.empty(B, L, device=dev); ctx = torch.empty(B, Ef, device=dev)
    keep = [f(att_h), f(P["decoder.attention.query_layer.weight"]), f(P["decoder.attention.v.weight"]), f(w), f(cum),
            f(pm.transpose(1, 2)), f(mem), lens.to(torch.int32).to(dev)]
    s = _lib.make("T2AttnStep", B=B, L=L, A=A, Ad=Ad, Ef=Ef, Kl=31, att_h=keep[0], ldh=A, Wq=keep[1], U=U, v=keep[2],
                  w_prev=keep[3], ldw=L, cum_prev=keep[4], ldcum=L, pmT=keep[5], memory=keep[6], len=keep[7],
                  e_part=e_part, th_out=th, w_out=w_out, ldwo=L, cum_out=cum_out, ldco=L, ctx_out=ctx, ldctx=Ef)
    _lib.call("t2_attn_step_fwd", s, st)
    torch.cuda.synchronize()
    assert _rel(w_out, w_ref) < 1e-5 and _rel(ctx, ctx_ref) < 1e-5
    assert _rel(cum_out, cum.double() + w_ref) < 1e-5
    assert float(w_out[1, int(lens[1]):].abs().max()) == 0.0


def test_philox_mask_statistics(dev):
    from tacotron2_amd import _lib
    n = 1 << 20
    m = torch.empty(n, device=dev)
    _lib.call("t2_philox_mask", m, n, 0.5, 1234, 7, torch.cuda.current_stream().cuda_stream)
    vals = torch.unique(m).cpu().tolist()
    assert vals == [0.0, 2.0]
    assert abs(float((m > 0).float().mean()) - 0.5) < 5e-3
    m2 = torch.empty(n, device=dev)
    _lib.call("t2_philox_mask", m2, n, 0.5, 1234, 8, torch.cuda.current_stream().cuda_stream)
    assert float((m != m2).float().mean()) > 0.4


def test_adam_clip_step_matches_oracle(dev):
    """t2_sumsq + t2_adam_step (global-norm clip 1.0, L2-in-gradient weight decay, bias correction) vs the oracle."""
    from tacotron2_amd import _lib
    n = 100003
    g_ = torch.Generator().manual_seed(2)
    p = torch.randn(n, generator=g_); grad = torch.randn(n, generator=g_) * 0.05
    m = torch.zeros(n); v = torch.zeros(n)
    pd_, gd, md, vd = p.to(dev), grad.to(dev), m.to(dev), v.to(dev)
    ss = torch.zeros(1, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for step in (1, 2, 3):
        coef, tot = R.clip_coef([grad], 1.0)
        p, m, v = R.adam_l2_step(p, grad * coef, m, v, step, 1e-3, 1e-6)
        _lib.call("t2_sumsq", gd, n, ss, st)
        _lib.call("t2_adam_step", pd_, gd, md, vd, n, ss, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-6, step, 1.0, st)
        torch.cuda.synchronize()
        assert abs(float(ss.sqrt()) - tot) < 1e-6 * tot
        assert float((pd_.cpu() - p).abs().max()) < 2e-6


def test_logmel_matches_float64_restatement(dev):
    """Device log-mel (DFT as an fp32-MFMA GEMM over overlapping windows) vs the float64 numpy restatement.  PARITY
    UNPINNED against the reference (speech_utils is not available): this pins the build's own definition."""
    import numpy as np
    from oracle.logmel_ref import logmel
    from tacotron2_amd.datasets.logmel import TacotronMelSpectrogram
    rng = np.random.default_rng(3)
    n = 22050 + 777
    t = np.arange(n) / 22050
    wav = (0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t) * np.exp(-3 * t) + 0.01 * rng.normal(size=n))
    wav[5000:5600] = 0.0                                   # digital silence -> exercises the 1e-5 clamp
    ref = logmel(wav)
    fe = TacotronMelSpectrogram(device=dev)
    got = fe(torch.from_numpy(wav.astype(np.float32)), id="0").double().cpu().numpy()
    assert got.shape == ref.shape == (1 + n // 256, 80)
    assert np.abs(got - ref).max() < 2e-3 and np.abs(got - ref).mean() < 1e-4


# ---- Griffin-Lim vocoding on the GEMM kernel (tacotron2_amd/vocoder.py; parity unpinned: properties only) -------------
@pytest.mark.gpu
def test_stft_istft_round_trip_is_exact():
    from tacotron2_amd.vocoder import GriffinLim
    gl = GriffinLim(n_iter=2)
    g = torch.Generator().manual_seed(3)
    y = (torch.rand(256 * 37, generator=g) * 2 - 1).cuda()
    spec = gl.stft(y)
    assert spec.shape == (38, 2, 513)
    # analysis against torch's FFT (same centring, reflect padding and periodic Hann window)
    ref = torch.stft(y.cpu().double(), 1024, 256, 1024, torch.hann_window(1024, periodic=True, dtype=torch.float64),
                     center=True, pad_mode="reflect", return_complex=True).t()
    assert torch.allclose(spec[:, 0].cpu().double(), ref.real, atol=2e-3)
    assert torch.allclose(spec[:, 1].cpu().double(), ref.imag, atol=2e-3)
    back = gl.istft(spec)
    assert back.shape == y.shape
    assert float((back - y).abs().max()) < 1e-4


@pytest.mark.gpu
def test_griffin_lim_converges_and_mel_round_trip():
    from tacotron2_amd.vocoder import GriffinLim
    gl = GriffinLim(n_iter=32)
    t = torch.arange(256 * 60, dtype=torch.float64) / 22050.0
    y = sum(a * torch.sin(2 * math.pi * f * t * (1 + 0.02 * torch.sin(2 * math.pi * 3 * t)))
            for a, f in ((0.4, 220.0), (0.25, 440.0), (0.15, 1320.0), (0.1, 3300.0))).float().cuda()
    spec = gl.stft(y)
    S = torch.sqrt((spec * spec).sum(1))
    out = gl.magnitude_to_audio(S, seed=1)
    assert out.shape == y.shape and bool(torch.isfinite(out).all())
    s2 = gl.stft(out)
    S2 = torch.sqrt((s2 * s2).sum(1))
    conv = float(torch.linalg.norm(S2 - S) / torch.linalg.norm(S))
    assert conv < 0.15, conv                      # spectral convergence after 32 iterations
    # the model-side entry point: log-mel in, audio out, and the audio's log-mel matches where there is energy
    lm = gl.front(y)
    wav = gl.mel_to_audio(lm, seed=2)
    assert wav.shape == y.shape and bool(torch.isfinite(wav).all())
    lm2 = gl.front(wav)
    loud = lm > (lm.max() - 6.0)
    assert float((lm2 - lm)[loud].abs().mean()) < 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,Ci,Co,level", [(32, 872, 80, 512, -5.5), (32, 872, 512, 80, 0.3), (3, 5, 64, 64, 2.0), (7, 61, 32, 200, -1.0)])
def test_batchnorm_statistics_from_the_gemm_epilogue_match_float64(B, L, Ci, Co, level):
    """T2Gemm.stat_out + T2Bn.tile_stats (round 5): the conv-as-GEMM of a postnet layer writes, per 128-row tile and column,
    {shift, sum (v - shift), sum (v - shift)^2} over the tile's real positions (rows of the padded layout with row % (L + 4) < L;
    the junk rows that straddle two samples are excluded), and t2_bn_fwd merges the tiles in double.  Against float64 statistics
    of the SAME fp32 convolution output: mean, 1/std and the running statistics, at the bench's postnet shapes (27,904 positions,
    first layer on a -5.5 log-mel level, last layer with N = 80 < one tile), a tiny padded length (L + 4 < 64: the modulo path) and a
    ragged tile count; and bit-identical normalised outputs to the statistics-kernel path within fp32 rounding of the statistics."""
    from tacotron2_amd import _lib
    from tacotron2_amd._lib import call, make
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 1000 + L)
    Lp = L + 4
    x_pad = torch.zeros(B, Lp, Ci)
    x_pad[:, 2:2 + L] = torch.randn(B, L, Ci, generator=g) * 0.25 + level
    w = torch.randn(Co, 5 * Ci, generator=g) / (5 * Ci) ** 0.5
    bias = torch.randn(Co, generator=g)
    xd, wd, bd = x_pad.to(dev), w.to(dev).contiguous(), bias.to(dev)
    M = B * Lp - 4
    raw = torch.zeros(B * Lp, Co, device=dev)
    ts = torch.full(((M + 127) // 128, 3, Co), float("nan"), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    gm = make("T2Gemm", A=xd, B=wd, C=raw, M=M, N=Co, K=5 * Ci, lda=Ci, ldb=5 * Ci, ldc=Co, a_kmajor=1, b_kmajor=1, alpha=1.0, bias=bd,
              splitk=1, batch=1, stat_out=ts, stat_Lp=Lp, stat_L=L)
    call("t2_gemm", gm, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ts).all())
    valid = (torch.arange(B * Lp, device=dev) % Lp < L) & (torch.arange(B * Lp, device=dev) < M)
    v64 = raw[valid].double()
    n = v64.shape[0]
    assert n == B * L
    mean64, var64 = v64.mean(0), v64.var(0, unbiased=False)
    outs = {}
    for name, use_tiles in (("tiles", True), ("kernel", False)):
        y = torch.empty(B, Lp, Co, device=dev)
        mean, invstd = torch.empty(Co, device=dev), torch.empty(Co, device=dev)
        sums = torch.zeros(2 * Co + 2, dtype=torch.float64, device=dev)
        rm, rv = torch.zeros(Co, device=dev), torch.ones(Co, device=dev)
        bn = make("T2Bn", B=B, L=L, C=Co, x=raw, Lp_x=Lp, gamma=torch.ones(Co, device=dev), beta=torch.zeros(Co, device=dev),
                  running_mean=rm, running_var=rv, training=1, momentum=0.1, eps=1e-5, sums=sums, mean=mean, invstd=invstd, act=2,
                  y=y, Lp_y=Lp, pad_y=2, tile_stats=ts if use_tiles else None, tile_M=M if use_tiles else 0)
        call("t2_bn_fwd", bn, st)
        torch.cuda.synchronize()
        assert float(sums[2 * Co]) == n
        assert float((mean.double() - mean64).abs().max()) < 2e-6 * max(1.0, abs(level) + 1), name
        rel = ((invstd.double() - 1 / torch.sqrt(var64 + 1e-5)).abs() * torch.sqrt(var64 + 1e-5)).max()
        # (the tile path shifts every tile by a value of its own; the statistics kernel shifts the whole layer by the channel's first
        #  value and sums 27,904 terms in fp32 per partial - it is the LESS accurate of the two)
        assert float(rel) < (3e-6 if use_tiles else 2e-5), (name, float(rel))
        assert float((rv.double() - (0.9 + 0.1 * var64 * n / max(n - 1, 1))).abs().max()) < 1e-5
        outs[name] = (y, mean, invstd)
    assert float((outs["tiles"][0] - outs["kernel"][0]).abs().max()) < 2e-5      # same statistics to rounding -> same outputs
    # the epilogue is refused where partial sums of partial products would be meaningless
    gm.splitk = 2; gm.accumulate = 2
    with pytest.raises(_lib.T2Error):
        call("t2_gemm", gm, st)
