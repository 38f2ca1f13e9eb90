"""t2_gemm (csrc/t2_gemm.hip) called directly through the C ABI (tacotron2_amd._lib.call / make) on the case list of
tests/gemm_ref.py and compared with its float64 restatement of the T2Gemm descriptor: the tile map, split-K, batch, load-path and
epilogue edges of BOTH kernels (T2Gemm.native_fp32 = 0 and 1, set in the struct) and, where named, precision 0, 1 and 2.  Which
path each case takes is recorded by gemm_ref.paths and held by the ledger of tests/test_gemm_ref_host.py, where the argument
rejections are tested too (the library refuses without a GPU); here one test repeats them on device pointers.

Every operand is a plain torch allocation, so the module runs unchanged under T2_GUARD_BYTES.  Inputs are flat buffers in which
every element the header does not say is read holds NaN (padding columns, the elements in front of the base and behind the last
one): an over-read poisons the result.  C lives in a larger buffer, ldc = N + 3 unless the case says otherwise, with sentinel rows in
front of and behind the M x N region and sentinel columns N..ldc; a store-mode call finds NaN in the region; everything outside it
must be bit-identical afterwards.

Metric: max |got - ref64| / scale, scale = |alpha| sum_k |a||b| + |bias| + |bias2| + |C0| (gemm_ref.reference).  Bounds
(gemm_ref.bound): split kernel 2e-6, native kernel 5e-5 (what test_split_gemm_is_as_accurate_as_f32_mfma holds them to at K = 4096),
+ splitk * (batches into one C) * 2^-24 with atomics, + 3 * 2^-16 at precision "high", + 2^-7 at "medium".  Every test prints
"[gemm] <case> <kernel>: <error> /<bound>" and then asserts.

Measured on one MI355X (worst case per family); the whole module, 175 tests, takes 3.3 s:
    family                      bound (split / native)    split kernel                            native kernel
    A tile map                  2e-6 (+ 2^-24) / 5e-5     1.30e-7 (19x3, atomic)                  3.04e-7 (9x3, atomic)
    B K edges, precision 0      2e-6 / 5e-5               1.35e-7 (K = 4, tn, base off by one)    3.16e-7 (K = 63, tn, base off by one)
    B precision 1 (high)        4.78e-5                   2.54e-5 (K = 1)                         -
    B precision 2 (medium)      7.81e-3                   7.26e-3 (K = 1)                         -
    C split-K                   2e-6 + splitk 2^-24       7.60e-8 (K = 512, splitk = 64)          2.01e-7 (tn, K = 83, splitk = 2)
    D batch                     2e-6 / 5e-5 (+ atomics)   1.24e-7 (c, Ef = 42)                    2.18e-7 (e, Ef = 42)
    E epilogue                  2e-6 / 5e-5               1.04e-7 (dense ldc)                     2.57e-7 (accumulate, relu, mask)
    F addressing                2e-6 / 5e-5               5.99e-8 (tap-strided, batch 2)          1.97e-7 (tap-strided)
(the precision 1 and 2 figures are those of the CPU emulation in tests/test_gemm_ref_host.py to three digits: K = 1 leaves the
kernel nothing to round but the operands)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_ref as G  # noqa: E402

KERNELS = list(G.KERNELS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def refs():
    """{case: (desc, bufs, logical operands, float64 reference, scale)} - computed once per case, shared, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            d, bufs, logical = G.make_inputs(G.CASES[name])
            cache[name] = (d, bufs, logical) + G.reference(d, bufs)
        return cache[name]
    return get


def _st():
    return torch.cuda.current_stream().cuda_stream


def _run(dev, descs, bufs, kernel, precision=0, share_cu=0):
    """Fresh device copies of `bufs`, one t2_gemm per descriptor on them in order; the C buffer afterwards (CPU)."""
    from tacotron2_amd import _lib
    dv = {k: v.to(dev) for k, v in bufs.items()}
    assert all(t.data_ptr() % 16 == 0 for t in dv.values())     # (gemm_ref.paths counts an offset of 4 elements as 16-byte aligned)
    ptr = lambda key, off: None if off is None else dv[key].data_ptr() + 4 * off
    for d in descs if isinstance(descs, list) else [descs]:
        g = _lib.make("T2Gemm", A=ptr("A", d["A"]), B=ptr("B", d["B"]), C=ptr("C", d["C"]), bias=ptr("bias", d["bias"]),
                      bias2=ptr("bias2", d["bias2"]), mulmask=ptr("mulmask", d["mulmask"]),
                      native_fp32=int(kernel == "native"), precision=precision, share_cu=share_cu,
                      **{k: d[k] for k in ("M", "N", "K", "lda", "ldb", "ldc", "a_kmajor", "b_kmajor", "alpha", "ldmask", "relu", "accumulate",
                                           "splitk", "batch", "sA", "sB", "sC", "a_tap_len", "a_tap_stride")})
        _lib.call("t2_gemm", g, _st())
    torch.cuda.synchronize()
    return dv["C"].cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _figure(label, d, bufs, cbuf, ref, scale, kernel, precision=0):
    """(label, error, bound) of one call's C buffer; everything outside the M x N regions must still hold its sentinel bits."""
    ic = G.c_index(d)
    outside = torch.ones(cbuf.numel(), dtype=torch.bool)
    outside[ic] = False
    assert int(outside.sum()) >= 4 * d["ldc"]
    assert torch.equal(_bits(cbuf)[outside], _bits(bufs["C"])[outside]), f"{label}: wrote outside the M x N region"
    return (label, G.metric(cbuf[ic], ref, scale), G.bound(d, kernel, precision))


def _check(case, kernel, figures):
    """figures: [(label, error, bound)]; prints them all, then asserts them all."""
    for label, e, b in figures:
        print(f"[gemm] {case}{label} {kernel}: {e:.2e} /{b:.1e}")
    bad = [(k, e, b) for k, e, b in figures if not e <= b]
    assert not bad, f"{case} {kernel}: over their bound [(call, error, bound)] {bad}"


def _family(f):
    return [n for n, c in G.CASES.items() if c["family"] == f]


# -----------------------------------------------------------------------------------------------------------------
# A. tile map
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", [n for n in _family("A") if "batch" not in n])
def test_tile_map_visits_every_tile_once(dev, refs, name, kernel):
    """Store into NaN (a tile the map never visits stays NaN) and accumulate = 2, splitk = 1 into zeros (a tile visited twice
    holds twice its value); the two results are the same bits."""
    d, bufs, lg, ref, scale = refs(name)
    store = _run(dev, d, bufs, kernel)
    d2, bufs2, _ = G.make_inputs(dict(G.CASES[name], accumulate=2, c0="zeros"), logical=lg)
    atomic = _run(dev, d2, bufs2, kernel)
    _check(name, kernel, [_figure(" store", d, bufs, store, ref, scale, kernel), _figure(" atomic", d2, bufs2, atomic, ref, scale, kernel)])
    ic = G.c_index(d)
    assert torch.equal(store[ic], atomic[ic])


@pytest.mark.parametrize("kernel", KERNELS)
def test_tile_map_under_batch_and_splitk(dev, refs, kernel):
    name = "A_tiles_9x3_batch2_splitk3"
    d, bufs, lg, ref, scale = refs(name)
    _check(name, kernel, [_figure("", d, bufs, _run(dev, d, bufs, kernel), ref, scale, kernel)])


# -----------------------------------------------------------------------------------------------------------------
# B. K edges and load paths
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("layout", list(G.LAYOUTS))
@pytest.mark.parametrize("K", G.K_EDGES)
def test_k_edges_in_three_placements(dev, refs, K, layout, kernel):
    """Vector-legal rows (K tail below 4 included), exact odd ld (scalar loads), aligned ld behind a base one float off (guarded
    loads on the interior tile): each within bound of float64, at precision 0, 1 and 2 on the split kernel, the levels strictly
    ordered.  At K = 33 and 64 the three placements give the same bits, a zero A gives exact zeros, share_cu changes nothing."""
    figures, region = [], {}
    for plc in G.PLACEMENTS:
        name = f"B_k{K}_{layout}_{plc}"
        d, bufs, lg, ref, scale = refs(name)
        ic = G.c_index(d)
        errs = {}
        for prec in ((0, 1, 2) if kernel == "split" else (0,)):
            cbuf = _run(dev, d, bufs, kernel, precision=prec)
            fig = _figure(f" {plc} precision {prec}", d, bufs, cbuf, ref, scale, kernel, prec)
            figures.append(fig)
            errs[prec] = fig[1]
            if prec == 0:
                region[plc] = cbuf[ic]
        if kernel == "split":
            assert errs[0] < errs[1] < errs[2], (name, errs)
        if K in (33, 64):
            zero_a = dict(bufs, A=torch.where(torch.isnan(bufs["A"]), bufs["A"], torch.zeros(())))
            assert bool((_run(dev, d, zero_a, kernel)[ic] == 0).all()), f"{name}: a zero A must give exact zeros"
            assert torch.equal(_bits(_run(dev, d, bufs, kernel, share_cu=1)[ic]), _bits(region[plc])), f"{name}: share_cu"
    _check(f"B_k{K}_{layout}", kernel, figures)
    if K in (33, 64):
        assert all(torch.equal(_bits(region["vec"]), _bits(region[p])) for p in ("exact", "off1")), "placements differ in bits"


# -----------------------------------------------------------------------------------------------------------------
# C. split-K, E. epilogue order
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", _family("C") + _family("E"))
def test_splitk_and_epilogue_cases(dev, refs, name, kernel):
    d, bufs, lg, ref, scale = refs(name)
    _check(name, kernel, [_figure("", d, bufs, _run(dev, d, bufs, kernel), ref, scale, kernel)])


# -----------------------------------------------------------------------------------------------------------------
# D. batch
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", _family("D"))
def test_batch_call_patterns(dev, refs, name, kernel):
    """The production call patterns; without atomics the batched call gives the bits of `batch` single calls at the offset pointers."""
    d, bufs, lg, ref, scale = refs(name)
    cbuf = _run(dev, d, bufs, kernel)
    _check(name, kernel, [_figure("", d, bufs, cbuf, ref, scale, kernel)])
    if d["accumulate"] != 2:
        singles = [dict(d, batch=1, sA=0, sB=0, sC=0, A=d["A"] + b * d["sA"], B=d["B"] + b * d["sB"], C=d["C"] + b * d["sC"])
                   for b in range(d["batch"])]
        assert torch.equal(_bits(_run(dev, singles, bufs, kernel)), _bits(cbuf)), f"{name}: batched call differs from single calls"


# -----------------------------------------------------------------------------------------------------------------
# F. addressing features equal their materialised form
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", _family("F"))
def test_overlapping_and_tap_strided_rows_equal_the_gathered_matrix(dev, refs, name, kernel):
    d, bufs, lg, ref, scale = refs(name)
    cbuf = _run(dev, d, bufs, kernel)
    d2, bufs2, _ = G.make_inputs(G.materialised(G.CASES[name], d), logical=lg)
    bufs2["bias"] = bufs["bias"]
    assert d2["a_tap_len"] == 0 and d2["lda"] >= d2["K"] and d2["ldc"] == d["ldc"]
    cbuf2 = _run(dev, d2, bufs2, kernel)
    _check(name, kernel, [_figure("", d, bufs, cbuf, ref, scale, kernel), _figure(" materialised", d2, bufs2, cbuf2, ref, scale, kernel)])
    assert torch.equal(_bits(cbuf), _bits(cbuf2)), f"{name}: differs from the same GEMM on the gathered A"


# -----------------------------------------------------------------------------------------------------------------
# G. argument rejections on device pointers (rc and message: tests/test_gemm_ref_host.py)
# -----------------------------------------------------------------------------------------------------------------
def test_rejected_calls_leave_c_alone_and_a_valid_call_follows(dev):
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(6000)
    A, B = torch.randn(16384, generator=g).to(dev), torch.randn(16384, generator=g).to(dev)
    extra = torch.zeros(16384, device=dev)
    ref = A[:4096].view(64, 64).double().cpu() @ B[:4096].view(64, 64).double().cpu().t()
    scale = A[:4096].view(64, 64).double().cpu().abs() @ B[:4096].view(64, 64).double().cpu().abs().t()
    for name, overrides, words in G.REJECTIONS:
        C = torch.full((16384,), G.SENTINEL, device=dev)
        with pytest.raises(_lib.T2Error, match="rc=1.*t2_gemm.*" + words):
            _lib.call("t2_gemm", G.rejected_call(_lib.make, overrides, A, B, C, extra), _st())
        torch.cuda.synchronize()
        assert bool((C == G.SENTINEL).all()) and bool((extra == 0).all()), name
        kernel = G.KERNELS[len(name) % 2]
        _lib.call("t2_gemm", G.rejected_call(_lib.make, dict(native_fp32=int(kernel == "native")), A, B, C, extra), _st())
        torch.cuda.synchronize()
        e = G.metric(C[:4096].view(64, 64).cpu(), ref, scale)
        assert e <= G.BASE_BOUND[kernel] and bool((C[4096:] == G.SENTINEL).all()), (name, kernel, e)
