"""The attention chain kernels (t2_attn_seq_fwd, t2_attn_seq_bwd) called directly through the C ABI and compared, output by
output, with the float64 autograd restatement of tests/attention_chain_ref.py.

Every operand is laid out as include/tacotron2_amd.h says (pmT transposed, th rows padded to L4, gates gate-interleaved, Z with
row stride 4A + Ad, packed weight streams from t2_lstm_pack_fwd / t2_lstm_pack_bwd, x16-tiled copies); the backward is fed
the stashes the forward KERNEL just wrote, so the pair is tested as the engine uses it.  Before the backward everything the
call is documented to write before reading is filled with NaN (dctx_tot, Z slots 0..T-1 and the dq part of slot T, de, G,
din_part, dh_rec, dgates_t slots 0..T-1, and the filter workspace ws_bd), and only what the header tells the caller to zero is
zeroed: a kernel that reads a word it should have written first leaves a NaN in a compared output.  All tensors are plain torch
allocations, so the module runs unchanged under T2_GUARD_BYTES (no guard plumbing: the guard bands belong to the engine's
workspaces).

Metric: attention_chain_ref.per_sample_rel - max over samples of max|got_b - ref_b| / max|ref_b| per output (time-major
outputs per sample over all frames); single-position samples (len = 1: reference exactly zero) are bounded absolutely by
attention_chain_ref.single_position_bounds.  Tolerances: attention_chain_ref.TOL, one constant per output = 16 x the
restatement's own float32-vs-float64 error over the case list (anchored by tests/test_attention_chain_host.py).

Chunked calls: none of the chain's kernels uses atomics on any output - dv_part / dU_part / dpmT are read-modify-write by their
one owning workgroup (old + this frame's sum, frames in a fixed descending order), G / din_part carry the location-path
gradient from one call to the next through memory - so the frames issued as several (t_hi, t_lo) calls, or several
(t_begin, t_end) calls forward, must give BIT-IDENTICAL results to one call; that is what is asserted.

Constants and what they come from (attention_chain_ref.F32_ERR / TOL; the kernels' own worst figures per output are printed by
every test as "[attention chain] <case>: <output> <error> (b<sample>) /<constant>" and tabulated in DESIGN.md 5):
    output     float32 restatement   constant (x 16)
    att_h      7.5e-7                1.20e-5
    ctx        6.5e-7                1.04e-5
    att_c      3.9e-7                6.24e-6
    gates      7.8e-7                1.25e-5
    cum        3.5e-7                5.60e-6
    align      4.4e-7                7.04e-6
    th         8.0e-7                1.28e-5
    dgates     5.8e-7                9.28e-6
    dq         9.8e-7                1.57e-5
    dctx_tot   1.8e-7                2.88e-6
    dpm        1.0e-6                1.60e-5
    dv         7.7e-7                1.23e-5
    dU         8.3e-7                1.33e-5"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_chain_ref as C  # noqa: E402

KL = C.KL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _untile16(xt, B):
    """x16 layout [..., K/16, Bp, 16] (include/tacotron2_amd.h, T2LstmStep.xt) -> (..., B, K)."""
    nch = xt.shape[-3]
    return xt[..., :B, :].transpose(-3, -2).reshape(*xt.shape[:-3], B, nch * 16)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dims(case):
    return tuple(case[k] for k in ("B", "L", "T", "A", "Ad", "Ef"))


def _device_inputs(dev, inp):
    f = lambda x: None if x is None else x.float().contiguous().to(dev)
    d = {k: f(inp[k]) for k in ("W_ih_ctx", "W_hh", "Wq", "U", "v", "pre", "memory", "att_drop", "dh_ext", "dctx_ext1", "dctx_ext2",
                                "dalign")}
    d["pmT"] = f(inp["pm"].transpose(1, 2))
    d["len"] = inp["len"].to(torch.int32).to(dev)
    return d


XP_COL0 = 16      # the second copy of the context goes to columns [16, 16 + Ef) of rows of 16 + Ef + 4 floats


def run_fwd(dev, case, d, packed=True, chunks=None):
    """t2_attn_seq_fwd; returns the raw stashes (device) as a dict.  Everything the call writes is NaN-filled first; slot 0 of
    the time-major stashes is the caller's (zero)."""
    from tacotron2_amd import _lib
    B, L, T, A, Ad, Ef = _dims(case)
    L4, Bp, ldx = (L + 3) // 4 * 4, (B + 15) // 16 * 16, A + Ef
    s = dict(xdec=_nan(dev, T + 1, B, ldx), att_c=_nan(dev, T + 1, B, A), gates=_nan(dev, T, B, 4 * A), align=_nan(dev, B, T, L),
             cum=_nan(dev, T + 1, B, L), th=_nan(dev, T, B, Ad, L4), xproj=_nan(dev, T, B, XP_COL0 + Ef + 4),
             e_part=_nan(dev, B, Ad // 16, L))
    for k in ("xdec", "att_c", "cum"):
        s[k][0] = 0
    wp = xdec_t = None
    if packed:
        segs = (_lib.S["T2Seg"] * 2)()       # in the column order of the xdec row [att_h | ctx]
        segs[0].w = d["W_hh"].data_ptr(); segs[0].ldw = A; segs[0].K = A
        segs[1].w = d["W_ih_ctx"].data_ptr(); segs[1].ldw = Ef; segs[1].K = Ef
        ntpad = (ldx // 16 + 15) // 16 * 16
        wp = _nan(dev, A // 4 * ntpad * 256)
        _lib.call("t2_lstm_pack_fwd", segs, 2, A, wp, _stream())
        # T2LstmStep.xt: pad rows must be finite - zero-filled when B is not a multiple of 16, as the engine does
        xdec_t = torch.zeros(T + 1, ldx // 16, Bp, 16, device=dev) if B != Bp else _nan(dev, T + 1, ldx // 16, Bp, 16)
        xdec_t[0] = 0
        s["xdec_t"] = xdec_t
    seq = _lib.make("T2AttnSeq", B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, Kl=KL, wpacked=wp, W_ih_ctx=d["W_ih_ctx"], ld_wih=Ef,
                    W_hh=d["W_hh"], Wq=d["Wq"], U=d["U"], v=d["v"], pre=d["pre"], pmT=d["pmT"], memory=d["memory"], len=d["len"],
                    att_drop=d["att_drop"], xdec=s["xdec"], att_c=s["att_c"], gates=s["gates"], align=s["align"], cum=s["cum"],
                    th=s["th"], xproj_ctx=s["xproj"].data_ptr() + 4 * XP_COL0, ld_xproj=XP_COL0 + Ef + 4, e_part=s["e_part"],
                    xdec_t=xdec_t)
    for t0, t1 in (chunks or [(0, 0)]):
        seq.t_begin, seq.t_end = t0, t1
        _lib.call("t2_attn_seq_fwd", seq, _stream())
    torch.cuda.synchronize()
    return s


def fwd_to_ref_layout(case, s):
    B, L, T, A, Ad, Ef = _dims(case)
    c = {k: x.cpu() for k, x in s.items()}
    out = dict(att_h=c["xdec"][1:, :, :A], ctx=c["xdec"][1:, :, A:], att_c=c["att_c"][1:],
               gates=c["gates"].view(T, B, A, 4).transpose(2, 3).reshape(T, B, 4 * A), cum=c["cum"][1:], align=c["align"],
               th=c["th"][..., :L].transpose(2, 3))
    return out, c


def run_bwd(dev, case, d, s, tiled, chunks=None):
    """t2_attn_seq_bwd on the forward kernel's stashes `s`; returns the outputs in the reference layouts (CPU) and the raw
    Z / dgates_t.  With `chunks` (descending (t_hi, t_lo) pairs) the NaN fill happens once, before the first call."""
    from tacotron2_amd import _lib
    B, L, T, A, Ad, Ef = _dims(case)
    Bp, ldz = (B + 15) // 16 * 16, 4 * A + Ad

    def pack_bwd(W, ldw, N4, ncols):
        out = _nan(dev, (ncols + 15) // 16 * ((N4 // 16 + 31) // 32 * 32) * 256)
        _lib.call("t2_lstm_pack_bwd", W, ldw, N4, None, 0, 0, ncols, out, _stream())
        return out
    wtp_ctx, wtp_h, wtp_q = pack_bwd(d["W_ih_ctx"], Ef, 4 * A, Ef), pack_bwd(d["W_hh"], A, 4 * A, A), pack_bwd(d["Wq"], A, Ad, A)
    Z = _nan(dev, T + 1, B, ldz)
    Z[T, :, :4 * A] = 0
    Zt = None
    if tiled:
        Zt = _nan(dev, T + 1, 4 * A // 16, Bp, 16)        # pad rows may hold NaN (test_lstm_step_bwd_packed_tiled)
        Zt[T] = 0
    o = dict(dctx_tot=_nan(dev, T, B, Ef), dpmT=torch.zeros(B, Ad, L, device=dev), dv=torch.zeros(B, Ad, device=dev),
             dU=torch.zeros(B, Ad * 2 * KL, device=dev))
    ws = dict(dc=torch.zeros(B, A, device=dev), G=_nan(dev, 2, B, L), de=_nan(dev, B, L), din_part=_nan(dev, B, Ad // 16, 2, L),
              dh_rec=_nan(dev, B, A), ws_bd=_nan(dev, Ad // 16 * 16896))
    sb = _lib.make("T2AttnSeqBwd", B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, Kl=KL, W_ih_ctx=d["W_ih_ctx"], ld_wih=Ef, W_hh=d["W_hh"],
                   Wq=d["Wq"], U=d["U"], v=d["v"], wtp_ctx=wtp_ctx, wtp_h=wtp_h, wtp_q=wtp_q, memory=d["memory"], xdec=s["xdec"],
                   att_c=s["att_c"], gates=s["gates"], align=s["align"], cum=s["cum"], th=s["th"], att_drop=d["att_drop"],
                   dh_ext=d["dh_ext"], ld_dh=A, dctx_ext1=d["dctx_ext1"], ld_dc1=Ef, dctx_ext2=d["dctx_ext2"], ld_dc2=Ef,
                   dgates=Z, dctx_tot=o["dctx_tot"], dq=None, dpmT=o["dpmT"], dv_part=o["dv"], dU_part=o["dU"], dc=ws["dc"],
                   G=ws["G"], de=ws["de"], din_part=ws["din_part"], dh_rec=ws["dh_rec"], dgates_t=Zt, ws_bd=ws["ws_bd"],
                   dalign=d["dalign"])
    for hi, lo in (chunks or [(0, 0)]):
        sb.t_hi, sb.t_lo = hi, lo
        _lib.call("t2_attn_seq_bwd", sb, _stream())
    torch.cuda.synchronize()
    Zc = Z.cpu()
    out = dict(dgates=Zc[:T, :, :4 * A], dq=Zc[1:, :, 4 * A:], dctx_tot=o["dctx_tot"].cpu(), dpm=o["dpmT"].cpu().transpose(1, 2),
               dv=o["dv"].cpu(), dU=o["dU"].cpu().view(B, Ad, 2, KL))
    return out, Zc, (None if Zt is None else Zt.cpu())


def _check(name, got, inp, ref, names):
    errs = C.errors(got, ref, inp["len"], names=names)
    line = ", ".join(f"{k} {e:.2e} (b{b}) /{C.TOL[k]:.1e}" for k, (e, b) in errs.items())
    print(f"[attention chain] {name}: {line}")
    bad = {k: (e, b) for k, (e, b) in errs.items() if not e <= C.TOL[k]}
    sp = C.single_position_violations(got, inp, ref)
    assert not bad and not sp, (f"{name}: outputs over their constant {{output: (per_sample_rel, sample)}} {bad}; "
                                f"single-position samples over their bound [(output, sample, value/bound)] {sp}")


@pytest.mark.parametrize("name", list(C.CASES))
def test_chain_fwd_bwd_against_float64(dev, name):
    """One case of attention_chain_ref.CASES, forward then backward, every stash and every output against float64."""
    case = C.CASES[name]
    B, L, T, A, Ad, Ef = _dims(case)
    inp = C.make_inputs(case)
    ref = C.chain(inp, torch.float64)
    d = _device_inputs(dev, inp)
    s = run_fwd(dev, case, d)
    got, raw = fwd_to_ref_layout(case, s)
    _check(name + " fwd", got, inp, ref, C.FWD_OUTPUTS)
    # the second copy of the context and the x16-tiled copy of xdec hold the same bits; columns around the copy are untouched
    assert torch.equal(raw["xproj"][:, :, XP_COL0:XP_COL0 + Ef], raw["xdec"][1:, :, A:])
    assert bool(torch.isnan(raw["xproj"][:, :, :XP_COL0]).all()) and bool(torch.isnan(raw["xproj"][:, :, XP_COL0 + Ef:]).all())
    assert torch.equal(_untile16(raw["xdec_t"], B), raw["xdec"])
    # align and cum are exactly 0 behind len[b]
    behind = torch.arange(L)[None, :] >= inp["len"][:, None]
    assert float(raw["align"].masked_select(behind[:, None, :].expand(B, T, L)).abs().sum()) == 0.0
    assert float(raw["cum"].masked_select(behind[None].expand(T + 1, B, L)).abs().sum()) == 0.0
    for b in range(B):
        if int(inp["len"][b]) == 1:
            assert torch.equal(raw["cum"][1:, b, 0], torch.arange(1, T + 1, dtype=torch.float32))

    out, Zc, Ztc = run_bwd(dev, case, d, s, tiled=case["tiled"])
    _check(name + " bwd", out, inp, ref, C.BWD_OUTPUTS)
    assert bool(torch.isfinite(Zc[:T, :, :4 * A]).all()) and bool(torch.isfinite(Zc[1:, :, 4 * A:]).all())
    if Ztc is not None:      # the tiled copy holds the same bits as the dgates part of Z
        assert torch.equal(_untile16(Ztc[:T], B), Zc[:T, :, :4 * A])


def _chunks(T, sizes):
    out, hi = [], T
    for n in sizes:
        out.append((hi, hi - n)); hi -= n
    assert hi == 0
    return out


# uneven chunk sizes, time-descending (the forward uses the same sizes ascending)
CHUNKED = [("L33_B17", (1, 4, 2)), ("L433_Ad144_Ef672", (1, 3)), ("mel_tail", (3, 1, 3)), ("shipped_T24", (2, 9, 1, 12)),
           ("L253", (2, 1))]


@pytest.mark.parametrize("name,sizes", CHUNKED)
def test_chain_chunked_calls_are_bit_identical(dev, name, sizes):
    """The frames issued as several (t_begin, t_end) / descending (t_hi, t_lo) calls with uneven sizes against one call: no
    atomics on any output, every accumulation order is fixed, so the results are bit-identical (module docstring).  The NaN
    fill of the workspaces happens once, before the first call."""
    case = C.CASES[name]
    T = case["T"]
    inp = C.make_inputs(case)
    d = _device_inputs(dev, inp)
    s1 = run_fwd(dev, case, d)
    fwd_chunks = [(T - hi, T - lo) for hi, lo in _chunks(T, sizes)]
    s2 = run_fwd(dev, case, d, chunks=fwd_chunks)
    behind = (torch.arange(s1["th"].shape[-1])[None, :] >= inp["len"][:, None])[None, :, None, :].to(dev)
    for k in ("xdec", "att_c", "gates", "align", "cum", "xproj", "xdec_t"):
        assert torch.equal(torch.nan_to_num(s1[k], nan=7.0), torch.nan_to_num(s2[k], nan=7.0)), k
    assert torch.equal(s1["th"].masked_fill(behind, 0.0), s2["th"].masked_fill(behind, 0.0))
    o1, Z1, Zt1 = run_bwd(dev, case, d, s1, tiled=case["tiled"])
    o2, Z2, Zt2 = run_bwd(dev, case, d, s1, tiled=case["tiled"], chunks=_chunks(T, sizes))
    for k in C.BWD_OUTPUTS:
        assert bool(torch.isfinite(o2[k]).all()), k
        assert torch.equal(o1[k], o2[k]), (k, float((o1[k] - o2[k]).abs().max()))
    if Zt1 is not None:
        assert torch.equal(_untile16(Zt1[:T], case["B"]), _untile16(Zt2[:T], case["B"]))


@pytest.mark.parametrize("name", ["L31_B15", "B33_L97", "L193_Ad144", "shipped_T24"])
def test_chain_fwd_two_segment_path(dev, name):
    """wpacked = NULL (two weight segments read in place, no x16-tiled copy) holds the same constants against float64 as the
    packed path, and the backward accepts its stashes."""
    case = C.CASES[name]
    inp = C.make_inputs(case)
    ref = C.chain(inp, torch.float64)
    d = _device_inputs(dev, inp)
    s = run_fwd(dev, case, d, packed=False)
    got, _ = fwd_to_ref_layout(case, s)
    _check(name + " fwd two-segment", got, inp, ref, C.FWD_OUTPUTS)
    out, _, _ = run_bwd(dev, case, d, s, tiled=not case["tiled"])       # the other dgates_t variant than the main test's
    _check(name + " bwd on two-segment stashes", out, inp, ref, C.BWD_OUTPUTS)
