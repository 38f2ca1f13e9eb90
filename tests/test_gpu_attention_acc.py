"""The attention backward with its accumulators off the frame chain (t2_attn_seq_bwd_stash + t2_attn_acc_bwd) against the
chain that accumulates in its per-slice launch (t2_attn_seq_bwd), both called through the C ABI on the same forward stashes,
and against the float64 autograd restatement of tests/attention_chain_ref.py.

What must hold:
  * everything that leaves the chain itself - Z (dgates | dq), dctx_tot, the x16-tiled dgates copy - and the location-path carry
    it leaves in its workspaces (G, din_part) is BIT-IDENTICAL between the two paths: the stash path changes none of that
    arithmetic, it only moves `de` to a per-frame slot;
  * dpm, dv, dU of the stash path hold the constants of the existing kernel tests (attention_chain_ref.TOL) against float64;
  * against float64 the stash path's error exceeds the legacy path's on the same inputs by at most F32_ERR[output]: the two paths
    add the same per-frame terms in another association (per-call partial sums in registers, then one add to memory, instead of
    one read-modify-write per frame), and F32_ERR is what one plain float32 evaluation of the chain - any one association - is
    off float64 by over the case list (attention_chain_ref.TOL is 16 x that);
  * the frames given to t2_attn_acc_bwd as one call or as one call per chain chunk both hold the above;
  * texts longer than one pass (L > 252) ignore the stash: every output, accumulators included, is bit-identical to
    t2_attn_seq_bwd, and t2_attn_acc_bwd leaves them alone.

Before each backward every workspace the calls are documented to write before reading is NaN (the de stash included).
Cases: the one-pass cases of attention_chain_ref.CASES (L = 1 .. 252, ragged batches, with and without dalign / att_drop /
dgates_t) and two more at L = 215, 216 around the position-tile width; long texts: L = 253 and L = 433.  Every test prints
"[attention acc] <case>: <output> stash <error> legacy <error> /<constant>" (figures in DESIGN.md 5)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_chain_ref as C  # noqa: E402
from tests import test_gpu_attention_chain as K  # noqa: E402

KL = C.KL
ACC_OUTPUTS = ("dpm", "dv", "dU")
CHAIN_OUTPUTS = ("dgates", "dq", "dctx_tot")

EXTRA = dict([
    C._case("L215", 3, 215, 3, 32, 32, 32, True, True, True, "L = 215: last position below the position-tile width"),
    C._case("L216", 3, 216, 3, 32, 16, 32, False, False, False, "L = 216: the position-tile width, no dalign"),
])
ONE_PASS = ["L1_B1_T1", "L2_T2", "L31_B15", "L32_B16_Ef640", "L33_B17", "B33_L97", "L192", "L193_Ad144", "L215", "L216", "L252",
            "Ad272", "Ad128_T1", "mel_tail", "no_dalign_no_drop", "shipped_T24"]
CHUNKED = [("L33_B17", (1, 4, 2)), ("mel_tail", (3, 1, 3)), ("L215", (2, 1)), ("shipped_T24", (2, 9, 1, 12)), ("L2_T2", (1, 1))]
LONG = [("L253", (2, 1)), ("L433_Ad144_Ef672", (1, 3))]


def _case(name):
    return C.CASES[name] if name in C.CASES else EXTRA[name]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def run_bwd(dev, case, d, s, stash, chunks=None):
    """The backward on the forward kernel's stashes `s`: stash = False: t2_attn_seq_bwd; True: t2_attn_seq_bwd_stash, each chunk
    followed by t2_attn_acc_bwd over the same frames; "late": every chain chunk first, then ONE t2_attn_acc_bwd over all frames.
    Returns the outputs in the reference layouts and the raw words both paths must agree on bit for bit."""
    from tacotron2_amd import _lib
    B, L, T, A, Ad, Ef = K._dims(case)
    Bp, ldz = (B + 15) // 16 * 16, 4 * A + Ad
    nan, st = K._nan, K._stream

    def pack_bwd(W, ldw, N4, ncols):
        out = nan(dev, (ncols + 15) // 16 * ((N4 // 16 + 31) // 32 * 32) * 256)
        _lib.call("t2_lstm_pack_bwd", W, ldw, N4, None, 0, 0, ncols, out, st())
        return out
    wtp_ctx, wtp_h, wtp_q = pack_bwd(d["W_ih_ctx"], Ef, 4 * A, Ef), pack_bwd(d["W_hh"], A, 4 * A, A), pack_bwd(d["Wq"], A, Ad, A)
    Z = nan(dev, T + 1, B, ldz)
    Z[T, :, :4 * A] = 0
    Zt = None
    if case["tiled"]:
        Zt = nan(dev, T + 1, 4 * A // 16, Bp, 16)
        Zt[T] = 0
    o = dict(dctx_tot=nan(dev, T, B, Ef), dpmT=torch.zeros(B, Ad, L, device=dev), dv=torch.zeros(B, Ad, device=dev),
             dU=torch.zeros(B, Ad * 2 * KL, device=dev))
    ws = dict(dc=torch.zeros(B, A, device=dev), G=nan(dev, 2, B, L), de=nan(dev, B, L), din_part=nan(dev, B, Ad // 16, 2, L),
              dh_rec=nan(dev, B, A), ws_bd=nan(dev, Ad // 16 * 16896))
    ld_stash = B * L + 3                        # a stride of its own: slots are not assumed to be packed
    de_stash = nan(dev, T, ld_stash)
    sb = _lib.make("T2AttnSeqBwd", B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, Kl=KL, W_ih_ctx=d["W_ih_ctx"], ld_wih=Ef, W_hh=d["W_hh"],
                   Wq=d["Wq"], U=d["U"], v=d["v"], wtp_ctx=wtp_ctx, wtp_h=wtp_h, wtp_q=wtp_q, memory=d["memory"], xdec=s["xdec"],
                   att_c=s["att_c"], gates=s["gates"], align=s["align"], cum=s["cum"], th=s["th"], att_drop=d["att_drop"],
                   dh_ext=d["dh_ext"], ld_dh=A, dctx_ext1=d["dctx_ext1"], ld_dc1=Ef, dctx_ext2=d["dctx_ext2"], ld_dc2=Ef,
                   dgates=Z, dctx_tot=o["dctx_tot"], dq=None, dpmT=o["dpmT"], dv_part=o["dv"], dU_part=o["dU"], dc=ws["dc"],
                   G=ws["G"], de=ws["de"], din_part=ws["din_part"], dh_rec=ws["dh_rec"], dgates_t=Zt, ws_bd=ws["ws_bd"],
                   dalign=d["dalign"])
    for hi, lo in (chunks or [(T, 0)]):
        sb.t_hi, sb.t_lo = hi, lo
        if not stash:
            _lib.call("t2_attn_seq_bwd", sb, st())
        else:
            _lib.call("t2_attn_seq_bwd_stash", sb, de_stash, ld_stash, st())
            if stash != "late":
                _lib.call("t2_attn_acc_bwd", sb, de_stash, ld_stash, lo, hi, st())
    if stash == "late":
        _lib.call("t2_attn_acc_bwd", sb, de_stash, ld_stash, 0, T, st())
    torch.cuda.synchronize()
    Zc = Z.cpu()
    out = dict(dgates=Zc[:T, :, :4 * A], dq=Zc[1:, :, 4 * A:], dctx_tot=o["dctx_tot"].cpu(), dpm=o["dpmT"].cpu().transpose(1, 2),
               dv=o["dv"].cpu(), dU=o["dU"].cpu().view(B, Ad, 2, KL))
    raw = dict(Z=Zc, dctx_tot=out["dctx_tot"], G=ws["G"].cpu(), din_part=ws["din_part"].cpu(), dc=ws["dc"].cpu(),
               dh_rec=ws["dh_rec"].cpu())
    if Zt is not None:
        raw["Zt"] = Zt.cpu()[:T, :, :B]
    return out, raw, de_stash.cpu()


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """Inputs, float64 reference, the forward kernel's stashes and the legacy backward of one case: computed once, shared by the
    tests of the case, never modified."""
    dev = torch.device("cuda:0")
    case = _case(name)
    inp = C.make_inputs(case)
    ref = C.chain(inp, torch.float64)
    d = K._device_inputs(dev, inp)
    s = K.run_fwd(dev, case, d)
    legacy = run_bwd(dev, case, d, s, stash=False)
    return case, inp, ref, d, s, legacy


def _same_bits(a, b):
    return torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def _compare(tag, name, got, raw, legacy, inp, ref):
    out1, raw1, _ = legacy
    for k in raw1:            # the chain's own outputs and the carry it leaves behind
        assert _same_bits(raw1[k], raw[k]), (tag, k)
    T, A4 = out1["dgates"].shape[0], out1["dgates"].shape[2]
    assert bool(torch.isfinite(raw["Z"][:T, :, :A4]).all()) and bool(torch.isfinite(raw["Z"][1:, :, A4:]).all())
    e_new = C.errors(got, ref, inp["len"], names=ACC_OUTPUTS)
    e_old = C.errors(out1, ref, inp["len"], names=ACC_OUTPUTS)
    print(f"[attention acc] {name} {tag}: " + ", ".join(
        f"{k} stash {e_new[k][0]:.2e} legacy {e_old[k][0]:.2e} /{C.TOL[k]:.1e}" for k in ACC_OUTPUTS))
    for k in ACC_OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), (tag, k)
    bad = {k: e_new[k] for k in ACC_OUTPUTS if not e_new[k][0] <= C.TOL[k]}
    sp = C.single_position_violations(got, inp, ref)
    assert not bad and not sp, (tag, bad, sp)
    worse = {k: (e_new[k][0], e_old[k][0]) for k in ACC_OUTPUTS if not e_new[k][0] <= e_old[k][0] + C.F32_ERR[k]}
    assert not worse, (tag, "error against float64 grew by more than F32_ERR {output: (stash, legacy)}", worse)


@pytest.mark.parametrize("name", ONE_PASS)
def test_stash_path_one_call(dev, name):
    """The chain as one call; the accumulators in ONE t2_attn_acc_bwd over all frames."""
    case, inp, ref, d, s, legacy = _prepared(name)
    got, raw, stash = run_bwd(dev, case, d, s, stash=True)
    _compare("one call", name, got, raw, legacy, inp, ref)
    B, L = case["B"], case["L"]
    assert bool(torch.isfinite(stash[:, :B * L]).all()) and bool(torch.isnan(stash[:, B * L:]).all())   # every slot, nothing behind
    assert bool(torch.isnan(legacy[2]).all())                                                           # null stash: untouched


@pytest.mark.parametrize("name,sizes", CHUNKED)
def test_stash_path_chunked(dev, name, sizes):
    """Uneven chain chunks, each followed by its t2_attn_acc_bwd (the engine's pattern); then the same chunks with one
    accumulate call over all frames at the end."""
    case, inp, ref, d, s, legacy = _prepared(name)
    chunks = K._chunks(case["T"], sizes)
    got, raw, _ = run_bwd(dev, case, d, s, stash=True, chunks=chunks)
    _compare(f"chunks {sizes}", name, got, raw, legacy, inp, ref)
    got, raw, _ = run_bwd(dev, case, d, s, stash="late", chunks=chunks)
    _compare(f"chunks {sizes}, one late accumulate", name, got, raw, legacy, inp, ref)


@pytest.mark.parametrize("name,sizes", LONG)
def test_long_text_ignores_the_stash(dev, name, sizes):
    """L > 252: the position-tiled kernel keeps accumulating in the chain; the stash calls give t2_attn_seq_bwd's bits."""
    case, inp, ref, d, s, legacy = _prepared(name)
    for chunks in (None, K._chunks(case["T"], sizes)):
        got, raw, _ = run_bwd(dev, case, d, s, stash=True, chunks=chunks)
        for k in raw:
            assert _same_bits(legacy[1][k], raw[k]), k
        for k in C.BWD_OUTPUTS:
            assert torch.equal(legacy[0][k], got[k]), k
    K._check(name + " bwd through the stash entries", got, inp, ref, C.BWD_OUTPUTS)


def test_bad_arguments_are_refused(dev):
    from tacotron2_amd import _lib
    lib = _lib.lib()
    x = torch.zeros(64, device=dev)
    sb = _lib.make("T2AttnSeqBwd", B=1, L=4, T=2, A=32, Ad=16, Ef=32, Kl=KL, th=x, align=x, cum=x, v=x, dpmT=x, dv_part=x, dU_part=x)
    import ctypes
    a = ctypes.addressof(sb)
    assert lib.t2_attn_acc_bwd(a, None, 4, 0, 2, None) == 1
    assert lib.t2_attn_acc_bwd(a, x.data_ptr(), 3, 0, 2, None) == 1 and b"ld_stash" in lib.t2_last_error()
    assert lib.t2_attn_acc_bwd(a, x.data_ptr(), 4, 1, 3, None) == 1 and b"frame range" in lib.t2_last_error()
    assert lib.t2_attn_acc_bwd(a, x.data_ptr(), 4, 1, 1, None) == 0            # empty range: nothing to do
