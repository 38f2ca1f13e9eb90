"""The decode loop's kernels (csrc/t2_infer.hip: t2_decoder_infer with the linear_rows kernel and the stop logic behind it,
t2_linear_rows, the stop scans) called directly through the C ABI and compared with the float64 restatement of
tests/decode_chain_ref.py.  No engine: every operand is a plain torch allocation laid out as include/tacotron2_amd.h says (x16-tiled
state and operand copies, packed weight streams from t2_lstm_pack_fwd, pmT transposed), so the module runs unchanged under
T2_GUARD_BYTES.

Everything a call writes is NaN-filled first (the pad columns of proj, the rows of proj and align at t >= t1, p1, p1_t, att_h, xproj,
e_part, slot 1 of att_c / dec_c / cum, frame 0's two prenet masks, which the header says are never read); only what the header tells
the caller to zero is zeroed (xs, slot 0 of att_c / dec_c / cum, done, state; with zoneout att_h and xproj; with the attention window
win_peak, and align, whose positions outside the window the windowed step does not write).

Metric: attention_chain_ref.per_sample_rel per output.  Tolerances: decode_chain_ref.TOL = 16 x the restatement's own
float32-vs-float64 error over the case list (anchored by tests/test_decode_chain_host.py).  `done` and `state` are compared exactly:
the cases keep every float64 stop logit 100 x TOL[stop] x max|logit| away from the threshold (asserted by the host test).

Constants and what they come from (every test prints "[decode chain] <case>: <output> <error> /<constant>"):
    output   float32 restatement   constant (x 16)   kernels, measured (worst case)
    mel      6.5e-7                1.04e-5           6.36e-7 (B64)
    stop     1.4e-6                2.24e-5           3.76e-6 (K1024)
    align    3.6e-7                5.76e-6           3.12e-7 (B64)
    xproj    3.9e-7                6.24e-6           3.65e-7 (no_mask)
    att_h    5.1e-7                8.16e-6           7.68e-7 (forward)
    att_c    6.3e-7                1.01e-5           4.15e-7 (zoneout)
    dec_c    3.8e-7                6.08e-6           5.06e-7 (K1024)
    cum      1.6e-7                2.56e-6           2.52e-7 (B5, row-major operands)
    xs       7.0e-7                1.12e-5           5.58e-7 (B64)
    t2_linear_rows (max error / max|reference|)  -  2e-6           2.96e-7 (B = 65, N = 81, K = 784)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import decode_chain_ref as DC  # noqa: E402
from tests import loss_options_ref as LR  # noqa: E402

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def refs():
    """{case: (inputs, folded operands, float64 reference)} - computed once per case, shared by the tests, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            case = DC.CASES[name]
            inp = DC.make_inputs(case)
            comb = DC.build_comb(inp)
            cache[name] = (inp, comb, DC.decode(case, inp, comb))
        return cache[name]
    return get


def _pack(dev, segs, H):
    """t2_lstm_pack_fwd of [(tensor, column offset, ld, K)] -> packed stream [H/4][NTpad][64][4]."""
    from tacotron2_amd import _lib
    arr = (_lib.S["T2Seg"] * len(segs))()
    for i, (w, col0, ld, K) in enumerate(segs):
        arr[i].w = w.data_ptr() + 4 * col0; arr[i].ldw = ld; arr[i].K = K
    ntpad = (sum(s[3] for s in segs) // 16 + 15) // 16 * 16
    out = torch.full((H // 4 * ntpad * 256,), NAN, device=dev)
    _lib.call("t2_lstm_pack_fwd", arr, len(segs), H, out, _st())
    return out


def setup(dev, case, inp, comb, tiled=("comb", "pre2", "p1")):
    """The operand block of one case and every buffer behind it: (T2Infer, {name: device tensor})."""
    from tacotron2_amd import _lib
    B, T, P, A, Ef, D, Ad, M, L = (case[k] for k in ("B", "T", "P", "A", "Ef", "D", "Ad", "M", "L"))
    Bp, Tcap, ldo = (B + 15) // 16 * 16, T + 2, (M + 1 + 3) // 4 * 4
    f = lambda x: None if x is None else x.float().contiguous().to(dev)
    nan = lambda *s: torch.full(s, NAN, device=dev)
    zoned, window = case["zone_p"] != 0.0, case["window"]
    w = {k: f(inp[k]) for k in ("W_pre2", "W_ih_att", "W_hh_att", "b_att_ih", "b_att_hh", "W_ih_dec", "W_hh_dec", "b_dec_ih", "b_dec_hh",
                                "Wq", "U", "v", "memory", "dec_pre")}
    w.update({k: f(x) for k, x in comb.items()})
    w["pmT"] = f(inp["pm"].transpose(1, 2))
    w["len"] = inp["len"].to(torch.int32).to(dev)
    w["W_comb_t"] = f(DC.tile_comb(comb["W_comb"], D, Ef)) if "comb" in tiled else None
    w["W_pre2_t"] = f(DC.tile16(inp["W_pre2"])) if "pre2" in tiled else None
    # packed in the column order of the tiled state: [prenet | att_h | ctx] and [att_h | ctx | dec_h]
    w["wp_att"] = _pack(dev, [(w["W_ih_att"], 0, P + Ef, P), (w["W_hh_att"], 0, A, A), (w["W_ih_att"], P, P + Ef, Ef)], A)
    w["wp_dec"] = _pack(dev, [(w["W_ih_dec"], 0, A + Ef, A), (w["W_ih_dec"], A, A + Ef, Ef), (w["W_hh_dec"], 0, D, D)], D)
    pmask = None
    if inp["prenet_mask"] is not None:
        pmask = f(inp["prenet_mask"])
        pmask[0] = NAN                                    # frame 0's masks are never read
    s = dict(xs=torch.zeros(2, (P + A + Ef + D) // 16, Bp, 16, device=dev),
             att_h=torch.zeros(B, A, device=dev) if zoned else nan(B, A),
             xproj=torch.zeros(B, D + Ef, device=dev) if zoned else nan(B, D + Ef),
             att_c=nan(2, B, A), dec_c=nan(2, B, D), cum=nan(2, B, L), p1=nan(B, P), e_part=nan(B, Ad // 16, L),
             p1_t=nan(P // 16, Bp, 16) if "p1" in tiled else None,
             proj=nan(Tcap, B, ldo), align=torch.zeros(B, Tcap, L, device=dev) if window else nan(B, Tcap, L),
             done=torch.zeros(B, dtype=torch.int32, device=dev), state=torch.zeros(2, dtype=torch.int32, device=dev))
    for k in ("att_c", "dec_c", "cum"):
        s[k][0] = 0
    opt = {}
    if zoned:
        s["zone_att"], s["zone_dec"] = torch.full((B, A), case["zone_p"], device=dev), torch.full((B, D), case["zone_p"], device=dev)
        opt.update(zone_p=case["zone_p"], zone_att=s["zone_att"], zone_dec=s["zone_dec"])
    if window:
        s["win_peak"] = torch.zeros(2, B, dtype=torch.int32, device=dev)
        opt.update(win_back=window[0], win_fwd=window[1], win_peak=s["win_peak"])
    a = _lib.make("T2Infer", B=B, L=L, A=A, D=D, Ef=Ef, Ad=Ad, P=P, M=M, Kl=DC.KL, Tcap=Tcap, W_comb=w["W_comb"], b_comb=w["b_comb"],
                  row_comb=w["row_comb"], W_pre2=w["W_pre2"], W_comb_t=w["W_comb_t"], W_pre2_t=w["W_pre2_t"], p1_t=s["p1_t"],
                  wp_att=w["wp_att"], b_att_ih=w["b_att_ih"], b_att_hh=w["b_att_hh"], wp_dec=w["wp_dec"], b_dec_ih=w["b_dec_ih"],
                  b_dec_hh=w["b_dec_hh"], Wq=w["Wq"], U=w["U"], v=w["v"], pmT=w["pmT"], memory=w["memory"], len=w["len"],
                  prenet_mask=pmask, xs=s["xs"], att_h=s["att_h"], att_c=s["att_c"], dec_c=s["dec_c"], cum=s["cum"], xproj=s["xproj"],
                  p1=s["p1"], e_part=s["e_part"], proj=s["proj"], ld_proj=ldo, align=s["align"], done=s["done"], state=s["state"],
                  dec_pre=w["dec_pre"], forward=int(case["forward"]), stop_logit=DC.threshold(case), **opt)
    a._keep += list(w.values())
    return a, {k: x for k, x in s.items() if x is not None}


def run(dev, case, inp, comb, calls=None, after=None, **kw):
    """t2_decoder_infer over `calls` ((t0, t1) pairs; default: one call over all frames); returns the buffers on the CPU.
    after(t0, t1, device buffers) runs behind each call (synchronised)."""
    from tacotron2_amd import _lib
    a, s = setup(dev, case, inp, comb, **kw)
    for t0, t1 in (calls or [(0, case["T"])]):
        _lib.call("t2_decoder_infer", a, t0, t1, _st())
        torch.cuda.synchronize()
        if after is not None:
            after(t0, t1, s)
    return {k: x.cpu() for k, x in s.items()}


def outputs(case, s, T=None):
    """The compared outputs in the reference's layouts."""
    T, B, M = case["T"] if T is None else T, case["B"], case["M"]
    cur = T & 1
    return dict(mel=s["proj"][:T, :, :M], stop=s["proj"][:T, :, M], align=s["align"][:, :T], xproj=s["xproj"], att_h=s["att_h"],
                att_c=s["att_c"][cur], dec_c=s["dec_c"][cur], cum=s["cum"][0 if case["window"] else cur], xs=DC.untile16(s["xs"], B))


def check(name, case, s, ref, lens):
    """Every output against float64 with its constant; done / state exactly; the NaN canaries and the copies."""
    T, B, P, A, Ef, D, M = (case[k] for k in ("T", "B", "P", "A", "Ef", "D", "M"))
    got = outputs(case, s)
    errs = DC.errors(got, ref)
    print(f"[decode chain] {name}: " + ", ".join(f"{k} {e:.2e} (b{b}) /{DC.TOL[k]:.1e}" for k, (e, b) in errs.items()))
    bad = {k: (e, b) for k, (e, b) in errs.items() if not e <= DC.TOL[k]}
    assert not bad, f"{name}: outputs over their constant {{output: (per_sample_rel, sample)}} {bad}"
    done, state = DC.stop_rule(ref["stop"], DC.threshold(case))
    assert torch.equal(s["done"], done) and torch.equal(s["state"], state), (name, s["done"].tolist(), s["state"].tolist())
    # canaries: pad columns of proj, rows behind the last frame, the other cum slot of the windowed loop, pad rows of the tiled state
    assert bool(torch.isnan(s["proj"][:, :, M + 1:]).all()) and bool(torch.isnan(s["proj"][T:]).all()), name
    if case["window"]:
        assert float(s["align"][:, T:].abs().sum()) == 0.0 and bool(torch.isnan(s["cum"][1]).all()), name
    else:
        assert bool(torch.isnan(s["align"][:, T:]).all()), name
    assert float(s["xs"][:, :, B:].abs().sum()) == 0.0, name
    # the row-major copies hold the bits of the tiled state: att_h / ctx of the last frame in slot T&1, its dec_h in slot (T-1)&1
    xs = got["xs"]
    assert torch.equal(s["att_h"], xs[T & 1, :, P:P + A]) and torch.equal(s["xproj"][:, D:], xs[T & 1, :, P + A:P + A + Ef]), name
    assert torch.equal(s["xproj"][:, :D], xs[(T - 1) & 1, :, P + A + Ef:]), name
    # the prenet scratch after the call's tail: the unmasked first layer; its tiled copy holds the same bits
    e, b = DC.per_sample_rel(s["p1"], ref["p1"])
    assert e <= DC.TOL["xs"], (name, "p1", e, b)
    if "p1_t" in s:
        assert torch.equal(DC.untile16(s["p1_t"], B), s["p1"]), name
    # align and cum are exactly 0 behind len[b]
    behind = torch.arange(case["L"])[None, :] >= lens[:, None]
    assert float(got["align"].masked_select(behind[:, None, :].expand_as(got["align"])).abs().sum()) == 0.0, name
    assert float(got["cum"].masked_select(behind).abs().sum()) == 0.0, name
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the chain against float64;  4. the long-K kernel;  5. options
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.CHAIN + ("K1024",) + DC.OPTIONS)
def test_decode_chain_against_float64(dev, refs, name):
    """T frames in one call: B = 1, 5, 17, 64 (one partial row block, a second one, the full group); D = Ef = 512 (K = 1024: the
    8-wave instance of the combined linear); each option once at B = 5."""
    case = DC.CASES[name]
    inp, comb, ref = refs(name)
    check(name, case, run(dev, case, inp, comb), ref, inp["len"])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the row-major fallback of the two small linears
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B5", "B17"])
def test_row_major_operands(dev, refs, name):
    """W_comb_t = W_pre2_t = p1_t = NULL, and W_pre2_t = NULL alone, hold the same constants against float64.  With W_pre2_t = NULL
    alone the combined linear is the tiled one, so the second prenet layer is fed the same p1 bits; its row-major branch walks the same
    chunks in the same waves (chunk c of row b is x[b][16c .. 16c+15] in either layout, the wave / round / lane split depends on K
    alone), so the prenet columns of the state - and with them every output of the loop - are bit-identical to the tiled run.  With
    W_comb_t = NULL the combined linear's K order is [dec_h | ctx] against [ctx | dec_h] of the tiled operand: another chunk-to-wave
    mapping, another summation order, so that variant is held to the constants only."""
    case = DC.CASES[name]
    inp, comb, ref = refs(name)
    full = run(dev, case, inp, comb)
    check(name + " tiled", case, full, ref, inp["len"])
    rm = run(dev, case, inp, comb, tiled=())
    check(name + " row-major", case, rm, ref, inp["len"])
    pre2 = run(dev, case, inp, comb, tiled=("comb", "p1"))
    check(name + " W_pre2_t = NULL", case, pre2, ref, inp["len"])
    P = case["P"]
    assert torch.equal(DC.untile16(pre2["xs"], case["B"])[:, :, :P], DC.untile16(full["xs"], case["B"])[:, :, :P])
    for k in full:
        assert torch.equal(torch.nan_to_num(pre2[k], nan=7.0), torch.nan_to_num(full[k], nan=7.0)), (name, k)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. chunked calls are bit-exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B5", "B17", "window", "zoneout"])
def test_chunked_calls_are_bit_identical(dev, refs, name):
    """Frames [0, T) as one call and as (0,1)(1,2)(2,2)(2,5)(5,T): the call's tail writes row t1-1 and the next call's first launch
    recomputes it bit for bit, every sum runs in a fixed order - so every buffer is bit-identical.  The empty call leaves every buffer
    untouched; behind each partial call state[1] == t1 and proj row t1-1 is final."""
    case = DC.CASES[name]
    T = case["T"]
    inp, comb, ref = refs(name)
    one = run(dev, case, inp, comb)
    snap = {}

    def after(t0, t1, s):
        c = {k: x.cpu() for k, x in s.items()}
        if t0 == t1:
            for k, x in c.items():
                assert torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(snap[k], nan=7.0)), (name, "empty call wrote", k)
        else:
            assert int(c["state"][1]) == t1, (name, t1, c["state"].tolist())
            assert torch.equal(c["proj"][t1 - 1, :, :case["M"] + 1], one["proj"][t1 - 1, :, :case["M"] + 1]), (name, "proj row", t1 - 1)
            assert bool(torch.isnan(c["proj"][t1:]).all()), (name, "rows behind the call", t1)
            done, state = DC.stop_rule(ref["stop"][:t1], DC.threshold(case))
            assert torch.equal(c["done"], done) and torch.equal(c["state"], state), (name, t1)
        snap.update(c)

    calls = [(0, 1), (1, 2), (2, 2), (2, 5), (5, T)]
    many = run(dev, case, inp, comb, calls=calls, after=after)
    for k in ("proj", "align", "done", "state", "xs", "att_c", "dec_c", "cum", "att_h", "xproj", "p1", "p1_t"):
        assert torch.equal(torch.nan_to_num(many[k], nan=7.0), torch.nan_to_num(one[k], nan=7.0)), (name, k)
    check(name + " chunked", case, many, ref, inp["len"])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev, refs):
    """rc = 1 before anything is launched: B = 65, a width that is no multiple of 16, forward together with win_peak, zone_p without
    its blocks, t1 < t0."""
    from tacotron2_amd import _lib
    case = DC.CASES["B5"]
    inp, comb, _ = refs("B5")
    big = dict(case, B=65)
    inp65 = DC.make_inputs(big)

    def refused(case, inp, comb, change, t0=0, t1=2):
        a, s = setup(dev, case, inp, comb)
        change(a, s)
        before = {k: x.clone() for k, x in s.items()}
        with pytest.raises(_lib.T2Error, match="rc=1"):
            _lib.call("t2_decoder_infer", a, t0, t1, _st())
        torch.cuda.synchronize()
        for k, x in s.items():
            assert torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(before[k], nan=7.0)), k

    refused(big, inp65, DC.build_comb(inp65), lambda a, s: None)                    # every buffer sized for the 65 rows
    for width in ("P", "A", "Ef", "D"):
        refused(case, inp, comb, lambda a, s, width=width: setattr(a, width, getattr(a, width) - 8))

    def both(a, s):
        a.forward = 1
        s["win_peak"] = torch.zeros(2, case["B"], dtype=torch.int32, device=dev)
        a.win_peak = s["win_peak"].data_ptr()
    refused(case, inp, comb, both)
    refused(case, inp, comb, lambda a, s: setattr(a, "zone_p", 0.1))
    refused(case, inp, comb, lambda a, s: None, t0=3, t1=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. t2_linear_rows against float64
# ---------------------------------------------------------------------------------------------------------------------------
# (B, N, K, bias, relu, mask).  K / 16 chunks are split over 4 waves (8 from K = 1024) in rounds of 12 chunks per wave: K = 16 and 48
# leave waves without a chunk, 768 is exactly one round of 4 waves and 784 one chunk into the second, 1008 / 1024 the last 4-wave and the
# first 8-wave shape, 1536 exactly one round of 8 waves and 1552 one chunk into the second.  Every K comes with a row tail (B % 16 != 0)
# and a column tail (N % 16 != 0); B = 65 and 130 are split into launches of 64 rows.
LINEAR_SHAPES = [(17, 49, 16, True, True, True), (1, 1, 16, False, False, False), (15, 1, 48, True, False, True),
                 (16, 81, 48, False, True, False), (17, 49, 768, False, True, True), (65, 81, 784, True, True, False),
                 (64, 49, 784, True, False, True), (17, 81, 1008, True, True, True), (17, 49, 1024, False, False, True),
                 (130, 49, 1536, True, True, True), (15, 81, 1552, True, False, False), (17, 1, 1552, False, True, True)]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("B,N,K,bias,relu,mask", LINEAR_SHAPES)
def test_linear_rows_against_float64(dev, B, N, K, bias, relu, mask):
    """One dot product per element: the 2e-6 class of the GEMM tests of tests/test_gpu_kernels.py (error relative to the output's
    maximum).  Strides larger than needed with NaN in the slack of x, w and the mask, a NaN canary around and between the rows of
    `out`."""
    from tacotron2_amd import _lib
    g = torch.Generator().manual_seed(100 * K + 10 * N + B)
    ldx, ldw, ldo, ldm, edge = K + 4, K + 8, N + 3, N + 5, 16
    x, w = torch.full((B, ldx), NAN), torch.full((N, ldw), NAN)
    x[:, :K] = torch.randn(B, K, generator=g)
    w[:, :K] = torch.randn(N, K, generator=g) * K ** -0.5
    bv = torch.randn(N, generator=g) if bias else None
    mk = None
    if mask:
        mk = torch.full((B, ldm), NAN)
        mk[:, :N] = (torch.rand(B, N, generator=g) >= 0.5).float() * 2
    ref = DC.linear_rows(x[:, :K], w[:, :K], bv, None if mk is None else mk[:, :N], relu)
    d = lambda t: None if t is None else t.to(dev)
    xd, wd, bd, md = d(x), d(w), d(bv), d(mk)
    buf = torch.full((edge + B * ldo + edge,), NAN, device=dev)
    _lib.call("t2_linear_rows", xd, ldx, wd, ldw, bd, md, ldm, int(relu), buf.data_ptr() + 4 * edge, ldo, B, N, K, _st())
    torch.cuda.synchronize()
    buf = buf.cpu()
    out = buf[edge:edge + B * ldo].view(B, ldo)
    assert bool(torch.isnan(buf[:edge]).all()) and bool(torch.isnan(buf[edge + B * ldo:]).all()) and bool(torch.isnan(out[:, N:]).all())
    got = out[:, :N]
    assert bool(torch.isfinite(got).all())
    e = _rel(got, ref)
    print(f"[decode chain] t2_linear_rows B={B} N={N} K={K} bias={bias} relu={relu} mask={mask}: {e:.2e} /2.0e-06")
    assert e < 2e-6
    if relu and mask:                                      # what the mask zeroes is exactly zero
        assert float(got[mk[:, :N] == 0].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the stop scans at scale
# ---------------------------------------------------------------------------------------------------------------------------
SCAN_GROUPS = (1, 64, 37, 64, 50, 23, 64, 1)      # 304 utterances: the scan's 256 threads take a second trip; sizes 64 and 1, 1 first and last
SCAN_STEPS = 9


def _scan_table(never, seed):
    """Seeded logits [steps][utterances]: magnitudes in [0.25, 0.6] or [1.1, 3.0] - away from 0 and from logit(0.7) = 0.8473 - with
    seeded signs; `never`: utterance 300 (second trip, in the last 64-wide group) never stops at either threshold; otherwise every
    utterance is below both thresholds at step 6 at the latest."""
    g = torch.Generator().manual_seed(seed)
    n = sum(SCAN_GROUPS)
    mag = torch.where(torch.rand(SCAN_STEPS, n, generator=g) < 0.5, 0.25 + 0.35 * torch.rand(SCAN_STEPS, n, generator=g),
                      1.1 + 1.9 * torch.rand(SCAN_STEPS, n, generator=g))
    sign = torch.where(torch.rand(SCAN_STEPS, n, generator=g) < 0.25, -1.0, 1.0)
    t = mag * sign
    t[6] = -t[6].abs()
    if never:
        t[:, 300] = 1.1 + t[:, 300].abs()
    return t.float()


@pytest.mark.parametrize("never", [True, False])
@pytest.mark.parametrize("r", [1, 3])
def test_stop_scan_at_scale(dev, never, r):
    """t2_stop_scan, t2_stop_scan_r and t2_stop_scan_thr on 304 utterances in 8 groups of unequal size, 9 stored steps, against
    loss_options_ref.stop_count exactly; the pad columns of proj are NaN.  One cap binds, one does not."""
    from tacotron2_amd import _lib
    table = _scan_table(never, seed=11 + r)
    n, Mr, ld = sum(SCAN_GROUPS), 2 * r, 2 * r + 3
    projs, k = [], 0
    for Bg in SCAN_GROUPS:
        p = torch.full((SCAN_STEPS, Bg, ld), NAN)
        p[:, :, :Mr] = 0.25
        p[:, :, Mr] = table[:, k:k + Bg]
        k += Bg
        projs.append(p.to(dev))
    scan = _lib.make("T2StopScan", proj=projs + [0] * (64 - len(projs)), Bg=list(SCAN_GROUPS) + [0] * (64 - len(SCAN_GROUPS)),
                     ngroups=len(SCAN_GROUPS), ld_proj=ld, M=Mr, nframes=SCAN_STEPS)
    thr7 = LR.stop_logit(0.7)
    assert float((table.abs()).min()) > 0.2 and float((table - thr7).abs().min()) > 0.2

    def go(entry, *args):
        lengths = torch.full((n,), -7, dtype=torch.int64, device=dev)
        out2 = torch.full((2,), -7, dtype=torch.int32, device=dev)
        _lib.call(entry, scan, *args, lengths, out2, _st())
        torch.cuda.synchronize()
        return lengths.cpu(), out2.cpu().tolist()

    assert LR.stop_count(table)[2] == (SCAN_STEPS if never else 7)
    for thr, entries in ((0.0, ("t2_stop_scan_r", "t2_stop_scan_thr")), (thr7, ("t2_stop_scan_thr",))):
        longest = int(LR.stop_count(table, thr=thr, r=r)[0].max())          # without a cap
        assert longest >= 2
        for max_len in (longest - 1, 1000):                                 # a cap that binds and one that does not
            want, frames, steps = LR.stop_count(table, thr=thr, r=r, max_len=max_len)
            assert int(want.max()) == min(max_len, longest)
            for entry in entries:
                lengths, out2 = go(entry, r, max_len, *((float(thr),) if entry.endswith("thr") else ()))
                assert torch.equal(lengths, want) and out2 == [frames, steps], (entry, thr, max_len, out2, [frames, steps])
    if r == 1:          # t2_stop_scan: rows are frames, no cap, out2 = {frames emitted, 0}
        want, frames, _ = LR.stop_count(table)
        lengths, out2 = go("t2_stop_scan")
        assert torch.equal(lengths, want) and out2 == [frames, 0]
