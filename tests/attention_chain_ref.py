"""Reference for the kernel-level tests of the attention chain (t2_attn_seq_fwd / t2_attn_seq_bwd, include/tacotron2_amd.h):
a plain torch restatement of the teacher-forced chain with the dtype as a parameter, in which every quantity the two calls
write is an autograd node of its own.  CPU only; importable without a GPU (tests/test_attention_chain_host.py checks the
restatement against oracle.tacotron2_ref, tests/test_gpu_attention_chain.py checks the kernels against the restatement).

Per frame t (model/decoder.py:68-90 with the input projection of the prenet hoisted into `pre`):
    gates = pre_t + ctx_{t-1} . W_ih_ctx^T + att_h_{t-1} . W_hh^T ;  att_h_t, att_c_t = lstm_cell(gates) ;  att_h_t *= att_drop_t
    q_t = att_h_t . Wq^T ;  e = v . tanh(q_t + loc([w_{t-1}, cum_{t-1}]) + pm)  with the FOLDED location filter U ;
    w_t = softmax(e masked behind len) ;  ctx_t = w_t . memory ;  cum_t = cum_{t-1} + w_t
Objective = sum_t  att_h_t . dh_ext_t + ctx_t . (dctx_ext1_t + dctx_ext2_t) + w_t . dalign_t, so that autograd's gradient of
    pre_t            is the kernel's  Z[t][:, :4A]      ("dgates")
    q_t (retained)   is               Z[t+1][:, 4A:]    ("dq")
    ctx_t (retained) is               dctx_tot[t]       (the total: upstream + what frame t+1 sends back)
    pm               is               dpmT transposed   ("dpm")
    per-sample copies of v and U are  dv_part, dU_part  (before the sum over samples).

The metric of both test modules:
    per_sample_rel(got, ref) = max over samples b of  max|got_b - ref_b| / max|ref_b|
per output, for time-major outputs per sample over all frames.  A sample whose reference slice is exactly zero is never
given a floor: it is either a single-position sample (len[b] = 1: weight exactly 1, dq/dpm/dv/dU exactly 0; bounded
absolutely by single_position_bounds) or must be exactly zero in `got` too.

CASES is the committed case list of the GPU test; F32_ERR / TOL are the tolerance constants derived from it (see TOL)."""
import math
from collections import OrderedDict

import torch

from oracle import tacotron2_ref as R

KL = 31
PAD = (KL - 1) // 2


# -----------------------------------------------------------------------------------------------------------------
# The committed case list.  Every edge of the kernels' position / dim / row tiling is hit by at least one case (all are
# run forward + backward on the GPU).  Flags: drop = att_drop given, dalign = upstream alignment gradient given,
# tiled = the x16-tiled dgates_t copy given to the backward, mel_tail = the upstream dh_ext / dctx_ext rows of the frames
# behind a per-sample "mel length" are zero while dalign is not (the header: those frames count for dalign).
# len[0] = L and, for B > 1, len[1] = 1 (the single-position sample); the rest is seeded.
# -----------------------------------------------------------------------------------------------------------------
def _case(name, B, L, T, A, Ad, Ef, drop, dalign, tiled, why, mel_tail=False):
    return name, dict(name=name, B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, drop=drop, dalign=dalign, tiled=tiled, mel_tail=mel_tail,
                      why=why)


CASES = OrderedDict([
    _case("L1_B1_T1", 1, 1, 1, 32, 16, 32, False, True, False,
          "L = 1, B = 1, T = 1: the only sample is a single position; one frame (no recurrent term at all); A = 32, Ad = 16, Ef = 32"),
    _case("L2_T2", 3, 2, 2, 32, 16, 32, True, False, True,
          "L = 2, T = 2: shortest text with a softmax to speak of; the location filter hangs over both ends"),
    _case("L31_B15", 15, 31, 7, 64, 32, 64, True, True, True,
          "L = 31 (one short 32-position block of the dw kernel), B = 15 (one pad row in the x16 tiles), T = 7, A = 64"),
    _case("L32_B16_Ef640", 16, 32, 2, 64, 16, 640, False, False, True,
          "L = 32 (exactly one dw block), B = 16 (no pad rows), Ef = 640 (the whole register image of the dw kernel)"),
    _case("L33_B17", 17, 33, 7, 64, 32, 64, True, True, False,
          "L = 33 (a second dw block of one position), B = 17 (second row tile of one row), dgates_t = NULL"),
    _case("B33_L97", 33, 97, 3, 64, 32, 64, True, True, True,
          "B = 33: two 32-row blocks in the cell kernels (the 32 x 32-tile forward cell at A % 64 == 0), 15 pad rows"),
    _case("L192", 2, 192, 2, 32, 16, 32, False, True, False,
          "L = 192: the last position the context kernel keeps in its register rows"),
    _case("L193_Ad144", 3, 193, 2, 32, 144, 32, True, False, True,
          "L = 193: first position past the context kernel's register rows; Ad = 144 (Ad/16 = 9: second pass of the din_part "
          "and e_part sums)"),
    _case("L252", 2, 252, 2, 32, 16, 32, True, True, True,
          "L = 252: the longest text the per-slice backward kernel takes in one pass"),
    _case("L253", 3, 253, 3, 32, 32, 64, False, True, False,
          "L = 253: the shortest text of the position-tiled per-slice kernel (tiles of 216: 216 + 37)"),
    _case("L256", 2, 256, 2, 32, 16, 32, True, False, False,
          "L = 256: exactly one pass of the forward kernels and of the dw kernel's location-gradient loop"),
    _case("L257", 3, 257, 2, 32, 16, 32, False, True, True,
          "L = 257: a second pass of one position"),
    _case("L431", 2, 431, 2, 32, 16, 32, True, True, False,
          "L = 431: last position inside the second position tile (tile 1 owns [216, 432))"),
    _case("L433_Ad144_Ef672", 3, 433, 4, 64, 144, 672, True, True, True,
          "L = 433: one position in the third tile; Ef = 672 (the tail loop above the 640-column register image), Ad = 144"),
    _case("L649_Ef1056", 2, 649, 3, 32, 16, 1056, True, True, False,
          "L = 649: one position in the fourth tile; Ef = 1056 (second 1024-column dctx block of the dw kernel)"),
    _case("Ad272", 2, 40, 2, 32, 272, 32, False, True, True,
          "Ad = 272 (Ad/16 = 17: third pass of the din_part / e_part sums)"),
    _case("Ad128_T1", 4, 60, 1, 64, 128, 160, True, False, True,
          "T = 1 with B > 1, Ad = 128 (Ad/16 = 8: exactly one pass of the partial sums)"),
    _case("mel_tail", 5, 50, 7, 64, 32, 64, True, True, True,
          "frames behind the mel length: upstream dh_ext / dctx_ext rows zero there, dalign not", mel_tail=True),
    _case("no_dalign_no_drop", 4, 75, 7, 64, 32, 96, False, False, False,
          "no dalign, no att_drop, dgates_t = NULL together; Ef = 96"),
    _case("shipped_T24", 4, 188, 24, 1024, 128, 512, True, True, True,
          "the shipped dims A = 1024, Ad = 128, Ef = 512 at L = 188 over T = 24 frames (error growth along the chain)"),
])


def make_inputs(case, seed=None):
    """Seeded float32 inputs of one case (the kernels get exactly these, the float64 reference their exact upcasts)."""
    B, L, T, A, Ad, Ef = (case[k] for k in ("B", "L", "T", "A", "Ad", "Ef"))
    if seed is None:
        seed = 1000 + 7 * L + 3 * B + T
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * sc
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    if B > 1:
        lens[1] = 1
    Wd, Wc = rn(Ad, 32, sc=32 ** -0.5), rn(32, 2, KL, sc=0.3)
    inp = dict(W_ih_ctx=rn(4 * A, Ef, sc=Ef ** -0.5), W_hh=rn(4 * A, A, sc=A ** -0.5), Wq=rn(Ad, A, sc=A ** -0.5),
               U=torch.einsum("af,fck->ack", Wd, Wc),
               v=rn(Ad, sc=2.0 * Ad ** -0.5),        # energies spread over a few units: near-uniform weights test little
               pre=rn(T, B, 4 * A), memory=rn(B, L, Ef), pm=rn(B, L, Ad),
               att_drop=(torch.rand(T, B, A, generator=g) >= 0.1).double() / 0.9,
               dh_ext=rn(T, B, A), dctx_ext1=rn(T, B, Ef), dctx_ext2=rn(T, B, Ef), dalign=rn(B, T, L))
    if not case["drop"]:
        inp["att_drop"] = None
    if not case["dalign"]:
        inp["dalign"] = None
    if case.get("mel_tail"):
        mel_len = torch.randint(1, T, (B,), generator=g)
        mel_len[0] = T
        behind = (torch.arange(T)[:, None] >= mel_len[None, :])[:, :, None]       # (T, B, 1)
        for k in ("dh_ext", "dctx_ext1", "dctx_ext2"):
            inp[k] = inp[k].masked_fill(behind, 0.0)
    inp = {k: (None if x is None else x.float()) for k, x in inp.items()}
    inp["len"] = lens
    return inp


FAULTS = ("cum_cut_216", "wprev_cut_last15", "ef_tail_640", "dalign_scale", "dh_last_sample", "din_slices_8")


def chain(inp, dtype=torch.float64, fault=None):
    """The chain in `dtype`; returns every forward stash and every backward output (float64 tensors, reference layouts):
    att_h, att_c (T,B,A); ctx (T,B,Ef); gates (T,B,4A) activated, blocks i,f,g,o; cum (T,B,L) AFTER frame t; th (T,B,L,Ad);
    align (B,T,L); dgates (T,B,4A); dq (T,B,Ad); dctx_tot (T,B,Ef); dpm (B,L,Ad); dv (B,Ad); dU (B,Ad,2,31).
    fault: one of FAULTS - a small detach / scale that restates a plausible kernel bug (the host test proves that the
    GPU test's comparison rejects each of them)."""
    assert fault is None or fault in FAULTS
    c = lambda x: None if x is None else x.to(dtype)
    W_ih_ctx, W_hh, Wq, U, v = (c(inp[k]) for k in ("W_ih_ctx", "W_hh", "Wq", "U", "v"))
    memory, att_drop = c(inp["memory"]), c(inp["att_drop"])
    dh_ext, dc1, dc2, da = (c(inp[k]) for k in ("dh_ext", "dctx_ext1", "dctx_ext2", "dalign"))
    lens = inp["len"]
    T, B, A4 = inp["pre"].shape
    A, L, Ad = A4 // 4, memory.shape[1], v.shape[0]
    if fault == "dalign_scale":
        da = da * (1 + 1e-2)
    if fault == "dh_last_sample":
        dh_ext = dh_ext.clone()
        dh_ext[T - 1, B - 1] = 0
    # per-sample leaves: autograd then yields the per-sample partials the kernels write
    vB = v[None].expand(B, Ad).clone().requires_grad_(True)
    UB = U[None].expand(B, Ad, 2, KL).clone().requires_grad_(True)
    pm = c(inp["pm"]).clone().requires_grad_(True)
    pre = c(inp["pre"]).clone().requires_grad_(True)
    mask = torch.arange(L)[None, :] >= lens[:, None]
    pos = torch.arange(L)[None, :]
    att_h = torch.zeros(B, A, dtype=dtype)
    att_c = torch.zeros(B, A, dtype=dtype)
    ctx = torch.zeros(B, memory.shape[2], dtype=dtype)
    w = torch.zeros(B, L, dtype=dtype)
    cum = torch.zeros(B, L, dtype=dtype)
    obj = torch.zeros((), dtype=dtype)
    st = {k: [] for k in ("att_h", "att_c", "ctx", "gates", "cum", "th", "align", "q")}
    for t in range(T):
        g = pre[t] + ctx @ W_ih_ctx.T + att_h @ W_hh.T
        att_h, att_c = R.lstm_cell(g, att_c)
        st["gates"].append(torch.cat([R._sigmoid(g[:, :A]), R._sigmoid(g[:, A:2 * A]), torch.tanh(g[:, 2 * A:3 * A]),
                                      R._sigmoid(g[:, 3 * A:])], 1))
        if att_drop is not None:
            att_h = att_h * att_drop[t]
        q = att_h @ Wq.T
        q.retain_grad()
        # the energies / softmax / context arithmetic of R.attention_fwd with the folded filter U as a leaf
        w_in, cum_in = w, cum
        if fault == "cum_cut_216":
            cum_in = torch.where(pos >= 216, cum.detach(), cum)
        if fault == "wprev_cut_last15":
            w_in = torch.where(pos >= L - 15, w.detach(), w)
        wp = torch.zeros(B, 2, L + 2 * PAD, dtype=dtype)
        wp[:, :, PAD:PAD + L] = torch.stack([w_in, cum_in], 1)
        win = wp.unfold(2, KL, 1)                                                # (B,2,L,K)
        loc = torch.einsum("bclk,back->bla", win, UB)                            # (B,L,Ad)
        if fault == "din_slices_8":
            loc = torch.cat([loc[..., :128], torch.einsum("bclk,back->bla", win.detach(), UB)[..., 128:]], -1)
        th = torch.tanh(q[:, None, :] + loc + pm)
        e = (th * vB[:, None, :]).sum(-1).masked_fill(mask, float("-inf"))
        p = torch.exp(e - e.max(1, keepdim=True).values)
        w = p / p.sum(1, keepdim=True)
        ctx = torch.einsum("bl,ble->be", w, memory)
        if fault == "ef_tail_640":          # forward value right, the weights' gradient ignores memory columns >= 640
            ctx_f = torch.einsum("bl,ble->be", w, torch.cat([memory[..., :640], memory[..., 640:] * 0], -1))
            ctx = ctx_f + (ctx - ctx_f).detach()
        ctx.retain_grad()
        cum = cum + w
        for k, x in (("att_h", att_h), ("att_c", att_c), ("ctx", ctx), ("cum", cum), ("th", th), ("align", w), ("q", q)):
            st[k].append(x)
        obj = obj + (att_h * dh_ext[t]).sum() + (ctx * (dc1[t] + dc2[t])).sum()
        if da is not None:
            obj = obj + (w * da[:, t]).sum()
    obj.backward()
    out = {k: torch.stack(st[k], 0).detach() for k in ("att_h", "att_c", "ctx", "gates", "cum", "th")}
    out["align"] = torch.stack(st["align"], 1).detach()
    out["dgates"] = pre.grad
    out["dq"] = torch.stack([x.grad for x in st["q"]], 0)
    out["dctx_tot"] = torch.stack([x.grad for x in st["ctx"]], 0)
    out["dpm"], out["dv"], out["dU"] = pm.grad, vB.grad, UB.grad
    return {k: x.double() for k, x in out.items()}


# -----------------------------------------------------------------------------------------------------------------
# the comparison
# -----------------------------------------------------------------------------------------------------------------
FWD_OUTPUTS = ("att_h", "ctx", "att_c", "gates", "cum", "align", "th")
BWD_OUTPUTS = ("dgates", "dq", "dctx_tot", "dpm", "dv", "dU")
TIME_MAJOR = ("att_h", "ctx", "att_c", "gates", "cum", "th", "dgates", "dq", "dctx_tot")      # (T, B, ...) -> sample axis 1
ZERO_AT_ONE_POSITION = ("dq", "dpm", "dv", "dU")       # exactly zero in the reference for a sample with len = 1


def by_sample(name, x):
    return x.transpose(0, 1) if name in TIME_MAJOR else x


def per_sample_rel(got, ref, zero_ok=()):
    """max over samples b of max|got_b - ref_b| / max|ref_b| (sample axis 0) and the sample that gives it.  A NaN / inf in
    `got` is an infinite error.  A sample whose reference slice is exactly zero must be exactly zero in `got`, except the
    samples listed in `zero_ok` (bounded elsewhere, single_position_bounds)."""
    worst, where = 0.0, -1
    for b in range(ref.shape[0]):
        g, r = got[b].double(), ref[b].double()
        if not bool(torch.isfinite(g).all()):
            return math.inf, b
        s = float(r.abs().max()) if r.numel() else 0.0
        d = float((g - r).abs().max()) if r.numel() else 0.0
        if s == 0.0:
            if b in zero_ok or d == 0.0:
                continue
            return math.inf, b
        if d / s > worst:
            worst, where = d / s, b
    return worst, where


def errors(got, ref, lens, names=None):
    """{output: (per_sample_rel, worst sample)} for every output present in `got` (reference layouts, see chain).  `th` is
    compared at the positions < len[b] only (behind them the stash is not defined)."""
    single = {b for b in range(len(lens)) if int(lens[b]) == 1}
    res = {}
    for k in (names or [n for n in FWD_OUTPUTS + BWD_OUTPUTS if n in got]):
        g, r = by_sample(k, got[k].double()), by_sample(k, ref[k])
        if k == "th":
            behind = (torch.arange(r.shape[2])[None, :] >= lens[:, None])[:, None, :, None]     # (B,1,L,1)
            g, r = g.masked_fill(behind, 0.0), r.masked_fill(behind, 0.0)
        res[k] = per_sample_rel(g, r, zero_ok=single if k in ZERO_AT_ONE_POSITION else ())
    return res


def single_position_bounds(inp, ref, b):
    """Absolute bounds on what a correct fp32 kernel may leave in dq / dpm / dv / dU of a sample with len[b] = 1.  Its weight
    is exactly 1 and the softmax backward  de = w * (up - sigma),  up = dw + dwx + da,  sigma = sum_l w_l (dw_l + dwx_l + da_l)
    cancels exactly in exact arithmetic; in fp32 the two sides sum the same terms in two orders, and what survives is bounded by
    the size of the cancelling terms:  |de_t| <= 2^-20 * S_t,  S_t = sum_e |dctx_tot[t,b,e]| |memory[b,0,e]| + |dwx_t| + |da_t|
    (2^-20 = 16 fp32 epsilons), all from the float64 reference; the reference's location-path term dwx_t of such a sample is
    exactly zero (every de behind it is), so |dwx_t| + |da_t| = |dalign[b,t,0]|.  Then with |1 - th^2| <= 1, |th| <= 1 and the
    location inputs |w_{t-1}| <= 1, |cum_{t-1}| <= t:
        |dq[t,a]| <= |v_a| 2^-20 S_t ;  |dpm[l,a]| <= |v_a| 2^-20 sum_t S_t ;  |dv[a]| <= 2^-20 sum_t S_t ;
        |dU[a,c,k]| <= |v_a| 2^-20 sum_t max(1, t) S_t."""
    eps16 = 2.0 ** -20
    v = inp["v"].double().abs()
    S = (ref["dctx_tot"][:, b].abs() * inp["memory"][b, 0].double().abs()[None, :]).sum(1)          # (T,)
    if inp["dalign"] is not None:
        S = S + inp["dalign"][b, :, 0].double().abs()
    T = S.shape[0]
    tw = torch.arange(T, dtype=torch.float64).clamp(min=1.0)
    return dict(dq=eps16 * S[:, None] * v[None, :],
                dpm=(eps16 * S.sum() * v)[None, :].expand(inp["pm"].shape[1], -1),
                dv=(eps16 * S.sum()).expand(v.shape[0]),
                dU=(eps16 * (S * tw).sum() * v)[:, None, None].expand(-1, 2, KL))


def single_position_violations(got, inp, ref):
    """[(output, sample, worst |value| / bound)] over the samples with len = 1 that exceed single_position_bounds, and the
    alignments / cumulative weights of such a sample that are not exactly [1, 0, ...] / [t + 1, 0, ...]."""
    bad = []
    for b in range(len(inp["len"])):
        if int(inp["len"][b]) != 1:
            continue
        bounds = single_position_bounds(inp, ref, b)
        for k, bound in bounds.items():
            if k not in got:
                continue
            g = by_sample(k, got[k].double())[b]
            if not bool(torch.isfinite(g).all()) or bool((g.abs() > bound).any()):
                ratio = float((g.abs() / bound.clamp(min=1e-300)).max())
                bad.append((k, b, ratio))
        if "align" in got:
            a = got["align"][b].double()
            if not (bool((a[:, 0] == 1.0).all()) and bool((a[:, 1:] == 0.0).all())):
                bad.append(("align", b, math.inf))
    return bad


# -----------------------------------------------------------------------------------------------------------------
# Tolerances: ONE constant per output for all cases, from the reference and not from the kernels:
#     TOL[k] = 16 x F32_ERR[k],   F32_ERR[k] = the largest per_sample_rel between the float32 and the float64 run of chain()
# over CASES (measured on the CPU with one thread, rounded up to two digits; test_attention_chain_host.py re-measures it and
# fails if any case exceeds its F32_ERR, so the constants cannot drift away from the reference).  The factor 16 covers what
# legitimately differs between two correct fp32 implementations of a chain of T frames: reduction orders (8-lane and 8-wave
# partial sums, MFMA accumulation) and the device's tanh / exp / sigmoid against libm's.  No constant is above 4e-5 (4 x the
# 1e-5 the single-launch tests in test_gpu_kernels.py allow relative to the batch's maximum).
# -----------------------------------------------------------------------------------------------------------------
#   measured (worst case):  att_h 7.27e-7 shipped_T24 | ctx 6.37e-7 L649_Ef1056 | att_c 3.78e-7 L32_B16_Ef640 | gates 7.63e-7 L31_B15
#     cum 3.36e-7 Ad128_T1 | align 4.25e-7 shipped_T24 | th 7.79e-7 shipped_T24 | dgates 5.67e-7 L32_B16_Ef640
#     dq 9.63e-7 L32_B16_Ef640 | dctx_tot 1.68e-7 L31_B15 | dpm 9.80e-7 L33_B17 | dv 7.58e-7 L32_B16_Ef640 | dU 8.09e-7 L433_Ad144_Ef672
#   (each rounded up to two digits with at least 2 % of headroom for another CPU's float32 summation orders)
F32_ERR = dict(
    att_h=7.5e-7, ctx=6.5e-7, att_c=3.9e-7, gates=7.8e-7, cum=3.5e-7, align=4.4e-7, th=8.0e-7,
    dgates=5.8e-7, dq=9.8e-7, dctx_tot=1.8e-7, dpm=1.0e-6, dv=7.7e-7, dU=8.3e-7,
)
TOL = {k: 16.0 * e for k, e in F32_ERR.items()}
TOL_CAP = 4e-5
