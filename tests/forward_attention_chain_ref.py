"""Reference for the kernel-level tests of the attention chain under FORWARD ATTENTION (T2AttnSeq.forward / t2_attn_seq_bwd_forward,
include/tacotron2_amd.h): tests/attention_chain_ref.py's `chain` restated with the prior, the dtype as a parameter, every
quantity the two calls write an autograd node of its own.  CPU only (tests/test_forward_attention_chain_host.py checks the
restatement, tests/test_gpu_forward_attention_training.py checks the kernels against it).

Per frame t, with e_t the masked energies of `chain` (their location features read [alpha_{t-1}, cum_{t-1}]):
    q_t(n)   = 0.5 alpha_{t-1}(n) + 0.5 alpha_{t-1}(n-1) + 1e-8       (alpha_{-1} = one-hot at 0; frame 0's location features see zeros)
    alpha_t  = q_t exp(e_t - max) / sum q_t exp(e_t - max)             (= softmax(e_t + log q_t))
    ctx_t = alpha_t . memory ;  cum_t = cum_{t-1} + alpha_t ;  align[:, t] = alpha_t
Objective and outputs as in `chain`.

init: a given state at frame 0, treated as constants - dict(align0 (B,L), cum (B,L), att_h (B,A), att_c (B,A)); ctx_0 = align0 . memory.
Frames then run from 1 and every time-major output has T - 1 rows (frames 1 .. T-1; `align` is (B, T-1, L)).  The kernels get the same
state through slot 1 of the stashes and row 0 of `align`, and t_begin = 1 / t_lo = 1.  Why: under the prior, frame t carries weight
only up to position about t + 1, so a tiling edge at position 32, 216, 252 or 256 sees weights of 1e-8 in a short chain from zero
and a kernel bug there would be invisible; a Gaussian bump next to the edge puts weights of 0.1 - 0.3 on both of its sides.

`recursion_fa` is the hand-coded backward of the rule (include/tacotron2_amd.h, t2_attn_seq_bwd_forward): g = dw + dwx + da + P,
de = alpha (g - sigma), r = de / q, P[n] = 0.5 r[n] + 0.5 r[n+1], with the cumulative-weights carry G kept separate.  Its `fault`
argument restates plausible kernel bugs (FAULTS_FA); chain_fa(fault=...) hands over to it."""
from collections import OrderedDict

import torch

from oracle import tacotron2_ref as R
from tests.attention_chain_ref import (KL, PAD, FWD_OUTPUTS, BWD_OUTPUTS, TOL_CAP, errors, make_inputs, per_sample_rel,  # noqa: F401
                                       single_position_violations)

V_SCALE = 0.25      # v of make_inputs is scaled by this in every case here (sharper energies only amplify the float32 reference's own
                    # error along the recursion: 6e-6 on dpm / dv unscaled against 9e-7 scaled, both measured on the restatement)


def _case(name, B, L, T, A, Ad, Ef, drop, dalign, tiled, why, bump=None, ragged=False, edges=(), chunk=0):
    return name, dict(name=name, B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, drop=drop, dalign=dalign, tiled=tiled, mel_tail=False, why=why,
                      bump=bump, ragged=ragged, edges=tuple(edges), chunk=chunk)


# bump: centre of the Gaussian start state (None = from zero).  edges: (l, l + 1) position pairs that must both carry weight.
# chunk: the GPU test issues the frames as calls of that many frames (0 = one call).
CASES_FA = OrderedDict([
    _case("L1_B1_T2", 1, 1, 2, 32, 16, 32, False, True, False, "L = 1, B = 1, T = 2: one position, the prior is the whole weight"),
    _case("L2_T3", 3, 2, 3, 32, 16, 32, True, False, True,
          "L = 2, T = 3 from zero: the w_prev == NULL one-hot prior, no r out of frame 0"),
    _case("L33_B17_zero", 17, 33, 8, 64, 32, 64, True, True, False, "L = 33, B = 17, T = 8 from zero with dalign and att_drop; dgates_t = NULL"),
    _case("L33_bump30", 3, 33, 12, 32, 16, 32, True, True, True, "the dw kernel's block edge 31|32", bump=30, edges=[(31, 32)]),
    _case("L257_bump250", 3, 257, 12, 32, 16, 32, False, True, False,
          "252|253 and the 255|256 round edge on the L > 252 path", bump=250, edges=[(252, 253), (255, 256)]),
    _case("L257_bump212", 2, 257, 12, 32, 16, 32, True, False, True, "the per-slice kernel's tile edge 215|216", bump=212, edges=[(215, 216)]),
    _case("L252_bump245", 2, 252, 12, 32, 16, 32, True, True, True, "the one-pass stash + acc path at its longest text", bump=245,
          edges=[(247, 248)]),
    _case("ragged_L60", 5, 60, 12, 32, 16, 32, True, True, False,
          "bump at len - 2 with len < L: r[len] = 0, mass piling on the last position, len[1] = 1", bump=58, ragged=True),
    _case("L33_bump30_chunk5", 3, 33, 12, 32, 16, 32, True, True, True,
          "the same T = 12 case through calls of 5 frames: the slot parity carried across calls, both parities", bump=30, edges=[(31, 32)],
          chunk=5),
    _case("L433_Ad144_Ef672_bump428", 3, 433, 12, 64, 144, 672, True, True, True, "the third position tile's one position", bump=428,
          edges=[(431, 432)]),
    _case("shipped_T24", 4, 188, 24, 1024, 128, 512, True, True, True, "the shipped dims A = 1024, Ad = 128, Ef = 512 at L = 188 from zero"),
])


def make_inputs_fa(case):
    """attention_chain_ref.make_inputs with v scaled by V_SCALE and, for a case with a bump, the start state `init` (float32
    tensors: the kernels get exactly these).  Returns (inp, init or None)."""
    inp = make_inputs(case)
    inp["v"] = inp["v"] * V_SCALE
    if case.get("ragged"):          # every sample shorter than L but the first
        lens = inp["len"]
        for b in range(2, case["B"]):
            lens[b] = max(3, int(lens[b]) - 7 * b) if int(lens[b]) > 3 else int(lens[b])
    if case.get("bump") is None:
        return inp, None
    B, L, A = case["B"], case["L"], case["A"]
    g = torch.Generator().manual_seed(77 + L + B)
    lens = inp["len"]
    centre = torch.minimum(torch.full((B,), case["bump"]), (lens - 2).clamp(min=0)).double()
    pos = torch.arange(L, dtype=torch.float64)[None, :]
    a0 = torch.exp(-0.5 * ((pos - centre[:, None]) / 2.0) ** 2).masked_fill(pos >= lens[:, None], 0.0)
    a0 = (a0 / a0.sum(1, keepdim=True)).float()
    a0 = a0 / a0.sum(1, keepdim=True)
    for b in range(B):
        if int(lens[b]) == 1:
            a0[b] = 0.0
            a0[b, 0] = 1.0
    init = dict(align0=a0, cum=(2.0 * a0), att_h=0.5 * torch.tanh(torch.randn(B, A, generator=g)),
                att_c=0.5 * torch.randn(B, A, generator=g))
    return inp, init


def _prior(a_prev, onehot, L, dtype, B):
    """q(n) = 0.5 a(n) + 0.5 a(n-1) + 1e-8; a = one-hot at 0 in front of frame 0."""
    if onehot:
        a_prev = torch.zeros(B, L, dtype=dtype)
        a_prev[:, 0] = 1.0
    sh = torch.cat([torch.zeros(B, 1, dtype=dtype), a_prev[:, :-1]], 1)
    return 0.5 * a_prev + 0.5 * sh + 1e-8


def _energies(pre_t, ctx, att_h, att_c, w_in, cum_in, drop_t, P, mask):
    """One frame up to the masked energies (the arithmetic of attention_chain_ref.chain)."""
    W_ih_ctx, W_hh, Wq, UB, vB, pm = P
    B, L = w_in.shape
    A = att_h.shape[1]
    g = pre_t + ctx @ W_ih_ctx.T + att_h @ W_hh.T
    att_h, att_c = R.lstm_cell(g, att_c)
    gates = torch.cat([R._sigmoid(g[:, :A]), R._sigmoid(g[:, A:2 * A]), torch.tanh(g[:, 2 * A:3 * A]), R._sigmoid(g[:, 3 * A:])], 1)
    if drop_t is not None:
        att_h = att_h * drop_t
    q = att_h @ Wq.T
    wp = torch.zeros(B, 2, L + 2 * PAD, dtype=w_in.dtype)
    wp[:, :, PAD:PAD + L] = torch.stack([w_in, cum_in], 1)
    loc = torch.einsum("bclk,back->bla", wp.unfold(2, KL, 1), UB)
    th = torch.tanh(q[:, None, :] + loc + pm)
    e = (th * vB[:, None, :]).sum(-1)
    return att_h, att_c, gates, q, th, e, e.masked_fill(mask, float("-inf"))


def _setup(inp, dtype, init):
    c = lambda x: None if x is None else x.to(dtype)
    T, B, A4 = inp["pre"].shape
    A, L, Ad = A4 // 4, inp["memory"].shape[1], inp["v"].shape[0]
    memory = c(inp["memory"])
    vB = c(inp["v"])[None].expand(B, Ad).clone().requires_grad_(True)
    UB = c(inp["U"])[None].expand(B, Ad, 2, KL).clone().requires_grad_(True)
    pm = c(inp["pm"]).clone().requires_grad_(True)
    pre = c(inp["pre"]).clone().requires_grad_(True)
    P = (c(inp["W_ih_ctx"]), c(inp["W_hh"]), c(inp["Wq"]), UB, vB, pm)
    mask = torch.arange(L)[None, :] >= inp["len"][:, None]
    if init is None:
        first = 0
        st = dict(att_h=torch.zeros(B, A, dtype=dtype), att_c=torch.zeros(B, A, dtype=dtype), w=torch.zeros(B, L, dtype=dtype),
                  cum=torch.zeros(B, L, dtype=dtype))
        st["ctx"] = torch.zeros(B, memory.shape[2], dtype=dtype)
    else:
        first = 1
        st = dict(att_h=c(init["att_h"]), att_c=c(init["att_c"]), w=c(init["align0"]), cum=c(init["cum"]))
        st["ctx"] = torch.einsum("bl,ble->be", st["w"], memory)
    return T, B, A, L, Ad, memory, pre, P, mask, first, st


FAULTS_FA = ("prior_detached", "shift_wrong_side", "carry_cut_32", "carry_cut_216", "carry_cut_256", "P_in_cum", "parity_chunk5")


def chain_fa(inp, dtype=torch.float64, init=None, fault=None, prior=True):
    """attention_chain_ref.chain under forward attention; the same outputs (float64 tensors, reference layouts), time-major ones
    over the frames first .. T-1 (first = 1 with `init`).  prior=False forces q = 1: the plain chain.  fault: one of FAULTS_FA
    (recursion_fa restates them; the forward outputs are the fault-free ones)."""
    if fault is not None:
        assert fault in FAULTS_FA and dtype == torch.float64
        return recursion_fa(inp, init, fault)
    c = lambda x: None if x is None else x.to(dtype)
    T, B, A, L, Ad, memory, pre, P, mask, first, s = _setup(inp, dtype, init)
    att_drop, dh_ext, dc1, dc2, da = (c(inp[k]) for k in ("att_drop", "dh_ext", "dctx_ext1", "dctx_ext2", "dalign"))
    att_h, att_c, ctx, w, cum = s["att_h"], s["att_c"], s["ctx"], s["w"], s["cum"]
    obj = torch.zeros((), dtype=dtype)
    st = {k: [] for k in ("att_h", "att_c", "ctx", "gates", "cum", "th", "align", "q")}
    for t in range(first, T):
        att_h, att_c, gates, q, th, _, e = _energies(pre[t], ctx, att_h, att_c, w, cum, None if att_drop is None else att_drop[t], P, mask)
        q.retain_grad()
        p = torch.exp(e - e.max(1, keepdim=True).values)
        if prior:
            p = p * _prior(w, t == 0, L, dtype, B)
        w = p / p.sum(1, keepdim=True)
        ctx = torch.einsum("bl,ble->be", w, memory)
        ctx.retain_grad()
        cum = cum + w
        for k, x in (("att_h", att_h), ("att_c", att_c), ("ctx", ctx), ("cum", cum), ("th", th), ("align", w), ("q", q), ("gates", gates)):
            st[k].append(x)
        obj = obj + (att_h * dh_ext[t]).sum() + (ctx * (dc1[t] + dc2[t])).sum()
        if da is not None:
            obj = obj + (w * da[:, t]).sum()
    obj.backward()
    out = {k: torch.stack(st[k], 0).detach() for k in ("att_h", "att_c", "ctx", "gates", "cum", "th")}
    out["align"] = torch.stack(st["align"], 1).detach()
    out["dgates"] = pre.grad[first:]
    out["dq"] = torch.stack([x.grad for x in st["q"]], 0)
    out["dctx_tot"] = torch.stack([x.grad for x in st["ctx"]], 0)
    out["dpm"], out["dv"], out["dU"] = P[5].grad, P[4].grad, P[3].grad
    return {k: x.double() for k, x in out.items()}


def recursion_fa(inp, init=None, fault=None):
    """The hand-coded float64 backward of the rule.  Each frame's map (previous state -> att_h, att_c, energies) is an autograd
    island with detached inputs - what the rule leaves unchanged (ds, dq, dpm, dv, dU, d_in, the cells) comes from autograd.grad
    of the island given de; de, sigma, r, P and the carry G are written out by hand, frame T-1 down to `first`."""
    dtype = torch.float64
    c = lambda x: None if x is None else x.to(dtype)
    T, B, A, L, Ad, memory, pre, P, mask, first, s = _setup(inp, dtype, init)
    W_ih_ctx, W_hh, Wq, UB, vB, pm = P
    att_drop, dh_ext, dc1, dc2, da = (c(inp[k]) for k in ("att_drop", "dh_ext", "dctx_ext1", "dctx_ext2", "dalign"))
    att_h, att_c, ctx, w, cum = s["att_h"], s["att_c"], s["ctx"], s["w"], s["cum"]
    fr, fw = [], {k: [] for k in ("att_h", "att_c", "ctx", "gates", "cum", "th", "align")}
    for t in range(first, T):
        leaves = [x.detach().clone().requires_grad_(True) for x in (att_h, att_c, ctx, w, cum)]
        h1, c1, gates, q, th, e_raw, e = _energies(pre[t], leaves[2], leaves[0], leaves[1], leaves[3], leaves[4],
                                                   None if att_drop is None else att_drop[t], P, mask)
        qp = _prior(w.detach(), t == 0, L, dtype, B)
        p = torch.exp(e.detach() - e.detach().max(1, keepdim=True).values) * qp
        w = p / p.sum(1, keepdim=True)
        att_h, att_c, ctx, cum = h1.detach(), c1.detach(), torch.einsum("bl,ble->be", w, memory), cum.detach() + w
        fr.append(dict(leaves=leaves, h1=h1, c1=c1, q=q, e=e_raw, alpha=w, qp=qp))
        for k, x in (("att_h", att_h), ("att_c", att_c), ("ctx", ctx), ("cum", cum), ("th", th.detach()), ("align", w), ("gates", gates.detach())):
            fw[k].append(x)
    z = lambda *sh: torch.zeros(*sh, dtype=dtype)
    dh_n, dc_n, dctx_n = z(B, A), z(B, A), z(B, memory.shape[2])
    din0, din1, G, r_next = z(B, L), z(B, L), z(B, L), z(B, L)
    r_hist = {}
    dgates, dq, dctx_tot = {}, {}, {}
    dpm, dv, dU = torch.zeros_like(pm), torch.zeros_like(vB), torch.zeros_like(UB)
    pos = torch.arange(L)[None, :]
    for t in range(T - 1, first - 1, -1):
        f = fr[t - first]
        alpha = f["alpha"]
        dct = dc1[t] + dc2[t] + dctx_n
        dw = torch.einsum("ble,be->bl", memory, dct)
        r_src = r_next
        if fault == "parity_chunk5" and t < T - 1 and (T - 1 - t) % 5 == 0 and (t + 2) in r_hist:
            r_src = r_hist[t + 2]        # the first frame of a later call reads the slot its own parity names: r of frame t + 2
        if fault in ("carry_cut_32", "carry_cut_216", "carry_cut_256"):
            r_src = r_src.masked_fill(pos >= int(fault.rsplit("_", 1)[1]), 0.0)
        if fault == "shift_wrong_side":
            Pn = 0.5 * r_src + 0.5 * torch.cat([z(B, 1), r_src[:, :-1]], 1)
        else:
            Pn = 0.5 * r_src + 0.5 * torch.cat([r_src[:, 1:], z(B, 1)], 1)
        if fault == "prior_detached":
            Pn = z(B, L)
        Gn = din1 + G + (Pn if fault == "P_in_cum" else 0.0)
        g = dw + din0 + Gn + Pn + (da[:, t] if da is not None else 0.0)
        sigma = (alpha * g).sum(1, keepdim=True)
        de = alpha * (g - sigma)
        r_next = de / f["qp"]
        r_hist[t] = r_next
        G = Gn
        grads = torch.autograd.grad([f["h1"], f["c1"], f["e"]], f["leaves"] + [pre, pm, vB, UB, f["q"]],
                                    [dh_ext[t] + dh_n, dc_n, de], allow_unused=True)
        nz = lambda x, like: torch.zeros_like(like) if x is None else x
        dh_n, dc_n, dctx_n, din0, din1 = (nz(x, l) for x, l in zip(grads[:5], f["leaves"]))
        dgates[t], dq[t], dctx_tot[t] = grads[5][t], grads[9], dct
        dpm, dv, dU = dpm + grads[6], dv + grads[7], dU + grads[8]
    rng = range(first, T)
    out = {k: torch.stack(x, 0) for k, x in fw.items() if k != "align"}
    out["align"] = torch.stack(fw["align"], 1)
    out.update(dgates=torch.stack([dgates[t] for t in rng]), dq=torch.stack([dq[t] for t in rng]),
               dctx_tot=torch.stack([dctx_tot[t] for t in rng]), dpm=dpm, dv=dv, dU=dU)
    return {k: x.detach().double() for k, x in out.items()}


def model_fa(P, d, case, dtype=torch.float64, recursion=True):
    """The whole model, teacher-forced and in training mode, under forward attention: R.tacotron2_fwd's teacher-forced path with
    R.decoder_step's lines around the attention call restated - the softmax y_t replaced by alpha_t = q_t y_t / sum q_t y_t in the
    context, the cumulative weights, the returned alignments and the next frame's location features (alpha_{-1} one-hot at 0, frame
    0's location features see zeros).  case = tests.test_gpu_model.random_case(...).  recursion=False keeps y_t: R.tacotron2_fwd.
    Returns (Pc, (mels, post, gates, alignments), names): parameters in `dtype` with requires_grad, outputs with their graph."""
    ci, lens, mel, tl, gate, masks = case
    cast = lambda v: v.to(dtype) if v.is_floating_point() else v
    Pc = {k: (cast(v).clone().requires_grad_(True) if (v.is_floating_point() and not R.is_buffer(k)) else cast(v).clone())
          for k, v in P.items()}
    m = {k: ([cast(x) for x in v] if isinstance(v, list) else cast(v)) for k, v in masks.items()}
    names = [k for k, v in Pc.items() if v.requires_grad]
    B, L = ci.shape
    mel = cast(mel)
    T = mel.shape[1]
    encoded = R.encoder_fwd(Pc, ci, lens, True, m.get("enc_drop"), {})
    memory, pm = R.condition(Pc, d, encoded, None, None)
    lmask = torch.arange(L)[None, :] >= lens[:, None]
    A, D, Ef = d["att_rnn_dim"], d["rnn_hidden_dim"], memory.shape[2]
    z = lambda *sh: torch.zeros(*sh, dtype=dtype)
    att_h, att_c, ctx, w, w_cum, dec_h, dec_c = z(B, A), z(B, A), z(B, Ef), z(B, L), z(B, L), z(B, D), z(B, D)
    prior = z(B, L)
    prior[:, 0] = 1.0
    pd = m.get("prenet_drop")
    dec_in = R.prenet_fwd(Pc, torch.cat([z(B, 1, mel.shape[2]), mel], 1), pd[0] if pd else None, pd[1] if pd else None)
    ad, dd = m.get("att_drop"), m.get("dec_drop")
    mels, gates, aligns = [], [], []
    for i in range(T):
        g = torch.cat([dec_in[:, i], ctx], -1) @ Pc["decoder.att_rnn.weight_ih"].T + Pc["decoder.att_rnn.bias_ih"] \
            + att_h @ Pc["decoder.att_rnn.weight_hh"].T + Pc["decoder.att_rnn.bias_hh"]
        att_h, att_c = R.lstm_cell(g, att_c)
        if ad is not None:
            att_h = att_h * ad[i]
        ctx, y = R.attention_fwd(Pc, att_h, memory, pm, torch.stack([w, w_cum], 1), lmask)
        if recursion:
            q = 0.5 * prior + 0.5 * torch.cat([z(B, 1), prior[:, :-1]], 1) + 1e-8
            a = q * y
            w = (a / a.sum(1, keepdim=True)).masked_fill(lmask, 0.0)
            ctx = torch.einsum("bl,ble->be", w, memory)
            prior = w
        else:
            w = y
        w_cum = w_cum + w
        g = torch.cat([att_h, ctx], -1) @ Pc["decoder.lstm.weight_ih"].T + Pc["decoder.lstm.bias_ih"] \
            + dec_h @ Pc["decoder.lstm.weight_hh"].T + Pc["decoder.lstm.bias_hh"]
        dec_h, dec_c = R.lstm_cell(g, dec_c)
        if dd is not None:
            dec_h = dec_h * dd[i]
        hc = torch.cat([dec_h, ctx], -1)
        gates.append(hc @ Pc["decoder.gate.weight"].T + Pc["decoder.gate.bias"])
        mels.append(hc @ Pc["decoder.mel_out.weight"].T + Pc["decoder.mel_out.bias"])
        aligns.append(w)
    mels, gates, aligns = torch.stack(mels, 1), torch.stack(gates, 1), torch.stack(aligns, 1)
    post = mels + R.postnet_fwd(Pc, mels, True, m.get("post_drop"), {})
    mm = (torch.arange(T)[None, :] >= tl.to(torch.int64)[:, None])[:, :, None]
    return Pc, (mels.masked_fill(mm, 0.0), post.masked_fill(mm, 0.0), gates.masked_fill(mm, -1000.0), aligns), names


def errors_fa(got, ref, inp, names=None):
    return errors(got, ref, inp["len"], names=names)


def single_position_violations_fa(got, inp, ref, first):
    """attention_chain_ref.single_position_violations on the frames first .. T-1 (its bounds read dalign / dctx_tot per frame)."""
    sub = dict(inp)
    if sub["dalign"] is not None:
        sub["dalign"] = sub["dalign"][:, first:]
    return single_position_violations(got, sub, ref)


# -----------------------------------------------------------------------------------------------------------------
# Tolerances, by the method of attention_chain_ref: TOL_FA[k] = 16 x F32_ERR_FA[k], F32_ERR_FA[k] = the largest per_sample_rel between
# the float32 and the float64 run of chain_fa over CASES_FA (one CPU thread, rounded up; test_forward_attention_chain_host.py
# re-measures them and fails if a case exceeds its constant or a TOL_FA exceeds TOL_CAP = 4e-5).
# -----------------------------------------------------------------------------------------------------------------
#   measured (worst case):  att_h 7.27e-7 shipped_T24 | ctx 5.14e-7 shipped_T24 | att_c 3.11e-7 L33_B17_zero | gates 6.15e-7 shipped_T24
#     cum 2.50e-7 shipped_T24 | align 2.70e-7 ragged_L60 | th 1.37e-6 shipped_T24 | dgates 5.62e-7 shipped_T24
#     dq 6.54e-7 L33_B17_zero | dctx_tot 1.38e-7 shipped_T24 | dpm 7.56e-7 L33_B17_zero | dv 9.54e-7 shipped_T24 | dU 7.13e-7 L33_B17_zero
#   (each rounded up to two digits with at least 2 % of headroom for another CPU's float32 summation orders)
F32_ERR_FA = dict(
    att_h=7.5e-7, ctx=5.3e-7, att_c=3.2e-7, gates=6.3e-7, cum=2.6e-7, align=2.8e-7, th=1.4e-6,
    dgates=5.8e-7, dq=6.7e-7, dctx_tot=1.5e-7, dpm=7.8e-7, dv=9.8e-7, dU=7.3e-7,
)
TOL_FA = {k: 16.0 * e for k, e in F32_ERR_FA.items()}
