"""Reference for the kernel-level tests of the autoregressive decode loop (t2_decoder_infer, include/tacotron2_amd.h): a plain
torch restatement of the loop with the dtype as a parameter - float64 is the reference, float32 only yields the tolerances.
CPU only; importable without a GPU (tests/test_decode_chain_host.py checks the restatement against oracle.tacotron2_ref,
tests/test_gpu_decode_chain.py checks the kernels against the restatement).

Per frame t, exactly as the header describes T2Infer:
    t > 0:  y = xproj_{t-1} . W_comb^T + b_comb (+ row_comb) ;  p1_t = relu(y[:, :P]) * mask[t][0] ;  proj[t-1] = y[:, P:] = [mel | stop logit]
            p2_t = relu(p1_t . W_pre2^T) * mask[t][1]                  (frame 0: p2 = 0, whatever the masks are)
    gates = [p2_t | ctx_{t-1}] . W_ih_att^T + att_h_{t-1} . W_hh_att^T + both biases ;  att_h_t, att_c_t = cell (zoned with zone_p)
    q = att_h_t . Wq^T ;  e = v . tanh(q + loc([w_{t-1}, cum_{t-1}]) + pm) with the FOLDED location filter U, masked behind len (and
            outside the window around the previous peak) ;  w_t = softmax(e) (forward attention: times the prior, renormalised) ;
            ctx_t = w_t . memory ;  cum_t = cum_{t-1} + w_t
    gates = [att_h_t | ctx_t] . W_ih_dec^T + dec_h_{t-1} . W_hh_dec^T + both biases (+ dec_pre) ;  dec_h_t, dec_c_t = cell
    xproj_t = [dec_h_t | ctx_t]
and after the last frame of a call the same combined linear once more, unmasked: proj[T-1].  Every utterance runs all T frames (the
kernel does not mask stopped utterances).  The sticky stop rule per frame: done[b] |= logit < thr, state = {all done, frames emitted}.

W_comb / b_comb / row_comb are folded in float64 from the raw weights and rounded ONCE to float32 (build_comb); the restatement and the
kernel both start from those float32 values, so the fold is not part of the error under test.

Metric: attention_chain_ref.per_sample_rel - max over samples of max|got_b - ref_b| / max|ref_b| per output.
Tolerances: TOL = 16 x F32_ERR, F32_ERR = the float32 restatement's own error against float64 over CASES, one value per output
(measured on the CPU with one thread by measure_f32_err, re-measured by tests/test_decode_chain_host.py; the factor 16 is the project's
convention for chain kernels, attention_chain_ref.TOL).  Never from a kernel's output.

Stop decisions are discrete, so every case keeps the float64 stop logits of every frame and utterance at least
STOP_MARGIN x TOL["stop"] x max|stop logit| away from its threshold (stop_margin; the seeds of CASES were chosen on the reference
alone so that this holds); `done` and `state` can then be compared exactly.  "Inside the run" below means that the loop goes on after
the stop: first-stop frame + 1 < T."""
from collections import OrderedDict

import numpy as np
import torch

from tests import attention_chain_ref as C
from tests import zoneout_ref as Z
from tests.forward_attention_chain_ref import _prior
from tests.loss_options_ref import stop_logit
from tests.test_attention_window_host import window_mask

KL, PAD = C.KL, C.PAD
per_sample_rel = C.per_sample_rel
GATE_SCALE, GATE_BIAS = 6.0, 0.3       # as tests/test_gpu_model.py::test_inference_midsize_matches_oracle: the stops are non-trivial
STOP_MARGIN = 100.0


# -----------------------------------------------------------------------------------------------------------------
# The committed case list.  Default dims: the four state widths pairwise distinct multiples of 16 (every offset of the tiled state
# is then distinct), M = 20 -> ld_proj = 24 with three pad columns per row, L = 13, T = 7, len = [13, 1, 7, seeded...].
# -----------------------------------------------------------------------------------------------------------------
def _case(name, B, seed, why, T=7, P=32, A=48, Ef=96, D=64, Ad=16, M=20, L=13, **opt):
    o = dict(no_mask=False, controls=False, zone_p=0.0, window=None, forward=False, tau=0.5)
    assert set(opt) <= set(o)
    o.update(opt)
    return name, dict(name=name, B=B, T=T, P=P, A=A, Ef=Ef, D=D, Ad=Ad, M=M, L=L, seed=seed, why=why, **o)


CASES = OrderedDict([
    _case("B1", 1, 1, "one utterance: a single partial row block"),
    _case("B5", 5, 1, "one partial row block of 5 rows"),
    _case("B17", 17, 1, "a second row block of one row"),
    _case("B64", 64, 24, "the full group: four row blocks, the 32 x 32-tile decoder cell (D % 64 == 0)"),
    _case("K1024", 3, 22, "D = Ef = 512: K = 1024, the 8-wave instance of the combined linear", T=3, P=16, A=32, Ef=512, D=512),
    _case("no_mask", 5, 1, "prenet_mask = NULL", no_mask=True),
    _case("controls", 5, 1, "row_comb together with dec_pre", controls=True),
    _case("zoneout", 5, 1, "zone_p = 0.1 with filled blocks", zone_p=0.1),
    _case("window", 5, 1, "the attention window (1 back, 2 forward)", window=(1, 2)),
    _case("forward", 5, 1, "forward attention", forward=True),
    _case("threshold", 5, 1, "stop_logit = logit(0.7)", tau=0.7),
])
CHAIN = ("B1", "B5", "B17", "B64")
OPTIONS = ("no_mask", "controls", "zoneout", "window", "forward", "threshold")


def threshold(case):
    """The case's stop threshold as the float32 logit the kernel is given (0.5 -> 0.0)."""
    return stop_logit(case["tau"])


def make_inputs(case, seed=None):
    """Seeded float32 raw weights and operands of one case (the kernels get exactly these, the float64 reference their upcasts)."""
    B, T, P, A, Ef, D, Ad, M, L = (case[k] for k in ("B", "T", "P", "A", "Ef", "D", "Ad", "M", "L"))
    g = torch.Generator().manual_seed(1000 + (case["seed"] if seed is None else seed))
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * sc
    lens = torch.randint(1, L + 1, (B,), generator=g)
    for b, n in enumerate((L, 1, 7)[:B]):
        lens[b] = n
    K = D + Ef
    Wd, Wc = rn(Ad, 32, sc=32 ** -0.5), rn(32, 2, KL, sc=0.3)
    inp = dict(W_pre1=rn(P, M, sc=(2.0 / M) ** 0.5), W_pre2=rn(P, P, sc=(2.0 / P) ** 0.5),
               W_mel=rn(M, K, sc=K ** -0.5), b_mel=rn(M, sc=0.1),
               W_gate=rn(1, K, sc=GATE_SCALE * K ** -0.5), b_gate=rn(1, sc=0.1) + GATE_BIAS,
               W_ih_att=rn(4 * A, P + Ef, sc=(P + Ef) ** -0.5), W_hh_att=rn(4 * A, A, sc=A ** -0.5),
               b_att_ih=rn(4 * A, sc=0.1), b_att_hh=rn(4 * A, sc=0.1),
               W_ih_dec=rn(4 * D, A + Ef, sc=(A + Ef) ** -0.5), W_hh_dec=rn(4 * D, D, sc=D ** -0.5),
               b_dec_ih=rn(4 * D, sc=0.1), b_dec_hh=rn(4 * D, sc=0.1),
               Wq=rn(Ad, A, sc=A ** -0.5), U=torch.einsum("af,fck->ack", Wd, Wc), v=rn(Ad, sc=2.0 * Ad ** -0.5),
               memory=rn(B, L, Ef), pm=rn(B, L, Ad),
               prenet_mask=(torch.rand(T, 2, B, P, generator=g) >= 0.5).double() * 2.0,
               cmel=rn(B, M, sc=0.3), dec_pre=rn(B, 4 * D, sc=0.3))
    if case["no_mask"]:
        inp["prenet_mask"] = None
    if not case["controls"]:
        inp["cmel"] = inp["dec_pre"] = None
    inp = {k: (None if x is None else x.float()) for k, x in inp.items()}
    inp["len"] = lens
    return inp


def build_comb(inp, round32=True):
    """W_comb [(P+M+1)][D+Ef] = [W_pre1 . W_mel ; W_mel ; W_gate], b_comb = [W_pre1 . b_mel ; b_mel ; b_gate] and, with controls,
    row_comb [B][P+M+1] = [W_pre1 . cmel_b ; cmel_b ; 0]: formed in float64 and rounded once to float32 (round32 = False: left in
    float64, for the comparison with the oracle)."""
    d = lambda k: inp[k].double()
    W = torch.cat([d("W_pre1") @ d("W_mel"), d("W_mel"), d("W_gate")], 0)
    b = torch.cat([d("W_pre1") @ d("b_mel"), d("b_mel"), d("b_gate")], 0)
    row = None
    if inp.get("cmel") is not None:
        cm = d("cmel")
        row = torch.cat([cm @ d("W_pre1").T, cm, torch.zeros(cm.shape[0], 1, dtype=torch.float64)], 1)
    f = (lambda x: None if x is None else x.float()) if round32 else (lambda x: x)
    return dict(W_comb=f(W), b_comb=f(b), row_comb=f(row))


# -----------------------------------------------------------------------------------------------------------------
# x16-tiled layouts (include/tacotron2_amd.h, T2LstmStep.xt): a (rows x K) matrix as [K/16][rows padded to 16][16]
# -----------------------------------------------------------------------------------------------------------------
def tile16(x):
    """(R, K) -> (K/16, Rp, 16); the pad rows are zero."""
    Rn, K = x.shape
    assert K % 16 == 0
    Rp = (Rn + 15) // 16 * 16
    out = torch.zeros(K // 16, Rp, 16, dtype=x.dtype)
    for c in range(K // 16):
        out[c, :Rn] = x[:, 16 * c:16 * c + 16]
    return out


def untile16(xt, rows):
    """(..., K/16, Rp, 16) -> (..., rows, K)."""
    nch = xt.shape[-3]
    return torch.cat([xt[..., c, :rows, :] for c in range(nch)], -1)


def tile_comb(W_comb, D, Ef):
    """W_comb_t [(Ef+D)/16][Npad][16]: the K chunks in the order [ctx | dec_h] of the tiled state (W_comb's own K order is that of
    xproj, [dec_h | ctx]), rows padded to 16 with zeros."""
    return tile16(torch.cat([W_comb[:, D:D + Ef], W_comb[:, :D]], 1))


# -----------------------------------------------------------------------------------------------------------------
# the restatement
# -----------------------------------------------------------------------------------------------------------------
def decode(case, inp, comb=None, dtype=torch.float64, T=None):
    """Frames [0, T) of the loop in `dtype` from the zero state.  Returns float64 tensors: mel (T,B,M), stop (T,B), align (B,T,L), the
    final xproj (B,D+Ef), att_h, att_c, dec_c, cum (B,.), the expected two slots of the tiled state untiled, xs (2,B,P+A+Ef+D), by the
    writer schedule of csrc/t2_infer.hip (prenet -> slot t&1; attention cell and context -> slot (t+1)&1; decoder cell -> slot t&1;
    frame 0 writes no prenet), and p1 (B,P) = what the call's tail leaves in the prenet scratch (unmasked)."""
    T = case["T"] if T is None else T
    P, A, Ef, D, L = (case[k] for k in ("P", "A", "Ef", "D", "L"))
    comb = comb or build_comb(inp)
    c = lambda x: None if x is None else x.to(dtype)
    W_comb, b_comb, row_comb = c(comb["W_comb"]), c(comb["b_comb"]), c(comb["row_comb"])
    W_pre2, pmask = c(inp["W_pre2"]), c(inp["prenet_mask"])
    W_ih_att, W_hh_att, b_att = c(inp["W_ih_att"]), c(inp["W_hh_att"]), c(inp["b_att_ih"]) + c(inp["b_att_hh"])
    W_ih_dec, W_hh_dec, b_dec = c(inp["W_ih_dec"]), c(inp["W_hh_dec"]), c(inp["b_dec_ih"]) + c(inp["b_dec_hh"])
    Wq, U, v, memory, pm, dec_pre = (c(inp[k]) for k in ("Wq", "U", "v", "memory", "pm", "dec_pre"))
    lens = inp["len"]
    B = memory.shape[0]
    z = None if case["zone_p"] == 0.0 else torch.full((), float(np.float32(case["zone_p"])), dtype=dtype)
    lmask = torch.arange(L)[None, :] >= lens[:, None]
    zeros = lambda *s: torch.zeros(*s, dtype=dtype)
    att_h, att_c, dec_h, dec_c, ctx = zeros(B, A), zeros(B, A), zeros(B, D), zeros(B, D), zeros(B, Ef)
    w, cum, xproj, p2 = zeros(B, L), zeros(B, L), zeros(B, D + Ef), zeros(B, P)
    peak = torch.zeros(B, dtype=torch.int64)
    xs = zeros(2, B, P + A + Ef + D)
    proj, align = [], []

    def combined(t, masked):
        y = xproj @ W_comb.T + b_comb
        if row_comb is not None:
            y = y + row_comb
        p1 = torch.relu(y[:, :P])
        if masked and pmask is not None:
            p1 = p1 * pmask[t, 0]
        return p1, y[:, P:]

    for t in range(T):
        if t > 0:
            p1, row = combined(t, True)
            proj.append(row)
            p2 = torch.relu(p1 @ W_pre2.T)
            if pmask is not None:
                p2 = p2 * pmask[t, 1]
            xs[t & 1, :, :P] = p2
        g = torch.cat([p2, ctx], 1) @ W_ih_att.T + att_h @ W_hh_att.T + b_att
        att_h, att_c = Z.zone_cell(g, att_c, att_h, None, z, z)
        # the energies / softmax / context arithmetic of attention_chain_ref.chain (folded filter U)
        mask = lmask | window_mask(peak, lens, L, case["window"]) if case["window"] else lmask
        q = att_h @ Wq.T
        wp = zeros(B, 2, L + 2 * PAD)
        wp[:, :, PAD:PAD + L] = torch.stack([w, cum], 1)
        loc = torch.einsum("bclk,ack->bla", wp.unfold(2, KL, 1), U)
        e = (torch.tanh(q[:, None, :] + loc + pm) * v[None, None, :]).sum(-1).masked_fill(mask, float("-inf"))
        p = torch.exp(e - e.max(1, keepdim=True).values)
        if case["forward"]:
            p = (p * _prior(w, t == 0, L, dtype, B)).masked_fill(lmask, 0.0)
        w = p / p.sum(1, keepdim=True)
        peak = w.argmax(1)
        ctx = torch.einsum("bl,ble->be", w, memory)
        cum = cum + w
        align.append(w)
        g = torch.cat([att_h, ctx], 1) @ W_ih_dec.T + dec_h @ W_hh_dec.T + b_dec
        if dec_pre is not None:
            g = g + dec_pre
        dec_h, dec_c = Z.zone_cell(g, dec_c, dec_h, None, z, z)
        xproj = torch.cat([dec_h, ctx], 1)
        xs[(t + 1) & 1, :, P:P + A] = att_h
        xs[(t + 1) & 1, :, P + A:P + A + Ef] = ctx
        xs[t & 1, :, P + A + Ef:] = dec_h
    p1, row = combined(T, False)
    proj.append(row)
    proj = torch.stack(proj, 0)
    out = dict(mel=proj[:, :, :-1], stop=proj[:, :, -1], align=torch.stack(align, 1), xproj=xproj, att_h=att_h, att_c=att_c,
               dec_c=dec_c, cum=cum, xs=xs, p1=p1)
    return {k: x.double() for k, x in out.items()}


def stop_rule(stop, thr):
    """The sticky rule over all frames of `stop` (T,B) against the float32 threshold `thr`: done [B] int32, state = [every utterance
    has stopped, frames emitted]."""
    below = stop.double() < float(np.float32(thr))
    done = below.any(0).to(torch.int32)
    return done, torch.tensor([int(bool(done.all())), stop.shape[0]], dtype=torch.int32)


def first_stops(stop, thr):
    """Per utterance the first frame with logit < thr, or None."""
    below = stop.double() < float(np.float32(thr))
    return [int(torch.nonzero(below[:, b])[0]) if bool(below[:, b].any()) else None for b in range(stop.shape[1])]


def stop_margin(stop, thr):
    """(smallest |logit - thr| over all frames and utterances, the distance the case must keep)."""
    s = stop.double()
    return float((s - float(np.float32(thr))).abs().min()), STOP_MARGIN * TOL["stop"] * float(s.abs().max())


def stop_pattern_ok(case, stop, thr):
    """B >= 3: two utterances first stop at different frames inside the run (the loop goes on after them) and one never stops."""
    if case["B"] < 3:
        return True
    first = first_stops(stop, thr)
    inside = {f for f in first if f is not None and f + 1 < stop.shape[0]}
    return len(inside) >= 2 and any(f is None for f in first)


# -----------------------------------------------------------------------------------------------------------------
# the comparison
# -----------------------------------------------------------------------------------------------------------------
OUTPUTS = ("mel", "stop", "align", "xproj", "att_h", "att_c", "dec_c", "cum", "xs")
SAMPLE_AXIS_1 = ("mel", "stop", "xs")


def by_sample(name, x):
    return x.transpose(0, 1) if name in SAMPLE_AXIS_1 else x


def errors(got, ref, names=OUTPUTS):
    """{output: (per_sample_rel, worst sample)}."""
    return {k: per_sample_rel(by_sample(k, got[k].double()), by_sample(k, ref[k])) for k in names}


# -----------------------------------------------------------------------------------------------------------------
# Tolerances: ONE constant per output for all cases, from the reference and not from the kernels (module docstring).
#   measured (worst case over CASES, one thread):
#     mel 6.32e-7 B64 | stop 1.34e-6 B64 | align 3.49e-7 B64 | xproj 3.76e-7 B17 | att_h 4.95e-7 B64 | att_c 6.11e-7 B64
#     dec_c 3.72e-7 B64 | cum 1.48e-7 B64 | xs 6.83e-7 B64
#   (each rounded up to two digits with at least 2 % of headroom for another CPU's float32 summation orders)
#   the kernels' own worst figures on an MI355X, for comparison only (tests/test_gpu_decode_chain.py prints them):
#     mel 6.36e-7 | stop 3.76e-6 | align 3.12e-7 | xproj 3.65e-7 | att_h 7.68e-7 | att_c 4.15e-7 | dec_c 5.06e-7 | cum 2.52e-7 | xs 5.58e-7
# -----------------------------------------------------------------------------------------------------------------
F32_ERR = dict(mel=6.5e-7, stop=1.4e-6, align=3.6e-7, xproj=3.9e-7, att_h=5.1e-7, att_c=6.3e-7, dec_c=3.8e-7, cum=1.6e-7, xs=7.0e-7)
TOL = {k: 16.0 * e for k, e in F32_ERR.items()}
TOL_CAP = C.TOL_CAP


def measure_f32_err():
    """{output: (worst per_sample_rel of the float32 restatement against float64 over CASES, case)} - one thread, as F32_ERR was measured."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        worst = {}
        for name, case in CASES.items():
            inp = make_inputs(case)
            comb = build_comb(inp)
            r64, r32 = decode(case, inp, comb, torch.float64), decode(case, inp, comb, torch.float32)
            for k, (e, _) in errors(r32, r64).items():
                if e > worst.get(k, (-1.0,))[0]:
                    worst[k] = (e, name)
    finally:
        torch.set_num_threads(threads)
    return worst


# -----------------------------------------------------------------------------------------------------------------
# t2_linear_rows: out[b][n] = act(x[b][:] . w[n][:] + bias[n]) * mask[b][n]
# -----------------------------------------------------------------------------------------------------------------
def linear_rows(x, w, bias, mask, relu, dtype=torch.float64):
    y = x.to(dtype) @ w.to(dtype).T
    if bias is not None:
        y = y + bias.to(dtype)
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = y * mask.to(dtype)
    return y.double()
