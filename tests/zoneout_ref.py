"""Float64-capable references for ZONEOUT on the decoder's two LSTM cells, for tests.  CPU only.

The rule (Krueger et al. 2017; ESPnet's ZoneOutCell), per cell and decoder step, with the dropout scale mask d and the zone masks
z_h, z_c in [0, 1] (0/1 draws in training, the rate itself in eval and decoding; an absent mask is 0):
    c~ = f * c_prev + i * g ;  h~ = o * tanh(c~) * d          (oracle.tacotron2_ref.lstm_cell, then the dropout mask)
    c  = z_c * c_prev + (1 - z_c) * c~ ;  h = z_h * h_prev + (1 - z_h) * h~
h and c are the carried state; h is what the attention query, the decoder LSTM and the projections see.

Three restatements, each with the dtype as a parameter:
  * decoder_step  - one decoder step composed from the oracle's pieces as tests/reduction_ref.py::_step is; without zone masks it IS
                    oracle.tacotron2_ref.decoder_step (tests/test_zoneout_host.py checks exact equality in float64);
  * cell_seq      - S steps of ONE recurrent cell, gates_s = pre_s + b1 + b2 + h_{s-1} . W^T, with autograd's gradients laid out as
                    the backward step kernels write them, and cell_seq_manual - the HAND-WRITTEN backward of include/tacotron2_amd.h
                    (T2LstmBwdStep) on the same inputs, with the two injectable faults of FAULTS;
  * chain         - tests/attention_chain_ref.py::chain with the rule in its attention-LSTM cell.

Metric: attention_chain_ref.per_sample_rel.  Tolerances: TOL = 16 x F32_ERR, F32_ERR = the float32 restatement's own error against
float64 over the committed cases, measured here (measure_f32_err) and re-measured by tests/test_zoneout_host.py - the convention of
tests/conv_path_ref.py."""
import functools
from collections import OrderedDict

import torch

from oracle import tacotron2_ref as R
from tests import attention_chain_ref as C

KL, PAD = C.KL, C.PAD


def zone(prev, new, z):
    """z * prev + (1 - z) * new; an absent mask is 0."""
    return new if z is None else z * prev + (1.0 - z) * new


def zone_cell(gates, c_prev, h_prev, drop, z_h, z_c):
    """One cell under the rule -> (h, c)."""
    h, c = R.lstm_cell(gates, c_prev)
    if drop is not None:
        h = h * drop
    return zone(h_prev, h, z_h), zone(c_prev, c, z_c)


def decoder_step(P, prev, st, memory, pm, lmask, att_drop, dec_drop, controls=None, zones=None, hook=None):
    """One decoder step on st = (att_h, att_c, ctx, w, w_cum, dec_h, dec_c) -> (mel, gate, st).  zones: None, or a dict with any
    of att_zone_h, att_zone_c, dec_zone_h, dec_zone_c (B, H).  hook: the attention hook of tests/reduction_ref.py (forward attention)."""
    zones = zones or {}
    att_h, att_c, ctx, w, w_cum, dec_h, dec_c = st
    g = torch.cat([prev, ctx], -1) @ P["decoder.att_rnn.weight_ih"].T + P["decoder.att_rnn.bias_ih"] \
        + att_h @ P["decoder.att_rnn.weight_hh"].T + P["decoder.att_rnn.bias_hh"]
    att_h, att_c = zone_cell(g, att_c, att_h, att_drop, zones.get("att_zone_h"), zones.get("att_zone_c"))
    ctx, w = R.attention_fwd(P, att_h, memory, pm, torch.stack([w, w_cum], 1), lmask)
    if hook is not None:
        w = hook(w, lmask)
        ctx = torch.einsum("bl,ble->be", w, memory)
    w_cum = w_cum + w
    xe = [controls] if controls is not None else []
    g = torch.cat([att_h, ctx] + xe, -1) @ P["decoder.lstm.weight_ih"].T + P["decoder.lstm.bias_ih"] \
        + dec_h @ P["decoder.lstm.weight_hh"].T + P["decoder.lstm.bias_hh"]
    dec_h, dec_c = zone_cell(g, dec_c, dec_h, dec_drop, zones.get("dec_zone_h"), zones.get("dec_zone_c"))
    hc = torch.cat([dec_h, ctx], -1)
    gate_o = hc @ P["decoder.gate.weight"].T + P["decoder.gate.bias"]
    mel_o = torch.cat([hc] + xe, -1) @ P["decoder.mel_out.weight"].T + P["decoder.mel_out.bias"]
    return mel_o, gate_o, (att_h, att_c, ctx, w, w_cum, dec_h, dec_c)


ZONE_KEYS = ("att_zone_h", "att_zone_c", "dec_zone_h", "dec_zone_c")


def model_fwd(P, d, r, *args, zones=None, rate=None, **kw):
    """tests/reduction_ref.py::reduction_fwd (same arguments and results: teacher forcing or decoding, any reduction factor r, the
    attention hook) with decoder_step as its step.  zones: {key of ZONE_KEYS: (S, B, H) masks, or (1, B, H) for every step};
    rate: instead of `zones`, the expectation rule of eval and decoding - every mask element is `rate`."""
    from tests import reduction_ref as RR
    dt = P["prenet.0.weight"].dtype
    count = [0]

    def step(P, prev, st, memory, pm, lmask, att_drop, dec_drop, controls, hook):
        s = count[0]
        count[0] += 1
        if rate is not None:
            z = {k: torch.full_like(st[0 if k.startswith("att") else 5], rate) for k in ZONE_KEYS}
        else:
            z = {k: _mask_at(v, s, dt) for k, v in (zones or {}).items()}
        return decoder_step(P, prev, st, memory, pm, lmask, att_drop, dec_drop, controls, z, hook)
    orig, RR._step = RR._step, step
    try:
        return RR.reduction_fwd(P, d, r, *args, **kw)
    finally:
        RR._step = orig


# -----------------------------------------------------------------------------------------------------------------
# One recurrent cell over S steps: the kernel-level reference
# -----------------------------------------------------------------------------------------------------------------
S_STEPS = 5
RATE = 0.1
# mask variants: 0/1 draws; fractional; ONE (B, H) block for every step (stride 0: how eval passes the rate); each mask alone
VARIANTS = ("01", "frac", "stride0", "h_only", "c_only")
# (B, H): B = 3 a partial row tile, 17 two tiles, 33 the persistent kernel's second 32-row block / the square tile's second row block;
# H = 16 / 32: one and two 16-column tiles of the backward; 64: the smallest H of the 32 x 32-tile forward; 528 at B = 17: 66
# workgroups, the smallest backward launch that takes the 4-wave packed kernel (8 waves up to 64 workgroups)
CELL_SHAPES = ((3, 16), (17, 32), (33, 32), (33, 64), (17, 528))


def cell_inputs(B, H, variant, S=S_STEPS):
    """Seeded float32 inputs of one cell sequence.  The 0/1 masks are drawn at rate 0.3 so that small cases hold both values;
    the fractional ones are uniform in [0, 1]."""
    g = torch.Generator().manual_seed(7000 + 31 * B + H + 1000 * VARIANTS.index(variant))
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * sc).float()
    inp = dict(W=rn(4 * H, H, sc=H ** -0.5), pre=rn(S, B, 4 * H), b1=rn(4 * H, sc=0.1), b2=rn(4 * H, sc=0.1),
               h0=rn(B, H, sc=0.5), c0=rn(B, H, sc=0.5), drop=(torch.rand(S, B, H, generator=g) >= 0.1).float() / 0.9,
               dh_ext=rn(S, B, H), dc_in=rn(B, H), dhz_in=rn(B, H))
    n = 1 if variant == "stride0" else S
    if variant == "01":
        zh, zc = ((torch.rand(n, B, H, generator=g) < 0.3).float() for _ in range(2))
    else:
        zh, zc = (torch.rand(n, B, H, generator=g) for _ in range(2))
    inp["zone_h"] = None if variant == "c_only" else zh
    inp["zone_c"] = None if variant == "h_only" else zc
    return inp


def _mask_at(z, s, dtype):
    return None if z is None else z[s if z.shape[0] > 1 else 0].to(dtype)


def cell_seq(inp, dtype=torch.float64):
    """Forward stashes h, c (S, B, H) (the CARRIED, zoned state), gates (S, B, 4H) activated in blocks i, f, g, o, and autograd's
    gradients of  sum_s h_s . dh_ext_s + c_{S-1} . dc_in + h_{S-1} . dhz_in:  dgates (S, B, 4H) w.r.t. pre, dc (B, H) w.r.t. c0 and
    dhz (B, H) w.r.t. the copy of h0 that enters step 0 through the zone mask only (what the kernels leave in `dc` / `dhz`)."""
    c = lambda x: x.to(dtype)
    W, b = c(inp["W"]), c(inp["b1"]) + c(inp["b2"])
    pre = c(inp["pre"]).clone().requires_grad_(True)
    c0 = c(inp["c0"]).clone().requires_grad_(True)
    h0_zone = c(inp["h0"]).clone().requires_grad_(True)
    S, B, H4 = pre.shape
    H = H4 // 4
    h, cc, h_zone_prev = c(inp["h0"]), c0, h0_zone
    st = dict(h=[], c=[], gates=[])
    obj = torch.zeros((), dtype=dtype)
    for s in range(S):
        g = pre[s] + b + h @ W.T
        st["gates"].append(torch.cat([R._sigmoid(g[:, :H]), R._sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]),
                                      R._sigmoid(g[:, 3 * H:])], 1))
        h, cc = zone_cell(g, cc, h_zone_prev, c(inp["drop"][s]), _mask_at(inp["zone_h"], s, dtype), _mask_at(inp["zone_c"], s, dtype))
        h_zone_prev = h
        st["h"].append(h); st["c"].append(cc)
        obj = obj + (h * c(inp["dh_ext"][s])).sum()
    obj = obj + (cc * c(inp["dc_in"])).sum() + (h * c(inp["dhz_in"])).sum()
    obj.backward()
    out = {k: torch.stack(v, 0).detach() for k, v in st.items()}
    out["dgates"], out["dc"] = pre.grad, c0.grad
    out["dhz"] = h0_zone.grad if h0_zone.grad is not None else torch.zeros(B, H, dtype=dtype)
    return {k: v.double() for k, v in out.items()}


FAULTS = ("tanh_c_cur", "no_dhz_carry")


def cell_seq_manual(inp, fwd, dtype=torch.float64, fault=None):
    """The hand-written backward (T2LstmBwdStep in include/tacotron2_amd.h) over steps S-1 .. 0 on the forward stashes `fwd` (gates,
    c of cell_seq; h is not needed) -> dgates, dc, dhz as cell_seq returns them.
    fault: "tanh_c_cur" - tanh of the STORED c (zoned) instead of the recomputed c~;  "no_dhz_carry" - Dh = dx without the carry."""
    assert fault is None or fault in FAULTS
    c = lambda x: x.to(dtype)
    W = c(inp["W"])
    S, B, H4 = inp["pre"].shape
    H = H4 // 4
    gates, cst = c(fwd["gates"]), c(fwd["c"])
    dc, dhz = c(inp["dc_in"]), c(inp["dhz_in"])
    dg_next = torch.zeros(B, 4 * H, dtype=dtype)
    dgs = [None] * S
    for s in range(S - 1, -1, -1):
        i, f, g, o = (gates[s][:, k * H:(k + 1) * H] for k in range(4))
        c_prev = cst[s - 1] if s > 0 else c(inp["c0"])
        zh, zc = _mask_at(inp["zone_h"], s, dtype), _mask_at(inp["zone_c"], s, dtype)
        zh = torch.zeros(B, H, dtype=dtype) if zh is None else zh
        zc = torch.zeros(B, H, dtype=dtype) if zc is None else zc
        dx = dg_next @ W + c(inp["dh_ext"][s])
        Dh = dx if fault == "no_dhz_carry" else dx + dhz
        dht = (1 - zh) * Dh * c(inp["drop"][s])
        dhz = zh * Dh
        tc = torch.tanh(cst[s] if fault == "tanh_c_cur" else f * c_prev + i * g)
        dct = (1 - zc) * dc + dht * o * (1 - tc * tc)
        d_o = dht * tc * o * (1 - o)
        d_i = dct * g * i * (1 - i)
        d_f = dct * c_prev * f * (1 - f)
        d_g = dct * i * (1 - g * g)
        dc = dct * f + zc * dc
        dg_next = torch.cat([d_i, d_f, d_g, d_o], 1)
        dgs[s] = dg_next
    return dict(dgates=torch.stack(dgs, 0).double(), dc=dc.double(), dhz=dhz.double())


@functools.lru_cache(maxsize=None)
def cell_reference(B, H, variant):
    """(inputs, float64 reference) of one cell sequence, computed once and shared (treat as read-only)."""
    inp = cell_inputs(B, H, variant)
    return inp, cell_seq(inp, torch.float64)


CELL_FWD, CELL_BWD = ("h", "c", "gates"), ("dgates", "dc", "dhz")


def cell_errors(got, ref, names):
    """{output: per_sample_rel}; the stashes are time-major (S, B, ...): per sample over all steps."""
    out = {}
    for k in names:
        g, r = got[k].double(), ref[k]
        if r.dim() == 3:
            g, r = g.transpose(0, 1), r.transpose(0, 1)
        out[k] = C.per_sample_rel(g, r)[0]
    return out


# -----------------------------------------------------------------------------------------------------------------
# The attention chain with the rule in its cell
# -----------------------------------------------------------------------------------------------------------------
def _chain_case(name, B, A, kind, bwd="plain"):
    """bwd: which backward entry the GPU test drives - "plain" (t2_attn_seq_bwd's path), "stash" (energy gradients stashed, dpmT / dv /
    dU rebuilt by t2_attn_acc_bwd: what the engine runs) or "forward" (forward attention in the forward and the backward, with the
    stash: what the engine runs under train_forward_attention)."""
    return name, dict(name=name, B=B, L=5, T=4, A=A, Ad=16, Ef=32, drop=True, dalign=True, tiled=True, mel_tail=False, kind=kind, bwd=bwd,
                      why=f"L = 5, T = 4 with zone masks of kind {kind}, backward {bwd}")


# B = 3 / A = 32: the one-tile packed cell; B = 33 / A = 64: two 32-row blocks, the 32 x 32-tile forward cell
CHAIN_CASES = OrderedDict([_chain_case("B3_01", 3, 32, "01"), _chain_case("B3_frac", 3, 32, "frac"),
                           _chain_case("B33_frac", 33, 64, "frac"), _chain_case("B33_stride0", 33, 64, "stride0"),
                           _chain_case("B3_frac_stash", 3, 32, "frac", "stash"), _chain_case("B33_01_stash", 33, 64, "01", "stash"),
                           _chain_case("B3_01_forward", 3, 32, "01", "forward"), _chain_case("B33_frac_forward", 33, 64, "frac", "forward")])


def chain_inputs(case):
    """attention_chain_ref.make_inputs plus zone_h / zone_c (T, B, A), or (1, B, A) for the stride-0 kind."""
    inp = C.make_inputs(case, seed=9000 + 7 * case["B"] + sum(ord(ch) for ch in case["kind"] + case["bwd"].replace("plain", "")))
    # Texts of 3 .. 5 positions behind the two fixed samples (len[0] = L, len[1] = 1).  A two-position text makes per_sample_rel
    # ill-conditioned for dq / dpm / dv / dU: the softmax backward of two weights near (1, 0) leaves a dq a hundred times below the
    # terms it is the difference of (seen on the chain WITHOUT zone masks: 2.4e-5 on such a sample at an absolute error of 1.2e-6
    # against gradients of size 4).  That is the attention backward's conditioning, covered by tests/test_gpu_attention_chain.py,
    # and no property of the cell that this file is about.
    for b in range(2, case["B"]):
        inp["len"][b] = 3 + b % 3
    g = torch.Generator().manual_seed(9100 + case["B"])
    n = 1 if case["kind"] == "stride0" else case["T"]
    shape = (n, case["B"], case["A"])
    if case["kind"] == "01":
        inp["zone_h"], inp["zone_c"] = ((torch.rand(*shape, generator=g) < 0.3).float() for _ in range(2))
    else:
        inp["zone_h"], inp["zone_c"] = (torch.rand(*shape, generator=g) for _ in range(2))
    return inp


def chain(inp, dtype=torch.float64, forward=False):
    """attention_chain_ref.chain (same inputs, same outputs, same objective) with zone_cell in place of the plain cell; att_h / att_c
    are the carried (zoned) state.  Without zone masks in `inp` it is that function.  forward: forward attention - the weights of
    frame t are the softmax terms times q_t(n) = 0.5 w_{t-1}(n) + 0.5 w_{t-1}(n-1) + 1e-8 (w_{-1} one-hot at 0), renormalised; without
    zone masks that is tests/forward_attention_chain_ref.py::chain_fa from the zero state."""
    c = lambda x: None if x is None else x.to(dtype)
    W_ih_ctx, W_hh, Wq, U, v = (c(inp[k]) for k in ("W_ih_ctx", "W_hh", "Wq", "U", "v"))
    memory, att_drop = c(inp["memory"]), c(inp["att_drop"])
    dh_ext, dc1, dc2, da = (c(inp[k]) for k in ("dh_ext", "dctx_ext1", "dctx_ext2", "dalign"))
    lens = inp["len"]
    T, B, A4 = inp["pre"].shape
    A, L, Ad = A4 // 4, memory.shape[1], v.shape[0]
    vB = v[None].expand(B, Ad).clone().requires_grad_(True)
    UB = U[None].expand(B, Ad, 2, KL).clone().requires_grad_(True)
    pm = c(inp["pm"]).clone().requires_grad_(True)
    pre = c(inp["pre"]).clone().requires_grad_(True)
    mask = torch.arange(L)[None, :] >= lens[:, None]
    att_h = torch.zeros(B, A, dtype=dtype)
    att_c = torch.zeros(B, A, dtype=dtype)
    ctx = torch.zeros(B, memory.shape[2], dtype=dtype)
    w = torch.zeros(B, L, dtype=dtype)
    cum = torch.zeros(B, L, dtype=dtype)
    obj = torch.zeros((), dtype=dtype)
    st = {k: [] for k in ("att_h", "att_c", "ctx", "gates", "cum", "th", "align", "q")}
    for t in range(T):
        g = pre[t] + ctx @ W_ih_ctx.T + att_h @ W_hh.T
        st["gates"].append(torch.cat([R._sigmoid(g[:, :A]), R._sigmoid(g[:, A:2 * A]), torch.tanh(g[:, 2 * A:3 * A]),
                                      R._sigmoid(g[:, 3 * A:])], 1))
        att_h, att_c = zone_cell(g, att_c, att_h, None if att_drop is None else att_drop[t],
                                 _mask_at(inp.get("zone_h"), t, dtype), _mask_at(inp.get("zone_c"), t, dtype))
        q = att_h @ Wq.T
        q.retain_grad()
        wp = torch.zeros(B, 2, L + 2 * PAD, dtype=dtype)
        wp[:, :, PAD:PAD + L] = torch.stack([w, cum], 1)
        loc = torch.einsum("bclk,back->bla", wp.unfold(2, KL, 1), UB)
        th = torch.tanh(q[:, None, :] + loc + pm)
        e = (th * vB[:, None, :]).sum(-1).masked_fill(mask, float("-inf"))
        p = torch.exp(e - e.max(1, keepdim=True).values)
        if forward:
            a_prev = w
            if t == 0:
                a_prev = torch.zeros(B, L, dtype=dtype)
                a_prev[:, 0] = 1.0
            p = p * (0.5 * a_prev + 0.5 * torch.cat([torch.zeros(B, 1, dtype=dtype), a_prev[:, :-1]], 1) + 1e-8)
        w = p / p.sum(1, keepdim=True)
        ctx = torch.einsum("bl,ble->be", w, memory)
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


@functools.lru_cache(maxsize=None)
def chain_reference(name):
    inp = chain_inputs(CHAIN_CASES[name])
    return inp, chain(inp, torch.float64, forward=CHAIN_CASES[name]["bwd"] == "forward")


# -----------------------------------------------------------------------------------------------------------------
# Tolerances: TOL[k] = 16 x F32_ERR[k], F32_ERR[k] = the largest per_sample_rel between the float32 and the float64 run of the
# restatement over the committed cases (cell.*: CELL_SHAPES x VARIANTS; chain.*: CHAIN_CASES), measured on the CPU with one thread and
# rounded up to two digits with >= 2 % of headroom.  tests/test_zoneout_host.py re-measures them and fails if a case exceeds its
# constant or a constant is more than twice what it measures.  The factor 16 covers what differs between two correct float32
# implementations: reduction orders (4 or 8 waves splitting K, MFMA accumulation) and the device's tanh / sigmoid against libm's.
# -----------------------------------------------------------------------------------------------------------------
#   measured (worst case):  cell.h 6.80e-7 B17_H528_c_only | cell.c 3.85e-7 B17_H528_h_only | cell.gates 9.45e-7 B17_H528_c_only
#     cell.dgates 4.21e-7 B17_H528_stride0 | cell.dc 3.76e-7 B33_H32_h_only | cell.dhz 2.99e-7 B33_H32_01
#     chain.att_h 3.74e-7 B33_frac_forward | chain.ctx 3.47e-7 B33_stride0 | chain.att_c 3.51e-7 B33_01_stash | chain.gates 5.67e-7 B33_stride0
#     chain.cum 1.24e-7 B33_frac | chain.align 2.41e-7 B33_stride0 | chain.th 3.19e-7 B33_frac | chain.dgates 3.48e-7 B33_stride0
#     chain.dq 1.16e-6 B33_stride0 | chain.dctx_tot 1.65e-7 B33_frac | chain.dpm 1.52e-6 B33_01_stash | chain.dv 1.16e-6 B33_frac
#     chain.dU 1.39e-6 B33_stride0
F32_ERR = {
    "cell.h": 7.0e-7, "cell.c": 4.0e-7, "cell.gates": 9.7e-7, "cell.dgates": 4.3e-7, "cell.dc": 3.9e-7, "cell.dhz": 3.1e-7,
    "chain.att_h": 3.9e-7, "chain.ctx": 3.6e-7, "chain.att_c": 3.6e-7, "chain.gates": 5.8e-7, "chain.cum": 1.3e-7,
    "chain.align": 2.5e-7, "chain.th": 3.3e-7, "chain.dgates": 3.6e-7, "chain.dq": 1.2e-6, "chain.dctx_tot": 1.7e-7,
    "chain.dpm": 1.6e-6, "chain.dv": 1.2e-6, "chain.dU": 1.5e-6,
}
TOL = {k: 16.0 * e for k, e in F32_ERR.items()}


def cell_f32_errors(B, H, variant):
    inp, r64 = cell_reference(B, H, variant)
    r32 = cell_seq(inp, torch.float32)
    names = [k for k in CELL_FWD + CELL_BWD if not (k == "dhz" and variant == "c_only")]      # (exactly zero without zone_h)
    return {"cell." + k: e for k, e in cell_errors(r32, r64, names).items()}


def chain_f32_errors(name):
    inp, r64 = chain_reference(name)
    r32 = chain(inp, torch.float32, forward=CHAIN_CASES[name]["bwd"] == "forward")
    return {"chain." + k: e for k, (e, _) in C.errors(r32, r64, inp["len"]).items()}


def measure_f32_err():
    """{output: (worst per_sample_rel, case)} over the committed cases, one thread."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    worst = {}

    def take(errs, case):
        for k, e in errs.items():
            if e > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (e, case)
    try:
        for B, H in CELL_SHAPES:
            for variant in VARIANTS:
                take(cell_f32_errors(B, H, variant), f"B{B}_H{H}_{variant}")
        for name in CHAIN_CASES:
            take(chain_f32_errors(name), name)
    finally:
        torch.set_num_threads(threads)
    return worst


if __name__ == "__main__":
    for k, (e, case) in measure_f32_err().items():
        print(f"{k} {e:.3e} {case}")
