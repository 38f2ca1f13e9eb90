"""Zoneout on the GPU.  Kernel level, through the C ABI: every forward path of the LSTM step kernels (generic, packed, 32 x 32
tiles, persistent), both backward kernels, the attention chain and the mask generator against the float64 references of
tests/zoneout_ref.py.

Sequence cases run S = 5 steps so that h, c (forward) and the dhz, dc carries (backward) all pass through several steps.  Everything a
call writes is NaN-filled first; dc and dhz go in non-zero; with zone masks the backward gets a NaN-filled c_cur (it must recompute
c~ from the stash, the stored c is the zoned one).  The backward runs on the float32 casts of the REFERENCE's stashes, so a forward
error cannot hide a backward one.

Metric and tolerances: attention_chain_ref.per_sample_rel against zoneout_ref.TOL = 16 x the float32 restatement's own error
(anchored by tests/test_zoneout_host.py, which also shows that the two likely backward mistakes land far above the constants).

Model level (second half of the file): the engine's training step, eval forward and decode against zoneout_ref.model_fwd, the
generated masks, zoneout = 0 against a model without the argument, cell_dropout = 0, the checkpoint round trip."""
import contextlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import zoneout_ref as Z  # noqa: E402
from tests import attention_chain_ref as C  # noqa: E402

S = Z.S_STEPS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _tile16(x, Bp):
    B, K = x.shape
    out = torch.zeros(K // 16, Bp, 16)
    out[:, :B] = x.reshape(B, K // 16, 16).permute(1, 0, 2)
    return out


def _untile16(xt, B):
    nch = xt.shape[-3]
    return xt[..., :B, :].transpose(-3, -2).reshape(*xt.shape[:-3], B, nch * 16)


def _pack_fwd(dev, W, H):
    from tacotron2_amd import _lib
    K = W.shape[1]
    segs = (_lib.S["T2Seg"] * 1)()
    segs[0].w = W.data_ptr(); segs[0].ldw = K; segs[0].K = K
    wp = _nan(dev, H // 4 * ((K // 16 + 15) // 16 * 16) * 256)
    _lib.call("t2_lstm_pack_fwd", segs, 1, H, wp, _stream())
    return wp


def _report(tag, errs, prefix):
    print(f"[zoneout] {tag}: " + ", ".join(f"{k} {e:.2e} /{Z.TOL[prefix + k]:.1e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e <= Z.TOL[prefix + k]}
    assert not bad, f"{tag}: outputs over their constant {bad}"


# ---------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------
def run_cell_fwd(dev, path, B, H, variant, alias=False):
    """S steps of one recurrent cell (input of step s = h of step s-1) on one of the four forward paths; returns h, c (S, B, H),
    gates (S, B, 4H) in the reference's layout, the tiled copy of h (or None) and the in-place buffer of the aliased run."""
    from tacotron2_amd import _lib
    inp, _ = Z.cell_reference(B, H, variant)
    d = {k: (None if v is None else v.contiguous().to(dev)) for k, v in inp.items()}
    Bp = (B + 15) // 16 * 16
    tiled = path != "generic"
    hrow, cst, gs = _nan(dev, S + 1, B, H), _nan(dev, S + 1, B, H), _nan(dev, S, B, 4 * H)
    hrow[0], cst[0] = d["h0"], d["c0"]
    kw = dict(B=B, H=H, nseg=1, pre=d["pre"], ldpre=4 * H, bias1=d["b1"], bias2=d["b2"], c_prev=cst[0], ldc_prev=H, drop=d["drop"],
              lddrop=H, h_out=hrow[1], ldh=H, c_out=cst[1], ldc_out=H, gates_out=gs, ldg=4 * H, zone_h=d["zone_h"], ldzone_h=H,
              zone_c=d["zone_c"], ldzone_c=H, h_prev=hrow[0], ldh_prev=H)
    zs = 0 if variant == "stride0" else B * H
    ikw = dict(pre=B * 4 * H, c_prev=B * H, drop=B * H, h_out=B * H, c_out=B * H, gates_out=B * 4 * H, zone_h=zs, zone_c=zs,
               h_prev=B * H)
    ht = hbuf = None
    if tiled:
        # T2LstmStep.xt: pad rows must be finite - zero-filled, the rows the kernel writes NaN-filled
        ht = torch.zeros(S + 1, H // 16, Bp, 16, device=dev)
        ht[1:, :, :B] = float("nan")
        ht[0] = _tile16(inp["h0"], Bp).to(dev)
        kw.update(wpacked=_pack_fwd(dev, d["W"], H), xt=ht[0], ht_out=ht[1], ht_col0=0)
        ikw.update(xt=H * Bp, ht_out=H * Bp)
    if alias:       # h in place: h_prev IS h_out; the stash of every step goes out through the second copy
        hbuf = d["h0"].clone()
        kw.update(h_out=hbuf, h_prev=hbuf, h_out2=hrow[1], ldh2=H)
        ikw.update(h_out=0, h_prev=0, h_out2=B * H)
    st = _lib.make("T2LstmStep", **kw)
    st.seg[0].x = hrow.data_ptr(); st.seg[0].ldx = H; st.seg[0].w = d["W"].data_ptr(); st.seg[0].ldw = H; st.seg[0].K = H
    inc = _lib.make("T2LstmStride", **ikw)
    inc.seg_x[0] = B * H
    if path == "persist":
        sync = torch.zeros(320, dtype=torch.int32, device=dev)
        _lib.call("t2_lstm_seq_fwd_persist", st, inc, S, sync, _stream())
        torch.cuda.synchronize()
        assert int(sync[256]) == 0, "an inter-workgroup wait timed out"
    else:
        _lib.call("t2_lstm_seq_fwd", st, inc, 1, S, _stream())
        torch.cuda.synchronize()
    got = dict(h=hrow[1:].cpu(), c=cst[1:].cpu(), gates=gs.cpu().view(S, B, H, 4).transpose(2, 3).reshape(S, B, 4 * H))
    return got, (None if ht is None else ht.cpu()), (None if hbuf is None else hbuf.cpu())


# (path, B, H): generic and packed at one, two and four row tiles; the 32 x 32-tile kernel (33..64 rows, H % 64 == 0); the persistent
# kernel with one tile, two tiles and a second 32-row block (a second launch that must load ITS rows of h_prev)
FWD_PATHS = [("generic", 3, 16), ("generic", 17, 32), ("generic", 33, 32), ("packed", 3, 16), ("packed", 17, 32), ("packed", 33, 32),
             ("square", 33, 64), ("persist", 3, 16), ("persist", 17, 32), ("persist", 33, 32)]


@pytest.mark.parametrize("variant", Z.VARIANTS + ("alias",))
@pytest.mark.parametrize("path,B,H", FWD_PATHS)
def test_cell_forward_against_float64(dev, path, B, H, variant):
    alias = variant == "alias"
    variant = "frac" if alias else variant
    _, ref = Z.cell_reference(B, H, variant)
    got, ht, hbuf = run_cell_fwd(dev, path, B, H, variant, alias=alias)
    _report(f"fwd {path} B{B} H{H} {variant}{' alias' if alias else ''}", Z.cell_errors(got, ref, Z.CELL_FWD), "cell.")
    if ht is not None:      # the tiled copy holds the same bits
        assert torch.equal(_untile16(ht[1:], B), got["h"])
    if hbuf is not None:    # the in-place buffer ends as the last step's h
        assert torch.equal(hbuf, got["h"][-1])


def test_zone_masks_of_zero_and_one(dev):
    """All-zero masks give the plain cell's h and c to the last bit but the sign of a zero; all-one masks keep h0 and c0 exactly."""
    from tacotron2_amd import _lib
    B, H = 17, 32
    inp, _ = Z.cell_reference(B, H, "frac")
    d = {k: (None if v is None else v.contiguous().to(dev)) for k, v in inp.items()}
    outs = {}
    for name, z in (("none", None), ("zero", torch.zeros(B, H, device=dev)), ("one", torch.ones(B, H, device=dev))):
        h, c = _nan(dev, B, H), _nan(dev, B, H)
        st = _lib.make("T2LstmStep", B=B, H=H, nseg=1, pre=d["pre"], ldpre=4 * H, bias1=d["b1"], bias2=d["b2"], c_prev=d["c0"], ldc_prev=H,
                       drop=d["drop"], lddrop=H, h_out=h, ldh=H, c_out=c, ldc_out=H, zone_h=z, ldzone_h=H, zone_c=z, ldzone_c=H,
                       h_prev=None if z is None else d["h0"], ldh_prev=H)
        st.seg[0].x = d["h0"].data_ptr(); st.seg[0].ldx = H; st.seg[0].w = d["W"].data_ptr(); st.seg[0].ldw = H; st.seg[0].K = H
        _lib.call("t2_lstm_step_fwd", st, 1, _stream())
        torch.cuda.synchronize()
        outs[name] = (h.cpu(), c.cpu())
    assert bool((outs["zero"][0] == outs["none"][0]).all()) and bool((outs["zero"][1] == outs["none"][1]).all())
    assert torch.equal(outs["one"][0], inp["h0"]) and torch.equal(outs["one"][1], inp["c0"])


# ---------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------
def run_cell_bwd(dev, packed, B, H, variant):
    """Steps S-1 .. 0 of t2_lstm_seq_bwd on the float32 casts of the reference's stashes -> dgates (S, B, 4H), dc, dhz (B, H)."""
    from tacotron2_amd import _lib
    inp, ref = Z.cell_reference(B, H, variant)
    d = {k: (None if v is None else v.contiguous().to(dev)) for k, v in inp.items()}
    gst = ref["gates"].float().view(S, B, 4, H).transpose(2, 3).contiguous().to(dev)          # gate-interleaved [b][u][4]
    cst = torch.cat([inp["c0"][None], ref["c"].float()], 0).contiguous().to(dev)               # the CARRIED (zoned) c, slot s = c_{s-1}
    c_cur = _nan(dev, B, H)
    Zs = _nan(dev, S + 1, B, 4 * H)
    Zs[S] = 0
    dc, dhz = d["dc_in"].clone(), d["dhz_in"].clone()
    wtp = None
    if packed:
        wtp = _nan(dev, (H + 15) // 16 * ((4 * H // 16 + 31) // 32 * 32) * 256)
        _lib.call("t2_lstm_pack_bwd", d["W"], H, 4 * H, None, 0, 0, H, wtp, _stream())
    last = lambda z: None if z is None else z[z.shape[0] - 1]
    st = _lib.make("T2LstmBwdStep", B=B, H=H, N4=4 * H, dg_next=Zs[S], lddg=4 * H, W=d["W"], ldw=H, wtpacked=wtp, ncols=H, epi=1,
                   ext1=d["dh_ext"][S - 1], ldx1=H, drop=d["drop"][S - 1], lddrop=H, gates=gst[S - 1], ldgs=4 * H, c_prev=cst[S - 1],
                   ldcp=H, c_cur=c_cur, ldcc=H, dc=dc, lddc=H, dg_out=Zs[S - 1], ldgo=4 * H, zone_h=last(d["zone_h"]), ldzone_h=H,
                   zone_c=last(d["zone_c"]), ldzone_c=H, dhz=dhz, lddhz=H)
    zs = 0 if variant == "stride0" else -B * H
    inc = _lib.make("T2LstmBwdStride", dg=-B * 4 * H, ext1=-B * H, drop=-B * H, gates=-B * 4 * H, c_prev=-B * H, c_cur=0, zone_h=zs,
                    zone_c=zs)
    _lib.call("t2_lstm_seq_bwd", st, inc, 1, S, _stream())
    torch.cuda.synchronize()
    return dict(dgates=Zs[:S].cpu(), dc=dc.cpu(), dhz=dhz.cpu())


# (packed, B, H): the generic kernel and the 8-wave packed kernel at one, two and three row tiles; (17, 528) = 66 workgroups is the
# smallest launch of the 4-wave packed kernel
BWD_PATHS = [(False, 3, 16), (False, 17, 32), (False, 33, 32), (True, 3, 16), (True, 17, 32), (True, 33, 32), (True, 17, 528)]


@pytest.mark.parametrize("variant", Z.VARIANTS)
@pytest.mark.parametrize("packed,B,H", BWD_PATHS)
def test_cell_backward_against_float64(dev, packed, B, H, variant):
    _, ref = Z.cell_reference(B, H, variant)
    got = run_cell_bwd(dev, packed, B, H, variant)
    names = [k for k in Z.CELL_BWD if not (k == "dhz" and variant == "c_only")]
    _report(f"bwd {'packed' if packed else 'generic'} B{B} H{H} {variant}", Z.cell_errors(got, ref, names), "cell.")
    if variant == "c_only":      # no zone_h: nothing is handed to h_{t-1} through the mask
        assert float(got["dhz"].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the attention chain
# ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _zoned_chain_calls(zone, case, dev):
    """The runners of tests/test_gpu_attention_chain.py call t2_attn_seq_fwd / t2_attn_seq_bwd on the operand blocks they build:
    send those two calls to the entries that take the T2AttnZone block beside them, in the case's backward variant (zoneout_ref:
    "plain"; "stash" - NaN-filled energy-gradient stash, then t2_attn_acc_bwd over all frames; "forward" - T2AttnSeq.forward = 1,
    the stash and a NaN-filled dprior workspace, which selects the forward-attention backward)."""
    from tacotron2_amd import _lib
    orig = _lib.call
    B, L, T, mode = case["B"], case["L"], case["T"], case["bwd"]

    def call(name, *args):
        if name == "t2_attn_seq_fwd":
            args[0].forward = 1 if mode == "forward" else 0
            return orig("t2_attn_seq_fwd_zone", args[0], zone, args[1])
        if name == "t2_attn_seq_bwd":
            if mode == "plain":
                return orig("t2_attn_seq_bwd_zone", args[0], None, 0, None, zone, args[1])
            stash = _nan(dev, T, B, L)
            dprior = _nan(dev, 2, B, L) if mode == "forward" else None
            orig("t2_attn_seq_bwd_zone", args[0], stash, B * L, dprior, zone, args[1])
            return orig("t2_attn_acc_bwd", args[0], stash, B * L, 0, T, args[1])
        return orig(name, *args)
    _lib.call = call
    try:
        yield
    finally:
        _lib.call = orig


@pytest.mark.parametrize("name", list(Z.CHAIN_CASES))
def test_attention_chain_against_float64(dev, name):
    """The chain at L = 5, T = 4 with zone masks on the attention-LSTM cell, forward and backward, in the three backward variants
    (t2_attn_seq_bwd's path; the stash + t2_attn_acc_bwd pair; forward attention with the stash); the backward reads the forward
    kernel's stashes, as the engine does (its c~ is recomputed from them)."""
    from tests import test_gpu_attention_chain as TC
    case = Z.CHAIN_CASES[name]
    B, T, A = case["B"], case["T"], case["A"]
    inp, ref = Z.chain_reference(name)
    d = TC._device_inputs(dev, inp)
    zh, zc = inp["zone_h"].contiguous().to(dev), inp["zone_c"].contiguous().to(dev)
    from tacotron2_amd import _lib
    dhz = torch.zeros(B, A, device=dev)
    zone = _lib.make("T2AttnZone", zone_h=zh, zone_c=zc, stride=0 if case["kind"] == "stride0" else B * A, dhz=dhz)
    with _zoned_chain_calls(zone, case, dev):
        s = TC.run_fwd(dev, case, d)
    got, raw = TC.fwd_to_ref_layout(case, s)
    errs = {k: e for k, (e, _) in C.errors(got, ref, inp["len"], names=C.FWD_OUTPUTS).items()}
    _report(f"chain {name} fwd", errs, "chain.")
    assert torch.equal(_untile16(raw["xdec_t"], B), raw["xdec"])
    with _zoned_chain_calls(zone, case, dev):
        out, Zc, _ = TC.run_bwd(dev, case, d, s, tiled=True)
    errs = {k: e for k, (e, _) in C.errors(out, ref, inp["len"], names=C.BWD_OUTPUTS).items()}
    _report(f"chain {name} bwd", errs, "chain.")
    assert not C.single_position_violations(out, inp, ref)
    assert bool(torch.isfinite(dhz).all())


# ---------------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(dev):
    from tacotron2_amd import _lib
    B, H = 3, 16
    x, W = torch.zeros(B, H, device=dev), torch.zeros(4 * H, H, device=dev)
    z, lens = torch.zeros(B, H, device=dev), torch.full((B,), 9, dtype=torch.int32, device=dev)

    def fwd(**kw):
        st = _lib.make("T2LstmStep", B=B, H=H, nseg=1, h_out=torch.zeros(B, H, device=dev), ldh=H, ldzone_h=H, ldzone_c=H, ldh_prev=H, **kw)
        st.seg[0].x = x.data_ptr(); st.seg[0].ldx = H; st.seg[0].w = W.data_ptr(); st.seg[0].ldw = H; st.seg[0].K = H
        _lib.call("t2_lstm_step_fwd", st, 1, _stream())
    fwd(zone_h=z, h_prev=x)
    with pytest.raises(_lib.T2Error, match="h_prev"):
        fwd(zone_h=z)
    with pytest.raises(_lib.T2Error, match="h_prev"):
        fwd(zone_c=z)
    with pytest.raises(_lib.T2Error, match="len"):
        fwd(zone_c=z, h_prev=x, len=lens, t=0)

    def bwd(**kw):
        st = _lib.make("T2LstmBwdStep", B=B, H=H, N4=4 * H, dg_next=torch.zeros(B, 4 * H, device=dev), lddg=4 * H, W=W, ldw=H, ncols=H,
                       epi=1, gates=torch.full((B, 4 * H), 0.5, device=dev), ldgs=4 * H, c_cur=x, ldcc=H,
                       dc=torch.zeros(B, H, device=dev), lddc=H, dg_out=torch.zeros(B, 4 * H, device=dev), ldgo=4 * H, ldzone_h=H,
                       ldzone_c=H, lddhz=H, **kw)
        _lib.call("t2_lstm_step_bwd", st, 1, _stream())
    bwd(zone_h=z, dhz=torch.zeros(B, H, device=dev))
    with pytest.raises(_lib.T2Error, match="dhz"):
        bwd(zone_h=z)
    with pytest.raises(_lib.T2Error, match="len"):
        bwd(zone_c=z, dhz=torch.zeros(B, H, device=dev), len=lens, t=0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# the mask generator
# ---------------------------------------------------------------------------------------------------------------------------
def test_bernoulli_mask_generator(dev):
    from tacotron2_amd import _lib
    n, p = 1 << 20, 0.1

    def draw(seed, sid, n=n, p=p):
        m = _nan(dev, n)
        _lib.call("t2_philox_bernoulli", m, n, p, seed, sid, _stream())
        torch.cuda.synchronize()
        return m
    a = draw(1234, 7)
    assert bool(((a == 0) | (a == 1)).all())                       # 0 or 1: no rescaling
    share = float(a.double().mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"[zoneout] share of ones {share:.6f} at p = {p}, n = {n}: {abs(share - p) / sigma:.2f} sigma")
    assert abs(share - p) <= 1.5e-3                                # 5 sigma (sigma = sqrt(p (1 - p) / n) = 2.9e-4)
    assert torch.equal(a, draw(1234, 7))                           # reproducible per (seed, stream id)
    assert not torch.equal(a, draw(1234, 8)) and not torch.equal(a, draw(1235, 7))
    assert abs(float((a * draw(1234, 8)).double().mean()) - p * p) <= 1.5e-3      # streams are independent draws, not shifts
    assert float(draw(1, 1, n=1001, p=0.0).sum()) == 0.0 and float(draw(1, 1, n=1001, p=1.0).sum()) == 1001.0
    # the counter convention of t2_philox_mask: element e is dropped there exactly where it is zoned here (same seed, stream, rate)
    scale = _nan(dev, n)
    _lib.call("t2_philox_mask", scale, n, p, 1234, 7, _stream())
    torch.cuda.synchronize()
    assert torch.equal(scale == 0, a == 1)


# ---------------------------------------------------------------------------------------------------------------------------
# model level: the engine's training step, eval forward and decode loop against zoneout_ref.model_fwd (float64), at the
# dimensions and with the criteria of tests/test_gpu_reduction_factor.py (outputs: mean-abs 1e-4, alignments 5e-5; losses: rtol 1e-5;
# every parameter gradient: 3e-4 of the tensor's largest element - tests/test_gpu_model.py::_grad_check)
# ---------------------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402

from oracle import tacotron2_ref as R  # noqa: E402
from tests import reduction_ref as RR  # noqa: E402

RATE = 0.1


def _zone_masks(B, S, A, D, seed, p=0.3):
    """Supplied 0/1 masks, drawn at 0.3 so that the few steps of a test hold plenty of both values."""
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(S, B, A if k.startswith("att") else D, generator=g) < p).float() for k in Z.ZONE_KEYS}


@functools.lru_cache(maxsize=None)
def _train_case(B, L, T, r, seed, hook=False, cell_dropout=True):
    """tests/test_gpu_reduction_factor.py::_model_case with zone masks: (dims, parameters, case, zone masks, float64 parameters
    with grad, reference outputs, names).  cell_dropout False: no att_drop / dec_drop masks on either side."""
    from tests.helpers import dekink_masks
    from tests.test_gpu_model import random_case
    from tests.test_gpu_reduction_factor import MID, _step_masks
    d = R.default_dims(**MID)
    P = RR.grouped_params(R.init_params(d, seed=5), d, r, seed=seed)
    ci, lens, mel, tl, gate, masks = random_case(d, B, L, T, seed, None)
    if r > 1 and all(int(x) % r == 0 for x in tl):
        tl[0] -= 1
        mel[0, tl[0]:] = 0.0; gate[0, tl[0] - 1:] = 0.0
    m = _step_masks(masks, T, r)
    if not cell_dropout:
        m = {k: v for k, v in m.items() if k not in ("att_drop", "dec_drop")}
    packed = torch.stack([mel[:, i] if i is not None else torch.zeros(B, d["num_mels"]) for i in RR.teacher_slots(T, r)], 1)
    m, _ = dekink_masks(P, d, ci, packed, m)
    S = RR.steps_of(T, r)
    zones = _zone_masks(B, S, d["att_rnn_dim"], d["rnn_hidden_dim"], seed + 7)
    Pc = {k: (v.double().clone().requires_grad_(True) if (v.is_floating_point() and not R.is_buffer(k)) else
              (v.double().clone() if v.is_floating_point() else v.clone())) for k, v in P.items()}
    names = [k for k, v in Pc.items() if v.requires_grad]
    m64 = {k: ([x.double() for x in v] if isinstance(v, list) else v.double()) for k, v in m.items()}
    o = Z.model_fwd(Pc, d, r, ci, lens, True, mel=mel.double(), mel_len=tl, training=True, masks=m64, new_stats={},
                    attention_hook=RR.forward_attention_hook if hook else None, zones=zones)
    dims = dict(d, reduction_factor=r, zoneout=RATE)
    if not cell_dropout:
        dims["cell_dropout"] = 0.0
    return dims, P, (ci, lens, mel, tl, gate, m), zones, Pc, o, names


def _engine_step(c, dev, dec_chain=None, guided=None, **fkw):
    from tests.test_gpu_model import build_engine, masks_to_device
    d, P, (ci, lens, mel, tl, gate, m), zones = c[:4]
    eng, ps = build_engine(d, P, dev)
    if dec_chain is not None:
        eng.dec_chain = dec_chain
    masks = masks_to_device(m, dev)
    masks.update({k: v.to(dev).contiguous() for k, v in zones.items()})
    outs, ctx = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=True, masks=masks, **fkw)
    ps.grad.zero_()
    loss3 = eng.loss_and_grads(outs, ctx, mel.to(dev), gate.to(dev), guided=guided)
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    return eng, ps, outs, loss3, ctx


def _ref_grads(c, total):
    Pc, names = c[4], c[6]
    gs = torch.autograd.grad(total, [Pc[k] for k in names], allow_unused=True, retain_graph=True)
    return {k: (torch.zeros_like(Pc[k]) if g is None else g) for k, g in zip(names, gs)}


@pytest.mark.parametrize("dec_chain", ["persistent", "steps"])
@pytest.mark.parametrize("B,r", [(3, 1), (3, 2), (33, 1), (33, 2)])
def test_training_step_against_float64(dev, B, r, dec_chain):
    from tests.test_gpu_reduction_factor import _check_outputs, _grad_report
    L, T = 21, 10
    c = _train_case(B, L, T, r, 400 + B + r)
    (ci, lens, mel, tl, gate, m), o = c[2], c[5]
    tot, bce, ml, pl = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())
    eng, ps, outs, loss3, ctx = _engine_step(c, dev, dec_chain=dec_chain)
    assert ctx["persist"] == (dec_chain == "persistent")            # the chain mode under test is the one that ran
    assert "dhz_dec" in eng._ws and "dhz_att" in eng._ws            # the carries come from the workspace allocator
    label = f"zoneout (B,L,T,r)=({B},{L},{T},{r}) {dec_chain}"
    _check_outputs(outs, o, label)
    ref3 = torch.stack([bce, ml, pl]).detach()
    assert torch.allclose(loss3.cpu(), ref3, rtol=1e-5, atol=1e-6), (loss3.cpu(), ref3)
    _grad_report(ps, _ref_grads(c, tot), label)


def _guided_term(al, lens, tl, r, sigma, alpha):
    """The guided-attention term on the reference's alignments (closed form of tests/reduction_ref.py, differentiable here)."""
    B = al.shape[0]
    steps = RR.steps_of(tl.to(torch.int64), r)
    g_tot = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        Nb, Tb = int(lens[b]), int(steps[b])
        ll = torch.arange(Nb, dtype=torch.float64)[None, :] / Nb
        ss = torch.arange(Tb, dtype=torch.float64)[:, None] / Tb
        g_tot = g_tot + ((1.0 - torch.exp(-((ll - ss) ** 2) / (2.0 * sigma * sigma))) * al[b, :Tb, :Nb]).sum() / (Nb * Tb)
    g_tot = alpha / B * g_tot
    assert abs(float(g_tot.detach()) - RR.guided_mask_sum(al.detach(), lens, tl, r, sigma, alpha)) < 1e-12
    return g_tot


def test_training_step_with_forward_and_guided_attention(dev):
    from tests.test_gpu_reduction_factor import _check_outputs, _grad_report
    B, L, T, r = 3, 21, 10, 2
    c = _train_case(B, L, T, r, 431, True)
    (ci, lens, mel, tl, gate, m), o = c[2], c[5]
    sigma, alpha = 0.4, 1.0
    g_tot = _guided_term(o[3], lens, tl, r, sigma, alpha)
    tot, bce, ml, pl = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())
    eng, ps, outs, loss3, _ = _engine_step(c, dev, guided=(sigma, alpha), forward_attention=True)
    _check_outputs(outs, o, "zoneout + forward + guided attention")
    assert torch.allclose(loss3.cpu(), torch.stack([bce, ml, pl]).detach(), rtol=1e-5, atol=1e-6)
    assert abs(float(eng.guided_loss.cpu()) - float(g_tot.detach())) < 1e-5 * max(1.0, float(g_tot.detach()))
    _grad_report(ps, _ref_grads(c, tot + g_tot), "zoneout + forward + guided attention")


def test_cell_dropout_zero_has_no_cell_masks(dev):
    """dims["cell_dropout"] = 0: make_masks generates no att_drop / dec_drop; the step matches the reference without them."""
    from tests.test_gpu_reduction_factor import _check_outputs, _grad_report
    c = _train_case(3, 21, 10, 1, 441, False, False)
    (ci, lens, mel, tl, gate, m), o = c[2], c[5]
    assert "att_drop" not in m and "dec_drop" not in m
    tot = R.tts_loss(o[0], o[1], o[2], mel.double(), gate.double())[0]
    eng, ps, outs, _, _ = _engine_step(c, dev)
    gen = eng.make_masks(3, 21, 10, True, 5, 0)
    assert "att_drop" not in gen and "dec_drop" not in gen and set(Z.ZONE_KEYS) <= set(gen) and "prenet_drop" in gen
    _check_outputs(outs, o, "zoneout, cell_dropout = 0")
    _grad_report(ps, _ref_grads(c, tot), "zoneout, cell_dropout = 0")


def test_generated_masks(dev):
    """Training: four independent 0/1 tensors [S][B][H] at the rate, per-seed (per-rank) streams, the dropout masks untouched by
    the option; eval: ONE block of the rate per cell, shared by zone_h and zone_c."""
    from tests.test_gpu_model import build_engine
    from tests.test_gpu_reduction_factor import MID
    d = R.default_dims(**MID)
    P = R.init_params(d, seed=5)
    eng, _ = build_engine(dict(d, zoneout=RATE), P, dev)
    B, L, T = 16, 21, 64
    m = {k: v.clone() if torch.is_tensor(v) else [x.clone() for x in v] for k, v in eng.make_masks(B, L, T, True, 11, 3).items()}
    for k in Z.ZONE_KEYS:
        z = m[k]
        assert z.shape == (T, B, 256) and bool(((z == 0) | (z == 1)).all())
        n = z.numel()
        assert abs(float(z.mean()) - RATE) <= 5 * math.sqrt(RATE * (1 - RATE) / n)
    assert not torch.equal(m["att_zone_h"], m["att_zone_c"]) and not torch.equal(m["dec_zone_h"], m["dec_zone_c"])
    other_rank = eng.make_masks(B, L, T, True, 11 + 7919, 3)
    assert not torch.equal(other_rank["att_zone_h"], m["att_zone_h"])
    plain, _ = build_engine(d, P, dev)
    pm = plain.make_masks(B, L, T, True, 11, 3)
    assert not (set(Z.ZONE_KEYS) & set(pm))
    for k in ("att_drop", "dec_drop"):
        assert torch.equal(pm[k], m[k])
    ev = eng.make_masks(B, L, T, False, 11, 3)
    assert ev["att_zone_h"].shape == (1, B, 256) and ev["att_zone_h"].data_ptr() == ev["att_zone_c"].data_ptr()
    assert bool((ev["att_zone_h"] == RATE).all()) and bool((ev["dec_zone_c"] == RATE).all())


def test_eval_forward_and_decode_use_the_expectation(dev):
    """Eval-mode teacher-forced forward (masks from make_masks: one block of the rate per cell, stride 0) and a 12-frame decode
    against the reference with every mask element = the rate."""
    from tests.test_gpu_model import build_engine, random_case
    from tests.test_gpu_reduction_factor import MID, _check_outputs, _check_decode, _decode_case
    B, L, T = 3, 21, 10
    d = R.default_dims(**dict(MID, dropout=0.0))
    P = R.init_params(d, seed=5)
    ci, lens, mel, tl, gate, _ = random_case(d, B, L, T, 451, None)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        o = Z.model_fwd(P64, d, 1, ci, lens, True, mel=mel.double(), mel_len=tl, training=False, rate=RATE)
    eng, ps = build_engine(dict(d, zoneout=RATE), P, dev)
    masks = eng.make_masks(B, L, T, False, 1, 0)
    outs, _ = eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=False, masks=masks, save_for_backward=False)
    torch.cuda.synchronize()
    eng.check_persistent_kernels()
    _check_outputs(outs, o, "zoneout eval forward")
    # decode: 12 frames (the cap).  The stop bias was chosen on the CPU restatement WITH the rule: at -0.44 nobody stops and every stop
    # logit of the run is at least 5e-3 from zero (asserted by _check_decode: 1e-3); the -0.4545 of the case without the rule
    # leaves one logit 2.5e-4 from zero
    cap = 12
    d2, P2, ci2, lens2, pm = _decode_case(3, 19, 1, cap, 303, -0.44)
    P2_64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P2.items()}
    with torch.no_grad():
        ref = Z.model_fwd(P2_64, d2, 1, ci2, lens2, False, max_len=cap, training=False, rate=RATE,
                          masks=dict(prenet_drop=[[pm[i, 0].double(), pm[i, 1].double()] for i in range(pm.shape[0])]))
    eng2, _ = build_engine(dict(d2, zoneout=RATE), P2, dev)
    out = eng2.infer(ci2.to(dev), lens2.to(dev), cap, prenet_masks=pm.to(dev).contiguous(), check_every=4)
    torch.cuda.synchronize()
    _check_decode(out, ref, 1, cap, need_both=False)
    assert out[0].shape[1] == cap
    plain, _ = build_engine(d2, P2, dev)
    out0 = plain.infer(ci2.to(dev), lens2.to(dev), cap, prenet_masks=pm.to(dev).contiguous(), check_every=4)
    n = min(out0[0].shape[1], out[0].shape[1])
    assert float((out0[0][:, :n] - out[0][:, :n]).abs().max()) > 1e-3       # (without the option it is another decode)


def _module_batch(dev, B=3, L=17, T=9, seed=3):
    g = torch.Generator().manual_seed(seed)
    ci = torch.randint(1, 39, (B, L), generator=g)
    lens = torch.tensor([L, L - 4, L - 2][:B])
    mel = torch.randn(B, T, 80, generator=g) - 2
    tl = torch.tensor([T, T - 2, T - 1][:B], dtype=torch.int32)
    return ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev)


def test_zoneout_zero_is_the_model_without_the_argument(dev):
    """Three models from one seed on one batch: A and A2 without the argument, Z with zoneout=0.0, cell_dropout=0.1.  Each runs a
    training forward + backward and a 12-step decode.  A2 is the control: whatever A and A2 have bit for bit in common (the engine's
    split-K and weight-gradient sums use atomics, so not everything: DESIGN.md section 9), A and Z must have bit for bit in common
    too - at the least the training alignments and the decode's mels, gates, alignments and lengths, which pass through both cells
    (measured reproducible; the training mels and both post-net outputs are not).  Everything else agrees to rounding, and no
    workspace of the option exists.  (The step kernels alone are compared bit for bit with the
    parent's by tools/lstm_step_digest.py, profiles/zoneout_bench.txt.)"""
    from tacotron2_amd.model.tacotron2 import Tacotron2
    from tests.test_gpu_reduction_factor import MID
    kw = dict(MID, encoder_kernel_size=5)
    ci, lens, mel, tl = _module_batch(dev)
    runs = []
    for extra in ({}, {}, dict(zoneout=0.0, cell_dropout=0.1)):
        m = Tacotron2(**kw, device=dev, seed=4, **extra)
        assert "zoneout" not in m.dims and "cell_dropout" not in m.dims
        m.train()
        o = m(ci, lens, True, mel_spectrogram=mel, mel_spectrogram_len=tl)
        (o[0].sum() + o[1].sum()).backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(m.store.grad).all())
        ws = {k: v.numel() for k, v in m._engine._ws.items()}
        m.eval()
        with torch.no_grad():
            dec = m._engine.infer(ci, lens, 12, training=False, seed=4)
        torch.cuda.synchronize()
        runs.append(dict(tf=[x.detach() for x in o], dec=list(dec), ws=ws))
    A, A2, Zm = runs
    names = [f"tf.{n}" for n in ("mels", "post", "gates", "align")] + [f"dec.{n}" for n in ("mels", "post", "gates", "align", "lengths")]
    same = {}
    for n, a, a2, z in zip(names, A["tf"] + A["dec"], A2["tf"] + A2["dec"], Zm["tf"] + Zm["dec"]):
        assert a.shape == z.shape, n
        same[n] = (torch.equal(a, a2), torch.equal(a, z))
        if same[n][0]:
            assert same[n][1], f"{n}: bit-identical between two models without the argument, not with zoneout = 0"
        assert float((a.double() - z.double()).abs().max()) < 1e-4, n
    print("[zoneout] zoneout = 0, (reproducible without the argument, identical with zoneout = 0): " + str(same))
    # the training alignments, and the decode up to the post-net (every sum of the decode loop runs in a fixed order)
    for n in ("tf.align", "dec.mels", "dec.gates", "dec.align", "dec.lengths"):
        assert same[n] == (True, True), (n, same[n])
    assert A["ws"] == Zm["ws"] and not any("zone" in k or "dhz" in k for k in A["ws"])      # no workspace of the option exists
    outs = [A["tf"]]
    on = Tacotron2(**kw, device=dev, seed=4, zoneout=RATE)
    on.train()
    o = on(ci, lens, True, mel_spectrogram=mel, mel_spectrogram_len=tl)
    assert on.dims["zoneout"] == RATE and float((o[0].detach() - outs[0][0]).abs().max()) > 1e-3
    with pytest.raises(ValueError, match="zoneout"):
        Tacotron2(**kw, device=dev, zoneout=1.5)
    with pytest.raises(ValueError, match="cell_dropout"):
        Tacotron2(**kw, device=dev, cell_dropout=1.0)


def test_checkpoint_round_trip_of_the_hyper_parameter(dev, tmp_path, capsys):
    from tacotron2_amd.model.tts_model import TTSModel
    from tests.test_gpu_reduction_factor import MID
    kw = dict(MID, encoder_kernel_size=5)
    tm = TTSModel(lr=1e-3, weight_decay=0.0, device=dev, zoneout=RATE, cell_dropout=0.0, **kw)
    ck = tm.checkpoint()
    assert ck["hyper_parameters"]["zoneout"] == RATE and ck["hyper_parameters"]["cell_dropout"] == 0.0
    path = str(tmp_path / "z.ckpt")
    torch.save(ck, path)
    back = TTSModel.load_from_checkpoint(path, device=dev)
    assert back.tacotron2.zoneout == RATE and back.tacotron2.cell_dropout == 0.0 and back.tacotron2._engine.zoneout == RATE
    assert capsys.readouterr().out.count("warning") == 0
    # another configured value loads (no parameter depends on it), wins, and says so once
    other = TTSModel.load_from_checkpoint(path, device=dev, zoneout=0.0)
    assert other.tacotron2.zoneout == 0.0 and other.tacotron2.cell_dropout == 0.0
    said = capsys.readouterr().out
    assert said.count("warning") == 1 and "zoneout" in said
    for a, b in zip(other.tacotron2.state_dict().values(), tm.tacotron2.state_dict().values()):
        assert torch.equal(a, b)
    # a file from before the option loads as zoneout 0 / cell_dropout 0.1, and the configuration can switch it on
    old = dict(ck, hyper_parameters={k: v for k, v in ck["hyper_parameters"].items() if k not in ("zoneout", "cell_dropout")})
    torch.save(old, path)
    assert TTSModel.load_from_checkpoint(path, device=dev).tacotron2.zoneout == 0.0
    assert TTSModel.load_from_checkpoint(path, device=dev, zoneout=RATE).tacotron2.zoneout == RATE
