"""The kernels around the conv stacks, the encoder BiLSTM walk and the conditioning, called directly through the C ABI
(tacotron2_amd._lib.call / make, include/tacotron2_amd.h) and compared, output by output, with the float64 references of
tests/conv_path_ref.py: t2_bn_fwd / t2_bn_bwd over their option matrix and as the two phases of synchronised statistics,
t2_embedding_fwd / _bwd, t2_condition_fwd / _bwd, t2_tanh_bias / t2_tanh_bwd, t2_colsum (both kernels behind the dispatch),
t2_pack_conv_weight(flip = 1) + t2_gemm (dgrad) and the split-K t2_gemm + t2_unpack_conv_wgrad (wgrad), t2_relu_mask_bwd /
t2_leaky_relu / t2_axpy / t2_swap01, t2_zero_regions, and t2_lstm_seq_fwd / t2_lstm_seq_fwd_persist_pz / t2_lstm_seq_bwd with n = 2.

Operands are laid out as the header documents: padded (B, L + 4, C) activations with data rows [2, L + 2), raw conv outputs and
their gradients in shifted rows b * Lp + l, time-major stashes with their zero start slots.  Every buffer a call is documented to
write is filled with NaN first, junk rows of an input that no kernel may read hold NaN too, only what the header tells the caller to
zero is zeroed, and every += output starts from a non-zero random value (expected: start + reference).  All tensors are plain torch
allocations, so the module runs unchanged under T2_GUARD_BYTES.

Metric: conv_path_ref.rel - max over samples of max|got_b - ref_b| / max|ref_b|, over the whole tensor for outputs without a batch
axis.  Tolerances: conv_path_ref.TOL, one constant per output = 16 x the reference's own float32-vs-float64 error over the case
list (anchored by tests/test_conv_path_ref_host.py); BatchNorm statistics keep the bounds of the two older BatchNorm tests
(conv_path_ref.STAT_BOUNDS).  With act = 1 the elements within 1e-4 of the ReLU kink are left out of the backward comparison (their
dy is zero), at most 1e-3 of the elements.  Pure selections and copies are held bit-equal, pad rows exactly zero, the pointwise
kernels to one float32 rounding of the float64 result (2^-24 |ref|; t2_leaky_relu's negative branch rounds twice).

Every test prints its worst figure per output as "[conv path] <case>: <output> <error> /<constant>" (tabulated in DESIGN.md 5).
    output               float32 restatement   constant (x 16)
    bn.y                 7.7e-6                1.23e-4
    bn.dx                5.0e-6                8.00e-5
    bn.dgamma            4.4e-6                7.04e-5
    bn.dbeta             2.0e-6                3.20e-5
    embedding.dtable     1.3e-7                2.08e-6
    condition.memory     4.7e-8                7.52e-7
    condition.denc       8.9e-8                1.42e-6
    condition.dspk_table 1.7e-7                2.72e-6
    condition.ddesc      1.7e-7                2.72e-6
    tanh.y               5.8e-8                9.28e-7
    tanh.bwd             6.1e-8                9.76e-7
    colsum               1.8e-6                2.88e-5
    conv.conv_dx         2.9e-7                4.64e-6
    conv.conv_dw         3.5e-7                5.60e-6
    bilstm.enc           1.8e-7                2.88e-6
    bilstm.c_final       2.3e-7                3.68e-6
    bilstm.dpre          3.0e-7                4.80e-6
    mean 2e-6 x max(1, |level| + 1) absolute | invstd 2e-5 (statistics kernel) / 3e-6 (GEMM-epilogue tiles) relative | running 1e-5"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_path_ref as C  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def _ptr(t, elem_off=0):
    return t.data_ptr() + 4 * elem_off


def _check(case, figures):
    """figures: [(output, error, bound)]; prints them all, then asserts them all."""
    print(f"[conv path] {case}: " + ", ".join(f"{k} {e:.2e} /{b:.1e}" for k, e, b in figures))
    bad = [(k, e, b) for k, e, b in figures if not e <= b]
    assert not bad, f"{case}: over their constant [(output, error, constant)] {bad}"


def _padded(dev, x, pad, fill=float("nan")):
    """(B, L, C) -> (B, L + 4, C) device buffer with the data at rows [pad, pad + L) and `fill` elsewhere."""
    B, L, Cn = x.shape
    out = torch.full((B, L + 4, Cn), fill, device=dev)
    out[:, pad:pad + L] = x.to(dev)
    return out


# -----------------------------------------------------------------------------------------------------------------
# BatchNorm
# -----------------------------------------------------------------------------------------------------------------
def _stat_figures(case_level, mean, invstd, rm, rv, ref, tiles=False):
    ib = C.STAT_BOUNDS["invstd_tiles" if tiles else "invstd_kernel"]
    return [("mean", float((mean.double().cpu() - ref["mean"]).abs().max()), C.STAT_BOUNDS["mean"] * max(1.0, abs(case_level) + 1)),
            ("invstd", float(((invstd.double().cpu() - ref["invstd"]).abs() / ref["invstd"]).max()), ib),
            ("running_mean", float((rm.double().cpu() - ref["running_mean"]).abs().max()), C.STAT_BOUNDS["running"]),
            ("running_var", float((rv.double().cpu() - ref["running_var"]).abs().max()), C.STAT_BOUNDS["running"])]


@pytest.mark.parametrize("name", list(C.BN_CASES))
def test_bn_option_matrix(dev, name):
    """t2_bn_fwd, then t2_bn_bwd on the forward kernel's own mean / invstd, one case of conv_path_ref.BN_CASES."""
    from tacotron2_amd._lib import call, make
    case = C.BN_CASES[name]
    inp, ref, bref = C.bn_reference(name)
    B, L, Cn, act, training = case["B"], case["L"], case["C"], case["act"], case["training"]
    Lp = L + 4
    f = lambda t: None if t is None else t.to(dev).contiguous()
    x = _padded(dev, inp["x"], 0)                                  # shifted rows b * Lp + l; the junk rows hold NaN
    gamma, beta, drop = f(inp["gamma"]), f(inp["beta"]), f(inp["drop"])
    rm, rv = f(inp["running_mean"]), f(inp["running_var"])
    shift = f(inp["shift"])
    lens = None if inp["lens"] is None else inp["lens"].to(torch.int32).to(dev)
    res = None if inp["res"] is None else _padded(dev, inp["res"], 2)
    Lp_y, pad_y = (L, 0) if case["res"] else (Lp, 2)               # with a residual: y at (L, 0), the residual at (L + 4, 2)
    y = _nan(dev, B, Lp_y, Cn)
    mean, invstd = _nan(dev, Cn), _nan(dev, Cn)
    mk_sums = lambda: torch.zeros(2 * Cn + 2, dtype=F64, device=dev) if case["prezeroed"] else _nan(dev, 2 * Cn + 2, dtype=F64)
    sums = mk_sums()
    bn = make("T2Bn", B=B, L=L, C=Cn, x=x, Lp_x=Lp, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, training=int(training),
              momentum=0.1, eps=1e-5, sums=sums, mean=mean, invstd=invstd, act=act, drop=drop, res=res, Lp_res=Lp, pad_res=2,
              len=lens, fill=case["fill"], y=y, Lp_y=Lp_y, pad_y=pad_y, shift=shift, sums_prezeroed=int(case["prezeroed"]))
    call("t2_bn_fwd", bn, _st())
    torch.cuda.synchronize()
    figs = _stat_figures(case["level"], mean, invstd, rm, rv, ref)
    if training:
        assert float(sums[2 * Cn]) == B * L
    else:                                                          # eval: the running statistics are read, not written
        assert torch.equal(rm.cpu(), inp["running_mean"]) and torch.equal(rv.cpu(), inp["running_var"])
        assert torch.equal(mean.cpu(), inp["running_mean"])
    yc = y.cpu()
    figs.append(("y", C.rel(yc[:, pad_y:pad_y + L], ref["y"]), C.TOL["bn.y"]))
    assert C.pad_rows_are_zero(yc, L, pad_y)
    # backward
    if act == 1:
        assert inp["kink_share"] <= C.KINK_SHARE
    dy = _padded(dev, inp["dy"], 2) if case["dy_pad"] else f(inp["dy"])
    Lp_dy, pad_dy = (Lp, 2) if case["dy_pad"] else (L, 0)
    dx = _nan(dev, B, Lp, Cn)
    dgamma, dbeta = f(inp["dgamma0"]), f(inp["dbeta0"])
    sums_b = mk_sums()
    bnb = make("T2Bn", B=B, L=L, C=Cn, x=x, Lp_x=Lp, gamma=gamma, beta=beta, training=int(training), momentum=0.1, eps=1e-5,
               sums=sums_b, mean=mean, invstd=invstd, act=act, drop=drop, dy=dy, Lp_dy=Lp_dy, pad_dy=pad_dy, dx=dx, Lp_dx=Lp,
               pad_dx=2, dgamma=dgamma, dbeta=dbeta, sums_prezeroed=int(case["prezeroed"]))
    call("t2_bn_bwd", bnb, _st())
    torch.cuda.synchronize()
    assert float(sums_b[2 * Cn]) == B * L
    dxc = dx.cpu()
    figs += [("dx", C.rel(dxc[:, 2:2 + L], bref["dx"]), C.TOL["bn.dx"]),
             ("dgamma", C.rel(dgamma.cpu(), inp["dgamma0"].double() + bref["dgamma"], False), C.TOL["bn.dgamma"]),
             ("dbeta", C.rel(dbeta.cpu(), inp["dbeta0"].double() + bref["dbeta"], False), C.TOL["bn.dbeta"])]
    assert C.pad_rows_are_zero(dxc, L, 2)
    _check(name, figs)


@pytest.mark.parametrize("name", list(C.SYNC_BN_CASES))
def test_sync_bn_two_shards_on_one_gpu(dev, name):
    """Phases 1 / 2 of the synchronised statistics on shards of 2 and 3 utterances, the all-reduce played by one addition of the
    two `sums` vectors (count word included), forward and backward (grad_share = 0.5): both shards see the float64 statistics of
    the whole batch, their y / dx are the whole batch's rows, their dgamma / dbeta shares add up to the whole batch's gradients.
    tiles: each shard's phase-1 statistics come from its own convolution GEMM's epilogue (T2Gemm.stat_out), as under the engine.
    (This case found the epilogue's float32 tile sums: 1/std off by 3.35e-6 against the 3e-6 bound with three tiles to average over;
    with the sums accumulated in double, csrc/t2_gemm.hip, 8.15e-7.)"""
    from tacotron2_amd._lib import call, make
    case = C.SYNC_BN_CASES[name]
    inp = C.make_inputs("sync_bn", case)
    B, L, Cn, act, tiles = case["B"], case["L"], case["C"], case["act"], case["tiles"]
    Lp = L + 4
    f = lambda t: None if t is None else t.to(dev).contiguous()
    cuts = ((0, 2), (2, 5))
    gamma, beta = f(inp["gamma"]), f(inp["beta"])
    xs, tstats = [], []
    if tiles:
        Ci = case["Ci"]
        w, bias = f(inp["conv_w"]), f(inp["conv_b"])
        for b0, b1 in cuts:
            xin = _padded(dev, inp["conv_x"][b0:b1], 2, fill=0.0)
            M = (b1 - b0) * Lp - 4
            raw = _nan(dev, (b1 - b0) * Lp, Cn)
            ts = _nan(dev, (M + 127) // 128, 3, Cn)
            call("t2_gemm", make("T2Gemm", A=xin, B=w, C=raw, M=M, N=Cn, K=5 * Ci, lda=Ci, ldb=5 * Ci, ldc=Cn, a_kmajor=1, b_kmajor=1,
                                 alpha=1.0, bias=bias, splitk=1, batch=1, stat_out=ts, stat_Lp=Lp, stat_L=L), _st())
            xs.append(raw.view(b1 - b0, Lp, Cn)); tstats.append((ts, M))
        torch.cuda.synchronize()
        x_whole = torch.cat([x[:, :L].cpu() for x in xs], 0)       # the BatchNorm input IS the fp32 convolution output
        level = float(x_whole.mean())
        shift_c = (x_whole.double().mean((0, 1)) + 0.3 * inp["beta"].double()).float()      # near the level, not the data mean
    else:
        x_whole, level, shift_c = inp["x"], case["level"], inp["shift"]
        xs = [_padded(dev, x_whole[b0:b1], 0) for b0, b1 in cuts]
        tstats = [(None, 0)] * 2
    rm0, rv0 = shift_c, inp["running_var"]
    assert float((shift_c.double() - x_whole.double().mean((0, 1))).abs().min()) > 0
    dy = inp["dy"]
    if act == 1:
        keep, share = C.kink_mask(C.bn(x_whole, inp["gamma"], inp["beta"], rm0, rv0, True, act, inp["drop"])["pre"])
        assert share <= C.KINK_SHARE
        dy = dy * keep.float()
    ref = C.bn(x_whole, inp["gamma"], inp["beta"], rm0, rv0, True, act, inp["drop"])
    bref = C.bn_bwd(x_whole, inp["gamma"], inp["beta"], rm0, rv0, dy, True, act, inp["drop"])

    sh = []
    for (b0, b1), x, (ts, M) in zip(cuts, xs, tstats):
        Bs = b1 - b0
        s = dict(Bs=Bs, x=x, y=_nan(dev, Bs, Lp, Cn), mean=_nan(dev, Cn), invstd=_nan(dev, Cn), rm=f(rm0).clone(), rv=f(rv0).clone(),
                 shift=f(shift_c).clone(), sums=_nan(dev, 2 * Cn + 2, dtype=F64), drop=None if inp["drop"] is None else f(inp["drop"][b0:b1]))
        s["bn"] = make("T2Bn", B=Bs, L=L, C=Cn, x=x, Lp_x=Lp, gamma=gamma, beta=beta, running_mean=s["rm"], running_var=s["rv"],
                       training=1, momentum=0.1, eps=1e-5, sums=s["sums"], mean=s["mean"], invstd=s["invstd"], act=act, drop=s["drop"],
                       y=s["y"], Lp_y=Lp, pad_y=2, phase=1, shift=s["shift"], sums_prezeroed=0, tile_stats=ts, tile_M=M)
        call("t2_bn_fwd", s["bn"], _st())
        sh.append(s)
    total = sh[0]["sums"][:2 * Cn + 1] + sh[1]["sums"][:2 * Cn + 1]
    assert float(total[2 * Cn]) == B * L
    figs = []
    for i, s in enumerate(sh):
        s["sums"][:2 * Cn + 1] = total
        s["bn"].phase = 2
        call("t2_bn_fwd", s["bn"], _st())
    torch.cuda.synchronize()
    for i, s in enumerate(sh):
        figs += [(f"{k}[{i}]", e, b) for k, e, b in _stat_figures(level, s["mean"], s["invstd"], s["rm"], s["rv"], ref, tiles)]
        assert C.pad_rows_are_zero(s["y"].cpu(), L, 2)
    figs.append(("y", C.rel(torch.cat([s["y"][:, 2:2 + L].cpu() for s in sh], 0), ref["y"]), C.TOL["bn.y"]))
    # backward
    for (b0, b1), s in zip(cuts, sh):
        s["dx"] = _nan(dev, s["Bs"], Lp, Cn)
        s["dgamma"], s["dbeta"] = f(inp["dgamma0"]).clone(), f(inp["dbeta0"]).clone()
        s["sums_b"] = _nan(dev, 2 * Cn + 2, dtype=F64)
        s["dy"] = f(dy[b0:b1])
        s["bnb"] = make("T2Bn", B=s["Bs"], L=L, C=Cn, x=s["x"], Lp_x=Lp, gamma=gamma, beta=beta, training=1, momentum=0.1, eps=1e-5,
                        sums=s["sums_b"], mean=s["mean"], invstd=s["invstd"], act=act, drop=s["drop"], dy=s["dy"], Lp_dy=L, pad_dy=0,
                        dx=s["dx"], Lp_dx=Lp, pad_dx=2, dgamma=s["dgamma"], dbeta=s["dbeta"], phase=1, sums_prezeroed=0)
        call("t2_bn_bwd", s["bnb"], _st())
    total = sh[0]["sums_b"] + sh[1]["sums_b"]
    assert float(total[2 * Cn]) == B * L
    for s in sh:
        s["sums_b"].copy_(total)
        s["bnb"].phase = 2; s["bnb"].grad_share = 0.5
        call("t2_bn_bwd", s["bnb"], _st())
    torch.cuda.synchronize()
    for s in sh:
        assert C.pad_rows_are_zero(s["dx"].cpu(), L, 2)
    figs.append(("dx", C.rel(torch.cat([s["dx"][:, 2:2 + L].cpu() for s in sh], 0), bref["dx"]), C.TOL["bn.dx"]))
    for k in ("dgamma", "dbeta"):
        got = sh[0][k].double().cpu() + sh[1][k].double().cpu()
        figs.append((k, C.rel(got, 2 * inp[k + "0"].double() + bref[k], False), C.TOL["bn." + k]))
    _check(name, figs)


# -----------------------------------------------------------------------------------------------------------------
# embedding, conditioning, tanh
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.EMBEDDING_CASES))
def test_embedding_fwd_bwd(dev, name):
    from tacotron2_amd._lib import call
    case = C.EMBEDDING_CASES[name]
    inp = C.make_inputs("embedding", case)
    B, L, E, V = case["B"], case["L"], case["E"], case["V"]
    idx, table = inp["idx"].to(dev), inp["table"].to(dev)
    out = _nan(dev, B, L + 4, E)
    call("t2_embedding_fwd", idx, table, out, B, L, E, 2, _st())
    torch.cuda.synchronize()
    oc = out.cpu()
    assert torch.equal(oc[:, 2:2 + L], inp["table"][inp["idx"]]) and C.pad_rows_are_zero(oc, L, 2)
    want = inp["dtable0"].double() + C.embedding_bwd(inp["idx"], inp["dout"], V)
    figs = []
    for pad in (0, 2):               # (Lp = L + 4, pad = 0): shifted rows, what the engine passes; pad = 2: the padded layout
        dout = _padded(dev, inp["dout"], pad)
        dtable = inp["dtable0"].to(dev).clone()
        call("t2_embedding_bwd", idx, dout, dtable, B, L, E, L + 4, pad, _st())
        torch.cuda.synchronize()
        figs.append((f"dtable(pad={pad})", C.rel(dtable.cpu(), want, False), C.TOL["embedding.dtable"]))
        assert torch.equal(dtable[0].cpu(), inp["dtable0"][0])                 # padding_idx: bit-unchanged
    _check(name, figs)


@pytest.mark.parametrize("name", list(C.CONDITION_CASES))
def test_condition_fwd_bwd(dev, name):
    """t2_condition_fwd, then t2_condition_bwd on the memory the forward kernel wrote."""
    from tacotron2_amd._lib import call
    case = C.CONDITION_CASES[name]
    inp = C.make_inputs("condition", case)
    B, L, E, Ef = case["B"], case["L"], case["E"], case["Ef"]
    ref = C.condition(inp["enc"], inp["spk_table"], inp["spk"], inp["desc"], inp["dmem"])
    f = lambda t: None if t is None else t.to(dev).contiguous()
    enc, tab, desc, dmem = f(inp["enc"]), f(inp["spk_table"]), f(inp["desc"]), f(inp["dmem"])
    spk = f(inp["spk"]) if case["spk"] else None
    memory = _nan(dev, B, L, Ef)
    call("t2_condition_fwd", enc, tab, spk, desc, memory, B, L, E, Ef, _st())
    torch.cuda.synchronize()
    mc = memory.cpu()
    figs = [("memory", C.rel(mc, ref["memory"]), C.TOL["condition.memory"])]
    if not case["spk"]:
        assert torch.equal(mc[..., :E], inp["enc"])
    if Ef > E:
        assert torch.equal(mc[..., E:], inp["desc"][:, None, :].expand(B, L, Ef - E))
    denc = _nan(dev, B, L, E)
    dspk = f(inp["dspk_table0"]).clone() if case["spk"] else None
    ddesc = torch.zeros(B, Ef - E, device=dev) if (case["ddesc"] and Ef > E) else None
    call("t2_condition_bwd", dmem, memory, spk, denc, dspk, ddesc, B, L, E, Ef, _st())
    torch.cuda.synchronize()
    figs.append(("denc", C.rel(denc.cpu(), ref["denc"]), C.TOL["condition.denc"]))
    if not case["spk"]:
        assert torch.equal(denc.cpu(), inp["dmem"][..., :E])
    else:
        figs.append(("dspk_table", C.rel(dspk.cpu(), inp["dspk_table0"].double() + ref["dspk_table"], False), C.TOL["condition.dspk_table"]))
        untouched = [r for r in range(case["V"]) if r not in inp["spk"].tolist()]
        assert torch.equal(dspk.cpu()[untouched], inp["dspk_table0"][untouched])
    if ddesc is not None:
        figs.append(("ddesc", C.rel(ddesc.cpu(), ref["ddesc"]), C.TOL["condition.ddesc"]))
    _check(name, figs)


@pytest.mark.parametrize("name", list(C.TANH_CASES))
def test_tanh_bias_and_tanh_bwd(dev, name):
    from tacotron2_amd._lib import call
    case = C.TANH_CASES[name]
    inp = C.make_inputs("tanh", case)
    rows, Cn = case["rows"], case["C"]
    figs = []
    for with_bias in (True, False):
        x = inp["x"].to(dev).clone()
        call("t2_tanh_bias", x, inp["bias"].to(dev) if with_bias else None, rows, Cn, _st())
        torch.cuda.synchronize()
        want = torch.tanh(inp["x"].double() + (inp["bias"].double() if with_bias else 0.0))
        figs.append((f"y(bias={int(with_bias)})", C.rel(x.cpu(), want, False), C.TOL["tanh.y"]))
    out = _nan(dev, rows, Cn)
    call("t2_tanh_bwd", inp["g"].to(dev), x, out, rows * Cn, _st())
    torch.cuda.synchronize()
    yk = x.cpu().double()                                           # the backward of the y the forward kernel wrote
    figs.append(("bwd", C.rel(out.cpu(), inp["g"].double() * (1 - yk * yk), False), C.TOL["tanh.bwd"]))
    _check(name, figs)


# -----------------------------------------------------------------------------------------------------------------
# column sums, conv weight layouts
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.COLSUM_CASES))
def test_colsum_both_kernels(dev, name):
    """out[c] += sum_r x[r][c] onto a non-zero out; the input sits on a -5.5 level, so a lost row is ~1/R of the result.  The
    columns between C and ld hold NaN."""
    from tacotron2_amd._lib import call
    case = C.COLSUM_CASES[name]
    inp = C.make_inputs("colsum", case)
    R_, Cn, ld, off = case["R"], case["C"], case["ld"], case["off"]
    buf = _nan(dev, off + R_ * ld)
    buf[off:].view(R_, ld)[:, :Cn] = inp["x"].to(dev)
    assert buf.data_ptr() % 16 == 0
    out = inp["out0"].to(dev).clone()
    call("t2_colsum", _ptr(buf, off), ld, R_, Cn, out, _st())
    torch.cuda.synchronize()
    _check(name, [("colsum", C.rel(out.cpu(), inp["out0"].double() + C.colsum(inp["x"]), False), C.TOL["colsum"])])


@pytest.mark.parametrize("name", list(C.CONV_CASES))
def test_conv_weight_layouts_as_the_backward_uses_them(dev, name):
    """t2_pack_conv_weight(flip = 1) + t2_gemm over the padded gradient rows = the convolution's input gradient; the split-K
    weight-gradient GEMM + t2_unpack_conv_wgrad = the weight gradient, accumulated onto a non-zero g."""
    from tacotron2_amd._lib import call, make
    case = C.CONV_CASES[name]
    inp = C.make_inputs("conv", case)
    B, L, Ci, Co, K = (case[k] for k in ("B", "L", "Ci", "Co", "K"))
    Lp, R_ = L + 4, B * (L + 4) - 4
    ref = C.conv_grads(inp["x"], inp["w"], inp["dy"])
    draw = _padded(dev, inp["dy"], 2, fill=0.0)                    # what t2_bn_bwd leaves: data rows [2, L + 2), zero rows elsewhere
    x_pad = _padded(dev, inp["x"], 2, fill=0.0)
    w = inp["w"].to(dev)
    wf = _nan(dev, Ci, K * Co)
    call("t2_pack_conv_weight", w, wf, Co, Ci, K, 1, _st())
    dx = _nan(dev, B * Lp, Ci)
    call("t2_gemm", make("T2Gemm", A=draw, B=wf, C=dx, M=R_, N=Ci, K=K * Co, lda=Co, ldb=K * Co, ldc=Ci, a_kmajor=1, b_kmajor=1,
                         alpha=1.0, splitk=1, batch=1), _st())
    dwp = torch.zeros(Co, K * Ci, device=dev)
    call("t2_gemm", make("T2Gemm", A=_ptr(draw, 2 * Co), B=x_pad, C=dwp, M=Co, N=K * Ci, K=R_, lda=Co, ldb=Ci, ldc=K * Ci, a_kmajor=0,
                         b_kmajor=0, alpha=1.0, accumulate=2, splitk=2, batch=1), _st())
    g = inp["g0"].to(dev).clone()
    call("t2_unpack_conv_wgrad", dwp, g, Co, Ci, K, _st())
    torch.cuda.synchronize()
    wfc = wf.cpu().view(Ci, K, Co)
    assert torch.equal(wfc, inp["w"].flip(2).permute(1, 2, 0))      # wp[ci][(K-1-k)*Co + co] = w[co][ci][k]
    _check(name, [("conv_dx", C.rel(dx.view(B, Lp, Ci)[:, :L].cpu(), ref["conv_dx"]), C.TOL["conv.conv_dx"]),
                  ("conv_dw", C.rel(g.cpu(), inp["g0"].double() + ref["conv_dw"], False), C.TOL["conv.conv_dw"])])


# -----------------------------------------------------------------------------------------------------------------
# pointwise glue, t2_swap01, t2_zero_regions
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.POINTWISE_SIZES)
def test_pointwise_glue(dev, n):
    """t2_relu_mask_bwd (mask / NULL), t2_leaky_relu, t2_axpy: one float32 rounding of the float64 result (2^-24 |ref|; the negative
    branch of t2_leaky_relu rounds scale * x and then slope * that: two); selections bit-equal, exact zeros where y <= 0."""
    from tacotron2_amd._lib import call
    g_ = torch.Generator().manual_seed(n)
    gr, y, x = (torch.randn(n, generator=g_) for _ in range(3))
    y[::5] = 0.0
    mask = (torch.rand(n, generator=g_) >= 0.5).float() * 2
    grd, yd, xd = gr.to(dev), y.to(dev), x.to(dev)
    figs = []
    for m in (mask, None):
        out = _nan(dev, n)
        call("t2_relu_mask_bwd", grd, yd, None if m is None else m.to(dev), out, n, _st())
        torch.cuda.synchronize()
        oc = out.cpu()
        assert bool((oc[y <= 0] == 0).all())
        if m is None:
            assert torch.equal(oc[y > 0], gr[y > 0])
        want = torch.where(y > 0, gr.double() * (1.0 if m is None else m.double()), torch.zeros(n, dtype=F64))
        figs.append((f"relu_mask_bwd(mask={int(m is not None)})", C.one_rounding(oc, want), 1.0))
    scale, slope, alpha = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.7, 0.1, -0.3))
    out = _nan(dev, n)
    call("t2_leaky_relu", xd, out, n, scale, slope, _st())
    torch.cuda.synchronize()
    v = scale * x.double()
    pos = x > 0
    oc = out.cpu()
    figs.append(("leaky_relu(+)", C.one_rounding(oc[pos], v[pos]), 1.0))
    figs.append(("leaky_relu(-)", C.one_rounding(oc[~pos], slope * v[~pos]), 2.0 + 2.0 ** -23))
    acc = y.to(dev).clone()
    call("t2_axpy", xd, acc, n, alpha, _st())
    torch.cuda.synchronize()
    figs.append(("axpy", C.one_rounding(acc.cpu(), alpha * x.double() + y.double()), 1.0))
    _check(f"pointwise n={n}", figs)


@pytest.mark.parametrize("shape", C.SWAP01_SHAPES)
def test_swap01(dev, shape):
    from tacotron2_amd._lib import call
    D0, D1, Cn = shape
    g_ = torch.Generator().manual_seed(D0 * 7 + D1)
    x, start = torch.randn(D0, D1, Cn, generator=g_), torch.randn(D1, D0, Cn, generator=g_)
    out = _nan(dev, D1, D0, Cn)
    call("t2_swap01", x.to(dev), out, D0, D1, Cn, 0, _st())
    acc = start.to(dev).clone()
    call("t2_swap01", x.to(dev), acc, D0, D1, Cn, 1, _st())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), x.transpose(0, 1).contiguous())
    _check(f"swap01 {shape}", [("accumulate", C.one_rounding(acc.cpu(), start.double() + x.transpose(0, 1).double()), 1.0)])


def test_zero_regions_clears_what_it_is_given_and_nothing_else(dev):
    """One launch with 64 regions of mixed kinds inside one sentinel-filled allocation: 16-byte-aligned runs, runs whose base is only
    4-byte aligned, byte counts that are no multiple of 16, strided rows (stride > row), one-row regions, and one region above 8 MB
    beside tiny ones.  Every word inside a region is 0, every word outside - the gaps between strided rows included - keeps the
    sentinel.  n = 0 launches nothing; a misaligned pointer, a stride below the row and a ragged byte count are refused."""
    from tacotron2_amd import _lib
    SENT = 0x5A5A5A5A
    big = 2 * 1024 * 1024 + 4096 + 4                   # words: 8.02 MB, a multiple of 16 bytes
    kinds = [("run16", 64), ("run4", 33), ("tail", 5), ("rows", (3, 7, 5)), ("one_row", 12), ("rows", (8, 12, 4)), ("run16", 4),
             ("run4", 1), ("rows", (1, 2, 9))]
    regions, w = [(0, big, 1, big)], big + 8            # (first word, row words, rows, stride words)
    for i in range(63):
        kind, arg = kinds[i % len(kinds)]
        w = (w + 3) // 4 * 4 + 4                         # a gap of at least one 16-byte line, then a 16-byte boundary
        if kind == "run16":
            regions.append((w, arg + 4 * (i % 3), 1, arg + 4 * (i % 3)))
        elif kind == "run4":
            regions.append((w + 1 + i % 3, arg, 1, arg))
        elif kind == "tail":
            regions.append((w, arg + 4 * (i % 2), 1, 0))
        elif kind == "one_row":
            regions.append((w + i % 2, arg, 1, 3))       # nrows = 1: one contiguous run, the stride is not read
        else:
            regions.append((w + (i % 2 if arg[0] % 4 else 0), arg[0], arg[2], arg[1]))
        r = regions[-1]
        w = r[0] + (r[2] - 1) * r[3] + r[1] if r[2] > 1 else r[0] + r[1]
    assert len(regions) == 64
    total = w + 16
    buf = torch.full((total,), SENT, dtype=torch.int32, device=dev)
    want = torch.full((total,), SENT, dtype=torch.int32)
    base = buf.data_ptr()
    for w0, rw, nr, sw in regions:
        for r in range(nr):
            want[w0 + r * sw: w0 + r * sw + rw] = 0
    assert int((want == 0).sum()) == sum(rw * nr for _, rw, nr, _ in regions)          # the regions do not overlap
    z = _lib.make("T2ZeroRegions", p=[base + 4 * r[0] for r in regions], row_bytes=[4 * r[1] for r in regions],
                  nrows=[r[2] for r in regions], stride_bytes=[4 * r[3] for r in regions], n=0)
    _lib.call("t2_zero_regions", z, _st())                                            # n = 0: OK, nothing launched
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    z.n = 64
    _lib.call("t2_zero_regions", z, _st())
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got, want), f"first differing word {int((got != want).nonzero()[0])}"
    for field, i, value in (("p", 0, base + 2), ("stride_bytes", 4, 8), ("row_bytes", 1, 6)):     # region 4: rows of 12 bytes
        bad = _lib.make("T2ZeroRegions", p=[base + 4 * r[0] for r in regions], row_bytes=[4 * r[1] for r in regions],
                        nrows=[r[2] for r in regions], stride_bytes=[4 * r[3] for r in regions], n=8)
        assert regions[4][2] > 1 and regions[4][1] * 4 > 8
        getattr(bad, field)[i] = value
        with pytest.raises(_lib.T2Error):
            _lib.call("t2_zero_regions", bad, _st())
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), want)


# -----------------------------------------------------------------------------------------------------------------
# encoder BiLSTM as a sequence
# -----------------------------------------------------------------------------------------------------------------
def _bilstm_fwd(dev, case, inp, d, persistent):
    """Both directions over all L steps, operands as tacotron2_amd.engine lays them out; returns the stashes (device)."""
    from tacotron2_amd import _lib
    B, L, H = case["B"], case["L"], case["H"]
    S, Lp, E, Bp = L, L + 4, 2 * H, (B + 15) // 16 * 16
    s = dict(hs=_nan(dev, 2, S + 1, B, H), cs=_nan(dev, 2, S + 1, B, H), gs=_nan(dev, 2, S, B, 4 * H), enc=_nan(dev, B, L, E))
    for k in ("hs", "cs"):
        s[k][0, 0] = 0; s[k][1, S] = 0                         # the zero start slots: forward before t = 0, reverse behind t = L - 1
    if persistent:
        # T2LstmStep.xt: pad rows must be finite - zero-filled when B is not a multiple of 16, as the engine does
        ht = torch.zeros(2, S + 1, H // 16, Bp, 16, device=dev) if B != Bp else _nan(dev, 2, S + 1, H // 16, Bp, 16)
        ht[0, 0] = 0; ht[1, S] = 0
        s["ht"] = ht
    steps = (_lib.S["T2LstmStep"] * 2)()
    incs = (_lib.S["T2LstmStride"] * 2)()
    for dr in range(2):
        t0, sg = (0, 1) if dr == 0 else (S - 1, -1)
        slot_in, slot_out = (0, 1) if dr == 0 else (S, S - 1)
        st = steps[dr]
        st.B, st.H, st.nseg = B, H, 1
        st.wpacked = d["wp"][dr].data_ptr()
        st.seg[0].x = _ptr(s["hs"][dr, slot_in]); st.seg[0].ldx = H
        st.seg[0].w = d["W"][dr].data_ptr(); st.seg[0].ldw = H; st.seg[0].K = H
        st.pre = _ptr(d["pre"], t0 * 8 * H + dr * 4 * H); st.ldpre = Lp * 8 * H
        st.c_prev = _ptr(s["cs"][dr, slot_in]); st.ldc_prev = H
        st.h_out = _ptr(s["hs"][dr, slot_out]); st.ldh = H
        st.h_out2 = _ptr(s["enc"], t0 * E + dr * H); st.ldh2 = L * E
        st.c_out = _ptr(s["cs"][dr, slot_out]); st.ldc_out = H
        st.gates_out = _ptr(s["gs"][dr, t0]); st.ldg = 4 * H
        st.len = d["len"].data_ptr(); st.t = t0
        ic = incs[dr]
        ic.seg_x[0] = sg * B * H
        ic.pre = sg * 8 * H; ic.c_prev = sg * B * H; ic.h_out = sg * B * H; ic.h_out2 = sg * E
        ic.c_out = sg * B * H; ic.gates_out = sg * B * 4 * H; ic.dt = sg
        if persistent:
            st.xt = _ptr(s["ht"][dr, slot_in]); st.ht_out = _ptr(s["ht"][dr, slot_out]); st.ht_col0 = 0
            ic.xt = sg * H * Bp; ic.ht_out = sg * H * Bp
    if persistent:
        assert _lib.call_value("t2_lstm_persist_resident_n", H, H, min(B, 32), 2) == 0, "2 x H/4 <= 16 workgroups must be resident"
        counters = torch.zeros((B + 31) // 32, 256, dtype=torch.int32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("t2_lstm_seq_fwd_persist_pz", steps, incs, 2, S, counters, flag, _st())
        torch.cuda.synchronize()
        assert int(flag[0]) == 0, "an inter-workgroup wait timed out"
    else:
        _lib.call("t2_lstm_seq_fwd", steps, incs, 2, S, _st())
        torch.cuda.synchronize()
    return s


def _bilstm_bwd(dev, case, inp, d, s):
    """t2_lstm_seq_bwd (n = 2) on the forward stashes `s`; returns dpre (B, Lp, 8H) on the CPU."""
    from tacotron2_amd import _lib
    B, L, H = case["B"], case["L"], case["H"]
    S, Lp, E = L, L + 4, 2 * H
    dgt = _nan(dev, 2, S + 1, B, 4 * H)       # dir 0: dgates_t at slot t (zero slot S); dir 1: at slot t + 1 (zero slot 0)
    dgt[0, S] = 0; dgt[1, 0] = 0
    dpre = _nan(dev, B, Lp, 8 * H)
    dc = torch.zeros(2, B, H, device=dev)
    steps = (_lib.S["T2LstmBwdStep"] * 2)()
    incs = (_lib.S["T2LstmBwdStride"] * 2)()
    for dr in range(2):
        sg, t0 = (-1, S - 1) if dr == 0 else (1, 0)          # BPTT runs against the forward processing order
        sp = steps[dr]
        sp.B, sp.H, sp.N4, sp.ncols, sp.epi = B, H, 4 * H, H, 1
        sp.W = d["W"][dr].data_ptr(); sp.ldw = H
        sp.wtpacked = d["wtp"][dr].data_ptr()
        sp.ext1 = _ptr(d["denc"], t0 * E + dr * H); sp.ldx1 = L * E
        sp.gates = _ptr(s["gs"][dr, t0]); sp.ldgs = 4 * H
        sp.c_prev = _ptr(s["cs"][dr, t0 if dr == 0 else t0 + 1]); sp.ldcp = H
        sp.c_cur = _ptr(s["cs"][dr, t0 + 1 if dr == 0 else t0]); sp.ldcc = H
        sp.dc = _ptr(dc[dr]); sp.lddc = H
        sp.dg_next = _ptr(dgt[dr, S if dr == 0 else 0]); sp.lddg = 4 * H
        sp.dg_out = _ptr(dgt[dr, t0 if dr == 0 else t0 + 1]); sp.ldgo = 4 * H
        sp.dg_out2 = _ptr(dpre, t0 * 8 * H + dr * 4 * H); sp.ldgo2 = Lp * 8 * H
        sp.len = d["len"].data_ptr(); sp.t = t0
        ic = incs[dr]
        ic.dg = sg * B * 4 * H; ic.dg2 = sg * 8 * H; ic.ext1 = sg * E; ic.gates = sg * B * 4 * H
        ic.c_prev = sg * B * H; ic.c_cur = sg * B * H; ic.dt = sg
    _lib.call("t2_lstm_seq_bwd", steps, incs, 2, S, _st())
    torch.cuda.synchronize()
    dg = dgt.cpu()
    dpc = dpre.cpu()
    # the second copy (dpre) holds the bits of the time-major stash
    assert torch.equal(dpc[:, :L, :4 * H], dg[0, :S].transpose(0, 1)) and torch.equal(dpc[:, :L, 4 * H:], dg[1, 1:].transpose(0, 1))
    return dpc


@pytest.mark.parametrize("name", list(C.BILSTM_CASES))
def test_bilstm_sequence_fwd_bwd(dev, name):
    """The encoder recurrence, both directions per launch: t2_lstm_seq_fwd (step launches) and t2_lstm_seq_fwd_persist_pz (one
    persistent launch; B = 33 runs two 32-row blocks) against conv_path_ref.bilstm in float64 and against each other, then
    t2_lstm_seq_bwd on each forward's own stashes against autograd."""
    from tacotron2_amd import _lib
    case = C.BILSTM_CASES[name]
    inp = C.make_inputs("bilstm", case)
    B, L, H = case["B"], case["L"], case["H"]
    S, Lp = L, L + 4
    ref = C.bilstm(inp["pre"], inp["W_hh_f"], inp["W_hh_r"], inp["lens"], inp["denc"])
    lens = inp["lens"]
    assert int(lens.min()) == 1 and int(lens.max()) == L
    d = dict(pre=_padded(dev, inp["pre"], 0), W=[inp["W_hh_f"].to(dev), inp["W_hh_r"].to(dev)], len=lens.to(torch.int32).to(dev),
             denc=inp["denc"].to(dev), wp=[], wtp=[])
    for W in d["W"]:
        seg = (_lib.S["T2Seg"] * 1)()
        seg[0].w = W.data_ptr(); seg[0].ldw = H; seg[0].K = H
        wp = _nan(dev, H // 4 * ((H // 16 + 15) // 16 * 16) * 256)
        _lib.call("t2_lstm_pack_fwd", seg, 1, H, wp, _st())
        wtp = _nan(dev, (H + 15) // 16 * ((4 * H // 16 + 31) // 32 * 32) * 256)
        _lib.call("t2_lstm_pack_bwd", W, H, 4 * H, None, 0, 0, H, wtp, _st())
        d["wp"].append(wp); d["wtp"].append(wtp)
    behind = torch.arange(L)[None, :] >= lens[:, None]                       # (B, L)
    bi = torch.arange(B)
    figs, outs = [], {}
    for mode in ("steps", "persistent"):
        s = _bilstm_fwd(dev, case, inp, d, mode == "persistent")
        c = {k: x.cpu() for k, x in s.items()}
        enc = c["enc"]
        assert bool(torch.isfinite(enc).all()) and float(enc[behind].abs().max() if bool(behind.any()) else 0.0) == 0.0
        # the time-major h stash holds the bits of enc: forward h_t at slot t + 1, reverse h_t at slot t
        assert torch.equal(c["hs"][0, 1:].transpose(0, 1), enc[..., :H]) and torch.equal(c["hs"][1, :S].transpose(0, 1), enc[..., H:])
        if mode == "persistent":
            Bp = (B + 15) // 16 * 16
            ht = c["ht"][:, :, :, :B, :].permute(0, 1, 3, 2, 4).reshape(2, S + 1, B, H)          # x16 tiles -> rows
            assert torch.equal(ht[0, 1:], c["hs"][0, 1:]) and torch.equal(ht[1, :S], c["hs"][1, :S])
        c_final = torch.stack([c["cs"][0, lens, bi], c["cs"][1, 0]], 0)      # forward: the state behind step len - 1; reverse: behind t = 0
        figs += [(f"enc[{mode}]", C.rel(enc, ref["enc"]), C.TOL["bilstm.enc"]),
                 (f"c_final[{mode}]", C.rel(c_final.transpose(0, 1), ref["c_final"].transpose(0, 1)), C.TOL["bilstm.c_final"])]
        dpre = _bilstm_bwd(dev, case, inp, d, s)
        assert bool(torch.isnan(dpre[:, L:]).all())                          # pad rows of dpre: untouched
        got = dpre[:, :L]
        assert bool(torch.isfinite(got).all()) and float(got[behind].abs().max() if bool(behind.any()) else 0.0) == 0.0
        figs.append((f"dpre[{mode}]", C.rel(got, ref["dpre"]), C.TOL["bilstm.dpre"]))
        outs[mode] = (enc, c["cs"], c["gs"])
    # the two forwards against each other, at the bound of test_lstm_seq_fwd_persistent_matches_step_launches
    for k, a, b in zip(("enc", "c", "gates"), outs["steps"], outs["persistent"]):
        a, b = torch.nan_to_num(a, nan=0.0).double(), torch.nan_to_num(b, nan=0.0).double()
        figs.append((f"{k}[steps vs persistent]", float((a - b).abs().max() / b.abs().max()), 2e-6))
    _check(name, figs)
