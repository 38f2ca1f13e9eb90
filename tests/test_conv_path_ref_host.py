"""CPU checks of the references and the comparison that tests/test_gpu_conv_path_kernels.py holds the conv-path, conditioning and
encoder-BiLSTM kernels to (tests/conv_path_ref.py): the restatements equal torch.nn / oracle.tacotron2_ref to 1e-12 in float64, the
tolerance constants are anchored to the references' own float32 error, the ReLU-kink exclusion stays under its cap, the comparison
rejects ten plausible kernel faults by at least 10 x its constants, and the case lists cover every tiling edge."""
import pytest
import torch

from oracle import tacotron2_ref as R
from tests import conv_path_ref as C

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_bn_equals_torch_batchnorm(training, act):
    """C.bn / C.bn_bwd against torch.nn.BatchNorm1d (momentum 0.1, running statistics included), activation / dropout / residual
    applied outside, forward and autograd."""
    B, L, Cn = 3, 11, 13
    g = torch.Generator().manual_seed(act + 10 * training)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, gamma, beta, rm, rv = 2.0 + 0.25 * rn(B, L, Cn), rn(Cn).abs() + 0.5, rn(Cn), 2.0 + 0.1 * rn(Cn), rn(Cn).abs() + 0.1
    drop, res, dy = (torch.rand(B, L, Cn, generator=g) >= 0.5).double() * 2, rn(B, L, Cn), rn(B, L, Cn)
    m = torch.nn.BatchNorm1d(Cn, eps=C.EPS, momentum=0.1).double()
    with torch.no_grad():
        m.weight.copy_(gamma); m.bias.copy_(beta); m.running_mean.copy_(rm); m.running_var.copy_(rv)
    m.train(training)
    m.num_batches_tracked.fill_(7)                       # momentum 0.1 whatever the batch count says
    xl = x.clone().requires_grad_(True)
    z = C._act(m(xl.transpose(1, 2)).transpose(1, 2), act) * drop
    want_dx, want_dg, want_db = torch.autograd.grad((z * dy).sum(), [xl, m.weight, m.bias])
    got = C.bn(x, gamma, beta, rm, rv, training, act, drop, res)
    assert _rel(got["y"], (z + res).detach()) < 1e-12
    assert _rel(got["running_mean"], m.running_mean) < 1e-12 and _rel(got["running_var"], m.running_var) < 1e-12
    if not training:
        assert torch.equal(got["running_mean"], rm) and torch.equal(got["running_var"], rv)
        assert torch.equal(got["mean"], rm) and _rel(got["invstd"], 1 / torch.sqrt(rv + C.EPS)) < 1e-15
    bw = C.bn_bwd(x, gamma, beta, rm, rv, dy, training, act, drop)
    assert _rel(bw["dx"], want_dx) < 1e-12 and _rel(bw["dgamma"], want_dg) < 1e-12 and _rel(bw["dbeta"], want_db) < 1e-12
    # the length mask comes last
    lens = torch.tensor([L, 1, 4])
    y2 = C.bn(x, gamma, beta, rm, rv, training, act, drop, res, lens, -3.5)["y"]
    behind = (torch.arange(L)[None, :] >= lens[:, None])[:, :, None].expand(B, L, Cn)
    assert bool((y2[behind] == -3.5).all()) and torch.equal(y2[~behind], got["y"][~behind])


def test_sync_bn_sums_give_the_whole_batch_statistics():
    case = C.SYNC_BN_CASES["sync_kernel_relu"]
    inp = C.make_inputs("sync_bn", case)
    whole = C.bn(inp["x"], inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"])
    st = C.sync_bn_stats([inp["x"][:2], inp["x"][2:]], inp["shift"])
    assert st["n"] == case["B"] * case["L"]
    assert _rel(st["mean"], whole["mean"]) < 1e-12 and _rel(st["invstd"], whole["invstd"]) < 1e-10


def test_embedding_equals_nn_embedding():
    for case in C.EMBEDDING_CASES.values():
        inp = C.make_inputs("embedding", case)
        assert int((inp["idx"] == 0).sum()) >= 1 or case["L"] == 1
        m = torch.nn.Embedding(case["V"], case["E"], padding_idx=0).double()
        with torch.no_grad():
            m.weight.copy_(inp["table"].double())
        out = m(inp["idx"])
        (out * inp["dout"].double()).sum().backward()
        got = C.embedding(inp["idx"], inp["table"], 2)
        assert torch.equal(got[:, 2:-2], out.detach()) and float(got[:, :2].abs().sum() + got[:, -2:].abs().sum()) == 0.0
        gb = C.embedding_bwd(inp["idx"], inp["dout"], case["V"])
        assert float((gb - m.weight.grad).abs().max()) <= 1e-12 * float(m.weight.grad.abs().max() + 1e-300)
        assert float(gb[0].abs().max()) == 0.0
    assert any(int((C.make_inputs("embedding", c)["idx"] == 0).sum()) for c in C.EMBEDDING_CASES.values() if c["L"] == 1)


def test_bilstm_equals_nn_lstm_on_a_packed_sequence():
    """Outputs, final cell states and - through an invertible input weight - the gradient w.r.t. the input projection, against
    torch.nn.LSTM(bidirectional=True) on a pack_padded_sequence with ragged lengths that include 1 and L."""
    B, L, H = 5, 7, 4
    I = 8 * H                                   # square stacked W_ih: dx = dpre . W_ih determines dpre
    g = torch.Generator().manual_seed(3)
    m = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():                       # nn.LSTM's own init, U(-1/sqrt(H), 1/sqrt(H)), drawn from g and not from the global
        for p in m.parameters():                # generator: the weights, and with them the condition of W_ih, are the same in every run
            p.uniform_(-H ** -0.5, H ** -0.5, generator=g)
    x = torch.randn(B, L, I, generator=g, dtype=F64).requires_grad_(True)
    lens = torch.tensor([L, 1, 3, L, 2])
    denc = torch.randn(B, L, 2 * H, generator=g, dtype=F64)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False)
    out, (hn, cn) = m(packed)
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=L)
    dx_want = torch.autograd.grad((out * denc).sum(), x)[0]
    Wih = torch.cat([m.weight_ih_l0, m.weight_ih_l0_reverse], 0).detach()
    bias = torch.cat([m.bias_ih_l0 + m.bias_hh_l0, m.bias_ih_l0_reverse + m.bias_hh_l0_reverse], 0).detach()
    pre = x.detach() @ Wih.T + bias
    got = C.bilstm(pre, m.weight_hh_l0.detach(), m.weight_hh_l0_reverse.detach(), lens, denc)
    assert _rel(got["enc"], out.detach()) < 1e-12
    assert _rel(got["c_final"], cn.detach()) < 1e-12
    assert _rel(got["dpre"] @ Wih, dx_want) < 1e-12
    assert float(torch.linalg.cond(Wih)) < 1e3
    behind = (torch.arange(L)[None, :] >= lens[:, None])
    assert float(got["enc"][behind].abs().max()) == 0.0 and float(got["dpre"][behind].abs().max()) == 0.0


def test_condition_and_conv_layers_equal_the_oracle():
    """C.condition against R.condition (speaker table + description vector), a five-layer post-net built from C.bn against
    R.postnet_fwd, and the whole encoder (C.embedding, C.bn, C.bilstm) against R.encoder_fwd."""
    d = R.default_dims(num_chars=11, encoded_dim=16, prenet_dim=8, att_rnn_dim=16, att_dim=8, rnn_hidden_dim=16, postnet_dim=24,
                       num_mels=10, dropout=0.5)
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in R.init_params(d, seed=4).items()}
    g = torch.Generator().manual_seed(8)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    B, L, T, E = 3, 9, 12, 16
    # conditioning
    enc, table, desc_in = rn(B, L, E), rn(4, E), rn(B, 6)
    Pc = {"speaker_embedding.weight": table, "description_embeddings_linear.0.weight": rn(128, 6) * 0.3,
          "description_embeddings_linear.0.bias": rn(128) * 0.1, "att_encoder.weight": rn(8, E + 128)}
    spk = torch.tensor([2, 2, 0])
    want, _ = R.condition(Pc, dict(speaker_tokens=True, description_embeddings=True), enc, spk, desc_in)
    desc = torch.tanh(desc_in @ Pc["description_embeddings_linear.0.weight"].T + Pc["description_embeddings_linear.0.bias"])
    assert _rel(C.condition(enc, table, spk, desc)["memory"], want) < 1e-12
    want, _ = R.condition(dict(Pc, **{"att_encoder.weight": rn(8, E)}), dict(speaker_tokens=False, description_embeddings=False), enc)
    assert torch.equal(C.condition(enc, None, None, None)["memory"], want)
    # post-net: conv + BatchNorm + tanh (not on the last layer) + dropout, training mode, new running statistics
    mels = rn(B, T, 10) - 5.5
    drops = [(torch.rand(B, T, c, generator=g) >= 0.5).double() * 2 for c in (24, 24, 24, 24, 10)]
    ns = {}
    want = R.postnet_fwd(P, mels, True, drops, ns)
    x = mels
    for li in range(5):
        k = f"postnet.postnet.{4 * li + 1}"
        o = C.bn(R.conv1d_cl(x, P[f"postnet.postnet.{4 * li}.weight"], None), P[k + ".weight"], P[k + ".bias"], P[k + ".running_mean"],
                 P[k + ".running_var"], True, 2 if li < 4 else 0, drops[li])
        x = o["y"]
        assert _rel(o["running_mean"], ns[k + ".running_mean"]) < 1e-12 and _rel(o["running_var"], ns[k + ".running_var"]) < 1e-12
    assert _rel(x, want) < 1e-12
    # encoder
    lens = torch.tensor([L, 1, 5])
    idx = torch.randint(1, 11, (B, L), generator=g) * (torch.arange(L)[None, :] < lens[:, None])
    edrop = [(torch.rand(B, L, E, generator=g) >= 0.5).double() * 2 for _ in range(3)]
    want = R.encoder_fwd(P, idx, lens, True, edrop)
    x = C.embedding(idx, P["encoder.embedding.weight"], 0)
    for li, i in enumerate((0, 4, 8)):
        k = f"encoder.convolutions.{i + 1}"
        x = C.bn(R.conv1d_cl(x, P[f"encoder.convolutions.{i}.weight"], P[f"encoder.convolutions.{i}.bias"]), P[k + ".weight"],
                 P[k + ".bias"], P[k + ".running_mean"], P[k + ".running_var"], True, 1, edrop[li])["y"]
    pre = torch.cat([x @ P["encoder.lstm.weight_ih_l0" + s].T + P["encoder.lstm.bias_ih_l0" + s] + P["encoder.lstm.bias_hh_l0" + s]
                     for s in ("", "_reverse")], 2)
    got = C.bilstm(pre, P["encoder.lstm.weight_hh_l0"], P["encoder.lstm.weight_hh_l0_reverse"], lens)["enc"]
    assert _rel(got, want) < 1e-12


def test_conv_grads_and_colsum_are_the_operations():
    inp = C.make_inputs("conv", C.CONV_CASES["Ci32_Co48"])
    x, w = inp["x"].double().requires_grad_(True), inp["w"].double().requires_grad_(True)
    dx, dw = torch.autograd.grad((R.conv1d_cl(x, w, None) * inp["dy"].double()).sum(), [x, w])
    got = C.conv_grads(inp["x"], inp["w"], inp["dy"])
    assert _rel(got["conv_dx"], dx) < 1e-12 and _rel(got["conv_dw"], dw) < 1e-12
    xs = C.make_inputs("colsum", C.COLSUM_CASES["R300_C80_ld96_o0"])["x"]
    assert _rel(C.colsum(xs), xs.double().sum(0)) < 1e-12


def test_tolerances_are_anchored_to_the_float32_references():
    """F32_ERR is what the float32 run of each reference differs from its float64 run by, over the committed case lists: no case
    exceeds its stored constant, no stored constant is more than twice the measured worst, TOL = 16 x F32_ERR."""
    worst = C.measure_f32_err()
    print({k: f"{v[0]:.2e} ({v[1]})" for k, v in worst.items()})
    assert set(worst) == set(C.F32_ERR) == set(C.TOL)
    for k, (e, name) in worst.items():
        assert e <= C.F32_ERR[k] <= 2.0 * e, (k, e, name, C.F32_ERR[k])
        assert C.TOL[k] == 16.0 * C.F32_ERR[k]
    assert C.STAT_BOUNDS == dict(mean=2e-6, invstd_kernel=2e-5, invstd_tiles=3e-6, running=1e-5)


def test_relu_kink_exclusion_stays_under_its_cap():
    names = [n for n, c in C.BN_CASES.items() if c["act"] == 1]
    assert len(names) >= 4
    for n in names:
        inp, fwd, _ = C.bn_reference(n)
        assert inp["kink_share"] <= C.KINK_SHARE, (n, inp["kink_share"])
        assert float(inp["dy"][fwd["pre"].abs() <= C.KINK].abs().sum()) == 0.0
    case = C.SYNC_BN_CASES["sync_kernel_relu"]
    inp = C.make_inputs("sync_bn", case)
    pre = C.bn(inp["x"], inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"], True, 1, inp["drop"])["pre"]
    assert C.kink_mask(pre)[1] <= C.KINK_SHARE


# -----------------------------------------------------------------------------------------------------------------
# the comparison rejects plausible faults by >= 10 x its constants
# -----------------------------------------------------------------------------------------------------------------
def _bn_args(inp):
    return inp["x"], inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"]


@pytest.mark.parametrize("name", ["lp7_relu_drop", "c8_relu", "lp7_tanh_res_len"])
def test_rejects_running_variance_from_the_biased_variance(name):
    inp, ref, _ = C.bn_reference(name)
    bad = C.bn(*_bn_args(inp), fault="biased_running_var")
    assert float((bad["running_var"] - ref["running_var"]).abs().max()) > 10 * C.STAT_BOUNDS["running"]


def test_rejects_sync_statistics_over_the_local_row_count():
    for case in C.SYNC_BN_CASES.values():
        inp = C.make_inputs("sync_bn", case)
        shards = [inp["x"][:2], inp["x"][2:]]
        ref, bad = C.sync_bn_stats(shards, inp["shift"]), C.sync_bn_stats(shards, inp["shift"], fault="local_count")
        assert float(((bad["invstd"] - ref["invstd"]).abs() / ref["invstd"]).max()) > 10 * C.STAT_BOUNDS["invstd_kernel"]
        n, nl = ref["n"], bad["n"]
        rv = [0.9 * inp["running_var"].double() + 0.1 * ref["var"] * k / (k - 1) for k in (n, nl)]     # n = 5L in the unbiased factor
        assert float((rv[0] - rv[1]).abs().max()) > 10 * C.STAT_BOUNDS["running"] or case["L"] > 20


@pytest.mark.parametrize("name", list(C.BN_CASES))
def test_rejects_parameter_gradients_overwritten(name):
    inp, _, bwd = C.bn_reference(name)
    for k, start in (("dgamma", inp["dgamma0"]), ("dbeta", inp["dbeta0"])):
        assert C.rel(bwd[k], start.double() + bwd[k], False) > 10 * C.TOL["bn." + k], k


@pytest.mark.parametrize("name", ["r135_relu_drop", "r135_tanh_dypad", "r135_none_res_len"])
def test_rejects_statistics_without_the_last_partial_row_block(name):
    inp, ref, _ = C.bn_reference(name)
    case = C.BN_CASES[name]
    bad = C.bn(*_bn_args(inp), act=case["act"], drop=inp["drop"], res=inp["res"], lens=inp["lens"], fill=case["fill"], fault="tail_rows")
    assert C.rel(bad["y"], ref["y"]) > 10 * C.TOL["bn.y"]
    assert float((bad["mean"] - ref["mean"]).abs().max()) > 10 * C.STAT_BOUNDS["mean"] * max(1.0, abs(case["level"]) + 1)


@pytest.mark.parametrize("fault", ["res_before_drop", "fill_before_res"])
def test_rejects_wrong_epilogue_order(fault):
    hit = 0
    for name, case in C.BN_CASES.items():
        if not case["res"] or (fault == "res_before_drop" and not case["drop"]) or (fault == "fill_before_res" and not case["lens"]):
            continue
        inp, ref, _ = C.bn_reference(name)
        bad = C.bn(*_bn_args(inp), training=case["training"], act=case["act"], drop=inp["drop"], res=inp["res"], lens=inp["lens"],
                   fill=case["fill"], fault=fault)
        assert C.rel(bad["y"], ref["y"]) > 10 * C.TOL["bn.y"], name
        hit += 1
    assert hit >= 2


def test_rejects_embedding_gradient_delivered_to_row_0():
    for case in C.EMBEDDING_CASES.values():
        inp = C.make_inputs("embedding", case)
        if not int((inp["idx"] == 0).sum()):
            continue
        ref = inp["dtable0"].double() + C.embedding_bwd(inp["idx"], inp["dout"], case["V"])
        bad = inp["dtable0"].double() + C.embedding_bwd(inp["idx"], inp["dout"], case["V"], fault="row0")
        assert C.rel(bad, ref, False) > 10 * C.TOL["embedding.dtable"]
        assert not torch.equal(bad[0].float(), inp["dtable0"][0])          # and the bit-equality check of row 0 sees it


@pytest.mark.parametrize("name", list(C.BILSTM_CASES))
def test_rejects_reverse_direction_started_at_the_padded_end(name):
    inp = C.make_inputs("bilstm", C.BILSTM_CASES[name])
    args = (inp["pre"], inp["W_hh_f"], inp["W_hh_r"], inp["lens"], inp["denc"])
    ref, bad = C.bilstm(*args), C.bilstm(*args, fault="reverse_from_L")
    assert C.rel(bad["enc"], ref["enc"]) > 10 * C.TOL["bilstm.enc"]
    assert C.rel(bad["dpre"], ref["dpre"]) > 10 * C.TOL["bilstm.dpre"]


def test_rejects_colsum_without_the_last_rows():
    hit = 0
    for case in C.COLSUM_CASES.values():
        if case["R"] % 4 == 0:
            continue
        inp = C.make_inputs("colsum", case)
        ref, bad = inp["out0"].double() + C.colsum(inp["x"]), inp["out0"].double() + C.colsum(inp["x"], fault="drop_tail")
        assert C.rel(bad, ref, False) > 10 * C.TOL["colsum"], case["name"]
        hit += 1
    assert hit >= 4


def test_rejects_a_pad_row_left_non_zero():
    """The pad rows of y / dx are compared exactly: the smallest value anywhere in them is seen."""
    B, L, Cn, pad = 2, 3, 8, 2
    buf = torch.zeros(B, L + 2 * pad, Cn)
    assert C.pad_rows_are_zero(buf, L, pad)
    for b, row in ((0, 0), (1, 1), (0, L + pad), (1, L + 2 * pad - 1)):
        bad = buf.clone()
        bad[b, row, Cn - 1] = 1e-38
        assert not C.pad_rows_are_zero(bad, L, pad)
    bad = buf.clone()
    bad[1, pad] = float("nan")                  # a data row is not its business
    assert C.pad_rows_are_zero(bad, L, pad)


def test_case_lists_cover_every_edge():
    bn = list(C.BN_CASES.values())
    rows = [c["B"] * c["L"] for c in bn]
    assert any(r > 128 and r % 4 for r in rows)                                   # a partial 128-row block that is no multiple of 4
    assert any(c["C"] % 64 and c["C"] > 64 for c in bn) and any(c["C"] < 64 for c in bn)
    assert any(c["B"] * (c["L"] + 4) * c["C"] > 4096 * 256 for c in bn)           # the apply kernels' grid-stride loops wrap
    assert {(c["B"], c["L"], c["C"]) for c in bn} == {(3, 45, 80), (2, 3, 64), (5, 131, 200), (2, 9, 8), (4, 1030, 256)}
    assert 18 <= len(bn) <= 24
    for key, vals in (("act", (0, 1, 2)), ("drop", (0, 1)), ("res", (0, 1)), ("lens", (0, 1)), ("training", (0, 1)), ("dy_pad", (0, 1)),
                      ("prezeroed", (0, 1)), ("shift", (0, 1))):
        for v in vals:
            assert sum(int(c[key]) == v for c in bn) >= 2, (key, v)
    for act in (0, 1, 2):                                                          # eval mode with every activation
        assert any(c["act"] == act and not c["training"] for c in bn)
    for c in bn:
        if c["lens"]:
            lens = C.make_inputs("bn", c)["lens"]
            assert int(lens[0]) == c["L"] and int(lens[1]) == 1
    assert any(c["tiles"] for c in C.SYNC_BN_CASES.values()) and any(not c["tiles"] for c in C.SYNC_BN_CASES.values())
    cond = list(C.CONDITION_CASES.values())
    assert {c["L"] % 16 for c in cond} >= {0, 1} and {c["L"] for c in cond} == {1, 16, 17, 37}
    assert any(c["Ef"] > 256 for c in cond) and {(c["E"], c["Ef"]) for c in cond} == {(32, 32), (32, 160), (200, 328)}
    for key in ("spk", "ddesc"):
        assert any(c[key] for c in cond) and any(not c[key] for c in cond)
    spk = C.make_inputs("condition", cond[0])["spk"]
    assert int(spk[0]) == int(spk[1])                                              # two utterances share a speaker row
    cs = list(C.COLSUM_CASES.values())
    vec = lambda c: c["C"] % 4 == 0 and c["C"] >= 256 and c["ld"] % 4 == 0 and c["off"] % 4 == 0
    assert any(vec(c) and c["C"] % 256 for c in cs) and sum(vec(c) for c in cs) == 4 and sum(not vec(c) for c in cs) == 5
    assert any(c["C"] == 260 and c["off"] == 1 for c in cs) and any(c["C"] == 260 and c["ld"] == 261 for c in cs)
    assert any(vec(c) and c["R"] == 1 for c in cs) and any(c["R"] % 4 for c in cs)
    assert {(c["E"], c["B"], c["L"]) for c in C.EMBEDDING_CASES.values()} == {(E, B, L) for E in (8, 80) for B, L in ((1, 1), (3, 50))}
    assert {(c["B"], c["L"], c["H"]) for c in C.BILSTM_CASES.values()} == {(3, 7, 16), (17, 6, 32), (33, 5, 16)}
    for c in C.BILSTM_CASES.values():
        lens = C.make_inputs("bilstm", c)["lens"]
        assert int(lens[0]) == c["L"] and int(lens[1]) == 1 and len(set(lens.tolist())) > 1
    assert any(c["rows"] * c["C"] > 4096 * 256 for c in C.TANH_CASES.values())
    assert max(C.POINTWISE_SIZES) > 4096 * 256 and set(C.POINTWISE_SIZES) == {1, 257, 4096 * 256 + 7}
    assert {(c["Ci"], c["Co"], c["K"]) for c in C.CONV_CASES.values()} == {(32, 48, 5), (80, 32, 5)}
