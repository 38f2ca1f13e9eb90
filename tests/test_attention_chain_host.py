"""CPU checks of the reference and the comparison that tests/test_gpu_attention_chain.py holds the attention-chain kernels
to (tests/attention_chain_ref.py): the restatement equals the oracle, the tolerance constants are anchored to the
reference's own float32 error, the case list covers every tiling edge, and the comparison rejects six plausible
kernel faults by at least 10 x its constants."""
import pytest
import torch

from oracle import tacotron2_ref as R
from tests import attention_chain_ref as C


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_restatement_equals_oracle_loop():
    """float64 att_h / ctx / align of the restatement against a loop over the attention half of R.decoder_step (R.lstm_cell +
    R.attention_fwd with the UNFOLDED location_conv / location_dense), and the per-sample dU summed over samples and pushed
    through the fold against autograd's gradients of the two unfolded weights of that loop."""
    B, L, T, A, Ad, Ef, F = 4, 41, 5, 32, 32, 64, 32
    case = dict(B=B, L=L, T=T, A=A, Ad=Ad, Ef=Ef, drop=True, dalign=True, tiled=False)
    inp = {k: (x.double() if torch.is_tensor(x) and x.is_floating_point() else x) for k, x in C.make_inputs(case, seed=5).items()}
    g = torch.Generator().manual_seed(6)
    Wd = (torch.randn(Ad, F, generator=g, dtype=torch.float64) * F ** -0.5).requires_grad_(True)
    Wc = (torch.randn(F, 2, C.KL, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    inp["U"] = torch.einsum("af,fck->ack", Wd, Wc).detach()
    ref = C.chain(inp, torch.float64)

    P = {"decoder.attention.query_layer.weight": inp["Wq"], "decoder.attention.v.weight": inp["v"][None],
         "decoder.attention.location_conv.weight": Wc, "decoder.attention.location_dense.weight": Wd}
    mask = torch.arange(L)[None, :] >= inp["len"][:, None]
    att_h = torch.zeros(B, A, dtype=torch.float64); att_c = torch.zeros(B, A, dtype=torch.float64)
    ctx = torch.zeros(B, Ef, dtype=torch.float64); w = torch.zeros(B, L, dtype=torch.float64); cum = torch.zeros(B, L, dtype=torch.float64)
    obj = 0.0
    hs, cs, ws = [], [], []
    for t in range(T):
        gates = inp["pre"][t] + ctx @ inp["W_ih_ctx"].T + att_h @ inp["W_hh"].T
        att_h, att_c = R.lstm_cell(gates, att_c)
        att_h = att_h * inp["att_drop"][t]
        ctx, w = R.attention_fwd(P, att_h, inp["memory"], inp["pm"], torch.stack([w, cum], 1), mask)
        cum = cum + w
        hs.append(att_h); cs.append(ctx); ws.append(w)
        obj = obj + (att_h * inp["dh_ext"][t]).sum() + (ctx * (inp["dctx_ext1"][t] + inp["dctx_ext2"][t])).sum() \
            + (w * inp["dalign"][:, t]).sum()
    gWd, gWc = torch.autograd.grad(obj, [Wd, Wc])
    assert _rel(ref["att_h"], torch.stack(hs).detach()) < 1e-12
    assert _rel(ref["ctx"], torch.stack(cs).detach()) < 1e-12
    assert _rel(ref["align"], torch.stack(ws, 1).detach()) < 1e-12
    dU = ref["dU"].sum(0)
    assert _rel(torch.einsum("ack,fck->af", dU, Wc.detach()), gWd) < 1e-11
    assert _rel(torch.einsum("ack,af->fck", dU, Wd.detach()), gWc) < 1e-11


def test_case_list_covers_every_edge():
    """Every edge the tiling of the kernels has (the issue's list) is the dimension of at least one committed case."""
    have = {k: {c[k] for c in C.CASES.values()} for k in ("B", "L", "T", "A", "Ad", "Ef")}
    want = dict(L={1, 2, 31, 32, 33, 192, 193, 252, 253, 256, 257, 431, 433, 649}, Ef={32, 640, 672, 1056}, Ad={16, 128, 144, 272},
                B={1, 15, 16, 17, 33}, T={1, 2, 7, 24}, A={32, 64, 1024})
    for k, s in want.items():
        assert s <= have[k], (k, sorted(s - have[k]))
    assert any(c["A"] == 1024 and c["Ad"] == 128 and c["Ef"] == 512 and c["T"] == 24 for c in C.CASES.values())
    for flag in ("drop", "dalign", "tiled"):        # every variant on at least two shapes, both ways
        assert sum(bool(c[flag]) for c in C.CASES.values()) >= 2 and sum(not c[flag] for c in C.CASES.values()) >= 2
    assert 16 <= len(C.CASES) <= 24
    for c in C.CASES.values():                      # what the header documents as supported
        assert c["Ad"] % 16 == 0 and c["Ef"] % 32 == 0 and c["A"] % 16 == 0
        inp_len = C.make_inputs(c)["len"]
        assert int(inp_len[0]) == c["L"] and (c["B"] == 1 or int(inp_len[1]) == 1)


def test_tolerances_are_anchored_to_the_float32_reference():
    """Over the committed case list the float32 run of the restatement differs from the float64 run by at most F32_ERR =
    TOL / 16 per output; no constant is above the cap; the float32 run leaves exactly zero where a single-position sample
    must be zero."""
    assert set(C.TOL) == set(C.FWD_OUTPUTS + C.BWD_OUTPUTS)
    for k, tol in C.TOL.items():
        assert tol == 16.0 * C.F32_ERR[k] and 0 < tol <= C.TOL_CAP, (k, tol)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # F32_ERR was measured with one thread (float32 reduction orders depend on the split)
    try:
        worst = {}
        for name, case in C.CASES.items():
            inp = C.make_inputs(case)
            r64, r32 = C.chain(inp, torch.float64), C.chain(inp, torch.float32)
            for k, (e, b) in C.errors(r32, r64, inp["len"]).items():
                if e > worst.get(k, (0.0,))[0]:
                    worst[k] = (e, name, b)
            assert C.single_position_violations(r32, inp, r64) == [], name
    finally:
        torch.set_num_threads(threads)
    print({k: f"{v[0]:.2e} ({v[1]}, sample {v[2]})" for k, v in worst.items()})
    for k, v in worst.items():
        assert v[0] <= C.F32_ERR[k], (k, v)


# (fault, case): each fault a small detach / scale inside the restatement (attention_chain_ref.chain, fault=)
FAULT_CASES = [
    ("cum_cut_216", "L433_Ad144_Ef672"),       # (a) gradient through cum_prev cut for positions >= 216 (a tile's carry lost)
    ("wprev_cut_last15", "L33_B17"),           # (b) gradient through w_prev cut for the last 15 positions (filter overhang)
    ("ef_tail_640", "L433_Ad144_Ef672"),       # (c) memory columns >= 640 without gradient in the context (dw tail loop)
    ("dalign_scale", "mel_tail"),              # (d) dalign x (1 + 1e-2)
    ("dh_last_sample", "L33_B17"),             # (e) the last sample's dh_ext of frame T-1 dropped at B = 17 (second row tile)
    ("din_slices_8", "L193_Ad144"),            # (f) din_part slices >= 8 dropped at Ad = 144 (second pass of the partial sum)
]


@pytest.mark.parametrize("fault,case", FAULT_CASES)
def test_comparison_rejects_injected_fault(fault, case):
    """The comparison the GPU test uses (errors() against TOL), fed the faulty float64 result in place of a kernel's, rejects at
    least one output by >= 10 x its constant."""
    assert {f for f, _ in FAULT_CASES} == set(C.FAULTS)
    inp = C.make_inputs(C.CASES[case])
    good, bad = C.chain(inp), C.chain(inp, fault=fault)
    ratio = {k: e / C.TOL[k] for k, (e, _) in C.errors(bad, good, inp["len"], names=C.BWD_OUTPUTS).items()}
    print(fault, case, {k: f"{r:.1f}" for k, r in ratio.items()})
    assert max(ratio.values()) >= 10.0, ratio
    # the fault-free run passes the same comparison exactly
    assert all(e == 0.0 for e, _ in C.errors(C.chain(inp), good, inp["len"]).values())


def test_metric_has_no_floor_to_hide_under():
    """per_sample_rel: a NaN or a non-zero value against an all-zero reference slice is an infinite error, an error confined to
    one sample is measured against that sample's own maximum, and only single-position samples are excused from the
    zero-reference rule (they get the absolute bound instead)."""
    ref = torch.zeros(3, 4, dtype=torch.float64); ref[0] = 100.0; ref[1] = 1e-3
    got = ref.clone(); got[1, 2] += 1e-6
    e, b = C.per_sample_rel(got, ref, zero_ok={2})
    assert b == 1 and abs(e - 1e-3) < 1e-9
    got2 = ref.clone(); got2[2, 0] = 1e-30
    assert C.per_sample_rel(got2, ref)[0] == float("inf")
    assert C.per_sample_rel(got2, ref, zero_ok={2})[0] == 0.0
    got3 = ref.clone(); got3[0, 1] = float("nan")
    assert C.per_sample_rel(got3, ref)[0] == float("inf")
    # single-position bound: a value above it is reported, one below is not
    inp = C.make_inputs(C.CASES["L31_B15"]); r = C.chain(inp)
    bound = C.single_position_bounds(inp, r, 1)
    assert all(float(x.min()) > 0 for x in bound.values())
    bad = {k: x.clone() for k, x in r.items()}
    bad["dq"][3, 1, 5] = 3.0 * float(bound["dq"][3, 5])
    assert [(k, b) for k, b, _ in C.single_position_violations(bad, inp, r)] == [("dq", 1)]
    ok = {k: x.clone() for k, x in r.items()}
    ok["dq"][3, 1, 5] = 0.5 * float(bound["dq"][3, 5])
    assert C.single_position_violations(ok, inp, r) == []
