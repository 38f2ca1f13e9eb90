"""Zoneout, host side: the float64 restatements of tests/zoneout_ref.py pinned to the oracle, the hand-written backward of
include/tacotron2_amd.h (T2LstmBwdStep) checked against autograd, the tolerance constants re-measured, and the two injected faults
rejected at those tolerances.  No GPU."""
import pytest
import torch

from oracle import tacotron2_ref as R
from tests import attention_chain_ref as C
from tests import zoneout_ref as Z
from tests.helpers import SMALL


def _step_case(seed=5, B=3, L=7):
    d = R.default_dims(**SMALL, dropout=0.5)
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in R.init_params(d, seed=3).items()}
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    A, D, Pd = d["att_rnn_dim"], d["rnn_hidden_dim"], d["prenet_dim"]
    Ef = P["decoder.att_rnn.weight_ih"].shape[1] - Pd
    memory = rn(B, L, Ef)
    pm = memory @ P["att_encoder.weight"].T
    lens = torch.tensor([L, 3, 5][:B])
    lmask = torch.arange(L)[None, :] >= lens[:, None]
    w = torch.softmax(rn(B, L).masked_fill(lmask, float("-inf")), 1)
    st = (rn(B, A) * 0.5, rn(B, A) * 0.5, rn(B, Ef), w, w * 2, rn(B, D) * 0.5, rn(B, D) * 0.5)
    drop = lambda n: (torch.rand(B, n, generator=g) >= 0.1).double() / 0.9
    return d, P, rn(B, Pd), st, memory, pm, lmask, drop(A), drop(D), g


def test_step_without_zone_masks_is_the_oracle_exactly():
    d, P, prev, st, memory, pm, lmask, ad, dd, _ = _step_case()
    ref = R.decoder_step(P, prev, *st, memory, pm, lmask, ad, dd)
    mel, gate, st2 = Z.decoder_step(P, prev, st, memory, pm, lmask, ad, dd)
    for a, b in zip((mel, gate) + st2, ref):
        assert torch.equal(a, b)
    # zero masks change nothing but the sign of a zero; masks of one keep the whole state
    B, A, D = prev.shape[0], d["att_rnn_dim"], d["rnn_hidden_dim"]
    z = dict(att_zone_h=torch.zeros(B, A, dtype=torch.float64), att_zone_c=torch.zeros(B, A, dtype=torch.float64),
             dec_zone_h=torch.zeros(B, D, dtype=torch.float64), dec_zone_c=torch.zeros(B, D, dtype=torch.float64))
    out0 = Z.decoder_step(P, prev, st, memory, pm, lmask, ad, dd, zones=z)
    for a, b in zip((out0[0], out0[1]) + out0[2], ref):
        assert torch.equal(a, b)
    out1 = Z.decoder_step(P, prev, st, memory, pm, lmask, ad, dd, zones={k: v + 1 for k, v in z.items()})
    for i in (0, 1, 5, 6):      # att_h, att_c, dec_h, dec_c
        assert torch.equal(out1[2][i], st[i])


@pytest.mark.parametrize("r,hook", [(1, False), (2, True)])
def test_model_forward_without_zone_masks_is_the_reduction_reference(r, hook):
    """model_fwd swaps the step of reduction_ref.reduction_fwd for decoder_step: without masks every output is that function's,
    bit for bit in float64 (teacher forcing, with and without the forward-attention hook)."""
    from tests import reduction_ref as RR
    from tests.test_reduction_factor_host import _small, _tf_case
    d, P = _small()
    P = RR.grouped_params(P, d, r, seed=1)
    ci, lens, mel, tl, masks = _tf_case(d, 3, 11, 9, r, 21)
    kw = dict(mel=mel, mel_len=tl, training=True, masks=masks, new_stats={}, attention_hook=RR.forward_attention_hook if hook else None)
    a = RR.reduction_fwd(P, d, r, ci, lens, True, **kw)
    b = Z.model_fwd(P, d, r, ci, lens, True, **dict(kw, new_stats={}))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    S = RR.steps_of(9, r)
    z = {k: (torch.rand(S, 3, d["att_rnn_dim" if k.startswith("att") else "rnn_hidden_dim"]) < 0.3).double() for k in Z.ZONE_KEYS}
    c = Z.model_fwd(P, d, r, ci, lens, True, zones=z, **dict(kw, new_stats={}))
    assert float((c[0] - a[0]).abs().max()) > 1e-3          # (and with masks it is another model)


def test_step_expectation_rule_is_the_interpolation():
    """Eval: every mask element is the rate p, so the carried state is p * previous + (1 - p) * the plain cell's."""
    d, P, prev, st, memory, pm, lmask, _, _, _ = _step_case()
    p = 0.1
    B, A, D = prev.shape[0], d["att_rnn_dim"], d["rnn_hidden_dim"]
    z = dict(att_zone_h=torch.full((B, A), p, dtype=torch.float64), att_zone_c=torch.full((B, A), p, dtype=torch.float64),
             dec_zone_h=torch.full((B, D), p, dtype=torch.float64), dec_zone_c=torch.full((B, D), p, dtype=torch.float64))
    plain = R.decoder_step(P, prev, *st, memory, pm, lmask, None, None)
    _, _, got = Z.decoder_step(P, prev, st, memory, pm, lmask, None, None, zones=z)
    assert torch.allclose(got[0], p * st[0] + (1 - p) * plain[2], rtol=0, atol=1e-15)      # att_h
    assert torch.allclose(got[1], p * st[1] + (1 - p) * plain[3], rtol=0, atol=1e-15)      # att_c


@pytest.mark.parametrize("variant", Z.VARIANTS)
@pytest.mark.parametrize("B,H", [(3, 16), (17, 32)])
def test_hand_written_backward_equals_autograd(B, H, variant):
    """The formulas of T2LstmBwdStep (0/1, fractional, stride-0 and single masks) against autograd of the restatement to 1e-12."""
    inp, ref = Z.cell_reference(B, H, variant)
    got = Z.cell_seq_manual(inp, ref, torch.float64)
    for k in Z.CELL_BWD:
        scale = max(1.0, float(ref[k].abs().max()))
        assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * scale, k


@pytest.mark.parametrize("fault", Z.FAULTS)
@pytest.mark.parametrize("variant", ["01", "frac"])
def test_injected_faults_are_rejected_at_the_gpu_tolerance(fault, variant):
    """tanh of the stored (zoned) c instead of the recomputed c~, and a dropped dhz carry: each puts at least one backward output
    over its constant, for 0/1 and for fractional masks (the GPU test applies the same metric and constants)."""
    inp, ref = Z.cell_reference(17, 32, variant)
    ok = Z.cell_errors(Z.cell_seq_manual(inp, ref, torch.float32), ref, Z.CELL_BWD)
    assert all(e <= Z.TOL["cell." + k] for k, e in ok.items()), ok
    bad = Z.cell_errors(Z.cell_seq_manual(inp, ref, torch.float32, fault=fault), ref, Z.CELL_BWD)
    over = {k: e for k, e in bad.items() if e > Z.TOL["cell." + k]}
    assert over, (fault, bad)
    assert max(over.values()) > 100 * max(Z.TOL.values()), (fault, bad)      # by a wide margin, not at the edge of the constant


def test_chain_without_zone_masks_is_the_attention_chain_reference():
    case = dict(Z.CHAIN_CASES["B3_frac"])
    inp = C.make_inputs(case)
    a, b = C.chain(inp, torch.float64), Z.chain(inp, torch.float64)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_chain_with_forward_attention_and_no_zone_masks_is_the_forward_attention_reference():
    from tests import forward_attention_chain_ref as FA
    inp = C.make_inputs(dict(Z.CHAIN_CASES["B3_01_forward"]))
    a, b = FA.chain_fa(inp, torch.float64), Z.chain(inp, torch.float64, forward=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float((b["align"] - Z.chain(inp, torch.float64)["align"]).abs().max()) > 1e-2


def test_tolerance_constants_are_what_the_restatements_measure():
    worst = Z.measure_f32_err()
    assert set(worst) == set(Z.F32_ERR)
    for k, (e, case) in worst.items():
        print(f"[zoneout f32] {k}: {e:.3e} ({case}) / {Z.F32_ERR[k]:.1e}")
        assert e <= Z.F32_ERR[k], (k, e, case)
        assert Z.F32_ERR[k] <= 2.0 * e, (k, e, "the stored constant is more than twice the measured error")
    assert all(abs(Z.TOL[k] - 16.0 * Z.F32_ERR[k]) < 1e-18 for k in Z.TOL) and max(Z.TOL.values()) <= C.TOL_CAP
