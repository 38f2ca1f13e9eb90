"""CPU checks of the reference that tests/test_gpu_decode_chain.py holds the decode-loop kernels to (tests/decode_chain_ref.py): the
tolerance constants are anchored to the restatement's own float32 error, every case keeps its stop logits away from the threshold, the
restatement equals the oracle's non-teacher-forced forward, and the layout helpers are what the header describes."""
import torch

from oracle import tacotron2_ref as R
from tests import decode_chain_ref as DC


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_tolerances_are_anchored_to_the_float32_reference():
    """Over the committed case list the float32 run of the restatement differs from the float64 run by at most F32_ERR = TOL / 16 per
    output (and by no less than half of it: a stored constant cannot drift away from what it was measured as); no constant is above the
    cap of the attention chain's."""
    assert set(DC.TOL) == set(DC.OUTPUTS) == set(DC.F32_ERR)
    for k, tol in DC.TOL.items():
        assert tol == 16.0 * DC.F32_ERR[k] and 0 < tol <= DC.TOL_CAP, (k, tol)
    worst = DC.measure_f32_err()
    print("[decode chain] float32 restatement against float64, worst case per output:")
    for k in DC.OUTPUTS:
        print(f"    {k:6s} {worst[k][0]:.2e} ({worst[k][1]})  stored F32_ERR {DC.F32_ERR[k]:.1e}  TOL {DC.TOL[k]:.2e}")
    for k, (e, name) in worst.items():
        assert 0.5 * DC.F32_ERR[k] <= e <= DC.F32_ERR[k], (k, e, name)


def test_case_list_is_what_the_gpu_test_needs():
    """The four state widths are pairwise distinct multiples of 16 in every case but the long-K one (D = Ef = 512), within what the
    entry points accept; the batch sizes cover one partial row block, a second one and the full group; every option occurs once."""
    for name, c in DC.CASES.items():
        assert c["Ef"] % 32 == 0 and c["Ad"] % 16 == 0 and all(c[k] % 16 == 0 for k in "PAD"), name
        assert (c["M"] + 1) % 4 != 0, name                       # pad columns in every proj row
        if name != "K1024":
            assert len({c["P"], c["A"], c["Ef"], c["D"]}) == 4, name
        lens = DC.make_inputs(c)["len"].tolist()
        assert lens[:3] == [13, 1, 7][:c["B"]] and all(1 <= n <= c["L"] for n in lens), name
    assert [DC.CASES[n]["B"] for n in DC.CHAIN] == [1, 5, 17, 64]
    k = DC.CASES["K1024"]
    assert k["D"] + k["Ef"] == 1024 and k["B"] == 3 and k["T"] == 3
    o = {n: DC.CASES[n] for n in DC.OPTIONS}
    assert all(c["B"] == 5 for c in o.values())
    assert o["no_mask"]["no_mask"] and o["controls"]["controls"] and o["zoneout"]["zone_p"] > 0 and o["window"]["window"] \
        and o["forward"]["forward"] and DC.threshold(o["threshold"]) != 0.0 and DC.threshold(DC.CASES["B5"]) == 0.0


def test_stop_logits_keep_their_distance_from_the_threshold():
    """On the float64 reference alone: every stop logit of every frame and utterance lies at least 100 x TOL[stop] x max|stop logit|
    away from the case's threshold, so a kernel within its tolerance takes the reference's stop decisions; and in every case with
    B >= 3 two utterances first stop at different frames inside the run and one never stops."""
    for name, case in DC.CASES.items():
        inp = DC.make_inputs(case)
        ref = DC.decode(case, inp)
        thr = DC.threshold(case)
        have, need = DC.stop_margin(ref["stop"], thr)
        print(f"[decode chain] {name}: threshold {thr:.4f}, smallest |logit - thr| {have:.3g} (needs {need:.3g}), first stops "
              f"{DC.first_stops(ref['stop'], thr)}")
        assert have >= need, (name, have, need)
        assert DC.stop_pattern_ok(case, ref["stop"], thr), (name, DC.first_stops(ref["stop"], thr))
        done, state = DC.stop_rule(ref["stop"], thr)
        assert state.tolist() == [int(all(f is not None for f in DC.first_stops(ref["stop"], thr))), case["T"]]
        # the float32 restatement takes the same decisions
        d32, s32 = DC.stop_rule(DC.decode(case, inp, dtype=torch.float32)["stop"], thr)
        assert torch.equal(done, d32) and torch.equal(state, s32), name


def test_restatement_equals_the_oracle_decoder():
    """float32 weights at r = 1, no options: the float64 restatement against oracle.tacotron2_ref's non-teacher-forced forward (run
    in float64 on the same weights).  With the fold left in float64 the two agree to 1e-11; with W_comb rounded to float32, as the
    kernel gets it, to 1e-7 of the output's maximum - one float32 rounding of the operands, the class of the oracle's own float32 run
    (printed)."""
    d = R.default_dims(num_chars=39, encoded_dim=32, num_mels=16, prenet_dim=16, att_rnn_dim=32, att_dim=16, rnn_hidden_dim=32,
                       postnet_dim=32, dropout=0.5)
    P32 = R.init_params(d, seed=3)
    # (the gate weight scaled, the bias left as it is: with these small weights the loop then stops after five frames)
    P32["decoder.gate.weight"] = P32["decoder.gate.weight"] * DC.GATE_SCALE
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in P32.items()}
    g = torch.Generator().manual_seed(5)
    B, L, N = 4, 17, 9
    lens = torch.tensor([17, 9, 13, 5])
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    pmask = (torch.rand(N + 1, 2, B, 16, generator=g) >= 0.5).double() * 2
    masks = dict(prenet_drop=[[pmask[i, 0], pmask[i, 1]] for i in range(N + 1)])
    trace = {}
    with torch.no_grad():
        mels, _, gates, aligns = R.tacotron2_fwd(P, d, ci, lens, False, max_len_override=N, training=False, masks=masks, trace=trace)
        o32 = R.tacotron2_fwd(P32, d, ci, lens, False, max_len_override=N, training=False,
                              masks=dict(prenet_drop=[[a.float(), b.float()] for a, b in masks["prenet_drop"]]))
    n = mels.shape[1]
    assert n >= 4
    case = dict(DC.CASES["B5"], B=B, T=n, P=16, A=32, Ef=32, D=32, Ad=16, M=16, L=L)
    inp = dict(W_pre1=P["prenet.0.weight"], W_pre2=P["prenet.3.weight"], W_mel=P["decoder.mel_out.weight"],
               b_mel=P["decoder.mel_out.bias"], W_gate=P["decoder.gate.weight"], b_gate=P["decoder.gate.bias"],
               W_ih_att=P["decoder.att_rnn.weight_ih"], W_hh_att=P["decoder.att_rnn.weight_hh"],
               b_att_ih=P["decoder.att_rnn.bias_ih"], b_att_hh=P["decoder.att_rnn.bias_hh"],
               W_ih_dec=P["decoder.lstm.weight_ih"], W_hh_dec=P["decoder.lstm.weight_hh"],
               b_dec_ih=P["decoder.lstm.bias_ih"], b_dec_hh=P["decoder.lstm.bias_hh"],
               Wq=P["decoder.attention.query_layer.weight"],
               U=torch.einsum("af,fck->ack", P["decoder.attention.location_dense.weight"], P["decoder.attention.location_conv.weight"]),
               v=P["decoder.attention.v.weight"][0], memory=trace["memory"], pm=trace["pm"], prenet_mask=pmask[:n], cmel=None,
               dec_pre=None, len=lens)
    lengths = trace["lengths"]
    keep = (torch.arange(n)[None, :] < lengths[:, None])                        # the oracle masks what lies behind `lengths`
    assert 0 < int(keep.sum()) < B * n                                          # some utterance stops inside the run
    for round32, tol in ((False, 1e-11), (True, 1e-7)):
        got = DC.decode(case, inp, DC.build_comb(inp, round32=round32))
        gm = got["mel"].transpose(0, 1).masked_fill(~keep[:, :, None], 0.0)
        gg = got["stop"].transpose(0, 1)[:, :, None].masked_fill(~keep[:, :, None], -1000.0)
        errs = dict(mel=_rel(gm, mels), gate=_rel(gg.masked_fill(~keep[:, :, None], 0.0), gates.masked_fill(~keep[:, :, None], 0.0)),
                    align=_rel(got["align"], aligns))
        print(f"[decode chain] restatement against the oracle, W_comb rounded to float32 = {round32}: {errs}")
        assert max(errs.values()) < tol, (round32, errs)
        assert torch.equal(gg == -1000.0, gates == -1000.0)
        # the count rule of the oracle is the stop rule's first stop where the loop went on
        first = DC.first_stops(got["stop"], 0.0)
        assert [int(x) for x in lengths] == [int((got["stop"][:n, b] >= 0).sum()) for b in range(B)] and len(first) == B
    print("[decode chain] the oracle's own float32 run against its float64 run:",
          dict(mel=_rel(o32[0].double(), mels), align=_rel(o32[3].double(), aligns)))


def test_layout_helpers():
    """tile16 / untile16 round-trip (pad rows zero), and the K chunks of W_comb_t run [ctx | dec_h] - checked on an index-valued
    matrix: element (n, k) = 1000 n + k of W_comb, k in the order [dec_h | ctx] of xproj."""
    g = torch.Generator().manual_seed(1)
    for rows, K in ((1, 16), (5, 48), (16, 32), (17, 240), (53, 160)):
        x = torch.randn(rows, K, generator=g)
        xt = DC.tile16(x)
        Rp = (rows + 15) // 16 * 16
        assert xt.shape == (K // 16, Rp, 16) and torch.equal(DC.untile16(xt, rows), x)
        assert float(xt[:, rows:].abs().sum()) == 0.0
        for c, b, j in ((0, 0, 0), (K // 16 - 1, rows - 1, 15), (K // 32, rows // 2, 7)):
            assert xt[c, b, j] == x[b, 16 * c + j]
    assert torch.equal(DC.untile16(torch.stack([DC.tile16(x), DC.tile16(2 * x)]), rows), torch.stack([x, 2 * x]))
    P, M, D, Ef = 32, 20, 64, 96
    N = P + M + 1
    W = (1000.0 * torch.arange(N)[:, None] + torch.arange(D + Ef)[None, :]).float()
    Wt = DC.tile_comb(W, D, Ef)
    assert Wt.shape == ((D + Ef) // 16, 64, 16)
    for c in range((D + Ef) // 16):
        for j in range(16):
            kk = 16 * c + j
            k = D + kk if kk < Ef else kk - Ef               # chunk position -> column of W_comb
            assert torch.equal(Wt[c, :N, j], W[:, k]), (c, j)
    assert float(Wt[:, N:].abs().sum()) == 0.0
