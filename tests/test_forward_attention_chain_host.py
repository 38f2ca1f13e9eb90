"""CPU checks of the reference and the comparison that tests/test_gpu_forward_attention_training.py holds the attention chain
under forward attention to (tests/forward_attention_chain_ref.py): with the prior forced to 1 the restatement is the plain
chain, the hand-coded recursion of the rule equals its autograd, the tolerance constants are anchored to the reference's own
float32 error, every edge a case names carries weight on both sides, and the comparison rejects seven plausible kernel faults."""
import functools

import pytest
import torch

from tests import attention_chain_ref as C
from tests import forward_attention_chain_ref as F


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(inp, init, float64 chain_fa) of a case, computed once and shared (never modified)."""
    inp, init = F.make_inputs_fa(F.CASES_FA[name])
    return inp, init, F.chain_fa(inp, torch.float64, init)


SMALL = [n for n in F.CASES_FA if n != "shipped_T24"]


@pytest.mark.parametrize("name", ["L2_T3", "L33_B17_zero"])
def test_prior_forced_to_one_is_the_plain_chain(name):
    inp, init, _ = _ref(name)
    assert init is None
    a, b = F.chain_fa(inp, torch.float64, prior=False), C.chain(inp, torch.float64)
    for k in C.FWD_OUTPUTS + C.BWD_OUTPUTS:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * max(1.0, float(b[k].abs().max())), k


@pytest.mark.parametrize("name", SMALL)
def test_hand_coded_recursion_equals_autograd(name):
    """de = alpha (g - sigma), r = de / q, P[n] = (r[n] + r[n+1]) / 2 with g = dw + dwx + da + P and the carry G kept separate."""
    inp, init, ref = _ref(name)
    rec = F.recursion_fa(inp, init)
    for k, (e, b) in F.errors_fa(rec, ref, inp).items():
        assert e <= 1e-10, (k, e, b)


def test_tolerances_are_anchored_to_the_float32_reference():
    assert set(F.TOL_FA) == set(C.FWD_OUTPUTS + C.BWD_OUTPUTS)
    for k, tol in F.TOL_FA.items():
        assert tol == 16.0 * F.F32_ERR_FA[k] and 0 < tol <= C.TOL_CAP, (k, tol)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # F32_ERR_FA was measured with one thread
    try:
        worst = {}
        for name, case in F.CASES_FA.items():
            inp, init, r64 = _ref(name)
            r32 = F.chain_fa(inp, torch.float32, init)
            for k, (e, b) in F.errors_fa(r32, r64, inp).items():
                if e > worst.get(k, (0.0,))[0]:
                    worst[k] = (e, name, b)
            assert F.single_position_violations_fa(r32, inp, r64, 0 if init is None else 1) == [], name
    finally:
        torch.set_num_threads(threads)
    print({k: f"{v[0]:.2e} ({v[1]}, sample {v[2]})" for k, v in worst.items()})
    for k, v in worst.items():
        assert v[0] <= F.F32_ERR_FA[k], (k, v)


def test_case_list_and_edge_coverage():
    """The issue's case list, and for each case that names an edge (l, l + 1): the float64 alignments have weight >= 1e-2 on both
    sides of it in some frame before the last one compared (a frame whose r the next frame reads)."""
    have = {(c["L"], c["bump"]) for c in F.CASES_FA.values()}
    assert {(1, None), (2, None), (33, None), (33, 30), (257, 250), (257, 212), (252, 245), (433, 428), (188, None)} <= have
    assert any(c["chunk"] == 5 for c in F.CASES_FA.values()) and any(c["ragged"] for c in F.CASES_FA.values())
    for flag in ("dalign", "tiled", "drop"):
        assert any(c[flag] for c in F.CASES_FA.values()) and any(not c[flag] for c in F.CASES_FA.values()), flag
    named = 0
    for name, case in F.CASES_FA.items():
        if not case["edges"]:
            continue
        _, init, ref = _ref(name)
        assert init is not None
        al = ref["align"][:, :-1]                        # frames 1 .. T-2
        for l0, l1 in case["edges"]:
            named += 1
            both = float(torch.minimum(al[:, :, l0], al[:, :, l1]).max())
            assert both >= 1e-2, (name, l0, l1, both)
    assert named >= 6
    inp, _, ref = _ref("ragged_L60")
    lens = inp["len"]
    assert int(lens[1]) == 1 and all(int(lens[b]) < 60 for b in range(1, 5))
    for b in (2, 3, 4):                                  # the last position of a short sample carries weight (r[len - 1] with r[len] = 0)
        assert float(ref["align"][b, :-1, int(lens[b]) - 1].max()) >= 1e-2, b


FAULT_CASES = [("prior_detached", "L33_B17_zero"), ("shift_wrong_side", "L33_bump30"), ("carry_cut_32", "L33_bump30"),
               ("carry_cut_216", "L257_bump212"), ("carry_cut_256", "L257_bump250"), ("P_in_cum", "L33_B17_zero"),
               ("parity_chunk5", "L33_bump30_chunk5")]


@pytest.mark.parametrize("fault,name", FAULT_CASES)
def test_comparison_rejects_injected_fault(fault, name):
    """errors() against TOL_FA, fed the faulty float64 result in place of a kernel's, rejects an output by >= 10 x its constant."""
    assert {f for f, _ in FAULT_CASES} == set(F.FAULTS_FA)
    inp, init, good = _ref(name)
    bad = F.chain_fa(inp, torch.float64, init, fault=fault)
    ratio = {k: e / F.TOL_FA[k] for k, (e, _) in F.errors_fa(bad, good, inp, names=C.BWD_OUTPUTS).items()}
    print(fault, name, {k: f"{r:.1f}" for k, r in ratio.items()})
    assert max(ratio.values()) >= 10.0, ratio


@pytest.mark.parametrize("name", [n for n in SMALL if F.CASES_FA[n]["L"] > 1])
def test_the_prior_changes_the_result(name):
    """Forward attention is not a small perturbation of the plain chain: > 1e-2 (relative, per sample) in align and dq."""
    inp, init, ref = _ref(name)
    plain = F.chain_fa(inp, torch.float64, init, prior=False)
    for k in ("align", "dq"):
        assert F.errors_fa(ref, plain, inp, names=[k])[k][0] > 1e-2, k


# ---------------------------------------------------------------------------------------------------------------------------
# the interfaces above the kernels (no GPU): C ABI, module API, config / CLI
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_training_option():
    """T2AttnSeq ends in `forward` (appended: every earlier field keeps its offset); the backward option is an entry of its own with
    the workspace as an argument, so T2AttnSeqBwd keeps its layout; NULL dprior / NULL alignments are refused before a launch."""
    import ctypes
    from tacotron2_amd import _lib, build
    fields = [f[0] for f in _lib._structs["T2AttnSeq"]]
    assert fields[-1] == "forward" and fields[-2] == "clk"
    assert [f[0] for f in _lib._structs["T2AttnSeqBwd"]][-1] == "dalign"
    ret, args = _lib._funcs["t2_attn_seq_bwd_forward"]
    assert ret == "int" and [a[0] for a in args] == ["T2AttnSeqBwd", "float", "int64_t", "float", "void"]
    build.build(verbose=False)
    lib = _lib.lib()
    assert lib.t2_sizeof(b"T2AttnSeq") == ctypes.sizeof(_lib.S["T2AttnSeq"])
    assert _lib.S["T2AttnSeq"].forward.offset == ctypes.sizeof(_lib.S["T2AttnSeq"]) - 8      # an int and 4 bytes of tail padding
    sb = _lib.make("T2AttnSeqBwd", B=1, L=4, T=2, A=32, Ad=16, Ef=32, Kl=31, ws_bd=8, th=8, align=8)
    assert lib.t2_attn_seq_bwd_forward(ctypes.addressof(sb), None, 0, None, None) == 1
    assert b"t2_attn_seq_bwd_forward" in lib.t2_last_error()
    sb.align = None
    assert lib.t2_attn_seq_bwd_forward(ctypes.addressof(sb), None, 0, 8, None) == 1


def test_module_switch_is_for_teacher_forcing_only():
    import types
    from tacotron2_amd.model import Tacotron2
    ci, ln = torch.zeros(1, 4, dtype=torch.int64), torch.tensor([4])
    fwd = types.SimpleNamespace(training=False)
    with pytest.raises(ValueError, match="teacher forcing only"):
        Tacotron2.forward(fwd, ci, ln, False, max_len_override=3, train_forward_attention=True)
    with pytest.raises(ValueError):                 # not a bool
        Tacotron2.forward(fwd, ci, ln, True, torch.zeros(1, 4, 16), ln, train_forward_attention="on")
    with pytest.raises(ValueError):                 # the decoding switch still refuses teacher forcing
        Tacotron2.forward(fwd, ci, ln, True, torch.zeros(1, 4, 16), ln, forward_attention=True)


def test_config_key_and_flag(monkeypatch, tmp_path):
    """training.forward_attention switches the option on; `main.py train --forward-attention` hands True to the driver (it wins over
    the key), no flag hands None (= the key decides); a value that is not a bool is refused."""
    from click.testing import CliRunner
    from tacotron2_amd.run.common import train_forward_attention_setting as setting
    from tests.test_forward_attention_host import _cli
    assert setting({}) is False and setting({"forward_attention": True}) is True
    assert setting({"forward_attention": False}, True) is True and setting({"forward_attention": True}, None) is True
    for bad in ({"forward_attention": 1}, {"forward_attention": "yes"}):
        with pytest.raises(ValueError):
            setting(bad)
    with pytest.raises(ValueError):
        setting({}, 1)
    cli, seen, pre = _cli(monkeypatch, tmp_path)
    import tacotron2_amd.run.train as train
    monkeypatch.setattr(train, "do_train", lambda **kw: seen.__setitem__("do_train", kw))
    for flag, want in ((["--forward-attention"], True), ([], None)):
        r = CliRunner().invoke(cli.main, pre + ["train", "--speech-dir", "s", "--synthetic"] + flag, obj={})
        assert r.exit_code == 0, r.output + repr(r.exception)
        assert seen["do_train"]["forward_attention"] is want


def test_ttsmodel_attribute_is_not_a_hyper_parameter():
    from tacotron2_amd.model import TTSModel
    tm = TTSModel(lr=1e-3, weight_decay=0.0, num_chars=5, encoded_dim=16, prenet_dim=16, att_rnn_dim=16, att_dim=16, rnn_hidden_dim=16,
                  postnet_dim=16, num_mels=8, device="cpu")
    assert tm.train_forward_attention is False and "train_forward_attention" not in tm.hparams
    assert "train_forward_attention" not in TTSModel.__init__.__code__.co_varnames
