"""Batch sizes across the step kernels' row blocks - 16-row MFMA tiles, 32-row blocks of the persistent launches, 64-row blocks
(a batch above 64 rows ends in a short block: where round 4's out-of-bounds read was) - with GUARD BANDS on every engine workspace,
every output and the ParamStore's flat buffers (tacotron2_amd/guard.py).  Every case compares outputs, loss and EVERY parameter
gradient (or the decode outputs) with the oracle, asserts the path it is named for, and ends with every band intact: a kernel that
writes past the end of a workspace, or reads past it into a NaN band, fails here even where the compared numbers would not move.
Also: the persistent launches' counter ring over forwards longer than it (Engine.persist_counters), a check that the bands see a
write into them on the device, and the loss kernel's input checks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tacotron2_ref as R  # noqa: E402
from tests.helpers import SMALL  # noqa: E402
from tests.oracle_jobs import TINY, case as job_case, edge_lengths_case  # noqa: E402
from tests.oracle_pool import oracle, release  # noqa: E402
from tests.test_attention_window_host import windowed_ref  # noqa: E402
from tests.test_gpu_fullsize import _hip_train_and_compare  # noqa: E402
from tests.test_gpu_model import MEL_L1_TOL, _dev, build_engine, l1, masks_to_device, mx  # noqa: E402

GUARD = 65536
MID = dict(num_chars=39, encoded_dim=128, prenet_dim=64, att_rnn_dim=256, att_dim=64, rnn_hidden_dim=256, postnet_dim=128,
           num_mels=80, dropout=0.5, speaker_tokens=True, num_speakers=4)


def _blocks64(B):
    """(64-row blocks, rows of the last one) of a batch of B in the step kernels."""
    n = (B + 63) // 64
    return n, B - 64 * (n - 1)


def _paths(B, dec_chain="persistent"):
    """The forward took the paths its batch size selects: the decoder-LSTM chain as persistent launches up to 64 rows (two 32-row
    blocks above 32), per-frame step launches above; the encoder BiLSTM as one persistent launch up to 32 rows."""
    def check(ctx):
        assert ctx["B"] == B
        assert ctx["persist"] == (B <= 64 and dec_chain == "persistent"), ctx["persist"]
        assert ctx["enc_persist"] == (B <= 32), ctx["enc_persist"]
    return check


def _clean(eng):
    assert eng.guard_check() == []
    eng.check_persistent_kernels()


# ---- (a) training step at TINY dims across the row blocks ---------------------------------------------------------------------
TINY_CASES = [(B, 21, 12, "persistent") for B in (1, 16, 17, 31, 32, 33, 63, 64, 65, 97, 129)] + \
             [(B, 21, 12, "steps") for B in (32, 33, 64)] + \
             [(33, 255, 63, "persistent"), (65, 256, 65, "persistent"), (17, 257, 65, "persistent")]


@pytest.mark.oracle("guard_tiny:{B}-{L}-{T}-{dec_chain}")
@pytest.mark.parametrize("B,L,T,dec_chain", TINY_CASES)
def test_guarded_tiny_train_step_across_row_blocks_matches_oracle(B, L, T, dec_chain):
    """Forward, loss, every gradient and the BN statistics against the oracle with guard bands on; ragged lengths down to one
    character and one frame in the same batch (L = 255 / 256 / 257: the attention kernels' 256-position rounds)."""
    dev = _dev()
    name = f"guard_tiny:{B}-{L}-{T}-{dec_chain}"      # (one job per test: the pool hands a result out once)
    c = job_case(name)
    ci, lens, mel, tl = c["case"][:4]
    assert ci.shape == (B, L) and mel.shape[1] == T and int(lens.max()) == L and int(tl.max()) == T
    if B > 1:
        assert int(lens.min()) == 1 and int(tl.min()) == 1
    if B > 64:
        assert _blocks64(B) == {65: (2, 1), 97: (2, 33), 129: (3, 1)}[B]

    def schedule(eng):
        eng.dec_chain = dec_chain
        assert eng.guard_bytes == GUARD and eng.ps.guard_bytes == GUARD
    _hip_train_and_compare(c["d"], c["P"], c["case"], dev, job=name, guard_bytes=GUARD, check_engine=schedule,
                           check_ctx=_paths(B, dec_chain))


# ---- (b) training step at the shipped sizes ----------------------------------------------------------------------------------
@pytest.mark.oracle("guard_full:{B}")
@pytest.mark.parametrize("B", [33, 65, 129])
def test_guarded_shipped_dims_train_step_above_32_rows_matches_oracle(B):
    """E = 512, LSTMs of 1024 (the packed / tiled kernel variants the bench runs) at 33 rows (two persistent 32-row blocks, three
    16-row tiles) and 65 / 129 rows (a last 64-row block of one row): every gradient against the oracle, bands intact."""
    dev = _dev()
    name = f"guard_full:{B}"
    c = job_case(name)
    _hip_train_and_compare(c["d"], c["P"], c["case"], dev, kw_cpu=c["kw"], kw_dev={k: v.to(dev) for k, v in c["kw"].items()},
                           job=name, guard_bytes=GUARD, check_ctx=_paths(B))


# ---- (c) autoregressive decoding, guarded --------------------------------------------------------------------------------------
def decode_case(B, N=24, seed=9):
    """MID dims, B utterances with ragged texts down to one character, replayed prenet masks, and the stop projection of
    tests/test_gpu_attention_window.py (stop logits cross zero at different frames)."""
    d = R.default_dims(**MID)
    P = R.init_params(d, seed=seed)
    P["decoder.gate.bias"] = P["decoder.gate.bias"] + 0.3
    P["decoder.gate.weight"] = P["decoder.gate.weight"] * 6.0
    g = torch.Generator().manual_seed(100 + B)
    L = 23
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    spk = torch.randint(0, 4, (B,), generator=g, dtype=torch.int32)
    pm = (torch.rand(N + 1, 2, B, d["prenet_dim"], generator=g) >= 0.5).float() * 2
    return d, P, ci, lens, spk, pm, N


DECODE_CASES = [(1, None, 1), (1, (1, 3), 3), (64, None, 3), (64, (1, 3), 1), (65, None, 1), (65, (1, 3), 3), (129, None, 3),
                (129, (1, 3), 1)]


@pytest.mark.parametrize("B,window,check_every,training", [c + (False,) for c in DECODE_CASES] + [(65, None, 3, True)])
def test_guarded_decode_across_groups_matches_oracle(B, window, check_every, training):
    """Engine.infer at 1, 64, 65 and 129 utterances (one, two and three decode groups; the last group of one row), without and with
    the attention window, host checks every frame and every third frame, against the float64 (windowed) reference: frame count,
    lengths, outputs, alignments, masked tails - and every band intact."""
    dev = _dev()
    d, P, ci, lens, spk, pm, N = decode_case(B)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    L = ci.shape[1]
    with torch.no_grad():
        rm, rp, rg, ra, rl = windowed_ref(P64, d, ci, lens, N, window or (L, L), speaker_id=spk, prenet_drop=pm, training=training)
    if B > 1:
        assert len(set(rl.tolist())) > 1, rl             # ragged stops, or the case would not test the stop path
    eng, ps = build_engine(d, P, dev, guard_bytes=GUARD)
    mels, post, gates, al, lengths = eng.infer(ci.to(dev), lens.to(dev), N, speaker_id=spk.to(dev), prenet_masks=pm.to(dev).contiguous(),
                                               check_every=check_every, attention_window=window, training=training)
    groups = sorted(k for k in eng._ws if k.startswith("inf") and k.endswith(".state"))
    assert groups == [f"inf{g}.state" for g in range((B + 63) // 64)]
    assert ("inf0.win_peak" in eng._ws) == (window is not None)
    _clean(eng)
    assert mels.shape == rm.shape, (mels.shape, rm.shape)
    assert torch.equal(lengths.cpu(), rl)
    assert l1(mels, rm) < MEL_L1_TOL and l1(post, rp) < MEL_L1_TOL
    assert mx(al, ra) < 5e-5
    assert torch.equal(gates.cpu() == -1000.0, rg == -1000.0)


# ---- (d) the persistent launches' counter ring -----------------------------------------------------------------------------------
@pytest.mark.oracle("ring_step")
def test_training_step_with_more_persistent_launches_than_the_counter_ring():
    """16-frame chunks over 760 frames at 33 rows: 51 decoder-LSTM launches of two 32-row blocks, more than the ring's 96 blocks
    (this raised an AssertionError on the host before).  Full training step against the oracle, bands intact."""
    from tacotron2_amd.engine import Engine, _chunk_sizes
    dev = _dev()
    c = job_case("ring_step")

    def schedule(eng):
        eng.chunk = 16
        assert len(_chunk_sizes(760, 16)) * 2 > Engine.PERSIST_RING
    _hip_train_and_compare(c["d"], c["P"], c["case"], dev, job="ring_step", guard_bytes=GUARD, check_engine=schedule,
                           check_ctx=_paths(33))


@pytest.mark.oracle("ring_fwd")
def test_long_forward_then_decode_then_the_same_forward():
    """T = 2900 frames (about 34 s of audio) at 33 rows with the default chunks: 98 counter blocks.  The forward against the oracle;
    then a decode and the same forward again - the ring starts over per phase, so the repeat gives the same outputs."""
    dev = _dev()
    c = job_case("ring_fwd")
    d, P, (ci, lens, mel, tl, gate, masks) = c["d"], c["P"], c["case"]
    o = oracle("ring_fwd")
    ref = o["ref"]
    release("ring_fwd")
    eng, ps = build_engine(d, P, dev, guard_bytes=GUARD)
    assert eng.chunk == 64
    args = (ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev))
    dmasks = masks_to_device(masks, dev)
    outs, ctx = eng.forward_tf(*args, training=True, masks=dmasks, save_for_backward=False)
    _paths(33)(ctx)
    _clean(eng)
    assert l1(outs[0], ref[0]) < MEL_L1_TOL and l1(outs[1], ref[1]) < MEL_L1_TOL
    assert mx(outs[3], ref[3]) < 2e-5
    assert ((outs[2].cpu() == -1000.0) == (ref[2] == -1000.0)).all()
    first = [x.clone() for x in outs]
    eng.infer(ci.to(dev), lens.to(dev), 5, check_every=2)
    outs2, _ = eng.forward_tf(*args, training=True, masks=dmasks, save_for_backward=False)
    _clean(eng)
    for a, b in zip(first, outs2):
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max()))


def test_encoder_submodule_called_120_times():
    """model/submodules.py's Encoder drives the persistent encoder launch without a phase: 120 calls (more than the ring's 96 blocks),
    every output the same as the first, the first against the oracle."""
    from tacotron2_amd.model import Tacotron2
    dev = _dev()
    d = R.default_dims(**SMALL, dropout=0.0)
    P = R.init_params(d, seed=8)
    m = Tacotron2(dropout=0.0, device=dev, **SMALL)
    m.load_state_dict(P)
    m.eval()
    m._engine.guard_bytes = GUARD
    g = torch.Generator().manual_seed(1)
    B, L = 5, 13
    lens = torch.tensor([13, 9, 4, 1, 11])
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    cid, lensd = ci.to(dev), lens.to(dev)
    first = m.encoder(cid, lensd)
    assert m._engine._persist_sync is not None and m._engine.persist_resident(SMALL["encoded_dim"] // 2, B, 2)
    assert mx(first, R.encoder_fwd(P, ci, lens, False)) < 1e-5
    for _ in range(119):
        assert torch.equal(m.encoder(cid, lensd), first)
    _clean(m._engine)


# ---- (e) the bands see a write on the device ---------------------------------------------------------------------------------------
def test_guard_bands_detect_a_write_past_a_workspace_on_the_device():
    """Test hook: the after-band of `proj` (T, B, M + 1), which the projection GEMM writes, starts one frame before the end of the
    view - the GEMM's last frame lands in the band, inside the allocation.  guard_check names the buffer, the side and the offset."""
    from tacotron2_amd._lib import T2Error
    dev = _dev()
    d = R.default_dims(**TINY)
    P = R.init_params(d, seed=4)
    B, L, T = 5, 11, 7
    M = d["num_mels"]
    ci, lens, mel, tl, gate, masks = edge_lengths_case(d, B, L, T, 44)
    eng, ps = build_engine(d, P, dev, guard_bytes=GUARD)
    frame = B * (M + 1)
    eng._guard_short["proj"] = frame
    eng.forward_tf(ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev), training=False, save_for_backward=False)
    hits = eng.guard_check()
    n = T * B * (M + 1)
    assert [h[:4] for h in hits] == [("proj", "after", n - frame, frame)], hits
    with pytest.raises(T2Error, match="proj after"):
        eng.check_persistent_kernels()


# ---- loss inputs on two devices --------------------------------------------------------------------------------------------------
def test_loss_rejects_a_target_on_another_device(monkeypatch):
    from tacotron2_amd.model import tts_model

    def kernel_must_not_run(*a, **k):
        raise AssertionError("the loss kernel was reached with a host pointer")
    monkeypatch.setattr(tts_model, "call", kernel_must_not_run)
    dev = _dev()
    B, T, M = 3, 5, 16
    mel = torch.randn(B, T, M, device=dev)
    gate = torch.randn(B, T, 1, device=dev)
    mlen = torch.tensor([5, 2, 1], dtype=torch.int32)
    for bad in ("mel_tgt", "gate_tgt", "mel_len"):
        args = dict(mel_tgt=mel.clone(), gate_tgt=torch.ones(B, T, 1, device=dev), mel_len=mlen.to(dev))
        args[bad] = args[bad].cpu()
        with pytest.raises(ValueError, match="cpu"):
            tts_model._LossTermsFn.apply(mel, mel + 0.1, gate, args["mel_tgt"], args["gate_tgt"], args["mel_len"])
