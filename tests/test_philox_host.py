"""CPU checks of tests/philox_ref.py, the bit-exact reference tests/test_gpu_philox.py holds t2_philox_mask, t2_philox_bernoulli and
the engine's masks to: the generator reproduces the published Philox4x32-10 known answers (Random123's kat_vectors), the two mask
functions share one convention, and the stream ids of one training step are distinct, stay inside the step's 64 ids and are what
Engine.make_masks passes to the library (recorded on a CPU engine, no library call is made)."""
import itertools

import numpy as np
import pytest

from tests import philox_ref as PR

KAT = [   # counter, key -> output (Random123 kat_vectors, philox4x32 10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SMALL = dict(encoded_dim=32, prenet_dim=16, att_rnn_dim=48, rnn_hidden_dim=64, num_mels=20, postnet_dim=24, dropout=0.5)
OPTIONS = list(itertools.product((True, False), (0.5, 0.0), (0.1, 0.0), (0.1, 0.0), (1, 2)))   # training, dropout, cell, zone, r


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    got = PR.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]


def test_known_answers_vectorised():
    """The three vectors as ONE call on arrays: the same words (the reference is used on arrays of counters)."""
    args = [np.array([k[0][j] for k in KAT], dtype=np.uint64) for j in range(4)] + \
           [np.array([k[1][j] for k in KAT], dtype=np.uint64) for j in range(2)]
    got = PR.philox4x32_10(*args)
    for j in range(4):
        assert got[j].dtype == np.uint64 and got[j].tolist() == [k[2][j] for k in KAT]


def test_words_follow_the_counter_convention():
    """Element e = 4 i + j is word j of counter (i, 0, stream lo, stream hi) under key (seed lo, seed hi): spelled out per element on
    scalars; both high halves reach the generator; the zero stream starts with the published zero vector."""
    seed, sid = (0x1234 << 32) | 0x9, (0xABCD << 32) | 0x3
    w = PR.words(11, seed, sid)
    for e in range(11):
        one = PR.philox4x32_10(e // 4, 0, 0x3, 0xABCD, 0x9, 0x1234)
        assert int(w[e]) == int(one[e % 4]), e
    assert [int(x) for x in PR.words(4, 0, 0)] == list(KAT[0][2])
    assert not np.array_equal(PR.words(64, seed, sid), PR.words(64, 0x9, sid))
    assert not np.array_equal(PR.words(64, seed, sid), PR.words(64, seed, 0x3))
    assert np.array_equal(PR.words(7, 5, 6), PR.words(64, 5, 6)[:7])          # n only cuts the tail


def test_uniform24_is_exact_and_half_open():
    u = PR.uniform24(np.array([0, 0xFF, 0x100, 0xFFFFFFFF, 0x80000000], dtype=np.uint64))
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9, 0.1234])
def test_mask_and_bernoulli_share_one_convention(p):
    n = 4099
    m, z, under = PR.mask(n, p, 1234, 7), PR.bernoulli(n, p, 1234, 7), PR.under(n, p, 1234, 7)
    assert m.dtype == z.dtype == np.float32
    assert np.array_equal(m == 0.0, under) and np.array_equal(z == 1.0, under)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert set(np.unique(m).tolist()) == {0.0, float(keep)} and set(np.unique(z).tolist()) == {0.0, 1.0}
    assert abs(float(under.mean()) - p) < 5.0 * (p * (1 - p) / n) ** 0.5


def test_rates_zero_and_one_give_the_constants():
    n = 1027
    assert np.array_equal(PR.mask(n, 0.0, 3, 4), np.ones(n, np.float32))
    assert np.array_equal(PR.bernoulli(n, 0.0, 3, 4), np.zeros(n, np.float32))
    assert np.array_equal(PR.bernoulli(n, 1.0, 3, 4), np.ones(n, np.float32))


def test_a_tie_is_kept():
    """p = k / 2^24 with k the top 24 bits of an element's word: u == p there, and u < p is false - kept / not zoned; one step up
    it falls."""
    w = PR.words(8, 1234, 7)
    k = int(w[5]) >> 8
    assert 0 < k < 2 ** 24 - 1
    p, p_up = k / 2.0 ** 24, (k + 1) / 2.0 ** 24
    assert float(np.float32(p)) == p and float(np.float32(p_up)) == p_up
    assert PR.mask(8, p, 1234, 7)[5] > 0.0 and PR.bernoulli(8, p, 1234, 7)[5] == 0.0
    assert PR.mask(8, p_up, 1234, 7)[5] == 0.0 and PR.bernoulli(8, p_up, 1234, 7)[5] == 1.0


def _plan(training, dropout, cell, zone, r, step, B=3, L=7, T=9):
    return PR.engine_stream_ids(dict(SMALL, dropout=dropout), B, L, T, training, step, r=r, cell_dropout=cell, zoneout=zone)


def test_stream_ids_of_a_step_are_distinct_and_stay_inside_its_64():
    """Steps 0..3, every option combination: the ids of one step are pairwise distinct and lie in [64 step, 64 step + 64), so no id
    of step s is one of step s + 1 (checked as well); dropout ids stay below the zone ids 48..51; with everything on a step uses
    12 + 4 ids."""
    for training, dropout, cell, zone, r in OPTIONS:
        seen = set()
        for step in range(4):
            plan = _plan(training, dropout, cell, zone, r, step)
            ids = [sid for *_, sid in plan]
            assert len(set(ids)) == len(ids), (training, dropout, cell, zone, r, step)
            assert all(0 <= sid - 64 * step < 64 for sid in ids)
            assert not (seen & set(ids))
            seen |= set(ids)
            for name, n, rate, sid in plan:
                zoned = name in PR.ZONE_KEYS
                assert (sid - 64 * step >= PR.ZONE_BASE) == zoned and n > 0 and 0.0 < rate < 1.0
                assert rate == (zone if zoned else cell if name in ("att_drop", "dec_drop") else dropout)
    full = _plan(True, 0.5, 0.1, 0.1, 1, 2)
    assert [sid - 128 for *_, sid in full] == list(range(12)) + [48, 49, 50, 51]
    assert [name for name, *_ in full] == ["prenet_drop.0", "prenet_drop.1", "enc_drop.0", "enc_drop.1", "enc_drop.2"] + \
        [f"post_drop.{i}" for i in range(5)] + ["att_drop", "dec_drop"] + list(PR.ZONE_KEYS)
    # eval: the prenet masks alone (AlwaysDropout), no stream for the zone blocks
    assert [name for name, *_ in _plan(False, 0.5, 0.1, 0.1, 1, 0)] == ["prenet_drop.0", "prenet_drop.1"]
    assert _plan(False, 0.0, 0.1, 0.1, 1, 0) == []
    # without dropout the cell masks move up to the step's first ids; the zone ids do not move
    assert [(n, s) for n, _, _, s in _plan(True, 0.0, 0.1, 0.1, 1, 1)] == [("att_drop", 64), ("dec_drop", 65)] + \
        [(k, 64 + 48 + i) for i, k in enumerate(PR.ZONE_KEYS)]


def test_element_counts_follow_the_reduction_factor():
    """r = 2, T = 9 frames: decoder-side masks have ceil(9 / 2) = 5 steps (the prenet's one more), the postnet's 9 frames."""
    B, L, T = 3, 7, 9
    n = {name: cnt for name, cnt, _, _ in _plan(True, 0.5, 0.1, 0.1, 2, 0, B, L, T)}
    assert n["prenet_drop.0"] == n["prenet_drop.1"] == 6 * B * 16 and n["enc_drop.2"] == B * L * 32
    assert n["post_drop.0"] == B * T * 24 and n["post_drop.4"] == B * T * 20
    assert n["att_drop"] == n["att_zone_h"] == n["att_zone_c"] == 5 * B * 48 and n["dec_drop"] == n["dec_zone_c"] == 5 * B * 64
    n1 = {name: cnt for name, cnt, _, _ in _plan(True, 0.5, 0.1, 0.1, 1, 0, B, L, T)}
    assert n1["prenet_drop.0"] == 10 * B * 16 and n1["att_drop"] == 9 * B * 48 and n1["post_drop.0"] == n["post_drop.0"]


def test_decode_ids_are_distinct():
    """1000 + t0 + 100003 g over t0 < 4096 and g < 4 (a call decodes at most 64 groups, but 100003 > 4096 + 1000 settles every g)."""
    ids = {PR.decode_stream_id(t0, g) for t0 in range(4096) for g in range(4)}
    assert len(ids) == 4 * 4096
    assert PR.decode_stream_id(0, 0) == 1000 and PR.decode_stream_id(32, 1) == 101035


@pytest.mark.parametrize("training,dropout,cell,zone,r", OPTIONS)
def test_plan_is_what_make_masks_passes_to_the_library(monkeypatch, training, dropout, cell, zone, r):
    """Engine.make_masks on a CPU engine with the library call recorded instead of made: kernel, element count, rate, seed and
    stream id of every call, in order, are engine_stream_ids; every mask has the restatement's shape."""
    import torch
    from oracle import tacotron2_ref as R
    from tacotron2_amd import engine as E
    from tacotron2_amd.params import ParamStore
    d = R.default_dims(num_chars=39, att_dim=16, reduction_factor=r, cell_dropout=cell, zoneout=zone, **dict(SMALL, dropout=dropout))
    eng = E.Engine(ParamStore(d, torch.device("cpu")))
    calls = []
    monkeypatch.setattr(E, "call", lambda name, out, n, p, seed, sid, st: calls.append((name, n, p, seed, sid)))
    monkeypatch.setattr(E, "_stream", lambda: None)
    B, L, T, step, seed = 3, 7, 9, 3, 1234 + PR.RANK_SEED_STRIDE
    masks = eng.make_masks(B, L, T, training, seed, step)
    plan = PR.engine_stream_ids(d, B, L, T, training, step, r=r, cell_dropout=cell, zoneout=zone)
    want = [("t2_philox_bernoulli" if name in PR.ZONE_KEYS else "t2_philox_mask", n, rate, seed, sid) for name, n, rate, sid in plan]
    assert calls == want
    shapes = PR.engine_mask_shapes(d, B, L, T, r)
    got = {}
    for key, v in masks.items():
        got.update({f"{key}.{i}": t for i, t in enumerate(v)} if isinstance(v, list) else {key: v})
    if not training and zone > 0.0:      # eval: one constant block of the rate per cell, no stream
        for cell_, H in (("att", 48), ("dec", 64)):
            for s in "hc":
                blk = got.pop(f"{cell_}_zone_{s}")
                assert blk.shape == (1, B, H) and bool((blk == zone).all())
    assert set(got) == {name for name, *_ in plan}
    for name, t in got.items():
        assert tuple(t.shape) == shapes[name], name
