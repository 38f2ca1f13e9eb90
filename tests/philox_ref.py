"""Bit-exact reference of the device mask generators t2_philox_mask / t2_philox_bernoulli (csrc/t2_elementwise.hip) and of the
stream-id plan of Engine.make_masks / Engine.infer: numpy only, no torch, importable without a GPU.  tests/test_philox_host.py pins
the generator to the published Random123 vectors and the id plan to its invariants, tests/test_gpu_philox.py holds the kernels and
the engine to this module bit for bit.  This is the definition a future in-kernel generator has to reproduce ("Random
streams").

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written from the paper's round:
    one round:  (c0, c1, c2, c3), (k0, k1)  ->  (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))
    M0 = 0xD2511F53, M1 = 0xCD9E8D57; ten rounds, the key raised by (0x9E3779B9, 0xBB67AE85) mod 2^32 BETWEEN rounds (round k runs
    under key + k * increment, k = 0..9).
The masks' convention on top of it:
    counter i = e // 4 for element e:  (i & 0xffffffff, i >> 32, stream_id & 0xffffffff, stream_id >> 32);  key (seed & 0xffffffff,
    seed >> 32);  element e = 4 i + j takes output word j;  u = (word >> 8) * 2^-24, exact in float32, in [0, 1).
    mask:       0 where u < float32(p), else float32(1) / (float32(1) - float32(p))  (a float32 quotient, correctly rounded)
    bernoulli:  1 where u < float32(p), else 0
so a tie u == p is kept (mask) / not zoned (bernoulli), p = 0 gives the constant 1 / 0 and bernoulli's p = 1 the constant 1."""
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
ROUNDS = 10
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint64 arrays (values < 2^32) of output words; every argument a 32-bit value or an array of them (broadcast)."""
    c0, c1, c2, c3, k0, k1 = (_u64(x) & _LO for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(ROUNDS):
        p0 = np.uint64(M0) * c0                 # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0 = (k0 + np.uint64(W0)) & _LO
        k1 = (k1 + np.uint64(W1)) & _LO
    return c0, c1, c2, c3


def uniform24(words):
    """(w >> 8) * 2^-24 as float32 - 24 bits, so the product is exact."""
    return ((_u64(words) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


@functools.lru_cache(maxsize=8)
def words(n, seed, stream_id):
    """The n 32-bit words of (seed, stream_id) in element order (uint64 array; cached, read-only)."""
    seed, stream_id = int(seed), int(stream_id)
    assert n >= 0 and 0 <= seed < 2 ** 64 and 0 <= stream_id < 2 ** 64
    i = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10(i & _LO, i >> _32, stream_id & 0xFFFFFFFF, stream_id >> 32, seed & 0xFFFFFFFF, seed >> 32)
    out = np.stack(w, axis=1).reshape(-1)[:n]
    out.setflags(write=False)
    return out


def keep_scale(p):
    """float32(1) / (float32(1) - float32(p)): numpy's float32 division is IEEE, correctly rounded."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def under(n, p, seed, stream_id):
    """bool [n]: u < float32(p) - the elements t2_philox_mask drops and t2_philox_bernoulli zones."""
    return uniform24(words(n, seed, stream_id)) < np.float32(p)


def mask(n, p, seed, stream_id):
    assert 0.0 <= p < 1.0
    return np.where(under(n, p, seed, stream_id), np.float32(0.0), keep_scale(p)).astype(np.float32)


def bernoulli(n, p, seed, stream_id):
    assert 0.0 <= p <= 1.0
    return np.where(under(n, p, seed, stream_id), np.float32(1.0), np.float32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# The id plan.  A training / teacher-forced step owns the 64 ids step * 64 .. step * 64 + 63.  The dropout masks take them from
# step * 64 upwards IN THE ORDER BELOW, and a site that is switched off takes none (its successors move up); the four zone masks
# sit at the fixed ids step * 64 + 48 .. 51, so that switching zoneout on does not change a dropout mask.
# ---------------------------------------------------------------------------------------------------------------------------
IDS_PER_STEP = 64
ZONE_BASE = 48
RANK_SEED_STRIDE = 7919        # rank k of a data-parallel run draws under seed + 7919 k (Trainer.train_step)
ZONE_KEYS = ("att_zone_h", "att_zone_c", "dec_zone_h", "dec_zone_c")


def engine_mask_shapes(d, B, L, T, r=1):
    """name -> shape of every mask Engine.make_masks can hand out; T in frames, S = ceil(T / r) decoder steps."""
    E, Pd, A, D, M, Pn = (d[k] for k in ("encoded_dim", "prenet_dim", "att_rnn_dim", "rnn_hidden_dim", "num_mels", "postnet_dim"))
    S = (T + r - 1) // r
    s = {f"prenet_drop.{i}": (S + 1, B, Pd) for i in range(2)}
    s.update({f"enc_drop.{i}": (B, L, E) for i in range(3)})
    s.update({f"post_drop.{i}": (B, T, c) for i, c in enumerate((Pn, Pn, Pn, Pn, M))})     # the postnet runs per frame
    s["att_drop"], s["dec_drop"] = (S, B, A), (S, B, D)
    s.update({k: (S, B, A if k.startswith("att") else D) for k in ZONE_KEYS})
    return s


def engine_stream_ids(d, B, L, T, training, step, r=1, cell_dropout=0.1, zoneout=0.0):
    """[(mask name, element count, rate, stream id)] in the order Engine.make_masks generates them: prenet x 2 (always, the
    reference's AlwaysDropout), then in training enc x 3, post x 5 (rate d["dropout"], all of these only when it is > 0), att, dec
    (rate cell_dropout, when > 0), and with zoneout > 0 in training the four Bernoulli zone masks.  (In eval the zone masks are
    constant blocks of the rate: no stream.)"""
    shp = engine_mask_shapes(d, B, L, T, r)
    p = float(d["dropout"])
    names = []
    if p > 0.0:
        names += [(f"prenet_drop.{i}", p) for i in range(2)]
    if training:
        if p > 0.0:
            names += [(f"enc_drop.{i}", p) for i in range(3)] + [(f"post_drop.{i}", p) for i in range(5)]
        if cell_dropout > 0.0:
            names += [("att_drop", float(cell_dropout)), ("dec_drop", float(cell_dropout))]
    out = [(name, int(np.prod(shp[name])), rate, step * IDS_PER_STEP + k) for k, (name, rate) in enumerate(names)]
    if training and zoneout > 0.0:
        out += [(key, int(np.prod(shp[key])), float(zoneout), step * IDS_PER_STEP + ZONE_BASE + i) for i, key in enumerate(ZONE_KEYS)]
    return out


def decode_stream_id(t0, group):
    """Engine.infer: the prenet masks of the chunk of decoder steps that starts at step t0, group `group` of 64 utterances."""
    return 1000 + t0 + 100003 * group
