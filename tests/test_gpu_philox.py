"""t2_philox_mask and t2_philox_bernoulli (csrc/t2_elementwise.hip) called through the C ABI, and the masks Engine.make_masks and
Engine.infer hand out, compared BIT FOR BIT (torch.equal on the float tensors) with tests/philox_ref.py - which
tests/test_philox_host.py pins to the published Philox4x32-10 vectors.  Every output buffer has a NaN-filled tail of 8 elements
behind n that must still be NaN afterwards.

Sizes: 1 .. 5 (partial counters), 1023 / 1025 (around a block of 256 threads x 4 elements), 2^20, and 4 * 1048576 + 4 * 257 + 3,
above the grid cap of 4096 blocks x 256 threads x 4 elements: every thread takes a second counter, 257 a third element block, the
last counter is partial.  Seeds and stream ids with bits in both halves of the 64-bit words.  Rates 0, 0.1, 0.5, 0.9 (and 1 for the
zone masks), and a rate k / 2^24 that an element's uniform hits exactly: the tie is kept / not zoned.

The keep value 1 / (1 - p) is compared as numpy's float32 quotient (correctly rounded); test_keep_value_is_the_rounded_quotient holds
the device division to it over 64 rates.  No deviation was found on the MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tacotron2_ref as R  # noqa: E402
from tests import philox_ref as PR  # noqa: E402
from tests import reduction_ref as RR  # noqa: E402
from tests.test_gpu_reduction_factor import MID  # noqa: E402

TAIL = 8
SMALL_N = (1, 2, 3, 4, 5, 1023, 1025)
BIG_N = (1 << 20, 4 * 1048576 + 4 * 257 + 3)
SEEDS = ((0, 0), (1234, 7), (2 ** 32 + 5, 3), (9, 2 ** 32 + 3), (2 ** 63 + 11, 2 ** 64 - 1))
RATES = {"t2_philox_mask": (0.0, 0.1, 0.5, 0.9), "t2_philox_bernoulli": (0.0, 0.1, 0.5, 0.9, 1.0)}
KERNELS = tuple(RATES)
REF = {"t2_philox_mask": PR.mask, "t2_philox_bernoulli": PR.bernoulli}
ZERO_VECTOR = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)      # Philox4x32-10 of counter 0, key 0 (Random123 kat_vectors)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(dev, kernel, n, p, seed, sid):
    """One call on a NaN-filled buffer of n + TAIL elements -> the first n elements (CPU); the tail must still be NaN."""
    from tacotron2_amd import _lib
    out = torch.full((n + TAIL,), float("nan"), device=dev)
    _lib.call(kernel, out, n, float(p), seed, sid, _st())
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(torch.isnan(out[n:]).all()), f"{kernel} n={n}: wrote behind n"
    return out[:n]


def _check(dev, kernel, n, p, seed, sid):
    got = _gen(dev, kernel, n, p, seed, sid)
    ref = torch.from_numpy(REF[kernel](n, p, seed, sid))
    if not torch.equal(got, ref):
        bad = torch.nonzero(got != ref).flatten()
        e = int(bad[0])
        raise AssertionError(f"{kernel} n={n} p={p!r} seed={seed} stream={sid}: {bad.numel()} elements differ, first {e}: got "
                             f"{float(got[e])!r} ({got[e].view(torch.int32).item():#010x}), reference {float(ref[e])!r} "
                             f"({ref[e].view(torch.int32).item():#010x})")
    return got


def _tie_rates(seed, sid, e=5):
    """(k / 2^24, (k + 1) / 2^24) for k the 24 bits of element e's word: both exact in float32, u == p at the first."""
    k = int(PR.words(8, seed, sid)[e]) >> 8
    assert 0 < k < 2 ** 24 - 1
    return k / 2.0 ** 24, (k + 1) / 2.0 ** 24


@pytest.mark.parametrize("seed,sid", SEEDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_small_sizes_match_the_reference_bit_for_bit(dev, kernel, seed, sid):
    for n in SMALL_N:
        for p in RATES[kernel] + _tie_rates(seed, sid):
            _check(dev, kernel, n, p, seed, sid)


@pytest.mark.parametrize("n", BIG_N)
@pytest.mark.parametrize("kernel", KERNELS)
def test_large_sizes_match_the_reference_bit_for_bit(dev, kernel, n):
    """2^20: every seed at p = 0.5.  Above the grid cap: two seeds (one with all four halves in use), every rate."""
    if n == BIG_N[0]:
        for seed, sid in SEEDS:
            _check(dev, kernel, n, 0.5, seed, sid)
    for seed, sid in (SEEDS[1], SEEDS[4]):
        for p in RATES[kernel]:
            got = _check(dev, kernel, n, p, seed, sid)
            if 0.0 < p < 1.0:
                share = float((got == 0).double().mean())
                want = p if kernel == "t2_philox_mask" else 1.0 - p
                assert abs(share - want) < 5.0 * (p * (1 - p) / n) ** 0.5


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_tie_is_kept(dev, kernel):
    """p = k / 2^24 with k the top 24 bits of element 5's word: u == p, and u < p is false - the element is kept (mask) / not zoned
    (bernoulli); at (k + 1) / 2^24 it falls."""
    seed, sid = SEEDS[1]
    p, p_up = _tie_rates(seed, sid)
    at, above = _check(dev, kernel, 1025, p, seed, sid), _check(dev, kernel, 1025, p_up, seed, sid)
    if kernel == "t2_philox_mask":
        assert float(at[5]) == float(PR.keep_scale(p)) and float(above[5]) == 0.0
    else:
        assert float(at[5]) == 0.0 and float(above[5]) == 1.0


def test_high_halves_of_seed_and_stream_arrive(dev):
    """The 64-bit words travel through ctypes whole and the kernel uses both halves: (2^32 + 5, 3) is not (5, 3), (9, 2^32 + 3) is
    not (9, 3) - and each is the reference's draw."""
    n = 4099
    for (seed, sid), (lo_seed, lo_sid) in (((2 ** 32 + 5, 3), (5, 3)), ((9, 2 ** 32 + 3), (9, 3)), ((2 ** 63 + 11, 2 ** 64 - 1), (11, 2 ** 32 - 1))):
        for kernel in KERNELS:
            a, b = _check(dev, kernel, n, 0.5, seed, sid), _check(dev, kernel, n, 0.5, lo_seed, lo_sid)
            assert float((a != b).float().mean()) > 0.4


def test_published_zero_vector_through_the_kernel(dev):
    """seed = 0, stream = 0: elements 0..3 are the words of the published vector 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  For each
    element t2_philox_bernoulli with n = 4 at p = (w >> 8) / 2^24 gives 0 (u == p) and at ((w >> 8) + 1) / 2^24 gives 1: both rates are
    exact in float32, so the top 24 bits of every word of the known answer are pinned on the device."""
    for e, w in enumerate(ZERO_VECTOR):
        k = w >> 8
        lo, hi = k / 2.0 ** 24, (k + 1) / 2.0 ** 24
        assert float(np.float32(lo)) == lo and float(np.float32(hi)) == hi
        at, above = _gen(dev, "t2_philox_bernoulli", 4, lo, 0, 0), _gen(dev, "t2_philox_bernoulli", 4, hi, 0, 0)
        assert float(at[e]) == 0.0 and float(above[e]) == 1.0, (e, hex(w), at.tolist(), above.tolist())
        # and the other elements are what their own words say
        want = [1.0 if (x >> 8) < k else 0.0 for x in ZERO_VECTOR]
        assert at.tolist() == want


def test_keep_value_is_the_rounded_quotient(dev):
    """1 / (1 - p) on the device against numpy's float32 quotient (IEEE, correctly rounded) over 64 rates, bit for bit."""
    worst = []
    for i in range(64):
        p = float(np.float32((i + 0.37) / 65.0))
        got = _gen(dev, "t2_philox_mask", 1024, p, 3, i)
        kept = got[got != 0]
        assert kept.numel() > 0 and bool((kept == kept[0]).all())
        want = PR.keep_scale(p)
        if float(kept[0]) != float(want):
            worst.append((p, kept[0].view(torch.int32).item(), int(np.float32(want).view(np.int32))))
    assert not worst, "keep value differs from the float32 quotient (p, device bits, numpy bits): " + \
        ", ".join(f"({p!r}, {a:#010x}, {b:#010x})" for p, a, b in worst)


def test_argument_errors_launch_nothing(dev):
    """p < 0, p >= 1 (mask), p > 1 (bernoulli), a NaN rate, a NULL output and n < 0 are T2_ERR_ARG before any launch: the buffer keeps
    its sentinel.  n = 0 is T2_OK and writes nothing."""
    from tacotron2_amd import _lib
    buf = torch.full((64,), float("nan"), device=dev)
    bad = [("t2_philox_mask", buf, 8, -0.1), ("t2_philox_mask", buf, 8, 1.0), ("t2_philox_mask", buf, 8, float("nan")),
           ("t2_philox_mask", None, 8, 0.5), ("t2_philox_mask", buf, -1, 0.5),
           ("t2_philox_bernoulli", buf, 8, -0.1), ("t2_philox_bernoulli", buf, 8, 1.5), ("t2_philox_bernoulli", buf, 8, float("nan")),
           ("t2_philox_bernoulli", None, 8, 0.5), ("t2_philox_bernoulli", buf, -1, 0.5)]
    for kernel, out, n, p in bad:
        assert _lib.call_value(kernel, out, n, p, 1, 2, _st()) == 1, (kernel, n, p)          # T2_ERR_ARG
        assert "bad arguments" in _lib.lib().t2_last_error().decode()
    with pytest.raises(_lib.T2Error, match="rc=1"):
        _lib.call("t2_philox_mask", buf, 8, 1.0, 1, 2, _st())
    for kernel in KERNELS:
        assert _lib.call_value(kernel, buf, 0, 0.5, 1, 2, _st()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the engine's masks
# ---------------------------------------------------------------------------------------------------------------------------
_P = {}


def _params(r):
    if r not in _P:
        d = R.default_dims(**MID)
        _P[r] = RR.grouped_params(R.init_params(d, seed=9), d, r, seed=1)
    return _P[r]


def _flat(masks):
    out = {}
    for key, v in masks.items():
        out.update({f"{key}.{i}": t for i, t in enumerate(v)} if isinstance(v, list) else {key: v})
    return out


MASK_CASES = [   # dims on top of MID, training, step, seed
    (dict(), True, 0, 1234), (dict(), True, 3, 1234 + PR.RANK_SEED_STRIDE), (dict(), False, 3, 1234),
    (dict(dropout=0.0), True, 3, 1234), (dict(cell_dropout=0.0), True, 0, 1234),
    (dict(zoneout=0.1), True, 3, 1234), (dict(zoneout=0.1), False, 0, 1234 + PR.RANK_SEED_STRIDE),
    (dict(reduction_factor=2), True, 3, 1234), (dict(reduction_factor=2, zoneout=0.1), True, 0, 1234),
]


@pytest.mark.parametrize("over,training,step,seed", MASK_CASES)
def test_engine_masks_are_the_reference_under_the_id_plan(dev, over, training, step, seed):
    """Engine.make_masks at the mid-size dims: every tensor it returns equals philox_ref under (seed, id) of engine_stream_ids, in
    shape and bits; nothing else is returned (in eval with zoneout: the constant blocks of the rate)."""
    from tests.test_gpu_model import build_engine
    d = dict(R.default_dims(**MID), **over)
    r = d.get("reduction_factor", 1)
    eng, ps = build_engine(d, _params(r), dev)
    B, L, T = 3, 7, 9
    got = _flat(eng.make_masks(B, L, T, training, seed, step))
    torch.cuda.synchronize()
    cell, zone = d.get("cell_dropout", 0.1), d.get("zoneout", 0.0)
    plan = PR.engine_stream_ids(d, B, L, T, training, step, r=r, cell_dropout=cell, zoneout=zone)
    shapes = PR.engine_mask_shapes(d, B, L, T, r)
    if not training and zone > 0.0:
        for c, H in (("att", d["att_rnn_dim"]), ("dec", d["rnn_hidden_dim"])):
            for s in "hc":
                blk = got.pop(f"{c}_zone_{s}")
                assert blk.shape == (1, B, H) and bool((blk == zone).all())
    assert list(got) == [name for name, *_ in plan]
    for name, n, rate, sid in plan:
        t = got[name].cpu()
        assert tuple(t.shape) == shapes[name] and t.is_contiguous() and t.numel() == n, name
        ref = (PR.bernoulli if name in PR.ZONE_KEYS else PR.mask)(n, rate, seed, sid)
        assert torch.equal(t.reshape(-1), torch.from_numpy(ref)), (name, sid)
        assert sid // 64 == step


def test_decode_prenet_masks_are_the_reference_under_the_decode_ids(dev):
    """Engine.infer with device-generated prenet masks, 66 utterances = two groups (64 + 2), 5 steps in chunks of 2: the mask
    workspace of each group (inf<g>.pmask, [Tcap][2][Bg][P], NaN-filled before the call) holds, chunk by chunk, the reference under
    stream 1000 + t0 + 100003 g.  The stop bias keeps every utterance running, so all three chunks are generated."""
    from tests.test_gpu_model import build_engine
    d = R.default_dims(**MID)
    P = dict(_params(1))
    P["decoder.gate.bias"] = P["decoder.gate.bias"] + 50.0
    eng, ps = build_engine(d, P, dev)
    B, L, cap, every, seed = 66, 6, 5, 2, 77
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(3, L + 1, (B,), generator=g); lens[0] = L
    ci = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    Pd = d["prenet_dim"]
    groups = [(0, 64), (1, 2)]
    for gi, Bg in groups:
        eng.buf(f"inf{gi}.pmask", cap, 2, Bg, Pd).fill_(float("nan"))
    mels, *_ = eng.infer(ci.to(dev), lens.to(dev), cap, seed=seed, check_every=every)
    torch.cuda.synchronize()
    assert mels.shape[1] == cap
    for gi, Bg in groups:
        pm = eng._ws[f"inf{gi}.pmask"][:cap * 2 * Bg * Pd].cpu().view(cap, -1)
        for t0 in range(0, cap, every):
            t1 = min(cap, t0 + every)
            ref = PR.mask((t1 - t0) * 2 * Bg * Pd, d["dropout"], seed, PR.decode_stream_id(t0, gi))
            assert torch.equal(pm[t0:t1].reshape(-1), torch.from_numpy(ref)), (gi, t0)
