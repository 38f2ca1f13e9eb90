"""t2_join / analysis.join_audio on the GPU against tests/join_ref.py.

Every case draws its inputs with a fixed seed and asserts IN THE REFERENCE, before the device is touched, that every frame energy
is further than 1e-9 (relative) from the activity threshold: a direct fp64 sum of at most F = 2048 non-negative terms is within
2048 * 2^-53 = 2.3e-13 of any other order of summation, so the kernel's order cannot flip a frame and s0, len, off and total must
be EQUAL.  The gains come from fp64 sums that may differ in their last bits and one cast: one float32 ulp.  y is then x * (gain *
e) in numpy float32 from the device's own gains, bit for bit.  The rows are NaN behind n[b] and in the padding up to ldx."""
import ctypes as C

import numpy as np
import pytest
import torch

import join_ref as R

pytestmark = pytest.mark.gpu
F, H = 2048, 512
DEV = "cuda:0"


def _rows(specs, seed, n_max=None):
    """specs: (n, a, b, amp) per row - n samples, noise of RMS amp in [a, b), exact zeros around it.  (x (B, n_max), n)."""
    rng = np.random.default_rng(seed)
    n = [s[0] for s in specs]
    x = np.zeros((len(specs), max(max(n), 1) if n_max is None else n_max), np.float32)
    for r, (_, a, b, amp) in enumerate(specs):
        x[r, a:b] = (amp * rng.standard_normal(b - a)).astype(np.float32)
    return x, n


def _poison(x, n, extra=5):
    """The device's copy: NaN behind every n[b] and in `extra` columns of padding; returned as the (B, n_max) view of it."""
    big = np.full((x.shape[0], x.shape[1] + extra), np.nan, np.float32)
    for b in range(len(n)):
        big[b, :n[b]] = x[b, :n[b]]
    return torch.from_numpy(big).to(DEV)[:, :x.shape[1]]


def _join(wav, n, pause, **kw):
    from tacotron2_amd import analysis
    kw = dict(kw)
    kw["frame_length"], kw["hop_length"] = kw.pop("F", F), kw.pop("H", H)
    y, total, plan = analysis.join_audio(wav, n, pause, **kw)
    return y.cpu().numpy(), total, {k: v.cpu().numpy() for k, v in plan.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(x, n, pause, extra=5, **kw):
    ref = R.join_ref(x, n, pause, **kw)
    assert (ref["margin"] > 1e-9).all(), ref["margin"]               # (before the device: the inputs alone meet the condition)
    y, total, plan = _join(_poison(x, n, extra), n, pause, **kw)
    assert total == ref["total"] == len(y)
    for k in ("s0", "len", "off"):
        assert plan[k].dtype == ref[k].dtype and np.array_equal(plan[k], ref[k]), (k, plan[k], ref[k])
    ulp = np.spacing(np.maximum(np.abs(plan["gain"]), np.abs(ref["gain"])))
    assert plan["gain"].dtype == np.float32 and (np.abs(plan["gain"] - ref["gain"]) <= ulp).all(), (plan["gain"], ref["gain"])
    want = R.write_ref(x, plan["s0"], plan["len"], plan["off"], plan["gain"], pause, total, kw.get("fade", 0))
    assert not np.isnan(y).any() and not np.isnan(want).any()
    assert np.array_equal(_bits(y), _bits(want))
    for b in range(len(n)):                                          # (the pauses: exactly +0.0)
        p0 = int(plan["off"][b]) + int(plan["len"][b])
        assert not _bits(y[p0:p0 + pause[b]]).any()
    return ref, y, plan


def test_one_empty_row():
    x = np.zeros((1, 16), np.float32)
    for pause in (0, 5):
        ref, y, plan = check(x, [0], [pause])
        assert len(y) == pause and plan["len"].tolist() == [0]
    from tacotron2_amd import analysis
    y, total, _ = analysis.join_audio(torch.zeros(1, 0, device=DEV), [0], [3])          # (a batch without a column)
    assert total == 3 and y.tolist() == [0.0, 0.0, 0.0]


def test_rows_of_f_minus_1_and_f_samples():
    x, n = _rows([(F - 1, 500, 900, 0.1), (F, 600, 1500, 0.1)], 1)
    ref, _, _ = check(x, n, [10, 0])
    assert ref["len"][0] == F - 1 and 0 < ref["len"][1] <= F          # the short row is kept whole, the other one is framed


def test_5000_samples_with_silence_at_both_ends_one_end_or_none():
    x, n = _rows([(5000, 1300, 3100, 0.1), (5000, 0, 2500, 0.1), (5000, 2700, 5000, 0.1), (5000, 0, 5000, 0.1)], 2)
    ref, _, _ = check(x, n, [3, 0, 9, 0])
    assert ref["s0"].tolist()[1] == 0 and ref["s0"][0] > 0 and ref["s0"][2] > 0 and ref["len"].tolist()[3] == 5000
    assert ref["len"][0] < 5000 and ref["s0"][2] + ref["len"][2] == 5000


def test_an_all_zero_row_between_two_live_ones():
    x, n = _rows([(6000, 1000, 4000, 0.1), (7000, 0, 0, 0.0), (5000, 500, 4500, 0.1)], 3)
    ref, y, plan = check(x, n, [100, 250, 0], fade=110)
    assert plan["len"].tolist()[1] == 0 and plan["off"][2] - plan["off"][1] == 250          # its pause alone
    x[1, 3000:3100] = np.float32(1e-5) * np.random.default_rng(4).standard_normal(100).astype(np.float32)     # -80 dB beside zeros:
    assert check(x, n, [100, 250, 0])[0]["len"][1] > 0                                      # the row's OWN peak is the ruler


def test_pauses_0_1_700():
    x, n = _rows([(4000, 300, 3000, 0.1), (3000, 1000, 2000, 0.1), (2500, 0, 2500, 0.1)], 5)
    ref, y, plan = check(x, n, [0, 1, 700], fade=64)
    assert ref["total"] == int(ref["len"].sum()) + 701


def test_70_rows_of_random_lengths():
    rng = np.random.default_rng(6)
    specs = []
    for _ in range(70):
        n = int(rng.integers(0, 9001))
        a = int(rng.integers(0, n + 1))
        specs.append((n, a, int(rng.integers(a, n + 1)), 0.1 * 10 ** float(rng.uniform(-1, 0))))
    specs[7], specs[8], specs[9] = (0, 0, 0, 0.0), (9000, 0, 9000, 0.1), (5000, 0, 0, 0.0)
    x, n = _rows(specs, 7)
    pause = [int(p) for p in rng.integers(0, 600, 70)]
    ref, _, _ = check(x, n, pause, fade=110, keep=441)
    check(x, n, pause, fade=110, keep=441, level=True, ceiling=0.25)
    assert (ref["len"] == 0).sum() >= 2 and (ref["len"] > 0).sum() > 50


def test_kept_lengths_around_the_chunk_sizes():
    lens = [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
    x, n = _rows([(k, 0, k, 0.1) for k in lens], 8)
    ref, _, _ = check(x, n, [0, 1, 0, 2, 0, 3, 0, 4, 0], trim=False, fade=110)
    assert ref["len"].tolist() == lens


@pytest.mark.parametrize("fade", [0, 110])
def test_fades_on_short_pieces(fade):
    lens = [1, 2, 219, 220, 221]
    x, n = _rows([(k, 0, k, 0.1) for k in lens], 9)
    x[:] = np.abs(x) + np.float32(0.01)
    ref, y, plan = check(x, n, [0, 0, 5, 0, 0], trim=False, fade=fade)
    if fade:
        w = R.fade_table(fade)
        assert y[0] == x[0, 0] and y[1] == x[1, 0] * w[55] and y[3] == x[2, 0] * w[(1 * 110) // 218]       # fl = 0, 1, 109
        o = int(plan["off"][3])
        assert y[o] == x[3, 0] * w[0] and y[o + 219] == x[3, 219] * w[0] and y[o + 109] == x[3, 109] * w[109]
    else:
        assert np.array_equal(y[:3], [x[0, 0], x[1, 0], x[1, 1]])


def test_level_clamps_a_row_12_db_down_and_one_12_db_up():
    down = 10 ** (-12 / 20)
    x, n = _rows([(6000, 500, 5500, 0.1), (6000, 500, 5500, 0.1), (6000, 500, 5500, 0.1), (6000, 500, 5500, 0.1 * down)], 10)
    ref, _, plan = check(x, n, [0, 0, 0, 0], level=True, max_gain=2.0)
    assert plan["gain"][3] == 2.0 and (plan["gain"][:3] < 1.0).all()                       # (it wants 3.5)
    x, n = _rows([(6000, 500, 5500, 0.1), (6000, 500, 5500, 0.1), (6000, 500, 5500, 0.1), (6000, 500, 5500, 0.1 / down)], 11)
    ref, _, plan = check(x, n, [0, 0, 0, 0], level=True, max_gain=2.0)
    assert plan["gain"][:3].tolist() == [2.0, 2.0, 2.0] and 0.5 < plan["gain"][3] < 1.0
    ref, _, plan = check(x, n, [0, 0, 0, 0], level=True, max_gain=1.25)
    assert np.array_equal(plan["gain"], np.float32([1.25, 1.25, 1.25, 0.8]))


def test_the_ceiling_engages_above_it_only():
    x, n = _rows([(6000, 500, 5500, 0.1), (6000, 500, 5500, 0.4)], 12)
    x[0] = np.clip(x[0], -0.5, 0.5)
    x[0, 3000] = 0.9                                                                        # peaks at 0.9 BEFORE its gain of about 2
    free = R.join_ref(x, n, [0, 0], level=True)
    assert (free["gain64"] * free["peak"]).max() > 1.0
    ref, y, plan = check(x, n, [0, 0], level=True, ceiling=1.0)
    assert (plan["gain"] < free["gain"]).all() and 1.0 - 1e-6 < np.abs(y).max() <= 1.0 + 2.0 ** -22          # (the cast and the product round once each)
    x, n = _rows([(6000, 500, 5500, 0.03), (6000, 500, 5500, 0.06)], 13)
    x[:] = np.clip(x, -0.2, 0.2)
    x[0, 3000] = 0.2
    free = R.join_ref(x, n, [0, 0], level=True)
    assert (free["gain64"] * free["peak"]).max() < 1.0
    ref, y, plan = check(x, n, [0, 0], level=True, ceiling=1.0)
    assert np.array_equal(plan["gain"], free["gain"]) or (np.abs(plan["gain"] - free["gain"]) <= np.spacing(free["gain"])).all()


@pytest.mark.parametrize("keep", [0, 441])
def test_keep_is_clamped_to_the_row(keep):
    x, n = _rows([(5000, 100, 4950, 0.1), (20000, 6000, 13000, 0.1)], 14)
    ref, _, plan = check(x, n, [0, 0], keep=keep)
    if keep:
        assert plan["s0"].tolist()[0] == 0 and plan["len"].tolist()[0] == 5000              # clamped at 0 and at n
        assert plan["s0"][1] == 10 * H - 441 and plan["s0"][1] + plan["len"][1] == 28 * H + 441
    else:
        assert plan["s0"][1] == 10 * H and plan["s0"][1] + plan["len"][1] == 28 * H


def test_a_strided_view_and_two_calls():
    x, n = _rows([(7000, 1000, 6000, 0.1), (3000, 0, 2000, 0.2), (6500, 3000, 6500, 0.05)], 15)
    ref, y, plan = check(x, n, [40, 0, 7], extra=37, fade=110, level=True, ceiling=0.5, keep=441)
    wav = _poison(x, n, 37)
    assert wav.stride(0) == x.shape[1] + 37 and not wav.is_contiguous()
    a = _join(wav, n, [40, 0, 7], fade=110, level=True, ceiling=0.5, keep=441)
    b = _join(wav, torch.tensor(n, device=DEV), torch.tensor([40, 0, 7], dtype=torch.int32, device=DEV), fade=110, level=True,
              ceiling=0.5, keep=441)                                                        # (device counts: the same launch)
    for got in (a, b):
        assert np.array_equal(_bits(got[0]), _bits(y)) and got[1] == ref["total"]
        assert all(np.array_equal(_bits(got[2][k]) if k == "gain" else got[2][k], _bits(plan[k]) if k == "gain" else plan[k]) for k in plan)


def test_rows_do_not_depend_on_the_batch_around_them():
    x3, n3 = _rows([(7000, 1000, 6000, 0.1), (2000, 100, 1500, 0.2), (6500, 3000, 6500, 0.05)], 16)
    x2, n2 = _rows([(9000, 0, 4000, 0.3), (8000, 5000, 8000, 0.02)], 17)
    x5 = np.zeros((5, 9000), np.float32)
    order = [(x2, 0), (x3, 0), (x3, 1), (x2, 1), (x3, 2)]
    for r, (src, i) in enumerate(order):
        x5[r, :src.shape[1]] = src[i]
    n5 = [n2[0], n3[0], n3[1], n2[1], n3[2]]
    _, y3, p3 = check(x3, n3, [5, 0, 9], fade=110, keep=100)
    _, y5, p5 = check(x5, n5, [1, 5, 0, 300, 9], extra=123, fade=110, keep=100)
    for i3, i5 in ((0, 1), (1, 2), (2, 4)):
        assert p3["s0"][i3] == p5["s0"][i5] and p3["len"][i3] == p5["len"][i5]
        a, b, k = int(p3["off"][i3]), int(p5["off"][i5]), int(p3["len"][i3])
        assert np.array_equal(_bits(y3[a:a + k]), _bits(y5[b:b + k]))


def test_a_device_count_out_of_range_refuses_the_batch_with_nothing_written():
    """The C entry itself: one n[b] of -1 or n_max + 1 gives total = -1 and y keeps its prefill (the batch is one document: no row of
    it is written); the same block with the row's own count writes what the wrapper writes."""
    from tacotron2_amd import _lib
    x, n = _rows([(7000, 1000, 6000, 0.1), (2000, 100, 1500, 0.2), (6500, 3000, 6500, 0.05)], 21)
    wav, pause, B, ld = _poison(x, n), [5, 0, 9], 3, x.shape[1]
    cap, lde = sum(n) + sum(pause), ld // H + 1
    want, total, _ = _join(wav, n, pause)

    def run(counts):
        t = lambda *shape, dtype: torch.empty(*shape, dtype=dtype, device=DEV)
        out = dict(total=torch.full((1,), 77, dtype=torch.int64, device=DEV), y=torch.full((cap,), -7.0, device=DEV))
        a = _lib.make("T2Join", x=wav, ldx=wav.stride(0), n=torch.tensor(counts, dtype=torch.int32, device=DEV),
                      pause=torch.tensor(pause, dtype=torch.int32, device=DEV), w=None, B=B, n_max=ld, trim=1, F=F, H=H, keep=0, fade=0,
                      level=0, top_db=60.0, max_gain=2.0, ceiling=0.0, energy=t(B, lde, dtype=torch.float64), lde=lde,
                      stat=t(B, 2, dtype=torch.float64), off=t(B, dtype=torch.int64), s0=t(B, dtype=torch.int32),
                      len=t(B, dtype=torch.int32), gain=t(B, dtype=torch.float32), cap=cap, **out)
        _lib.call("t2_join", a, _lib.stream())
        torch.cuda.synchronize()
        return int(out["total"].item()), out["y"].cpu().numpy()

    for bad in (-1, ld + 1):
        t, y = run([n[0], bad, n[2]])
        assert t == -1 and (y == -7.0).all(), (bad, t)
    t, y = run(n)
    assert t == total and np.array_equal(_bits(y[:t]), _bits(want))


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses_bad_arguments():
    from tacotron2_amd import analysis, engine
    assert engine.join_audio is analysis.join_audio
    wav = torch.zeros(2, 4096, device=DEV)
    ok = dict(n=[4096, 100], pause=[0, 0])

    def refused(match, wav=wav, **kw):
        with pytest.raises(ValueError, match=match):
            analysis.join_audio(wav, **{**ok, **kw})

    refused("wav must be a float32", wav=None)
    refused("wav must be a float32", wav=wav.double())
    refused("wav must be on the GPU", wav=wav.cpu())
    refused("batch of 0", wav=torch.zeros(0, 8, device=DEV), n=[], pause=[])
    refused("batch of 65536", wav=torch.zeros(65536, 1, device=DEV), n=[0] * 65536, pause=[0] * 65536)
    refused("last dimension of wav must be contiguous", wav=torch.zeros(2, 8192, device=DEV)[:, ::2])
    refused("overlapping rows", wav=torch.zeros(8192, device=DEV).as_strided((2, 4096), (100, 1)))
    for bad in (1, 0, -2048):
        refused("frame_length must be an integer >= 2", frame_length=bad)
    refused("frame_length must be even", frame_length=2047)
    refused("frame_length must be an integer", frame_length=2048.0)
    refused("hop_length must be an integer >= 1", hop_length=0)
    refused("keep must be an integer >= 0", keep=-1)
    refused("fade must be an integer >= 0", fade=-1)
    for bad in (-1.0, float("nan"), float("inf"), "60"):
        refused("top_db must be a finite number >= 0", top_db=bad)
    for bad in (0.99, 0.0, float("nan"), float("inf")):
        refused("max_gain must be", max_gain=bad)
    for bad in (-0.5, float("nan")):
        refused("ceiling must be a finite number >= 0", ceiling=bad)
    refused("trim must be a flag", trim=2)
    refused("level must be a flag", level=-1)
    refused("level must be a flag", level=1.0)
    refused("n must be 2 integers", n=[4096])
    refused("n must be 2 integers", n=[1.0, 2.0])
    refused("n must lie in 0 .. 4096", n=[4097, 0])
    refused("n must lie in 0 .. 4096", n=[-1, 0])
    refused("pause must lie in 0 ..", pause=[0, -1])
    refused("pause must be 2 integers", pause=[0, 0, 0])
    # counts on the device are the kernel's to refuse: no clamp, nothing read or written, one ValueError after the launch
    refused("refused on the device", n=torch.tensor([4097, 0], device=DEV))
    refused("refused on the device", n=torch.tensor([-1, 0], device=DEV))
    refused("refused on the device", pause=torch.tensor([0, -3], device=DEV))


def test_the_c_entry_returns_t2_err_arg():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    B, ld = 2, 4096
    t = dict(x=torch.zeros(B, ld, device=DEV), n=torch.zeros(B, dtype=torch.int32, device=DEV), pause=torch.zeros(B, dtype=torch.int32, device=DEV),
             w=torch.ones(8, device=DEV), energy=torch.zeros(B, ld // H + 1, dtype=torch.float64, device=DEV),
             stat=torch.zeros(B, 2, dtype=torch.float64, device=DEV), off=torch.zeros(B, dtype=torch.int64, device=DEV),
             s0=torch.zeros(B, dtype=torch.int32, device=DEV), len=torch.zeros(B, dtype=torch.int32, device=DEV),
             gain=torch.zeros(B, device=DEV), total=torch.full((1,), 77, dtype=torch.int64, device=DEV), y=torch.zeros(16, device=DEV))
    ok = dict(t, ldx=ld, B=B, n_max=ld, trim=1, F=F, H=H, keep=0, fade=8, level=0, top_db=60.0, max_gain=2.0, ceiling=0.0, lde=ld // H + 1, cap=16)
    stream = torch.cuda.current_stream().cuda_stream
    bad = [dict(F=2047), dict(F=0), dict(B=0), dict(B=65536), dict(H=0), dict(keep=-1), dict(fade=-1), dict(top_db=-1.0),
           dict(top_db=float("nan")), dict(top_db=float("inf")), dict(max_gain=0.5), dict(ceiling=-1.0), dict(ldx=ld - 1), dict(trim=2),
           dict(level=3), dict(w=None), dict(x=None), dict(n=None), dict(pause=None), dict(y=None), dict(total=None), dict(gain=None),
           dict(energy=None), dict(lde=ld // H), dict(cap=-1), dict(n_max=-1)]
    for kw in bad:
        a = _lib.make("T2Join", **{**ok, **kw})
        assert lib.t2_join(C.addressof(a), stream) == 1, kw                                  # T2_ERR_ARG, before any launch
        assert b"t2_join" in lib.t2_last_error()
    torch.cuda.synchronize()
    assert t["total"].item() == 77                                                           # nothing ran
    for kw in (dict(), dict(w=None, fade=0), dict(energy=None, trim=0), dict(y=None, cap=0)):
        assert lib.t2_join(C.addressof(_lib.make("T2Join", **{**ok, **kw})), stream) == 0, kw
    torch.cuda.synchronize()
    assert t["total"].item() == 0
