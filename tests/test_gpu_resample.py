"""t2_resample on the GPU through the C ABI against the float64 restatement tests/resample_ref.py, per output sample.

The bound is a-priori, from the restatement: |y_gpu[m] - y_ref[m]| <= (2K + 2) * 2^-24 * sum_k |h_k| |x_k| - the taps rounded to fp32
once, 2K fused multiply-adds in fp32, with room to spare; it is never taken from what the kernel gives.  Designs: toy tables of random
taps (U, D, K) = (3, 2, 2), (1, 2, 3), (2, 1, 1) - K odd takes the kernel's dword tap loads, K even its dwordx4 loads - plus (1, 17, 1)
and (1, 1, 8200), whose input span per block of 1024 outputs passes the 64 KB of LDS the kernel stages it in (its unstaged form),
and the real 24000, 44100, 16000 and 11025 -> 22050 (147 / 160, 1 / 2, 441 / 320, 2 / 1).  Every design runs ONE ragged batch whose
rows are the lengths that matter: n_in = 1, n_in < 2K, the n_in that give exactly one block of 1024 outputs and one output either
side, n_in U divisible by D and not; ldx and ldy differ from every length, NaN sits behind every row's n_in (a finite output proves
that nothing there was read), the output buffer is pre-filled and guarded."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
FILL = 123.0
TOYS = {"toy_3_2_2": (3, 2, 2), "toy_1_2_3": (1, 2, 3), "toy_2_1_1": (2, 1, 1), "toy_1_17_1": (1, 17, 1), "toy_1_1_8200": (1, 1, 8200)}
REAL = {"real_147_160": 24000, "real_1_2": 44100, "real_441_320": 16000, "real_2_1": 11025}


@functools.lru_cache(maxsize=None)
def design(name):
    """(U, D, K, float64 table of the restatement, fp32 table the kernel gets)."""
    if name in TOYS:
        U, D, K = TOYS[name]
        t32 = np.random.default_rng(U * 1000 + D * 10 + K).uniform(-1, 1, (U, 2 * K)).astype(np.float32)
        return U, D, K, t32.astype(np.float64), t32
    from tacotron2_amd.datasets.resample import plan
    U, D, K, ref = R.design(REAL[name], 22050)
    assert plan(REAL[name], 22050)[:3] == (U, D, K)
    return U, D, K, ref, plan(REAL[name], 22050)[3]


def n_in_for(n_out, U, D):
    """The smallest n_in with ceil(n_in U / D) >= n_out."""
    n = (n_out * D) // U - 2
    while R.out_len(max(n, 0), U, D) < n_out:
        n += 1
    return max(n, 1)


def lengths_for(U, D, K):
    if K > 1000:            # the 16 400-tap toy: every row is shorter than 2K, the longest one makes two blocks of outputs
        return [1, 300, 1100, 3 * D, 3 * D + 1]
    return [1, max(1, K), max(1, 2 * K - 1), 3 * D, 3 * D + 1,
            n_in_for(1023, U, D), n_in_for(1024, U, D), n_in_for(1025, U, D), n_in_for(2049, U, D) + 3]


def run(signals, U, D, K, t32, pad_x=37, pad_y=29, ldy=None):
    """One t2_resample call: rows of `signals`, row stride max n_in + pad_x with NaN behind each row; y pre-filled with FILL, row stride
    ldy = max n_out + pad_y, 64 guard floats behind the last row.  Returns (y (B, ldy), guard) as numpy."""
    from tacotron2_amd import _lib
    dev = torch.device("cuda:0")
    B = len(signals)
    ldx = max(len(s) for s in signals) + pad_x
    n_out = [R.out_len(len(s), U, D) for s in signals]
    ldy = max(n_out) + pad_y if ldy is None else ldy
    x = torch.full((B, ldx), float("nan"), dtype=torch.float32)
    for b, s in enumerate(signals):
        x[b, :len(s)] = torch.from_numpy(s)
    x = x.to(dev)
    y = torch.full((B * ldy + 64,), FILL, dtype=torch.float32, device=dev)
    n = torch.tensor([len(s) for s in signals], dtype=torch.int64, device=dev)
    a = _lib.make("T2Resample", x=x, ldx=ldx, n_in=n, y=y, ldy=ldy, n_out_max=max(n_out), table=torch.from_numpy(t32).to(dev),
                  U=U, D=D, K=K, B=B)
    _lib.call("t2_resample", a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    return y[:B * ldy].reshape(B, ldy), y[B * ldy:]


@functools.lru_cache(maxsize=None)
def case(name):
    U, D, K, ref, t32 = design(name)
    rng = np.random.default_rng(7)
    signals = [rng.standard_normal(n).astype(np.float32) for n in lengths_for(U, D, K)]
    return signals, run(signals, U, D, K, t32)


@pytest.mark.parametrize("name", list(TOYS) + list(REAL))
def test_against_the_float64_restatement(name):
    U, D, K, ref, t32 = design(name)
    signals, (y, guard) = case(name)
    assert np.isfinite(y).all()                                   # NaN sits behind every n_in: nothing there was read
    assert (guard == FILL).all()                                  # nothing behind ldy of the last row was written
    worst = 0.0
    for b, s in enumerate(signals):
        want, bound = R.apply(s, ref, U, D, K)
        n_out = R.out_len(len(s), U, D)
        assert len(want) == n_out
        err = np.abs(y[b, :n_out] - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, len(s), int(np.argmax(err - bound)))
        assert (y[b, n_out:] == 0.0).all(), (name, len(s))         # exactly zero in [n_out, ldy)
    print(f"{name}: lengths {[len(s) for s in signals]}, largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("name", ["toy_3_2_2", "toy_1_2_3", "real_147_160", "real_441_320", "toy_1_17_1"])
def test_bit_identical_between_calls_and_a_row_does_not_depend_on_its_batch(name):
    U, D, K, ref, t32 = design(name)
    rng = np.random.default_rng(11)
    n1 = n_in_for(1500, U, D)
    signals = [rng.standard_normal(n).astype(np.float32) for n in (n1 + 700, n1, 5)]
    y, guard = run(signals, U, D, K, t32)
    y2, _ = run(signals, U, D, K, t32)
    assert np.array_equal(y, y2) and (guard == FILL).all()
    alone, _ = run(signals[1:2], U, D, K, t32, pad_x=3, pad_y=200)          # row 1 alone: another B, ldx and ldy
    n_out = R.out_len(n1, U, D)
    assert np.array_equal(alone[0, :n_out].view(np.uint32), y[1, :n_out].view(np.uint32))
    assert (alone[0, n_out:] == 0.0).all() and (y[1, n_out:] == 0.0).all()


def test_output_index_times_d_beyond_32_bits():
    """U / D = 641 / 640 with n_out * D > 2^31 (13.4 MB of input): m * D must be formed in 64 bits.  The last 4096 outputs are compared."""
    U, D, K = 641, 640, 2
    t32 = np.random.default_rng(3).uniform(-1, 1, (U, 2 * K)).astype(np.float32)
    n_in = n_in_for(2 ** 31 // D + 5000, U, D)
    x = np.random.default_rng(4).standard_normal(n_in).astype(np.float32)
    n_out = R.out_len(n_in, U, D)
    assert (n_out - 4096) * D > 2 ** 31
    y, guard = run([x], U, D, K, t32)
    want, bound = R.apply(x, t32.astype(np.float64), U, D, K, first=n_out - 4096)
    assert np.isfinite(y).all() and (guard == FILL).all() and (y[0, n_out:] == 0.0).all()
    assert (np.abs(y[0, n_out - 4096:n_out] - want) <= bound).all()


def test_every_argument_rejection_returns_1():
    from tacotron2_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    x, y = torch.zeros(2, 64, device=dev), torch.zeros(2, 64, device=dev)
    n = torch.tensor([10, 20], dtype=torch.int64, device=dev)
    table = torch.zeros(3, 4, device=dev)
    good = dict(x=x, ldx=64, n_in=n, y=y, ldy=64, n_out_max=30, table=table, U=3, D=2, K=2, B=2)
    assert lib.t2_resample(C.addressof(_lib.make("T2Resample", **good)), None) == 0
    bad = [dict(B=0), dict(B=65536), dict(U=0), dict(D=0), dict(K=0), dict(U=-1), dict(U=1024, K=513), dict(U=2 ** 20, K=1),
           dict(ldy=29), dict(n_out_max=-1), dict(x=None), dict(y=None), dict(n_in=None), dict(table=None)]
    for kw in bad:
        assert lib.t2_resample(C.addressof(_lib.make("T2Resample", **dict(good, **kw))), None) == 1, kw
        assert b"t2_resample" in lib.t2_last_error(), kw
    assert lib.t2_resample(None, None) == 1
    torch.cuda.synchronize()
    assert float(y.abs().sum()) == 0.0


def test_module_api_resampler_and_engine():
    """Resampler.batch / .one and engine.resample: the kernel's outputs for the planned table, lengths as host integers."""
    from tacotron2_amd import engine
    from tacotron2_amd.datasets.resample import Resampler
    dev = torch.device("cuda:0")
    U, D, K, ref, t32 = design("real_147_160")
    rng = np.random.default_rng(5)
    sig = [rng.standard_normal(n).astype(np.float32) for n in (3200, 1601)]
    x = torch.zeros(2, 3300)
    for b, s in enumerate(sig):
        x[b, :len(s)] = torch.from_numpy(s)
    rs = Resampler(22050, dev)
    out, n_out = rs.batch(x.to(dev), [len(s) for s in sig], 24000)
    assert n_out == [2940, 1471] and out.shape == (2, 2944)
    out2, n_out2 = engine.resample(x.to(dev), torch.tensor([3200, 1601], device=dev), 24000, 22050)
    assert n_out2 == n_out and torch.equal(out, out2)
    for b, s in enumerate(sig):
        want, bound = R.apply(s, ref, U, D, K)
        got = out[b].cpu().numpy()
        assert (np.abs(got[:n_out[b]] - want) <= bound).all() and (got[n_out[b]:] == 0).all()
        one = rs.one(s, 24000)
        assert one.dtype == np.float32 and np.array_equal(one, got[:n_out[b]])
    same, n_same = rs.batch(x.to(dev), [3200, 1601], 22050)              # already at the target rate: untouched
    assert n_same == [3200, 1601] and torch.equal(same.cpu(), x)
    assert rs.one(sig[0], 22050) is not None and np.array_equal(rs.one(sig[0], 22050), sig[0])
    with pytest.raises(ValueError, match="44057"):
        rs.one(sig[0], 44057)
