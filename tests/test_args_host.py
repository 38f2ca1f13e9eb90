"""tacotron2_amd/_args.py on the CPU: every shared argument check with the values its callers rely on and its message word for word
under two caller names, the stride rules of strided_3d on CPU views, and the module layout - engine re-exports analysis' names as
the same objects, and analysis and _args import without engine.  The refusals of whole calls are in the GPU modules' lists."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tacotron2_amd import _args as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("yin", "some_caller")
CUDA = torch.device("cuda:0")          # (a name only: no tensor is ever put there)
REEXPORTED = ["yin", "prosody_stats", "voice_quality", "corpus_stats", "pitch_viterbi", "f0_path_stats", "f0_figures", "resample",
              "yin_lags", "YIN_MAX_SPAN", "PROSODY_MAX_T", "PROSODY_NSTAT", "YIN_DEFAULTS", "VQ_MAX_CYCLES", "CORPUS_NSTAT",
              "PITCH_MAX_STATES", "F0_NSTAT", "VITERBI_DEFAULTS", "_RESAMPLERS"]


def refused(call, message):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == message


# ---- scalars ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FNS)
def test_int_arg(fn):
    assert A.int_arg(fn, "hop", 256) == 256 and A.int_arg(fn, "hop", -3) == -3 and A.int_arg(fn, "hop", 0) == 0
    assert A.int_arg(fn, "hop", 1, 1) == 1 and A.int_arg(fn, "n_ceps", 32, 1, 32) == 32
    for v in (True, False, 2.0, float("nan"), "3", None, np.int64(3)):        # (no caller takes a numpy integer today)
        refused(lambda: A.int_arg(fn, "hop", v), f"{fn}: hop must be an integer, got {v!r}")
    for v in (True, 1.0, 0, -1, float("inf"), np.int32(4)):
        refused(lambda: A.int_arg(fn, "span", v, 1), f"{fn}: span must be an integer >= 1, got {v!r}")
    for v in (True, 13.0, 0, -1, 33):
        refused(lambda: A.int_arg(fn, "n_ceps", v, 1, 32), f"{fn}: n_ceps must be an integer in 1 .. 32, got {v!r}")


@pytest.mark.parametrize("fn", FNS)
def test_real_arg(fn):
    for v in (0.1, 0, -1, -2.5, 3, np.float32(0.5), np.int64(2), np.float64(-1.0)):
        got = A.real_arg(fn, "thr", v)
        assert type(got) is float and got == float(v)
    for v in (True, False, float("nan"), float("inf"), -float("inf"), "0.1", None, 1j, np.float32("nan")):
        refused(lambda: A.real_arg(fn, "thr", v), f"{fn}: thr must be a finite number, got {v!r}")
    for v in (0, 0.0, 0.25, 7, np.float32(0.5), np.int64(0)):
        assert A.real_arg(fn, "w", v, nonneg=True) == float(v)
    for v in (True, -1, -0.1, float("nan"), float("inf"), np.float64(-1e-300), None):
        refused(lambda: A.real_arg(fn, "w", v, nonneg=True), f"{fn}: w must be a finite number >= 0, got {v!r}")


@pytest.mark.parametrize("fn", FNS)
def test_batch_arg(fn):
    assert A.batch_arg(fn, 1) is None and A.batch_arg(fn, 65535) is None
    for B in (0, 65536):
        refused(lambda: A.batch_arg(fn, B), f"{fn}: batch of {B}, outside 1 .. 65535")


@pytest.mark.parametrize("fn", FNS)
def test_lags(fn):
    assert A.lags(fn, 22050, 60, 500) == (44, 367) and A.lags(fn, 22050, 60.0, 500.0) == (44, 367)
    assert A.lags(fn, 8000, 80.0, 800.0) == (10, 100)
    assert A.lags(fn, 22050, 1.0, 500.0) == (44, 22050)   # (a range too wide for a kernel is refused by the caller's own limit)
    for fmin, fmax in ((600.0, 500.0), (500.0, 500.0), (0.0, 500.0), (-1.0, 500.0), (60.0, float("inf")), (float("nan"), 500.0)):
        refused(lambda: A.lags(fn, 22050, fmin, fmax), f"{fn}: need 0 < fmin < fmax, got fmin = {fmin!r}, fmax = {fmax!r}")
    for sr in (22050.0, True, 0, -8000, "22050", np.int64(22050)):
        refused(lambda: A.lags(fn, sr, 60.0, 500.0), f"{fn}: sr must be an integer >= 1, got {sr!r}")
    # the rule the pitch kernels add (yin_lags alone never had it: a meter may be described before it is used)
    assert A.usable_lags(fn, 44, 367, 22050, 60.0, 500.0) is None and A.usable_lags(fn, 2, 4, 8, 2.0, 4.0) is None
    for (fmin, fmax), (lo, hi) in (((60.0, 22050.0), (1, 367)), ((490.0, 500.0), (44, 45)), ((60.0, 11025.0), (2, 367))):
        assert A.lags(fn, 22050, fmin, fmax) == (lo, hi)
        if (lo, hi) != (2, 367):
            refused(lambda: A.usable_lags(fn, lo, hi, 22050, fmin, fmax),
                    f"{fn}: lags {lo} .. {hi} of {fmin} .. {fmax} Hz at 22050 Hz: need tau_min >= 2 and tau_max > tau_min + 1")
    assert A.usable_lags(fn, 2, 367, 22050, 60.0, 11025.0) is None


def test_yin_lags_keeps_its_prefix():
    from tacotron2_amd import analysis
    assert analysis.yin_lags(22050, 60, 500) == (44, 367) and analysis.yin_lags(22050, 60.0, 22050.0) == (1, 367)
    refused(lambda: analysis.yin_lags(22050, 600.0, 500.0), "yin: need 0 < fmin < fmax, got fmin = 600.0, fmax = 500.0")
    refused(lambda: analysis.yin_lags(22050.0, 60.0, 500.0), "yin: sr must be an integer >= 1, got 22050.0")


# ---- tensors: what fires before the device check, then the device check itself --------------------------------------------------------
@pytest.mark.parametrize("fn", FNS)
def test_tensor_arg_and_devices(fn):
    x3 = torch.zeros(2, 5, 7)
    assert A.tensor_arg(fn, "cmnd", x3, 3, "(B, T, tau_max + 1)") is None
    for bad in (x3.double(), x3[0], x3.int(), x3.numpy(), None):
        refused(lambda: A.tensor_arg(fn, "cmnd", bad, 3, "(B, T, tau_max + 1)"), f"{fn}: cmnd must be a float32 (B, T, tau_max + 1) tensor")
    refused(lambda: A.tensor_arg(fn, "cycles", x3[0], 2, "(B, T)", torch.int32), f"{fn}: cycles must be a int32 (B, T) tensor")
    refused(lambda: A.on_gpu(fn, "cmnd", x3), f"{fn}: cmnd must be on the GPU, got cpu")
    assert A.on_device(fn, "a", x3, torch.device("cpu")) is None
    for bad in (x3, None, [1, 2]):
        refused(lambda: A.on_device(fn, "n", bad, CUDA), f"{fn}: n must be a tensor on the device of the signals, cuda:0")
        refused(lambda: A.on_device(fn, "len_a", bad, CUDA, engine=True), f"{fn}: len_a must be a tensor on the engine's device cuda:0")


@pytest.mark.parametrize("fn", FNS)
def test_lengths(fn):
    cpu = torch.device("cpu")
    for n in (torch.tensor([3, 4]), torch.tensor([3, 4], dtype=torch.int16), torch.tensor([3, 4], dtype=torch.uint8)):
        assert A.lengths(fn, "n", n, 2, cpu) is n
    for bad in (torch.tensor([3.0, 4.0]), torch.tensor([True, False]), torch.tensor([3]), torch.tensor([[3, 4]]), torch.tensor(3)):
        refused(lambda: A.lengths(fn, "n", bad, 2, cpu), f"{fn}: n must be 2 integers")
        refused(lambda: A.lengths(fn, "len_b", bad, 2, cpu, engine=True), f"{fn}: len_b must be 2 integers")
    refused(lambda: A.lengths(fn, "n", torch.tensor([3.0, 4.0]), 2, CUDA), f"{fn}: n must be a tensor on the device of the signals, cuda:0")
    refused(lambda: A.lengths(fn, "lens", [3, 4], 2, CUDA, engine=True), f"{fn}: lens must be a tensor on the engine's device cuda:0")


@pytest.mark.parametrize("fn", FNS)
def test_padded_wav_on_host_tensors(fn):
    wav, n = torch.zeros(2, 3000), torch.tensor([3000, 10])
    args = (n, None, 22050, 256, 1024, 60.0, 500.0)
    for bad in (wav.double(), wav[0], wav[None], wav.numpy(), None):
        refused(lambda: A.padded_wav(fn, bad, *args), f"{fn}: wav must be a float32 (B, samples) tensor")
    refused(lambda: A.padded_wav(fn, wav, *args), f"{fn}: wav must be on the GPU, got cpu")


@pytest.mark.parametrize("fn", FNS)
def test_same_shape_2d_on_host_tensors(fn):
    f0, z = torch.zeros(2, 12), torch.zeros(2, 12)
    cyc = torch.zeros(2, 12, dtype=torch.int32)
    for bad in (z.double(), z[0], None, cyc):            # (every array passes all three checks before the next one is looked at)
        refused(lambda: A.same_shape_2d(fn, (("f0", bad), ("aper", z))), f"{fn}: f0 must be a float32 (B, T) tensor")
    refused(lambda: A.same_shape_2d(fn, (("cycles", z), ("f0", f0)), dtypes=dict(cycles=torch.int32)), f"{fn}: cycles must be a int32 (B, T) tensor")
    refused(lambda: A.same_shape_2d(fn, (("f0", f0), ("cycles", cyc)), dtypes=dict(cycles=torch.int32)),
            f"{fn}: f0 must be on the GPU, all on one device")


@pytest.mark.parametrize("fn", FNS)
def test_dense_arg(fn):
    cpu = torch.device("cpu")
    x = torch.zeros(2, 12)
    assert A.dense_arg(fn, "f0", x, (2, 12), cpu) is None and A.dense_arg(fn, "f0_a", x, (2, None), cpu) is None
    for bad in (None, x.double(), x[:, :11], x[0], x.t().contiguous().t(), torch.zeros(2, 24)[:, ::2]):
        refused(lambda: A.dense_arg(fn, "f0", bad, (2, 12), cpu), f"{fn}: f0 must be a contiguous float32 (2, 12) tensor on cpu")
    refused(lambda: A.dense_arg(fn, "power", x, (2, 12), CUDA), f"{fn}: power must be a contiguous float32 (2, 12) tensor on cuda:0")
    for bad in (torch.zeros(2, 0), torch.zeros(3, 5), torch.zeros(2), x.long()):
        refused(lambda: A.dense_arg(fn, "f0_b", bad, (2, None), cpu), f"{fn}: f0_b must be a contiguous float32 (2, T >= 1) tensor on cpu")


# ---- strided_3d -----------------------------------------------------------------------------------------------------------------------
def parent_strides(x):
    """What Engine.durations and Engine._check_seq derived before the checks were shared.  (pitch_viterbi had (T - 1) * ld_t + C for
    B == 1: the same number for a contiguous tensor, and a field that no kernel multiplies by anything but the batch index 0.)"""
    B, T, C = x.shape
    ld_t = x.stride(1) if T > 1 else C
    return (x.stride(0) if B > 1 else T * ld_t), ld_t


def test_strided_3d_accepts_dense_and_row_padded_views():
    big = torch.zeros(3, 9, 16)
    cases = dict(contiguous=torch.zeros(3, 5, 7), cut=big[:, :5, :7], cut_rows=big[:, :5], B1=big[:1, :5, :7], B1_dense=torch.zeros(1, 5, 7),
                 T1=big[:, :1, :7], T1_B1=big[1:2, 2:3, :7], C1=big[:, :5, :1], spaced=torch.zeros(2, 40).as_strided((2, 3, 4), (20, 6, 1)))
    for name, x in cases.items():
        assert A.strided_3d("dtw", "a", x) == parent_strides(x), name
    assert A.strided_3d("dtw", "a", cases["contiguous"]) == (35, 7) and A.strided_3d("dtw", "a", cases["cut"]) == (144, 16)
    assert A.strided_3d("dtw", "a", cases["B1"]) == (80, 16) and A.strided_3d("dtw", "a", cases["T1"]) == (144, 7)
    assert A.strided_3d("dtw", "a", cases["T1_B1"]) == (7, 7) and A.strided_3d("dtw", "a", cases["C1"]) == (144, 16)


@pytest.mark.parametrize("fn", FNS)
def test_strided_3d_refuses_strided_columns_and_overlapping_rows(fn):
    x = torch.zeros(2, 5, 8)
    for bad in (x[:, :, ::2], x.transpose(1, 2), x[:, :, None, 0].expand(2, 5, 8)):
        refused(lambda: A.strided_3d(fn, "cmnd", bad), f"{fn}: the last dimension of cmnd must be contiguous")
    flat = torch.zeros(200)
    for strides in ((40, 4, 1), (20, 8, 1), (0, 8, 1), (40, 0, 1)):          # rows overlap; utterances overlap; one row for all
        bad = flat.as_strided((2, 5, 8), strides)
        refused(lambda: A.strided_3d(fn, "mel", bad), f"{fn}: overlapping rows of mel (strides {strides})")
    assert A.strided_3d(fn, "mel", flat.as_strided((1, 5, 8), (0, 8, 1))) == (40, 8)        # (B == 1: the batch stride is not used)
    refused(lambda: A.strided_3d(fn, "mel", flat.as_strided((1, 5, 8), (40, 4, 1))), f"{fn}: overlapping rows of mel (strides (40, 4, 1))")


# ---- wav_rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FNS)
def test_wav_rows_messages(fn):
    x = torch.zeros(2, 100)
    assert A.wav_rows(fn, "wav", x) == (2, 100, 100) and A.wav_rows(fn, "wav", x, 100) == (2, 100, 100)
    for bad in (x.double(), x[0], x[None], x.int(), x.numpy(), None):
        refused(lambda: A.wav_rows(fn, "wav", bad), f"{fn}: wav must be a float32 (B, samples) tensor")
    refused(lambda: A.wav_rows(fn, "wav", torch.zeros(0, 100)), f"{fn}: batch of 0, outside 1 .. 65535")
    refused(lambda: A.wav_rows(fn, "wav", torch.zeros(1, 1).expand(65536, 1)), f"{fn}: batch of 65536, outside 1 .. 65535")
    refused(lambda: A.wav_rows(fn, "wav", x, 99), f"{fn}: rows of 100 samples, above the limit of 99")
    refused(lambda: A.wav_rows(fn, "wav", torch.zeros(0, 100), 99), f"{fn}: batch of 0, outside 1 .. 65535")       # (the batch first)
    refused(lambda: A.wav_rows(fn, "wav", torch.zeros(2, 200)[:, ::2]), f"{fn}: the last dimension of wav must be contiguous")
    refused(lambda: A.wav_rows(fn, "wav", torch.zeros(2, 200)[:, ::2], 99), f"{fn}: rows of 100 samples, above the limit of 99")   # (the limit before the layout)
    refused(lambda: A.wav_rows(fn, "wav", torch.zeros(200).as_strided((2, 100), (50, 1))), f"{fn}: overlapping rows of wav (row stride 50, 100 samples)")
    refused(lambda: A.row_stride(fn, "lag", torch.zeros(20, dtype=torch.int32).as_strided((2, 10), (5, 1)), "frames"),
            f"{fn}: overlapping rows of lag (row stride 5, 10 frames)")


def test_wav_rows_stride_rule_on_views():
    big = torch.zeros(2, 4096)
    assert A.wav_rows("f", "wav", torch.zeros(1, 0)) == (1, 0, 1)                      # one row without a column: a stride of 1, not 0
    assert A.wav_rows("f", "wav", big[:, :3000]) == (2, 3000, 4096)                    # a cut of a larger buffer keeps its stride
    assert A.wav_rows("f", "wav", big[:1, :3000]) == (1, 3000, 3000) and A.wav_rows("f", "wav", big[1:, 5:]) == (1, 4091, 4091)
    assert A.wav_rows("f", "wav", torch.zeros(3, 1)) == (3, 1, 1) and A.wav_rows("f", "wav", big[:, 7:8]) == (2, 1, 4096)
    refused(lambda: A.wav_rows("f", "wav", torch.zeros(3000, 2).t()), "f: the last dimension of wav must be contiguous")
    refused(lambda: A.wav_rows("f", "wav", torch.zeros(1, 1).expand(2, 5)), "f: the last dimension of wav must be contiguous")
    flat = torch.zeros(300)
    for stride in (99, 50, 1, 0):
        refused(lambda: A.wav_rows("f", "wav", flat.as_strided((3, 100), (stride, 1))), f"f: overlapping rows of wav (row stride {stride}, 100 samples)")
    assert A.wav_rows("f", "wav", flat.as_strided((3, 100), (100, 1))) == (3, 100, 100)
    assert A.wav_rows("f", "wav", flat.as_strided((1, 100), (0, 1))) == (1, 100, 100)  # (B == 1: the row stride is not used)


# ---- the module layout ------------------------------------------------------------------------------------------------------------------
def test_engine_reexports_the_measurements_as_the_same_objects():
    from tacotron2_amd import analysis, engine
    for name in REEXPORTED:
        assert getattr(engine, name) is getattr(analysis, name), name
    public = [k for k, v in vars(analysis).items() if not k.startswith("_") and getattr(v, "__module__", None) == analysis.__name__]
    assert sorted(public) == sorted(k for k in REEXPORTED if callable(getattr(analysis, k)))
    assert not hasattr(engine, "_check_lengths")


@pytest.mark.parametrize("module", ["analysis", "_args"])
def test_imports_without_engine(module):
    code = f"import sys, tacotron2_amd.{module}; print('tacotron2_amd.engine' in sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "False", (r.stdout, r.stderr)
