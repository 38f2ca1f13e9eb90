"""Per-character durations on the GPU: t2_align_durations (csrc/t2_align.hip) against the float64 restatement of
tests/durations_ref.py, then Engine.durations, the module surface and the two drivers.

Criteria.  `dur` must be EQUAL to the reference in both modes.  Equality is only meaningful away from ties, so every monotonic
case first asserts that the reference's own smallest on-path decision margin |Q[s-1][n] - Q[s-1][n-1]| is at least 1e-6: the kernel
runs the same fp64 recurrence in the same order, and its fp64 log differs from the host's by ~1e-15 (the seeded kernel-level inputs
below give margins between 1.1e-2 and 4.5, computed on the CPU; the engine-level alignments come from the GPU and are checked as they come).  `stats` within 4e-6 absolute: the float32 rounding of a double-accumulated mean of values in
[-18.5, 1] (half an ulp at 18.5 is 9.5e-7; the sum order and the device log add ~1e-14)."""
import ctypes as C
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import durations_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6
STATS_TOL = 4e-6
MODES = {"argmax": 0, "monotonic": 1}


def _dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def _softmax_rows(rng, B, S, L, N, sharpen):
    """(B, S, L) float32: softmax over the first N positions of normal scores, optionally with a sharpened diagonal; NaN behind N."""
    z = rng.normal(size=(B, S, N))
    if sharpen:
        s = np.arange(S)
        z[:, s, np.minimum(s * N // S, N - 1)] += sharpen
    e = np.exp(z - z.max(axis=2, keepdims=True))
    a = np.full((B, S, L), np.nan, dtype=np.float32)
    a[:, :, :N] = e / e.sum(axis=2, keepdims=True)
    return a


def _kernel(a, chars_len, frames_len, r, mode, dev, back="alloc"):
    """One t2_align_durations call on the tensor `a` (device, any strides with a contiguous last dimension) -> (dur, stats) numpy."""
    from tacotron2_amd import _lib
    B, S, L = a.shape
    dur = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    stats = torch.full((B, 4), float("nan"), device=dev)
    bk = torch.empty(B * S * L, dtype=torch.uint8, device=dev) if (back == "alloc" and mode == "monotonic") else None
    cl = torch.as_tensor(chars_len, dtype=torch.int32).to(dev)
    fl = torch.as_tensor(frames_len, dtype=torch.int32).to(dev)
    st = _lib.make("T2AlignDur", align=a, ld_b=a.stride(0), ld_s=a.stride(1), B=B, S=S, L=L, r=r, mode=MODES[mode], chars_len=cl,
                   frames_len=fl, dur=dur, ld_dur=L, stats=stats, back=bk)
    _lib.call("t2_align_durations", st, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dur.cpu().numpy(), stats.cpu().numpy()


def _compare(a_np, chars_len, frames_len, r, dev, a_dev=None, label=""):
    """Both modes of the kernel against the reference on the same array; returns the monotonic durations."""
    a_dev = torch.from_numpy(a_np).to(dev) if a_dev is None else a_dev
    out = None
    for mode in ("monotonic", "argmax"):
        rd, rs, margin = R.durations_batch(a_np, chars_len, frames_len, r, mode)
        print(f"[durations] {label} {mode}: smallest on-path margin {margin:.3e}")
        assert margin >= MARGIN, (label, mode, margin)
        dur, stats = _kernel(a_dev, chars_len, frames_len, r, mode, dev)
        err = float(np.abs(stats.astype(np.float64) - rs).max())
        print(f"[durations] {label} {mode}: dur mismatches {int((dur != rd).sum())}, stats error {err:.3e} /{STATS_TOL:.0e}")
        assert np.isfinite(stats).all()
        assert np.array_equal(dur, rd), (label, mode, np.argwhere(dur != rd)[:8].tolist())
        assert err <= STATS_TOL, (label, mode, err)
        if mode == "monotonic":
            out = dur
    return out


# (S, L, N): N = L except at the cap; (64,64) has one feasible path; (300,257) crosses the 256-thread stride and a wave boundary
SHAPES = [(1, 1, 1), (64, 64, 64), (65, 64, 64), (40, 7, 7), (300, 257, 257), (500, 300, 300), (12, 4096, 9)]


@pytest.mark.parametrize("S,L,N", SHAPES)
def test_kernel_equals_the_reference(S, L, N):
    dev = _dev()
    rng = np.random.default_rng(1000 * S + L)
    # two utterances per case: plain softmax-of-normal rows and rows with a sharpened diagonal
    a = np.concatenate([_softmax_rows(rng, 1, S, L, N, 0.0), _softmax_rows(rng, 1, S, L, N, 4.0)])
    dur = _compare(a, [N, N], [S, S], 1, dev, label=f"({S},{L},{N})")
    assert (dur[:, :N] >= 1).all() and not dur[:, N:].any() and dur.sum(1).tolist() == [S, S]


def test_ragged_batch_reads_nothing_behind_the_lengths():
    """B = 5 with mixed lengths - an empty text, an utterance without frames, one with fewer steps than characters - everything
    behind each utterance's N_b and S_b NaN, and batch rows further apart than S*L with NaN in the gap."""
    dev = _dev()
    B, S, L, gap = 5, 20, 12, 37
    chars_len, frames_len = [12, 0, 7, 9, 5], [20, 15, 0, 6, 13]
    rng = np.random.default_rng(42)
    a = np.full((B, S, L), np.nan, dtype=np.float32)
    for b, (N, F) in enumerate(zip(chars_len, frames_len)):
        if N and F:
            a[b, :F, :N] = _softmax_rows(rng, 1, F, N, N, 3.0 if b % 2 else 0.0)[0]
    flat = torch.full((B, S * L + gap), float("nan"), device=dev)
    flat[:, :S * L] = torch.from_numpy(a).to(dev).view(B, S * L)
    a_dev = flat.as_strided((B, S, L), (S * L + gap, L, 1))
    dur = _compare(a, chars_len, frames_len, 1, dev, a_dev=a_dev, label="ragged")
    _, stats = _kernel(a_dev, chars_len, frames_len, 1, "monotonic", dev)
    assert stats[:, 2].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0] and not stats[1].any() and not stats[2].any()
    for b, (N, F) in enumerate(zip(chars_len, frames_len)):
        assert not dur[b, N:].any() and dur[b].sum() == (F if N else 0)


@pytest.mark.parametrize("r,F", [(2, 37), (3, 64), (3, 62)])
def test_reduction_factor_frames_per_step(r, F):
    dev = _dev()
    S, L, N = (F + r - 1) // r + 2, 10, 9          # two step rows more than the utterances use: NaN
    rng = np.random.default_rng(r * 100 + F)
    a = _softmax_rows(rng, 2, S, L, N, 3.0)
    F2 = F - r - 1                                  # a second utterance with another remainder
    a[0, (F + r - 1) // r:] = np.nan
    a[1, (F2 + r - 1) // r:] = np.nan
    dur = _compare(a, [N, N], [F, F2], r, dev, label=f"r={r} F={F}")
    assert dur.sum(1).tolist() == [F, F2]
    assert dur[0, N - 1] % r == (F % r or r) % r   # the last character holds the short last step


def test_a_tie_stays_on_the_character():
    dev = _dev()
    a = torch.full((1, 4, 2), 0.5, device=dev)
    dur, stats = _kernel(a, [2], [4], 1, "monotonic", dev)
    assert dur.tolist() == [[1, 3]] and stats[0, 2] == 1.0 and abs(stats[0, 0] - 0.5) <= STATS_TOL


def test_argmax_of_equal_maxima_is_the_lowest_position():
    """L = 130, argmax mode: a wave's lane l scans positions l, l + 64, l + 128.  Step 0 has equal maxima at 5 and 70 (lanes 5 and 6:
    the shuffle walk decides), step 1 at 5 and 69 (both lane 5: its serial scan decides), step 2 at 70 and 129 (lanes 6 and 1, the
    higher lane holding the lower position).  The lower position wins each time, as numpy's argmax."""
    dev = _dev()
    a = np.full((1, 3, 130), 0.001, dtype=np.float32)
    a[0, 0, [5, 70]], a[0, 1, [5, 69]], a[0, 2, [70, 129]] = 0.25, 0.25, 0.25
    rd, rs, _ = R.durations_batch(a, [130], [3], 1, "argmax")
    assert rd[0, 5] == 2 and rd[0, 70] == 1 and rd.sum() == 3
    dur, stats = _kernel(torch.from_numpy(a).to(dev), [130], [3], 1, "argmax", dev)
    assert np.array_equal(dur, rd), np.nonzero(dur[0])[0].tolist()
    assert float(np.abs(stats.astype(np.float64) - rs).max()) <= STATS_TOL
    dur, stats = _kernel(torch.from_numpy(a).to(dev), [130], [3], 1, "monotonic", dev)      # (3 steps < 130 characters: the argmax fall-back)
    assert np.array_equal(dur, rd) and stats[0, 2] == 0.0


def test_staircase_alignment_gives_back_its_durations():
    dev = _dev()
    d = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5], dtype=np.int32)
    N, S, L = len(d), int(d.sum()), 16
    a = np.full((1, S, L), np.nan, dtype=np.float32)
    a[0, :, :N] = 0.1 / (N - 1)
    a[0, np.arange(S), np.repeat(np.arange(N), d)] = 0.9
    dur = _compare(a, [N], [S], 1, dev, label="staircase")
    assert dur[0, :N].tolist() == d.tolist()
    assert _kernel(torch.from_numpy(a).to(dev), [N], [S], 1, "argmax", dev)[0][0, :N].tolist() == d.tolist()


def test_argument_errors_launch_nothing():
    from tacotron2_amd import _lib
    dev = _dev()
    lib = _lib.lib()
    B, S = 1, 3
    for L, r, mode, with_back, word in ((4097, 1, 1, True, b"T2_ALIGN_MAX_L"), (8, 1, 2, True, b"mode"), (8, 1, 1, False, b"back"),
                                        (8, 0, 0, True, b"r >= 1")):
        a = torch.full((B, S, L), 1.0 / L, device=dev)
        dur = torch.full((B, L), -7, dtype=torch.int32, device=dev)
        stats = torch.full((B, 4), -7.0, device=dev)
        one = torch.ones(B, dtype=torch.int32, device=dev)
        st = _lib.make("T2AlignDur", align=a, ld_b=S * L, ld_s=L, B=B, S=S, L=L, r=r, mode=mode, chars_len=one, frames_len=one,
                       dur=dur, ld_dur=L, stats=stats, back=torch.zeros(B * S * L, dtype=torch.uint8, device=dev) if with_back else None)
        assert lib.t2_align_durations(C.addressof(st), None) == 1            # T2_ERR_ARG
        assert word in lib.t2_last_error(), lib.t2_last_error()
        torch.cuda.synchronize()
        assert bool((dur == -7).all()) and bool((stats == -7.0).all())       # nothing ran
        with pytest.raises(_lib.T2Error):
            _lib.call("t2_align_durations", st, None)


# ---- engine and module level ------------------------------------------------------------------------------------------------------
TINY = dict(num_chars=39, encoded_dim=64, encoder_kernel_size=5, num_mels=80, prenet_dim=32, att_rnn_dim=64, att_dim=32,
            rnn_hidden_dim=64, postnet_dim=64, dropout=0.5)       # the dims of tests/test_gpu_cli.py::_cfg
GUARD = 4096


def _tiny_model(r, dev):
    from tacotron2_amd.model import Tacotron2
    m = Tacotron2(**TINY, device=dev, seed=11, reduction_factor=r)
    m._engine.guard_bytes = GUARD
    m.eval()
    return m


def _batch(dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    B, L, T = 3, 11, 25
    lens, tl = torch.tensor([11, 7, 4]), torch.tensor([25, 19, 12])
    ci = torch.zeros(B, L, dtype=torch.int64)
    mel = torch.zeros(B, T, 80)
    for b in range(B):
        ci[b, :lens[b]] = torch.randint(1, 40, (int(lens[b]),), generator=g)
        mel[b, :tl[b]] = torch.randn(int(tl[b]), 80, generator=g) - 3
    return ci.to(dev), lens.to(dev), mel.to(dev), tl.to(dev)


def _check_engine(eng, align, chars_len, frames_len, label):
    a_np = align.cpu().numpy()
    cl, fl = chars_len.cpu().numpy(), frames_len.cpu().numpy()
    res = {}
    for mode in ("monotonic", "argmax"):
        rd, rs, margin = R.durations_batch(a_np, cl, fl, eng.r, mode)
        print(f"[durations] {label} {mode}: smallest on-path margin {margin:.3e}")
        assert margin >= MARGIN, (label, mode, margin)
        dur, stats = eng.durations(align, chars_len, frames_len, mode=mode)
        assert dur.dtype == torch.int32 and stats.dtype == torch.float32 and dur.shape == a_np[:, 0].shape and stats.shape == (len(cl), 4)
        assert np.array_equal(dur.cpu().numpy(), rd), (label, mode)
        assert float(np.abs(stats.cpu().numpy().astype(np.float64) - rs).max()) <= STATS_TOL
        assert dur.sum(1).cpu().tolist() == [int(min(f, eng.r * a_np.shape[1])) for f in fl]
        res[mode] = (dur, stats)
    eng.check_persistent_kernels()          # guard bands on: raises on a band hit
    assert eng.guard_check() == [] and {"dur.dur", "dur.stats", "dur.back"} <= set(eng._guards)
    return res


@pytest.mark.parametrize("r", [1, 2])
def test_engine_durations_of_a_teacher_forced_forward(r):
    dev = _dev()
    m = _tiny_model(r, dev)
    ci, lens, mel, tl = _batch(dev)
    dur, stats, align = m.durations(ci, lens, mel, tl)
    assert not m.training and align.shape == (3, (25 + r - 1) // r, 11)
    res = _check_engine(m._engine, align, lens, tl, f"forward_tf r={r}")
    assert torch.equal(dur, res["monotonic"][0]) and torch.equal(stats, res["monotonic"][1])
    assert dur.sum(1).cpu().tolist() == tl.cpu().tolist()
    # int64 lengths and another integer dtype give the same result; the module keeps its train / eval state
    d16, _ = m._engine.durations(align, lens.to(torch.int16), tl.to(torch.int16))
    assert torch.equal(d16, dur)
    m.train()
    d2, s2, _ = m.durations(ci, lens, mel, tl, mode="argmax")
    assert m.training and torch.equal(d2, res["argmax"][0])


@pytest.mark.parametrize("r", [1, 2])
def test_engine_durations_of_a_decode_through_a_strided_view(r):
    dev = _dev()
    m = _tiny_model(r, dev)
    ci, lens, _, _ = _batch(dev)
    m.store.P["decoder.gate.bias"].fill_(5.0)          # never stops: every utterance runs to the 23-frame cap
    out = m._engine.infer(ci, lens, 23, seed=3, check_every=8)
    align, lengths = out[3], out[4]
    ns = align.shape[1]
    big = torch.full((3, ns + 3, 11), float("nan"), device=dev)
    big[:, :ns] = align
    view = big[:, :ns]                       # the layout of a decode's alignments before they are cut: rows further apart than ns * L
    assert not view.is_contiguous()
    res = _check_engine(m._engine, view, lens, lengths, f"infer r={r}")
    assert res["monotonic"][0].sum(1).cpu().tolist() == lengths.cpu().tolist()


def test_engine_durations_refuses_what_the_kernel_cannot_take():
    dev = _dev()
    m = _tiny_model(1, dev)
    eng = m._engine
    one = torch.ones(2, dtype=torch.int32, device=dev)
    a = torch.full((2, 3, 8), 0.125, device=dev)
    with pytest.raises(ValueError, match="4096"):
        eng.durations(torch.zeros(2, 1, 4097, device=dev), one, one)
    with pytest.raises(ValueError, match="float32"):
        eng.durations(a.double(), one, one)
    with pytest.raises(ValueError, match="contiguous"):
        eng.durations(a.transpose(1, 2), one, one)
    with pytest.raises(ValueError, match="device"):
        eng.durations(a.cpu(), one, one)
    with pytest.raises(ValueError, match="device"):
        eng.durations(a, one.cpu(), one)
    with pytest.raises(ValueError, match="mode"):
        eng.durations(a, one, one, mode="viterbi")


# ---- drivers ------------------------------------------------------------------------------------------------------------------------
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"


def _run(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_duration_export_and_say_durations_out(tmp_path):
    sr = 22050
    speech = tmp_path / "wavs"
    speech.mkdir()
    rng = np.random.default_rng(0)
    texts, samples, rows = {}, {}, []
    for i in range(6):
        k = sr // 2 + 997 * i
        x = 0.3 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(k) / sr) + 0.01 * rng.normal(size=k)
        with wave.open(str(speech / f"u{i}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes((x * 32767).astype("<i2").tobytes())
        texts[f"u{i}.wav"] = f"Utterance number {i}{', and a few more words' * (i % 3)}, Dr. Who says hi!"
        samples[f"u{i}.wav"] = k
        rows.append(f"{texts[f'u{i}.wav']}|u{i}.wav|{i % 4}")
    (tmp_path / "train.csv").write_text("\n".join(["text|wav|speaker_id"] + rows[:4]) + "\n")
    (tmp_path / "val.csv").write_text("\n".join(["text|wav|speaker_id"] + rows[4:]) + "\n")
    cfg = {"dataset": {"train": str(tmp_path / "train.csv"), "val": str(tmp_path / "val.csv"),
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^",
                                         "silence": 512, "trim": False, "num_mels": 80, "cache": True}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "precision": "16-mixed",
                        "args": {"max_steps": 6, "val_check_interval": 0.5}},
           "model": {"scheduler_milestones": [0.5, 0.75],
                     "args": {"prenet_dim": 32, "att_rnn_dim": 64, "att_dim": 32, "rnn_hidden_dim": 64, "postnet_dim": 64,
                              "dropout": 0.5, "char_embedding_dim": 64, "encoder_kernel_size": 5}},
           "extensions": {"speaker_tokens": {"active": True, "num_speakers": 4}, "controls": {"active": False}}}
    cfgp = tmp_path / "cfg.json"
    cfgp.write_text(json.dumps(cfg))
    res = tmp_path / "res"
    _run(["--config", str(cfgp), "--device", "0", "train", "--speech-dir", "unused", "--results-dir", str(res), "--synthetic",
          "--max-steps", "3"])
    ck = str(res / "final.ckpt")
    exp = tmp_path / "dur"
    _run(["--config", str(cfgp), "--device", "0", "duration-export", "--speech-dir", str(speech), "--checkpoint", ck,
          "--results-dir", str(exp)])
    from tacotron2_amd.datasets.text import TextEncoder
    enc = TextEncoder(ALLOWED, "^", expand_abbrev=True)
    lines = (exp / "durations.csv").read_text().splitlines()
    assert lines[0] == "wav|n_chars|n_frames|focus_rate|path_logp|feasible|argmax_agreement" and len(lines) == 7
    assert sorted(os.listdir(exp)) == sorted([f"u{i}.wav.dur.npy" for i in range(6)] + ["durations.csv"])
    for line in lines[1:]:
        wav, n_chars, n_frames, focus, logp, feasible, agree = line.split("|")
        d = np.load(exp / f"{wav}.dur.npy")
        frames = 1 + (samples[wav] + 512) // 256                 # samples after the configured silence pad
        assert d.dtype == np.int32 and d.shape == (len(enc.encode(texts[wav])),) == (int(n_chars),)
        assert int(d.sum()) == frames == int(n_frames) and (d >= 0).all()
        assert 0.0 < float(focus) <= 1.0 and float(logp) < 0.0 and feasible in ("0", "1") and 0.0 <= float(agree) <= 1.0
        if feasible == "1":
            assert (d >= 1).all()                                # a monotonic path gives every character a step
    # say --durations-out: character timestamps from the decode's own alignments
    npy, js = tmp_path / "say.npy", tmp_path / "say.json"
    _run(["--config", str(cfgp), "--device", "0", "say", "--checkpoint", ck, "--text", "Hello, Mr. Smith-Jones!", "--out", str(npy),
          "--random-seed", "3", "--speaker-id", "1", "--durations-out", str(js)])
    mel = np.load(npy)
    out = json.loads(js.read_text())
    assert len(out) == 1
    o = out[0]
    sym = list(TextEncoder(ALLOWED, "^", expand_abbrev=False).clean("Hello, Mr. Smith-Jones!"))
    assert o["symbols"] == sym and len(o["frames"]) == len(o["start_s"]) == len(o["end_s"]) == len(sym)
    total = sum(o["frames"])
    assert total == mel.shape[0] and o["end_s"][-1] == total * 256 / 22050 and o["start_s"][0] == 0.0
    assert all(abs(e - s - f * 256 / 22050) < 1e-9 for s, e, f in zip(o["start_s"], o["end_s"], o["frames"]))
    # (a model of three training steps may stop after a few frames: fewer frames than symbols has no monotonic path, and says so)
    assert o["feasible"] is (total >= len(sym)) and 0.0 < o["focus_rate"] <= 1.0
    assert min(o["frames"]) >= (1 if o["feasible"] else 0)
