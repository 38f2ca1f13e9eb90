"""`main.py train` with the optimiser options on synthetic batches, a resume from its checkpoint, and `main.py say --ema` on the
result: the checkpoint carries the shadow weights, the counter and the schedule; the printed learning rates are Trainer.lr_at's; the
resume continues the schedule and the counter; `say --ema` decodes from the shadow weights, bit for bit what `say` gives on a copy of
the file whose state_dict was replaced by them; without shadow weights it exits with a message that names the file."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_cli import ALLOWED, ROOT  # noqa: E402

OPTS = ["--ema-decay", "0.999", "--decoupled-weight-decay", "--lr-schedule", "exponential", "--lr-warmup", "2", "--lr-decay", "2,2,1e-5"]


def _cfg(tmp_path):
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv",
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "silence": 512,
                                         "trim": False, "num_mels": 80, "cache": True}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-2, "name": "tiny", "precision": "16-mixed",
                        "args": {"max_steps": 6, "val_check_interval": 0.5, "log_every_n_steps": 1}},
           "model": {"scheduler_milestones": [],
                     "args": {"prenet_dim": 32, "att_rnn_dim": 64, "att_dim": 32, "rnn_hidden_dim": 64, "postnet_dim": 64, "dropout": 0.5,
                              "char_embedding_dim": 64, "encoder_kernel_size": 5}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    return str(p)


def _cli(args, ok=True):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def _lrs(out):
    return {int(m.group(1)): m.group(2) for m in re.finditer(r"^step (\d+)/\d+ training_gate_loss .* lr (\S+) ", out, flags=re.M)}


def _say(cfg, ckpt, out, *extra, ok=True):
    """24 frames at most, and a stop threshold of 0.01: four steps from random weights leave the stop probability near 0.5, where the
    default threshold may end the decode at its first frame; the comparison needs frames to compare."""
    return _cli(["--config", cfg, "--device", "0", "say", "--checkpoint", str(ckpt), "--text", "Hello there.", "--out", str(out),
                 "--random-seed", "3", "--max-len", "24", "--stop-threshold", "0.01"] + list(extra), ok=ok)


def test_cli_train_resume_and_say_with_the_ema_weights(tmp_path):
    from tacotron2_amd.options import OptimizerOptions, lr_at
    cfg = _cfg(tmp_path)
    res = tmp_path / "res"
    train = ["--config", cfg, "--device", "0", "train", "--speech-dir", "unused", "--synthetic"]
    out = _cli(train + ["--results-dir", str(res), "--max-steps", "4"] + OPTS).stdout
    o = OptimizerOptions(decoupled_weight_decay=True, ema_decay=0.999, schedule="exponential", warmup_steps=2, decay_start=2, decay_steps=2,
                         min_lr=1e-5)
    want = {t + 1: f"{lr_at(1e-3, [], o, t):.2e}" for t in range(6)}
    assert [want[k] for k in (1, 2, 3, 4, 5)] == ["5.00e-04", "1.00e-03", "1.00e-03", "1.00e-04", "1.00e-05"]
    assert _lrs(out) == {k: want[k] for k in (1, 2, 3, 4)}, out
    ck = torch.load(res / "final.ckpt", map_location="cpu", weights_only=True)
    assert ck["global_step"] == 4 and ck["ema"] == {"decay": 0.999, "num_updates": 4}
    assert list(ck["ema_state_dict"]) == list(ck["state_dict"])
    moved = [k for k, v in ck["state_dict"].items() if v.is_floating_point() and "running_" not in k and not torch.equal(v, ck["ema_state_dict"][k])]
    assert len(moved) >= 0.9 * sum(1 for k in ck["state_dict"] if "running_" not in k and "num_batches" not in k), moved
    assert ck["optimizer_states"][0]["param_groups"][0]["decoupled_weight_decay"] is True
    sch = ck["lr_schedulers"][0]
    assert sch["t2_schedule"] == dict(schedule="exponential", warmup_steps=2, decay_start=2, decay_steps=2, min_lr=1e-5, milestones=[])
    assert sch["last_epoch"] == 4 and sch["base_lrs"] == [1e-3] and sch["_last_lr"] == [lr_at(1e-3, [], o, 4)]
    # resume without naming the schedule again: the file's schedule and counter continue at step 5
    res2 = tmp_path / "res2"
    out2 = _cli(train + ["--results-dir", str(res2), "--max-steps", "6", "--resume-ckpt", str(res / "final.ckpt"), "--ema-decay", "0.999",
                         "--decoupled-weight-decay"]).stdout
    assert _lrs(out2) == {5: want[5], 6: want[6]}, out2
    assert "schedule" in out2 and "replaces the configured one" in out2
    ck2 = torch.load(res2 / "final.ckpt", map_location="cpu", weights_only=True)
    assert ck2["global_step"] == 6 and ck2["ema"]["num_updates"] == 6 and ck2["lr_schedulers"][0]["t2_schedule"] == sch["t2_schedule"]
    # say --ema: another log-mel than say, and bit for bit say's on a copy whose state_dict is the shadow weights
    a, b, c = tmp_path / "live.npy", tmp_path / "ema.npy", tmp_path / "copy.npy"
    _say(cfg, res / "final.ckpt", a)
    _say(cfg, res / "final.ckpt", b, "--ema")
    swapped = dict(ck, state_dict=ck["ema_state_dict"])
    del swapped["ema_state_dict"], swapped["ema"]
    torch.save(swapped, tmp_path / "swapped.ckpt")
    _say(cfg, tmp_path / "swapped.ckpt", c)
    live, ema, copy = np.load(a), np.load(b), np.load(c)
    assert np.isfinite(ema).all() and ema.shape[1] == 80 and ema.shape[0] >= 2 and live.shape[0] >= 2 and ema.any() and live.any()
    assert live.shape != ema.shape or not np.array_equal(live, ema)
    assert copy.shape == ema.shape and np.array_equal(copy.view(np.int32), ema.view(np.int32))
    # no shadow weights in the file: an error that names it
    bad = _say(cfg, tmp_path / "swapped.ckpt", tmp_path / "none.npy", "--ema", ok=False)
    assert "swapped.ckpt" in bad.stderr and "EMA" in bad.stderr and not os.path.exists(tmp_path / "none.npy")
