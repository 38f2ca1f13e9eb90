"""`main.py test --score [--no-audio]` on the GPU: a three-utterance manifest of generated WAVs (the way tests/test_gpu_cli.py builds
its inputs), the weights of the reference-generated `infer` fixture (small dims; utterances stop within a few frames).  scores.csv
against TTSModel.score on the same batch, scores.json against the CSV, a failure row under a tiny --max-len, and the plain `test`
untouched.  The command runs through its click entry in this process (option parsing, config, driver, decode; no interpreter
start)."""
import json
import math
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"
TEXTS = ["Hi there.", "A somewhat longer sentence, Dr. Who!", "Testing: one; two? three."]
HEADER = "i|wav|n_chars|ref_frames|syn_frames|stopped|mcd_dtw|path_len|dur_ratio|focus_rate"


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from tests.helpers import load_golden, params_from
    tmp = tmp_path_factory.mktemp("score")
    sr = 22050
    speech = tmp / "wavs"
    speech.mkdir()
    rng = np.random.default_rng(0)
    rows = ["text|wav|speaker_id"]
    for i, t in enumerate(TEXTS):
        k = sr // 8 + 997 * i
        x = 0.3 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(k) / sr) + 0.01 * rng.normal(size=k)
        with wave.open(str(speech / f"u{i}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes((x * 32767).astype("<i2").tobytes())
        rows.append(f"{t}|u{i}.wav|0")
    csvp = tmp / "test.csv"
    csvp.write_text("\n".join(rows) + "\n")
    sd = {"tacotron2." + k: v for k, v in params_from(load_golden("infer")).items()}
    hp = dict(lr=1e-3, weight_decay=1e-6, num_chars=39, encoded_dim=32, num_mels=16, prenet_dim=16, att_rnn_dim=32, att_dim=16,
              rnn_hidden_dim=32, postnet_dim=32, dropout=0.5)
    ck = tmp / "m.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hp, "global_step": 0, "epoch": 0}, ck)
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv", "test": str(csvp),
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "num_mels": 16,
                                         "silence": 512, "trim": False}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "args": {"max_steps": 6}},
           "model": {"scheduler_milestones": [], "args": {"prenet_dim": 16, "att_rnn_dim": 32, "att_dim": 16, "rnn_hidden_dim": 32,
                                                          "postnet_dim": 32, "dropout": 0.5, "char_embedding_dim": 32}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    cfgp = tmp / "cfg.json"
    cfgp.write_text(json.dumps(cfg))
    return dict(tmp=tmp, speech=speech, ck=ck, cfgp=cfgp, cfg=cfg, samples=[sr // 8 + 997 * i for i in range(3)])


def _test_cmd(s, res, extra, speech=None):
    from click.testing import CliRunner
    import main as cli
    return CliRunner().invoke(cli.main, ["--config", str(s["cfgp"]), "--device", "0", "test", "--speech-dir", str(speech or s["speech"]),
                                         "--checkpoint", str(s["ck"]), "--results-dir", str(res), "--batch-size", "3", "--max-len",
                                         "40"] + extra, obj={})


def _rows(res):
    lines = (res / "scores.csv").read_text().splitlines()
    assert lines[0] == HEADER
    return [dict(zip(HEADER.split("|"), l.split("|"))) for l in lines[1:]]


def _expected(s, max_len=40):
    """TTSModel.score on the manifest as ONE batch, the recordings through the dataset's item path."""
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.datasets.tts_dataset import TTSDataset
    from tacotron2_amd.run.test import load_test_model
    dev = torch.device("cuda:0")
    cfg = s["cfg"]
    model = load_test_model(cfg["dataset"], cfg["training"], cfg["model"], cfg["extensions"], str(s["ck"]), dev)
    enc = TextEncoder(ALLOWED, "^", True)
    ids = [torch.tensor(enc.encode(t)) for t in TEXTS]
    ds = TTSDataset(filenames=[f"u{i}.wav" for i in range(3)], texts=TEXTS, base_dir=str(s["speech"]), device=dev,
                    **dict(cfg["dataset"]["preprocessing"], cache=False))
    refs = [ds[i][0]["mel_spectrogram"] for i in range(3)]
    assert [len(r) for r in refs] == [1 + (n + 512) // 256 for n in s["samples"]]           # samples after the silence pad
    _, sc = model.score(torch.nn.utils.rnn.pad_sequence(ids, batch_first=True).to(dev), torch.tensor([len(i) for i in ids], device=dev),
                        torch.nn.utils.rnn.pad_sequence(refs, batch_first=True), torch.tensor([len(r) for r in refs], device=dev),
                        max_len_override=max_len)
    return {k: v.cpu().tolist() for k, v in sc.items()}, [len(i) for i in ids]


def _check_json(res, rows, max_len=40):
    agg = json.loads((res / "scores.json").read_text())
    ok = [r for r in rows if r["stopped"] == "1"]
    assert agg["n"] == len(rows) == 3 and agg["n_stopped"] == len(ok) and abs(agg["failure_rate"] - (1 - len(ok) / 3)) < 1e-12
    assert agg["settings"] == {"n_ceps": 13, "attention_window": None, "forward_attention": False, "stop_threshold": 0.5, "r": 1,
                               "max_len": max_len}
    assert abs(agg["focus_rate_mean"] - np.mean([float(r["focus_rate"]) for r in rows])) < 1e-5
    if ok:
        mcds = [float(r["mcd_dtw"]) for r in ok]
        assert abs(agg["mcd_dtw_mean"] - np.mean(mcds)) < 1e-5 and abs(agg["mcd_dtw_median"] - np.median(mcds)) < 1e-5
        assert abs(agg["abs_log_dur_ratio_mean"] - np.mean([abs(math.log(int(r["syn_frames"]) / int(r["ref_frames"]))) for r in ok])) < 1e-5
    else:
        assert agg["mcd_dtw_mean"] is None and agg["mcd_dtw_median"] is None and agg["abs_log_dur_ratio_mean"] is None
    return agg


def test_score_no_audio_writes_the_scores_of_ttsmodel_score(setup):
    s = setup
    res = s["tmp"] / "res_noaudio"
    r = _test_cmd(s, res, ["--score", "--no-audio"])
    assert r.exit_code == 0, (r.output, r.exception)
    want, n_chars = _expected(s)
    rows = _rows(res)
    print("scores.csv:", rows)
    assert len(rows) == 3 and any(want["stopped"])
    fails = set()
    for k, row in enumerate(rows):
        assert row["i"] == str(k + 1) and row["wav"] == f"u{k}.wav" and int(row["n_chars"]) == n_chars[k]
        assert int(row["ref_frames"]) == want["ref_frames"][k] and int(row["syn_frames"]) == want["syn_frames"][k]
        assert row["stopped"] == ("1" if want["stopped"][k] else "0") and int(row["path_len"]) == want["path_len"][k]
        assert abs(float(row["focus_rate"]) - want["focus_rate"][k]) <= 1e-6
        if want["stopped"][k]:
            assert abs(float(row["mcd_dtw"]) - want["mcd"][k]) <= 1e-6 and float(row["mcd_dtw"]) > 0
            assert abs(float(row["dur_ratio"]) - want["syn_frames"][k] / want["ref_frames"][k]) <= 1e-6
            assert max(want["syn_frames"][k], want["ref_frames"][k]) <= int(row["path_len"]) < want["syn_frames"][k] + want["ref_frames"][k]
        else:
            assert row["mcd_dtw"] == "" and row["dur_ratio"] == "" and row["path_len"] == "0"
            fails.add(k + 1)
    _check_json(res, rows)
    assert sorted(os.listdir(res)) == sorted(["scores.csv", "scores.json"] + (["failures.csv"] if fails else []))


def test_score_with_audio_adds_the_scores_to_the_plain_outputs(setup):
    s = setup
    plain, scored = s["tmp"] / "res_plain", s["tmp"] / "res_scored"
    r = _test_cmd(s, plain, [], speech="unused")              # without --score no recording is read: the directory need not exist
    assert r.exit_code == 0, (r.output, r.exception)
    r = _test_cmd(s, scored, ["--score"])
    assert r.exit_code == 0, (r.output, r.exception)
    files = sorted(os.listdir(plain))
    assert files and set(files) <= {"1.wav", "2.wav", "3.wav", "failures.csv"}          # what `test` wrote before this option existed
    assert sorted(os.listdir(scored)) == sorted(files + ["scores.csv", "scores.json"])
    for f in files:
        assert (plain / f).read_bytes() == (scored / f).read_bytes(), f
    rows = _rows(scored)
    assert rows == _rows(s["tmp"] / "res_noaudio") if (s["tmp"] / "res_noaudio").exists() else len(rows) == 3
    _check_json(scored, rows)


def test_score_an_utterance_that_misses_its_stop_is_a_failure_row(setup):
    s = setup
    res = s["tmp"] / "res_short"
    r = _test_cmd(s, res, ["--score", "--no-audio", "--max-len", "1"])      # one frame: no utterance reaches a stop
    assert r.exit_code == 0, (r.output, r.exception)
    rows = _rows(res)
    assert len(rows) == 3
    for k, row in enumerate(rows):
        assert row["stopped"] == "0" and row["mcd_dtw"] == "" and row["syn_frames"] == "0" and row["path_len"] == "0"
        assert int(row["ref_frames"]) == 1 + (s["samples"][k] + 512) // 256 and 0 < float(row["focus_rate"]) <= 1
    agg = _check_json(res, rows, max_len=1)
    assert agg["n_stopped"] == 0 and agg["failure_rate"] == 1.0
    assert [l.split("|")[0] for l in (res / "failures.csv").read_text().splitlines()] == ["1", "2", "3"]


def test_score_a_missing_recording_is_named_before_any_decoding(setup):
    s = setup
    res = s["tmp"] / "res_missing"
    other = s["tmp"] / "wavs2"
    other.mkdir()
    for i in (0, 2):
        (other / f"u{i}.wav").write_bytes((s["speech"] / f"u{i}.wav").read_bytes())
    r = _test_cmd(s, res, ["--score", "--no-audio"], speech=other)
    assert r.exit_code != 0 and isinstance(r.exception, FileNotFoundError) and "u1.wav" in str(r.exception)
    assert not res.exists()
