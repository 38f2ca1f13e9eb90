"""`say --text-file` on the weights of the reference-generated `infer` fixture: the document is split, decoded in
chunks, vocoded, joined by analysis.join_audio and written as one .wav.  Every decode is bounded by --max-len 40."""
import importlib.util
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"
# two paragraphs, five sentences, the second one above --max-chars 40, and a line that cleans to nothing
TEXT = ("Dr. Smith came. He stayed for a long while; then, quite late, he left again.\n"
        "Was it so?\n\n***\n\nThe 2nd part. It ends here!\n")
PIECES = [("Dr. Smith came.", 0, "sentence"), ("He stayed for a long while; then,", 0, "clause"), ("quite late, he left again.", 0, "sentence"),
          ("Was it so?", 0, "paragraph"), ("The 2nd part.", 2, "sentence"), ("It ends here!", 2, "end")]
SR = 22050
PAUSE = dict(sentence=round(0.25 * SR), clause=round(0.12 * SR), paragraph=round(0.60 * SR), end=0)


def _setup(root):
    from helpers import load_golden, params_from
    z = load_golden("infer")
    sd = {"tacotron2." + k: v for k, v in params_from(z).items()}
    hp = dict(lr=1e-3, weight_decay=1e-6, num_chars=39, encoded_dim=32, num_mels=16, prenet_dim=16, att_rnn_dim=32, att_dim=16,
              rnn_hidden_dim=32, postnet_dim=32, dropout=0.5)
    ck = root / "m.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hp, "global_step": 0, "epoch": 0}, ck)
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv", "test": "none.csv",
                       "preprocessing": {"allowed_chars": ALLOWED, "expand_abbreviations": True, "end_token": "^", "num_mels": 16}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "args": {"max_steps": 6}},
           "model": {"scheduler_milestones": [], "args": {"prenet_dim": 16, "att_rnn_dim": 32, "att_dim": 16, "rnn_hidden_dim": 32,
                                                          "postnet_dim": 32, "dropout": 0.5, "char_embedding_dim": 32}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    cfgp = root / "cfg.json"
    cfgp.write_text(json.dumps(cfg))
    doc = root / "doc.txt"
    doc.write_text(TEXT, encoding="utf-8")
    return cfg, cfgp, ck, doc


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from helpers import write_hifigan_checkpoint
    root = tmp_path_factory.mktemp("saydoc")
    cfg, cfgp, ck, doc = _setup(root)
    return dict(root=root, cfg=cfg, cfgp=cfgp, ck=ck, doc=doc, hifi=write_hifigan_checkpoint(str(root / "hifi"), n_mels=16))


def _kw(setup, vocoder, **more):
    cfg = setup["cfg"]
    kw = dict(dataset_config=cfg["dataset"], training_config=cfg["training"], model_config=cfg["model"], extensions_config=cfg["extensions"],
              device=0, checkpoint=str(setup["ck"]), text_file=str(setup["doc"]), random_seed=3, max_len=40, max_chars=40)
    if vocoder == "hifi_gan":
        kw["hifi_gan_checkpoint"] = setup["hifi"]
    return dict(kw, **more)


def _read(path):
    with wave.open(str(path), "rb") as w:
        return w.getframerate(), w.getnframes(), w.readframes(w.getnframes())


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifi_gan"])
def test_the_document_is_split_decoded_joined_and_written(setup, tmp_path, monkeypatch, capsys, vocoder):
    from tacotron2_amd import analysis, vocoder as V
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.model.tts_model import TTSModel
    from tacotron2_amd.run.say import do_say_document
    decodes = []
    forward = TTSModel.forward

    def recording(self, *a, **k):
        out = forward(self, *a, **k)
        decodes.append((k["chars_idx_len"].cpu().tolist(), out[2].detach().cpu().numpy()))
        return out
    monkeypatch.setattr(TTSModel, "forward", recording)
    dur = tmp_path / "dur.json"
    y, plan, info = do_say_document(output=str(tmp_path / "a.wav"), durations_out=str(dur), **_kw(setup, vocoder))
    assert [tuple(p) for p in info["pieces"]] == PIECES and info["chunks"] == 1 and len(decodes) == 1
    # the WAV is write_wav of join_audio over the per-piece waveforms, with the pauses the breaks imply and the driver's settings
    n = [int(w.numel()) for w in info["waveforms"]]
    assert n == info["n"] and all(k > 0 for k in n)
    if vocoder == "hifi_gan":
        assert n == [f * 256 for f in info["frames"]]                          # the padded batch's rows cut at frames * 256
    buf = torch.zeros(len(n), max(n) + 3, device="cuda:0")
    for i, w in enumerate(info["waveforms"]):
        buf[i, :n[i]] = w
    pause = [PAUSE[b] for _, _, b in PIECES]
    want, total, plan2 = analysis.join_audio(buf, n, pause, trim=True, top_db=60.0, frame_length=2048, hop_length=512, keep=441, fade=110,
                                             level=False, ceiling=0.0)
    assert torch.equal(want, y) and total == y.numel() and all(torch.equal(plan[k], plan2[k]) for k in plan)
    V.write_wav(str(tmp_path / "want.wav"), want, SR)
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "want.wav").read_bytes() and _read(tmp_path / "a.wav")[:2] == (SR, total)
    # the JSON: one object per surviving piece, in order
    recs = json.loads(dur.read_text())
    enc = TextEncoder(ALLOWED, "^")
    assert [(r["piece"], r["text"], r["paragraph"]) for r in recs] == [(i, t, p) for i, (t, p, _) in enumerate(PIECES)]
    off, s0, ln, gain = (plan[k].cpu().tolist() for k in ("off", "s0", "len", "gain"))
    assert off == sorted(off) and gain == [1.0] * len(PIECES)
    for i, r in enumerate(recs):
        assert r["symbols"] == list(enc.clean(PIECES[i][0])) and sum(r["frames"]) == info["frames"][i]
        assert (r["offset_s"], r["trim_start_s"], r["length_s"], r["pause_s"], r["gain"]) == (off[i] / SR, s0[i] / SR, ln[i] / SR, pause[i] / SR, 1.0)
        lo, hi = r["offset_s"], r["offset_s"] + r["length_s"]
        assert all(lo <= a <= b <= hi + 1e-12 for a, b in zip(r["start_s"], r["end_s"])) and len(r["start_s"]) == len(r["symbols"])
        assert r["start_s"][1:] == r["end_s"][:-1] and isinstance(r["feasible"], bool) and isinstance(r["focus_rate"], float)
    assert [r["offset_s"] for r in recs] == sorted(r["offset_s"] for r in recs)
    # stopped agrees with the gate mask of the one decode: the pieces went in sorted by encoded length
    lens, gates = decodes[0]
    order = sorted(range(len(PIECES)), key=lambda i: (len(enc.encode(PIECES[i][0])), i))
    assert lens == [len(enc.encode(PIECES[i][0])) for i in order] and gates.shape[1] <= 40
    for k, i in enumerate(order):
        valid = int((gates[k, :, 0] != -1000.0).sum())
        assert recs[i]["stopped"] == info["stopped"][i] == (valid < gates.shape[1])
        assert info["frames"][i] == max(min(valid, gates.shape[1] - 1), 1)
    cap = capsys.readouterr()
    assert f"say: {len(PIECES)} pieces in 1 chunks" in cap.out
    for i, ok in enumerate(info["stopped"]):                                     # a piece cut at --max-len is reported, not an error
        assert ok or f"piece {i} did not stop within --max-len 40" in cap.err and repr(PIECES[i][0][:40]) in cap.err

    # --batch-size 2: the same pieces in the same order, in three decodes.  The audio may differ from the run above - the prenet's
    # dropout mask depends on the row of the batch a piece is decoded in - so only the structure is compared.
    del decodes[:]
    y2, plan2, info2 = do_say_document(output=str(tmp_path / "b.wav"), durations_out=str(dur), batch_size=2, **_kw(setup, vocoder))
    assert info2["pieces"] == info["pieces"] and info2["chunks"] == 3 == len(decodes) and [len(d[0]) for d in decodes] == [2, 2, 2]
    assert [r["text"] for r in json.loads(dur.read_text())] == [t for t, _, _ in PIECES] and _read(tmp_path / "b.wav")[1] == y2.numel() > 0

    # --out-sample-rate: one resampling of the joined waveform, the header at 16000
    if vocoder == "griffin_lim":
        y3, plan3, info3 = do_say_document(output=str(tmp_path / "c.wav"), out_sample_rate=16000, **_kw(setup, vocoder))
        total3 = int(plan3["off"][-1]) + int(plan3["len"][-1])
        rate, frames, _ = _read(tmp_path / "c.wav")
        assert rate == 16000 and frames == -(-total3 * 320 // 441) == y3.numel()
        with pytest.raises(ValueError, match="text-file needs a .wav target"):
            do_say_document(output=str(tmp_path / "c.npy"), **_kw(setup, vocoder))


def test_the_module_api_takes_a_text_and_loads_nothing(setup):
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.model.tts_model import TTSModel
    model = TTSModel.load_from_checkpoint(str(setup["ck"]), device=torch.device("cuda:0"))
    model.eval()
    y, plan, info = model.say_document("One. Two, three.", TextEncoder(ALLOWED, "^"), max_len=20, level=True, fade_ms=2.0)
    assert [p.text for p in info["pieces"]] == ["One.", "Two, three."] and y.is_cuda and y.dim() == 1
    assert y.numel() == int(plan["off"][-1]) + int(plan["len"][-1]) and float(y.abs().max()) <= 1.0 + 2.0 ** -22
    assert info["join"]["ceiling"] == 1.0 and info["join"]["fade"] == 44 and info["pause"] == [round(0.25 * SR), 0]
    with pytest.raises(ValueError, match="nothing to say"):
        model.say_document("*** ###", TextEncoder(ALLOWED, "^"))


def test_cli_say_text_file(setup, tmp_path):
    doc = tmp_path / "n.txt"
    doc.write_text("It cost 3 pounds. The 2nd was 50% more!\n\nDone.\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint",
                        str(setup["ck"]), "--text-file", str(doc), "--out", str(tmp_path / "o.wav"), "--max-len", "40", "--expand-numbers",
                        "--level", "--durations-out", str(tmp_path / "d.json"), "--random-seed", "3"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rate, frames, pcm = _read(tmp_path / "o.wav")
    assert rate == SR and frames > 0 and len(pcm) == 2 * frames and "3 pieces in 1 chunks" in r.stdout
    recs = json.loads((tmp_path / "d.json").read_text())
    assert [x["text"] for x in recs] == ["It cost three pounds.", "The second was fifty percent more!", "Done."]
    assert [x["paragraph"] for x in recs] == [0, 0, 1]


def _main():
    spec = importlib.util.spec_from_file_location("t2_main_cli", os.path.join(ROOT, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.main


def test_usage_errors_name_the_option(setup, tmp_path):
    from click.testing import CliRunner
    head = ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"])]
    doc = ["--text-file", str(setup["doc"])]
    cases = [(["--text", "Hi.", *doc, "--out", "o.wav"], "--text-file"), ([], "--text-file"), (["--text", "Hi.", "--pause", "0.1,0.1,0.1"], "--pause"),
             ([*doc, "--out", str(tmp_path / "o.npy")], "--text-file"), ([*doc, "--out", "o.wav", "--batch-size", "65"], "--batch-size"),
             ([*doc, "--out", "o.wav", "--batch-size", "0"], "--batch-size"), (["--text", "Hi.", "--level"], "--level"),
             (["--text", "Hi.", "--max-chars", "50"], "--max-chars"), ([*doc, "--out", "o.wav", "--pause", "1,2"], "--pause"),
             ([*doc, "--out", "o.wav", "--fade-ms", "-1"], "--fade-ms"), (["--text", "Hi.", "--max-len", "0"], "--max-len")]
    main = _main()
    for args, name in cases:
        r = CliRunner().invoke(main, head + args)
        assert r.exit_code == 2 and name in r.output and "Usage:" in r.output, (args, r.exit_code, r.output, r.exception)
    assert not (tmp_path / "o.npy").exists()


def test_say_text_is_what_do_say_writes_at_max_len_5000(setup, tmp_path):
    """The new --max-len option defaults to what do_say always took: `say --text` writes the same bytes as before."""
    from click.testing import CliRunner
    from tacotron2_amd.run.say import do_say
    r = CliRunner().invoke(_main(), ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"]), "--text", "Hi there.",
                                     "--out", str(tmp_path / "cli.npy"), "--random-seed", "3"])
    assert r.exit_code == 0, (r.output, r.exception)
    cfg = setup["cfg"]
    do_say(dataset_config=cfg["dataset"], training_config=cfg["training"], model_config=cfg["model"], extensions_config=cfg["extensions"],
           device=0, checkpoint=str(setup["ck"]), text="Hi there.", output=str(tmp_path / "api.npy"), random_seed=3, max_len=5000)
    assert (tmp_path / "cli.npy").read_bytes() == (tmp_path / "api.npy").read_bytes() and len(np.load(tmp_path / "api.npy")) > 0
