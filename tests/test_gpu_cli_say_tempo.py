"""`say --tempo / --pitch-shift` on the weights of the reference-generated `infer` fixture: the vocoded waveform goes
through analysis.time_stretch / pitch_shift before it is written; in document mode the whole piece buffer does, in one launch in front
of the join.  Every decode is bounded by --max-len 40; two runs with one seed decode the same frames."""
import importlib.util
import json
import os
import wave

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOWED = "!'(),.:;? \\-abcdefghijklmnopqrstuvwxyz"
SR = 22050
DEV = "cuda:0"
DOC = "One came. Two stayed, three left!\n\nIt ends here.\n"


def _setup(root):
    """A checkpoint of the `infer` fixture's weights and the config that goes with it."""
    from helpers import load_golden, params_from
    sd = {"tacotron2." + k: v for k, v in params_from(load_golden("infer")).items()}
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
    return cfg, cfgp, ck


def _main():
    spec = importlib.util.spec_from_file_location("t2_main_cli", os.path.join(ROOT, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.main


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from helpers import write_hifigan_checkpoint
    root = tmp_path_factory.mktemp("saytempo")
    cfg, cfgp, ck = _setup(root)
    doc = root / "three.txt"
    doc.write_text(DOC, encoding="utf-8")
    return dict(root=root, cfg=cfg, cfgp=cfgp, ck=ck, doc=doc, hifi=write_hifigan_checkpoint(str(root / "hifi"), n_mels=16))


def _kw(setup, vocoder, **more):
    cfg = setup["cfg"]
    kw = dict(dataset_config=cfg["dataset"], training_config=cfg["training"], model_config=cfg["model"], extensions_config=cfg["extensions"],
              device=0, checkpoint=str(setup["ck"]), random_seed=3, max_len=40)
    if vocoder == "hifi_gan":
        kw["hifi_gan_checkpoint"] = setup["hifi"]
    return dict(kw, **more)


def _frames(path):
    with wave.open(str(path), "rb") as w:
        return w.getframerate(), w.getnframes()


@pytest.fixture
def written(monkeypatch):
    """The float waveforms that reach vocoder.write_wav, by file name."""
    from tacotron2_amd import vocoder as V
    seen = {}
    write = V.write_wav

    def recording(name, wav, rate):
        seen[str(name)] = torch.as_tensor(wav).detach().float().reshape(-1).cpu().clone()
        return write(name, wav, rate)
    monkeypatch.setattr(V, "write_wav", recording)
    return seen


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifi_gan"])
def test_say_tempo_is_time_stretch_of_the_plain_run(setup, tmp_path, written, vocoder):
    from tacotron2_amd import analysis, vocoder as V
    from tacotron2_amd.run.say import do_say
    a, b, c = (str(tmp_path / f"{k}.wav") for k in "abc")
    do_say(text="Hi there.", output=a, durations_out=str(tmp_path / "a.json"), **_kw(setup, vocoder))
    do_say(text="Hi there.", output=b, durations_out=str(tmp_path / "b.json"), tempo=0.8, **_kw(setup, vocoder))
    x = written[a]
    n = x.numel()
    assert n > 0 and written[b].numel() == -(-n * 1000 // 800) == _frames(b)[1] and _frames(b)[0] == SR
    y, n_out, pos = analysis.time_stretch(x.to(DEV)[None, :], [n], 0.8)
    assert torch.equal(written[b], y[0, :n_out[0]].cpu())
    V.write_wav(str(tmp_path / "want.wav"), y[0, :n_out[0]].cpu(), SR)
    assert (tmp_path / "b.wav").read_bytes() == (tmp_path / "want.wav").read_bytes()
    # the times: the nominal map, and the two new fields
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text())[0] for k in "ab")
    assert "tempo" not in ra and "pitch_shift_semitones" not in ra
    assert (rb["tempo"], rb["pitch_shift_semitones"]) == (0.8, 0.0) and rb["frames"] == ra["frames"] and rb["symbols"] == ra["symbols"]
    assert rb["start_s"] == [t / 0.8 for t in ra["start_s"]] and rb["end_s"] == [t / 0.8 for t in ra["end_s"]]
    # pitch and tempo together, then the output rate: pitch_shift of the plain run's waveform, resampled once more
    do_say(text="Hi there.", output=c, tempo=1.25, pitch_shift=3, out_sample_rate=16000, **_kw(setup, vocoder))
    z, nz, eff, sr_mid = analysis.pitch_shift(x.to(DEV)[None, :], [n], 3.0, SR, 1.25)
    assert sr_mid == 26200 and abs(eff - 1.25) < 1e-3 and abs(nz[0] - n / 1.25) <= 2e-3 * n / 1.25 + 1
    want, nw = analysis.resample(z[:, :nz[0]].contiguous(), nz, SR, 16000)
    assert torch.equal(written[c], want[0, :nw[0]].cpu()) and _frames(c) == (16000, nw[0])


def test_the_corner_of_both_ranges_and_two_texts_in_one_launch(setup, tmp_path, written, monkeypatch):
    """--tempo 2 --pitch-shift -12 at 22 050 Hz needs a stretch by 4.009, past time_stretch's own range: the driver runs it through
    pitch_shift.  Two texts go through ONE t2_stretch launch, each row what it is alone."""
    from click.testing import CliRunner
    from tacotron2_amd import analysis, stretch
    from tacotron2_amd.run.say import do_say
    texts = ["Hi there.", "One came, two stayed."]
    do_say(text=texts, output=str(tmp_path / "a.wav"), **_kw(setup, "griffin_lim"))
    launches = []
    call = stretch.call
    monkeypatch.setattr(stretch, "call", lambda name, *a: (launches.append(name), call(name, *a))[1])
    do_say(text=texts, output=str(tmp_path / "b.wav"), tempo=2.0, pitch_shift=-12, **_kw(setup, "griffin_lim"))
    assert launches == ["t2_stretch"]
    for i in range(2):
        x = written[str(tmp_path / f"a_{i}.wav")]
        n = x.numel()
        z, nz, eff, sr_mid = analysis.pitch_shift(x.to(DEV)[None, :], [n], -12.0, SR, 2.0)
        assert sr_mid == 11000 and abs(eff - 2.0) < 1e-3 * 2.0 and abs(nz[0] - n / 2.0) <= 2e-3 * n / 2.0 + 1
        assert torch.equal(written[str(tmp_path / f"b_{i}.wav")], z[0, :nz[0]].cpu()) and _frames(tmp_path / f"b_{i}.wav") == (SR, nz[0])
    r = CliRunner().invoke(_main(), [
        "--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"]), "--max-len", "40", "--random-seed", "3",
        "--text-file", str(setup["doc"]), "--out", str(tmp_path / "doc.wav"), "--tempo", "0.5", "--pitch-shift", "12"])
    assert r.exit_code == 0 and _frames(tmp_path / "doc.wav")[1] > 0, (r.output, r.exception)


def test_tempo_one_and_no_shift_launch_nothing_and_write_the_same_bytes(setup, tmp_path, monkeypatch):
    from click.testing import CliRunner
    from tacotron2_amd import stretch
    monkeypatch.setattr(stretch, "call", lambda *a: pytest.fail("--tempo 1 --pitch-shift 0 must launch nothing"))
    head = ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"]), "--max-len", "40", "--random-seed", "3"]
    main = _main()
    for name, more in (("plain", []), ("unit", ["--tempo", "1", "--pitch-shift", "0"])):
        r = CliRunner().invoke(main, head + ["--text", "Hi there.", "--out", str(tmp_path / f"{name}.wav")] + more)
        assert r.exit_code == 0, (r.output, r.exception)
        r = CliRunner().invoke(main, head + ["--text-file", str(setup["doc"]), "--out", str(tmp_path / f"{name}_doc.wav")] + more)
        assert r.exit_code == 0, (r.output, r.exception)
    assert (tmp_path / "plain.wav").read_bytes() == (tmp_path / "unit.wav").read_bytes() and _frames(tmp_path / "plain.wav")[1] > 0
    assert (tmp_path / "plain_doc.wav").read_bytes() == (tmp_path / "unit_doc.wav").read_bytes()


def test_a_document_at_tempo_1_25(setup, tmp_path):
    from tacotron2_amd import analysis
    from tacotron2_amd.run.say import do_say_document
    kw = _kw(setup, "hifi_gan", text_file=str(setup["doc"]))
    _, plan0, base = do_say_document(output=str(tmp_path / "a.wav"), durations_out=str(tmp_path / "a.json"), **kw)
    y, plan, info = do_say_document(output=str(tmp_path / "b.wav"), durations_out=str(tmp_path / "b.json"), tempo=1.25, **kw)
    assert [p.text for p in info["pieces"]] == ["One came.", "Two stayed, three left!", "It ends here."] and info["chunks"] == 1
    assert info["voice"].tempo == 1.25 and info["voice"].ratio == (1250, 1000) and base["voice"] is None
    # the pieces: ONE time_stretch call over the padded buffer of the plain run's pieces
    n0 = base["n"]
    assert info["n"] == [-(-k * 1000 // 1250) for k in n0] and info["frames"] == base["frames"]
    buf = torch.zeros(3, max(n0), device=DEV)
    for i, w in enumerate(base["waveforms"]):
        buf[i, :n0[i]] = w
    s, ns, _ = analysis.time_stretch(buf, n0, 1.25)
    assert all(torch.equal(info["waveforms"][i], s[i, :ns[i]]) for i in range(3))
    # the pauses: divided by the tempo
    assert base["pause"] == [round(0.25 * SR), round(0.60 * SR), 0] and info["pause"] == [round(0.25 * SR / 1.25), round(0.60 * SR / 1.25), 0]
    # the total: what the plan says, and what is in the file
    off, s0, ln = (plan[k].cpu().tolist() for k in ("off", "s0", "len"))
    assert y.numel() == off[-1] + ln[-1] == sum(ln) + sum(info["pause"]) and _frames(tmp_path / "b.wav") == (SR, y.numel())
    assert off == [0, ln[0] + info["pause"][0], ln[0] + info["pause"][0] + ln[1] + info["pause"][1]]
    assert all(0 < ln[i] <= info["n"][i] for i in range(3))
    # the times: piece-local ones scaled before they meet the join's plan
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text()) for k in "ab")
    for i in range(3):
        local, local0 = info["durations"][i], base["durations"][i]
        assert local["end_s"] == [t / 1.25 for t in local0["end_s"]] and local["start_s"] == [t / 1.25 for t in local0["start_s"]]
        r = rb[i]
        assert (r["tempo"], r["pitch_shift_semitones"]) == (1.25, 0.0) and "tempo" not in ra[i] and r["frames"] == ra[i]["frames"]
        assert (r["offset_s"], r["trim_start_s"], r["length_s"], r["pause_s"]) == (off[i] / SR, s0[i] / SR, ln[i] / SR, info["pause"][i] / SR)
        doc = lambda t: off[i] / SR + min(max(t - s0[i] / SR, 0.0), ln[i] / SR)
        assert r["end_s"] == [doc(t) for t in local["end_s"]] and r["start_s"] == [doc(t) for t in local["start_s"]]
        assert r["end_s"][-1] <= (off[i] + ln[i]) / SR + 1e-12


def test_usage_errors_name_the_option(setup, tmp_path):
    from click.testing import CliRunner
    head = ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"])]
    text, doc = ["--text", "Hi."], ["--text-file", str(setup["doc"])]
    npy = str(tmp_path / "o.npy")
    cases = [([*text, "--out", "o.wav", "--tempo", "0.4"], "--tempo"), ([*text, "--out", "o.wav", "--tempo", "2.5"], "--tempo"),
             ([*text, "--out", "o.wav", "--tempo", "nan"], "--tempo"), ([*text, "--out", "o.wav", "--tempo", "fast"], "--tempo"),
             ([*text, "--out", "o.wav", "--pitch-shift", "13"], "--pitch-shift"), ([*doc, "--out", "o.wav", "--pitch-shift", "-12.5"], "--pitch-shift"),
             ([*doc, "--out", "o.wav", "--tempo", "0"], "--tempo"), ([*text, "--out", npy, "--tempo", "0.8"], "--tempo"),
             ([*text, "--out", npy, "--pitch-shift", "2"], "--pitch-shift"), ([*text, "--out", npy, "--tempo", "1"], "--tempo")]
    main = _main()
    for args, name in cases:
        r = CliRunner().invoke(main, head + args)
        assert r.exit_code == 2 and name in r.output and "Usage:" in r.output, (args, r.exit_code, r.output, r.exception)
    assert not (tmp_path / "o.npy").exists()
    from tacotron2_amd.run.say import do_say
    with pytest.raises(ValueError, match="--tempo and --pitch-shift need a .wav target"):
        do_say(text="Hi.", output=npy, tempo=0.8, **_kw(setup, "griffin_lim"))
    with pytest.raises(ValueError, match="--pitch-shift must lie in -12 .. 12"):
        do_say(text="Hi.", output=str(tmp_path / "o.wav"), pitch_shift=12.5, **_kw(setup, "griffin_lim"))
