"""`say --loudness / --true-peak` on the weights of the reference-generated `infer` fixture: the samples that would be
written go through ONE analysis.normalize_loudness call as the last step - behind the voice chain, the join and --out-sample-rate, at
the rate of the header.  The random HiFi-GAN generator of tests/helpers.py ends at about 1e-5 of full scale, -94 dBFS, below BS.1770's
absolute gate of -70 LUFS; its last layer's gain is raised here (LOUDER) until the rows are audible.  Griffin-Lim of this fixture's few
frames is digital silence and so covers the row without a loudness.  Every decode is bounded by --max-len 40; two runs with one seed decode the same frames."""
import json
import math

import pytest
import torch

from test_gpu_cli_say_tempo import DEV, SR, _frames, _kw, _main, _setup  # noqa: F401  (the same checkpoint, config and helpers)

pytestmark = pytest.mark.gpu
DOC = "One came. Two stayed, three left!\n\nIt ends here.\n"
LOUDER = 2.0e4                  # on conv_post's weight-norm gain: the pre-tanh output, about 1e-5, comes to some tenths of full scale


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from helpers import write_hifigan_checkpoint
    root = tmp_path_factory.mktemp("sayloud")
    cfg, cfgp, ck = _setup(root)
    doc = root / "three.txt"
    doc.write_text(DOC, encoding="utf-8")
    hifi = write_hifigan_checkpoint(str(root / "hifi"), n_mels=16)
    sd = torch.load(hifi, map_location="cpu", weights_only=True)
    sd["generator"]["conv_post.weight_g"] *= LOUDER
    torch.save(sd, hifi)
    return dict(root=root, cfg=cfg, cfgp=cfgp, ck=ck, doc=doc, hifi=hifi)


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


@pytest.fixture
def launches(monkeypatch):
    """The library calls of the model-free audio modules, by name and in order."""
    from tacotron2_amd import analysis, join, loudness, psola, stretch
    from tacotron2_amd.datasets import resample
    seen = []
    for mod in (stretch, analysis, psola, join, loudness, resample):
        call = mod.call
        monkeypatch.setattr(mod, "call", lambda name, *a, _call=call: (seen.append(name), _call(name, *a))[1])
    return seen


def _normalized(x, rate, target, ceiling=-1.0):
    """analysis.normalize_loudness of one host waveform as one row: (the samples, the stats as host numbers)."""
    from tacotron2_amd import analysis
    y, stats = analysis.normalize_loudness(x.to(DEV)[None, :], [x.numel()], rate, target=target, ceiling=ceiling)
    return y[0].cpu(), {k: v[0].item() for k, v in stats.items()}


def test_loudness_is_normalize_loudness_of_the_plain_run(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import do_say
    a, b, c = (str(tmp_path / f"{k}.wav") for k in "abc")
    do_say(text="Hi there.", output=a, durations_out=str(tmp_path / "a.json"), **_kw(setup, "hifi_gan"))
    plain = list(launches)
    del launches[:]
    do_say(text="Hi there.", output=c, loudness=None, true_peak=None, **_kw(setup, "hifi_gan"))
    assert launches == plain and (tmp_path / "a.wav").read_bytes() == (tmp_path / "c.wav").read_bytes()          # without the option: the plain run
    del launches[:]
    capsys.readouterr()
    do_say(text="Hi there.", output=b, durations_out=str(tmp_path / "b.json"), loudness=-20, **_kw(setup, "hifi_gan"))
    assert launches == plain + ["t2_loudness"]                                                 # the only added library call
    x = written[a]
    want, st = _normalized(x, SR, -20.0)
    assert x.numel() > 0 and not st["flags"] & 2 and torch.equal(written[b], want) and not torch.equal(written[b], x)
    assert _frames(b) == (SR, x.numel())
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text())[0] for k in "ab")
    assert set(rb) - set(ra) == {"loudness_lufs", "gain_db", "true_peak_dbtp"} and all(rb[k] == ra[k] for k in ra)
    assert rb["loudness_lufs"] == st["lufs"] and abs(rb["gain_db"] - 20.0 * math.log10(st["gain"])) <= 1e-9
    assert abs(rb["true_peak_dbtp"] - 20.0 * math.log10(st["gain"] * st["true_peak"])) <= 1e-9 and rb["true_peak_dbtp"] <= -1.0 + 1e-4
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and line[0].startswith(f"say: {b}: {st['lufs']:.2f} LUFS, gain {rb['gain_db']:+.2f} dB, true peak {rb['true_peak_dbtp']:.2f} dBTP")
    again = _normalized(written[b], SR, -20.0)[1]                                               # what was written reads the target, or was bounded
    assert abs(again["lufs"] + 20.0) <= 1e-3 or st["flags"] & 12


def test_a_silent_row_is_written_as_it_is(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import do_say
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    do_say(text="Hi there.", output=a, **_kw(setup, "griffin_lim"))
    capsys.readouterr()
    do_say(text="Hi there.", output=b, loudness=-16, true_peak=-2, durations_out=str(tmp_path / "b.json"), **_kw(setup, "griffin_lim"))
    assert launches == ["t2_loudness"] and written[a].numel() > 0 and not written[a].abs().max() > 0
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
    assert capsys.readouterr().out.strip() == f"say: {b}: no loudness (left as it is)"
    rec = json.loads((tmp_path / "b.json").read_text())[0]
    assert rec["loudness_lufs"] is None and rec["gain_db"] == 0.0 and rec["true_peak_dbtp"] is None


def test_the_normalisation_is_the_last_step_at_the_rate_of_the_header(setup, tmp_path, written):
    from tacotron2_amd import analysis
    from tacotron2_amd.run.say import do_say
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    do_say(text="Hi there.", output=a, **_kw(setup, "hifi_gan"))
    do_say(text="Hi there.", output=b, tempo=1.25, out_sample_rate=16000, loudness=-20, true_peak=-3, **_kw(setup, "hifi_gan"))
    x = written[a]
    s, ns, _ = analysis.time_stretch(x.to(DEV)[None, :], [x.numel()], 1.25)
    z, nz = analysis.resample(s[:, :ns[0]].contiguous(), ns, SR, 16000)
    want, st = _normalized(z[0, :nz[0]].cpu(), 16000, -20.0, -3.0)
    assert torch.equal(written[b], want) and _frames(b) == (16000, nz[0])
    assert not torch.equal(want, _normalized(z[0, :nz[0]].cpu(), SR, -20.0, -3.0)[0])           # (the rate matters: another filter)


def test_several_texts_are_the_rows_of_one_call(setup, tmp_path, written, launches):
    from tacotron2_amd.run.say import do_say
    texts = ["Hi there.", "One came, two stayed."]
    do_say(text=texts, output=str(tmp_path / "a.wav"), **_kw(setup, "hifi_gan"))
    del launches[:]
    do_say(text=texts, output=str(tmp_path / "b.wav"), loudness=-23, durations_out=str(tmp_path / "b.json"), **_kw(setup, "hifi_gan"))
    assert launches == ["t2_loudness"]
    recs = json.loads((tmp_path / "b.json").read_text())
    for i in range(2):
        want, st = _normalized(written[str(tmp_path / f"a_{i}.wav")], SR, -23.0)               # each row what it is alone
        assert torch.equal(written[str(tmp_path / f"b_{i}.wav")], want) and recs[i]["loudness_lufs"] == st["lufs"]
    assert recs[0]["loudness_lufs"] != recs[1]["loudness_lufs"]


def test_a_document_is_one_row_behind_the_join_and_the_level(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import do_say_document
    kw = _kw(setup, "hifi_gan", text_file=str(setup["doc"]), level=True)
    y0, _, base = do_say_document(output=str(tmp_path / "a.wav"), durations_out=str(tmp_path / "a.json"), **kw)
    plain = list(launches)
    del launches[:]
    capsys.readouterr()
    y, _, info = do_say_document(output=str(tmp_path / "b.wav"), durations_out=str(tmp_path / "b.json"), loudness=-18, true_peak=-1.5, **kw)
    assert launches == plain + ["t2_loudness"] and plain.count("t2_join") == 1 and base["loudness"] is None
    want, st = _normalized(written[str(tmp_path / "a.wav")], SR, -18.0, -1.5)                   # the programme's loudness: the joined document
    assert torch.equal(written[str(tmp_path / "b.wav")], want) and torch.equal(y.cpu(), want) and _frames(tmp_path / "b.wav") == (SR, y0.numel())
    assert info["loudness"]["loudness_lufs"] == st["lufs"] and info["join"]["level"] is True
    out = capsys.readouterr().out
    assert f"say: {tmp_path / 'b.wav'}: {st['lufs']:.2f} LUFS, gain " in out
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text()) for k in "ab")
    assert len(rb) == 3 and all(r["loudness_lufs"] == st["lufs"] and r["gain"] == r0["gain"] for r, r0 in zip(rb, ra)) and "gain_db" not in ra[0]
    z, _, _ = do_say_document(output=str(tmp_path / "c.wav"), out_sample_rate=16000, loudness=-18, **kw)       # behind the resampling
    assert _frames(tmp_path / "c.wav") == (16000, z.numel()) and z.numel() == -(-y0.numel() * 16000 // SR)
    bounded = json.loads((tmp_path / "b.json").read_text())[0]["true_peak_dbtp"] > -1.5 - 1e-4        # (a gain lowered to the ceiling)
    assert bounded or abs(_normalized(z.cpu(), 16000, -18.0)[1]["lufs"] + 18.0) <= 1e-3


def test_model_say_document_and_the_command_line_carry_the_options(setup, tmp_path, launches):
    from click.testing import CliRunner
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.run.common import load_decode_model
    from tacotron2_amd.run.say import do_say
    cfg = setup["cfg"]
    pre = cfg["dataset"]["preprocessing"]
    model = load_decode_model(cfg["dataset"], cfg["training"], cfg["model"], cfg["extensions"], str(setup["ck"]), torch.device(DEV), 3, None, None, None)
    enc = TextEncoder(pre["allowed_chars"], pre.get("end_token"), expand_abbrev=False)
    y, plan, info = model.say_document(DOC, enc, pre, max_len=40, loudness=-16, true_peak=-2)
    assert launches == ["t2_join", "t2_loudness"] and info["loudness"]["flags"] & 2 and y.numel() > 0       # (Griffin-Lim: silence, left as it is)
    with pytest.raises(ValueError, match="--true-peak needs --loudness"):
        model.say_document(DOC, enc, pre, max_len=40, true_peak=-2)
    head = ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"]), "--max-len", "40", "--random-seed", "3",
            "--hifi-gan-checkpoint", setup["hifi"]]
    r = CliRunner().invoke(_main(), head + ["--text", "Hi there.", "--out", str(tmp_path / "cli.wav"), "--loudness", "-20", "--true-peak", "-3"])
    assert r.exit_code == 0 and "LUFS, gain" in r.output, (r.output, r.exception)
    do_say(text="Hi there.", output=str(tmp_path / "api.wav"), loudness=-20.0, true_peak=-3.0, **_kw(setup, "hifi_gan"))
    assert (tmp_path / "cli.wav").read_bytes() == (tmp_path / "api.wav").read_bytes()
    r = CliRunner().invoke(_main(), head + ["--text-file", str(setup["doc"]), "--out", str(tmp_path / "doc.wav"), "--loudness", "-16"])
    assert r.exit_code == 0 and "LUFS, gain" in r.output and _frames(tmp_path / "doc.wav")[1] > 0, (r.output, r.exception)
