"""`say --limiter` on the weights of the reference-generated `infer` fixture, patterned on test_gpu_cli_say_loudness.py: its
checkpoint, its LOUDER HiFi-GAN generator and its recording of write_wav.  The random generator's output is noise-like, with a crest
factor above 12 dB, so a target of -8 LUFS under a ceiling of -6 dBTP is out of reach of a plain gain: the run without the flag
reports `peak-limited`, and with it the last step's library calls are t2_loudness, t2_limit, t2_loudness and nothing else is added.
Every decode is bounded by --max-len 40; two runs with one seed decode the same frames."""
import json
import math

import pytest
import torch

from test_gpu_cli_say_loudness import DOC, setup, written  # noqa: F401  (the same fixtures and the LOUDER generator)
from test_gpu_cli_say_tempo import DEV, SR, _frames, _kw, _main

pytestmark = pytest.mark.gpu
TARGET, CEILING = -8.0, -6.0
THREE = ["t2_loudness", "t2_limit", "t2_loudness"]
FIELDS = {"loudness_lufs", "gain_db", "true_peak_dbtp", "limited_samples", "limiter_max_reduction_db", "output_lufs"}


@pytest.fixture
def launches(monkeypatch):
    """The library calls of the model-free audio modules, the limiter's among them, by name and in order."""
    from tacotron2_amd import analysis, join, limiter, loudness, psola, stretch
    from tacotron2_amd.datasets import resample
    seen = []
    for mod in (stretch, analysis, psola, join, loudness, limiter, resample):
        call = mod.call
        monkeypatch.setattr(mod, "call", lambda name, *a, _call=call: (seen.append(name), _call(name, *a))[1])
    return seen


def _limited(x, rate=SR):
    """analysis.normalize_loudness(limiter=True) of one host waveform as one row: (the samples, the stats as host numbers)."""
    from tacotron2_amd import analysis
    y, stats = analysis.normalize_loudness(x.to(DEV)[None, :], [x.numel()], rate, target=TARGET, ceiling=CEILING, limiter=True)
    return y[0].cpu(), {k: v[0].item() for k, v in stats.items()}


def _line(name, st):
    return (f"say: {name}: {st['lufs']:.2f} LUFS, gain {20.0 * math.log10(st['gain']):+.2f} dB, limited {st['n_over']} samples by up to "
            f"{-20.0 * math.log10(st['min_gain']):.2f} dB, now {st['output_lufs']:.2f} LUFS, true peak "
            f"{20.0 * math.log10(st['output_true_peak']):.2f} dBTP" + (", boost capped" if st["flags"] & 8 else "") + (", short" if st["flags"] & 1 else ""))


def test_limiter_is_normalize_loudness_limiter_of_the_plain_run(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd import analysis
    from tacotron2_amd.run.say import do_say
    a, p, q, b = (str(tmp_path / f"{k}.wav") for k in "apqb")
    do_say(text="Hi there.", output=a, durations_out=str(tmp_path / "a.json"), **_kw(setup, "hifi_gan"))
    plain = list(launches)
    del launches[:]
    capsys.readouterr()
    do_say(text="Hi there.", output=p, loudness=TARGET, true_peak=CEILING, **_kw(setup, "hifi_gan"))
    assert launches == plain + ["t2_loudness"] and "peak-limited" in capsys.readouterr().out          # the plain gain falls short
    del launches[:]
    do_say(text="Hi there.", output=q, loudness=TARGET, true_peak=CEILING, limiter=None, **_kw(setup, "hifi_gan"))
    assert launches == plain + ["t2_loudness"] and (tmp_path / "p.wav").read_bytes() == (tmp_path / "q.wav").read_bytes()     # without the flag
    del launches[:]
    capsys.readouterr()
    do_say(text="Hi there.", output=b, durations_out=str(tmp_path / "b.json"), loudness=TARGET, true_peak=CEILING, limiter=True, **_kw(setup, "hifi_gan"))
    assert launches == plain + THREE                                                             # nothing else is added
    x = written[a]
    want, st = _limited(x)
    assert x.numel() > 0 and st["n_over"] > 0 and st["limiter_flags"] & 1 and torch.equal(written[b], want) and _frames(b) == (SR, x.numel())
    assert not torch.equal(written[b], written[p])
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text())[0] for k in "ab")
    assert set(rb) - set(ra) == FIELDS and all(rb[k] == ra[k] for k in ra)
    assert rb["loudness_lufs"] == st["lufs"] and abs(rb["gain_db"] - 20.0 * math.log10(st["gain"])) <= 1e-9
    assert rb["limited_samples"] == st["n_over"] and abs(rb["limiter_max_reduction_db"] + 20.0 * math.log10(st["min_gain"])) <= 1e-9
    assert rb["output_lufs"] == st["output_lufs"] and abs(rb["true_peak_dbtp"] - 20.0 * math.log10(st["output_true_peak"])) <= 1e-9
    out = capsys.readouterr().out.strip().splitlines()
    assert out == [_line(b, st)], out
    c = 10.0 ** (CEILING / 20.0)
    again = {k: v[0].item() for k, v in analysis.loudness(written[b].to(DEV)[None, :], [x.numel()], SR).items()}
    assert again["true_peak"] <= c * (1.0 + 1e-5) and again["lufs"] == st["output_lufs"]       # what was written holds the ceiling
    plain_lufs = analysis.loudness(written[p].to(DEV)[None, :], [x.numel()], SR)["lufs"][0].item()
    print(f"plain {plain_lufs:.2f} LUFS, limiter {again['lufs']:.2f} LUFS, target {TARGET}")
    assert abs(again["lufs"] - TARGET) < abs(plain_lufs - TARGET)


def test_a_document_is_limited_as_one_row(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import do_say_document
    kw = _kw(setup, "hifi_gan", text_file=str(setup["doc"]))
    y0, _, base = do_say_document(output=str(tmp_path / "a.wav"), durations_out=str(tmp_path / "a.json"), **kw)
    plain = list(launches)
    del launches[:]
    capsys.readouterr()
    y, _, info = do_say_document(output=str(tmp_path / "b.wav"), durations_out=str(tmp_path / "b.json"), loudness=TARGET, true_peak=CEILING,
                                 limiter=True, **kw)
    assert launches == plain + THREE and plain.count("t2_join") == 1 and base["loudness"] is None
    want, st = _limited(written[str(tmp_path / "a.wav")])                                        # the joined document, one row
    assert torch.equal(written[str(tmp_path / "b.wav")], want) and torch.equal(y.cpu(), want) and _frames(tmp_path / "b.wav") == (SR, y0.numel())
    assert info["loudness"]["limited_samples"] == st["n_over"] > 0 and info["loudness"]["output_lufs"] == st["output_lufs"]
    assert _line(tmp_path / "b.wav", st) in capsys.readouterr().out
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text()) for k in "ab")
    assert len(rb) == 3 and all(set(r) - set(r0) == FIELDS and r["limited_samples"] == st["n_over"] for r, r0 in zip(rb, ra))


def test_a_silent_row_is_written_as_it_is(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import do_say
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    do_say(text="Hi there.", output=a, **_kw(setup, "griffin_lim"))
    capsys.readouterr()
    do_say(text="Hi there.", output=b, loudness=-16, true_peak=-2, limiter=True, durations_out=str(tmp_path / "b.json"), **_kw(setup, "griffin_lim"))
    assert launches == THREE and written[a].numel() > 0 and not written[a].abs().max() > 0
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
    assert capsys.readouterr().out.strip() == f"say: {b}: no loudness (left as it is)"
    rec = json.loads((tmp_path / "b.json").read_text())[0]
    assert rec["loudness_lufs"] is None and rec["gain_db"] == 0.0 and rec["true_peak_dbtp"] is None
    assert rec["limited_samples"] == 0 and rec["limiter_max_reduction_db"] == 0.0 and rec["output_lufs"] is None


def test_limiter_without_loudness_raises_before_any_launch_and_the_command_line_carries_the_flag(setup, tmp_path, launches):
    from click.testing import CliRunner
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.run.common import load_decode_model
    from tacotron2_amd.run.say import do_say, do_say_document
    with pytest.raises(ValueError, match="--limiter needs --loudness"):
        do_say(text="Hi there.", output=str(tmp_path / "x.wav"), limiter=True, **_kw(setup, "hifi_gan"))
    with pytest.raises(ValueError, match="--limiter needs --loudness"):
        do_say_document(output=str(tmp_path / "x.wav"), limiter=True, **_kw(setup, "hifi_gan", text_file=str(setup["doc"])))
    cfg = setup["cfg"]
    pre = cfg["dataset"]["preprocessing"]
    model = load_decode_model(cfg["dataset"], cfg["training"], cfg["model"], cfg["extensions"], str(setup["ck"]), torch.device(DEV), 3, None, None, None)
    enc = TextEncoder(pre["allowed_chars"], pre.get("end_token"), expand_abbrev=False)
    with pytest.raises(ValueError, match="--limiter needs --loudness"):
        model.say_document(DOC, enc, pre, max_len=40, limiter=True)
    assert launches == [] and not (tmp_path / "x.wav").exists()
    y, plan, info = model.say_document(DOC, enc, pre, max_len=40, loudness=-16, true_peak=-2, limiter=True)
    assert launches == ["t2_join"] + THREE and info["loudness"]["flags"] & 2 and info["loudness"]["limited_samples"] == 0    # (Griffin-Lim: silence)
    head = ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"]), "--max-len", "40", "--random-seed", "3",
            "--hifi-gan-checkpoint", setup["hifi"]]
    r = CliRunner().invoke(_main(), head + ["--text", "Hi there.", "--out", str(tmp_path / "cli.wav"), "--limiter"])
    assert r.exit_code == 2 and "--limiter needs --loudness" in r.output and not (tmp_path / "cli.wav").exists()
    r = CliRunner().invoke(_main(), head + ["--text", "Hi there.", "--out", str(tmp_path / "cli.wav"), "--loudness", str(TARGET), "--true-peak",
                                            str(CEILING), "--limiter"])
    assert r.exit_code == 0 and "LUFS, gain" in r.output and " samples by up to " in r.output, (r.output, r.exception)
    do_say(text="Hi there.", output=str(tmp_path / "api.wav"), loudness=TARGET, true_peak=CEILING, limiter=True, **_kw(setup, "hifi_gan"))
    assert (tmp_path / "cli.wav").read_bytes() == (tmp_path / "api.wav").read_bytes()
    r = CliRunner().invoke(_main(), head + ["--text-file", str(setup["doc"]), "--out", str(tmp_path / "doc.wav"), "--loudness", str(TARGET),
                                            "--true-peak", str(CEILING), "--limiter"])
    assert r.exit_code == 0 and " samples by up to " in r.output and _frames(tmp_path / "doc.wav")[1] > 0, (r.output, r.exception)
