"""`say --denoise` on the weights of the reference-generated `infer` fixture, patterned on test_gpu_cli_say_loudness.py: its
checkpoint, its LOUDER HiFi-GAN generator, its recording of write_wav and its recorder of the audio modules' library calls, extended by
the new module.  The denoiser is the FIRST step behind the generator: its bias call (analysis mode) and its own call precede whatever
the plain run launches.  Every decode runs to --max-len 40 (LONG); two runs with one seed decode the same frames."""
import json

import pytest
import torch

from test_gpu_cli_say_loudness import DOC, setup, written  # noqa: F401  (the same fixtures and the LOUDER generator)
from test_gpu_cli_say_tempo import DEV, SR, _frames, _kw as _kw_default, _main

pytestmark = pytest.mark.gpu
FIELDS = {"denoise_strength", "denoise_gated_fraction"}
LONG = 1e-4                                  # stop threshold: these weights stop "Hi there." after 2 frames, 512 samples, a row the denoiser
                                             # copies; with it every decode runs to --max-len 40, 10 240 samples


def _kw(setup, vocoder, **more):
    return _kw_default(setup, vocoder, stop_threshold=LONG, **more)


@pytest.fixture
def launches(monkeypatch):
    """The library calls of the model-free audio modules, the denoiser's among them, by name and in order."""
    from tacotron2_amd import analysis, denoise, join, limiter, loudness, psola, stretch
    from tacotron2_amd.datasets import resample
    seen = []
    for mod in (stretch, analysis, psola, join, loudness, limiter, denoise, resample):
        call = mod.call
        monkeypatch.setattr(mod, "call", lambda name, *a, _call=call: (seen.append(name), _call(name, *a))[1])
    return seen


def _generator(setup):
    from tacotron2_amd.hifigan import Generator
    return Generator.from_checkpoint(setup["hifi"], DEV)


def _denoised(setup, x, strength):
    """analysis.denoise of one host waveform as one row with the generator's bias: (the samples, the gated fraction)."""
    from tacotron2_amd import analysis
    y, stats = analysis.denoise(x.to(DEV)[None, :], [x.numel()], analysis.vocoder_bias(_generator(setup)), strength)
    return y[0].cpu(), stats["gated_fraction"][0].item()


def test_without_the_option_and_with_strength_0_nothing_changes(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import do_say
    a, b, c = (str(tmp_path / f"{k}.wav") for k in "abc")
    do_say(text="Hi there.", output=a, durations_out=str(tmp_path / "a.json"), **_kw(setup, "hifi_gan"))
    plain, line = list(launches), capsys.readouterr().out
    for out, strength in ((b, None), (c, 0)):
        del launches[:]
        do_say(text="Hi there.", output=out, durations_out=str(tmp_path / "x.json"), denoise=strength, **_kw(setup, "hifi_gan"))
        assert launches == plain and capsys.readouterr().out == line
        assert (tmp_path / "a.wav").read_bytes() == open(out, "rb").read()
        assert (tmp_path / "a.json").read_text() == (tmp_path / "x.json").read_text()


def test_denoise_is_analysis_denoise_of_the_plain_run(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import denoise_line, do_say
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    do_say(text="Hi there.", output=a, durations_out=str(tmp_path / "a.json"), **_kw(setup, "hifi_gan"))
    plain = list(launches)
    del launches[:]
    capsys.readouterr()
    do_say(text="Hi there.", output=b, durations_out=str(tmp_path / "b.json"), denoise=0.1, **_kw(setup, "hifi_gan"))
    assert launches == ["t2_denoise", "t2_denoise"] + plain            # the bias (analysis mode), the denoiser, then the plain run's calls
    out = capsys.readouterr().out.strip().splitlines()
    x = written[a]
    want, frac = _denoised(setup, x, 0.1)
    assert x.numel() > 512 and torch.equal(written[b], want) and not torch.equal(want, x) and _frames(b) == (SR, x.numel())
    assert out == [denoise_line(b, 0.1, frac)] and out[0].startswith(f"say: {b}: denoise 0.1, ") and out[0].endswith(" % of bins gated")
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text())[0] for k in "ab")
    assert set(rb) - set(ra) == FIELDS and all(rb[k] == ra[k] for k in ra)
    assert rb["denoise_strength"] == 0.1 and rb["denoise_gated_fraction"] == frac


def test_the_denoiser_runs_in_front_of_the_voice_chain_and_the_loudness_stays_last(setup, tmp_path, written, launches):
    from tacotron2_amd import analysis
    from tacotron2_amd.run.say import do_say
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    do_say(text=["Hi there.", "One came, two stayed."], output=a, **_kw(setup, "hifi_gan"))
    del launches[:]
    do_say(text=["Hi there.", "One came, two stayed."], output=b, denoise=0.5, tempo=0.8, loudness=-16, durations_out=str(tmp_path / "b.json"),
           **_kw(setup, "hifi_gan"))
    assert launches[:2] == ["t2_denoise", "t2_denoise"] and launches.count("t2_denoise") == 2       # both texts are rows of ONE call
    assert launches.index("t2_stretch") == 2 and launches[-1] == "t2_loudness" and launches.count("t2_loudness") == 1
    recs = json.loads((tmp_path / "b.json").read_text())
    for i in range(2):                                                    # each row what it is alone, then the chain of the plain options
        clean, frac = _denoised(setup, written[str(tmp_path / f"a_{i}.wav")], 0.5)
        s, ns, _ = analysis.time_stretch(clean.to(DEV)[None, :], [clean.numel()], 0.8)
        want, _ = analysis.normalize_loudness(s[:, :ns[0]].contiguous(), ns, SR, target=-16.0)
        assert torch.equal(written[str(tmp_path / f"b_{i}.wav")], want[0, :ns[0]].cpu())
        assert recs[i]["denoise_gated_fraction"] == frac and recs[i]["tempo"] == 0.8 and "loudness_lufs" in recs[i]


def test_a_document_is_denoised_chunk_by_chunk_in_front_of_the_join(setup, tmp_path, written, launches, capsys):
    from tacotron2_amd.run.say import denoise_line, do_say_document
    kw = _kw(setup, "hifi_gan", text_file=str(setup["doc"]))
    y0, _, base = do_say_document(output=str(tmp_path / "a.wav"), durations_out=str(tmp_path / "a.json"), **kw)
    plain = list(launches)
    assert plain.count("t2_join") == 1 and base["denoise"] is None
    for batch_size, chunks in ((64, 1), (2, 2)):
        del launches[:]
        capsys.readouterr()
        y, _, info = do_say_document(output=str(tmp_path / "b.wav"), durations_out=str(tmp_path / "b.json"), denoise=0.5, batch_size=batch_size, **kw)
        assert info["chunks"] == chunks and launches == ["t2_denoise"] * (1 + chunks) + plain   # the bias, one call per chunk, then the join
        den = info["denoise"]
        assert den["strength"] == 0.5 and len(den["pieces"]) == 3 and 0.0 <= min(den["pieces"]) <= den["gated_fraction"] <= max(den["pieces"]) <= 1.0
        assert denoise_line(str(tmp_path / "b.wav"), 0.5, den["gated_fraction"]) in capsys.readouterr().out
        ra, rb = (json.loads((tmp_path / f"{k}.json").read_text()) for k in "ab")
        assert len(rb) == 3 and all(set(r) - set(r0) == FIELDS for r, r0 in zip(rb, ra))
        assert [r["denoise_gated_fraction"] for r in rb] == den["pieces"] and all(r["denoise_strength"] == 0.5 for r in rb)
        assert _frames(tmp_path / "b.wav")[0] == SR and y.numel() > 0 and not torch.equal(y.cpu(), y0.cpu())


def test_the_usage_errors_leave_no_file_and_launch_nothing(setup, tmp_path, launches):
    from click.testing import CliRunner
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.run.common import load_decode_model
    from tacotron2_amd.run.say import do_say, do_say_document
    wav, npy = str(tmp_path / "x.wav"), str(tmp_path / "x.npy")
    for fn, kw in ((do_say, dict(text="Hi there.")), (do_say_document, dict(text_file=str(setup["doc"])))):
        with pytest.raises(ValueError, match="--denoise needs --hifi-gan-checkpoint"):
            fn(output=wav, denoise=0.1, **_kw(setup, "griffin_lim", **kw))
        with pytest.raises(ValueError, match="--denoise needs a .wav target"):
            fn(output=npy, denoise=0.1, **_kw(setup, "hifi_gan", **kw))
        with pytest.raises(ValueError, match="--denoise must lie in 0 .. 1"):
            fn(output=wav, denoise=1.5, **_kw(setup, "hifi_gan", **kw))
    cfg = setup["cfg"]
    pre = cfg["dataset"]["preprocessing"]
    model = load_decode_model(cfg["dataset"], cfg["training"], cfg["model"], cfg["extensions"], str(setup["ck"]), torch.device(DEV), 3, None, None, LONG)
    enc = TextEncoder(pre["allowed_chars"], pre.get("end_token"), expand_abbrev=False)
    with pytest.raises(ValueError, match="--denoise needs --hifi-gan-checkpoint"):
        model.say_document(DOC, enc, pre, max_len=40, denoise=0.1)       # (its default vocoder is a Griffin-Lim)
    assert launches == [] and not (tmp_path / "x.wav").exists() and not (tmp_path / "x.npy").exists()
    y, _, info = model.say_document(DOC, enc, pre, vocoder=_generator(setup), max_len=40, denoise=0.1)
    assert launches == ["t2_denoise", "t2_denoise", "t2_join"] and info["denoise"]["strength"] == 0.1 and y.numel() > 0
    head = ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"]), "--max-len", "40", "--random-seed", "3", "--stop-threshold", str(LONG)]
    hifi = ["--hifi-gan-checkpoint", setup["hifi"]]
    for args, msg in ((["--text", "Hi there.", "--out", str(tmp_path / "cli.wav"), "--denoise", "0.1"], "--denoise needs --hifi-gan-checkpoint"),
                      (["--text", "Hi there.", "--out", str(tmp_path / "cli.npy"), "--denoise", "0.1"] + hifi, "--denoise needs a .wav target"),
                      (["--text", "Hi there.", "--out", str(tmp_path / "cli.wav"), "--denoise", "2"] + hifi, "--denoise must lie in 0 .. 1")):
        r = CliRunner().invoke(_main(), head + args)
        assert r.exit_code == 2 and msg in r.output and not (tmp_path / "cli.wav").exists() and not (tmp_path / "cli.npy").exists()
    r = CliRunner().invoke(_main(), head + hifi + ["--text", "Hi there.", "--out", str(tmp_path / "cli.wav"), "--denoise", "0.1"])
    assert r.exit_code == 0 and f"say: {tmp_path / 'cli.wav'}: denoise 0.1, " in r.output, (r.output, r.exception)
    do_say(text="Hi there.", output=str(tmp_path / "api.wav"), denoise=0.1, **_kw(setup, "hifi_gan"))
    assert (tmp_path / "cli.wav").read_bytes() == (tmp_path / "api.wav").read_bytes()
    r = CliRunner().invoke(_main(), head + hifi + ["--text-file", str(setup["doc"]), "--out", str(tmp_path / "doc.wav"), "--denoise", "0.1"])
    assert r.exit_code == 0 and " % of bins gated" in r.output and _frames(tmp_path / "doc.wav")[1] > 0, (r.output, r.exception)
