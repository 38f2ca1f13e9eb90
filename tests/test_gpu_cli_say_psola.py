"""`say --preserve-formants / --pitch-range` on the weights of the reference-generated `infer` fixture: the vocoded
waveform goes through analysis.pitch_shift_psola before it is written; in document mode the whole piece buffer does, one launch of each
kernel in front of the join.  Every decode is bounded by --max-len 40; two runs with one seed decode the same frames."""
import json

import pytest
import torch

from test_gpu_cli_say_tempo import DEV, SR, _frames, _kw, _main, _setup  # noqa: F401  (the same checkpoint, config and helpers)

pytestmark = pytest.mark.gpu
DOC = "One came. Two stayed, three left!\n\nIt ends here.\n"


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from helpers import write_hifigan_checkpoint
    root = tmp_path_factory.mktemp("saypsola")
    cfg, cfgp, ck = _setup(root)
    doc = root / "three.txt"
    doc.write_text(DOC, encoding="utf-8")
    return dict(root=root, cfg=cfg, cfgp=cfgp, ck=ck, doc=doc, hifi=write_hifigan_checkpoint(str(root / "hifi"), n_mels=16))


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
    """The library calls made from stretch.py, analysis.py and psola.py, by name and in order."""
    from tacotron2_amd import analysis, psola, stretch
    seen = []
    for mod in (stretch, analysis, psola):
        call = mod.call
        monkeypatch.setattr(mod, "call", lambda name, *a, _call=call: (seen.append(name), _call(name, *a))[1])
    return seen


def _head(setup):
    return ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"]), "--max-len", "40", "--random-seed", "3"]


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifi_gan"])
def test_preserve_formants_is_pitch_shift_psola_of_the_plain_run(setup, tmp_path, written, launches, vocoder):
    from tacotron2_amd import analysis
    from tacotron2_amd.run.say import do_say
    a, b, c, d = (str(tmp_path / f"{k}.wav") for k in "abcd")
    do_say(text="Hi there.", output=a, **_kw(setup, vocoder))
    do_say(text="Hi there.", output=b, pitch_shift=3, **_kw(setup, vocoder))
    assert launches == ["t2_stretch"]
    del launches[:]
    do_say(text="Hi there.", output=c, pitch_shift=3, preserve_formants=True, durations_out=str(tmp_path / "c.json"), **_kw(setup, vocoder))
    assert launches == ["t2_yin", "t2_pitch_viterbi", "t2_psola"]
    x = written[a]
    n = x.numel()
    assert n > 0 and written[c].numel() == n == _frames(c)[1] and _frames(c)[0] == SR         # the plain run's length
    if vocoder == "hifi_gan":                      # (Griffin-Lim of this fixture's few frames is digital silence, and stays it)
        m = min(n, written[b].numel())
        assert not torch.equal(written[c], x) and not torch.equal(written[c][:m], written[b][:m])
    y, n_out, eff = analysis.pitch_shift_psola(x.to(DEV)[None, :], [n], 3.0, SR)
    assert n_out == [n] and eff == 1.0 and torch.equal(written[c], y[0, :n].cpu())
    rec = json.loads((tmp_path / "c.json").read_text())[0]
    assert (rec["tempo"], rec["pitch_shift_semitones"], rec["preserve_formants"], rec["pitch_range"]) == (1.0, 3.0, True, 1.0)
    # with the tempo and the output rate: the stretch first, the pitch tracked on the stretched signal, the resampling last
    do_say(text="Hi there.", output=d, tempo=1.25, pitch_shift=-2, pitch_range=1.5, out_sample_rate=16000, **_kw(setup, vocoder))
    s, ns, _ = analysis.time_stretch(x.to(DEV)[None, :], [n], 1.25)
    z, nz, eff = analysis.pitch_shift_psola(x.to(DEV)[None, :], [n], -2.0, SR, 1.5, 1.25)
    assert nz == ns and eff == 1.25
    want, nw = analysis.resample(z[:, :nz[0]].contiguous(), nz, SR, 16000)
    assert torch.equal(written[d], want[0, :nw[0]].cpu()) and _frames(d) == (16000, nw[0])


def test_pitch_range_alone_runs_from_the_command_line(setup, tmp_path):
    from click.testing import CliRunner
    main = _main()
    for name, more in (("plain", []), ("flat", ["--pitch-range", "0.5"])):
        r = CliRunner().invoke(main, _head(setup) + ["--text", "Hi there.", "--out", str(tmp_path / f"{name}.wav")] + more)
        assert r.exit_code == 0, (r.output, r.exception)
    assert _frames(tmp_path / "flat.wav") == _frames(tmp_path / "plain.wav") and _frames(tmp_path / "flat.wav")[1] > 0


def test_a_document_takes_one_launch_of_each_kernel_for_all_pieces(setup, tmp_path, launches):
    from tacotron2_amd import analysis
    from tacotron2_amd.run.say import do_say_document
    kw = _kw(setup, "hifi_gan", text_file=str(setup["doc"]))
    _, plan0, base = do_say_document(output=str(tmp_path / "a.wav"), durations_out=str(tmp_path / "a.json"), **kw)
    assert launches == []
    y, plan, info = do_say_document(output=str(tmp_path / "b.wav"), durations_out=str(tmp_path / "b.json"), tempo=1.25, pitch_shift=2,
                                    pitch_range=0.5, **kw)
    assert launches == ["t2_stretch", "t2_yin", "t2_pitch_viterbi", "t2_psola"]                # three pieces, ONE launch each
    assert len(info["pieces"]) == 3 and info["chunks"] == 1
    v = info["voice"]
    assert (v.psola, v.tempo, v.ratio, v.semitones, v.pitch_range) == (True, 1.25, (1250, 1000), 2.0, 0.5)
    n0 = base["n"]
    assert info["n"] == [-(-k * 1000 // 1250) for k in n0] and info["frames"] == base["frames"]       # the stretch's counts: no resampling
    buf = torch.zeros(3, max(n0), device=DEV)
    for i, w in enumerate(base["waveforms"]):
        buf[i, :n0[i]] = w
    z, nz, eff = analysis.pitch_shift_psola(buf, n0, 2.0, SR, 0.5, 1.25)
    assert nz == info["n"] and all(torch.equal(info["waveforms"][i], z[i, :nz[i]]) for i in range(3))
    # the pauses: divided by the tempo only
    assert base["pause"] == [round(0.25 * SR), round(0.60 * SR), 0] and info["pause"] == [round(0.25 * SR / 1.25), round(0.60 * SR / 1.25), 0]
    assert _frames(tmp_path / "b.wav") == (SR, y.numel())
    ra, rb = (json.loads((tmp_path / f"{k}.json").read_text()) for k in "ab")
    for i in range(3):
        local, local0 = info["durations"][i], base["durations"][i]
        assert local["end_s"] == [t / 1.25 for t in local0["end_s"]] and local["start_s"] == [t / 1.25 for t in local0["start_s"]]
        r = rb[i]
        assert (r["tempo"], r["pitch_shift_semitones"], r["preserve_formants"], r["pitch_range"]) == (1.25, 2.0, True, 0.5)
        assert "preserve_formants" not in ra[i] and "pitch_range" not in ra[i] and r["frames"] == ra[i]["frames"]


def test_model_say_document_carries_the_two_options(setup, launches):
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.run.common import load_decode_model
    cfg = setup["cfg"]
    pre = cfg["dataset"]["preprocessing"]
    model = load_decode_model(cfg["dataset"], cfg["training"], cfg["model"], cfg["extensions"], str(setup["ck"]), torch.device(DEV), 3, None, None, None)
    enc = TextEncoder(pre["allowed_chars"], pre.get("end_token"), expand_abbrev=False)
    y, plan, info = model.say_document(DOC, enc, pre, max_len=40, preserve_formants=True, pitch_shift=-3, pitch_range=1.2)
    assert launches == ["t2_yin", "t2_pitch_viterbi", "t2_psola"] and info["voice"].psola and y.numel() > 0


def test_the_no_op_combination_launches_nothing_and_writes_the_same_bytes(setup, tmp_path, monkeypatch):
    from click.testing import CliRunner
    from tacotron2_amd import analysis, psola, stretch
    for mod in (stretch, analysis, psola):
        monkeypatch.setattr(mod, "call", lambda *a: pytest.fail("--pitch-shift 0 --pitch-range 1 --preserve-formants must launch nothing"))
    main = _main()
    for name, more in (("plain", []), ("unit", ["--pitch-shift", "0", "--pitch-range", "1", "--preserve-formants"])):
        r = CliRunner().invoke(main, _head(setup) + ["--text", "Hi there.", "--out", str(tmp_path / f"{name}.wav")] + more)
        assert r.exit_code == 0, (r.output, r.exception)
        r = CliRunner().invoke(main, _head(setup) + ["--text-file", str(setup["doc"]), "--out", str(tmp_path / f"{name}_doc.wav")] + more)
        assert r.exit_code == 0, (r.output, r.exception)
    assert (tmp_path / "plain.wav").read_bytes() == (tmp_path / "unit.wav").read_bytes() and _frames(tmp_path / "plain.wav")[1] > 0
    assert (tmp_path / "plain_doc.wav").read_bytes() == (tmp_path / "unit_doc.wav").read_bytes()


def test_usage_errors_name_the_option(setup, tmp_path):
    from click.testing import CliRunner
    head = ["--config", str(setup["cfgp"]), "--device", "0", "say", "--checkpoint", str(setup["ck"])]
    text, doc = ["--text", "Hi."], ["--text-file", str(setup["doc"])]
    npy = str(tmp_path / "o.npy")
    cases = [([*text, "--out", "o.wav", "--pitch-range", "2.5"], "--pitch-range"), ([*text, "--out", "o.wav", "--pitch-range", "-0.1"], "--pitch-range"),
             ([*doc, "--out", "o.wav", "--pitch-range", "nan"], "--pitch-range"), ([*text, "--out", "o.wav", "--pitch-range", "wide"], "--pitch-range"),
             ([*text, "--out", "o.wav", "--preserve-formants"], "--preserve-formants"), ([*doc, "--out", "o.wav", "--preserve-formants", "--tempo", "1.2"], "--preserve-formants"),
             ([*text, "--out", "o.wav", "--preserve-formants", "--pitch-shift", "13"], "--pitch-shift"),
             ([*text, "--out", npy, "--pitch-range", "0.5"], "--pitch-range"), ([*text, "--out", npy, "--pitch-shift", "2", "--preserve-formants"], "--preserve-formants")]
    main = _main()
    for args, name in cases:
        r = CliRunner().invoke(main, head + args)
        assert r.exit_code == 2 and name in r.output and "Usage:" in r.output, (args, r.exit_code, r.output, r.exception)
    assert not (tmp_path / "o.npy").exists()
    from tacotron2_amd.run.say import do_say
    with pytest.raises(ValueError, match="--preserve-formants needs --pitch-shift or --pitch-range"):
        do_say(text="Hi.", output=str(tmp_path / "o.wav"), preserve_formants=True, **_kw(setup, "griffin_lim"))
    with pytest.raises(ValueError, match="--pitch-range must lie in 0 .. 2"):
        do_say(text="Hi.", output=str(tmp_path / "o.wav"), pitch_range=3.0, **_kw(setup, "griffin_lim"))
