"""tacotron2_amd/voice.py on the CPU: `say`'s plan over a grid of rates, tempi, shifts and the three paths against what
run/say.py's voice_settings returned before there was one plan (tests/voice_plan_parent.json: every field, or the refusal's message,
written by that commit's voice_settings; floats by repr), the analysis entry points building the same plan, and the module layout."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "voice_plan_parent.json")) as f:
    ROWS = json.load(f)
MODES = dict(wsola=(None, None), formants=(True, None), range=(True, 0.5))
FIELDS = ("tempo", "requested_tempo", "semitones", "ratio", "sr_mid", "frame", "tolerance", "psola", "pitch_range", "active")


def test_the_grid_is_the_one_the_fixture_was_written_for():
    rates, tempi, shifts = (22050, 16000, 24000, 44100, 48000), (None, 0.5, 0.501, 1.0, 1.999, 2.0), (None, -12, -11.9, -1, 0, 0.01, 5, 12)
    assert [r[:4] for r in ROWS] == [[rate, t, st, m] for rate in rates for t in tempi for st in shifts for m in MODES]
    assert sum(1 for r in ROWS if r[4] is None) == 5 and sum(1 for r in ROWS if r[4] and "refused" in r[4]) == 30


@pytest.mark.parametrize("rate", [22050, 16000, 24000, 44100, 48000])
def test_say_s_plan_is_the_parent_s_and_the_analysis_functions_build_the_same(rate, monkeypatch):
    from tacotron2_amd import psola, stretch, voice
    from tacotron2_amd.run.say import voice_settings
    spied = []
    monkeypatch.setattr(voice, "run_voice", lambda plan, wav, n, *a, **kw: (spied.append(plan), (wav, n))[1])
    x = torch.zeros(2, 3000)
    checked = 0
    for _, tempo, semitones, mode, want in (r for r in ROWS if r[0] == rate):
        formants, rng = MODES[mode]
        if want is not None and "refused" in want:
            with pytest.raises(ValueError) as e:
                voice_settings(tempo, semitones, rate, True, formants, rng)
            assert str(e.value) == want["refused"]
            continue
        plan = voice_settings(tempo, semitones, rate, True, formants, rng)
        if want is None:
            assert plan is None
            continue
        assert isinstance(plan, voice.VoicePlan) and plan.sample_rate == rate
        for k in FIELDS:
            got = getattr(plan, k)
            assert (list(got) if k == "ratio" else got) == want[k] and type(got) is (tuple if k == "ratio" else type(want[k])), \
                (tempo, semitones, mode, k, got, want[k])
        # the entry point of the path this point takes plans the same stretch (a plain tempo has none: pitch_shift always resamples)
        if plan.psola:
            psola.pitch_shift_psola(x, [3000, 2], plan.semitones, rate, plan.pitch_range, plan.requested_tempo, frame=plan.frame,
                                    tolerance=plan.tolerance)
        elif plan.semitones != 0.0:
            stretch.pitch_shift(x, [3000, 2], plan.semitones, rate, plan.requested_tempo, plan.frame, plan.tolerance)
        else:
            continue
        theirs = spied.pop()
        assert not spied and theirs.psola == plan.psola
        assert (theirs.ratio, theirs.sr_mid, theirs.tempo, theirs.frame, theirs.tolerance) == (plan.ratio, plan.sr_mid, plan.tempo, plan.frame,
                                                                                                 plan.tolerance)
        checked += 1
    assert checked == 6 * (6 + 7 + 8)          # six tempi; wsola: the 6 shifts other than 0, formants: those and 0, range: None as well


def test_an_inactive_plan_and_no_plan_launch_nothing():
    from tacotron2_amd.run.say import apply_voice, voice_settings
    x, n = torch.zeros(2, 100), [100, 2]
    for voice in (None, voice_settings(1.0, 0, 22050), voice_settings(None, 0, 22050, True, True, 1.0)):
        assert voice is None or voice.active is False
        got = apply_voice(x, n, voice)
        assert got[0] is x and got[1] is n


def test_layout():
    code = ("import sys, tacotron2_amd.voice as v\n"
            "assert 'tacotron2_amd.engine' not in sys.modules and 'torch' not in sys.modules, sorted(m for m in sys.modules if 'torch' in m)[:3]\n"
            "assert v.wav_target('a.wav', None) and v.wav_target('a.npy', 'g') and not v.wav_target('a.npy', None)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    from tacotron2_amd import analysis, engine
    assert analysis._RESAMPLERS is engine._RESAMPLERS
    pkg = os.path.join(ROOT, "tacotron2_amd")
    defining = [os.path.relpath(os.path.join(d, f), pkg) for d, _, files in os.walk(pkg) for f in files if f.endswith(".py")
                and "def _stream(" in open(os.path.join(d, f)).read()]
    assert defining == [] and engine._stream is __import__("tacotron2_amd._lib", fromlist=["stream"]).stream
