"""The driver's route through the voice chain and the model-free one are the same bits: run/say.py's
apply_voice(buf, n, voice_settings(...)) against analysis.pitch_shift, pitch_shift_psola and time_stretch called with the plan's window,
on a two-row cut of a wider buffer whose second row is shorter than one frame, and on a batch without a column."""
import numpy as np
import pytest
import torch

import psola_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 22050
CASES = dict(wsola=(1.25, 3, None), psola=(1.25, 3, True), tempo=(0.8, None, None))


@pytest.fixture(scope="module")
def batch():
    """(2, 3000) as big[:, :3000] of a (2, 4096) buffer that is NaN wherever no sample is: a synthetic vowel of 3000 samples with a
    little noise on it, and 2 samples."""
    x = R.vowel(100, 1000.0, 200.0, n=3000) + 1e-4 * np.random.default_rng(0).standard_normal(3000)
    big = torch.full((2, 4096), float("nan"))
    big[0, :3000] = torch.from_numpy(x.astype(np.float32))
    big[1, :2] = big[0, 500:502]
    return big.to(DEV)[:, :3000], [3000, 2]


def _model_free(plan, buf, n):
    from tacotron2_amd import analysis
    if plan.psola:
        return analysis.pitch_shift_psola(buf, n, plan.semitones, SR, plan.pitch_range, plan.requested_tempo, frame=plan.frame,
                                          tolerance=plan.tolerance)[:2]
    if plan.semitones != 0.0:
        return analysis.pitch_shift(buf, n, plan.semitones, SR, plan.requested_tempo, plan.frame, plan.tolerance)[:2]
    return analysis.time_stretch(buf, n, plan.requested_tempo, plan.frame, plan.tolerance)[:2]


@pytest.mark.parametrize("case", list(CASES))
def test_apply_voice_is_the_analysis_function_of_its_path(batch, case):
    from tacotron2_amd.run.say import apply_voice, voice_settings
    buf, n = batch
    tempo, semitones, formants = CASES[case]
    plan = voice_settings(tempo, semitones, SR, True, formants, None)
    assert plan.active and plan.psola == bool(formants) and (plan.frame, plan.tolerance) == (1024, 256)
    y, n_out = apply_voice(buf, n, plan)
    want, n_want = _model_free(plan, buf, n)
    assert n_out == list(n_want) and all(type(v) is int for v in n_out)
    assert n_out == ([-(-3000 * 1000 // 1250), 2] if formants else n_out) and 0 < n_out[1] <= 4 and abs(n_out[0] - 3000 / plan.tempo) <= 8
    assert y.shape == want.shape and torch.equal(y, want)
    assert bool(torch.isfinite(y[0, :n_out[0]]).all()) and bool(torch.isfinite(y[1, :n_out[1]]).all()) and float(y[0, :n_out[0]].abs().max()) > 0


@pytest.mark.parametrize("case", list(CASES))
def test_a_batch_without_a_column_passes(case):
    """B = 1, ld = 0: no launch error on any path.  (Before there was one plan, the PSOLA path handed the stretch's empty output to yin
    and t2_yin refused its null pointer on the host - seen on an MI355X; run_voice now returns behind the stretch.)"""
    from tacotron2_amd.run.say import apply_voice, voice_settings
    tempo, semitones, formants = CASES[case]
    plan = voice_settings(tempo, semitones, SR, True, formants, None)
    y, n_out = apply_voice(torch.zeros(1, 0, device=DEV), [0], plan)
    want, n_want = _model_free(plan, torch.zeros(1, 0, device=DEV), [0])
    torch.cuda.synchronize()
    assert n_out == [0] == list(n_want) and y.shape[0] == 1 and y.shape == want.shape
