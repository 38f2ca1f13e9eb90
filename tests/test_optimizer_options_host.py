"""The optimiser options on the host (no GPU): the tolerances of tests/optimizer_options_ref.py re-measured, its restatement against
torch.optim.AdamW and Tensor.lerp_ in float64, Trainer.lr_at for the three schedules at hand-computed steps, the EMA's num_updates
ramp, every refusal of check_optimizer_options, the usage errors of the new `main.py train` options, and the checkpoint round trips
on CPU stores: the EMA weights, the AdamW flag, the schedule state, the three resume cases and the byte-identical default."""
import copy
import json
import math
import pickle

import numpy as np
import pytest
import torch

from tests import optimizer_options_ref as OR
from tests import optimizer_ref as O
from tests.helpers import SMALL

f32 = O.f32


# ---------------------------------------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    return OR.measure_f32_err()


def test_case_list_covers_what_it_promises():
    cs = list(OR.CASES.values())
    assert {c["decoupled"] for c in cs} == {0, 1}
    assert {c["d"] for c in cs} == {None} | set(OR.DECAYS) and set(OR.DECAYS) == {0.0, 0.5, 0.999, 0.9999, 11.0 / 20.0}
    assert {c["wd"] for c in cs} == {0.0, 1e-6, 0.1} and {c["clip"] for c in cs} == set(O.CLIPS) and len(O.CLIPS) == 4
    assert {c["step"] for c in cs} == {1, 2, 1000} and {c["n"] for c in cs} == {1, 255, 257, 4099, 1048576 + 777}
    for dec in (0, 1):                      # both paths with and without the EMA, at the size above the grid cap too
        assert {c["d"] is None for c in cs if c["decoupled"] == dec} == {True, False}
        assert any(c["n"] > 4096 * 256 for c in cs if c["decoupled"] == dec)


def test_constants_are_16_times_the_float32_restatements_own_error(measured):
    """Each constant lies in [measured, 2 x measured]; the coupled path's are optimizer_ref's, which must hold over this list too."""
    for k in O.OUTPUTS:
        got, name = measured["decoupled"][k]
        print(f"[optimizer-options] float32 restatement, decoupled {k}: {got:.3g} ({name}), constant {OR.F32_ERR_DECOUPLED[k]:.3g}")
        assert got <= OR.F32_ERR_DECOUPLED[k] <= 2.0 * got, (k, got)
        assert OR.TOL_DECOUPLED[k] == 16.0 * OR.F32_ERR_DECOUPLED[k]
        got, name = measured["coupled"][k]
        print(f"[optimizer-options] float32 restatement, coupled {k}: {got:.3g} ({name}), optimizer_ref's constant {O.F32_ERR[k]:.3g}")
        assert 0.0 < got <= O.F32_ERR[k], (k, got)
        assert OR.TOL_COUPLED[k] == O.TOL[k]
    got, name = measured["ema"]
    print(f"[optimizer-options] float32 restatement, ema: {got:.3g} ({name}), constant {OR.F32_ERR_EMA:.3g}")
    assert got <= OR.F32_ERR_EMA <= 2.0 * got and OR.TOL_EMA == 16.0 * OR.F32_ERR_EMA


def test_restatement_identities():
    """Coupled without an EMA is optimizer_ref's restatement; a non-finite norm returns all five inputs; ema == p' is a fixed point
    and the padding stays 0 in float32 too."""
    case = OR.CASES["dec0_dNone"]
    inp = OR.make_inputs(case)
    a, b = OR.reference(case, inp), O.reference(case, inp)
    assert all(np.array_equal(a[k], b[k]) for k in O.OUTPUTS) and "ema" not in a
    case = OR.CASES["dec1_d0.5"]
    inp = OR.make_inputs(case)
    out = OR.adam_opt_step(inp["p"], inp["g"], inp["m"], inp["v"], float("nan"), decoupled=1, ema=inp["ema"], d=0.5, **O.step_kwargs(case))
    assert all(np.array_equal(out[k], inp[k].astype(np.float64)) for k in OR.OUTPUTS)
    ref32 = OR.reference(case, inp, np.float32)
    again = OR.ema_step(ref32["p"], ref32["p"], 0.5, np.float32)
    assert np.array_equal(again, ref32["p"]) and not ref32["ema"][inp["pad"]].any() and not ref32["p"][inp["pad"]].any()


@pytest.mark.parametrize("wd", [0.0, 1e-6, 0.1])
def test_decoupled_restatement_is_torch_adamw(wd):
    """Five steps without a clip against torch.optim.AdamW in float64 under the float32-rounded hyper-parameters the ABI takes.  Each
    step starts from the restatement's previous float32-rounded state (its inputs are float32 arrays) with Adam's step counter set to
    match.  Bound: AdamW orders the same operations differently (lerp, addcdiv, sqrt(v) / sqrt(bc2)); a few dozen float64 roundings
    of 1.1e-16 each, relative to the terms of the sum - 1e-13 of (|p| + lr |ratio|) and of |m|, |v|."""
    n = 4099
    rng = np.random.default_rng(3)
    p, m, v = rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    lr = 1e-3
    for step in range(1, 6):
        g = (rng.standard_normal(n) * 0.01).astype(np.float32)
        ref = OR.adam_opt_step(p, g, m, v, None, 0.0, lr, wd, step, decoupled=1)
        tp = torch.nn.Parameter(torch.from_numpy(p).double())
        opt = torch.optim.AdamW([tp], lr=f32(lr), betas=(f32(O.BETA1), f32(O.BETA2)), eps=f32(O.EPS), weight_decay=f32(wd))
        opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m).double(),
                         "exp_avg_sq": torch.from_numpy(v).double()}
        tp.grad = torch.from_numpy(g).double()
        opt.step()
        st = opt.state[tp]
        assert float(st["step"]) == step
        dp = np.abs(tp.detach().numpy() - ref["p"]) / (np.abs(ref["p"]) + f32(lr) * np.abs(ref["ratio"]))
        dm = np.abs(st["exp_avg"].numpy() - ref["m"]) / (np.abs(ref["m"]) + O.TINY)
        dv = np.abs(st["exp_avg_sq"].numpy() - ref["v"]) / (np.abs(ref["v"]) + O.TINY)
        print(f"[optimizer-options] AdamW wd={wd} step {step}: p {dp.max():.3g} m {dm.max():.3g} v {dv.max():.3g} /1e-13")
        assert dp.max() <= 1e-13 and dm.max() <= 1e-13 and dv.max() <= 1e-13
        if wd == 0.1:                       # decoupled: the decay is NOT in the moments - the coupled restatement's m differs
            assert not np.allclose(O.adam_clip_step(p, g, m, v, None, 0.0, lr, wd, step)["m"], ref["m"], rtol=1e-6, atol=0)
        p, m, v = (ref[k].astype(np.float32) for k in "pmv")


@pytest.mark.parametrize("d", OR.DECAYS)
def test_ema_restatement_is_lerp(d):
    """ema + (1 - d) (p' - ema) against Tensor.lerp_(p', 1 - d) in float64, the update of torch.optim.swa_utils' EMA.  lerp_ switches
    to p' - (p' - ema) d above a weight of 0.5: the same number up to three float64 roundings of the terms - 4e-16 (|ema| + |p'|)."""
    rng = np.random.default_rng(5)
    e = rng.standard_normal(4099).astype(np.float32)
    p = (e.astype(np.float64) * (1 + rng.uniform(-0.125, 0.125, 4099)))
    got = OR.ema_step(e, p, d)
    want = torch.from_numpy(e).double().lerp_(torch.from_numpy(p), 1.0 - f32(d)).numpy()
    assert np.max(np.abs(got - want) / (np.abs(e) + np.abs(p))) <= 4e-16
    if d == 0.0:
        assert np.allclose(got, p, rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------------------
# schedules, the ramp, the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _trainer(lr=1e-3, milestones=(), **opts):
    from tacotron2_amd.model.tts_model import TTSModel
    from tacotron2_amd.trainer import Trainer
    d = dict(SMALL, dropout=0.5)
    model = TTSModel(lr=lr, weight_decay=1e-6, scheduler_milestones=list(milestones), device="cpu", **d)
    tr = Trainer(model.tacotron2.store, lr=lr, weight_decay=1e-6, scheduler_milestones=list(milestones),
                 optimizer_options=opts if opts else None)
    return model, tr


def test_options_module_needs_no_torch():
    import subprocess
    import sys
    code = ("import sys; from tacotron2_amd.options import OptimizerOptions, check_optimizer_options, optimizer_options_setting; "
            "assert 'torch' not in sys.modules; print(OptimizerOptions())")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(__import__("pathlib").Path(__file__).parent.parent))
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ("OptimizerOptions(decoupled_weight_decay=False, ema_decay=0.0, grad_clip=1.0, schedule='multistep', "
                                  "warmup_steps=0, decay_start=0, decay_steps=0, min_lr=0.0)")


def test_lr_at_multistep_and_warmup():
    _, plain = _trainer(milestones=(4, 9))
    _, off = _trainer(milestones=(4, 9), schedule="multistep")
    for t, want in ((0, 1e-3), (3, 1e-3), (4, 1e-3 * 0.1), (8, 1e-3 * 0.1), (9, 1e-3 * (0.1 ** 2)), (50, 1e-3 * (0.1 ** 2))):
        assert plain.lr_at(t) == want == off.lr_at(t)          # today's values, to the bit
    _, warm = _trainer(milestones=(4, 9), warmup_steps=4)
    assert [warm.lr_at(t) for t in range(4)] == [1e-3 * 0.25, 1e-3 * 0.5, 1e-3 * 0.75, 1e-3]      # ends exactly at base
    assert warm.lr_at(4) == 1e-3 * 0.1 and warm.lr_at(9) == 1e-3 * (0.1 ** 2)


def test_lr_at_exponential():
    _, tr = _trainer(schedule="exponential", decay_start=10, decay_steps=4, min_lr=1e-5)
    assert tr.lr_at(0) == 1e-3 and tr.lr_at(9) == 1e-3 and tr.lr_at(10) == 1e-3          # (min_lr / base)^0
    assert tr.lr_at(12) == pytest.approx(1e-4, rel=1e-12)                               # half way: the geometric mean
    assert tr.lr_at(11) == pytest.approx(1e-3 * 10 ** -0.5, rel=1e-12)
    assert tr.lr_at(14) == pytest.approx(1e-5, rel=1e-12) and tr.lr_at(14) == tr.lr_at(15) == tr.lr_at(10 ** 6)     # reaches it, stays
    _, tw = _trainer(schedule="exponential", decay_start=2, decay_steps=2, min_lr=1e-5, warmup_steps=2)
    assert [tw.lr_at(t) for t in range(5)] == pytest.approx([5e-4, 1e-3, 1e-3, 1e-4, 1e-5], rel=1e-12)
    assert tw.lr_at(1) == 1e-3


def test_lr_at_noam():
    _, tr = _trainer(schedule="noam", warmup_steps=100)
    assert tr.lr_at(0) == 1e-3 * 0.01 and tr.lr_at(49) == 1e-3 * 0.5
    assert tr.lr_at(99) == 1e-3                                       # the peak: step W
    assert tr.lr_at(399) == pytest.approx(1e-3 * 0.5, rel=1e-12)      # sqrt(100 / 400)
    assert all(tr.lr_at(t) < 1e-3 for t in (0, 50, 98, 100, 101, 1000))


def test_ema_num_updates_ramp():
    from tacotron2_amd.options import ema_decay_at
    assert ema_decay_at(0.9999, 1) == 2.0 / 11.0 and ema_decay_at(0.9999, 10) == 11.0 / 20.0 and ema_decay_at(0.9999, 90) == 0.91
    assert ema_decay_at(0.5, 7) == 8.0 / 17.0 and ema_decay_at(0.5, 8) == 0.5 and ema_decay_at(0.5, 10 ** 6) == 0.5
    assert ema_decay_at(0.9999, 89990) == 0.9999 and ema_decay_at(0.9999, 89980) < 0.9999      # (1 + k) / (10 + k) crosses D at 89989
    ds = [ema_decay_at(0.999, k) for k in range(1, 20000)]
    assert all(a <= b for a, b in zip(ds, ds[1:])) and ds[-1] == 0.999


@pytest.mark.parametrize("opts,kw,key", [
    (dict(ema_decay=1.0), {}, "ema_decay"), (dict(ema_decay=-0.1), {}, "ema_decay"), (dict(ema_decay=float("nan")), {}, "ema_decay"),
    (dict(ema_decay="0.9"), {}, "ema_decay"), (dict(ema_decay=True), {}, "ema_decay"), (dict(ema_decay=1.0 - 1e-9), {}, "ema_decay"),
    (dict(grad_clip=-1.0), {}, "grad_clip"), (dict(grad_clip=float("inf")), {}, "grad_clip"),
    (dict(schedule="cosine"), {}, "schedule"), (dict(schedule=None), {}, "schedule"),
    (dict(schedule="exponential"), {}, "decay_steps"), (dict(schedule="exponential", decay_steps=0, min_lr=1e-5), {}, "decay_steps"),
    (dict(schedule="exponential", decay_steps=5), {}, "min_lr"), (dict(schedule="exponential", decay_steps=5, min_lr=0.0), {}, "min_lr"),
    (dict(schedule="exponential", decay_steps=5, min_lr=2e-3), dict(lr=1e-3), "min_lr"),
    (dict(schedule="noam"), {}, "warmup_steps"), (dict(schedule="noam", warmup_steps=0), {}, "warmup_steps"),
    (dict(schedule="noam", warmup_steps=10), dict(milestones=[5]), "milestones"),
    (dict(warmup_steps=-1), {}, "warmup_steps"), (dict(warmup_steps=1.5), {}, "warmup_steps"), (dict(decay_start=-2), {}, "decay_start"),
    (dict(decoupled_weight_decay=1), {}, "decoupled_weight_decay"), (dict(momentum=0.9), {}, "momentum"), ([1, 2], {}, "optimizer options"),
])
def test_check_optimizer_options_refuses_and_names_the_key(opts, kw, key):
    from tacotron2_amd.options import check_optimizer_options
    with pytest.raises(ValueError, match=key):
        check_optimizer_options(opts, **kw)


def test_check_optimizer_options_accepts_and_the_setting_lets_the_command_line_win():
    from tacotron2_amd.options import OptimizerOptions, check_optimizer_options, optimizer_options_setting
    assert check_optimizer_options(None) == OptimizerOptions() == check_optimizer_options({}) == check_optimizer_options(OptimizerOptions())
    assert check_optimizer_options(dict(grad_clip=0)).grad_clip == 0.0 and check_optimizer_options(dict(ema_decay=0)).ema_decay == 0.0
    assert check_optimizer_options(dict(schedule="exponential", decay_steps=5, min_lr=1e-3), lr=1e-3).min_lr == 1e-3
    assert check_optimizer_options(dict(schedule="noam", warmup_steps=1)).warmup_steps == 1
    cfg = {"optimizer": {"ema_decay": 0.5, "decoupled_weight_decay": True, "grad_clip": 2.0}}
    o = optimizer_options_setting(cfg, lr=1e-3, ema_decay=0.999, decoupled_weight_decay=None, grad_clip=None, schedule=None)
    assert o == OptimizerOptions(decoupled_weight_decay=True, ema_decay=0.999, grad_clip=2.0)
    assert optimizer_options_setting(cfg, decoupled_weight_decay=False).decoupled_weight_decay is False
    assert optimizer_options_setting({}) == OptimizerOptions()
    with pytest.raises(ValueError, match="training.optimizer"):
        optimizer_options_setting({"optimizer": [0.999]})
    with pytest.raises(ValueError, match="ema_decay"):
        optimizer_options_setting({"optimizer": {"ema_decay": 2}})


def test_trainer_takes_the_options():
    _, tr = _trainer(grad_clip=0.25, ema_decay=0.9, decoupled_weight_decay=True)
    assert tr.max_norm == 0.25 and tr.ema_on and tr.ps.ema is not None and torch.equal(tr.ps.ema, tr.ps.flat) and tr.ema_updates == 0
    _, tr = _trainer()
    assert tr.max_norm == 1.0 and not tr.ema_on and tr.ps.ema is None
    with pytest.raises(ValueError, match="min_lr"):
        _trainer(lr=1e-3, schedule="exponential", decay_steps=3, min_lr=1e-2)
    with pytest.raises(ValueError, match="milestones"):
        _trainer(milestones=(3,), schedule="noam", warmup_steps=5)


def test_store_swap_ema_exchanges_in_place():
    model, tr = _trainer(ema_decay=0.9)
    ps = tr.ps
    ps.ema.mul_(0.5)
    f0, e0, ptr = ps.flat.clone(), ps.ema.clone(), (ps.flat.data_ptr(), ps.ema.data_ptr())
    ps.swap_ema()
    assert torch.equal(ps.flat, e0) and torch.equal(ps.ema, f0) and ptr == (ps.flat.data_ptr(), ps.ema.data_ptr())
    assert torch.equal(model.tacotron2.store.P["prenet.0.weight"], e0[ps.offsets["prenet.0.weight"]:][:ps.P["prenet.0.weight"].numel()].view_as(ps.P["prenet.0.weight"]))
    ps.swap_ema()
    assert torch.equal(ps.flat, f0) and torch.equal(ps.ema, e0)
    _, plain = _trainer()
    with pytest.raises(RuntimeError, match="init_ema"):
        plain.ps.swap_ema()


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
def _config(tmp_path, milestones=(), optimizer=None):
    cfg = {"dataset": {"train": "none.csv", "val": "none.csv", "preprocessing": {"allowed_chars": "abc", "end_token": "^", "num_mels": 80}},
           "training": {"lr": 1e-3, "batch_size": 4, "weight_decay": 1e-6, "name": "tiny", "args": {"max_steps": 6}},
           "model": {"scheduler_milestones": list(milestones), "args": {}},
           "extensions": {"speaker_tokens": {"active": False}, "controls": {"active": False}}}
    if optimizer is not None:
        cfg["training"]["optimizer"] = optimizer
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    return str(p)


@pytest.mark.parametrize("args,word,milestones,optimizer", [
    (["--ema-decay", "1.0"], "0 <= D < 1", (), None), (["--ema-decay", "x"], "0 <= D < 1", (), None),
    (["--ema-decay", "-0.5"], "0 <= D < 1", (), None),
    (["--grad-clip", "-1"], ">= 0", (), None), (["--grad-clip", "nan"], ">= 0", (), None),
    (["--lr-schedule", "cosine"], "cosine", (), None),
    (["--lr-warmup", "-3"], "steps", (), None), (["--lr-warmup", "2.5"], "steps", (), None),
    (["--lr-decay", "2,2"], "START,STEPS,MIN_LR", (), None), (["--lr-decay", "2,0,1e-5"], "START,STEPS,MIN_LR", (), None),
    (["--lr-decay", "a,2,1e-5"], "START,STEPS,MIN_LR", (), None), (["--lr-decay", "2,2,0"], "START,STEPS,MIN_LR", (), None),
    (["--lr-schedule", "exponential"], "decay_steps", (), None),
    (["--lr-schedule", "exponential", "--lr-decay", "2,2,1e-2"], "min_lr", (), None),
    (["--lr-schedule", "noam"], "warmup_steps", (), None),
    (["--lr-schedule", "noam", "--lr-warmup", "10"], "milestones", (0.5,), None),
    ([], "ema_decay", (), {"ema_decay": 1.5}), ([], "unknown key", (), {"beta3": 1}),
])
def test_cli_usage_errors(tmp_path, args, word, milestones, optimizer):
    """Each is a usage error (exit status 2) that names the option or the key, raised before anything is loaded or trained."""
    from click.testing import CliRunner

    import main as cli
    res = CliRunner().invoke(cli.main, ["--config", _config(tmp_path, milestones, optimizer), "train", "--speech-dir", "unused",
                                        "--synthetic"] + args)
    assert res.exit_code == 2, (res.exit_code, res.output, res.exception)
    assert word in res.output, res.output


def test_cli_options_reach_do_train(tmp_path, monkeypatch):
    """The parsed values, and only the options that were given, travel to do_train as its `optimizer` dict; --ema sets model.use_ema."""
    from click.testing import CliRunner

    import main as cli
    import tacotron2_amd.run.train as T
    seen = {}
    monkeypatch.setattr(T, "do_train", lambda **kw: seen.update(kw))
    res = CliRunner().invoke(cli.main, ["--config", _config(tmp_path, optimizer={"ema_decay": 0.5}), "train", "--speech-dir", "unused",
                                        "--ema-decay", "0.999", "--decoupled-weight-decay", "--grad-clip", "0", "--lr-schedule",
                                        "exponential", "--lr-warmup", "2", "--lr-decay", "2,2,1e-5"])
    assert res.exit_code == 0, res.output
    assert seen["optimizer"] == dict(ema_decay=0.999, decoupled_weight_decay=True, grad_clip=0.0, schedule="exponential", warmup_steps=2,
                                     decay_start=2, decay_steps=2, min_lr=1e-5)
    res = CliRunner().invoke(cli.main, ["--config", _config(tmp_path), "train", "--speech-dir", "unused", "--no-decoupled-weight-decay"])
    assert res.exit_code == 0 and seen["optimizer"] == dict(ema_decay=None, decoupled_weight_decay=False, grad_clip=None, schedule=None,
                                                            warmup_steps=None)
    cfg = dict(dataset_config={}, training_config={}, model_config={"a": 1}, extensions_config={}, device=0)
    assert cli.with_ema(cfg, False) is cfg and cli.with_ema(cfg, True)["model_config"] == {"a": 1, "use_ema": True} and "use_ema" not in cfg["model_config"]
    from tacotron2_amd.run.common import use_ema_setting
    assert use_ema_setting({}) is False and use_ema_setting({"use_ema": True}) is True and use_ema_setting({"use_ema": True}, None) is True
    with pytest.raises(ValueError, match="use_ema"):
        use_ema_setting({"use_ema": 1})


# ---------------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------------
def _fill(tr, seed=1, step=6, ema_updates=6):
    ps = tr.ps
    ps.init_adam()
    g = torch.Generator().manual_seed(seed)
    ps.exp_avg.copy_(torch.randn(ps.numel, generator=g) * 0.01); ps.exp_avg_sq.copy_(torch.rand(ps.numel, generator=g) * 1e-4)
    tr.global_step = step
    if ps.ema is not None:
        for name, v in ps.P.items():       # a shadow that differs from the weights in every tensor, padding left equal
            o = ps.offsets[name]
            ps.ema[o:o + v.numel()].copy_((v * 0.75 + 0.01).reshape(-1))
        tr.ema_updates = ema_updates


def _roundtrip(model, tr, tmp_path, name="ck.ckpt"):
    from tacotron2_amd.checkpoint import lightning_checkpoint, save_atomic
    path = str(tmp_path / name)
    save_atomic(lightning_checkpoint(model, tr, epoch=1), path)
    return path, torch.load(path, map_location="cpu", weights_only=True)          # the only loader the product uses


def test_default_checkpoint_is_byte_identical(tmp_path):
    """Plain multistep without a warm-up and no option: the lr_schedulers entry and the param_groups are what they were, byte for
    byte, whether the Trainer is built without the argument or with all options off; no EMA keys."""
    from tacotron2_amd.checkpoint import scheduler_state
    from tacotron2_amd.options import OptimizerOptions
    want = [{"milestones": __import__("collections").Counter([4, 9]), "gamma": 0.1, "base_lrs": [1e-3], "last_epoch": 6, "_step_count": 7,
             "_get_lr_called_within_step": False, "_last_lr": [1e-3 * 0.1]}]
    blobs = []
    for opts in (None, OptimizerOptions()):
        from tacotron2_amd.model.tts_model import TTSModel
        from tacotron2_amd.trainer import Trainer
        model = TTSModel(lr=1e-3, weight_decay=1e-6, scheduler_milestones=[4, 9], device="cpu", **dict(SMALL, dropout=0.5))
        tr = Trainer(model.tacotron2.store, lr=1e-3, weight_decay=1e-6, scheduler_milestones=[4, 9], **({} if opts is None else dict(optimizer_options=opts)))
        _fill(tr)
        _, ck = _roundtrip(model, tr, tmp_path)
        assert "ema_state_dict" not in ck and "ema" not in ck
        assert ck["lr_schedulers"] == want and ck["optimizer_states"][0]["param_groups"][0]["decoupled_weight_decay"] is False
        blobs.append((pickle.dumps(ck["lr_schedulers"]), pickle.dumps(ck["optimizer_states"][0]["param_groups"])))
    assert blobs[0] == blobs[1] and blobs[0][0] == pickle.dumps(want) == pickle.dumps([scheduler_state([4, 9], 1e-3, 1e-3 * 0.1, 6)])


def test_adamw_checkpoint_loads_into_torch_adamw_and_steps_like_the_restatement(tmp_path):
    from tacotron2_amd.checkpoint import reference_param_order
    lr, wd = 2.0 ** -10, 2.0 ** -7            # exact in float32: the checkpoint's python floats are the ABI's floats
    from tacotron2_amd.model.tts_model import TTSModel
    from tacotron2_amd.trainer import Trainer
    d = dict(SMALL, dropout=0.5)
    model = TTSModel(lr=lr, weight_decay=wd, device="cpu", **d)
    tr = Trainer(model.tacotron2.store, lr=lr, weight_decay=wd, optimizer_options=dict(decoupled_weight_decay=True))
    _fill(tr)
    _, ck = _roundtrip(model, tr, tmp_path)
    group = ck["optimizer_states"][0]["param_groups"][0]
    assert group["decoupled_weight_decay"] is True and group["weight_decay"] == wd and group["lr"] == lr
    order = reference_param_order(d)
    sd = {k[len("tacotron2."):]: v for k, v in ck["state_dict"].items()}
    params = [torch.nn.Parameter(sd[n].double().clone()) for n in order]
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd)
    opt.load_state_dict(copy.deepcopy(ck["optimizer_states"][0]))
    assert opt.param_groups[0]["lr"] == lr and float(opt.state[params[0]]["step"]) == 6.0
    opt.param_groups[0]["betas"], opt.param_groups[0]["eps"] = (f32(O.BETA1), f32(O.BETA2)), f32(O.EPS)     # as the ABI takes them
    gen = torch.Generator().manual_seed(2)
    before = [(p.detach().float().numpy().copy(), opt.state[p]["exp_avg"].float().numpy().copy(),
               opt.state[p]["exp_avg_sq"].float().numpy().copy()) for p in params]
    grads = [(torch.randn(p.shape, generator=gen) * 0.01) for p in params]
    for p, g in zip(params, grads):
        p.grad = g.double()
    opt.step()
    worst = 0.0
    for p, g, (p0, m0, v0) in zip(params, grads, before):
        ref = OR.adam_opt_step(p0.ravel(), g.numpy().ravel(), m0.ravel(), v0.ravel(), None, 0.0, lr, wd, 7, decoupled=1)
        dev_ = np.abs(p.detach().numpy().ravel() - ref["p"]) / (np.abs(ref["p"]) + lr * np.abs(ref["ratio"]) + O.TINY)
        worst = max(worst, float(dev_.max()))
    print(f"[optimizer-options] torch.optim.AdamW step on the written state: {worst:.3g} /1e-13")
    assert worst <= 1e-13


def test_ema_and_schedule_round_trip_and_resume(tmp_path, capsys):
    opts = dict(ema_decay=0.999, decoupled_weight_decay=True, schedule="exponential", warmup_steps=2, decay_start=2, decay_steps=8, min_lr=1e-5)
    model, tr = _trainer(**opts)
    _fill(tr, ema_updates=6)
    path, ck = _roundtrip(model, tr, tmp_path)
    # the file: the live weights, the shadow weights under the same keys and shapes, the counter, the schedule
    assert ck["ema"] == {"decay": 0.999, "num_updates": 6}
    assert list(ck["ema_state_dict"]) == list(ck["state_dict"])
    for k, v in ck["state_dict"].items():
        e = ck["ema_state_dict"][k]
        assert e.shape == v.shape and e.dtype == v.dtype, k
        if v.is_floating_point() and "running_" not in k:
            assert torch.equal(e, v * 0.75 + 0.01), k
        else:
            assert torch.equal(e, v), k               # BatchNorm buffers: the live ones
    sch = ck["lr_schedulers"][0]
    assert sch == {"t2_schedule": dict(schedule="exponential", warmup_steps=2, decay_start=2, decay_steps=8, min_lr=1e-5, milestones=[]),
                   "base_lrs": [1e-3], "last_epoch": 6, "_step_count": 7, "_last_lr": [tr.lr_at(6)]}
    assert tr.lr_at(6) == pytest.approx(1e-3 * (1e-2) ** 0.5, rel=1e-12)
    # 1. EMA on, the file has the shadow: restored with the counter; the schedule replaces the configured one, one line says so
    from tacotron2_amd.checkpoint import restore_trainer
    model2, tr2 = _trainer(ema_decay=0.9, schedule="noam", warmup_steps=50)
    model2.load_checkpoint_dict(ck)
    capsys.readouterr()
    assert restore_trainer(ck, tr2)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "schedule" in out and "replaces" in out
    assert tr2.ema_updates == 6 and tr2.global_step == 6 and torch.equal(tr2.ps.flat, tr.ps.flat)
    for n, v in tr.ps.P.items():
        o = tr.ps.offsets[n]
        assert torch.equal(tr2.ps.ema[o:o + v.numel()], tr.ps.ema[o:o + v.numel()]), n
    assert tr2.optimizer_options.schedule == "exponential" and tr2.optimizer_options.ema_decay == 0.9
    assert [tr2.lr_at(t) for t in range(12)] == [tr.lr_at(t) for t in range(12)]
    #    the same schedule configured: nothing is printed
    model3, tr3 = _trainer(**opts)
    model3.load_checkpoint_dict(ck)
    restore_trainer(ck, tr3)
    assert capsys.readouterr().out == "" and tr3.optimizer_options == tr.optimizer_options
    # 2. EMA on, the file has none: initialised from the restored weights, one line
    modelp, trp = _trainer(milestones=(4, 9))
    _fill(trp)
    _, ckp = _roundtrip(modelp, trp, tmp_path, "plain.ckpt")
    model4, tr4 = _trainer(milestones=(4, 9), ema_decay=0.99)
    tr4.ps.ema.fill_(7.0); tr4.ema_updates = 3
    model4.load_checkpoint_dict(ckp)
    restore_trainer(ckp, tr4)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "no EMA weights" in out
    assert torch.equal(tr4.ps.ema, tr4.ps.flat) and torch.equal(tr4.ps.flat, trp.ps.flat) and tr4.ema_updates == 0
    # 3. EMA off, the file has one: dropped, one line (and its schedule still replaces the configured multistep)
    model5, tr5 = _trainer(**{k: v for k, v in opts.items() if k != "ema_decay"})
    model5.load_checkpoint_dict(ck)
    restore_trainer(ck, tr5)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "dropped" in out and tr5.ps.ema is None and not tr5.ema_on
    # a multistep file under a configured exponential schedule: multistep comes back, one line
    model6, tr6 = _trainer(**{k: v for k, v in opts.items() if k != "ema_decay"})
    model6.load_checkpoint_dict(ckp)
    restore_trainer(ckp, tr6)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "multistep" in out and tr6.milestones == [4, 9] and tr6.lr_at(5) == trp.lr_at(5) == 1e-3 * 0.1


def test_loading_the_shadow_weights_for_decoding(tmp_path):
    from tacotron2_amd.model.tts_model import TTSModel
    model, tr = _trainer(ema_decay=0.999)
    _fill(tr)
    path, ck = _roundtrip(model, tr, tmp_path)
    live = TTSModel.load_from_checkpoint(path, device="cpu")
    shadow = TTSModel.load_from_checkpoint(path, device="cpu", use_ema=True)
    assert torch.equal(live.tacotron2.store.flat, tr.ps.flat)
    for n, v in tr.ps.P.items():
        assert torch.equal(shadow.tacotron2.store.P[n], v * 0.75 + 0.01), n
    assert torch.equal(shadow.tacotron2.store.buf_flat, tr.ps.buf_flat)
    model.load_checkpoint_dict(ck, use_ema=True)
    assert torch.equal(model.tacotron2.store.flat, shadow.tacotron2.store.flat)
    # a file without them: an error that names the file
    modelp, trp = _trainer()
    _fill(trp)
    plain, ckp = _roundtrip(modelp, trp, tmp_path, "plain.ckpt")
    with pytest.raises(KeyError, match="plain.ckpt"):
        TTSModel.load_from_checkpoint(plain, device="cpu", use_ema=True)
    with pytest.raises(KeyError, match="EMA"):
        modelp.load_checkpoint_dict(ckp, use_ema=True)
