"""tacotron2_amd/options.py and the drivers' shared pieces of run/common.py on the host (CPU only): the module imports without torch,
a usage error of main.py does not load it, decode_settings is the one table of argument / config / default, every moved name is
the same object where it used to live, and emitted_frames is the rule `say` had twice."""
import os
import subprocess
import sys
import types

import pytest
import torch

from tacotron2_amd import options as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED_FROM_ENGINE = ["check_attention_window", "check_forward_attention", "check_rate", "check_guided_attention", "MEL_LOSSES",
                     "LOSS_DEFAULTS", "check_loss_options", "check_stop_threshold", "stop_logit"]
MOVED_FROM_COMMON = ["train_forward_attention_setting", "loss_options_setting", "stop_threshold_setting", "guided_attention_setting"]


def test_options_and_a_usage_error_do_not_import_torch():
    code = ("import sys\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import tacotron2_amd.options\n"
            "assert 'torch' not in sys.modules, 'options imported torch'\n"
            "assert not any(m.endswith('._lib') for m in sys.modules), 'options imported the library'\n"
            "import main\n"
            "assert 'torch' not in sys.modules, 'main imported torch'\n"
            "from click.testing import CliRunner\n"
            "r = CliRunner().invoke(main.main, ['say', '--checkpoint', 'k.ckpt', '--text', 'hi', '--stop-threshold', '2'], obj={})\n"
            "assert r.exit_code == 2 and 'stop-threshold' in r.output and '0 < P < 1' in r.output, r.output\n"
            "assert 'torch' not in sys.modules, 'the usage error imported torch'\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_moved_names_are_the_same_objects_where_they_lived():
    from tacotron2_amd import engine
    from tacotron2_amd.run import common
    for name in MOVED_FROM_ENGINE:
        assert getattr(engine, name) is getattr(O, name), name
    for name in MOVED_FROM_COMMON:
        assert getattr(common, name) is getattr(O, name), name
    assert common.decode_settings is O.decode_settings and common.decode_settings_of is O.decode_settings_of


# (argument, the config's value or ABSENT, what comes out): the argument wins, else the config, else the default
ABSENT = object()
TABLE = {
    "attention_window": [(None, ABSENT, None), (None, [1, 3], (1, 3)), (None, (0, 0), (0, 0)), ((0, 2), ABSENT, (0, 2)),
                         ((0, 2), [1, 3], (0, 2)), ([2, 5], [1, 3], (2, 5)), (None, None, None)],
    "forward_attention": [(None, ABSENT, False), (None, True, True), (None, False, False), (True, ABSENT, True), (True, False, True),
                          (False, True, False)],
    "stop_threshold": [(None, ABSENT, 0.5), (None, 0.4, 0.4), (0.3, ABSENT, 0.3), (0.3, 0.4, 0.3), (None, 1e-3, 1e-3)],
}


@pytest.mark.parametrize("key", list(TABLE))
def test_decode_settings_argument_wins_then_config_then_default(key):
    for arg, cfg, want in TABLE[key]:
        got = O.decode_settings({} if cfg is ABSENT else {key: cfg}, **{key: arg})
        assert isinstance(got, O.DecodeSettings) and getattr(got, key) == want and type(getattr(got, key)) is type(want), (arg, cfg)
        others = {k: v for k, v in got._asdict().items() if k != key}
        assert others == {k: v for k, v in O.DecodeSettings()._asdict().items() if k != key}


def test_decode_settings_refuses_what_the_loaders_refused():
    """The expectations of test_attention_window_host / test_forward_attention_host on load_test_model, with the text each check
    raises."""
    both = "forward_attention does not compose with attention_window: use one of the two"
    for md, w, f in [({"forward_attention": True, "attention_window": [1, 3]}, None, None), ({"forward_attention": True}, (1, 3), None),
                     ({"attention_window": [1, 3]}, None, True), ({}, (1, 3), True)]:
        with pytest.raises(ValueError) as e:
            O.decode_settings(md, w, f)
        assert str(e.value) == both
    assert O.decode_settings({"attention_window": [1, 3]}).forward_attention is False
    assert O.decode_settings({"forward_attention": True}, None, False) == O.DecodeSettings()       # an explicit False wins too
    for md, text in [({"attention_window": [-1, 3]}, "attention_window must be two integers >= 0, got [-1, 3]"),
                     ({"attention_window": 5}, "attention_window must be (back, fwd), got 5"),
                     ({"forward_attention": "yes"}, "forward_attention must be True or False, got 'yes'"),
                     ({"forward_attention": 1}, "forward_attention must be True or False, got 1"),
                     ({"stop_threshold": 2}, "stop_threshold must be a number with 0 < threshold < 1, got 2"),
                     ({"stop_threshold": True}, "stop_threshold must be a number with 0 < threshold < 1, got True")]:
        with pytest.raises(ValueError) as e:
            O.decode_settings(md)
        assert str(e.value) == text
    # today's order: the window is checked first, then forward attention against it, then the threshold
    with pytest.raises(ValueError, match="attention_window must be two integers"):
        O.decode_settings({"attention_window": [-1, 3], "forward_attention": "yes", "stop_threshold": 2})
    with pytest.raises(ValueError, match="forward_attention must be True or False"):
        O.decode_settings({"forward_attention": "yes", "stop_threshold": 2})
    with pytest.raises(ValueError, match="stop_threshold must be a number"):
        O.decode_settings({}, stop_threshold=0.0)


def test_decode_settings_of_a_model_and_its_kwargs():
    assert tuple(O.decode_settings_of(object())) == (None, False, 0.5)
    m = types.SimpleNamespace(attention_window=(1, 3), stop_threshold=0.3)                      # a stand-in that lacks one attribute
    s = O.decode_settings_of(m)
    assert s == O.DecodeSettings((1, 3), False, 0.3)
    assert s.kwargs() == dict(attention_window=(1, 3), forward_attention=False, stop_threshold=0.3)
    assert list(O.DecodeSettings().kwargs()) == ["attention_window", "forward_attention", "stop_threshold"]


def test_load_decode_model_puts_the_settings_and_the_overrides_on_the_model(monkeypatch):
    from tacotron2_amd.model.tts_model import TTSModel
    from tacotron2_amd.run.common import load_decode_model
    seen = {}

    def mk(checkpoint, device=None, **kw):
        seen.update(kw, checkpoint=checkpoint, device=device)
        return types.SimpleNamespace(eval=lambda: seen.__setitem__("eval", True), tacotron2=types.SimpleNamespace(_seed=0))
    monkeypatch.setattr(TTSModel, "load_from_checkpoint", mk)
    ds, tr = {"preprocessing": {"allowed_chars": "ab"}}, {"lr": 1e-3, "weight_decay": 0.0, "args": {"max_steps": 10}}
    ext = {"speaker_tokens": {"active": False}, "controls": {"active": False}}
    md = {"scheduler_milestones": [0.5], "stop_threshold": 0.4}
    m = load_decode_model(ds, tr, md, ext, "k.ckpt", "cpu", 7, (1, 3))
    assert (m.attention_window, m.forward_attention, m.stop_threshold, m.tacotron2._seed) == ((1, 3), False, 0.4, 7)
    assert seen["eval"] and seen["checkpoint"] == "k.ckpt" and seen["device"] == "cpu" and seen["scheduler_milestones"] == [5]
    m = load_decode_model(ds, tr, md, ext, "k.ckpt", "cpu", scheduler_milestones=[])
    assert seen["scheduler_milestones"] == [] and m.tacotron2._seed == 0 and m.attention_window is None


def parent_frames_host(post, gates):
    """`say`'s rule as do_say wrote it before emitted_frames, on the host in numpy (kept verbatim as the reference)."""
    post = post.cpu().numpy()
    valid = (gates.cpu().numpy()[:, :, 0] != -1000.0).sum(1)
    n_emitted = post.shape[1]
    return [len(post[b, :max(min(int(valid[b]), n_emitted - 1), 1)]) for b in range(post.shape[0])]


def parent_frames_device(post, gates):
    """The same rule as say_document wrote it, on the tensor's device: (frames, stopped)."""
    n_emitted = post.shape[1]
    valid = (gates[:, :, 0] != -1000.0).sum(1).cpu().tolist()             # (do_say's rule: all emitted frames but the last)
    fr = [max(min(int(v), n_emitted - 1), 1) for v in valid]
    return fr, [valid[k] < n_emitted for k in range(len(valid))]


def _gates(n, unmasked):
    g = torch.linspace(-3.0, 3.0, len(unmasked) * n).reshape(len(unmasked), n, 1).clone()
    for b, k in enumerate(unmasked):
        g[b, k:] = -1000.0
    return g


def test_emitted_frames_is_the_rule_say_had_twice():
    from tacotron2_amd.run.common import emitted_frames
    n = 6
    gates = _gates(n, [3, n, 0, 1, n - 1])          # k < n unmasked; never masked; all masked; one frame; stopped at the last frame
    post = torch.zeros(5, n, 4)
    frames, stopped = emitted_frames(gates, n)
    assert frames == [3, n - 1, 1, 1, n - 1] and stopped == [True, False, True, True, True]
    assert all(type(f) is int for f in frames) and all(type(s) is bool for s in stopped)
    assert frames == parent_frames_host(post, gates) and (frames, stopped) == parent_frames_device(post, gates)
    for unmasked in ([1], [0]):                     # n = 1: one frame either way
        g1 = _gates(1, unmasked)
        assert emitted_frames(g1, 1)[0] == [1] == parent_frames_host(torch.zeros(1, 1, 4), g1)
        assert emitted_frames(g1, 1) == parent_frames_device(torch.zeros(1, 1, 4), g1)
    g = torch.Generator().manual_seed(5)
    for n in (2, 7, 12):
        gates = _gates(n, torch.randint(0, n + 1, (9,), generator=g).tolist())
        post = torch.zeros(9, n, 3)
        assert emitted_frames(gates, n) == parent_frames_device(post, gates) and emitted_frames(gates, n)[0] == parent_frames_host(post, gates)


def test_encode_texts_pads_once_and_free_run_passes_the_models_settings():
    from tacotron2_amd.run.common import encode_texts, free_run, pad_ids
    enc = types.SimpleNamespace(encode=lambda t: [ord(c) - 96 for c in t])
    ids, chars, lens = encode_texts(enc, ["abc", "a", "ba"], "cpu")
    assert [i.tolist() for i in ids] == [[1, 2, 3], [1], [2, 1]] and all(i.dtype == torch.int64 for i in ids)
    assert chars.tolist() == [[1, 2, 3], [1, 0, 0], [2, 1, 0]] and lens.tolist() == [3, 1, 2] and lens.dtype == torch.int64
    assert encode_texts(enc, ["ab"])[1:] == (None, None)
    c2, l2 = pad_ids([ids[1], ids[2]], "cpu")
    assert c2.tolist() == [[1, 0], [2, 1]] and l2.tolist() == [1, 2]
    calls = []

    class Model:
        attention_window, stop_threshold = (1, 3), 0.3

        def __call__(self, **kw):
            calls.append((kw, torch.is_grad_enabled()))
            return "loss", "post", "gates", "align"
    assert tuple(free_run(Model(), chars, lens, 12, speaker_id="s")) == ("post", "gates", "align")
    kw, grad = calls[0]
    assert not grad and kw["chars_idx"] is chars and kw["chars_idx_len"] is lens and kw.pop("speaker_id") == "s"
    assert {k: v for k, v in kw.items() if k not in ("chars_idx", "chars_idx_len")} == dict(
        teacher_forcing=False, max_len_override=12, attention_window=(1, 3), forward_attention=False, stop_threshold=0.3)
