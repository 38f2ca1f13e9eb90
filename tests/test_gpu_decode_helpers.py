"""run/common.py's free_run and emitted_frames on the GPU, on the small model of tests/test_gpu_cli_say_document.py: free_run is
the direct free-running call under the settings that are on the model, bit for bit, and emitted_frames is the host rule `say` had."""
import pytest
import torch

from tacotron2_amd.options import DecodeSettings

pytestmark = pytest.mark.gpu
TEXTS = ["", "hello.", "good morning"]          # 1, 7 and 13 encoded symbols (the end token included)
MAX_LEN = 12


def _seeded(model):
    model.tacotron2._seed, model.tacotron2._calls = 3, 0


@pytest.fixture(scope="module")
def model_and_batch(tmp_path_factory):
    from test_gpu_cli_say_document import ALLOWED, _setup
    from tacotron2_amd.datasets.text import TextEncoder
    from tacotron2_amd.model.tts_model import TTSModel
    from tacotron2_amd.run.common import encode_texts
    dev = torch.device("cuda:0")
    _, _, ck, _ = _setup(tmp_path_factory.mktemp("helpers"))
    model = TTSModel.load_from_checkpoint(str(ck), device=dev)
    model.eval()
    ids, chars, lens = encode_texts(TextEncoder(ALLOWED, "^"), TEXTS, dev)
    assert [len(i) for i in ids] == [1, 7, 13] and chars.shape == (3, 13) and lens.tolist() == [1, 7, 13]
    # At the fixture's stop bias every row stops within 7 frames.  The bias only shifts the stop logits, so one decode under a bias
    # that never stops shows every row's 12 logits, and a shift between the lowest logit of the row that dips lowest and that of the
    # row that dips least gives a batch in which the first stops and the second runs into the cap.
    bias = model.tacotron2.store.P["decoder.gate.bias"]
    _seeded(model)
    with torch.no_grad():
        bias.add_(30.0)
        gates = model(chars_idx=chars, chars_idx_len=lens, teacher_forcing=False, max_len_override=MAX_LEN)[2]
        assert gates.shape == (3, MAX_LEN, 1) and float(gates.min()) > 0
        low = (gates[:, :, 0] - 30.0).min(1).values
        assert float(low.max() - low.min()) > 1e-3, low           # (logits near 30 are known to 2e-6: the midpoint separates the rows)
        bias.sub_(30.0 + 0.5 * float(low.max() + low.min()))
    return model, chars, lens


@pytest.mark.parametrize("settings", [DecodeSettings(), DecodeSettings(attention_window=(1, 3)), DecodeSettings(forward_attention=True),
                                      DecodeSettings(stop_threshold=0.3)], ids=["default", "window", "forward", "threshold"])
def test_free_run_is_the_direct_call_and_emitted_frames_the_host_rule(model_and_batch, settings):
    from test_options_host import parent_frames_host
    from tacotron2_amd.run.common import emitted_frames, free_run
    model, chars, lens = model_and_batch
    model.attention_window, model.forward_attention, model.stop_threshold = settings
    _seeded(model)
    got = free_run(model, chars, lens, MAX_LEN)
    _seeded(model)
    with torch.no_grad():
        want = model(chars_idx=chars, chars_idx_len=lens, teacher_forcing=False, max_len_override=MAX_LEN,
                     attention_window=settings.attention_window, forward_attention=settings.forward_attention,
                     stop_threshold=settings.stop_threshold)[1:]
    assert len(got) == 3 and all(g.is_cuda and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))
    post, gates, align = got
    n = post.shape[1]
    assert 1 <= n <= MAX_LEN and gates.shape == (3, n, 1) and align.shape[:2] == (3, n)
    frames, stopped = emitted_frames(gates, n)
    print(f"{settings}: emitted {n}, frames {frames}, stopped {stopped}")
    assert frames == parent_frames_host(post, gates)
    assert stopped == [int((gates[b, :, 0] != -1000.0).sum()) < n for b in range(3)]
    if settings == DecodeSettings():            # the batch has both kinds of row: one that stopped, one that ran into the cap
        assert n == MAX_LEN and True in stopped and False in stopped, (n, frames, stopped)
