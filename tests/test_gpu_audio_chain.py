"""The audio chain at both ends of the model, stage by stage against the float64 references of tests/audio_ref.py:
wave -> log-mel through the C ABI (t2_logmel_fwd, t2_logmel_batch_workspace, t2_logmel_batch_fwd via tacotron2_amd._lib.call, with
the caller's own padded / spec / mag / tmp / out buffers) and TacotronMelSpectrogram's tables and workspace reuse; mel -> wave
through vocoder.GriffinLim (stft, istft of inconsistent spectrograms, mel_to_linear, the first iterations of the recursion from
its seeded phases) and hifigan._Conv / _Up called directly on margin buffers, Generator's batch and shape handling, and the
independence of both vocoders from the process-wide matmul precision switch.

Every buffer a C-ABI call or a layer writes is NaN-filled, exactly the documented size, and followed by a 64-word sentinel tail
that must come back untouched; input rows no kernel may read hold NaN.  Geometries, lengths, signals and layer shapes are the
case tables of audio_ref (odd sizes, one sample to either side of a hop multiple, ~141 frames across the GEMM's 128-row tile,
L = 1 and L > 128 rows, the k-GEMM fallback of Ci % 32 != 0).

Metrics.  Pure selections (padded, a batch row against the single path, a second copy) are held bit-equal.  spec, mag, tmp, stft,
istft, mel_to_linear and the layer outputs: max|got - ref| / max|ref| per utterance / call.  The mel in the linear domain:
max_f max_m |exp(out) - max(ref, 1e-5)| / max(max_m ref[f], 1e-5); in the log domain, per element, |out - log ref| over the
elements with ref >= 1e-4 (>= 75 % of the live elements of every case, tests/test_audio_ref_host.py).  Digitally silent frames,
and empty filters in every frame: finite and within 2 float32 ulps (2e-6) of log(1e-5).  Griffin-Lim: relative L2 of the waveform
after 1 and 2 iterations (the recursion amplifies rounding: float32 is at 1e-6 / 3e-6 / 1.4e-5 / 1.5e-2 after 1 / 2 / 4 / 8).

Tolerances: audio_ref.TOL, one constant per output = 16 x the float32 restatement's own error against float64 over the case lists
(anchored by tests/test_audio_ref_host.py).  Every test prints its worst figure per output as
"[audio] <case>: <output> <error> /<constant>" (tabulated in DESIGN.md 5):
    output          float32 restatement   constant (x 16)   MI355X (worst case)
    spec            1.0e-6                1.60e-5           5.52e-7
    mag             9.5e-7                1.52e-5           5.86e-7
    tmp             9.5e-7                1.52e-5           3.00e-7
    mel_lin         9.6e-7                1.54e-5           1.59e-6 (a silent frame: the device's logf(1e-5f), below)
    mel_log         6.5e-5                1.04e-3           2.42e-5
    floor           -                     2e-6              1.59e-6 (logf(1e-5f) = -11.512927, 1.7 float32 ulps off)
    stft            7.2e-7                1.15e-5           4.22e-7
    istft           5.1e-7                8.16e-6           4.19e-7
    mel_to_linear   2.7e-7                4.32e-6           1.57e-7
    gl1             1.4e-6                2.24e-5           4.83e-7
    gl2             1.6e-6                2.56e-5           6.01e-7
    conv            3.1e-7                4.96e-6           3.03e-7
    conv_acc        1.6e-7                2.56e-6           2.38e-7
    up              2.9e-7                4.64e-6           1.56e-7
    fb / basis (absolute, float64 tables)  1e-6             9.19e-10 / 2.98e-8
    generator (absolute, after tanh)       2e-5             4.49e-7
    selections, margins, sentinels, precision independence: bit-equal"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import audio_ref as A  # noqa: E402

TAIL = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


class _Out:
    """A NaN-filled output of exactly n words with a sentinel tail of 64 words behind it."""

    def __init__(self, dev, n, dtype=torch.float32):
        self.n = int(n)
        self.base = torch.empty(self.n + TAIL, dtype=dtype, device=dev)
        self.fill = float("nan") if dtype.is_floating_point else -1
        self.sentinel = A.SENTINEL if dtype.is_floating_point else -7777
        self.base[:self.n] = self.fill
        self.base[self.n:] = self.sentinel
        self.t = self.base[:self.n]

    def intact(self):
        return bool((self.base[self.n:] == self.sentinel).all())

    def untouched(self):
        return bool(torch.isnan(self.t).all()) if self.base.dtype.is_floating_point else bool((self.t == self.fill).all())


def _check(case, figures):
    """figures: [(output, error, bound)]; prints them all, then asserts them all."""
    print(f"[audio] {case}: " + ", ".join(f"{k} {e:.2e} /{b:.1e}" for k, e, b in figures))
    bad = [(k, e, b) for k, e, b in figures if not e <= b]
    assert not bad, f"{case}: over their constant [(output, error, constant)] {bad}"


def _bits(ok):
    """A bit-equality as a figure: 0 when it holds, inf when not."""
    return 0.0 if ok else math.inf


_FE = {}


def _fe(dev, geom):
    from tacotron2_amd.datasets.logmel import TacotronMelSpectrogram
    if geom not in _FE:
        g = A.GEOMETRIES[geom]
        _FE[geom] = TacotronMelSpectrogram(g["n_mels"], g["sr"], g["n_fft"], g["hop"], g["f_min"], g["f_max"], dev)
    return _FE[geom]


def _dims(geom):
    g = A.GEOMETRIES[geom]
    nb = g["n_fft"] // 2 + 1
    return g["n_fft"], g["hop"], g["n_mels"], nb, (nb + 3) // 4 * 4


def _wav(dev, y):
    """The utterance with NaN behind it."""
    w = torch.full((y.numel() + TAIL,), float("nan"), device=dev)
    w[:y.numel()] = y.to(dev)
    return w


def _mel_figs(out, ref):
    f = A.mel_figures(out.cpu(), ref)
    return [("mel_lin", f["mel_lin"], A.TOL["mel_lin"]), ("mel_log", f["mel_log"], A.TOL["mel_log"]), ("floor", f["floor"], A.FLOOR_TOL)]


# -----------------------------------------------------------------------------------------------------------------
# t2_logmel_fwd
# -----------------------------------------------------------------------------------------------------------------
_SINGLE = {}


def _single(dev, geom, n):
    """The four stages of t2_logmel_fwd on the caller's own buffers (run once per case, shared with the batch tests)."""
    from tacotron2_amd._lib import call
    if (geom, n) not in _SINGLE:
        n_fft, hop, n_mels, nb, ldm = _dims(geom)
        fe = _fe(dev, geom)
        frames = 1 + n // hop
        bufs = dict(padded=_Out(dev, n + n_fft), spec=_Out(dev, frames * 2 * nb), mag=_Out(dev, frames * ldm), out=_Out(dev, frames * n_mels))
        call("t2_logmel_fwd", _wav(dev, A.signal(geom, n)), n, fe.basis, fe.fb, bufs["padded"].t, bufs["spec"].t, bufs["mag"].t,
             bufs["out"].t, n_fft, hop, n_mels, _st())
        torch.cuda.synchronize()
        _SINGLE[geom, n] = bufs
    return _SINGLE[geom, n]


@pytest.mark.parametrize("geom,n", [(g, n) for g in A.GEOMETRIES for n in A.lengths(g)])
def test_logmel_fwd_every_stage(dev, geom, n):
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    frames = 1 + n // hop
    ref = A.log_mel_case(geom, n)
    b = _single(dev, geom, n)
    assert all(v.intact() for v in b.values()), "a sentinel tail was written"
    mag = b["mag"].t.view(frames, ldm).cpu()
    out = b["out"].t.view(frames, n_mels)
    figs = [("padded", _bits(torch.equal(b["padded"].t.cpu(), ref["padded"])), 0.0),
            ("spec", A.rel(b["spec"].t.view(frames, 2 * nb).cpu(), ref["spec"]), A.TOL["spec"]),
            ("mag", A.rel(mag[:, :nb], ref["mag"]), A.TOL["mag"]),
            ("mag_pad", _bits(bool((mag[:, nb:] == 0).all())), 0.0)] + _mel_figs(out, ref)
    _check(f"logmel_fwd {geom} n={n}", figs)


@pytest.mark.parametrize("geom", ["default", "oddhop"])
def test_logmel_fwd_rejects_an_utterance_too_short_to_reflect(dev, geom):
    from tacotron2_amd._lib import T2Error, call
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    fe = _fe(dev, geom)
    n = n_fft // 2
    frames = 1 + n // hop
    bufs = [_Out(dev, n + n_fft), _Out(dev, frames * 2 * nb), _Out(dev, frames * ldm), _Out(dev, frames * n_mels)]
    with pytest.raises(T2Error, match="reflect"):
        call("t2_logmel_fwd", _wav(dev, torch.ones(n)), n, fe.basis, fe.fb, *[b.t for b in bufs], n_fft, hop, n_mels, _st())
    torch.cuda.synchronize()
    assert all(b.untouched() and b.intact() for b in bufs)                      # nothing was launched


# -----------------------------------------------------------------------------------------------------------------
# t2_logmel_batch_workspace / t2_logmel_batch_fwd
# -----------------------------------------------------------------------------------------------------------------
def _workspace(geom, B, n_max):
    from tacotron2_amd._lib import call
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    sizes = (ctypes.c_int64 * 5)()
    call("t2_logmel_batch_workspace", B, n_max, n_fft, hop, n_mels, sizes)
    return list(sizes)


def _batch_lengths(geom, B):
    """B = 5: every length of the list but 9 * hop, mixed; B = 1: that one."""
    ns = A.lengths(geom)
    return [ns[5], ns[0], ns[3], ns[1], ns[4]] if B == 5 else [ns[2]]


@pytest.mark.parametrize("T_extra,want_gate", [(0, True), (3, False), (3, True), (0, False)])
@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("geom", A.BATCH_GEOMETRIES)
def test_logmel_batch(dev, geom, B, T_extra, want_gate):
    from tacotron2_amd._lib import call
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    fe = _fe(dev, geom)
    ns = _batch_lengths(geom, B)
    n_max = max(ns)
    sizes = _workspace(geom, B, n_max)
    Tp = 1 + n_max // hop + n_fft // hop
    assert sizes == [B * Tp * hop, B * Tp * 2 * nb, B * Tp * ldm, B * Tp * n_mels, Tp]
    ld = n_max + 29                                                               # ld_wav > n_max, NaN behind every utterance
    wavs = torch.full((B, ld), float("nan"), device=dev)
    for b, n in enumerate(ns):
        wavs[b, :n] = A.signal(geom, n).to(dev)
    n_dev = torch.tensor(ns, dtype=torch.int64, device=dev)
    T_out = 1 + n_max // hop + T_extra
    ws = [_Out(dev, s) for s in sizes[:4]]
    mel, gate, mel_len = _Out(dev, B * T_out * n_mels), _Out(dev, B * T_out), _Out(dev, B, torch.int32)
    call("t2_logmel_batch_fwd", wavs, ld, n_dev, B, n_max, fe.basis, fe.fb, ws[0].t, ws[1].t, ws[2].t, ws[3].t, mel.t, T_out,
         gate.t if want_gate else None, mel_len.t, n_fft, hop, n_mels, _st())
    torch.cuda.synchronize()
    assert all(o.intact() for o in ws + [mel, gate, mel_len]), "a sentinel tail was written"
    assert gate.untouched() or want_gate
    refs = [A.log_mel_case(geom, n) for n in ns]
    exp_mel, exp_gate, exp_len = A.batch_layout([r["out"] for r in refs], T_out)
    got = mel.t.view(B, T_out, n_mels).cpu()
    tmp = ws[3].t.view(B * Tp, n_mels).cpu()
    padded = ws[0].t.view(B, Tp * hop).cpu()
    worst = {}
    for b, (n, ref) in enumerate(zip(ns, refs)):
        f = 1 + n // hop
        one = _single(dev, geom, n)["out"].t.view(f, n_mels).cpu()
        figs = [("row_vs_single", _bits(torch.equal(got[b, :f], one)), 0.0),
                ("behind", _bits(bool((got[b, f:] == 0).all())), 0.0),
                ("padded", _bits(torch.equal(padded[b, :n + n_fft], ref["padded"]) and bool((padded[b, n + n_fft:] == 0).all())), 0.0),
                ("tmp", A.rel(tmp[b * Tp:b * Tp + f], ref["lin"]), A.TOL["tmp"])] + _mel_figs(got[b, :f], ref)
        for k, e, bound in figs:
            if e >= worst.get(k, (-1.0, 0.0))[0]:
                worst[k] = (e, bound)
    figs = [(k, e, bound) for k, (e, bound) in worst.items()]
    figs.append(("mel_len", _bits(torch.equal(mel_len.t.cpu(), exp_len)), 0.0))
    if want_gate:
        figs.append(("gate", _bits(torch.equal(gate.t.view(B, T_out).cpu(), exp_gate)), 0.0))
    assert exp_mel.shape == got.shape
    _check(f"logmel_batch {geom} B={B} T+{T_extra} gate={int(want_gate)}", figs)


def test_logmel_batch_rejections_come_before_any_launch(dev):
    from tacotron2_amd._lib import T2Error, call
    sizes = (ctypes.c_int64 * 5)()
    o = A.GEOMETRIES["oddhop"]
    with pytest.raises(T2Error, match="bad arguments"):
        call("t2_logmel_batch_workspace", 2, 500, o["n_fft"], o["hop"], o["n_mels"], sizes)
    with pytest.raises(T2Error, match="bad arguments"):
        call("t2_logmel_batch_workspace", 2, 32, 64, 16, 12, sizes)             # n_max <= n_fft / 2
    assert list(sizes) == [0] * 5

    def attempt(geom, B, n_max, ld, T_out, match, sizes_from="small"):
        n_fft, hop, n_mels, nb, ldm = _dims(geom)
        fe = _fe(dev, geom)
        need = _workspace(sizes_from, B, max(n_max, 100))
        wavs = torch.ones(B, max(ld, n_max), device=dev)
        n_dev = torch.full((B,), min(n_max, ld), dtype=torch.int64, device=dev)
        outs = [_Out(dev, s) for s in need[:4]] + [_Out(dev, B * max(T_out, 1) * n_mels), _Out(dev, B * max(T_out, 1))]
        mel_len = _Out(dev, B, torch.int32)
        with pytest.raises(T2Error, match=match):
            call("t2_logmel_batch_fwd", wavs, ld, n_dev, B, n_max, fe.basis, fe.fb, outs[0].t, outs[1].t, outs[2].t, outs[3].t, outs[4].t,
                 T_out, outs[5].t, mel_len.t, n_fft, hop, n_mels, _st())
        torch.cuda.synchronize()
        assert all(x.untouched() and x.intact() for x in outs + [mel_len]), (geom, match)

    attempt("oddhop", 2, 500, 512, 1 + 500 // 24, "n_fft % hop == 0")
    attempt("small", 2, 32, 64, 3, "n_fft/2 < n_max")                             # n_max <= n_fft / 2
    attempt("small", 2, 500, 499, 1 + 500 // 16, "n_max <= ld_wav")               # n_max > ld_wav
    attempt("small", 2, 500, 512, 500 // 16, "T_out is shorter")                  # one frame short


# -----------------------------------------------------------------------------------------------------------------
# TacotronMelSpectrogram: tables, reused workspaces
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["sr16k", "narrow"])
def test_front_end_tables_are_the_float64_tables(dev, geom):
    g = A.GEOMETRIES[geom]
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    fe = _fe(dev, geom)
    fb = A.mel_filterbank(g["sr"], n_fft, n_mels, g["f_min"], g["f_max"])
    assert fe.fb.shape == (n_mels, ldm) and fe.basis.shape == (2 * nb, n_fft)
    figs = [("fb", float((fe.fb[:, :nb].double().cpu() - fb).abs().max()), 1e-6),
            ("fb_pad", _bits(bool((fe.fb[:, nb:] == 0).all())), 0.0),
            ("basis", float((fe.basis.double().cpu() - A.dft_basis(n_fft)).abs().max()), 1e-6)]
    _check(f"tables {geom}", figs)


@pytest.mark.parametrize("geom", ["sr16k", "narrow"])
def test_front_end_batch_on_reused_workspaces_equals_a_fresh_instance(dev, geom):
    from tacotron2_amd.datasets.logmel import TacotronMelSpectrogram
    g = A.GEOMETRIES[geom]
    n_fft, hop, n_mels, nb, ldm = _dims(geom)

    def run(fe, ns):
        wavs = torch.zeros(len(ns), max(ns), device=dev)
        for b, n in enumerate(ns):
            wavs[b, :n] = A.signal(geom, n).to(dev)
        return fe.batch(wavs, torch.tensor(ns, dtype=torch.int64, device=dev), max(ns))

    ns = A.lengths(geom)
    big, small = [ns[5], ns[2], ns[0], ns[4]], [ns[3], ns[1]]
    used = TacotronMelSpectrogram(n_mels, g["sr"], n_fft, hop, g["f_min"], g["f_max"], dev)
    run(used, big)
    ws = [w.data_ptr() for w in used._batch_ws]
    got = run(used, small)
    assert [w.data_ptr() for w in used._batch_ws] == ws                          # the large batch's workspaces served the small one
    fresh = run(TacotronMelSpectrogram(n_mels, g["sr"], n_fft, hop, g["f_min"], g["f_max"], dev), small)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, fresh))
    for b, n in enumerate(small):
        f = 1 + n // hop
        assert torch.equal(got[0][b, :f].cpu(), _single(dev, geom, n)["out"].t.view(f, n_mels).cpu())
        assert got[2][b].item() == f


# -----------------------------------------------------------------------------------------------------------------
# vocoder.GriffinLim
# -----------------------------------------------------------------------------------------------------------------
_GL = {}


def _gl(dev, geom, n_iter=2):
    from tacotron2_amd.vocoder import GriffinLim
    if (geom, n_iter) not in _GL:
        g = A.GEOMETRIES[geom]
        _GL[geom, n_iter] = GriffinLim(g["n_mels"], g["sr"], g["n_fft"], g["hop"], g["f_min"], g["f_max"], n_iter, A.MOMENTUM, dev)
    return _GL[geom, n_iter]


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_griffin_lim_stft(dev, geom):
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    gl = _gl(dev, geom)
    figs = []
    for n in A.lengths(geom):
        got = gl.stft(A.signal(geom, n).to(dev))
        assert got.shape == (1 + n // hop, 2, nb)
        figs.append((f"stft n={n}", A.rel(got.cpu(), A.stft3(A.signal(geom, n), n_fft, hop)), A.TOL["stft"]))
    _check(f"griffin_lim {geom}", figs)


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_griffin_lim_istft_of_inconsistent_spectrograms(dev, geom):
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    gl = _gl(dev, geom)
    figs = []
    for frames in A.ISTFT_FRAMES:
        s = A.random_spec(geom, frames)
        got = gl.istft(s.to(dev))
        assert got.shape == (hop * (frames - 1),)
        figs.append((f"istft frames={frames}", A.rel(got.cpu(), A.istft(s, n_fft, hop)), A.TOL["istft"]))
    _check(f"griffin_lim {geom}", figs)


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_griffin_lim_mel_to_linear(dev, geom):
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    gl = _gl(dev, geom)
    fb = gl.front.fb[:, :nb].cpu()                                   # the product's own float32 table (pinned above and in test_gpu_frontend)
    g = A.GEOMETRIES[geom]
    assert float((fb.double() - A.mel_filterbank(g["sr"], n_fft, n_mels, g["f_min"], g["f_max"])).abs().max()) < 1e-6
    m = A.random_mel(geom)
    ref = A.mel_to_linear(m, fb)
    got = gl.mel_to_linear(m.to(dev)).cpu()
    zero = ref == 0
    assert 0.05 < float(zero.double().mean()) < 0.95                 # the clamp has work
    _check(f"griffin_lim {geom}", [("mel_to_linear", A.rel(got, ref), A.TOL["mel_to_linear"]),
                                   ("clamp", max(0.0, -float(got.min())), 0.0)])


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_griffin_lim_recursion_from_its_seeded_phases(dev, geom):
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    S, ph = A.gl_input(geom)
    figs = []
    for it in A.GL_ITERS:
        got = _gl(dev, geom, it).magnitude_to_audio(S.to(dev), seed=A.GL_SEED)
        ref = A.griffin_lim(S, ph, it, A.MOMENTUM, n_fft, hop)
        figs.append((f"gl{it}", A.rel_l2(got.cpu(), ref), A.TOL[f"gl{it}"]))
    _check(f"griffin_lim {geom}", figs)


@pytest.mark.parametrize("geom", A.VOCODER_GEOMETRIES)
def test_griffin_lim_too_short_returns_silence(dev, geom):
    n_fft, hop, n_mels, nb, ldm = _dims(geom)
    gl = _gl(dev, geom)
    for frames in (1, 2, 3):                                          # hop * (frames - 1) <= n_fft / 2
        y = gl.magnitude_to_audio(torch.ones(frames, nb, device=dev))
        assert y.shape == (hop * (frames - 1),) and y.is_cuda and not bool(y.any())
    assert gl.magnitude_to_audio(torch.ones(4, nb, device=dev)).shape == (3 * hop,)     # the first length that is vocoded


# -----------------------------------------------------------------------------------------------------------------
# hifigan._Conv / _Up on margin buffers, Generator
# -----------------------------------------------------------------------------------------------------------------
def _layer_out(dev, L, Co, margin_fill, start=None):
    """The (L + 2 * PAD, Co) output of a layer call inside an _Out: NaN (or the residual) in the data rows, `margin_fill` around."""
    o = _Out(dev, (L + 2 * A.PAD) * Co)
    y = o.t.view(L + 2 * A.PAD, Co)
    y[:A.PAD] = margin_fill
    y[A.PAD + L:] = margin_fill
    if start is not None:
        y[A.PAD:A.PAD + L] = start.to(dev)
    return o, y


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", A.CONV_CASES, ids=str)
def test_hifigan_conv_layer(dev, case, accumulate):
    from tacotron2_amd import hifigan
    assert hifigan.PAD == A.PAD
    Ci, Co, k, d = case
    figs = []
    for L in A.CONV_LENGTHS:
        i = A.conv_inputs(case, L)
        conv = hifigan._Conv(i["w"], i["b"], d, dev)
        assert conv.p == d * (k - 1) // 2
        x = A.margin_input(i["x"], conv.p).to(dev)                    # NaN in the margin rows beyond the layer's reach
        o, y = _layer_out(dev, L, Co, A.SENTINEL, i["res"] if accumulate else None)
        conv(x, y, L, accumulate=accumulate)
        torch.cuda.synchronize()
        assert o.intact(), "the sentinel tail was written"
        got = y.cpu()
        assert bool((got[:A.PAD] == A.SENTINEL).all()) and bool((got[A.PAD + L:] == A.SENTINEL).all()), "a margin row was written"
        ref = A.conv1d(i["x"], i["w"], i["b"], d, i["res"] if accumulate else None)
        key = "conv_acc" if accumulate else "conv"
        figs.append((f"{key} L={L}", A.rel(got[A.PAD:A.PAD + L], ref), A.TOL[key]))
    _check(f"hifigan conv {case} accumulate={int(accumulate)}", figs)


@pytest.mark.parametrize("case", A.UP_CASES, ids=str)
def test_hifigan_upsampling_layer(dev, case):
    from tacotron2_amd import hifigan
    Ci, Co, u = case
    figs = []
    for L in A.UP_LENGTHS:
        i = A.up_inputs(case, L)
        up = hifigan._Up(i["w"], i["b"], u, dev)
        x = A.margin_input(i["x"], 1).to(dev)                         # rows q - 1 = -1 and q = L are read; nothing farther out
        o, y = _layer_out(dev, L * u, Co, float("nan"))
        up(x, y, L)
        torch.cuda.synchronize()
        assert o.intact(), "the sentinel tail was written"
        got = y.cpu()
        ref = A.conv_transpose1d(i["x"], i["w"], i["b"], u)
        figs.append((f"up L={L}", A.rel(got[A.PAD:A.PAD + L * u], ref), A.TOL["up"]))
        figs.append((f"margins L={L}", _bits(torch.equal(got, A.margin_expected(got[A.PAD:A.PAD + L * u], 0.0))), 0.0))
    _check(f"hifigan up {case}", figs)


def _small_generator(dev):
    from tacotron2_amd.hifigan import Generator
    cfg = dict(resblock="1", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
               resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3], [1, 5]])
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g)
    sd = {"conv_pre.weight": rnd(32, 80, 7) * 0.05, "conv_pre.bias": rnd(32) * 0.1}
    ch = 32
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        sd[f"ups.{i}.weight"] = rnd(ch, ch // 2, k) * (0.6 / (ch * 2) ** 0.5); sd[f"ups.{i}.bias"] = rnd(ch // 2) * 0.1
        ch //= 2
        for j, (kk, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            for c in range(len(dil)):
                for part in ("convs1", "convs2"):
                    sd[f"resblocks.{i * 2 + j}.{part}.{c}.weight"] = rnd(ch, ch, kk) * (0.5 / (ch * kk) ** 0.5)
                    sd[f"resblocks.{i * 2 + j}.{part}.{c}.bias"] = rnd(ch) * 0.05
    sd["conv_post.weight"] = rnd(1, ch, 7) * 0.3; sd["conv_post.bias"] = rnd(1) * 0.1
    return cfg, sd, Generator(cfg, dev).load_state_dict(sd), rnd


def test_generator_shapes_batches_and_one_frame(dev):
    from oracle import hifigan_ref as H
    cfg, sd, gen, rnd = _small_generator(dev)
    mel = rnd(2, 80, 9) * 1.5 - 4.0
    both = gen(mel.to(dev))
    assert both.shape == (2, 1, 72)
    assert torch.equal(gen(mel[0].to(dev)), gen(mel[:1].to(dev)))                   # (80, T) is (1, 80, T)
    for b in range(2):
        assert torch.equal(both[b], gen(mel[b].to(dev))[0])                         # a batch is its utterances vocoded alone
    one = gen(mel[:1, :, :1].to(dev))                                               # T = 1: L = 1 rows into every layer
    assert one.shape == (1, 1, 8)
    sd64 = {k: v.double() for k, v in sd.items()}
    figs = [("T=9", float((both[:, 0].double().cpu() - torch.stack([H.generator_fwd(sd64, cfg, m.double()) for m in mel])).abs().max()), 2e-5),
            ("T=1", float((one[0, 0].double().cpu() - H.generator_fwd(sd64, cfg, mel[0, :, :1].double())).abs().max()), 2e-5)]
    _check("hifigan generator (absolute, after tanh: the bound of test_gpu_hifigan)", figs)


def test_vocoders_do_not_depend_on_the_matmul_precision(dev):
    """set_float32_matmul_precision is the reference's torch.set_float32_matmul_precision: it touches the model's matmuls, not
    the vocoders - both run their GEMMs at full float32 accuracy whatever the training configuration asked for."""
    from tacotron2_amd import engine
    cfg, sd, gen, rnd = _small_generator(dev)
    mel = (rnd(1, 80, 6) * 1.5 - 4.0).to(dev)
    gl = _gl(dev, "small")
    y = A.signal("small", A.lengths("small")[4]).to(dev)
    s = A.random_spec("small", 5).to(dev)
    m = A.random_mel("small").to(dev)
    run = lambda: dict(generator=gen(mel), stft=gl.stft(y), istft=gl.istft(s), mel_to_linear=gl.mel_to_linear(m))
    prev = engine.GEMM_PRECISION[0]
    try:
        engine.set_float32_matmul_precision("highest")
        hi = run()
        engine.set_float32_matmul_precision("medium")
        lo = run()
        torch.cuda.synchronize()
    finally:
        engine.GEMM_PRECISION[0] = prev
    _check("precision independence", [(k, _bits(torch.equal(hi[k], lo[k])), 0.0) for k in hi])
