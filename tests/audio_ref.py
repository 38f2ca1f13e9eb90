"""float64 references, case tables and tolerance constants of the audio chain at both ends of the model (TEST INFRASTRUCTURE):
wave -> log-mel (t2_logmel_fwd, t2_logmel_batch_fwd: csrc/t2_logmel.hip, datasets/logmel.py) and mel -> wave (vocoder.GriffinLim:
STFT, inverse STFT, mel inversion, the Griffin-Lim recursion; hifigan._Conv / _Up on their margin buffers).

Plain torch on the CPU; nothing of tacotron2_amd is imported.  Every function takes a `dtype`: float64 is the reference, float32
is the restatement of the same arithmetic that anchors TOL.  The tables (window-folded DFT bases, the slaney filterbank, its
pseudo-inverse) are built in float64 and then cast to `dtype`, as the product builds them in float64 and stores float32.  `fault`
keywords apply the mutations of tests/test_audio_ref_host.py to the restatement (never to product code).

tests/test_audio_ref_host.py checks the references against independent routes (torch.stft, a direct DFT, oracle/logmel_ref.py,
torch.nn.functional convolutions) and anchors the constants; tests/test_gpu_audio_chain.py compares the kernels with them."""
import functools
import math
from collections import OrderedDict

import numpy as np
import torch

from oracle import hifigan_ref as H

F64 = torch.float64
FLOOR = 1e-5                 # the clamp in front of the logarithm
COVER = 1e-4                 # the per-element log comparison covers ref >= 10 x the floor
FLOOR_TOL = 2e-6             # silent frames and empty filters: 2 float32 ulps of log(1e-5) = -11.5129 (ulp 9.5e-7)

GEOMETRIES = OrderedDict(
    default=dict(n_fft=1024, hop=256, n_mels=80, sr=22050, f_min=0.0, f_max=8000.0),     # nb = 513 -> ldm = 516
    small=dict(n_fft=64, hop=16, n_mels=12, sr=16000, f_min=0.0, f_max=8000.0),          # f_max = Nyquist, nb = 33 -> ldm = 36
    narrow=dict(n_fft=256, hop=64, n_mels=80, sr=22050, f_min=0.0, f_max=8000.0),        # four filters hold no DFT bin at all
    sr16k=dict(n_fft=1024, hop=256, n_mels=40, sr=16000, f_min=0.0, f_max=8000.0),
    oddhop=dict(n_fft=64, hop=24, n_mels=12, sr=16000, f_min=0.0, f_max=8000.0),         # n_fft % hop != 0: single-utterance entry only
)
BATCH_GEOMETRIES = [g for g in GEOMETRIES if g != "oddhop"]


def lengths(geom):
    """Shortest legal, one window, 9 hops and one sample to either side, ~141 frames (crosses the GEMM's 128-row tile)."""
    g = GEOMETRIES[geom]
    n_fft, hop = g["n_fft"], g["hop"]
    return [n_fft // 2 + 1, n_fft, 9 * hop, 9 * hop - 1, 9 * hop + 1, 140 * hop + hop // 2 + 5]


def amplitude(geom):
    """The signal's scale: mel energies grow with the window length, so short windows get louder signals (coverage condition)."""
    return 1024.0 / GEOMETRIES[geom]["n_fft"]


@functools.lru_cache(maxsize=None)
def signal(geom, n, silence=True):
    """(n,) float32: two sinusoids (one decaying) over a white floor of sigma = 0.01, times amplitude(geom); with `silence` a block
    of 2 * n_fft exact zeros where it fits (n >= 2 * n_fft + hop / 2), at an offset that is no multiple of the hop."""
    g = GEOMETRIES[geom]
    n_fft, hop, sr = g["n_fft"], g["hop"], g["sr"]
    rng = np.random.default_rng(1000 * list(GEOMETRIES).index(geom) + n % 997)
    t = np.arange(n) / sr
    x = 0.3 * np.sin(2 * np.pi * 0.017 * sr * t) + 0.15 * np.sin(2 * np.pi * 0.11 * sr * t) * np.exp(-2.0 * t * sr / n)
    x = amplitude(geom) * (x + 0.01 * rng.normal(size=n))
    if silence and n >= 2 * n_fft + hop // 2:
        z0 = hop // 4 + 3 if n < 6 * n_fft else 5 * hop + 3
        x[z0:z0 + 2 * n_fft] = 0.0
    return torch.from_numpy(x.astype(np.float32))


# -----------------------------------------------------------------------------------------------------------------
# wave -> log-mel
# -----------------------------------------------------------------------------------------------------------------
def hann(n_fft, fault=None):
    n = torch.arange(n_fft, dtype=F64)
    return 0.5 - 0.5 * torch.cos(2 * math.pi * n / (n_fft - 1 if fault == "symmetric_hann" else n_fft))      # periodic


def dft_basis(n_fft, fault=None):
    """(2 * nb, n_fft) float64: the window-folded [cos ; -sin] rows, bin k = row k (Re) and row nb + k (Im)."""
    nb = n_fft // 2 + 1
    ang = 2 * math.pi * torch.outer(torch.arange(nb, dtype=F64), torch.arange(n_fft, dtype=F64)) / n_fft
    win = hann(n_fft, fault)
    return torch.cat([torch.cos(ang) * win, -torch.sin(ang) * win], 0)


def reflect_pad(y, pad, fault=None):
    """(n,) -> (n + 2 * pad,): out[i] = y[reflect(i - pad)], the edge samples not repeated.  A pure selection (dtype of y)."""
    n = y.numel()
    assert n > pad
    j = torch.arange(n + 2 * pad) - pad - (1 if fault == "pad_off_by_one" else 0)
    j = j.abs()
    j = torch.where(j >= n, 2 * (n - 1) - j, j).clamp_(min=0)
    return y[j]


def frame_rows(padded, n, n_fft, hop):
    """The overlapping analysis windows (frames, n_fft), frames = 1 + n // hop."""
    frames = 1 + n // hop
    idx = torch.arange(frames)[:, None] * hop + torch.arange(n_fft)[None, :]
    return padded[idx]


def stft_ri(y, n_fft, hop, dtype=F64, fault=None):
    """(n,) -> (frames, 2 * nb) = [Re | Im] of the centred, reflect-padded, periodic-Hann STFT."""
    rows = frame_rows(reflect_pad(y, n_fft // 2, fault), y.numel(), n_fft, hop).to(dtype)
    return rows @ dft_basis(n_fft, fault).to(dtype).t()


def magnitude(spec, dtype=F64, fault=None):
    nb = spec.shape[1] // 2
    re, im = spec[:, :nb].to(dtype), spec[:, nb:].to(dtype)
    mag = torch.sqrt(re * re + im * im)
    if fault == "nyquist_dropped":
        mag[:, nb - 1] = 0
    return mag


def _hz_to_mel(f):
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    return torch.where(f >= min_log_hz, min_log_hz / f_sp + torch.log(f.clamp(min=1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, f_min, f_max, fault=None):
    """(n_mels, nb) float64 triangular filters on the slaney mel scale with slaney (area) normalisation."""
    nb = n_fft // 2 + 1
    freqs = torch.linspace(0, sr // 2, nb, dtype=F64)
    lo, hi = _hz_to_mel(torch.tensor([f_min, f_max], dtype=F64))
    pts = _mel_to_hz(torch.linspace(float(lo), float(hi), n_mels + 2, dtype=F64))
    fb = torch.zeros(n_mels, nb, dtype=F64)
    for m in range(n_mels):
        left, centre, right = pts[m], pts[m + 1], pts[m + 2]
        tri = torch.minimum((freqs - left) / (centre - left), (right - freqs) / (right - centre)).clamp(min=0.0)
        fb[m] = tri * (2.0 / (right - left))
    if fault == "filter_norm":
        fb[(4 * n_mels) // 5] *= 1.05
    return fb


def linear_mel(mag, fb, dtype=F64):
    return mag.to(dtype) @ fb.to(dtype).t()


def log_mel(y, geom, dtype=F64, fault=None):
    """Every stage of the single-utterance path: padded (n + n_fft,), spec (frames, 2 * nb), mag (frames, nb), lin and out
    (frames, n_mels), and the two masks the comparisons need - silent (frames,): every sample of the window is exactly zero;
    empty (n_mels,): the filter holds no DFT bin."""
    g = GEOMETRIES[geom]
    n_fft, hop = g["n_fft"], g["hop"]
    padded = reflect_pad(y, n_fft // 2, fault)
    spec = stft_ri(y, n_fft, hop, dtype, fault)
    mag = magnitude(spec, dtype, fault)
    fb = mel_filterbank(g["sr"], n_fft, g["n_mels"], g["f_min"], g["f_max"], fault)
    lin = linear_mel(mag, fb, dtype)
    out = torch.log(lin.clamp(min=1e-6 if fault == "floor" else FLOOR))
    silent = (frame_rows(padded, y.numel(), n_fft, hop) == 0).all(1)
    return dict(padded=padded, spec=spec, mag=mag, lin=lin, out=out, silent=silent, empty=(fb == 0).all(1))


@functools.lru_cache(maxsize=None)
def log_mel_case(geom, n, dtype=F64):
    return log_mel(signal(geom, n), geom, dtype)


def batch_layout(outs, T_out):
    """[(frames_b, n_mels) log-mel] -> mel (B, T_out, n_mels) zero-padded, gate (B, T_out): ones, the last valid frame 0, zeros
    behind it, and mel_len (B,)."""
    B, n_mels = len(outs), outs[0].shape[1]
    mel = torch.zeros(B, T_out, n_mels, dtype=outs[0].dtype)
    gate = torch.zeros(B, T_out, dtype=outs[0].dtype)
    for b, o in enumerate(outs):
        mel[b, :o.shape[0]] = o
        gate[b, :o.shape[0] - 1] = 1
    return mel, gate, torch.tensor([o.shape[0] for o in outs], dtype=torch.int32)


# -----------------------------------------------------------------------------------------------------------------
# mel -> wave: the Griffin-Lim vocoder
# -----------------------------------------------------------------------------------------------------------------
def idft_basis(n_fft, fault=None):
    """(2 * nb, n_fft) float64: x[n] = (1 / N) sum_k h_k (Re_k cos - Im_k sin), h = 1 at DC and Nyquist and 2 between, times the
    synthesis window."""
    nb = n_fft // 2 + 1
    ang = 2 * math.pi * torch.outer(torch.arange(nb, dtype=F64), torch.arange(n_fft, dtype=F64)) / n_fft
    herm = torch.full((nb, 1), 2.0, dtype=F64)
    herm[0] = herm[-1] = 1.0
    if fault == "herm_dc":
        herm[0] = 2.0
    return torch.cat([torch.cos(ang) * herm, -torch.sin(ang) * herm], 0) * (hann(n_fft)[None, :] / n_fft)


def istft(spec, n_fft, hop, dtype=F64, fault=None):
    """(frames, 2, nb) -> (hop * (frames - 1),): windowed inverse DFT of every frame, overlap-add, division by
    clamp(sum win^2, 1e-8), the centre cut.  Defined for inconsistent spectrograms too (no frame needs to be anyone's STFT)."""
    frames = spec.shape[0]
    yf = spec.reshape(frames, -1).to(dtype) @ idft_basis(n_fft, fault).to(dtype)              # (frames, n_fft)
    total = n_fft + hop * (frames - 1)
    idx = (torch.arange(frames)[:, None] * hop + torch.arange(n_fft)[None, :]).reshape(-1)
    win = hann(n_fft)
    w = (win if fault == "env_sum_win" else win * win).to(dtype)
    y = torch.zeros(total, dtype=dtype).index_add_(0, idx, yf.reshape(-1))
    env = torch.zeros(total, dtype=dtype).index_add_(0, idx, w.repeat(frames))
    return (y / env.clamp(min=1e-8))[n_fft // 2: total - n_fft // 2]


def stft3(y, n_fft, hop, dtype=F64):
    """stft_ri in the vocoder's shape (frames, 2, nb)."""
    return stft_ri(y, n_fft, hop, dtype).reshape(-1, 2, n_fft // 2 + 1)


def mel_to_linear(mel_mag, fb, dtype=F64):
    """(frames, n_mels) x the (n_mels, nb) filterbank -> (frames, nb): the minimum-norm solution, clamped at zero."""
    pinv = torch.linalg.pinv(fb.to(F64)).to(dtype)                                             # (nb, n_mels)
    return (mel_mag.to(dtype) @ pinv.t()).clamp(min=0.0)


def griffin_lim(S, phases, n_iter, momentum, n_fft, hop, dtype=F64, fault=None):
    """The fast Griffin-Lim recursion of GriffinLim.magnitude_to_audio from given starting phases (frames, nb):
    alpha = m / (1 + m), no momentum term in the first iteration, normalisation by |.| + 1e-16."""
    S = S.to(dtype)
    ph = phases.to(dtype)
    ang = torch.stack([torch.cos(ph), torch.sin(ph)], 1)
    alpha = momentum if fault == "alpha" else momentum / (1 + momentum)
    tprev = None
    for _ in range(n_iter):
        rebuilt = stft3(istft(ang * S[:, None, :], n_fft, hop, dtype), n_fft, hop, dtype)
        ang = rebuilt if tprev is None else rebuilt - alpha * tprev
        ang = ang / (torch.sqrt((ang * ang).sum(1, keepdim=True)) + 1e-16)
        tprev = rebuilt
    return istft(ang * S[:, None, :], n_fft, hop, dtype)


VOCODER_GEOMETRIES = ("default", "small")
ISTFT_FRAMES = (2, 5, 141)
GL_FRAMES = 21
GL_ITERS = (1, 2)            # the recursion amplifies rounding: float32 sits at 1e-6 / 3e-6 / 1.4e-5 / 1.5e-2 after 1 / 2 / 4 / 8
GL_SEED = 3
MOMENTUM = 0.99


def random_spec(geom, frames):
    g = torch.Generator().manual_seed(40 + frames)
    return torch.randn(frames, 2, GEOMETRIES[geom]["n_fft"] // 2 + 1, generator=g)


def random_mel(geom, frames=7):
    """Positive mel magnitudes with no spectrum behind them: their minimum-norm solution has negative bins."""
    g = torch.Generator().manual_seed(50)
    return torch.rand(frames, GEOMETRIES[geom]["n_mels"], generator=g) * 3.0 + 0.01


def gl_input(geom):
    """(S, phases): the magnitude of a signal's own STFT (no silence: every frame has energy) and the seeded starting phases,
    drawn as GriffinLim.magnitude_to_audio draws them."""
    g = GEOMETRIES[geom]
    y = signal(geom, g["hop"] * (GL_FRAMES - 1), False)
    S = magnitude(stft_ri(y, g["n_fft"], g["hop"])).float()
    ph = 2 * np.pi * torch.rand(S.shape, generator=torch.Generator(device="cpu").manual_seed(GL_SEED))
    return S, ph


# -----------------------------------------------------------------------------------------------------------------
# mel -> wave: the HiFi-GAN layers on their margin buffers
# -----------------------------------------------------------------------------------------------------------------
PAD = 32                                     # hifigan.PAD (asserted equal in the GPU module)
CONV_CASES = [(80, 32, 7, 1), (32, 32, 11, 5), (64, 64, 7, 3), (16, 16, 3, 3), (8, 8, 11, 5), (8, 1, 7, 1)]     # (Ci, Co, k, d)
CONV_LENGTHS = (1, 2, 33, 130)
UP_CASES = [(32, 16, 8), (16, 8, 2), (64, 32, 4)]                                                                # (Ci, Co, u)
UP_LENGTHS = (1, 3, 40)
SENTINEL = -7777.0


def conv_inputs(case, L):
    Ci, Co, k, d = case
    g = torch.Generator().manual_seed(Ci * 1000 + k * 10 + d + 7 * L)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(L, Ci), w=r(Co, Ci, k) / math.sqrt(Ci * k), b=r(Co) * 0.1, res=r(L, Co))


def up_inputs(case, L):
    Ci, Co, u = case
    g = torch.Generator().manual_seed(Ci * 1000 + u + 7 * L)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(L, Ci), w=r(Ci, Co, 2 * u) / math.sqrt(2 * Ci), b=r(Co) * 0.1)


def conv1d(x, w, b, d, res=None, dtype=F64, fault=None):
    """(L, Ci) -> (L, Co) 'same' convolution (oracle.hifigan_ref.conv1d), plus the residual the accumulate epilogue starts from."""
    y = H.conv1d(x.to(dtype), w.to(dtype), b.to(dtype), d - 1 if fault == "dilation" else d)
    return y if res is None else res.to(dtype) + y


def conv_transpose1d(x, w, b, u, dtype=F64, fault=None):
    """(L, Ci) -> (L * u, Co): ConvTranspose1d(k = 2u, stride u, padding u / 2) (oracle.hifigan_ref.conv_transpose1d)."""
    if fault == "taps_swapped":
        w = torch.cat([w[:, :, u:], w[:, :, :u]], 2)
    return H.conv_transpose1d(x.to(dtype), w.to(dtype), b.to(dtype), u)


def margin_input(x, reach):
    """(L, C) -> the (L + 2 * PAD, C) buffer a layer reads: zero in the `reach` margin rows next to the data (the 'same' padding
    the kernels read), NaN in the rows farther out, which no kernel may read."""
    L, C = x.shape
    buf = torch.full((L + 2 * PAD, C), float("nan"))
    buf[PAD - reach:PAD + L + reach] = 0.0
    buf[PAD:PAD + L] = x
    return buf


def margin_expected(y, fill):
    """What the (L + 2 * PAD, C) output buffer holds after a layer call: y in the data rows, `fill` in both margins."""
    L, C = y.shape
    buf = torch.full((L + 2 * PAD, C), fill, dtype=y.dtype)
    buf[PAD:PAD + L] = y
    return buf


# -----------------------------------------------------------------------------------------------------------------
# Metrics
# -----------------------------------------------------------------------------------------------------------------
def rel(got, ref):
    """max|got - ref| / max|ref| over one utterance / one layer call; inf for a non-finite result."""
    got = got.double()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return math.inf
    return float((got - ref.double()).abs().max() / ref.double().abs().max())


def rel_l2(got, ref):
    got = got.double()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return math.inf
    return float((got - ref.double()).norm() / ref.double().norm())


def mel_figures(out, ref):
    """The three comparisons of a log-mel (frames, n_mels) against log_mel()'s dict:
    mel_lin: max_f max_m |exp(out) - max(lin, 1e-5)| / max(max_m lin[f], 1e-5);
    mel_log: max |out - log lin| over the elements with lin >= 1e-4;
    floor:   max |out - log(1e-5)| over silent frames and over empty filters in every frame (inf when something is not finite)."""
    out = out.double()
    lin = ref["lin"].double()
    if out.shape != lin.shape or not bool(torch.isfinite(out).all()):
        return dict(mel_lin=math.inf, mel_log=math.inf, floor=math.inf)
    lin_f = lin.clamp(min=FLOOR)
    figs = dict(mel_lin=float(((torch.exp(out) - lin_f).abs() / lin_f.max(1, keepdim=True)[0]).max()))
    cover = lin >= COVER
    figs["mel_log"] = float((out - torch.log(lin_f))[cover].abs().max()) if bool(cover.any()) else 0.0
    at_floor = ref["silent"][:, None] | ref["empty"][None, :]
    figs["floor"] = float((out - math.log(FLOOR))[at_floor].abs().max()) if bool(at_floor.any()) else 0.0
    return figs


def coverage(ref):
    """Share of the elements of non-silent frames in non-empty filters that the per-element log comparison covers."""
    live = (~ref["silent"])[:, None] & (~ref["empty"])[None, :]
    return float((ref["lin"][live] >= COVER).double().mean())


# -----------------------------------------------------------------------------------------------------------------
# Tolerances: ONE constant per output, from the references and not from the kernels (the rule of conv_path_ref.TOL):
#     TOL[k] = 16 x F32_ERR[k],   F32_ERR[k] = the largest figure of the float32 run of the reference against its float64 run over
# the case lists above, measured on the CPU with one thread and rounded up to two digits with >= 2 % of headroom.
# test_audio_ref_host.py re-measures every one and fails if a case exceeds its F32_ERR or if a stored constant is more than twice
# what it measures.  The factor 16 covers what legitimately differs between two correct float32 implementations: the GEMM's
# reduction order and operand split, the device's sqrt / log / sin / cos against libm's.
#   measured (worst case):
#     spec 9.41e-7 narrow_n8997 | mag 8.95e-7 narrow_n8997 | tmp 8.93e-7 narrow_n8997 | mel_lin 9.05e-7 narrow_n8997
#     mel_log 6.08e-5 narrow_n8997 | stft 6.81e-7 default_n35973 | istft 4.78e-7 default_f141 | mel_to_linear 2.53e-7 default
#     gl1 1.27e-6 default | gl2 1.43e-6 default | conv 2.93e-7 (8, 1, 7, 1)_L1 | conv_acc 1.47e-7 (64, 64, 7, 3)_L130
#     up 2.75e-7 (64, 32, 4)_L3
#   (mel_log: an element of 1e-4 in a frame whose loudest bin is 1e5 times that carries the frame's rounding, not its own)
# -----------------------------------------------------------------------------------------------------------------
F32_ERR = {
    "spec": 1.0e-6, "mag": 9.5e-7, "tmp": 9.5e-7, "mel_lin": 9.6e-7, "mel_log": 6.5e-5,
    "stft": 7.2e-7, "istft": 5.1e-7, "mel_to_linear": 2.7e-7, "gl1": 1.4e-6, "gl2": 1.6e-6,
    "conv": 3.1e-7, "conv_acc": 1.6e-7, "up": 2.9e-7,
}
TOL = {k: 16.0 * e for k, e in F32_ERR.items()}


def _worse(worst, key, e, name):
    if e > worst.get(key, (-1.0, ""))[0]:
        worst[key] = (e, name)


def measure_f32_err():
    """{output: (worst figure, case)} of the float32 restatement against float64 over every case list, one thread."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    worst = {}
    try:
        for geom in GEOMETRIES:
            for n in lengths(geom):
                r64, r32 = log_mel_case(geom, n), log_mel(signal(geom, n), geom, torch.float32)
                name = f"{geom}_n{n}"
                _worse(worst, "spec", rel(r32["spec"], r64["spec"]), name)
                _worse(worst, "mag", rel(r32["mag"], r64["mag"]), name)
                _worse(worst, "tmp", rel(r32["lin"], r64["lin"]), name)
                figs = mel_figures(r32["out"], r64)
                _worse(worst, "mel_lin", figs["mel_lin"], name)
                _worse(worst, "mel_log", figs["mel_log"], name)
        for geom in VOCODER_GEOMETRIES:
            g = GEOMETRIES[geom]
            n_fft, hop = g["n_fft"], g["hop"]
            for n in lengths(geom):
                y = signal(geom, n)
                _worse(worst, "stft", rel(stft3(y, n_fft, hop, torch.float32), stft3(y, n_fft, hop)), f"{geom}_n{n}")
            for frames in ISTFT_FRAMES:
                s = random_spec(geom, frames)
                _worse(worst, "istft", rel(istft(s, n_fft, hop, torch.float32), istft(s, n_fft, hop)), f"{geom}_f{frames}")
            fb = mel_filterbank(g["sr"], n_fft, g["n_mels"], g["f_min"], g["f_max"]).float()
            m = random_mel(geom)
            _worse(worst, "mel_to_linear", rel(mel_to_linear(m, fb, torch.float32), mel_to_linear(m, fb)), geom)
            S, ph = gl_input(geom)
            for it in GL_ITERS:
                e = rel_l2(griffin_lim(S, ph, it, MOMENTUM, n_fft, hop, torch.float32), griffin_lim(S, ph, it, MOMENTUM, n_fft, hop))
                _worse(worst, f"gl{it}", e, geom)
        for case in CONV_CASES:
            for L in CONV_LENGTHS:
                i = conv_inputs(case, L)
                name = f"{case}_L{L}"
                _worse(worst, "conv", rel(conv1d(i["x"], i["w"], i["b"], case[3], None, torch.float32), conv1d(i["x"], i["w"], i["b"], case[3])), name)
                _worse(worst, "conv_acc", rel(conv1d(i["x"], i["w"], i["b"], case[3], i["res"], torch.float32),
                                              conv1d(i["x"], i["w"], i["b"], case[3], i["res"])), name)
        for case in UP_CASES:
            for L in UP_LENGTHS:
                i = up_inputs(case, L)
                _worse(worst, "up", rel(conv_transpose1d(i["x"], i["w"], i["b"], case[2], torch.float32),
                                        conv_transpose1d(i["x"], i["w"], i["b"], case[2])), f"{case}_L{L}")
    finally:
        torch.set_num_threads(threads)
    return worst
