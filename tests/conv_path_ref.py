"""References for the kernel-level tests of everything around the conv stacks, the encoder BiLSTM and the conditioning
(include/tacotron2_amd.h: t2_bn_fwd / t2_bn_bwd, t2_embedding_*, t2_condition_*, t2_colsum, the conv weight layouts, t2_lstm_seq_fwd /
_persist_pz / t2_lstm_seq_bwd with n = 2, the pointwise glue): plain torch restatements with the dtype as a parameter, one function per
operation.  CPU only; nothing is imported from tacotron2_amd.  tests/test_conv_path_ref_host.py checks the restatements against
torch.nn / oracle.tacotron2_ref and anchors the constants below; tests/test_gpu_conv_path_kernels.py checks the kernels against the
restatements in float64.

The metric of both modules (rel below, attention_chain_ref.per_sample_rel): max over samples b of max|got_b - ref_b| / max|ref_b|;
outputs without a batch axis (statistics, parameter gradients, column sums) are compared over the whole tensor.

CASES holds the committed case lists, one list per kernel family; make_inputs(family, case) draws the float32 inputs the kernels get
(the float64 reference gets their exact upcasts); F32_ERR / TOL are the tolerance constants (see TOL)."""
import functools
import math
from collections import OrderedDict

import torch

from oracle import tacotron2_ref as R
from tests.attention_chain_ref import per_sample_rel

EPS, MOMENTUM = 1e-5, 0.1
KINK = 1e-4            # ReLU: elements with |pre-activation| <= KINK are left out of the backward comparison ...
KINK_SHARE = 1e-3      # ... and may be at most this share of the elements


# -----------------------------------------------------------------------------------------------------------------
# the operations
# -----------------------------------------------------------------------------------------------------------------
def _act(z, act):
    return torch.relu(z) if act == 1 else torch.tanh(z) if act == 2 else z


def bn(x, gamma, beta, rmean, rvar, training=True, act=0, drop=None, res=None, lens=None, fill=0.0, dtype=torch.float64,
       fault=None):
    """BatchNorm1d over the B*L rows of x (B, L, C), then act (0 none, 1 relu, 2 tanh), * drop, + res, rows l >= len[b] = fill, in
    that order.  Training: batch statistics, biased variance for the normalisation, running statistics updated with momentum 0.1
    and the UNBIASED variance; eval: the running statistics, left alone.  Returns y, mean, invstd, running_mean, running_var (the
    new ones) and pre (the normalised, scaled and shifted value the activation sees).
    fault: "biased_running_var", "res_before_drop", "fill_before_res", "tail_rows" (the statistics miss the rows >= 128)."""
    c = lambda t: None if t is None else t.to(dtype)
    x, gamma, beta, rmean, rvar, drop, res = (c(t) for t in (x, gamma, beta, rmean, rvar, drop, res))
    B, L, C = x.shape
    flat = x.reshape(B * L, C)
    if training:
        src = flat[:128] if fault == "tail_rows" else flat
        n = src.shape[0]
        mean = src.mean(0)
        var = ((src - mean) ** 2).mean(0)
        unb = var if fault == "biased_running_var" else var * (n / max(n - 1, 1))
        new_rm = (1 - MOMENTUM) * rmean + MOMENTUM * mean
        new_rv = (1 - MOMENTUM) * rvar + MOMENTUM * unb
    else:
        mean, var, new_rm, new_rv = rmean, rvar, rmean, rvar
    invstd = 1.0 / torch.sqrt(var + EPS)
    pre = (x - mean) * invstd * gamma + beta
    y = _act(pre, act)
    if fault == "res_before_drop" and res is not None:
        y = y + res
    if drop is not None:
        y = y * drop
    if lens is not None and fault == "fill_before_res":
        y = torch.where((torch.arange(L)[None, :] >= lens[:, None])[:, :, None], torch.full_like(y, fill), y)
    if res is not None and fault != "res_before_drop":
        y = y + res
    if lens is not None and fault != "fill_before_res":
        y = torch.where((torch.arange(L)[None, :] >= lens[:, None])[:, :, None], torch.full_like(y, fill), y)
    return dict(y=y, mean=mean, invstd=invstd, running_mean=new_rm, running_var=new_rv, pre=pre)


def bn_bwd(x, gamma, beta, rmean, rvar, dy, training=True, act=0, drop=None, dtype=torch.float64):
    """Autograd of  act(bn(x)) * drop  contracted with dy: dx, dgamma, dbeta.  The kernel's backward knows nothing of the residual or
    the length mask (the caller masks dy and routes the residual's gradient itself), so they are left out here too.  In eval mode the
    statistics are constants: dx = gamma * invstd * dz."""
    c = lambda t: None if t is None else t.to(dtype)
    xl, gl, bl = (c(t).clone().requires_grad_(True) for t in (x, gamma, beta))
    y = bn(xl, gl, bl, c(rmean), c(rvar), training, act, c(drop), dtype=dtype)["y"]
    dx, dgamma, dbeta = torch.autograd.grad((y * c(dy)).sum(), [xl, gl, bl])
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def sync_bn_stats(shards, shift, dtype=torch.float64, fault=None):
    """What the two phases of the synchronised statistics compute: every shard's sums of (x - shift) and (x - shift)^2 and its row
    count, added over the shards, then mean and 1/std of the whole batch.  fault "local_count": divided by shard 0's row count."""
    s1 = sum((s.to(dtype).reshape(-1, s.shape[-1]) - shift.to(dtype)).sum(0) for s in shards)
    s2 = sum(((s.to(dtype).reshape(-1, s.shape[-1]) - shift.to(dtype)) ** 2).sum(0) for s in shards)
    n = sum(s.shape[0] * s.shape[1] for s in shards)
    if fault == "local_count":
        n = shards[0].shape[0] * shards[0].shape[1]
    md = s1 / n
    var = (s2 / n - md * md).clamp(min=0)
    return dict(mean=md + shift.to(dtype), invstd=1.0 / torch.sqrt(var + EPS), var=var, n=n)


def embedding(idx, table, pad, dtype=torch.float64):
    """(B, L) ids -> (B, L + 2 pad, E): table rows at the data rows, zero rows around them."""
    B, L = idx.shape
    out = torch.zeros(B, L + 2 * pad, table.shape[1], dtype=dtype)
    out[:, pad:pad + L] = table.to(dtype)[idx]
    return out


def embedding_bwd(idx, dout, V, dtype=torch.float64, fault=None):
    """index_add of dout (B, L, E) into a (V, E) table gradient; row 0 (padding_idx) receives nothing.  fault: "row0"."""
    g = torch.zeros(V, dout.shape[-1], dtype=dtype)
    g.index_add_(0, idx.reshape(-1), dout.to(dtype).reshape(-1, dout.shape[-1]))
    if fault != "row0":
        g[0] = 0
    return g


def condition(enc, spk_table, spk, desc, dmem=None, dtype=torch.float64):
    """memory[..., :E] = tanh(enc + spk_table[spk]) (enc itself without a speaker table), memory[..., E:] = desc broadcast over L.
    With dmem: autograd's denc, dspk_table, ddesc too."""
    c = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(dmem is not None)
    e, tab, de = c(enc), c(spk_table), c(desc)
    m = e if tab is None else torch.tanh(e + tab[spk.long()][:, None, :])
    if de is not None:
        m = torch.cat([m, de[:, None, :].expand(-1, e.shape[1], -1)], 2)
    out = dict(memory=m.detach())
    if dmem is not None:
        leaves = [(k, t) for k, t in (("denc", e), ("dspk_table", tab), ("ddesc", de)) if t is not None]
        for (k, _), g in zip(leaves, torch.autograd.grad((m * dmem.to(dtype)).sum(), [t for _, t in leaves])):
            out[k] = g
    return out


def bilstm(pre, W_hh_f, W_hh_r, lens, denc=None, dtype=torch.float64, fault=None):
    """Both directions of a packed-sequence LSTM as an explicit loop.  pre (B, L, 8H) = the hoisted input projection, biases
    included, [forward 4H | reverse 4H], gate order i, f, g, o; a leaf.  Rows with t >= len[b] give h = c = 0 and leave the state
    alone, so the reverse direction starts at len[b] - 1.  Returns enc (B, L, 2H), c_final (2, B, H) and - with denc - autograd's
    dpre (B, L, 8H).  fault "reverse_from_L": the reverse direction's state runs through the rows behind len[b]."""
    B, L, H8 = pre.shape
    H = H8 // 8
    p = pre.to(dtype).clone().requires_grad_(denc is not None)
    outs, cf = [], []
    for d, W in enumerate((W_hh_f.to(dtype), W_hh_r.to(dtype))):
        h = torch.zeros(B, H, dtype=dtype)
        c = torch.zeros(B, H, dtype=dtype)
        col = [None] * L
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            hn, cn = R.lstm_cell(p[:, t, d * 4 * H:(d + 1) * 4 * H] + h @ W.T, c)
            act = (t < lens)[:, None]
            keep = torch.ones_like(act) if (fault == "reverse_from_L" and d == 1) else act
            h, c = torch.where(keep, hn, h), torch.where(keep, cn, c)
            col[t] = torch.where(act, hn, torch.zeros_like(hn))
        outs.append(torch.stack(col, 1))
        cf.append(c)
    enc = torch.cat(outs, 2)
    out = dict(enc=enc.detach(), c_final=torch.stack(cf, 0).detach())
    if denc is not None:
        out["dpre"] = torch.autograd.grad((enc * denc.to(dtype)).sum(), p)[0]
    return out


def colsum(x, dtype=torch.float64, fault=None):
    """sum over the rows of x (R, C), one row after the other (the plain loop; float32's error then grows with R as a kernel's
    partial sums do).  fault "drop_tail": without the last R % 4 rows."""
    R_ = x.shape[0] - (x.shape[0] % 4 if fault == "drop_tail" else 0)
    acc = torch.zeros(x.shape[1], dtype=dtype)
    for r in range(R_):
        acc = acc + x[r].to(dtype)
    return acc


def conv_grads(x, w, dy, dtype=torch.float64):
    """Gradients of the k = 5 'same' Conv1d (channel-last x (B, L, Ci), w (Co, Ci, K)) contracted with dy (B, L, Co)."""
    xl, wl = x.to(dtype).clone().requires_grad_(True), w.to(dtype).clone().requires_grad_(True)
    y = torch.nn.functional.conv1d(xl.transpose(1, 2), wl, padding=(w.shape[2] - 1) // 2).transpose(1, 2)
    dx, dw = torch.autograd.grad((y * dy.to(dtype)).sum(), [xl, wl])
    return dict(conv_dx=dx, conv_dw=dw)


def rel(got, ref, batched=True):
    """The metric: per_sample_rel over axis 0, or over the whole tensor for outputs without a batch axis."""
    if not batched:
        got, ref = got[None], ref[None]
    return per_sample_rel(got, ref)[0]


# -----------------------------------------------------------------------------------------------------------------
# The committed case lists
# -----------------------------------------------------------------------------------------------------------------
def _bn(name, B, L, C, level, act, drop=False, res=False, lens=False, training=True, dy_pad=False, prezeroed=False, shift=False):
    """res: the residual sits at (Lp, pad) = (L + 4, 2) and y at (L, 0) (the post-net's last layer).  lens: ragged lengths
    (len[0] = L, len[1] = 1) with fill = -3.5, dy masked behind them.  dy_pad: dy in the (L + 4, 2) layout, else (L, 0).
    prezeroed: sums_prezeroed = 1 with caller-zeroed sums, else 0 with NaN-filled sums.  shift: `shift` given in phase 0."""
    return name, dict(name=name, B=B, L=L, C=C, level=level, act=act, drop=drop, res=res, lens=lens, training=training,
                      dy_pad=dy_pad, prezeroed=prezeroed, shift=shift, fill=-3.5)


BN_CASES = OrderedDict([
    # (3, 45, 80): 135 rows = one full and one partial 128-row block, 135 % 4 = 3, two channel blocks with a 16-wide tail
    _bn("r135_relu_drop", 3, 45, 80, -5.5, 1, drop=True),
    _bn("r135_tanh_dypad", 3, 45, 80, 0.3, 2, dy_pad=True, prezeroed=True),
    _bn("r135_none_res_len", 3, 45, 80, 2.0, 0, drop=True, res=True, lens=True),
    _bn("r135_eval_relu", 3, 45, 80, -5.5, 1, drop=True, training=False),
    _bn("r135_eval_tanh_res", 3, 45, 80, 0.3, 2, res=True, training=False, dy_pad=True),
    _bn("r135_shift_tanh", 3, 45, 80, -5.5, 2, drop=True, shift=True, prezeroed=True),
    # (2, 3, 64): Lp = 7, n = 6 rows (the unbiased factor is 1.2)
    _bn("lp7_relu_drop", 2, 3, 64, -5.5, 1, drop=True, prezeroed=True),
    _bn("lp7_none_dypad", 2, 3, 64, 0.3, 0, dy_pad=True),
    _bn("lp7_eval_none_len", 2, 3, 64, 2.0, 0, lens=True, training=False),
    _bn("lp7_tanh_res_len", 2, 3, 64, 2.0, 2, drop=True, res=True, lens=True, prezeroed=True),
    # (5, 131, 200): 655 rows = five full blocks and one of 15, four channel blocks with an 8-wide tail
    _bn("r655_relu_drop_len", 5, 131, 200, -5.5, 1, drop=True, lens=True),
    _bn("r655_tanh_drop_dypad", 5, 131, 200, 0.3, 2, drop=True, dy_pad=True, prezeroed=True),
    _bn("r655_none_res", 5, 131, 200, 2.0, 0, res=True),
    _bn("r655_eval_tanh", 5, 131, 200, -5.5, 2, drop=True, training=False, prezeroed=True),
    _bn("r655_shift_relu", 5, 131, 200, 0.3, 1, shift=True, dy_pad=True),
    # (2, 9, 8): C < 64
    _bn("c8_relu", 2, 9, 8, 0.3, 1),
    _bn("c8_tanh_res_len", 2, 9, 8, 2.0, 2, res=True, lens=True, dy_pad=True),
    _bn("c8_eval_none", 2, 9, 8, -5.5, 0, drop=True, training=False),
    _bn("c8_none_drop", 2, 9, 8, -5.5, 0, drop=True, prezeroed=True),
    # (4, 1030, 256): the padded output has more than 4096 * 256 elements: the grid-stride loops of the apply kernels wrap
    _bn("wrap_tanh_drop", 4, 1030, 256, -5.5, 2, drop=True, prezeroed=True),
])

# a batch of 5 utterances as shards of 2 and 3; tiles: the phase-1 statistics from the producing GEMM's epilogue (the input is then
# the convolution's input, Ci channels, and the BatchNorm input is whatever the GEMM stored)
SYNC_BN_CASES = OrderedDict([
    ("sync_kernel_relu", dict(name="sync_kernel_relu", B=5, L=45, C=80, level=-5.5, act=1, drop=True, tiles=False)),
    ("sync_kernel_tanh", dict(name="sync_kernel_tanh", B=5, L=9, C=200, level=2.0, act=2, drop=False, tiles=False)),
    ("sync_tiles_tanh", dict(name="sync_tiles_tanh", B=5, L=45, C=80, Ci=32, level=-5.5, act=2, drop=True, tiles=True)),
])

EMBEDDING_CASES = OrderedDict((f"E{E}_B{B}_L{L}", dict(name=f"E{E}_B{B}_L{L}", E=E, B=B, L=L, V=6))
                              for E in (8, 80) for B, L in ((1, 1), (3, 50)))


def _cond(name, L, E, Ef, spk, ddesc):
    return name, dict(name=name, B=3, L=L, E=E, Ef=Ef, spk=spk, ddesc=ddesc, V=4)


CONDITION_CASES = OrderedDict([
    _cond("L1_E32_spk", 1, 32, 32, True, False),
    _cond("L16_Ef160_spk", 16, 32, 160, True, True),
    _cond("L17_Ef160_nospk", 17, 32, 160, False, True),
    _cond("L37_Ef328_spk", 37, 200, 328, True, True),
    _cond("L17_Ef328_spk_noddesc", 17, 200, 328, True, False),
    _cond("L37_E32_nospk", 37, 32, 32, False, False),
    _cond("L16_Ef328_nospk_noddesc", 16, 200, 328, False, False),
    _cond("L1_Ef160_spk", 1, 32, 160, True, True),
])

TANH_CASES = OrderedDict([("r3_c128", dict(name="r3_c128", rows=3, C=128)), ("wrap", dict(name="wrap", rows=4097, C=256))])

# (R, C, ld, base offset in floats): the first three take the generic kernel, the next four the 16-byte one (C % 4 == 0, C >= 256,
# ld % 4 == 0, 16-byte base), the last two are its fall-backs at C = 260
COLSUM_CASES = OrderedDict((f"R{R}_C{C}_ld{ld}_o{off}", dict(name=f"R{R}_C{C}_ld{ld}_o{off}", R=R, C=C, ld=ld, off=off))
                           for R, C, ld, off in ((3, 5, 5, 0), (300, 80, 96, 0), (1, 64, 64, 0), (33, 256, 256, 0), (1000, 260, 264, 0),
                                                 (1, 512, 512, 0), (29, 2592, 2592, 0), (1000, 260, 264, 1), (1000, 260, 261, 0)))

CONV_CASES = OrderedDict((f"Ci{Ci}_Co{Co}", dict(name=f"Ci{Ci}_Co{Co}", Ci=Ci, Co=Co, K=5, B=3, L=21)) for Ci, Co in ((32, 48), (80, 32)))

POINTWISE_SIZES = (1, 257, 4096 * 256 + 7)
SWAP01_SHAPES = ((1, 1, 1), (1, 257, 1), (257, 1, 1), (1, 1, 4096 * 256 + 7), (7, 5, 3), (5, 1030, 204))     # (D0, D1, C)

BILSTM_CASES = OrderedDict((f"B{B}_L{L}_H{H}", dict(name=f"B{B}_L{L}_H{H}", B=B, L=L, H=H)) for B, L, H in ((3, 7, 16), (17, 6, 32), (33, 5, 16)))

CASES = dict(bn=BN_CASES, sync_bn=SYNC_BN_CASES, embedding=EMBEDDING_CASES, condition=CONDITION_CASES, tanh=TANH_CASES,
             colsum=COLSUM_CASES, conv=CONV_CASES, bilstm=BILSTM_CASES)


def _lens(g, B, L):
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    if B > 1:
        lens[1] = 1
    return lens


def make_inputs(family, case, seed=None):
    """Seeded float32 inputs of one case, drawn on the CPU."""
    if seed is None:
        seed = 4000 + sum(ord(ch) for ch in family + case["name"])
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * sc).float()
    if family in ("bn", "sync_bn"):
        B, L, C, level = case["B"], case["L"], case["C"], case["level"]
        inp = dict(x=(level + 0.25 * torch.randn(B, L, C, generator=g, dtype=torch.float64)).float(),
                   gamma=(torch.rand(C, generator=g) + 0.5), beta=rn(C, sc=0.1),
                   running_mean=(level + rn(C, sc=0.05)), running_var=(0.0625 * (0.5 + torch.rand(C, generator=g))),
                   drop=(torch.rand(B, L, C, generator=g) >= 0.5).float() * 2, dy=rn(B, L, C), res=rn(B, L, C),
                   dgamma0=rn(C), dbeta0=rn(C), lens=_lens(g, B, L))
        if family == "sync_bn":
            inp["shift"] = inp["running_mean"].clone()
            if case["tiles"]:
                Ci = case["Ci"]
                inp["conv_x"] = (level + 0.25 * torch.randn(B, L, Ci, generator=g, dtype=torch.float64)).float()
                inp["conv_w"] = rn(C, 5 * Ci, sc=(5 * Ci) ** -0.5)
                inp["conv_b"] = rn(C)
            if not case["drop"]:
                inp["drop"] = None
            return inp
        inp["shift"] = inp["running_mean"].clone() if case["shift"] else None
        for k in ("drop", "res", "lens"):
            if not case[k]:
                inp[k] = None
        if case["lens"]:
            inp["dy"] = inp["dy"].masked_fill((torch.arange(L)[None, :] >= inp["lens"][:, None])[:, :, None], 0.0)
        return inp
    if family == "embedding":
        B, L, E, V = case["B"], case["L"], case["E"], case["V"]
        idx = torch.randint(0, V, (B, L), generator=g)
        if L > 1:
            idx[0, 0], idx[B - 1, L - 1], idx[0, 1] = 0, 0, V - 1
        else:
            idx[0, 0] = 0 if E == 80 else 3
        return dict(idx=idx, table=rn(V, E), dout=rn(B, L, E), dtable0=rn(V, E))
    if family == "condition":
        B, L, E, Ef, V = case["B"], case["L"], case["E"], case["Ef"], case["V"]
        return dict(enc=rn(B, L, E), spk_table=rn(V, E) if case["spk"] else None, spk=torch.tensor([2, 2, 0], dtype=torch.int32),
                    desc=rn(B, Ef - E) if Ef > E else None, dmem=rn(B, L, Ef), dspk_table0=rn(V, E))
    if family == "tanh":
        rows, C = case["rows"], case["C"]
        return dict(x=rn(rows, C, sc=1.5), bias=rn(C), g=rn(rows, C))
    if family == "colsum":
        return dict(x=(-5.5 + 0.25 * torch.randn(case["R"], case["C"], generator=g, dtype=torch.float64)).float(), out0=rn(case["C"]))
    if family == "conv":
        B, L, Ci, Co, K = (case[k] for k in ("B", "L", "Ci", "Co", "K"))
        return dict(x=rn(B, L, Ci), w=rn(Co, Ci, K, sc=(Ci * K) ** -0.5), dy=rn(B, L, Co), g0=rn(Co, Ci, K))
    if family == "bilstm":
        B, L, H = case["B"], case["L"], case["H"]
        return dict(pre=rn(B, L, 8 * H), W_hh_f=rn(4 * H, H, sc=H ** -0.5), W_hh_r=rn(4 * H, H, sc=H ** -0.5), lens=_lens(g, B, L),
                    denc=rn(B, L, 2 * H))
    raise KeyError(family)


def kink_mask(pre):
    """Elements that stay in the ReLU backward comparison, and the share that leaves it."""
    keep = pre.abs() > KINK
    return keep, 1.0 - float(keep.double().mean())


@functools.lru_cache(maxsize=None)
def bn_reference(name, dtype=torch.float64):
    """(inputs, forward reference, backward reference) of one BN_CASES entry, computed once and shared (treat as read-only).  With
    act = 1, dy is zero at the elements within KINK of the kink (from the FLOAT64 pre-activation, whatever `dtype` is)."""
    case = BN_CASES[name]
    inp = dict(make_inputs("bn", case))
    args = (inp["x"], inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"])
    kw = dict(training=case["training"], act=case["act"], drop=inp["drop"])
    if case["act"] == 1:
        pre64 = bn(*args, **kw)["pre"]
        keep, inp["kink_share"] = kink_mask(pre64)
        inp["dy"] = inp["dy"] * keep.float()
    fwd = bn(*args, res=inp["res"], lens=inp["lens"], fill=case["fill"], dtype=dtype, **kw)
    bwd = bn_bwd(*args, inp["dy"], dtype=dtype, **kw)
    return inp, fwd, bwd


# -----------------------------------------------------------------------------------------------------------------
# Tolerances: ONE constant per output for all cases of its family, from the references and not from the kernels (the standing rule
# of attention_chain_ref.TOL):
#     TOL[k] = 16 x F32_ERR[k],   F32_ERR[k] = the largest `rel` between the float32 and the float64 run of the reference over the
# family's case list, measured on the CPU with one thread and rounded up to two digits with >= 2 % of headroom.
# test_conv_path_ref_host.py re-measures every one of them and fails if a case exceeds its F32_ERR or if a stored constant is more
# than twice what it measures, so the constants cannot drift away from the references.  The factor 16 covers what legitimately
# differs between two correct float32 implementations: reduction orders (4 row lanes, 128-row blocks, atomics) and the device's
# exp / rcp against libm's.  Statistics keep the bounds of the two existing BatchNorm tests (STAT_BOUNDS).
# -----------------------------------------------------------------------------------------------------------------
#   measured (worst case of the family's list):
#     bn.y 7.52e-6 wrap_tanh_drop | bn.dx 4.81e-6 lp7_relu_drop | bn.dgamma 4.23e-6 r135_shift_tanh | bn.dbeta 1.94e-6 wrap_tanh_drop
#     embedding.dtable 1.18e-7 E8_B3_L50 | condition.memory 4.53e-8 L1_E32_spk | condition.denc 8.71e-8 L16_Ef160_spk
#     condition.dspk_table 1.65e-7 L16_Ef160_spk | condition.ddesc 1.64e-7 L16_Ef160_spk | tanh.y 5.63e-8 wrap | tanh.bwd 5.92e-8 wrap
#     colsum 1.74e-6 R1000_C260_ld261_o0 | conv.conv_dx 2.78e-7 Ci80_Co32 | conv.conv_dw 3.40e-7 Ci80_Co32
#     bilstm.enc 1.70e-7 B17_L6_H32 | bilstm.c_final 2.16e-7 B17_L6_H32 | bilstm.dpre 2.88e-7 B33_L5_H16
#   (bn.y / bn.dx: the float32 restatement takes the mean of up to 4120 values on a -5.5 level in float32 and subtracts it from
#    every element - 22 float32 epsilons of a 0.25 spread - which the kernels, with their statistics in double, do not)
F32_ERR = {
    "bn.y": 7.7e-6, "bn.dx": 5.0e-6, "bn.dgamma": 4.4e-6, "bn.dbeta": 2.0e-6,
    "embedding.dtable": 1.3e-7,
    "condition.memory": 4.7e-8, "condition.denc": 8.9e-8, "condition.dspk_table": 1.7e-7, "condition.ddesc": 1.7e-7,
    "tanh.y": 5.8e-8, "tanh.bwd": 6.1e-8,
    "colsum": 1.8e-6,
    "conv.conv_dx": 2.9e-7, "conv.conv_dw": 3.5e-7,
    "bilstm.enc": 1.8e-7, "bilstm.c_final": 2.3e-7, "bilstm.dpre": 3.0e-7,
}
TOL = {k: 16.0 * e for k, e in F32_ERR.items()}
# mean: absolute, x max(1, |level| + 1); invstd: relative, statistics kernel / GEMM-epilogue tiles; running statistics: absolute
STAT_BOUNDS = dict(mean=2e-6, invstd_kernel=2e-5, invstd_tiles=3e-6, running=1e-5)


def f32_errors(family, name):
    """{output: rel(float32 run, float64 run)} of one case: what F32_ERR is the maximum of."""
    case = CASES[family][name]
    out = {}
    if family == "bn":
        _, f64, b64 = bn_reference(name, torch.float64)
        _, f32, b32 = bn_reference(name, torch.float32)
        out["bn.y"] = rel(f32["y"], f64["y"])
        out["bn.dx"] = rel(b32["dx"], b64["dx"])
        out["bn.dgamma"] = rel(b32["dgamma"], b64["dgamma"], False)
        out["bn.dbeta"] = rel(b32["dbeta"], b64["dbeta"], False)
        return out
    inp = make_inputs(family, case)
    if family == "embedding":
        r = [embedding_bwd(inp["idx"], inp["dout"], case["V"], dt) for dt in (torch.float32, torch.float64)]
        out["embedding.dtable"] = rel(r[0], r[1], False)
    elif family == "condition":
        r = [condition(inp["enc"], inp["spk_table"], inp["spk"], inp["desc"], inp["dmem"], dt) for dt in (torch.float32, torch.float64)]
        for k in r[1]:
            out["condition." + k] = rel(r[0][k], r[1][k], k in ("memory", "denc", "ddesc"))
    elif family == "tanh":
        y = [torch.tanh(inp["x"].to(dt) + inp["bias"].to(dt)) for dt in (torch.float32, torch.float64)]
        out["tanh.y"] = rel(y[0], y[1], False)
        yk = y[0]                                        # the backward reads the float32 y a forward wrote
        b = [inp["g"].to(dt) * (1 - yk.to(dt) * yk.to(dt)) for dt in (torch.float32, torch.float64)]
        out["tanh.bwd"] = rel(b[0], b[1], False)
    elif family == "colsum":
        out["colsum"] = rel(inp["out0"] + colsum(inp["x"], torch.float32), inp["out0"].double() + colsum(inp["x"]), False)
    elif family == "conv":
        r = [conv_grads(inp["x"], inp["w"], inp["dy"], dt) for dt in (torch.float32, torch.float64)]
        out["conv.conv_dx"] = rel(r[0]["conv_dx"], r[1]["conv_dx"])
        out["conv.conv_dw"] = rel(inp["g0"] + r[0]["conv_dw"], inp["g0"].double() + r[1]["conv_dw"], False)
    elif family == "bilstm":
        r = [bilstm(inp["pre"], inp["W_hh_f"], inp["W_hh_r"], inp["lens"], inp["denc"], dt) for dt in (torch.float32, torch.float64)]
        out["bilstm.enc"] = rel(r[0]["enc"], r[1]["enc"])
        out["bilstm.c_final"] = rel(r[0]["c_final"].transpose(0, 1), r[1]["c_final"].transpose(0, 1))
        out["bilstm.dpre"] = rel(r[0]["dpre"], r[1]["dpre"])
    return out


F32_FAMILIES = ("bn", "embedding", "condition", "tanh", "colsum", "conv", "bilstm")


def measure_f32_err():
    """{output: (worst rel, case)} over every family's case list, one thread."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    worst = {}
    try:
        for fam in F32_FAMILIES:
            for name in CASES[fam]:
                for k, e in f32_errors(fam, name).items():
                    if e > worst.get(k, (-1.0, ""))[0]:
                        worst[k] = (e, name)
    finally:
        torch.set_num_threads(threads)
    return worst


def pad_rows_are_zero(buf, L, pad):
    """Every word of the rows outside [pad, pad + L) of a (B, Lp, C) buffer is exactly zero."""
    return bool((buf[:, :pad] == 0).all()) and bool((buf[:, pad + L:] == 0).all())


def one_rounding(got, ref64):
    """Largest |got - ref| in units of one float32 rounding of ref: half an ulp <= 2^-24 |ref| (the smallest subnormal at zero)."""
    bound = ref64.abs() * 2.0 ** -24 + 2.0 ** -149
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got.double() - ref64).abs() / bound).max()) if ref64.numel() else 0.0
