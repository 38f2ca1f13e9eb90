"""Float64-capable restatement of the model with a REDUCTION FACTOR r (every decoder step emits r consecutive mel frames), for tests.

Composed from the oracle's pieces (oracle/tacotron2_ref.py: encoder_fwd, condition, prenet_fwd, decoder_step, postnet_fwd,
tts_loss), which are shape-agnostic: decoder_step works unchanged with a (r*M)-row `decoder.mel_out`.  CPU only.

The rule, S = ceil(T / r) decoder steps for T frames:
  * row j*M + m of a step's projection is mel bin m of the step's j-th frame: frame s*r + j of `mels` is block j of step s;
  * the stop logit is one per step, repeated over the step's r frames in `gates`;
  * step 0 sees the zero frame, step s >= 1 the LAST frame of the previous group through the prenet: under teacher forcing frame
    r*s - 1 of the target (always < T), in decoding the predicted columns (r-1)*M .. r*M - 1 of the previous step;
  * frames at or beyond S*r > T are dropped; masking, postnet and loss run on the (B, T, M) frames as in the oracle;
  * `alignments` is (B, S, L), one row per step;
  * decoding: at most ceil(max_len / r) steps; the oracle's count rule on steps, lengths = min(r * counted steps, max_len); outputs
    have n = min(r * steps run, max_len) frames.
With r = 1 every line reduces to oracle.tacotron2_fwd (tests/test_reduction_factor_host.py checks exact equality in float64).

Masks (oracle convention, all optional): enc_drop [3 x (B,L,E)], post_drop [5 x (B,T,C)] per frame; prenet_drop per STEP - teacher
forcing [2 x (B,S+1,P)], decoding a list per step of [2 x (B,P)] (entry 0 for the zero frame); att_drop (S,B,A), dec_drop (S,B,D).

attention_hook: None, or a factory `hook = attention_hook(B, L, dtype)` whose result maps a step's softmax weights to the weights
the model uses: `w = hook(y, lmask)` (context, cumulative weights, returned alignments and the next step's location features all
use w).  `forward_attention_hook` is the rule of tests/forward_attention_chain_ref.py / tests/test_forward_attention_host.py."""
import torch

from oracle import tacotron2_ref as R


def steps_of(T, r):
    """ceil(T / r) for ints or integer tensors."""
    return (T + r - 1) // r


def teacher_slots(T, r):
    """Frame index held by slots 1 .. S of the teacher pack [S+1][B][M] (slot 0 is the zero frame): r*s - 1, or None where that
    lies behind the target (only slot S, which no step reads)."""
    return [r * s - 1 if r * s - 1 < T else None for s in range(1, steps_of(T, r) + 1)]


def decode_lengths(counted_steps, steps_run, r, max_len):
    """(lengths, n) of a decode: lengths = min(r * counted steps, max_len) per utterance, n = min(r * steps run, max_len) frames."""
    return torch.clamp(counted_steps * r, max=max_len), min(r * steps_run, max_len)


def grouped_params(P, d, r, seed=0):
    """A copy of the oracle-layout parameters `P` with seeded (r*M)-row `decoder.mel_out.weight` / `.bias` (the oracle's scales:
    uniform +-1/sqrt(fan_in), bias +-0.05); r = 1 returns an unchanged copy."""
    out = dict(P)
    if r == 1:
        return out
    g = torch.Generator().manual_seed(1000 + seed)
    w, b = P["decoder.mel_out.weight"], P["decoder.mel_out.bias"]
    M, K = w.shape
    bound = 1.0 / K ** 0.5
    out["decoder.mel_out.weight"] = ((torch.rand(r * M, K, generator=g, dtype=torch.float64) * 2 - 1) * bound).to(w.dtype)
    out["decoder.mel_out.bias"] = ((torch.rand(r * M, generator=g, dtype=torch.float64) * 2 - 1) * 0.05).to(b.dtype)
    return out


def forward_attention_hook(B, L, dtype):
    """alpha_t(n) = q_t(n) y_t(n) / sum_m q_t(m) y_t(m), q_t(n) = 0.5 alpha_{t-1}(n) + 0.5 alpha_{t-1}(n-1) + 1e-8, alpha_{-1} one-hot
    at position 0; exactly 0 at masked positions."""
    state = {"prior": None}

    def hook(y, lmask):
        prior = state["prior"]
        if prior is None:
            prior = torch.zeros(B, L, dtype=dtype)
            prior[:, 0] = 1.0
        shifted = torch.cat([torch.zeros_like(prior[:, :1]), prior[:, :-1]], 1)
        a = (0.5 * prior + 0.5 * shifted + 1e-8) * y
        a = (a / a.sum(1, keepdim=True)).masked_fill(lmask, 0.0)
        state["prior"] = a
        return a
    return hook


def _step(P, prev, st, memory, pm, lmask, att_drop, dec_drop, controls, hook):
    """One decoder step on the state tuple st = (att_h, att_c, ctx, w, w_cum, dec_h, dec_c) -> (mel (B, r*M), gate (B, 1), st).
    Without a hook this IS R.decoder_step; with one, its lines restated with the hook between the softmax and the context."""
    att_h, att_c, ctx, w, w_cum, dec_h, dec_c = st
    if hook is None:
        mel_o, gate_o, att_h, att_c, ctx, w, w_cum, dec_h, dec_c = R.decoder_step(
            P, prev, att_h, att_c, ctx, w, w_cum, dec_h, dec_c, memory, pm, lmask, att_drop, dec_drop, extra_decoder_in=controls)
        return mel_o, gate_o, (att_h, att_c, ctx, w, w_cum, dec_h, dec_c)
    g = torch.cat([prev, ctx], -1) @ P["decoder.att_rnn.weight_ih"].T + P["decoder.att_rnn.bias_ih"] \
        + att_h @ P["decoder.att_rnn.weight_hh"].T + P["decoder.att_rnn.bias_hh"]
    att_h, att_c = R.lstm_cell(g, att_c)
    if att_drop is not None:
        att_h = att_h * att_drop
    _, y = R.attention_fwd(P, att_h, memory, pm, torch.stack([w, w_cum], 1), lmask)
    w = hook(y, lmask)
    ctx = torch.einsum("bl,ble->be", w, memory)
    w_cum = w_cum + w
    xe = [controls] if controls is not None else []
    g = torch.cat([att_h, ctx] + xe, -1) @ P["decoder.lstm.weight_ih"].T + P["decoder.lstm.bias_ih"] \
        + dec_h @ P["decoder.lstm.weight_hh"].T + P["decoder.lstm.bias_hh"]
    dec_h, dec_c = R.lstm_cell(g, dec_c)
    if dec_drop is not None:
        dec_h = dec_h * dec_drop
    hc = torch.cat([dec_h, ctx], -1)
    gate_o = hc @ P["decoder.gate.weight"].T + P["decoder.gate.bias"]
    mel_o = torch.cat([hc] + xe, -1) @ P["decoder.mel_out.weight"].T + P["decoder.mel_out.bias"]
    return mel_o, gate_o, (att_h, att_c, ctx, w, w_cum, dec_h, dec_c)


def reduction_fwd(P, d, r, chars_idx, chars_len, teacher_forcing, mel=None, mel_len=None, speaker_id=None,
                  description_embeddings=None, max_len=None, training=True, masks=None, new_stats=None, controls=None,
                  attention_hook=None):
    """Teacher forcing: (mels (B,T,M), mels_post, gates (B,T,1), alignments (B,S,L)).  Decoding (teacher_forcing=False, max_len in
    frames): the same four with n frames / the steps run, and `lengths` (int64, frames) as a fifth."""
    masks = masks or {}
    dt = P["prenet.0.weight"].dtype
    B, L = chars_idx.shape
    M = d["num_mels"]
    assert P["decoder.mel_out.weight"].shape[0] == r * M
    encoded = R.encoder_fwd(P, chars_idx, chars_len, training, masks.get("enc_drop"), new_stats)
    memory, pm = R.condition(P, d, encoded, speaker_id, description_embeddings)
    lmask = torch.arange(L)[None, :] >= chars_len[:, None]
    A, D, Ef = d["att_rnn_dim"], d["rnn_hidden_dim"], memory.shape[2]
    z = lambda n: torch.zeros(B, n, dtype=dt)
    st = (z(A), z(A), z(Ef), z(L), z(L), z(D), z(D))
    hook = attention_hook(B, L, dt) if attention_hook is not None else None
    pd = masks.get("prenet_drop")
    ad, dd = masks.get("att_drop"), masks.get("dec_drop")
    if teacher_forcing:
        T = mel.shape[1]
        S = steps_of(T, r)
        # the teacher pack, S + 1 slots as the oracle's T + 1: the zero frame, then frame r*s - 1 (ESPnet's ys[:, r-1::r]); steps
        # 0 .. S-1 read slots 0 .. S-1
        slots = [mel[:, i] if i is not None else torch.zeros(B, M, dtype=dt) for i in teacher_slots(T, r)]
        dec_in = torch.cat([torch.zeros(B, 1, M, dtype=dt), torch.stack(slots, 1)], 1)
        dec_in = R.prenet_fwd(P, dec_in, pd[0] if pd else None, pd[1] if pd else None)
        lengths = mel_len.to(torch.int64)
    else:
        T = int(max_len)
        S = steps_of(T, r)
        prev = R.prenet_fwd(P, torch.zeros(B, M, dtype=dt), pd[0][0] if pd else None, pd[0][1] if pd else None)
        done = torch.zeros(B, dtype=torch.bool)
        counted = torch.zeros(B, dtype=torch.int64)
    mels, gates, aligns = [], [], []
    for s in range(S):
        if teacher_forcing:
            prev = dec_in[:, s]
        mel_o, gate_o, st = _step(P, prev, st, memory, pm, lmask, ad[s] if ad is not None else None,
                                  dd[s] if dd is not None else None, controls, hook)
        mels.append(mel_o.reshape(B, r, M)); gates.append(gate_o[:, None, :].expand(B, r, 1)); aligns.append(st[3])
        if not teacher_forcing:
            g = gate_o[:, 0]
            done = done | (g < 0.0)
            counted = counted + (g >= 0.0).to(torch.int64)
            if bool(done.all()):
                break
            prev = R.prenet_fwd(P, mel_o[:, (r - 1) * M:].detach(), pd[s + 1][0] if pd else None, pd[s + 1][1] if pd else None)
    if teacher_forcing:
        n = T
    else:
        lengths, n = decode_lengths(counted, len(mels), r, T)
    mels = torch.cat(mels, 1)[:, :n]; gates = torch.cat(gates, 1)[:, :n]; aligns = torch.stack(aligns, 1)
    post = mels + R.postnet_fwd(P, mels, training, masks.get("post_drop"), new_stats)
    mm = (torch.arange(n)[None, :] >= lengths[:, None])[:, :, None]
    out = (mels.masked_fill(mm, 0.0), post.masked_fill(mm, 0.0), gates.masked_fill(mm, -1000.0), aligns)
    return out if teacher_forcing else out + (lengths,)


def guided_mask_sum(align, chars_len, mel_len, r, sigma, alpha):
    """Closed form of the guided-attention loss over (B, S, L) alignments with the step lengths ceil(mel_len / r):
    alpha / B * sum_b sum_{s < T_b, l < N_b} (1 - exp(-(l/N_b - s/T_b)^2 / (2 sigma^2))) align[b, s, l] / (N_b T_b), in float64."""
    al = align.double()
    B, S, L = al.shape
    total = 0.0
    for b in range(B):
        Nb, Tb = min(int(chars_len[b]), L), min(int(steps_of(int(mel_len[b]), r)), S)
        if Nb * Tb == 0:
            continue
        l = torch.arange(Nb, dtype=torch.float64)[None, :] / Nb
        s = torch.arange(Tb, dtype=torch.float64)[:, None] / Tb
        G = 1.0 - torch.exp(-((l - s) ** 2) / (2.0 * sigma * sigma))
        total += float((G * al[b, :Tb, :Nb]).sum()) / (Nb * Tb)
    return alpha / B * total
