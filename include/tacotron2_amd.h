/* tacotron2_amd.h - C ABI of libtacotron2_amd.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * Tacotron 2 hot path of mattm458/tacotron2.
 *
 * The reference has NO native/FFI boundary: its hot path is nn.Module composition
 * (model/encoder.py, model/attention.py, model/decoder.py, model/postnet.py, model/tacotron2.py) and every
 * device kernel is an implicit ATen call.  This header is therefore the boundary a maintainer would bind
 * (ctypes) from those modules' forward()s; each entry cites the reference lines whose
 * ATen sequence it replaces.
 *
 * Conventions
 *  - plain C: raw DEVICE pointers, ints, floats; no torch / C++ types.  `stream` is a hipStream_t passed as
 *    void* (NULL = default stream).  Kernels are enqueued on it; nothing here synchronises or allocates
 *    (workspaces are passed in), so every entry is safe inside stream capture and re-entrant per stream.
 *  - every function returns 0 on success, a T2_ERR_* code otherwise, and never throws; t2_last_error()
 *    returns a human-readable message for the calling thread.
 *  - all floating point is fp32 (north_star), row-major, channel-last: (B,L,C) / (B,T,C); sequence stashes
 *    used by the frame loop are time-major [t][b][...].  LSTM gate order is PyTorch's i,f,g,o and weight
 *    matrices are [out][in] exactly as in the reference state_dict.
 *  - dropout is always an explicit *scale mask* tensor (0 or 1/(1-p)); NULL = identity.  Masks come from
 *    t2_philox_mask in production or from the caller in parity tests (SURVEY.md section 7 "Dropout RNG parity").
 */
#ifndef TACOTRON2_AMD_H
#define TACOTRON2_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define T2_OK 0
#define T2_ERR_ARG 1     /* bad argument / unsupported shape */
#define T2_ERR_LAUNCH 2  /* HIP launch or runtime error */
#define T2_ERR_RESIDENCY 3  /* a persistent launch would not be fully co-resident on this device (caller: use the per-step launches) */

const char* t2_last_error(void);
int t2_version(void);
int t2_sizeof(const char* struct_name); /* sizeof of an ABI struct by name, -1 if unknown */
/* diagnostic: enable/disable in-kernel clock stamps of the packed LSTM step kernel and read back 8 words: [0],[1] =
 * (s_memtime, s_memrealtime) at kernel entry of workgroup 0, [6],[7] = the same at its exit; [2..5] unused */
int t2_debug_clock(int enable, uint64_t* out8);

/* ------------------------------------------------------------------------------------------------
 * Generic fp32 MFMA GEMM:  C[M,N] (op)= alpha * A[M,K] x B[K,N]  (+ bias[n] + bias2[n]) (relu) (* mask[m,n])
 * Used for every dense contraction of the path: nn.Linear / nn.Conv1d (as GEMM over overlapping
 * channel-last rows) forward, dgrad and wgrad (model/tacotron2.py:85-92,229; model/encoder.py:33-39;
 * model/postnet.py:9-15; model/decoder.py:26-51 hoisted input projections).
 *   a_kmajor=1: A element (m,k) at A[m*lda + k];  a_kmajor=0: at A[k*lda + m]
 *   b_kmajor=1: B element (k,n) at B[n*ldb + k];  b_kmajor=0: at B[k*ldb + n]
 *   accumulate: 0 store, 1 C += result (plain), 2 C += result (fp32 atomics; required when splitk > 1)
 *   batch > 1: blockIdx.z strides A,B,C by sA,sB,sC elements.
 */
typedef struct {
    const float* A; const float* B; float* C;
    int M, N, K;
    int64_t lda, ldb, ldc;
    int a_kmajor, b_kmajor;
    float alpha;
    const float* bias; const float* bias2;
    const float* mulmask; int64_t ldmask;
    int relu;
    int accumulate;
    int splitk;
    int batch; int64_t sA, sB, sC;
    int share_cu;                    /* hint: 1 = keep ONE workgroup per CU (extra dynamic LDS), leaving LDS for the small kernels
                                        of a concurrent stream; two 73 KB workgroups per CU otherwise lock them out */
    int native_fp32;                 /* 0 (default): fp32 result on the bf16 matrix pipe by error-free 3-way operand splitting
                                        (6 exact bf16 products per element pair, two fp32 accumulators; csrc/t2_gemm.hip);
                                        1: v_mfma_f32_32x32x2_f32 (f32-input MFMA, 1/16 of the bf16 rate) */
    int a_tap_len; int64_t a_tap_stride;   /* optional (a_kmajor = 1): the K axis of A is a_tap_len-long blocks that are a_tap_stride
                                        elements apart: element (m, k) at A[m*lda + (k / a_tap_len)*a_tap_stride + k % a_tap_len].  A DILATED
                                        Conv1d(k, d) on channel-last rows is then ONE GEMM (tap block j = the Ci channels of row
                                        m + j*d: a_tap_len = Ci, a_tap_stride = d*Ci, lda = Ci) instead of k accumulating ones
                                        (model/hifi_gan.py:60-87).  a_tap_len must be a multiple of 32; 0 = plain rows */
    int precision;                   /* the reference's training.float32_matmul_precision (run/train.py:170), split kernel only:
                                        0 = "highest" (default): six bf16 products per element pair, fp32-exact operands;
                                        1 = "high": three products (a1b1 + a1b2 + a2b1, "bf16x3" in torch's terms, ~16
                                            significand bits); 2 = "medium": one bf16 product */
    float* stat_out; int stat_Lp, stat_L;  /* optional (split kernel, plain store): per-tile column statistics of the stored values for
                                        the BatchNorm that follows a conv-as-GEMM (model/encoder.py:33-41, model/postnet.py:9-16):
                                        stat_out[ceil(M/128)][3][N] = {shift, sum (v - shift), sum (v - shift)^2} over the tile's rows
                                        with row % stat_Lp < stat_L (real positions of the padded row layout); shift = the column's
                                        value at the tile's first such row.  t2_bn_fwd(tile_stats = ...) merges them (no atomics, no
                                        extra pass over the activations).  NULL = off */
} T2Gemm;
int t2_gemm(const T2Gemm* g, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One LSTM-cell step (nn.LSTMCell / one time step of nn.LSTM), M = batch rows on the MFMA M axis:
 *   gates[b][:] = pre[b][:] + bias1 + bias2 + sum_s x_s[b][0:K_s] . W_s[row][0:K_s]      (i,f,g,o blocks of H)
 *   c' = f*c + i*g ; h' = o*tanh(c') ; h' *= drop[b][:]         (the dropped h is the carried h,
 *                                                                model/decoder.py:75,101,114,118)
 * Replaces model/decoder.py:70-75 (att_rnn), :94-101 (lstm) and one step of model/encoder.py:64.
 * `len`/`t` (optional): rows with t >= len[b] are inactive: h' = c' = 0 (packed-sequence semantics,
 * model/encoder.py:61-65).
 */
typedef struct { const float* x; int64_t ldx; const float* w; int64_t ldw; int K; } T2Seg;
typedef struct {
    int B, H;
    int nseg; T2Seg seg[3];
    const float* wpacked;            /* optional lane-contiguous copy of the segment weights (t2_lstm_pack_fwd) */
    const float* pre; int64_t ldpre;
    const float* bias1; const float* bias2;
    const float* c_prev; int64_t ldc_prev;
    const float* drop; int64_t lddrop;
    float* h_out; int64_t ldh;       /* post-dropout h */
    float* h_out2; int64_t ldh2;     /* optional second copy (NULL to skip) */
    float* c_out; int64_t ldc_out;
    float* gates_out; int64_t ldg;   /* optional stash of the activated gates for backward, gate-interleaved: row b holds
                                        [u][4] = (i, f, g, o) of unit u (16-byte items; ldg >= 4H, 16-byte aligned rows) */
    const int32_t* len; int t;       /* optional activity predicate */
    /* x16-tiled operands (packed path only).  A (B x K) matrix in x16 layout is stored [K/16][Bp][16] with
     * Bp = round_up(B,16): one 16-row x 16-column MFMA operand tile is ONE contiguous 1 KB block, so a wave-load reads
     * 8 full cache lines instead of 16 half lines (measured 3.4 us per step at K = 1536, tools/ubench_cell.hip).
     * xt: tiled copy of the single input segment (replaces seg[0].x; rows >= B must be finite);
     * ht_out: tiled copy of h written at columns [ht_col0, ht_col0 + H) of a tiled matrix with the same Bp. */
    const float* xt;
    float* ht_out; int ht_col0;
    /* Zoneout (Krueger et al. 2017; ESPnet's ZoneOutCell), optional: with c~ and h~ the cell's results as above (h~ post-dropout),
     *   c' = zone_c * c_prev + (1 - zone_c) * c~ ;   h' = zone_h * h_prev + (1 - zone_h) * h~
     * are what every output carries (h_out, h_out2, ht_out, c_out; gates_out keeps the activated gates).  Masks are [B][H] floats
     * in [0, 1]: 0/1 draws in training (t2_philox_bernoulli), the rate itself in eval - one formula for both.  Either mask may be
     * NULL (reads as 0); with both NULL the step is exactly the step without these fields.  h_prev [B][H] is required with a
     * mask and may alias h_out (a thread reads only the element it then writes).  Masks together with `len` are an error. */
    const float* zone_h; int64_t ldzone_h;
    const float* zone_c; int64_t ldzone_c;
    const float* h_prev; int64_t ldh_prev;
} T2LstmStep;
/* n = 1 or 2 independent cells in one launch (the two directions of the encoder BiLSTM). */
int t2_lstm_step_fwd(const T2LstmStep* steps, int n, void* stream);
/* Weight streams re-laid once per optimisation step so that every wave-instruction of the step kernels reads one
 * contiguous 1 KB block (16 B per lane) instead of 16 rows with a power-of-two stride:
 *   fwd: out[H/4][NTpad][64][4],  NT = sum_s K_s/16;   bwd: out[ceil(ncols/16)][NCHpad][64][4] (transposed),
 *   NCH = N4/16 + N2/16; chunk counts are zero-padded (fwd: multiple of 16, bwd: multiple of 32) so the kernels' main
 *   loops are branch-free. */
int t2_lstm_pack_fwd(const T2Seg* segs, int nseg, int H, float* out, void* stream);
int t2_lstm_pack_bwd(const float* W, int64_t ldw, int N4, const float* W2, int64_t ldw2, int N2, int ncols, float* out,
                     void* stream);

/* S consecutive steps of a recurrence: step s uses base[i] with every non-NULL pointer advanced by
 * s * inc[i].<field> ELEMENTS (negative = time-descending, the reverse BiLSTM direction) and t += s*dt.
 * Replaces the packed nn.LSTM of model/encoder.py:59-65 and, with hoisted input projections, the
 * decoder-LSTMCell recurrence of model/decoder.py:94-101 over all frames (model/tacotron2.py:276-317). */
typedef struct {
    int64_t seg_x[3]; int64_t pre, c_prev, drop, h_out, h_out2, c_out, gates_out; int dt;
    int64_t xt, ht_out;
    int64_t zone_h, zone_c, h_prev;  /* 0 = the same [B][H] block at every step (eval: a block filled with the rate) */
} T2LstmStride;
int t2_lstm_seq_fwd(const T2LstmStep* base, const T2LstmStride* inc, int n, int S, void* stream);
/* The same S steps of ONE cell as ONE persistent, weight-stationary launch (csrc/t2_lstm.hip): every workgroup keeps its
 * weight slice in LDS and the workgroups exchange h_s through the x16-tiled stash (write-through stores, sharded arrival
 * counters, sc1 loads), so the launch can run on its own stream next to other work without streaming weights every step.
 * Needs: packed single-segment path with K = H, `pre` (hoisted input projection), B <= 64 (rows are independent: blocks of
 * 32 rows run as consecutive launches), H/4 <= 256 workgroups, base->ht_out == base->xt + inc->xt (step s+1 reads the tiled h
 * of step s), inc->xt == inc->ht_out.  h_out2 (a second plain copy of h with its own stride) is written when given.
 * sync: >= 272 device words of scratch; words [0, 256) are the arrival counters (zeroed by every launch), word 256 is the
 * timeout flag: zeroed by the CALLER before first use and sticky - a wait that timed out (bounded spins) sets it, every launch
 * that sees it ends early (outputs unusable) until the caller has read and cleared it.
 * Zoneout: the kernel keeps h of its own (row, unit) in a register across the steps as it keeps c; h_prev is read ONCE, at the first
 * step of the launch (inc->h_prev is not used). */
int t2_lstm_seq_fwd_persist(const T2LstmStep* base, const T2LstmStride* inc, int S, uint32_t* sync, void* stream);
/* n = 1 or 2 INDEPENDENT cells of the same B and H in one persistent launch (grid.y = n; base[i], inc[i]): the two directions of
 * the encoder BiLSTM (model/encoder.py:47-52), each walking its own way through time (inc[i] may be negative; base[i].len and
 * base[i].t + s * inc[i].dt give the packed-sequence masking).  n * H/4 <= 256 workgroups; cell i counts arrivals in words
 * [128 i, 128 i + 128) of `sync`, the timeout flag is word 256 for all. */
int t2_lstm_seq_fwd_persist_n(const T2LstmStep* base, const T2LstmStride* inc, int n, int S, uint32_t* sync, void* stream);
/* The same with the scratch split and the clearing left to the caller: `counters` = [ceil(B/32)][256] words that the caller has
 * ZEROED on this stream since their last use (the engine clears a ring of them once per step with t2_zero_regions instead of one
 * memset per launch), `flag` = the sticky timeout word. */
int t2_lstm_seq_fwd_persist_pz(const T2LstmStep* base, const T2LstmStride* inc, int n, int S, uint32_t* counters, uint32_t* flag,
                               void* stream);
/* Residency check of the persistent launch above, without launching anything: T2_OK when H/4 workgroups with this K's weight
 * slice in LDS are all co-resident (compute units of the current device x hipOccupancyMaxActiveBlocksPerMultiprocessor),
 * T2_ERR_RESIDENCY otherwise - the caller then runs the same steps as t2_lstm_seq_fwd launches.  t2_lstm_seq_fwd_persist makes
 * the same check itself and returns the same code. */
int t2_lstm_persist_resident(int H, int K, int B);
int t2_lstm_persist_resident_n(int H, int K, int B, int n);      /* the same for n cells per launch (n * H/4 workgroups) */
/* Clears up to 64 memory regions with ONE launch (the reference's `torch.zeros` / `zero_()` of its state tensors, e.g.
 * model/tacotron2.py:126-153 init_hidden - one ATen fill each).  Region i: nrows[i] rows of row_bytes[i] bytes, stride_bytes[i] apart
 * (nrows = 1: one contiguous run); pointers and sizes are multiples of 4 bytes. */
typedef struct {
    void* p[64];
    int64_t row_bytes[64];
    int64_t nrows[64];
    int64_t stride_bytes[64];
    int n;
} T2ZeroRegions;
int t2_zero_regions(const T2ZeroRegions* r, void* stream);
/* Stream-concurrency probe (no reference counterpart: the reference is single-stream, run/train.py:235-243).  The engine needs
 * its two streams on different hardware queues (tacotron2_amd/__init__.py); Trainer.queue_check times `n` dependent one-thread
 * launches on one stream (t2_stream_probe_chain: word[0] += 1 per launch) alone and next to ONE idle wave that holds the other
 * stream for `microseconds` of wall-clock time (t2_stream_probe_spin, bounded: <= 50 ms and <= 2^24 polls).  Streams that share a
 * queue serialise: the chain then takes the spin's time longer. */
int t2_stream_probe_chain(uint32_t* word, int n, void* stream);
int t2_stream_probe_spin(uint32_t* word, int microseconds, void* stream);
/* Debug / test hook: bound of the inter-workgroup waits of t2_lstm_seq_fwd_persist in polls (default 1 << 21; < 0: every wait
 * is treated as timed out, which raises the sticky flag sync[256] deterministically).  Returns the previous value. */
int t2_debug_persist_spin_limit(int polls);
/* Makes the sticky timeout flag of the persistent launches (sync[256]) fatal without a host synchronisation: if *flag != 0,
 * x[0..n) is overwritten with NaN (the engine passes the decoder projection of the forward, so every output, the loss and
 * every gradient of that step become NaN and t2_adam_step - which skips a step whose gradient norm is not finite - leaves
 * the weights alone).  The host raises at its next synchronisation point. */
int t2_guard_poison(const uint32_t* flag, float* x, int64_t n, void* stream);
/* One step of back-propagation through time for an LSTM cell (autograd of the cells above):
 *   dx[b][u] = sum_n dg_next[b][n] * W[n*ldw + u]          (n over N4 = 4H' rows of the producing cell)
 *   epi = 0: dx_out = dx + ext1 + ext2                      (gradient w.r.t. a non-recurrent input slice)
 *   epi = 1: dh = (dx + ext1 + ext2) * drop; pointwise cell backward with the stashed activations of
 *            step t -> dg_out[b][4H] (pre-activation gate grads), dc[b][H] updated in place.
 * dg_next may be NULL (last frame: no recurrent contribution). */
typedef struct {
    int B, H, N4;
    const float* dg_next; int64_t lddg;
    const float* W; int64_t ldw;
    const float* dg2; int64_t lddg2; const float* W2; int64_t ldw2; int N2;  /* optional second K segment (+= dg2 . W2) */
    const float* wtpacked;           /* optional lane-contiguous transposed copy of W (and W2) (t2_lstm_pack_bwd) */
    int ncols; int epi;
    const float* ext1; int64_t ldx1; const float* ext2; int64_t ldx2;
    float* dx_out; int64_t lddx;
    const float* drop; int64_t lddrop;
    const float* gates; int64_t ldgs;       /* the forward stash, gate-interleaved [b][u][4] (T2LstmStep.gates_out) */
    const float* c_prev; int64_t ldcp; const float* c_cur; int64_t ldcc;
    float* dc; int64_t lddc;
    float* dg_out; int64_t ldgo;
    float* dg_out2; int64_t ldgo2;          /* optional second copy of dg_out with its own row stride */
    const int32_t* len; int t;
    /* x16-tiled operands (packed path only, layout as in T2LstmStep): dgt_next = tiled copy of dg_next ([N4/16][Bp][16]),
     * read instead of dg_next (which must still be non-NULL); dgt_out = tiled copy of dg_out ([4H/16][Bp][16]). */
    const float* dgt_next;
    float* dgt_out;
    int off_chain;                          /* 1: this step is NOT on the critical chain of its stream schedule (the decoder-LSTM BPTT,
                                               a chunk ahead on the side stream): its waves keep the default issue priority instead
                                               of the chain kernels' raised one */
    /* Zoneout (T2LstmStep), epi = 1 only.  With Dh = (dx + ext1 + ext2) + dhz and Dc = dc going in:
     *   dh~ = (1 - zone_h) * Dh * drop ;  dhz <- zone_h * Dh  (the share of h_{t-1}, read by the next launch = step t-1)
     *   tc  = tanh(c~), c~ = f * c_prev + i * g RECOMPUTED from the stash (where zone_c > 0, c_cur is not c~; c_cur is not read)
     *   dc~ = (1 - zone_c) * Dc + dh~ * o * (1 - tc^2) ;  d_o = dh~ * tc * o (1 - o) ;  d_i, d_f, d_g from dc~ as without masks
     *   dc <- dc~ * f + zone_c * Dc
     * dhz [B][H] is an in/out carry like dc (the caller zero-fills both before the last step), required with a mask.  With both
     * masks NULL, dhz is not touched and the step is exactly the step without these fields.  Not together with `len`. */
    const float* zone_h; int64_t ldzone_h;
    const float* zone_c; int64_t ldzone_c;
    float* dhz; int64_t lddhz;
} T2LstmBwdStep;
int t2_lstm_step_bwd(const T2LstmBwdStep* steps, int n, void* stream);
typedef struct { int64_t dg, dg2, ext1, ext2, drop, gates, c_prev, c_cur; int dt; int64_t dgt; int64_t zone_h, zone_c; } T2LstmBwdStride;
/* S steps; every pointer advances by its stride each step.  The caller lays the dgates stash out with one extra
 * zero-filled slot so that base[i].dg_next (the slot 'after' the first processed step) is valid and zero. */
int t2_lstm_seq_bwd(const T2LstmBwdStep* base, const T2LstmBwdStride* inc, int n, int S, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Location-sensitive attention, one frame (model/attention.py:52-69 + cumulative update model/decoder.py:78-90).
 *   U   [Ad][2][Kl]  = location_dense.weight . location_conv.weight, folded once per forward by
 *                      t2_attn_fold_location (pure re-association of two linear maps)
 *   pmT [B][Ad][L]   = processed memory (att_encoder output, model/tacotron2.py:229) stored transposed
 *   len [B] int32    : positions l >= len[b] are masked to -inf before the softmax (model/attention.py:63)
 *   e_part           : workspace [B][Ad/16][L];  th_out: optional stash [B][Ad][L4] of tanh(.) for backward, rows padded
 *                      to L4 = round_up(L,4) floats (16-byte aligned; must be 16-byte aligned itself)
 * Any text length whose per-sample images fit the 160 KB of LDS (energies kernel: 24 bytes per position - about 6,000 characters);
 * the kernels walk texts above 256 positions in rounds.
 * Writes w_out (new attention weights = the alignments row), cum_out = cum_prev + w, ctx_out (context).
 *
 * Windowed attention (inference only; ESPnet's attention constraint, Mozilla TTS's `windowing`): with win_peak != NULL,
 * win_back, win_fwd >= 0, frame t of utterance b attends only to the positions
 *     max(0, m[b] - win_back) <= l <= min(len[b] - 1, m[b] + win_fwd),   m[b] = win_peak[0][b] = the previous frame's peak
 * (every other position gets energy -inf before the softmax: its weight is exactly 0 and w_out / cum_out are not written
 * there).  The step then writes win_peak[0][b] = m_t[b], the argmax of its weights (lowest position on ties, as torch.argmax).
 * Before the first frame the caller zero-fills row 0 (m_{-1} = 0).  Row 1 is the step's own hand-off from the energies to the
 * context launch (the previous peak: a launch's readers of the old peak and its writer of the new one are different workgroups).
 * The location features still read w_prev / cum_prev over the full row (the window +- (Kl-1)/2 positions), so w_prev must be
 * the previous frame's full weights row (zero outside its window).  Energies, softmax and context touch only the window: the
 * work and bytes per frame follow its width, not L.  The cumulative weights are updated in place (cum_out == cum_prev
 * required), th_out must be NULL.  A window as wide as the text (win_back, win_fwd >= L) is the unconstrained step.
 *
 * Forward attention (autoregressive decoding only; Zhang et al. 2018, Mozilla TTS's `forward_attn` without a transition agent):
 * with forward != 0 the step carries a probability over monotonic paths - attention stays where it is or advances one position
 * per frame.  For utterance b with length len, frame t >= 0 and position n:
 *     y_t(n)     = the softmax over the masked energies of frame t (model/attention.py:52-69); the energies come from the location
 *                  features of [alpha_{t-1}, cum_{t-1}] exactly as without the option: the weights fed back (w_prev) are the forward
 *                  weights alpha, and at frame 0 the location features see zeros
 *     q_t(n)     = 0.5 alpha_{t-1}(n) + 0.5 alpha_{t-1}(n-1) + 1e-8,   alpha_{t-1}(-1) = 0
 *     alpha_{-1} = one-hot at position 0 (w_prev == NULL): q_0(0) = q_0(1) = 0.5 + 1e-8, q_0(n) = 1e-8 elsewhere.  The 1e-8 floor
 *                  keeps the sum positive when the softmax puts its mass where the prior is zero
 *     alpha_t(n) = q_t(n) y_t(n) / sum_m q_t(m) y_t(m) for n < len, exactly 0.0 for n >= len
 * Everything downstream uses alpha_t: the context sum_n alpha_t(n) memory(n), cum_t = cum_{t-1} + alpha_t, the returned
 * alignments row (w_out) and the next frame's location features.  The softmax denominator cancels, so the kernel multiplies
 * each exp term by q before its one block sum.  forward together with win_peak or with th_out is an argument error (the teacher-forced chain, T2AttnSeq.forward, keeps the stash); w_out must
 * not be w_prev (every workgroup of the context launch reads w_prev, one of them writes w_out). */
typedef struct {
    int B, L, A, Ad, Ef, Kl;
    const float* att_h; int64_t ldh;
    const float* Wq; const float* U; const float* v;
    const float* w_prev; int64_t ldw;        /* NULL = zeros (first frame) */
    const float* cum_prev; int64_t ldcum;    /* NULL = zeros */
    const float* pmT; const float* memory; const int32_t* len;
    float* e_part; float* th_out;
    float* w_out; int64_t ldwo; float* cum_out; int64_t ldco;
    float* ctx_out; int64_t ldctx; float* ctx_out2; int64_t ldctx2;
    float* ctxt_out; int ctxt_col0;          /* optional x16-tiled copy of the context (see T2LstmStep) */
    uint64_t* clk;                           /* diagnostic, normally NULL: 32 device words; workgroup (0,0) stamps the shader
                                                clock (s_memtime) at phase boundaries: energies [0..3], context [8..13] */
    int win_back, win_fwd;                   /* attention window (with win_peak): see "Windowed attention" above */
    int32_t* win_peak;                       /* NULL = unconstrained (the whole text); else [2][B] int32 device words */
    int forward;                             /* 0 = off; else forward attention: see "Forward attention" above */
} T2AttnStep;
int t2_attn_fold_location(const float* Wd, const float* Wc, float* U, int Ad, int F, int Kl, void* stream);
int t2_attn_step_fwd(const T2AttnStep* s, void* stream);

/* Teacher-forced attention chain over all T frames (the attention half of the loop at
 * model/tacotron2.py:276-317; in teacher-forced mode it does not depend on the decoder LSTM, so the two
 * recurrences are run as separate chains with their input projections hoisted into large GEMMs).
 * Time-major stashes use slot s = t+1; the caller zero-fills slot 0 (initial states, model/tacotron2.py:126-153).
 *   pre   [T][B][4A]     prenet part of att_rnn.weight_ih + both biases (hoisted GEMM)
 *   xdec  [T+1][B][A+Ef] cols [0,A) = att_h_t (post-dropout), cols [A,A+Ef) = context_t
 *   att_c [T+1][B][A], gates [T][B][4A] (activated, optional), cum [T+1][B][L], th [T][B][Ad][L4] (optional, L4 = round_up(L,4))
 *   align [B][T][L]      the alignments output
 *   xproj_ctx            optional second copy of context_t, row (t,b) at xproj_ctx[(t*B+b)*ld_xproj] */
typedef struct {
    int B, L, T, A, Ad, Ef, Kl;
    const float* W_ih_ctx; int64_t ld_wih;
    const float* W_hh; const float* Wq; const float* U; const float* v;
    const float* wpacked;            /* optional t2_lstm_pack_fwd of segments (W_ih_ctx, Ef), (W_hh, A) */
    const float* pre; const float* pmT; const float* memory; const int32_t* len;
    const float* att_drop;
    float* xdec; float* att_c; float* gates; float* align; float* cum; float* th;
    float* xproj_ctx; int64_t ld_xproj;
    float* e_part;
    int t_begin, t_end;              /* frame range [t_begin, t_end) of this call; 0,0 = all T frames */
    float* xdec_t;                   /* optional (with wpacked): x16-tiled copy of xdec, [T+1][(A+Ef)/16][Bp][16], slot 0
                                        zero-filled by the caller; the attention-LSTM step then reads its input from it */
    uint64_t* clk;                   /* diagnostic (T2AttnStep.clk), normally NULL */
    int forward;                     /* 0 = off; else every frame is a forward-attention step (T2AttnStep.forward, "Forward attention"
                                        above) that keeps its tanh stash: training under the monotonic prior.  Frame 0 has the one-hot
                                        prior; a call with t_begin > 0 reads alpha_{t_begin-1} from `align` */
} T2AttnSeq;
int t2_attn_seq_fwd(const T2AttnSeq* a, void* stream);

/* Back-propagation through the attention chain, frames T-1 .. 0 (autograd of t2_attn_seq_fwd), 4 launches / frame:
 *   one launch for both products of dgates[t+1] (dctx_tot[t] = dctx_ext1[t] + dctx_ext2[t] + dgates[t+1].W_ih_ctx and
 *   dh_rec = dh_ext[t] + dgates[t+1].W_hh) ; attention backward (weights/energies, then per attention-dim slice) ;
 *   attention-LSTM cell backward with dh = dh_rec + dq[t].Wq.
 * Upstream gradients are time-major rows (t,b) with their own leading dimensions.  Outputs: dgates = Z [T+1][B][4A+Ad]
 * with Z[s][b] = [dgates_s (4A) | dq_{s-1} (Ad)] (the caller zero-fills slot T's first 4A columns; `dq` is unused),
 * dctx_tot [T][B][Ef] (inputs of the post-loop weight-gradient GEMMs) and the per-sample
 * accumulators dpmT [B][Ad][L], dv_part [B][Ad], dU_part [B][Ad][2][Kl] (caller zero-fills; summed over b after).
 * Workspaces: dc [B][A] (zero-filled), G [2][B][L], de [B][L], din_part [B][Ad/16][2][L].
 * Texts of up to 252 positions take the per-slice kernel in one pass; longer ones are walked in position tiles of 216 (+ 16 on
 * either side: a tile's gradient reaches 15 positions beyond it through the location filter) inside the same launch - no length
 * limit but the LDS (8 bytes per position for the location-input gradient of the whole text, 42 KB for a tile). */
typedef struct {
    int B, L, T, A, Ad, Ef, Kl;
    const float* W_ih_ctx; int64_t ld_wih;
    const float* W_hh; const float* Wq; const float* U; const float* v;
    const float* wtp_ctx;            /* optional t2_lstm_pack_bwd(W_ih_ctx, ncols = Ef) */
    const float* wtp_h;              /* t2_lstm_pack_bwd(W_hh, A, 4A, ncols = A) */
    const float* wtp_q;              /* t2_lstm_pack_bwd(Wq, A, Ad, ncols = A) */
    const float* memory; const float* xdec; const float* att_c; const float* gates; const float* align;
    const float* cum; const float* th; const float* att_drop;
    const float* dh_ext; int64_t ld_dh;
    const float* dctx_ext1; int64_t ld_dc1;
    const float* dctx_ext2; int64_t ld_dc2;
    float* dgates; float* dctx_tot; float* dq; float* dpmT; float* dv_part; float* dU_part;
    float* dc; float* G; float* de; float* din_part;
    float* dh_rec;                   /* workspace [B][A]: dh_ext[t] + dgates[t+1].W_hh */
    int t_hi, t_lo;                  /* frames t_hi-1 .. t_lo of this call (descending); 0,0 = T-1 .. 0 */
    float* dgates_t;                 /* optional x16-tiled copy of the dgates part of Z: [T+1][4A/16][Bp][16], slot T
                                        zero-filled by the caller; read by the per-frame products of dgates[t+1] */
    uint64_t* clk;                   /* diagnostic, normally NULL: 128 zeroed device words, read by the -DT2_STAMPS build only: s_memtime
                                        stamps of workgroup (0,0) at phase boundaries of the dw kernel [16..19] and the ds kernel
                                        [24..30]; [32] event counter and [40..127] a ring of the last 11 launches of the frame chain
                                        (products, dw, ds, cell backward) with wall-clock entry / exit and phase stamps (t2_common.hpp) */
    float* ws_bd;                    /* workspace of (Ad/16) * 16896 floats: the per-slice kernel runs its two correlations (dU, d_in)
                                        on the bf16 matrix pipe with exactly split operands (six products, fp32 accuracy); the
                                        workspace receives the d_in filter operand in fragment layout, rewritten by every call */
    const float* dalign;             /* optional upstream gradient w.r.t. the alignments AS RETURNED (each w_t after the softmax, before
                                        it is added into the cumulative weights), layout of `align`: frame t of utterance b at
                                        dalign + (b*T + t)*L, every frame (also those behind an utterance's mel length).  It joins the
                                        softmax backward of the frame's first launch, de[l] = w[l] * (dw[l] + dwx[l] + da[l] - sigma)
                                        with sigma = sum_l w[l] * (dw[l] + dwx[l] + da[l]), and nothing else: not the
                                        cumulative-weights carry G.  NULL = no such gradient (the same loads and arithmetic as without
                                        the operand) */
} T2AttnSeqBwd;
int t2_attn_seq_bwd(const T2AttnSeqBwd* a, void* stream);

/* The same chain with the three accumulators nothing on it waits for (dpmT, dv_part, dU_part) taken off it.
 *   t2_attn_seq_bwd_stash: frame t writes its energy gradients to de_stash + t * ld_stash ([B][L], ld_stash >= B * L; the
 *   stash spans all T frames) instead of the reused workspace `de`, and the per-slice launch computes only what the next launch
 *   needs (ds -> dq, the location-input gradient); dpmT, dv_part and dU_part are NOT touched.  de_stash = NULL: exactly
 *   t2_attn_seq_bwd.
 *   t2_attn_acc_bwd: one launch, grid (B, Ad/16), for the frames t_end-1 .. t_begin (the chain's order) that a stash call has
 *   finished: rebuilds ds from the stashed de, the tanh stash and v, keeps its dpmT slice, dv and dU sums in registers over
 *   the frames and adds them to dpmT / dv_part / dU_part once.  It may run on another stream behind the chain call's event;
 *   calls for different frame ranges must not overlap each other (plain read-modify-write, no atomics).  It reads th, align,
 *   cum, v, dpmT, dv_part, dU_part and the dims of `a`.  Sums are re-associated per call: results match t2_attn_seq_bwd to
 *   rounding, not bit for bit; everything else the chain writes is bit-identical.
 * Texts longer than one pass (L > 252) ignore the stash: t2_attn_seq_bwd_stash accumulates in the chain as t2_attn_seq_bwd
 * does, and t2_attn_acc_bwd returns without a launch.
 * (The stash travels as arguments: T2AttnSeqBwd keeps its layout.) */
int t2_attn_seq_bwd_stash(const T2AttnSeqBwd* a, float* de_stash, int64_t ld_stash, void* stream);
/* The backward of a t2_attn_seq_fwd with T2AttnSeq.forward != 0 (forward attention under teacher forcing): t2_attn_seq_bwd_stash
 * (de_stash = NULL: t2_attn_seq_bwd) with the prior's term in the softmax backward.  The weights are
 * alpha_t = softmax(e_t + log q_t), so with g_t = dw + dwx + da + P_{t+1} (P_T = 0):
 *     de_t[l] = alpha_t[l] (g_t[l] - sum_m alpha_t[m] g_t[m])
 *     r_t[l]  = de_t[l] / q_t[l]                       (t >= 1; exactly 0 behind len)
 *     P_t[n]  = 0.5 r_t[n] + 0.5 r_t[n+1],   r_t[L] = 0
 * P_t is the gradient frame t hands to alpha_{t-1} through its prior (none from frame 0: its prior is a constant).  It reaches
 * alpha_{t-1} directly, as dalign does: it is not part of the cumulative-weights carry G.  Same launches per frame (the first one is
 * another instantiation of the same kernel); everything else - the per-slice launches, t2_attn_acc_bwd on the stash - is unchanged:
 * they are functions of de, th, align and cum.
 *   dprior: workspace [2][B][L].  Frame t writes r_t (every position < L) into slot t & 1 - the ABSOLUTE frame's parity - and
 *   frame t-1 reads it, so (t_hi, t_lo) calls carry it from one call to the next as they carry G.  No zero-fill.
 * dprior == NULL or a->align == NULL is T2_ERR_ARG before any launch.  (The workspace travels as an argument: T2AttnSeqBwd keeps
 * its layout.) */
int t2_attn_seq_bwd_forward(const T2AttnSeqBwd* a, float* de_stash, int64_t ld_stash, float* dprior, void* stream);
int t2_attn_acc_bwd(const T2AttnSeqBwd* a, const float* de_stash, int64_t ld_stash, int t_begin, int t_end, void* stream);
/* Zoneout on the attention-LSTM cell of the chain (T2LstmStep.zone_h / zone_c).  The masks travel as an operand block of their own, as
 * the stash and the forward-attention workspace travel as arguments: `forward` stays the last field of T2AttnSeq and `dalign` the last
 * of T2AttnSeqBwd, which the ABI tests of those two options assert (tests/test_forward_attention_chain_host.py,
 * tests/test_guided_attention_host.py: the field's offset against the struct's size).
 *   zone_h, zone_c: frame t reads the [B][A] block at zone_x + t * stride (stride 0 = one block for every frame: eval); either may be
 *                   NULL.  h_prev of frame t is slot t of xdec; att_c then holds the zoned c and xdec the zoned h.
 *   dhz           : backward only, required with a mask: in/out carry [B][A] (T2LstmBwdStep.dhz), zero-filled by the caller where dc
 *                   is.  The cell backward of the chain adds it where it forms dh = dh_rec + dq.Wq.
 * t2_attn_seq_fwd_zone is t2_attn_seq_fwd with the masks; t2_attn_seq_bwd_zone is t2_attn_seq_bwd_stash (de_stash may be NULL) or, with
 * dprior != NULL, t2_attn_seq_bwd_forward, with the masks.  z == NULL or both masks NULL: exactly those calls. */
typedef struct { const float* zone_h; const float* zone_c; int64_t stride; float* dhz; } T2AttnZone;
int t2_attn_seq_fwd_zone(const T2AttnSeq* a, const T2AttnZone* z, void* stream);
int t2_attn_seq_bwd_zone(const T2AttnSeqBwd* a, float* de_stash, int64_t ld_stash, float* dprior, const T2AttnZone* z, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Conv stacks (encoder model/encoder.py:31-46,57; postnet model/postnet.py:8-49).
 * Activations use the padded channel-last layout (B, Lp = L+4, C): data rows [2, L+2), zero rows elsewhere, so a
 * k=5 'same' Conv1d is one t2_gemm with overlapping A rows (lda = C, K = 5C) against packed weights.
 *   t2_pack_conv_weight   flip=0: wp[co][k*Ci+ci] = w[co][ci][k]  (forward / wgrad layout)
 *                         flip=1: wp[ci][(K-1-k)*Co+co] = w[co][ci][k]  (dgrad: correlation with the flipped kernel)
 *   t2_unpack_conv_wgrad  g[co][ci][k] += gp[co][k*Ci+ci]
 */
int t2_embedding_fwd(const int64_t* idx, const float* table, float* out, int B, int L, int E, int pad, void* stream);
int t2_embedding_bwd(const int64_t* idx, const float* dout, float* dtable, int B, int L, int E, int Lp, int pad, void* stream);
int t2_pack_conv_weight(const float* w, float* wp, int Co, int Ci, int K, int flip, void* stream);
int t2_unpack_conv_wgrad(const float* gp, float* g, int Co, int Ci, int K, void* stream);

/* BatchNorm1d (+ activation + dropout mask [+ residual + length mask]) over the B*L valid rows of a raw conv
 * output in shifted row layout (row b*Lp_x + l).  training: batch statistics incl. padded positions, running
 * stats updated with momentum (unbiased variance), exactly nn.BatchNorm1d; eval: running statistics.
 * forward  (t2_bn_fwd): y[b][pad_y + l][c] = mask(act(bn(x))*drop + res); pad rows of y are zero-filled.
 * backward (t2_bn_bwd): dx (grad w.r.t. x, written at rows b*Lp_dx + pad_dx + l, other rows zero), dgamma/dbeta +=.
 * act: 0 none, 1 relu, 2 tanh.  sums: workspace of 2*C + 2 doubles (two sums per channel, then the row count they cover).
 * Synchronised statistics over data-parallel ranks (model/encoder.py:41, model/postnet.py:16,30,44 see the WHOLE batch in the
 * single-device reference): phase 1 = accumulate the sums only, the caller all-reduces `sums` (count included), phase 2 =
 * finalize + apply from the reduced sums; `shift` [C] must then be a rank-independent shift of the statistics sums (the
 * running mean), and in the backward `grad_share` = 1/world scales this rank's dgamma/dbeta contribution (the gradient
 * all-reduce adds the ranks' shares).  phase 0 / shift NULL / grad_share 0 = single-device behaviour. */
typedef struct {
    int B, L, C;
    const float* x; int Lp_x;
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;
    int training; float momentum, eps;
    double* sums;
    float* mean; float* invstd;
    int act;
    const float* drop;
    const float* res; int Lp_res, pad_res;
    const int32_t* len; float fill;
    float* y; int Lp_y, pad_y;
    const float* dy; int Lp_dy, pad_dy;
    float* dx; int Lp_dx, pad_dx;
    float* dgamma; float* dbeta;
    int phase; const float* shift; float grad_share;
    int sums_prezeroed;          /* 1: the caller has cleared `sums` on this stream (e.g. as one region of t2_zero_regions) */
    const float* tile_stats; int tile_M;   /* forward, training: the producing GEMM's T2Gemm.stat_out and its M (rows of the GEMM):
                                    the batch statistics come from these per-tile partials (merged in double) instead of a pass
                                    over x; NULL = the statistics kernel */
} T2Bn;
int t2_bn_fwd(const T2Bn* s, void* stream);
int t2_bn_bwd(const T2Bn* s, void* stream);

/* small data-movement / pointwise pieces of model/tacotron2.py:201-212,255,327-345 and model/tts_model.py:197-201 */
int t2_colsum(const float* x, int64_t ld, int64_t R, int C, float* out, void* stream);          /* out[c] += sum_r x[r][c] */
int t2_mel_to_tm(const float* mel, float* out, int B, int T, int M, void* stream);              /* (B,T,M) -> [T+1][B][M], slot 0 = 0 */
int t2_swap01(const float* in, float* out, int D0, int D1, int C, int accumulate, void* stream); /* (D0,D1,C) -> (D1,D0,C) */
int t2_finalize_fwd(const float* proj, int64_t ld_proj, const int32_t* len, float* mels, float* gates, float* post_in, int B,
                    int T, int M, void* stream);
int t2_finalize_bwd(const float* dpost_in, float* dproj, int B, int T, int M, void* stream);
/* upstream gradients of (mels, mels_post, gates) (any may be NULL) -> d_post_out (B,T,M) and dproj [T][B][M+1], masked */
int t2_outgrad_pack(const float* d_mels, const float* d_post, const float* d_gates, const int32_t* len, float* d_post_out,
                    float* dproj, int B, int T, int M, void* stream);
int t2_loss_fwd_bwd(const float* mels, const float* post, const float* gates, const float* mel_tgt, const float* gate_tgt,
                    const int32_t* len, int B, int T, int M, double* loss3 /* gate, mel, post */, float* d_post, float* dproj,
                    float grad_scale, void* stream);
/* The same three loss terms for the nn.Module surface (TTSModel.training_step / validation_step, model/tts_model.py:165-253): loss3
 * and - each optional - the dense gradients w.r.t. mels (B,T,M), mels_post (B,T,M) and gates (B,T,1), zero at masked positions. */
int t2_loss_terms(const float* mels, const float* post, const float* gates, const float* mel_tgt, const float* gate_tgt,
                  const int32_t* len, int B, int T, int M, double* loss3, float* d_mels, float* d_post, float* d_gates,
                  float grad_scale, void* stream);
/* Guided-attention loss (Tachibana et al. 2018) on the alignments (B,T,L) of a teacher-forced forward: value and gradient in ONE launch.
 *   G[b][t][l] = 1 - exp(-(l/N_b - t/T_b)^2 / (2 sigma^2))      for t < T_b and l < N_b, else 0
 *   loss       = alpha / B * sum_b ( sum_{t,l} G[b][t][l] * align[b][t][l] ) / (N_b * T_b)
 *   dalign     = grad_scale * alpha / (B * N_b * T_b) * G[b][t][l]    (optional; written over the whole (B,T,L), zeros included)
 * N_b = chars_len[b] clipped to [0, L], T_b = mel_len[b] clipped to [0, T] (device int32); an utterance with N_b * T_b == 0
 * contributes nothing.  The mean is taken per utterance and then over the batch (equal shards averaged = the whole batch).  The
 * loss is accumulated in double into ONE device double; sigma > 0, alpha >= 0 (customary: 0.4, 1.0). */
int t2_guided_attn(const float* align, const int32_t* chars_len, const int32_t* mel_len, int B, int T, int L, float sigma,
                   float alpha, double* loss, float* dalign, float grad_scale, void* stream);
/* Reduction factor r >= 1 (a decoder step emits r consecutive mel frames; S = ceil(T / r) steps for T frames): the boundary kernels
 * above with a run-time r.  Each operation has ONE kernel body; the entry points without the suffix run it with r = 1 as a constant,
 * and so do these when r == 1 - their results are then those of the entry point above, bit for bit.  r <= 0 is refused (rc = 1), and so
 * is B, T or M < 1, at r == 1 too (the entry points without the suffix do not check that).  A step's projection row is [r*M + 1] wide: column j*M + m is mel bin m of frame s*r + j, column r*M
 * the step's ONE stop logit.  Frames at or beyond T of the last step are dropped (forward) / get a zero gradient (backward).
 *   t2_mel_to_tm_r     (B,T,M) -> [S+1][B][M]: slot 0 = 0, slot s = frame r*s - 1, the LAST frame of the previous group (0 where r*s - 1 >= T:
 *                      only slot S, which no step reads)
 *   t2_finalize_fwd_r  proj [S][B][ld_proj] -> mels (B,T,M) masked 0, gates (B,T,1) = the step's logit repeated over its frames,
 *                      masked -1000, post_in (B,T+4,M) padded layout (unmasked)
 *   t2_finalize_bwd_r  dproj[s][b][j*M + m] += dpost_in[b][s*r + j][m]
 *   t2_outgrad_pack_r / t2_loss_fwd_bwd_r  as t2_outgrad_pack / t2_loss_fwd_bwd (the same three sums, the same d_post) with dproj
 *                      [S][B][r*M+1]; the gradient of a step's stop logit is the sum over its frames below T and below len[b],
 *                      formed by one thread per (b, s) - no atomics.  d_post and dproj are required. */
int t2_mel_to_tm_r(const float* mel, float* out, int B, int T, int M, int r, void* stream);
int t2_finalize_fwd_r(const float* proj, int64_t ld_proj, const int32_t* len, float* mels, float* gates, float* post_in, int B,
                      int T, int M, int r, void* stream);
int t2_finalize_bwd_r(const float* dpost_in, float* dproj, int B, int T, int M, int r, void* stream);
int t2_outgrad_pack_r(const float* d_mels, const float* d_post, const float* d_gates, const int32_t* len, float* d_post_out,
                      float* dproj, int B, int T, int M, int r, void* stream);
int t2_loss_fwd_bwd_r(const float* mels, const float* post, const float* gates, const float* mel_tgt, const float* gate_tgt,
                      const int32_t* len, int B, int T, int M, int r, double* loss3, float* d_post, float* dproj,
                      float grad_scale, void* stream);
/* Loss options (no reference counterpart: model/tts_model.py:197-201 is the plain mean of three terms over the padded batch).
 * With len[b] the utterance's mel length a frame (b, t) is VALID when t < min(len[b], T); n_f = the number of valid frames.
 *   mel_loss    0 = l2 (the reference), 1 = l1: |e|, gradient sign(e) with sign(0) = 0, 2 = l1+l2: the sum of the two means; for both
 *               mel terms.  loss3 stays {gate, mel, post}.
 *   masked      != 0: the three sums run over the valid frames only; the gate term is divided by n_f, the mel terms by n_f * M.  n_f is
 *               formed on the device inside the same launch (every workgroup sums min(len[b], T) before its loop: no host read, no
 *               second launch).  Invalid positions of the five tensors are not READ (NaN or Inf there reaches neither loss3 nor a
 *               gradient); their gradients are written as 0.  n_f == 0: zero terms and zero gradients.
 *   stop_weight w > 0 on the STOP class (gate target 0: one frame per utterance, datasets/tts_dataset.py:213-214): per frame
 *               y softplus(-x) + w (1 - y) softplus(x), gradient sigmoid(x) (y + w (1 - y)) - y; the divisor stays the plain count
 *               (B*T, or n_f when masked) - torch's pos_weight convention mirrored onto the other class.  w == 1 is the unweighted
 *               expression, not the general formula.
 * t2_loss_fwd_bwd_opt = t2_loss_fwd_bwd_r (r >= 1) and t2_loss_terms_opt = t2_loss_terms with the options; {0, 0, 1.0f} forwards to those
 * entries after this entry's own checks (bit for bit their results), anything else launches a further instantiation of the same
 * kernel body.  With a reduction factor the gate term still counts frames and dproj's gate column is the sum over the step's frames.
 * NULL options, mel_loss outside {0, 1, 2}, a stop_weight that is not finite or <= 0, and B, T or M < 1 are refused (rc = 1) before
 * anything is launched. */
typedef struct { int mel_loss; int masked; float stop_weight; } T2LossOpts;
int t2_loss_fwd_bwd_opt(const float* mels, const float* post, const float* gates, const float* mel_tgt, const float* gate_tgt,
                        const int32_t* len, int B, int T, int M, int r, double* loss3, float* d_post, float* dproj,
                        float grad_scale, const T2LossOpts* opts, void* stream);
int t2_loss_terms_opt(const float* mels, const float* post, const float* gates, const float* mel_tgt, const float* gate_tgt,
                      const int32_t* len, int B, int T, int M, double* loss3, float* d_mels, float* d_post, float* d_gates,
                      float grad_scale, const T2LossOpts* opts, void* stream);
int t2_relu_mask_bwd(const float* g, const float* y, const float* mask, float* out, int64_t n, void* stream);
int t2_condition_fwd(const float* enc, const float* spk_table, const int32_t* spk, const float* desc, float* memory, int B,
                     int L, int E, int Ef, void* stream);
/* dspk_table and ddesc are ACCUMULATED into (atomics): the caller zero-fills ddesc */
int t2_condition_bwd(const float* dmem, const float* memory, const int32_t* spk, float* denc, float* dspk_table, float* ddesc,
                     int B, int L, int E, int Ef, void* stream);
int t2_tanh_bias(float* x, const float* bias, int64_t rows, int C, void* stream);
/* HiFi-GAN V1 generator glue (model/hifi_gan.py:89-97,139-144,198-216; every convolution of the generator is t2_gemm over
 * overlapping / shifted channel-last rows): y = leaky_relu(scale * x, slope) and y += alpha * x */
int t2_leaky_relu(const float* x, float* y, int64_t n, float scale, float slope, void* stream);
int t2_axpy(const float* x, float* y, int64_t n, float alpha, void* stream);
int t2_tanh_bwd(const float* g, const float* y, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Autoregressive decoding: forward(teacher_forcing=False, max_len_override=N) of model/tacotron2.py:262-325.
 *   t2_linear_rows  out[b][n] = act(x[b][:] . w[n][:] + bias[n]) * mask[b][n]   (nn.Linear on <= batch rows; K % 16 == 0)
 *   t2_decoder_infer runs frames [t0, t1) of one group of <= 64 utterances with no host synchronisation, 6 launches per
 *   frame: state[0] = "every utterance of the group has stopped" (sticky), state[1] = frames emitted, done [B] int32.
 *   The first prenet layer is folded onto the mel projection (two linear maps with nothing in between):
 *     W_comb [(P+M+1)][D+Ef] = [W_pre1 . W_mel ; W_mel ; W_gate],  b_comb [(P+M+1)] = [W_pre1 . b_mel ; b_mel ; b_gate],
 *     row_comb (optional) [B][P+M+1] = per-utterance term of the prosody controls ([W_pre1 . cmel_b ; cmel_b ; 0])
 *   (built by the caller with t2_gemm once per call), so frame t's first launch yields p1_t AND the outputs of frame t-1
 *   from xproj_{t-1}, every sum in a fixed order (bit-reproducible stop decisions).
 *   t2_stop_scan derives the reference's break frame and `lengths` (model/tacotron2.py:319-322: counts every emitted frame
 *   whose stop logit is >= 0, Appendix C.4) from the stored logits of all groups, so groups may be decoded a few frames past
 *   the break (the host looks at state[0] only now and then; with several groups all run until ALL have stopped, exactly as
 *   the reference's single loop over the whole batch does).
 * Buffers: xs [2][(P+A+Ef+D)/16][Bp][16] = the recurrent state in the x16-tiled layout of T2LstmStep.xt, columns
 * [prenet_out | att_h | ctx | dec_h], two ping-pong slots, zero-filled by the caller (P, A, Ef, D multiples of 16);
 * att_h [B][A] and xproj [B][D+Ef] = [dec_h | ctx] row-major copies; p1 [B][P] prenet scratch;
 * att_c [2][B][A], dec_c [2][B][D], cum [2][B][L] (ping-pong, slot 0 zero-filled by the caller);
 * proj [Tcap][B][ld_proj] (cols 0..M-1 mel, col M stop logit; row t is written by the first launch of frame t+1 or by the
 * call's tail); align [B][Tcap][L]; prenet_mask [frames][2][B][P] or NULL (frame 0's masks are never read);
 * wp_att = t2_lstm_pack_fwd of the attention-LSTM weights in the column order [prenet | att_h | ctx],
 * wp_dec = t2_lstm_pack_fwd of the decoder-LSTM weights in the column order [att_h | ctx | dec_h]. */
int t2_linear_rows(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* mask,
                   int64_t ldmask, int relu, float* out, int64_t ldo, int B, int N, int K, void* stream);
typedef struct {
    int B, L, A, D, Ef, Ad, P, M, Kl, Tcap;
    const float* W_comb; const float* b_comb; const float* row_comb;
    const float* W_pre2;
    /* optional x16-tiled copies (layout of T2LstmStep.xt: [K/16][rows padded to 16][16]) of the two small linears' operands:
     * W_comb_t [(Ef+D)/16][Npad][16] with the K chunks in the order [ctx | dec_h] (the order of the tiled state), Npad =
     * round_up(P+M+1, 16); W_pre2_t [P/16][P][16]; p1_t [P/16][Bp][16] scratch.  With them every wave-load of these launches is
     * one contiguous 1 KB block (NULL: row-major operands, 16 half cache lines per wave-load). */
    const float* W_comb_t; const float* W_pre2_t; float* p1_t;
    const float* wp_att; const float* b_att_ih; const float* b_att_hh;
    const float* wp_dec; const float* b_dec_ih; const float* b_dec_hh;
    const float* Wq; const float* U; const float* v;
    const float* pmT; const float* memory; const int32_t* len;
    const float* prenet_mask;
    float* xs; float* att_h; float* att_c; float* dec_c; float* cum; float* xproj; float* p1; float* e_part;
    float* proj; int64_t ld_proj; float* align;
    int32_t* done; int32_t* state;
    const float* dec_pre;            /* optional [B][4D]: per-utterance term added to the decoder-LSTM pre-activations of
                                        every frame (controls . W_ih[:, A+Ef:]^T, model/decoder.py:94-99) */
    int win_back, win_fwd;           /* attention window (T2AttnStep), >= 0; only read when win_peak != NULL */
    int32_t* win_peak;               /* NULL = unconstrained attention (as before); else [2][B] int32, zero-filled by the caller
                                        before frame 0: the windowed attention step of every frame (T2AttnStep), with the
                                        cumulative weights kept in place in cum slot 0 (slot 1 unused) */
    int forward;                     /* 0 = off; else forward attention in every frame (T2AttnStep.forward; frame 0 starts from the
                                        one-hot prior).  Not together with win_peak */
    float zone_p;                    /* zoneout rate of both cells in decoding (the expectation rule: every mask element is the rate);
                                        0 = off.  Otherwise zone_att [B][A] and zone_dec [B][D] are blocks the caller has FILLED with
                                        zone_p (each serves as zone_h and zone_c of its cell).  The cells write h in place (att_h, the
                                        dec_h columns of xproj), so h_prev aliases h_out - a thread reads only the element it then
                                        writes; both buffers must therefore be zero-filled before frame 0, like the c slots */
    const float* zone_att; const float* zone_dec;
    float stop_logit;                /* stop threshold as a logit: a step stops when its stop logit < stop_logit.  0 = the reference's
                                        rule (model/tacotron2.py:319-322: gate < 0, sigmoid < 0.5); for a threshold 0 < tau < 1 the
                                        caller passes log(tau / (1 - tau)) formed in double and rounded to float - the SAME float it
                                        gives t2_stop_scan_thr, so the in-loop flags and the scan agree exactly.  Must be finite */
} T2Infer;
int t2_decoder_infer(const T2Infer* a, int t0, int t1, void* stream);
/* proj[g] [nframes][Bg[g]][ld_proj] for g < ngroups (<= 64 groups of up to 64 utterances) -> lengths [sum Bg] int64,
 * out2 = {frames emitted n, 0} */
typedef struct { const float* proj[64]; int Bg[64]; int ngroups; int64_t ld_proj; int M, nframes; } T2StopScan;
int t2_stop_scan(const T2StopScan* s, int64_t* lengths, int32_t* out2, void* stream);
/* With a reduction factor r the decode loop runs unchanged on steps: T2Infer.M = r * num_mels, the first prenet layer folded
 * onto the LAST block of the projection (W_comb = [W_pre1 . W_mel[(r-1)M : rM] ; W_mel ; W_gate], b_comb and row_comb alike), Tcap
 * and align in steps.  t2_stop_scan_r (r >= 1, max_len >= 1) applies the count rule to the `nframes` stored STEPS (T2StopScan.M =
 * r * num_mels): lengths [sum Bg] = min(r * counted steps, max_len) frames, out2 = {frames emitted = min(r * steps, max_len), steps
 * emitted}.  At r = 1 that is t2_stop_scan's result cut at max_len, with the steps in out2[1]. */
int t2_stop_scan_r(const T2StopScan* s, int r, int max_len, int64_t* lengths, int32_t* out2, void* stream);
/* The same scan against a stop threshold (T2Infer.stop_logit; departs from model/tacotron2.py:319-322, which compares with 0): a step
 * stops when logit < stop_logit, and the count rule counts the steps with logit >= stop_logit; the break after the last utterance's
 * first stop, the steps and the max_len cut are unchanged.  t2_stop_scan_r is the stop_logit = 0.0f call of the same body.  A
 * stop_logit that is not finite is refused (rc = 1). */
int t2_stop_scan_thr(const T2StopScan* s, int r, int max_len, float stop_logit, int64_t* lengths, int32_t* out2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-character durations from alignments (no reference counterpart; the teacher export that duration-based models such as
 * FastSpeech train on, and character timestamps at decode time): how many mel frames each input character lasts, from the
 * (B, S, L) alignments of a teacher-forced forward or of a decode.  One launch, one 256-thread workgroup per utterance
 * (csrc/t2_align.hip); no cross-workgroup synchronisation, no atomics to global memory.
 *   N_b = clip(chars_len[b], 0, L) characters, F_b = clip(frames_len[b], 0, r*S) mel frames, S_b = ceil(F_b / r) decoder steps.
 *   Frames per step: step s < S_b - 1 carries r frames, the last step F_b - r*(S_b - 1).  Every step is assigned ONE position
 *   pos[s] < N_b; dur[b][n] = the sum of the frames of the steps assigned to n, so sum_n dur[b][n] == F_b always; dur[b][n] = 0
 *   for N_b <= n < L.
 *   mode 0 (argmax): pos[s] = the LOWEST n < N_b with the largest align[b][s][n].
 *   mode 1 (monotonic; the monotonic alignment search of Glow-TTS, Kim et al. 2020): the best path that starts on the first
 *     character, ends on the last and stays or advances by one per step.  With la[s][n] = log((double)fmaxf(a, 1e-8f)):
 *       Q[0][0] = la[0][0], Q[0][n > 0] = -inf;   Q[s][n] = la[s][n] + max(Q[s-1][n], Q[s-1][n-1])
 *     the predecessor of (s, n) is n-1 only when Q[s-1][n-1] > Q[s-1][n] STRICTLY (a tie stays at n); pos is the backtrack
 *     from (S_b - 1, N_b - 1), so every character gets at least one step.  The recurrence runs in fp64: over a few thousand
 *     steps Q reaches ~4e4, where an fp32 ulp (4e-3) is the size of real decision margins.
 *     Infeasible utterance (S_b < N_b: fewer steps than characters): its positions are those of mode 0.
 *   N_b == 0 or S_b == 0: dur[b] and stats[b] are zero.
 *   stats[b][0..3], each accumulated in double and stored as float:
 *     [0] focus rate = mean_s max_{n < N_b} align[b][s][n]        [1] mean_s la[s][pos[s]]
 *     [2] feasible = (S_b >= N_b) ? 1 : 0 (either mode)           [3] share of the steps with pos[s] == the argmax position (mode 0: 1)
 *   Nothing at n >= N_b or s >= S_b is read.  back: mode 1 workspace of B*S*L bytes (bit 0 = predecessor is n-1, bit 1 = the
 *   step's argmax), rewritten by every call; may be NULL in mode 0.
 *   L > T2_ALIGN_MAX_L (two fp64 rows of Q in LDS: 64 KB at the cap), r < 1, a mode other than 0 / 1, a NULL back in mode 1 or
 *   leading dimensions smaller than the shapes are T2_ERR_ARG before any launch. */
#define T2_ALIGN_MAX_L 4096
typedef struct {
    const float* align; int64_t ld_b, ld_s;   /* align[b*ld_b + s*ld_s + n], n contiguous */
    int B, S, L, r, mode;                     /* r >= 1 frames per step; mode 0 = argmax, 1 = monotonic */
    const int32_t* chars_len;                 /* [B] device; N_b = clip(., 0, L) */
    const int32_t* frames_len;                /* [B] device; F_b = clip(., 0, r*S); S_b = ceil(F_b / r) */
    int32_t* dur; int64_t ld_dur;             /* [B][ld_dur >= L]: frames per character, 0 for n >= N_b */
    float* stats;                             /* [B][4] */
    uint8_t* back;                            /* mode 1 workspace [B][S][L]; may be NULL in mode 0 */
} T2AlignDur;
int t2_align_durations(const T2AlignDur* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-character pitch and energy on the grid of t2_align_durations (no reference counterpart; the two further targets FastSpeech 2
 * and FastPitch train on, csrc/t2_variance.hip, DESIGN 5.15, restated in float64 in tests/variance_ref.py): a pitch track and a
 * log-mel are cut at the character boundaries and averaged, and the sums a normalisation needs are collected.  ONE launch, one
 * 256-thread workgroup per utterance; no cross-workgroup synchronisation, no global atomics; every sum is taken in a fixed order,
 * so two calls are bit-identical.
 *   Inputs: f0[b*ld_f0 + t] in Hz (t2_yin's track or t2_pitch_viterbi's: frame t centred on sample hop*t, as the mel frame is);
 *   the log-mel mel[b*ld_b + t*ld_t + m], M bins, m contiguous (the natural log of a magnitude); dur[b*ld_dur + n] int32.
 *   N_b = clip(chars_len[b], 0, L) characters, F_b = clip(frames_len[b], 0, T) frames.
 *   Frame t is VOICED iff t < F_b and f0 > 0 (a NaN is unvoiced); p(t) = log((double)f0) with log_pitch, else (double)f0.
 *   Energy e(t) = sqrt(sum_m exp(2.0 * (double)mel[t][m])): the L2 norm of the mel magnitudes, in fp64.
 *   Filled pitch q(t), t < F_b.  interpolate = 0: q = p on the voiced frames, 0 elsewhere.  interpolate = 1, with u0 / u1 the first /
 *     last voiced frame: q(t) = p(u0) before u0 and p(u1) behind u1; between neighbouring voiced frames a < t < c
 *       q(t) = p(a) + (p(c) - p(a)) * ((double)(t - a) / (double)(c - a));   q = 0 everywhere without a voiced frame.
 *   Character n < N_b covers the frames [s_n, s_n + max(dur[n], 0)), s_n the prefix sum (int64), clipped to F_b;
 *     consistent = (sum_{n < N_b} max(dur[n], 0) == F_b).
 *   char_pitch [B][L]: interpolate = 0: the mean of p over the VOICED frames of the span, 0 without one (FastPitch's rule);
 *     interpolate = 1: the mean of q over ALL frames of the span, 0 for an empty span (FastSpeech 2's rule).
 *   char_energy [B][L]: the mean of e over the span, 0 for an empty span.  char_voiced [B][L] int32: the span's voiced frames.
 *   Entries n >= N_b of the three are written as 0.  frame_pitch / frame_energy [B][T] (either may be NULL): q and e as float;
 *   entries t >= F_b are not written.
 *   stats [B][T2_VAR_NSTAT] doubles: [0] F_b  [1] voiced frames  [2] sum p, [3] sum p^2 over the voiced frames  [4] sum q, [5] sum q^2,
 *     [6] sum e, [7] sum e^2 over all frames  [8] consistent  [9] the characters n < N_b without a voiced frame.
 *   Every mean and sum is fp64 (the tolerance of the tests then follows from the formats, not from a measurement); a character's
 *   sums run in frame order.  N_b == 0 or F_b == 0: the three character rows are 0, the frame outputs are 0 for t < F_b, the stats
 *   are 0 except [8], and nothing of f0 or mel is read.  Nothing at t >= F_b is ever read, nor dur at n >= N_b.
 *   q and e stay in LDS as doubles with the span starts: 16 T + 4 (L + 1) bytes = 80 KB at both caps (plus 4.8 KB of partials).
 *   T2_ERR_ARG before any launch: a null pointer (the two frame outputs excepted), B, T, L or M < 1, T > T2_VAR_MAX_T,
 *   L > T2_VAR_MAX_L, a flag other than 0 / 1, ld_f0 < T, ld_dur < L, ld_t < M, ld_b < (T-1)*ld_t + M. */
#define T2_VAR_MAX_T 4096
#define T2_VAR_MAX_L 4096
#define T2_VAR_NSTAT 10
typedef struct {
    const float* f0; int64_t ld_f0;           /* f0[b*ld_f0 + t], Hz; not > 0 = unvoiced */
    const float* mel; int64_t ld_b, ld_t;     /* mel[b*ld_b + t*ld_t + m], m contiguous */
    const int32_t* dur; int64_t ld_dur;       /* [B][ld_dur >= L]: frames per character (t2_align_durations) */
    int B, T, L, M, log_pitch, interpolate;
    const int32_t* chars_len;                 /* [B] device; N_b = clip(., 0, L) */
    const int32_t* frames_len;                /* [B] device; F_b = clip(., 0, T) */
    float* char_pitch;                        /* [B][L] */
    float* char_energy;                       /* [B][L] */
    int32_t* char_voiced;                     /* [B][L] */
    float* frame_pitch;                       /* optional [B][T]: q */
    float* frame_energy;                      /* optional [B][T]: e */
    double* stats;                            /* [B][T2_VAR_NSTAT] */
} T2CharVariance;
int t2_char_variance(const T2CharVariance* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Objective scoring of a free-running decode against the recording: mel-cepstral distortion under dynamic time warping
 * (MCD-DTW; no reference counterpart - the reference's `test` decodes the recordings and drops them).  Two entries
 * (csrc/t2_dtw.hip), the rule in DESIGN 5.9, restated in float64 in tests/mcd_dtw_ref.py.
 *
 * t2_mel_cepstra: log-mels (B, T, M) -> mel-cepstral coefficients (B, T, K), the orthonormal DCT-II without c[0]:
 *     out[b][t][k-1] = sum_m mel[b][t][m] * basis[m][k-1],  basis[m][k-1] = sqrt(2/M) cos(pi k (m + 1/2) / M),  k = 1 .. K
 *   basis [M][K] row-major is built by the HOST in float64 and rounded once to float32.  Plain fp32 FMAs in the order m = 0 .. M-1
 *   (not t2_gemm: the result does not depend on any matmul-precision setting).  Rows t >= clip(len[b], 0, T) are neither read nor
 *   written.  mel[b*ld_b + t*ld_t + m] and out[b*ld_ob + t*ld_ot + k], last dimension contiguous.
 *   T2_ERR_ARG before any launch: a null pointer, B, T, M < 1, M > T2_CEPS_MAX_M, K outside 1 .. T2_DTW_MAX_K, overlapping strides
 *   (ld_t < M, ld_b < (T-1)*ld_t + M, ld_ot < K, ld_ob < (T-1)*ld_ot + K).
 *
 * t2_dtw: for every pair b, the cheapest warping path between a[b] (la = clip(len_a[b], 0, Ta) rows of K features) and b[b]
 * (lb rows) under the frame distance d(i, j) = scale * sqrtf(sum_k (a[i][k] - b[j][k])^2), formed in fp32 on the fly (no Ta x Tb
 * distance matrix in memory):
 *     D[0][0] = d(0,0);   D[i][j] = d(i,j) + min(D[i-1][j-1], D[i-1][j], D[i][j-1])   (predecessors outside the matrix excluded)
 *   ties: the diagonal first, then (i-1, j), then (i, j-1) - a later candidate wins only when STRICTLY smaller.  D and the minimum
 *   are fp64: totals reach ~1e5 over a few thousand cells, where an fp32 ulp is the size of real decision margins.
 *   cost[b] = D[la-1][lb-1]; path_len[b] = the number of cells of that path (max(la, lb) .. la + lb - 1), carried through the
 *   recurrence beside D (length of the chosen predecessor + 1), so the score needs no workspace.  la == 0 or lb == 0: cost 0,
 *   path_len 0, nothing of the pair's rows is read.  scale = 10 sqrt(2) / ln 10 on cepstra gives the MCD distance in dB.
 *   back: optional workspace [B][Ta][Tb] bytes (0 diagonal, 1 = (i-1, j), 2 = (i, j-1)); with it, path [B][Ta+Tb-1][2] int32
 *   receives the cells (i, j) in FORWARD order, path_len[b] of them (the rest of the row is not written).
 *   One 256-thread workgroup per pair walks the anti-diagonals i + j = k (each depends on k-1 and k-2 only), one barrier per
 *   diagonal; three rotating rows of fp64 D and of int32 lengths, indexed by i, in dynamic LDS: 3 * Ta * (8 + 4) bytes =
 *   147 456 at Ta = T2_DTW_MAX_T = 4096, inside the 160 KB (163 840) a workgroup may take.  No cross-workgroup synchronisation,
 *   no global atomics.
 *   T2_ERR_ARG before any launch: a null pointer, B, Ta, Tb < 1, Ta or Tb above T2_DTW_MAX_T, K outside 1 .. T2_DTW_MAX_K, a path
 *   without back, overlapping strides (ld_at < K, ld_ab < (Ta-1)*ld_at + K, the same for b), a scale that is not finite. */
#define T2_DTW_MAX_T 4096
#define T2_DTW_MAX_K 32
#define T2_CEPS_MAX_M 1024
typedef struct {
    const float* mel; int64_t ld_b, ld_t;     /* mel[b*ld_b + t*ld_t + m], m contiguous */
    int B, T, M, K;
    const int32_t* len;                       /* [B] device; rows t < clip(., 0, T) are transformed */
    const float* basis;                       /* [M][K] device */
    float* out; int64_t ld_ob, ld_ot;         /* out[b*ld_ob + t*ld_ot + k] */
} T2MelCeps;
int t2_mel_cepstra(const T2MelCeps* a, void* stream);
typedef struct {
    const float* a; int64_t ld_ab, ld_at;     /* a[b*ld_ab + i*ld_at + k], k contiguous */
    const float* b; int64_t ld_bb, ld_bt;     /* b[b*ld_bb + j*ld_bt + k] */
    int B, Ta, Tb, K;
    const int32_t* len_a; const int32_t* len_b;   /* [B] device each */
    float scale;
    double* cost;                             /* [B] */
    int32_t* path_len;                        /* [B] */
    uint8_t* back;                            /* optional workspace [B][Ta][Tb] */
    int32_t* path;                            /* optional [B][Ta+Tb-1][2]; needs back */
} T2Dtw;
int t2_dtw(const T2Dtw* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prosody measurement of synthesised audio (no reference counterpart in this repository - the reference extracts its features with
 * Praat; csrc/t2_prosody.hip, the rule in DESIGN 5.10, restated in float64 in tests/prosody_ref.py).
 *
 * t2_yin: the YIN pitch tracker (de Cheveigne & Kawahara 2002, steps 2 to 5) on the mel grid.  wav[b*ld_wav + i] is a padded batch
 *   of signals, n [B] their sample counts (DEVICE array, int64, as t2_logmel_batch_fwd takes it; clipped to 0 .. n_max).
 *   T = 1 + n_max / hop frames per utterance; frame t analyses the S = W + tau_max samples [s0, s0 + S), s0 = t*hop - S/2.  A frame
 *   is VALID iff s0 >= 0 and s0 + S <= n[b]; an invalid frame reads nothing and gets f0 = 0, aper = 1, power = 0 (cmnd: all 1).
 *   Nothing at or behind n[b] is ever read.  With x the span of a valid frame:
 *     d(tau)  = sum_{j<W} (x[j] - x[j+tau])^2, tau = 1 .. tau_max;  cm(0) = 1, cm(tau) = d(tau) * tau / sum_{k<=tau} d(k), 1 where
 *               that sum is not positive;  power = sum_{j<W} x[j]^2 / W;
 *     pick    = the smallest c in [tau_min, tau_max) with cm(c) < thr, walked down while c + 1 < tau_max and cm(c+1) < cm(c); without
 *               one, the first argmin of cm over [tau_min, tau_max);  aper = cm(pick);
 *     voiced iff aper < vthr and power > power_floor; then off = 0.5 (cm(pick-1) - cm(pick+1)) / (cm(pick-1) - 2 cm(pick) + cm(pick+1)),
 *               0 when that denominator is not positive, clamped to [-1, 1], and f0 = sr / (pick + off) Hz; f0 = 0 otherwise.
 *   Outputs f0, aper, power [B][T]; cmnd [B][T][tau_max + 1] is optional (NULL: not written).
 *   One 256-thread workgroup per (frame, utterance); the span and four rows of partial d (one per wave) in dynamic LDS,
 *   (S + 4 (tau_max + 1)) floats - at most 5 * T2_YIN_MAX_SPAN * 4 = 81 920 bytes.  fp32 throughout, no atomics, every sum in a fixed
 *   order: two calls give bit-identical outputs.
 *   T2_ERR_ARG before any launch: a null pointer (cmnd excepted), B < 1 or > 65535, n_max < 0, hop < 1, sr < 1, W < 16, tau_min < 2,
 *   tau_max <= tau_min + 1, S > T2_YIN_MAX_SPAN, ld_wav < n_max.
 *
 * t2_prosody_stats: one row of T2_PROSODY_NSTAT floats per utterance from t2_yin's [B][T] outputs.  Frame t of utterance b is valid
 *   under the same rule (n, hop, S); voiced = valid and f0 > 0.  out[b] = { valid frames, voiced frames, mean logf(f0), p5_hz, p95_hz,
 *   mean 10 log10(power), mean aper, 0 }, the means and percentiles over the voiced frames: with v the voiced f0 sorted ascending and
 *   n_v their count, p5_hz = v[(5 (n_v - 1) + 50) / 100] and p95_hz = v[(95 (n_v - 1) + 50) / 100] (integer division) - elements of
 *   the track, found by rank counting in LDS (rank by (value, frame index): exact, ties included).  Means in fp64, fixed order.
 *   Without a voiced frame fields 2 .. 6 are NaN.  One 256-thread workgroup per utterance.
 *   T2_ERR_ARG before any launch: a null pointer, B < 1 or > 65535, T < 1 or > T2_PROSODY_MAX_T, hop < 1, S < 1. */
#define T2_YIN_MAX_SPAN 4096
#define T2_PROSODY_NSTAT 8
#define T2_PROSODY_MAX_T 4096
typedef struct {
    const float* wav; int64_t ld_wav;         /* wav[b*ld_wav + i] */
    const int64_t* n;                         /* [B] device */
    int B; int64_t n_max;
    int sr, hop, W, tau_min, tau_max;
    float thr, vthr, power_floor;
    float* f0; float* aper; float* power;     /* [B][T], T = 1 + n_max / hop */
    float* cmnd;                              /* optional [B][T][tau_max + 1] */
} T2Yin;
int t2_yin(const T2Yin* a, void* stream);
typedef struct {
    const float* f0; const float* aper; const float* power;      /* [B][T] */
    const int64_t* n;                         /* [B] device */
    int B, T, hop, S;                         /* S = W + tau_max of the t2_yin call */
    float* out;                               /* [B][T2_PROSODY_NSTAT] */
} T2ProsodyStats;
int t2_prosody_stats(const T2ProsodyStats* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Voice quality of a corpus or a synthesis (no reference counterpart - the reference extracts jitter, shimmer and nhr with Praat;
 * csrc/t2_prosody.hip, the rule in DESIGN 5.12, restated in float64 in tests/voice_quality_ref.py).
 *
 * t2_voice_quality: per-frame cycle matching on the mel grid.  wav / ld_wav / n / n_max and the framing are t2_yin's: S = W + tau_max,
 *   frame t spans [s0, s0 + S) with s0 = t*hop - S/2 and is VALID iff s0 >= 0 and s0 + S <= n[b] (n clipped to 0 .. n_max), T = 1 +
 *   n_max / hop.  f0 [B][T] is a pitch track in Hz - t2_yin's or t2_pitch_viterbi's - with 0 (or anything not > 0) = unvoiced.
 *   For a valid frame with f0 > 0, x its span:
 *     L = lrintf(sr / f0) (fp32 quotient, clamped to [tau_min, tau_max - 1]);  d = max(2, (L + 7) / 8);
 *     K = min((S - 2 L - d) / L + 1, T2_VQ_MAX_CYCLES) (integer division);  the frame is MEASURED iff K >= 3.
 *   Cycle i = 0 .. K-1 has its anchor at c = i L:  a = x[c .. c+L),  b_tau = x[c+tau .. c+tau+L) for tau = L-d .. L+d,
 *     ncc(tau) = sum a b_tau / sqrt(sum a^2 * sum b_tau^2), 0 when that product is not positive;  tau* = the FIRST argmax;
 *     off = 0.5 (ncc(tau*-1) - ncc(tau*+1)) / (ncc(tau*-1) - 2 ncc(tau*) + ncc(tau*+1)) clamped to [-1, 1], 0 when tau* is L-d or L+d
 *     or that denominator is not negative;  T_i = tau* + off,  r_i = ncc(tau*),  A_i = sqrt(sum a^2 / L).
 *   Per frame, sums over i ascending:  jitter = mean_{i<K-1} |T_{i+1} - T_i| / mean_i T_i;  shimmer the same over A, 0 when mean A is
 *     0;  r = mean r_i clamped to [1e-3, 1 - 1e-6];  nhr = (1 - r) / r;  hnr_db = 10 log10(r / (1 - r)) (Boersma's harmonicity).
 *   Outputs [B][T]: jitter, shimmer, nhr, hnr_db and cycles (int32, K of a measured frame).  Every other frame - invalid, unvoiced,
 *   K < 3 - gets exactly 0, 0, 0, 0, 0 and nothing of its signal is read (of an invalid frame not f0 either).  Nothing at or behind
 *   n[b] is ever read.  cyc [B][T][T2_VQ_MAX_CYCLES][3] is optional (NULL: not written): T_i, r_i, A_i in the rows i < K and ZEROS in
 *   the rows behind, all zeros for a frame that is not measured - every element is written.
 *   One 256-thread workgroup per (frame, utterance).  Dynamic LDS: the span and two tables of S/2 + 160 floats ((cycle, tau) products
 *   and window energies; K (2 d + 1) <= 7 S / 16 for L >= 16 and <= 160 below), at most (2 S + 320) * 4 = 34 048 bytes.  One thread per
 *   (cycle, tau) pair sums its product left to right; the K + 1 window energies sum x[i L .. i L + L)^2 are summed left to right by
 *   one thread each (the energy of b_L of cycle i IS that of a of cycle i + 1) and sum b_tau^2 runs from tau = L outwards, one sample
 *   dropped and one added per step - never recomputed per tau.  fp32 throughout, no atomics, every sum in a fixed order: two calls
 *   give bit-identical outputs.
 *   T2_ERR_ARG before any launch: what t2_yin rejects (thr, vthr, power_floor and its outputs do not exist here), a null f0 or output
 *   (cyc excepted).
 *
 * t2_corpus_stats: one row of T2_CORPUS_NSTAT floats per utterance from the [B][T] arrays of t2_yin (f0 or t2_pitch_viterbi's, power)
 *   and t2_voice_quality.  Frame t is valid under the same rule (n, hop, S); voiced = valid and f0 > 0; measured = valid and cycles >
 *   0; loud = valid and power > power_floor.  out[b] = { valid, voiced, measured, loud frames, mean f0 (Hz) over the voiced frames,
 *   mean jitter, shimmer, nhr, hnr_db over the measured frames, mean 10 log10(power) over the loud frames, 0, 0 }.  A mean over an
 *   empty set is 0 (its count says so).  Invalid frames are not read.  fp64 accumulation in a fixed order, one 256-thread workgroup
 *   per utterance, one launch.
 *   T2_ERR_ARG before any launch: a null pointer, B < 1 or > 65535, T < 1, hop < 1, S < 1, a power_floor that is NaN. */
#define T2_VQ_MAX_CYCLES 32
#define T2_CORPUS_NSTAT 12
typedef struct {
    const float* wav; int64_t ld_wav;         /* wav[b*ld_wav + i] */
    const int64_t* n;                         /* [B] device */
    int B; int64_t n_max;
    int sr, hop, W, tau_min, tau_max;
    const float* f0;                          /* [B][T], T = 1 + n_max / hop */
    float* jitter; float* shimmer; float* nhr; float* hnr_db; int32_t* cycles;     /* [B][T] */
    float* cyc;                               /* optional [B][T][T2_VQ_MAX_CYCLES][3] */
} T2VoiceQuality;
int t2_voice_quality(const T2VoiceQuality* a, void* stream);
typedef struct {
    const float* f0; const float* power;      /* [B][T] */
    const float* jitter; const float* shimmer; const float* nhr; const float* hnr_db; const int32_t* cycles;     /* [B][T] */
    const int64_t* n;                         /* [B] device */
    int B, T, hop, S;                         /* S = W + tau_max of the t2_yin call */
    float power_floor;
    float* out;                               /* [B][T2_CORPUS_NSTAT] */
} T2CorpusStats;
int t2_corpus_stats(const T2CorpusStats* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Smoothed pitch and F0 metrics along a warping path (no reference counterpart; csrc/t2_pitch.hip, the rules in DESIGN 5.11,
 * restated in float64 in tests/pitch_ref.py).
 *
 * t2_pitch_viterbi: the cheapest state sequence through t2_yin's normalised difference function, one per utterance - the decoding
 *   toolkits run on the host (pYIN's second stage), with one candidate per integer lag.  cmnd[b*ld_b + t*ld_t + tau], tau = 0 ..
 *   tau_max, float32, and power [B][T] are t2_yin's outputs.  States: the N = tau_max - tau_min lags tau_min .. tau_max-1 in this
 *   order (state k = lag tau_min + k), then one unvoiced state U (index N).  len[b] (DEVICE int32, clipped to 0 .. T) frames are
 *   decoded; frames behind it get f0 = 0, aper = 1, lag = 0 and nothing of them is read.  All accumulation in fp64, additions only:
 *     local(t, k) = (double) cmnd[b][t][tau_min + k] if power[b][t] > power_floor, else +inf;   local(t, U) = u;
 *     trans(k', k) = fabs(lw[k] - lw[k']), allowed iff <= trans_max;  voiced -> U and U -> voiced cost c_sw;  U -> U costs 0;
 *     D_0[s] = local(0, s);   D_t[s] = (D_{t-1}[s'] + trans) + local(t, s), the additions in exactly this association.
 *   lw [N] fp64 (DEVICE) is built by the HOST: lw[k] = w * log2(tau_min + k) with w >= 0, so it does not decrease and the allowed
 *   predecessors of a target are ONE run of states around it; the kernel takes that run (it walks from the target outwards until
 *   the first transition above trans_max), which for a table that does not decrease is the rule above.
 *   ties: a voiced target takes its voiced predecessors in ascending lag, then U - a later candidate wins only when STRICTLY
 *   smaller; target U takes U first, then the voiced predecessors ascending, under the same rule; termination takes the first
 *   minimum over the voiced states ascending, then U.
 *   Outputs [B][T]: lag = the lag of the chosen state, 0 for U;  aper = cmnd[t][lag] for a voiced frame, 1 for U;  f0 = t2_yin's own
 *   parabolic formula on cmnd[t][lag-1 .. lag+1] in fp32 (off clamped to [-1, 1], 0 when the denominator is not positive; f0 =
 *   sr / (lag + off)), 0 for U.  cost [B] fp64 = the minimum, 0 for len[b] == 0.  back: workspace uint16 [B][T][N+1], the chosen
 *   predecessor state of every (frame >= 1, state).
 *   One 256-thread workgroup per utterance, one barrier per frame; in dynamic LDS two rotating fp64 rows of D [N+1] and the lw
 *   table [N]: (3 N + 2) * 8 bytes = 98 320 at N = T2_PITCH_MAX_STATES = 4096, inside the 160 KB (163 840) a workgroup may take.
 *   The runs do not depend on t and are found once per launch (registers of the thread that owns the target).  Target U's minimum
 *   over the voiced predecessors of frame t is reduced as frame t-1 writes them (wave minima by shuffles, left beside D in front of
 *   that frame's barrier).  No cross-workgroup synchronisation, no atomics; two calls give bit-identical outputs.
 *   T2_ERR_ARG before any launch: a null pointer, B < 1 or > 65535, T < 1 or > T2_PROSODY_MAX_T, sr < 1, tau_min < 2, tau_max <=
 *   tau_min + 1, N > T2_PITCH_MAX_STATES, overlapping strides (ld_t < tau_max + 1, ld_b < (T-1)*ld_t + tau_max + 1), a trans_max, u or
 *   c_sw that is not finite or is negative, a power_floor that is NaN.
 *
 * t2_f0_path_stats: two pitch tracks compared along t2_dtw's path.  path [B][P][2] int32 holds path_len[b] (clipped to 0 .. P) cells
 *   (i, j); f0_a [B][Ta] and f0_b [B][Tb] are in Hz, 0 = unvoiced; n_a, n_b [B] (DEVICE int64) the sample counts.  Frame t of a
 *   track is valid under t2_prosody_stats' rule (t*hop - S/2 >= 0 and t*hop - S/2 + S <= n) and only inside the track (0 <= t <
 *   Ta resp. Tb); a cell is scored only when both of its frames are valid, and the tracks are read at valid frames only.
 *   out[b] = T2_F0_NSTAT doubles: { scored cells, cells with both frames voiced, only a voiced, only b voiced, sum d, sum d^2 with
 *   d = 1200 (log2 fa - log2 fb) over the both-voiced cells, then over the same cells sum la, sum lb, sum la^2, sum lb^2, sum la*lb
 *   with la = log2 fa, lb = log2 fb (what a Pearson correlation needs), 0 }.  fp64 throughout, every sum in a fixed order.
 *   path_len[b] == 0: a row of zeros, nothing is read.  One 256-thread workgroup per pair.
 *   T2_ERR_ARG before any launch: a null pointer, B < 1 or > 65535, P, Ta, Tb < 1, hop < 1, S < 1. */
#define T2_PITCH_MAX_STATES 4096
#define T2_F0_NSTAT 12
typedef struct {
    const float* cmnd; int64_t ld_b, ld_t;    /* cmnd[b*ld_b + t*ld_t + tau], tau = 0 .. tau_max contiguous */
    const float* power;                       /* [B][T] */
    const int32_t* len;                       /* [B] device; clipped to 0 .. T */
    const double* lw;                         /* [N] device, N = tau_max - tau_min */
    int B, T, sr, tau_min, tau_max;
    float power_floor;
    double trans_max, u, c_sw;
    float* f0; float* aper; int32_t* lag;     /* [B][T] */
    double* cost;                             /* [B] */
    uint16_t* back;                           /* workspace [B][T][N+1] */
} T2PitchViterbi;
int t2_pitch_viterbi(const T2PitchViterbi* a, void* stream);
typedef struct {
    const int32_t* path;                      /* [B][P][2] */
    const int32_t* path_len;                  /* [B] device; clipped to 0 .. P */
    const float* f0_a; const float* f0_b;     /* [B][Ta], [B][Tb] */
    const int64_t* n_a; const int64_t* n_b;   /* [B] device each */
    int B, P, Ta, Tb, hop, S;
    double* out;                              /* [B][T2_F0_NSTAT] */
} T2F0PathStats;
int t2_f0_path_stats(const T2F0PathStats* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sample-rate conversion (the reference resamples offline with librosa and pydub, preprocessing/hifi_tts.py:73-78, and its dataset
 * discards the header's rate, datasets/tts_dataset.py:191; csrc/t2_resample.hip, the rule in DESIGN 5.14, restated in float64 in
 * tests/resample_ref.py).
 *
 * t2_resample: a batched polyphase FIR for the rational ratio U / D in fp32.  x[b*ldx + i] is a padded batch of signals, n_in [B] their
 *   sample counts (DEVICE array, int64; negative counts as 0).  Row b has n_out[b] = ceil(n_in[b] * U / D) outputs, computed on the
 *   device and clipped to n_out_max, the caller's bound.  table [U][2K] fp32 holds the filter by phase: column c of row p is tap
 *   k = c - K + 1, k = -K+1 .. K.  For m < n_out[b], with m * D formed in 64 bits:
 *     i0 = floor(m * D / U),  p = (m * D) mod U,  y[b*ldy + m] = sum_{k = -K+1 .. K} table[p][k + K - 1] * x[b*ldx + i0 + k],
 *   one fmaf per tap in ascending k.  A sample outside [0, n_in[b]) counts as zero and is never loaded; for n_out[b] <= m < ldy the
 *   kernel writes 0.0f (t2_logmel_batch_fwd wants rows zero-filled behind their utterance).  Nothing behind ldy is written.
 *   One 256-thread workgroup per 1024 consecutive outputs of one row, their input span, at most 1023 D / U + 2K + 2 floats, staged once
 *   in dynamic LDS (up to 64 KB; a longer span is read from global memory, the same sum), the table read from global memory.  No
 *   atomics, a fixed order: two calls give bit-identical outputs, and a row's outputs do not depend on B, ldx, ldy or the other rows.
 *   T2_ERR_ARG before any launch: a null pointer, B < 1 or > 65535, U, D or K < 1, U * 2K > 2^20, n_out_max < 0, ldy < n_out_max. */
typedef struct {
    const float* x; int64_t ldx; const int64_t* n_in;   /* [B] device; rows are read only in [0, n_in[b]) */
    float* y; int64_t ldy; int64_t n_out_max;           /* y[b][m] for m < ldy */
    const float* table; int U, D, K;                    /* [U][2K] fp32, tap k = -K+1 .. K of phase p */
    int B;
} T2Resample;
int t2_resample(const T2Resample* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Joining synthesised pieces into one waveform (no reference counterpart: its `say` speaks one text; csrc/t2_join.hip, the rule in
 * DESIGN 5.16, restated in numpy in tests/join_ref.py).
 *
 * t2_join: x[b*ldx + i] float32 is a padded batch of B waveforms, n[b] (DEVICE int32, 0 <= n[b] <= n_max <= ldx) their sample
 *   counts, pause[b] (DEVICE int32, >= 0) the samples of silence behind piece b.  Nothing is read from a row at or behind n[b].
 *   SPAN of row b - the rule of trim_silence (datasets/tts_dataset.py), the ruler the corpus was trimmed on.  With trim = 0 or n[b] < F
 *   it is [0, n[b]).  Otherwise frame f = 0 .. n[b] / H is centred on sample f H (zero padded, F even):
 *     e_f = the fp64 sum of x[i]^2 over [f H - F/2, f H + F/2) within [0, n[b]);   e_max = max_f e_f;
 *     frame f is active iff e_f > e_max * 10^(-top_db / 10)  (the factor is formed once, by the host, in fp64);
 *     with the first and last active frames f0, f1:  s0 = max(0, f0 H - keep),  s1 = min(n[b], (f1 + 1) H + keep).
 *   A row without an active frame - e_max == 0, or top_db == 0 - has the EMPTY span s0 = s1 = 0 and contributes its pause alone.
 *   (trim_silence floors both levels at 1e-10 and so keeps an all-zero signal whole; a synthesised piece of silence is dropped.)
 *   Over the span: sumsq_b (fp64) and peak_b = max |x|.
 *   PLAN, in fp64:  len_b = s1 - s0,  rms_b = sqrt(sumsq_b / len_b).  gain_b = 1 with level = 0; with level = 1
 *     rms_doc = sqrt(sum_b sumsq_b / sum_b len_b),  gain_b = clamp(rms_doc / rms_b, 1 / max_gain, max_gain),  1 where len_b == 0 or
 *     rms_b == 0.  If ceiling > 0 and pk = max_b gain_b peak_b > ceiling, every gain is multiplied by ceiling / pk.  One cast to
 *     float32.  off_b = the exclusive int64 scan of len_b + pause_b, total = off_B.  Written: off, s0, len, gain [B] each, total [1].
 *   WRITE, with fl_b = min(fade, len_b / 2) (integer division), for i < len_b:
 *     y[off_b + i] = x[b*ldx + s0 + i] * (gain_b * e)   - two float32 multiplications in this order, nothing fused -
 *     e = w_b(i) for i < fl_b,  w_b(len_b - 1 - i) for i >= len_b - fl_b,  1.0f elsewhere;   w_b(i) = w[(2 i + 1) fade / (2 fl_b)]
 *     in integer arithmetic, so that a shortened fade samples the same table;  y[off_b + len_b + j] = 0.0f for j < pause_b.
 *   w [fade] float32 is built by the HOST: w[k] = float32(0.5 - 0.5 cos(pi (k + 0.5) / fade)) formed in fp64; fade = 0: no table,
 *   no fades.  y holds cap floats, the caller's bound sum n + sum pause; nothing at or behind total is written.
 *   REFUSED on the device, not clamped: an n[b] outside 0 .. n_max, a negative pause[b] or total > cap give total = -1 and all
 *   off = 0; such rows are never read and nothing is written to y.
 *   Workspaces: energy [B][lde] fp64 with lde >= n_max / H + 1 (may be NULL with trim = 0), stat [B][2] fp64 (sumsq, peak).
 *   Four launches on one stream: frame energies (one wave per frame, grid frames / 4 x B), spans and sums (one 1024-thread
 *   workgroup per row), the plan (one workgroup), the write (grid chunks x B).  No cross-workgroup synchronisation, no atomics,
 *   every sum in a fixed order: two calls give bit-identical outputs, and a row's span does not depend on B, ldx or the other rows.
 *   T2_ERR_ARG before any launch: a null pointer (x only when n_max > 0, w only when fade > 0, y only when cap > 0, energy only
 *   when trim = 1), B < 1 or > 65535, F < 2 or odd, H < 1, keep < 0, fade < 0, top_db not finite or < 0, max_gain not finite or
 *   < 1, ceiling not finite or < 0, n_max < 0, ldx < n_max, lde < n_max / H + 1 with trim = 1, cap < 0, a trim or level other than
 *   0 / 1. */
typedef struct {
    const float* x; int64_t ldx;                        /* rows are read only inside [0, n[b]) */
    const int32_t* n; const int32_t* pause;             /* [B] device each */
    const float* w;                                     /* [fade] fp32, host-made; NULL with fade = 0 */
    int B, n_max, trim, F, H, keep, fade, level;
    double top_db, max_gain, ceiling;
    double* energy; int64_t lde;                        /* workspace [B][lde] */
    double* stat;                                       /* workspace [B][2] */
    int64_t* off; int32_t* s0; int32_t* len; float* gain;   /* the plan, [B] each */
    int64_t* total;                                     /* [1]; -1: refused */
    float* y; int64_t cap;
} T2Join;
int t2_join(const T2Join* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Time stretching of a waveform: WSOLA (Verhelst & Roelands 1993; the rule as in Driedger & Mueller 2014; no reference counterpart;
 * csrc/t2_stretch.hip, the rule in DESIGN 5.17, restated in numpy in tests/stretch_ref.py).
 *
 * t2_stretch: x[b*ldx + i] float32 is a padded batch of B waveforms of finite samples, n[b] (DEVICE int32, 0 <= n[b] <= n_max <= ldx)
 *   their sample counts.  Nothing is read from a row at or behind n[b]; x~ is x with zeros outside [0, n[b]).  The tempo is the
 *   rational P / Q, the window N (even, 4 .. T2_STRETCH_MAX_N) with Hs = N / 2, the tolerance D (0 .. T2_STRETCH_MAX_D).  Every
 *   position is an integer formed in integer arithmetic; no float decides anything.
 *   LENGTHS  n_out = ceil(n Q / P);  frames m = 0 .. M - 1,  M = ceil(n_out / Hs) + 1;  the nominal input centre of frame m is
 *     a_m = (m Hs P + Q / 2) div Q  in int64.
 *   SEARCH SIGNAL  peak = max |x[i]| over i < n[b];  q[i] = (int) rint((double) x[i] * 1023.0 / (double) peak), an IEEE fp64
 *     division, ties to even;  q = 0 everywhere when peak == 0.  |q| <= 1023 and N <= 2048 keep every score below 2^31
 *     (1023^2 * 2048 = 2143291392): int32 sums are exact in any order.
 *   OFFSETS  delta_0 = 0,  p_m = a_m + delta_m.  For m >= 1, with c = p_{m-1} + Hs, the natural continuation of the frame before:
 *     score(d) = sum_{k = -Hs .. Hs - 1} q~[a_m + d + k] * q~[c + k]   for d in [-D, D];
 *     delta_m = the d of the largest score; ties go to the smaller |d|, then to the negative one.
 *   OVERLAP-ADD  w [N] float32 is the periodic Hann window built by the HOST: w[k] = float32(0.5 - 0.5 cos(2 pi k / N)) formed in
 *     fp64; w[k] + w[k + Hs] = 1, so nothing is normalised.  For j = m Hs + i, 0 <= i < Hs, j < n_out:
 *       y[b*ldy + j] = w[Hs + i] * x~[p_m + i] + w[i] * x~[p_{m+1} - Hs + i]   - two float32 products and one sum, nothing fused -
 *     and y[b*ldy + j] = 0.0f for n_out <= j < ldy.
 *   Written besides y: pos[b*ldp + m] = p_m (int32) for m < M and 0 for M <= m < ldp;  n_out[b] (int32).
 *   REFUSED on the device, not clamped: a row with n[b] outside 0 .. n_max gets n_out[b] = -1; nothing else is read or written for it.
 *   P == Q is NOT an identity (the correlation is not normalised); a caller that wants one launches nothing.
 *   One launch, one 1024-thread workgroup per row, three phases: the peak; the chain of frames - template (N int16) and search
 *   region (N + 2D int16) in LDS, a thread scores four adjacent offsets over a slice of the template, one workgroup-wide argmax
 *   per frame -; a parallel sweep that writes y.  No atomics and integer decisions: two calls give bit-identical outputs, and
 *   a row's outputs do not depend on B, ldx, ldy, ldp or the other rows.
 *   T2_ERR_ARG before any launch: a null pointer (x only when n_max > 0, y only when ldy > 0), B < 1 or > 65535, N outside
 *   4 .. 2048 or odd, D outside 0 .. 1024, P or Q outside 1 .. 2^20 or P / Q outside 1/8 .. 8, n_max outside 0 .. 2^27
 *   (so that n_out <= 2^30 and every position fits int32),
 *   ldx < n_max, ldy < ceil(n_max Q / P), ldp < ceil(ceil(n_max Q / P) / Hs) + 1. */
#define T2_STRETCH_MAX_N 2048
#define T2_STRETCH_MAX_D 1024
typedef struct {
    const float* x; int64_t ldx;                        /* rows are read only inside [0, n[b]) */
    const int32_t* n;                                   /* [B] device */
    const float* w;                                     /* [N] fp32, host-made periodic Hann */
    int B, n_max, N, D, P, Q;
    float* y; int64_t ldy;                              /* y[b][j] for j < ldy */
    int32_t* pos; int64_t ldp;                          /* pos[b][m] = p_m */
    int32_t* n_out;                                     /* [B]; -1: refused */
} T2Stretch;
int t2_stretch(const T2Stretch* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pitch change of a waveform at its own length and with its own formants: TD-PSOLA (Moulines & Charpentier 1990; no reference
 * counterpart; csrc/t2_psola.hip, the rule in DESIGN 5.18, restated in numpy in tests/psola_ref.py).
 *
 * t2_psola: x[b*ldx + i] float32 is a padded batch of B waveforms of finite samples, n[b] (DEVICE int32, 0 <= n[b] <= n_max <= ldx)
 *   their sample counts; nothing is read from a row at or behind n[b].  lag[b*ldt + t] (int32) is the pitch period in samples at
 *   frame t, centred on sample t hop, 0 = unvoiced (t2_pitch_viterbi's lag); rho[b*ldt + t] (int32, Q16) the output period over the
 *   input period there, taken as 65536 where lag == 0.  U is the mark spacing in unvoiced stretches.  All divisions are integer
 *   divisions; no float decides anything but the comparisons of input samples in the analysis chain.
 *     Tb = min(T, 1 + n / hop),  t(s) = min((s + hop / 2) / hop, Tb - 1),  per(s) = lag[t(s)].
 *   ANALYSIS MARKS  a_0 = 0.  Given a_k: step = per(a_k), or U if that is 0;  c = a_k + step.  c >= n: a_{k+1} = n is the terminal
 *     mark, K = k + 1.  Else, with per(c) > 0: d = min(per(c), step) / 4 and a_{k+1} = the index of the largest x in
 *     [c - d, min(c + d, n - 1)], the smallest index on a tie; with per(c) == 0: a_{k+1} = c.  Marks before the terminal one are at
 *     least 12 and at most 5120 samples apart.
 *   SYNTHESIS MARKS, int64 in 1/256 sample:  s_0 = 0, r_0 = 0, k(0) = 0;  s_{j+1} = s_j + (((a_{k(j)+1} - a_{k(j)}) * rho[t(r_j)]) >> 8);
 *     r_{j+1} = (s_{j+1} + 128) >> 8.  r_{j+1} >= n: the terminal r_J = n with k(J) = K.  Else k(j+1) = the mark among 0 .. K - 1
 *     nearest to r_{j+1}, the smaller k on a tie.  With rho == 65536 throughout, r == a.
 *   OVERLAP-ADD  w [1025] float32 is built by the HOST: w[u] = float32(0.5 - 0.5 cos(pi u / 1024)) formed in fp64.  Grain j = 0 .. J
 *     copies the analysis grain k = k(j): at output sample i, e = i - r_j, it reads x[a_k + e] with weight 1 at e = 0,
 *     w[((L + e) * 1024) / L] for -L < e < 0 with L = a_k - a_{k-1} (nothing for k = 0), w[1024 - (e * 1024) / R] for 0 < e < R with
 *     R = a_{k+1} - a_k (nothing for k = K).  For i < n, over the grains that reach i in ascending j:
 *       y[b*ldy + i] = (sum_j w_j * x[..]) / max(sum_j w_j, 1)   - float32 products and sums, nothing fused, one IEEE division -
 *     and y[b*ldy + i] = 0.0f for n <= i < ldy.
 *   Written besides y: a[b*ldm + k] = a_k for k <= K and 0 behind up to ldm;  r[b*lds + j] = r_j and kmap[b*lds + j] = k(j) for
 *     j <= J and 0 behind up to lds;  n_marks[b] = K + 1,  n_syn[b] = J + 1.  K + 1 <= n / 12 + 2.  A terminal spacing a_K - a_{K-1} as
 *     small as one sample makes the synthesis steps of the grains nearest to a_{K-1} as small as rho / 256 of a sample, up to 10250
 *     of them; every other step is at least 3 samples: J + 1 <= n / 3 + T2_PSOLA_SYN_TAIL.
 *   REFUSED on the device, not clamped: n[b] outside 0 .. n_max; among the frames t < Tb a lag outside {0} and T2_PSOLA_MIN_LAG ..
 *     T2_PSOLA_MAX_LAG, or at a voiced frame a rho outside T2_PSOLA_MIN_RHO .. T2_PSOLA_MAX_RHO (1/4 .. 4).  Such a row gets
 *     n_marks[b] = -1; nothing else is written for it, and x is not read.
 *   One launch, one 1024-thread workgroup per row: the check; the analysis chain by one wave on pieces of the signal in LDS; the
 *   synthesis chain by one thread; a sweep in which every thread gathers its samples' grains.  No atomics: two calls give
 *   bit-identical outputs, and a row's outputs do not depend on B, the leading dimensions or the other rows.
 *   T2_ERR_ARG before any launch: a null pointer (x only when n_max > 0, y only when ldy > 0), B < 1 or > 65535, n_max outside
 *   0 .. 2^27, ldx < n_max, T < 1, ldt < T, hop outside 16 .. 2^20, U outside 16 .. 4096, ldy < n_max, ldm < n_max / 12 + 2,
 *   lds < n_max / 3 + T2_PSOLA_SYN_TAIL. */
#define T2_PSOLA_MIN_LAG 16
#define T2_PSOLA_MAX_LAG 4096
#define T2_PSOLA_MIN_RHO 16384
#define T2_PSOLA_MAX_RHO 262144
#define T2_PSOLA_SYN_TAIL 10256
typedef struct {
    const float* x; int64_t ldx;                        /* rows are read only inside [0, n[b]) */
    const int32_t* n;                                   /* [B] device */
    const int32_t* lag; const int32_t* rho; int64_t ldt;   /* [B][T] each, rows ldt apart */
    const float* w;                                     /* [1025] fp32, host-made raised cosine */
    int B, n_max, T, hop, U;
    float* y; int64_t ldy;                              /* y[b][i] for i < ldy */
    int32_t* a; int64_t ldm;                            /* a[b][k] = a_k */
    int32_t* r; int32_t* kmap; int64_t lds;             /* r[b][j] = r_j, kmap[b][j] = k(j) */
    int32_t* n_marks; int32_t* n_syn;                   /* [B] each; n_marks -1: refused */
} T2Psola;
int t2_psola(const T2Psola* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Programme loudness and true peak of a waveform, and its normalisation: ITU-R BS.1770-4 for one channel (K-weighting, 400 ms blocks
 * in steps of 100 ms, the absolute and the relative gate, a true peak from 4x oversampling; no reference counterpart;
 * csrc/t2_loudness.hip, the rule in DESIGN 5.20, restated in float64 in tests/loudness_ref.py).
 *
 * t2_loudness: x[b*ldx + i] float32 is a padded batch of B waveforms of finite samples, n[b] (DEVICE int32, 0 <= n[b] <= n_max <= ldx)
 *   their sample counts; nothing is read from a row at or behind n[b].
 *   K-WEIGHTING  two biquads in cascade, the shelf b1 / a1 and the high-pass b2 / a2 (a[0] = 1), formed by the HOST in fp64 for the
 *     row's sample rate (tacotron2_amd/loudness.py: k_weighting).  Each runs as  v = b[0] u + s1;  s1 = b[1] u - a[1] v + s2;
 *     s2 = b[2] u - a[2] v  in fp64 over [0, n[b]) from s1 = s2 = 0; y is the output of the second.
 *   HOP ENERGIES  with H samples per hop and N = 4 H:  E[b*lde + h] = the fp64 sum of y^2 over [h H, (h + 1) H) for every whole hop,
 *     h < n / H.
 *   BLOCKS  a row with n >= N has J = n / H - 3 blocks  z_j = (((E_j + E_{j+1}) + E_{j+2}) + E_{j+3}) / N.  A row with 0 < n < N is
 *     ONE block of all its samples, z_0 = (sum of y^2 over [0, n)) / n, and sets the flag `short`.  n == 0: J = 0.
 *   GATES, in the linear domain:  block j passes the absolute gate iff z_j > abs_gate (the host's 10^((-70 + 0.691) / 10)), and
 *     the relative one iff it also has z_j > 0.1 * mean(z over the blocks past the absolute gate).
 *     lufs = -0.691 + 10 log10(mean z over the blocks past both).  Without a block past the absolute gate the row has NO loudness:
 *     lufs = NaN, the flag `undefined`, gain 1.
 *   PEAKS  sample_peak = max |x[i]|.  true_peak = the largest magnitude among the 4 n values t2_resample writes for this row with
 *     U = 4, D = 1 and this table [4][2K]:  for m < 4 n,  i0 = m / 4, p = m % 4,
 *     sum_{k = -K+1 .. K} table[p][k + K - 1] * x[i0 + k],  one fmaf per tap in ascending k from 0.0f, samples outside [0, n) zero and
 *     never loaded.  The 4x signal is not written.
 *   GAIN, in fp64, only with y != NULL (y == NULL: the entry measures, gain = 1 and neither `limited` nor `capped` is set):
 *     g = 10^((target - lufs) / 20);  g > max_gain: g = max_gain, flag `capped`;  then g * true_peak > ceiling: g = ceiling /
 *     true_peak, flag `limited` (max_gain and ceiling LINEAR, from the host).  gain[b] = (float) g, and
 *     y[b*ldy + i] = x[b*ldx + i] * gain[b]  for i < n[b] - one float32 product -,  0.0f for n[b] <= i < ldy.
 *   stat[b*T2_LOUD_NSTAT + ..] fp64:  0 lufs,  1 gain (before the rounding to float32),  2 true_peak,  3 sample_peak,  4 n_blocks = J,
 *     5 n_below_abs,  6 n_below_rel (past the absolute gate, not past the relative one),  7 rel_gate_lufs = -0.691 + 10 log10 of the
 *     relative threshold (NaN without a loudness),  8 momentary_max_lufs = -0.691 + 10 log10(max_j z_j) (-inf for silence, NaN with
 *     J = 0),  9 flags: bit 0 short, 1 undefined, 2 limited, 3 capped.
 *   REFUSED on the device, not clamped: a row with n[b] outside 0 .. n_max gets flags = -1; nothing else is written for it (E, gain
 *     and y included) and x is not read.
 *   Launches on one stream: the filter and hop energies (one 256-thread workgroup per row: every thread filters a chunk of 32
 *     samples from a zero state, the 4 end states of the 256 chunks of a pass meet in a scan through the chunk-transition matrix and
 *     its powers - formed by the entry from a1, a2, b2 in fp64 -, and every thread filters its chunk again from its true state); the
 *     peaks (grid tiles of 1024 samples x B, the span in LDS as t2_resample stages it, the tile maxima joined by an integer maximum
 *     on the bits of the non-negative value); gates and gain (one workgroup per row over E); the scaling.  Every sum in a fixed
 *     order: two calls give bit-identical E, stat, gain and y, and a row's results do not depend on B, ldx, ldy, lde or the other rows.
 *   T2_ERR_ARG before any launch: a null pointer (x only when n_max > 0, y never: it selects measuring), B < 1 or > 65535, n_max < 0,
 *     ldx < n_max, H < 1, lde < n_max / H, K outside 1 .. T2_LOUD_MAX_K, ldy < n_max with y, a coefficient, gate, target, max_gain
 *     or ceiling that is not finite, max_gain or ceiling <= 0. */
#define T2_LOUD_NSTAT 10
#define T2_LOUD_MAX_K 4096
typedef struct {
    const float* x; int64_t ldx;                        /* rows are read only inside [0, n[b]) */
    const int32_t* n;                                   /* [B] device */
    const float* table; int K;                          /* [4][2K] fp32: datasets/resample.plan(sr, 4 sr) */
    int B, n_max, H;
    double b1[3], a1[3], b2[3], a2[3];                  /* the K-weighting at the rows' rate, host-made */
    double abs_gate, target, max_gain, ceiling;         /* linear mean square; LUFS; linear; linear */
    double* E; int64_t lde;                             /* [B][lde] hop energies */
    double* stat;                                       /* [B][T2_LOUD_NSTAT] */
    float* gain;                                        /* [B] */
    float* y; int64_t ldy;                              /* NULL: measure only */
} T2Loudness;
int t2_loudness(const T2Loudness* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Look-ahead true-peak limiter of a padded batch of waveforms (no reference counterpart; csrc/t2_limit.hip, the rule in DESIGN 5.21,
 * restated sequentially in float64 in tests/limiter_ref.py).  It holds the true peak t2_loudness measures under a ceiling with a gain
 * that moves, where t2_loudness's own bound turns the whole row down.
 *
 * t2_limit: x[b*ldx + i] float32 is a padded batch of B waveforms of finite samples v, already at their target gain, n[b] (DEVICE
 *   int32, 0 <= n[b] <= n_max) their sample counts; nothing is read from a row at or behind n[b].  ceiling c LINEAR, fp64; L the
 *   look-ahead in samples, 1 .. 2048; a the release coefficient in (0, 1), host-made in fp64 as exp(-1 / (release_s * sr)); table
 *   [4][2K] as t2_loudness takes it.  Per row:
 *   1 ENVELOPE  P[i] = max(|v[i]|, |u[4i]|, .., |u[4i+3]|), u the 4 n values t2_resample writes for this row with U = 4, D = 1 and this
 *     table, in t2_loudness's arithmetic: one fmaf per tap in ascending k from 0.0f, samples outside [0, n) zero and never loaded.
 *     env[i] = max(P[i-1], P[i]), P[-1] = 0: a value between the samples i and i + 1 is made of both, so both carry its reduction.
 *     env[b*lde + i] float32 is written for i < n[b].
 *   2 REQUIRED GAIN  r[i] = (double)env[i] > c ? (float)(c / (double)env[i]) : 1.0f - one fp64 division, rounded once.
 *   3 LOOK-AHEAD  h[i] = min r[k] over i <= k <= min(i + L, n - 1): exact.
 *   4 RELEASE, in fp64:  e[i] = min(h[i], a * e[i-1] + (1 - a)),  e[m] = h[0] for every m < 0: the limiter is already down when the
 *     row starts (with e = 1 in front of the row a peak inside the first L samples would break the bound of step 5).
 *   5 ATTACK  s[i] = (e[i-L] + .. + e[i]) / (L + 1) in fp64.  Every term is at most h of its own index, which is at most r[i], so
 *     s[i] <= r[i] up to the rounding of the sum.  A row with no env[i] > c has s == 1 exactly.  curve[b*ldc + i] = (float)s[i], i < n[b].
 *   6 APPLY  w[i] = v[i] * curve[i], one float32 product.
 *   7 TRIM  the gain now moves between samples, so the 4x values of w can pass c by a hair.  peak_after = max_i P[i] of w (step 1,
 *     the same taps).  peak_after > c:  t = the largest float32 with (double)t * peak_after <= c,  y[i] = w[i] * t;  else t = 1 and
 *     y = w bit for bit.  y[b*ldy + i] = 0.0f for n[b] <= i < ldy.
 *   stat[b*8 + ..] fp64:  0 in_peak = max env,  1 n_over = the count of env[i] > c,  2 min_gain = min s,  3 peak_after,  4 trim = t,
 *     5 flags: bit 0 active (n_over > 0), bit 1 trimmed,  6, 7: 0.
 *   REFUSED on the device, not clamped: a row with n[b] outside 0 .. n_max gets flags = -1; nothing else is written for it (env,
 *     curve and y included) and x is not read.
 *   Launches on one stream, plain: the envelope (grid tiles of 1024 samples x B, the span in LDS as t2_loudness's peak launch stages
 *     it); the curve (one 256-thread workgroup per row in passes of 4096 samples with a halo of L on both sides: the sliding minimum
 *     by doubling in LDS, the release chunked - every thread runs 16 samples from the neutral state e = 1, the chunk ends meet in a
 *     scan over d = 1 - e, d_end[t] = max(local_end[t], a^16 d_end[t-1]) - a carried d that is not zero is held where the fp64
 *     recurrence itself stops, about tau / 2 ulps under 1 -, and every thread runs its chunk again from its true state -, the box sum; the last L values of e and the release state are carried from pass to pass; a row without a sample above c
 *     gets curve = 1 and skips all of it); apply and the peak of w (the envelope's grid; the maxima joined by an integer maximum on
 *     the bits of the non-negative value); the trim.  Two calls give bit-identical env, curve, y and stat, and a row's results do not
 *     depend on B, the leading dimensions or the other rows.
 *   T2_ERR_ARG before any launch: a null pointer (x only when n_max > 0), B < 1 or > 65535, n_max < 0, ldx, lde, ldc or ldy < n_max,
 *     K outside 1 .. T2_LOUD_MAX_K, L outside 1 .. 2048, a not in (0, 1), a ceiling that is not finite or <= 0. */
enum { T2_LIMIT_NSTAT = 8, T2_LIMIT_MAX_L = 2048 };
typedef struct {
    const float* x; int64_t ldx;                        /* rows are read only inside [0, n[b]) */
    const int32_t* n;                                   /* [B] device */
    const float* table; int K;                          /* [4][2K] fp32: datasets/resample.plan(sr, 4 sr) */
    int B, n_max, L;
    double a, ceiling;                                  /* release coefficient; linear */
    float* env; int64_t lde;                            /* [B][lde] */
    float* curve; int64_t ldc;                          /* [B][ldc] */
    float* y; int64_t ldy;                              /* [B][ldy], zeros behind n[b] */
    double* stat;                                       /* [B][8] */
} T2Limit;
int t2_limit(const T2Limit* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spectral subtraction of a stationary bias spectrum - a vocoder's own buzz - from a padded batch of waveforms (the method of the
 * denoisers that ship with other Tacotron 2 / HiFi-GAN toolchains; no reference counterpart; csrc/t2_denoise.hip, the rule in DESIGN
 * 5.22, restated in float64 in tests/denoise_ref.py).
 *
 * t2_denoise: x[b*ldx + i] float32 is a padded batch of B waveforms of finite samples, n[b] (DEVICE int32, 0 <= n[b] <= n_max) their
 *   sample counts; nothing is read from a row at or behind n[b].  The geometry is fixed: N = T2_DENOISE_NFFT = 1024, hop H =
 *   T2_DENOISE_HOP = 256, win [1024] the periodic Hann window and tw [768][2] = (cos, sin) of 2 pi k / 1024, both fp32 tables made
 *   by the host in float64; bias [513] float32, strength a float >= 0.  Per row, with n = n[b]:
 *   SHORT  n <= 512 cannot be reflected: y[i] = x[i] bit for bit, no frame is formed (F = 0, gated = 0, no mag row), flag `short`.
 *   FRAMING  else the row is reflect-padded by 512 samples on both sides at its OWN length, p[j] = x[|j - 512|] in front and
 *     x[2 (n - 1) - (j - 512)] behind, and has F = 1 + n / 256 frames; frame t is p[256 t .. 256 t + 1024), that is the samples
 *     256 t - 512 .. 256 t + 511 of the row.  Every sample i < n lies under at least two frames with a positive window.
 *   PER FRAME  a[j] = p[256 t + j] * win[j];  Z = the 1024-point DFT of a;  per bin k <= 512:  m = sqrtf(fmaf(re, re, im * im)),
 *     thr = strength * bias[k] (one float32 product),  g = m > thr ? (m - thr) / m : 0,  Z[k] and Z[1024 - k] scaled by g;
 *     c = the real part of the inverse DFT / 1024;  the frame's term at j is (c[j] * win[j]).
 *     mag[(b*f_max + t)*ldm + k] = m, the magnitude BEFORE the gate, when mag is given.
 *   OVERLAP-ADD  y[i] = (the sum of the terms of the frames over i, in ASCENDING t, from 0.0f) / (the sum over the same frames, in
 *     the same order, of the float32 products win * win), i < n: the divisor is formed from the frames that exist and is not 1.5
 *     near the row's ends (its minimum: tests/denoise_ref.py).  y[b*ldy + i] = 0.0f for n[b] <= i < ldy.  bias == 0 is the
 *     identity up to the rounding of the two transforms.
 *   y == NULL is ANALYSIS mode: mag alone is written (and stat 0 and 2); there is no inverse transform and bias is not read.
 *   gated[b] int32 = the bins of the row with g == 0 (0 in analysis mode);  stat[b*4 + ..] fp64:  0 F,  1 gated,  2 flags: bit 0
 *     short,  3: 0.  gated and stat are zeroed by the entry itself in front of the launch.
 *   REFUSED on the device, not clamped: a row with n[b] outside 0 .. n_max gets flags = -1; nothing else is written for it (y and
 *     mag included; its gated and the rest of its stat keep the entry's zeros) and x is not read.
 *   ONE launch, grid (tiles of 16 hops = 4096 samples, B), 256 threads: a workgroup stages the samples its frames touch in LDS,
 *     runs the 19 frames that reach its tile one after another through a radix-4 FFT in LDS, adds them into an LDS tile and writes
 *     its samples once; the three halo frames are computed again by the neighbouring tile; a frame is counted and its mag row
 *     written by ONE workgroup, the tile that owns it.  The float sums have a fixed order and the counts are integer atomics:
 *     two calls give bit-identical y, mag, gated and stat, and a row's results do not depend on B, the leading dimensions or the
 *     other rows.
 *   T2_ERR_ARG before any launch: a null pointer (x only when n_max > 0; bias only with y; y and mag may each be NULL, not both),
 *     B < 1 or > 65535, n_max < 0, ldx < n_max, a strength that is negative or not finite, with y: ldy < n_max, with mag:
 *     ldm < 513 or f_max < 1 + n_max / 256. */
enum { T2_DENOISE_NFFT = 1024, T2_DENOISE_HOP = 256, T2_DENOISE_NSTAT = 4 };
typedef struct {
    const float* x; int64_t ldx;                        /* rows are read only inside [0, n[b]) */
    const int32_t* n;                                   /* [B] device */
    int B, n_max;
    const float* win; const float* tw;                  /* [1024]; [768][2]: host-made in float64 */
    const float* bias; float strength;                  /* [513] */
    float* y; int64_t ldy;                              /* [B][ldy], zeros behind n[b]; NULL: analysis mode */
    float* mag; int64_t ldm; int f_max;                 /* [B][f_max][ldm]; NULL: not written */
    int32_t* gated;                                     /* [B] */
    double* stat;                                       /* [B][4] */
} T2Denoise;
int t2_denoise(const T2Denoise* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Log-mel front-end (datasets/tts_dataset.py:166-168,204; definition restated from datasets/prosody_dataset.py:39-50,67):
 * wav [n] fp32 -> out [frames = 1 + n/hop][n_mels] natural-log mel.  basis [2*(n_fft/2+1)][n_fft] = window-folded
 * [cos ; -sin] DFT rows, fb [n_mels][ldm] mel filterbank rows zero-padded to ldm = round_up(n_fft/2+1, 4) (both built by the
 * host once, tacotron2_amd/datasets/logmel.py).  Workspaces: padded [n + n_fft], spec [frames][2*(n_fft/2+1)], mag [frames][ldm]. */
int t2_logmel_frames(int64_t n_samples, int hop);
int t2_logmel_fwd(const float* wav, int64_t n, const float* basis, const float* fb, float* padded, float* spec, float* mag,
                  float* out, int n_fft, int hop, int n_mels, void* stream);

/* The same front-end for ONE TRAINING BATCH in one pass - what the reference's 8 DataLoader workers + collate produce on the host
 * (run/train.py:150-158, datasets/tts_dataset.py:184-214, datasets/tts_dataloader.py:8-35): wavs [B][ld_wav] = the B decoded (trimmed,
 * silence-padded) utterances, zero-filled rows; n_dev [B] = their sample counts (DEVICE array, int64; n_max = the largest of
 * them, known to the host); every utterance's reflect-padded signal becomes one row of `padded` [B][Tp*hop], so that the analysis
 * windows of the WHOLE batch are the overlapping rows of ONE DFT GEMM (row b*Tp + f = frame f of utterance b, lda = hop; the
 * n_fft/hop - 1 rows that straddle two utterances are computed and dropped).  Outputs in the batch layout of the model:
 * mel (B, T_out, n_mels) zero behind each utterance's 1 + n_b/hop frames (T_out >= the longest: the caller may pad further, e.g. to a
 * data-parallel step's global shape), gate (B, T_out, 1) ones with the last valid frame 0 (datasets/tts_dataset.py:213-214; may be
 * NULL), mel_len [B] int32 (may be NULL).  Per frame the arithmetic is exactly t2_logmel_fwd's: results are bit-identical.
 * t2_logmel_batch_workspace: element counts of padded / spec / mag / tmp and Tp (out5[0..4]). */
int t2_logmel_batch_workspace(int B, int64_t n_max, int n_fft, int hop, int n_mels, int64_t* out5);
int t2_logmel_batch_fwd(const float* wavs, int64_t ld_wav, const int64_t* n_dev, int B, int64_t n_max, const float* basis,
                        const float* fb, float* padded, float* spec, float* mag, float* tmp, float* mel, int64_t T_out,
                        float* gate, int32_t* mel_len, int n_fft, int hop, int n_mels, void* stream);

/* dropout scale masks and the optimizer of model/tts_model.py:78-91 + Lightning gradient_clip_val=1.0 (run/train.py:240) on one
 * flat fp32 parameter buffer.
 * t2_philox_mask: Philox4x32-10, one counter per FOUR elements.  Element e = 4 i + j takes output word j of
 *   counter (i & 0xffffffff, i >> 32, stream_id & 0xffffffff, stream_id >> 32) under key (seed & 0xffffffff, seed >> 32);
 *   u = (word >> 8) * 2^-24 in [0, 1);  out[e] = 0 where u < p, else the float quotient 1 / (1 - p) - a tie u == p is kept.
 *   0 <= p < 1; n = 0 is a no-op.  tests/philox_ref.py states this bit for bit (DESIGN.md 5.13 has the stream-id map). */
int t2_philox_mask(float* out, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* zoneout masks: 1 with probability p, else 0 - no rescaling; the same counter convention (0 <= p <= 1) */
int t2_philox_bernoulli(float* out, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);
int t2_sumsq(const float* g, int64_t n, double* out, void* stream);
/* A step whose global gradient norm (sumsq) is NaN or infinite is SKIPPED: parameters and moments stay as they are (the
 * reference would write NaN into every weight, torch clip_grad_norm_ + Adam; there is nothing to match in that state). */
int t2_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, float max_norm, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* t2_adam_step with options: decoupled weight decay (AdamW) and an exponential moving average (EMA) of the parameters, folded
 * into the same elementwise pass.  The first fourteen fields are t2_adam_step's arguments.  With
 *   tot  = sqrt(*sumsq) * grad_scale,  clip = min(1, max_norm / (tot + 1e-6)) * grad_scale   (grad_scale alone when sumsq is NULL
 *   or max_norm <= 0),  bc1 = 1 - beta1^step,  bc2 = 1 - beta2^step                           - all as in t2_adam_step -
 * per element:
 *   decoupled = 0:  g' = g * clip + wd * p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;
 *                   p' = p - lr * (m' / bc1) / (sqrtf(v' / bc2) + eps)        exactly t2_adam_step's arithmetic, in its order
 *   decoupled = 1:  g' = g * clip (no wd * p term);  m', v' as above from g';
 *                   p1 = p * (1 - lr * wd);  p' = p1 - lr * (m' / bc1) / (sqrtf(v' / bc2) + eps)
 *                   torch.optim.AdamW's order: the decay first, then the step
 *   ema != NULL:    ema' = ema + (1 - d) * (p' - ema),  d = ema_decay         the lerp form of torch.optim.swa_utils: ema == p'
 *                   is a fixed point, so padding and tensors that do not move stay bit-equal to their parameter
 * A step whose *sumsq is not finite is SKIPPED: p, m, v and ema stay as they are.
 * With decoupled = 0 and ema = NULL the entry launches the kernel t2_adam_step launches.  T2_ERR_ARG before any launch: a null p, g,
 * m or v; n < 0; step < 1; decoupled not 0 or 1; with ema, ema_decay outside [0, 1) or NaN, or [ema, ema + n) overlapping
 * [p, p + n), g, m or v.  n == 0 is T2_OK without a launch. */
typedef struct {
    float* p; const float* g; float* m; float* v; int64_t n; const double* sumsq;
    float max_norm, lr, beta1, beta2, eps, weight_decay; int step; float grad_scale;
    float* ema; float ema_decay; int decoupled;
} T2AdamOpt;
int t2_adam_step_opt(const T2AdamOpt* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
