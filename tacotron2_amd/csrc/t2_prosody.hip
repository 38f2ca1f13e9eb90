// Prosody measurement of synthesised audio (include/tacotron2_amd.h: t2_yin, t2_prosody_stats): the YIN pitch tracker on
// the mel grid and per-utterance statistics of its track.  An evaluation path beside a ~50 ms decode, so both kernels are plain, in
// the style of t2_dtw.hip: no cross-workgroup synchronisation, nothing persistent, no atomics.
//
//   t2_yin: ONE 256-thread workgroup per (frame, utterance).  The span x[0 .. W + tau_max) is staged once in LDS.  Lanes run along
//     tau: at a fixed j the 64 lanes of a wave read x[j + tau] at consecutive addresses (conflict-free) and x[j] at one address (a
//     broadcast).  The j range is cut into four contiguous quarters, one per wave; every wave walks ALL lags (two per lane and pass, so
//     tau_max > 128 wraps into further passes) and leaves its partial d(tau) in its own LDS row; the rows are added in wave order.
//     The prefix sum over tau: every thread owns ceil(tau_max / 256) consecutive lags, then a wave scan by shuffles and the wave totals
//     in order.  The pick is a min-reduction of (index) and of (value, index) - order-independent - and a short walk by thread 0.
//     Every sum has a fixed association: two launches are bit-identical.
//   t2_prosody_stats: ONE workgroup per utterance; the track's voiced f0 in LDS, percentiles by rank counting over (value, index).
// Voice quality of a corpus (t2_voice_quality, t2_corpus_stats), in the same style:
//   t2_voice_quality: ONE workgroup per (frame, utterance), the same span in LDS; one thread per (cycle, lag) pair sums its product
//     left to right, the window energies are a running sum, the picks and the frame's means short serial walks (see vq_kernel).
//   t2_corpus_stats: ONE workgroup per utterance; counts and fp64 sums per thread, a shuffle tree, then the waves in order.
#include "t2_measure.hpp"

namespace {

#define PR_THREADS 256
#define PR_WAVES (PR_THREADS / T2_WAVE)

// (value, index) minimum, ties to the lower index
__device__ __forceinline__ bool yin_better(float ov, int oi, float mv, int mi) { return ov < mv || (ov == mv && oi < mi); }

__global__ __launch_bounds__(PR_THREADS) void yin_kernel(T2Yin p, int T) {
    extern __shared__ float lds[];
    __shared__ float red[PR_WAVES];
    __shared__ float red_v[PR_WAVES];
    __shared__ int red_i[PR_WAVES], red_f[PR_WAVES];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int W = p.W, TM = p.tau_max, S = W + TM, NT = TM + 1;
    float* x = lds;                 // [S] the span
    float* part = lds + S;          // [PR_WAVES][NT] partial d per wave; row 0 becomes d, then cm; row 1 the thread-local prefix
    const long o = (long)b * T + t;
    long nb = p.n[b];
    nb = nb < 0 ? 0 : (nb > p.n_max ? p.n_max : nb);
    long s0;
    if (!t2m_frame_valid(t, p.hop, S, nb, &s0)) {           // (uniform over the workgroup) nothing is read
        if (tid == 0) { p.f0[o] = 0.f; p.aper[o] = 1.f; p.power[o] = 0.f; }
        if (p.cmnd) for (int k = tid; k < NT; k += PR_THREADS) p.cmnd[o * NT + k] = 1.f;
        return;
    }
    const float* src = p.wav + (long)b * p.ld_wav + s0;
    for (int i = tid; i < S; i += PR_THREADS) x[i] = src[i];
    __syncthreads();

    // partial difference function of this wave's quarter of j, all lags
    const int Wq = (W + PR_WAVES - 1) / PR_WAVES, j0 = min(W, w * Wq), j1 = min(W, j0 + Wq);
    for (int tau0 = 0; tau0 < NT; tau0 += 2 * T2_WAVE) {
        const int ta = tau0 + lane, tb = ta + T2_WAVE;
        const float* xa = x + min(ta, TM);            // (lags behind tau_max: clamped to stay inside the span, not stored)
        const float* xb = x + min(tb, TM);
        float sa = 0.f, sb = 0.f;
#pragma unroll 4
        for (int j = j0; j < j1; ++j) {
            const float xj = x[j];
            const float da = xj - xa[j], db = xj - xb[j];
            sa = fmaf(da, da, sa);
            sb = fmaf(db, db, sb);
        }
        if (ta < NT) part[w * NT + ta] = sa;
        if (tb < NT) part[w * NT + tb] = sb;
    }
    float ps = 0.f;
    for (int j = tid; j < W; j += PR_THREADS) ps = fmaf(x[j], x[j], ps);
    const float power = t2_block_sum(ps, red) / (float)W;      // (its barriers also complete `part`)

    // d(tau) in wave order, and the prefix sum over tau: C consecutive lags per thread
    const int C = (TM + PR_THREADS - 1) / PR_THREADS;
    const int c0 = 1 + tid * C;
    float tot = 0.f;
    for (int i = 0; i < C; ++i) {
        const int tau = c0 + i;
        if (tau <= TM) {
            float d = part[tau];
#pragma unroll
            for (int r = 1; r < PR_WAVES; ++r) d += part[r * NT + tau];
            tot += d;
            part[tau] = d;
            part[NT + tau] = tot;
        }
    }
    float inc = tot;
#pragma unroll
    for (int s = 1; s < T2_WAVE; s <<= 1) {
        const float v = __shfl_up(inc, s, T2_WAVE);
        if (lane >= s) inc += v;
    }
    float excl = __shfl_up(inc, 1, T2_WAVE);
    if (lane == 0) excl = 0.f;
    __syncthreads();                                   // (red was read by every thread in t2_block_sum)
    if (lane == T2_WAVE - 1) red[w] = inc;
    __syncthreads();
    float base = 0.f;
    for (int r = 0; r < w; ++r) base += red[r];
    base += excl;
    for (int i = 0; i < C; ++i) {
        const int tau = c0 + i;
        if (tau <= TM) {
            const float sum = base + part[NT + tau];
            part[tau] = sum > 0.f ? part[tau] * (float)tau / sum : 1.f;
        }
    }
    if (tid == 0) part[0] = 1.f;
    __syncthreads();
    const float* cm = part;
    if (p.cmnd) for (int k = tid; k < NT; k += PR_THREADS) p.cmnd[o * NT + k] = cm[k];

    // the pick: the first lag under thr, and the first argmin, over [tau_min, tau_max)
    int first = 0x7fffffff, mi = 0x7fffffff;
    float mv = __builtin_inff();
    for (int c = p.tau_min + tid; c < TM; c += PR_THREADS) {
        const float v = cm[c];
        if (v < p.thr && c < first) first = c;
        if (v < mv) { mv = v; mi = c; }
    }
    first = t2m_wave_reduce(first, T2mMin());
    t2m_wave_pick(mv, mi, yin_better);
    if (lane == 0) { red_f[w] = first; red_v[w] = mv; red_i[w] = mi; }
    __syncthreads();
    if (tid == 0) {
        for (int r = 1; r < PR_WAVES; ++r) first = min(first, red_f[r]);
        t2m_combine_picks<PR_WAVES>(red_v, red_i, mv, mi, yin_better);
        int c = mi;
        if (first != 0x7fffffff) {
            c = first;
            while (c + 1 < TM && cm[c + 1] < cm[c]) ++c;
        }
        const float ap = cm[c];
        float f0 = 0.f;
        if (ap < p.vthr && power > p.power_floor) {
            const float a = cm[c - 1], e = cm[c + 1];          // (tau_min >= 2 and c < tau_max: both inside the row)
            const float den = a - 2.f * ap + e;
            float off = den > 0.f ? 0.5f * (a - e) / den : 0.f;
            off = fminf(fmaxf(off, -1.f), 1.f);
            f0 = (float)p.sr / ((float)c + off);
        }
        p.f0[o] = f0; p.aper[o] = ap; p.power[o] = power;
    }
}

__global__ __launch_bounds__(PR_THREADS) void prosody_stats_kernel(T2ProsodyStats p) {
    __shared__ float v[T2_PROSODY_MAX_T];              // f0 of the voiced frames, 0 elsewhere
    __shared__ double redd[3][PR_WAVES];
    __shared__ int redn[2][PR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, T = p.T;
    const long nb = p.n[b] < 0 ? 0 : p.n[b];
    const float* f0 = p.f0 + (long)b * T;
    const float* ap = p.aper + (long)b * T;
    const float* pw = p.power + (long)b * T;
    int cnt[2] = {0, 0};                               // valid, voiced
    double m[3] = {0.0, 0.0, 0.0};                     // log f0, 10 log10 power, aperiodicity over the voiced frames
    for (int t = tid; t < T; t += PR_THREADS) {
        long s0;
        const bool valid = t2m_frame_valid(t, p.hop, p.S, nb, &s0);
        const float f = valid ? f0[t] : 0.f;
        const bool voiced = f > 0.f;
        v[t] = voiced ? f : 0.f;
        cnt[0] += valid;
        if (voiced) {
            ++cnt[1];
            m[0] += (double)logf(f);
            m[1] += (double)(10.f * log10f(pw[t]));
            m[2] += (double)ap[t];
        }
    }
    t2m_sums_to_thread0(cnt, m, redn, redd);
    const int n_valid = cnt[0], n_voiced = cnt[1];     // (in every thread)
    float* out = p.out + (long)b * T2_PROSODY_NSTAT;
    if (tid == 0) {
        const float nan = __builtin_nanf("");
        out[0] = (float)n_valid; out[1] = (float)n_voiced;
        out[2] = n_voiced ? (float)(m[0] / n_voiced) : nan;
        out[5] = n_voiced ? (float)(m[1] / n_voiced) : nan;
        out[6] = n_voiced ? (float)(m[2] / n_voiced) : nan;
        out[7] = 0.f;
        if (!n_voiced) { out[3] = nan; out[4] = nan; }
    }
    if (!n_voiced) return;
    // rank of every voiced frame among the voiced frames by (value, index): a permutation of 0 .. n_voiced - 1, so exactly one frame
    // holds each of the two wanted ranks
    const int k5 = (5 * (n_voiced - 1) + 50) / 100, k95 = (95 * (n_voiced - 1) + 50) / 100;
    for (int t = tid; t < T; t += PR_THREADS) {
        const float f = v[t];
        if (f > 0.f) {
            int rank = 0;
            for (int j = 0; j < T; ++j) {
                const float g = v[j];
                rank += (g > 0.f && (g < f || (g == f && j < t))) ? 1 : 0;
            }
            if (rank == k5) out[3] = f;
            if (rank == k95) out[4] = f;
        }
    }
}

// t2_voice_quality: ONE workgroup per (frame, utterance), the span in LDS.  Work items are the (cycle, tau) pairs, one
// per thread and pass, in the order pair = cycle * ND + (tau - (L - d)): the lanes of a wave run along tau, so at a fixed j they read
// b at consecutive LDS addresses (conflict-free) and a at one address per cycle (a broadcast; a wave spans more than one cycle only
// when ND < 64, then with two or three distinct addresses).  The window energies are K + 1 left-to-right sums by the lanes of the
// last wave and a running update from tau = L outwards; cycle picks and the frame's means are short serial walks.
__global__ __launch_bounds__(PR_THREADS) void vq_kernel(T2VoiceQuality p, int T, int cap) {
    extern __shared__ float lds[];
    __shared__ float en[T2_VQ_MAX_CYCLES + 1];         // sum x[i L .. i L + L)^2
    __shared__ float cT[T2_VQ_MAX_CYCLES], cR[T2_VQ_MAX_CYCLES], cA[T2_VQ_MAX_CYCLES];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int S = p.W + p.tau_max;
    const long o = (long)b * T + t;
    long nb = p.n[b];
    nb = nb < 0 ? 0 : (nb > p.n_max ? p.n_max : nb);
    long s0;
    int K = 0, L = 0, d = 0;
    if (t2m_frame_valid(t, p.hop, S, nb, &s0)) {             // (uniform over the workgroup)
        const float f = p.f0[o];
        if (f > 0.f) {
            const float q = fminf(fmaxf((float)p.sr / f, (float)p.tau_min), (float)(p.tau_max - 1));
            L = (int)lrintf(q);
            d = max(2, (L + 7) / 8);
            const int room = S - 2 * L - d;
            K = room < 0 ? 0 : min(room / L + 1, T2_VQ_MAX_CYCLES);
        }
    }
    float* cyc = p.cyc ? p.cyc + o * (3 * T2_VQ_MAX_CYCLES) : nullptr;
    if (K < 3) {                                       // not measured: nothing of the signal is read
        if (tid == 0) { p.jitter[o] = 0.f; p.shimmer[o] = 0.f; p.nhr[o] = 0.f; p.hnr_db[o] = 0.f; p.cycles[o] = 0; }
        if (cyc) for (int k = tid; k < 3 * T2_VQ_MAX_CYCLES; k += PR_THREADS) cyc[k] = 0.f;
        return;
    }
    const int ND = 2 * d + 1;
    K = min(K, cap / ND);                              // (never binds - K ND <= cap, t2_voice_quality below; keeps the tables' bounds local)
    const int NP = K * ND;
    float* x = lds;                                    // [S] the span
    float* dot = lds + S;                              // [cap] sum a b per pair, then ncc
    float* eb = dot + cap;                             // [cap] sum b^2 per pair
    const float* src = p.wav + (long)b * p.ld_wav + s0;
    for (int i = tid; i < S; i += PR_THREADS) x[i] = src[i];
    __syncthreads();

    if (tid >= PR_THREADS - T2_WAVE && tid - (PR_THREADS - T2_WAVE) <= K) {      // (K + 1 <= 33 lanes of the last wave)
        const float* a = x + (tid - (PR_THREADS - T2_WAVE)) * L;                 // (K + 1) L <= S
        float s = 0.f;
        for (int j = 0; j < L; ++j) s = fmaf(a[j], a[j], s);
        en[tid - (PR_THREADS - T2_WAVE)] = s;
    }
    for (int pp = tid; pp < NP; pp += PR_THREADS) {
        const int i = pp / ND, k = pp - i * ND;
        const float* a = x + i * L;
        const float* bb = a + (L - d + k);             // last read: (K - 1) L + (L + d) + L - 1 <= S - 1
        float s = 0.f;
#pragma unroll 4
        for (int j = 0; j < L; ++j) s = fmaf(a[j], bb[j], s);
        dot[pp] = s;
    }
    __syncthreads();
    if (tid < K) {                                     // sum b^2: the window of tau = L is that of the next cycle's a
        const float* a = x + tid * L;
        float* e = eb + tid * ND + d;
        float s = en[tid + 1];
        e[0] = s;
        for (int k = 1; k <= d; ++k) {                 // tau = L + k from L + k - 1: x[c + tau - 1] leaves, x[c + tau - 1 + L] enters
            const float lo = a[L + k - 1], hi = a[2 * L + k - 1];
            s = fmaf(hi, hi, fmaf(-lo, lo, s));
            e[k] = s;
        }
        s = en[tid + 1];
        for (int k = 1; k <= d; ++k) {                 // tau = L - k from L - k + 1: x[c + tau] enters, x[c + tau + L] leaves
            const float lo = a[L - k], hi = a[2 * L - k];
            s = fmaf(lo, lo, fmaf(-hi, hi, s));
            e[-k] = s;
        }
    }
    __syncthreads();
    for (int pp = tid; pp < NP; pp += PR_THREADS) {
        const float den = en[pp / ND] * eb[pp];
        dot[pp] = den > 0.f ? dot[pp] / sqrtf(den) : 0.f;
    }
    __syncthreads();
    if (tid < K) {
        const float* c = dot + tid * ND;
        int ki = 0;
        float m = c[0];
        for (int k = 1; k < ND; ++k)
            if (c[k] > m) { m = c[k]; ki = k; }
        float off = 0.f;
        if (ki > 0 && ki < ND - 1) {
            const float a = c[ki - 1], e = c[ki + 1];
            const float den = a - 2.f * m + e;
            off = den < 0.f ? 0.5f * (a - e) / den : 0.f;
            off = fminf(fmaxf(off, -1.f), 1.f);
        }
        cT[tid] = (float)(L - d + ki) + off;
        cR[tid] = m;
        cA[tid] = sqrtf(en[tid] / (float)L);
    }
    __syncthreads();
    if (cyc)
        for (int k = tid; k < 3 * T2_VQ_MAX_CYCLES; k += PR_THREADS) {
            const int i = k / 3, q = k - 3 * i;
            cyc[k] = i < K ? (q == 0 ? cT[i] : (q == 1 ? cR[i] : cA[i])) : 0.f;
        }
    if (tid == 0) {
        float sT = 0.f, sA = 0.f, sR = 0.f, dT = 0.f, dA = 0.f;
        for (int i = 0; i < K; ++i) { sT += cT[i]; sA += cA[i]; sR += cR[i]; }
        for (int i = 0; i + 1 < K; ++i) { dT += fabsf(cT[i + 1] - cT[i]); dA += fabsf(cA[i + 1] - cA[i]); }
        const float mT = sT / (float)K, mA = sA / (float)K;
        const float r = fminf(fmaxf(sR / (float)K, 1e-3f), 1.f - 1e-6f);
        p.jitter[o] = dT / (float)(K - 1) / mT;
        p.shimmer[o] = mA > 0.f ? dA / (float)(K - 1) / mA : 0.f;
        p.nhr[o] = (1.f - r) / r;
        p.hnr_db[o] = 10.f * log10f(r / (1.f - r));
        p.cycles[o] = K;
    }
}

__global__ __launch_bounds__(PR_THREADS) void corpus_stats_kernel(T2CorpusStats p) {
    __shared__ double redd[6][PR_WAVES];
    __shared__ int redn[4][PR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, T = p.T;
    const long nb = p.n[b] < 0 ? 0 : p.n[b];
    const long r0 = (long)b * T;
    int cnt[4] = {0, 0, 0, 0};                         // valid, voiced, measured, loud
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // f0, jitter, shimmer, nhr, hnr_db, 10 log10 power
    for (int t = tid; t < T; t += PR_THREADS) {
        long s0;
        if (!t2m_frame_valid(t, p.hop, p.S, nb, &s0)) continue;          // an invalid frame is not read
        ++cnt[0];
        const float f = p.f0[r0 + t], pw = p.power[r0 + t];
        if (f > 0.f) { ++cnt[1]; s[0] += (double)f; }
        if (p.cycles[r0 + t] > 0) {
            ++cnt[2];
            s[1] += (double)p.jitter[r0 + t]; s[2] += (double)p.shimmer[r0 + t];
            s[3] += (double)p.nhr[r0 + t]; s[4] += (double)p.hnr_db[r0 + t];
        }
        if (pw > p.power_floor) { ++cnt[3]; s[5] += (double)(10.f * log10f(pw)); }
    }
    t2m_sums_to_thread0(cnt, s, redn, redd);
    if (tid == 0) {
        float* out = p.out + (long)b * T2_CORPUS_NSTAT;
        for (int q = 0; q < 4; ++q) out[q] = (float)cnt[q];
        out[4] = cnt[1] ? (float)(s[0] / cnt[1]) : 0.f;
        for (int q = 1; q < 5; ++q) out[4 + q] = cnt[2] ? (float)(s[q] / cnt[2]) : 0.f;
        out[9] = cnt[3] ? (float)(s[5] / cnt[3]) : 0.f;
        out[10] = 0.f; out[11] = 0.f;
    }
}

// The frame geometry t2_yin and t2_voice_quality share (G: T2Yin or T2VoiceQuality); *T_out = the frames of a padded row.
template <typename G>
int pr_geometry(const char* name, const G* a, int64_t* T_out) {
#define PR_REQUIRE(cond, text)                                                \
    do {                                                                      \
        if (!(cond)) {                                                        \
            char msg[96];                                                     \
            snprintf(msg, sizeof(msg), "%s: %s", name, text);                 \
            T2_REQUIRE(false, msg);                                           \
        }                                                                     \
    } while (0)
    PR_REQUIRE(a->B >= 1 && a->B <= 65535, "B outside 1 .. 65535");
    PR_REQUIRE(a->n_max >= 0, "n_max < 0");
    PR_REQUIRE(a->hop >= 1 && a->sr >= 1, "need hop, sr >= 1");
    PR_REQUIRE(a->W >= 16, "W below 16");
    PR_REQUIRE(a->tau_min >= 2, "tau_min below 2");
    PR_REQUIRE(a->tau_max > a->tau_min + 1, "need tau_max > tau_min + 1");
    PR_REQUIRE((int64_t)a->W + a->tau_max <= T2_YIN_MAX_SPAN, "W + tau_max above T2_YIN_MAX_SPAN (4096)");
    PR_REQUIRE(a->ld_wav >= a->n_max, "ld_wav < n_max");
    *T_out = 1 + a->n_max / a->hop;
    PR_REQUIRE(*T_out <= 0x7fffffff, "more than 2^31 - 1 frames");
#undef PR_REQUIRE
    return T2_OK;
}

}  // namespace

extern "C" int t2_voice_quality(const T2VoiceQuality* a, void* stream) {
    (void)hipGetLastError();
    T2_REQUIRE(a && a->wav && a->n && a->f0 && a->jitter && a->shimmer && a->nhr && a->hnr_db && a->cycles, "t2_voice_quality: null");
    int64_t T;
    T2_TRY(pr_geometry("t2_voice_quality", a, &T));
    // pairs of one frame: K <= S / L cycles of 2 d + 1 <= L / 4 + 3 lags for L >= 16 (<= S/4 + 3 S/16), 32 cycles of 5 lags below
    const int S = a->W + a->tau_max, cap = S / 2 + 160;
    const size_t bytes = ((size_t)S + 2 * (size_t)cap) * sizeof(float);
    hipLaunchKernelGGL(vq_kernel, dim3((unsigned)T, (unsigned)a->B), dim3(PR_THREADS), bytes, ST, *a, (int)T, cap);
    T2_CHECK_LAUNCH(); return T2_OK;
}

extern "C" int t2_corpus_stats(const T2CorpusStats* a, void* stream) {
    (void)hipGetLastError();
    T2_REQUIRE(a && a->f0 && a->power && a->jitter && a->shimmer && a->nhr && a->hnr_db && a->cycles && a->n && a->out,
               "t2_corpus_stats: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_corpus_stats: B outside 1 .. 65535");
    T2_REQUIRE(a->T >= 1, "t2_corpus_stats: T < 1");
    T2_REQUIRE(a->hop >= 1 && a->S >= 1, "t2_corpus_stats: need hop, S >= 1");
    T2_REQUIRE(a->power_floor == a->power_floor, "t2_corpus_stats: power_floor is NaN");
    hipLaunchKernelGGL(corpus_stats_kernel, dim3((unsigned)a->B), dim3(PR_THREADS), 0, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}

extern "C" int t2_yin(const T2Yin* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->wav && a->n && a->f0 && a->aper && a->power, "t2_yin: null");
    int64_t T;
    T2_TRY(pr_geometry("t2_yin", a, &T));
    const size_t bytes = ((size_t)a->W + a->tau_max + (size_t)PR_WAVES * (a->tau_max + 1)) * sizeof(float);
    T2_REQUIRE(t2_allow_lds(yin_kernel, bytes), "t2_yin: LDS request refused");
    hipLaunchKernelGGL(yin_kernel, dim3((unsigned)T, (unsigned)a->B), dim3(PR_THREADS), bytes, ST, *a, (int)T);
    T2_CHECK_LAUNCH(); return T2_OK;
}

extern "C" int t2_prosody_stats(const T2ProsodyStats* a, void* stream) {
    (void)hipGetLastError();
    T2_REQUIRE(a && a->f0 && a->aper && a->power && a->n && a->out, "t2_prosody_stats: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_prosody_stats: B outside 1 .. 65535");
    T2_REQUIRE(a->T >= 1 && a->T <= T2_PROSODY_MAX_T, "t2_prosody_stats: T outside 1 .. T2_PROSODY_MAX_T (4096)");
    T2_REQUIRE(a->hop >= 1 && a->S >= 1, "t2_prosody_stats: need hop, S >= 1");
    hipLaunchKernelGGL(prosody_stats_kernel, dim3((unsigned)a->B), dim3(PR_THREADS), 0, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
