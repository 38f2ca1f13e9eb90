// Smoothed pitch and F0 metrics (include/tacotron2_amd.h: t2_pitch_viterbi, t2_f0_path_stats): a Viterbi decode through
// t2_yin's normalised difference function, and the statistics of two pitch tracks along t2_dtw's path.  An evaluation path, so both
// kernels are plain, in the style of t2_dtw.hip and t2_prosody.hip: no cross-workgroup synchronisation, nothing persistent, no atomics.
//
//   t2_pitch_viterbi: ONE 256-thread workgroup per utterance walks the frames.  Frame t reads row t-1 of D only, so two rotating rows
//     of fp64 D [N+1] live in LDS beside the lw table; thread `tid` owns the voiced targets k = tid, tid + 256, ... and walks each
//     one's run of allowed predecessors [lo, hi] (found once, in registers) in ascending order; the last thread also owns target U.
//     U's minimum over ALL voiced predecessors of the next frame is a reduction of D_t[k] + c_sw: every thread forms that sum as it
//     writes D_t[k], the waves reduce (value, index) by shuffles - order-independent, ties to the lower index - and leave four
//     partials beside D in front of the frame's ONE barrier; the owner of U combines them in the next frame.  cmnd of frame t+1 is
//     loaded BEFORE the barrier of frame t, so no global load sits between a barrier and the LDS reads that depend on it.  The back
//     pointers go to global memory (uint16), thread 0 walks them back (T dependent loads), then the block forms f0 and aper.
//   t2_f0_path_stats: ONE workgroup per pair strides over the path's cells; counts and fp64 sums by wave shuffles, then in wave order.
#include "t2_measure.hpp"

namespace {

#define PV_THREADS 256
#define PV_WAVES (PV_THREADS / T2_WAVE)
#define PV_NONE 0x7fffffff
#define PV_CHUNK 8

// (value, index) minimum, ties to the lower index
__device__ __forceinline__ bool pv_better(double ov, int oi, double mv, int mi) { return ov < mv || (ov == mv && oi < mi); }

// MAXC = the voiced targets one thread can own: N <= MAXC * 256.  dynamic LDS: D[2][N+1] doubles, then lw[N]
template <int MAXC>
__global__ __launch_bounds__(PV_THREADS) void pitch_viterbi_kernel(T2PitchViterbi p) {
    extern __shared__ double lds[];
    __shared__ double wv[2][PV_WAVES];                   // wave minima of D_t[k] + c_sw and their states, by parity of t
    __shared__ int wi[2][PV_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int T = p.T, tau_min = p.tau_min, N = p.tau_max - p.tau_min, NS = N + 1;
    double* D = lds;
    double* lw = lds + 2 * (long)NS;
    const int n = min(max(p.len[b], 0), T);
    const long o = (long)b * T;
    for (int t = n + tid; t < T; t += PV_THREADS) { p.f0[o + t] = 0.f; p.aper[o + t] = 1.f; p.lag[o + t] = 0; }
    if (n == 0) {                                        // (uniform over the workgroup) nothing is read
        if (tid == 0) p.cost[b] = 0.0;
        return;
    }
    for (int k = tid; k < N; k += PV_THREADS) lw[k] = p.lw[k];
    __syncthreads();

    const double inf = (double)__builtin_inff();
    const double tmax = p.trans_max, c_sw = p.c_sw;
    const int nc = (N + PV_THREADS - 1) / PV_THREADS;    // (<= MAXC: the entry picks the instance)
    int lo[MAXC], hi[MAXC];                              // the run of allowed predecessors of every owned target: once per launch
    double lwk[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int k = tid + c * PV_THREADS;
        lo[c] = 0; hi[c] = -1; lwk[c] = 0.0;
        if (c < nc && k < N) {
            const double x = lw[k];
            int a = k, e = k;
            while (a > 0 && fabs(x - lw[a - 1]) <= tmax) --a;
            while (e + 1 < N && fabs(x - lw[e + 1]) <= tmax) ++e;
            lo[c] = a; hi[c] = e; lwk[c] = x;
        }
    }

    const float* cm = p.cmnd + (long)b * p.ld_b + tau_min;           // cm[t * ld_t + k] = cmnd of state k
    const float* pw = p.power + o;
    const int64_t ldt = p.ld_t;
    uint16_t* back = p.back + o * NS;
    const float finf = __builtin_inff();
    float ln[MAXC];                                      // local costs of this thread's targets in the NEXT frame
    {
        const bool loud = pw[0] > p.power_floor;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int k = tid + c * PV_THREADS;
            ln[c] = (c < nc && k < N && loud) ? cm[k] : finf;
        }
    }
    for (int t = 0; t < n; ++t) {
        float lc[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) lc[c] = ln[c];
        if (t + 1 < n) {
            const bool loud = pw[t + 1] > p.power_floor;
            const float* row = cm + (long)(t + 1) * ldt;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int k = tid + c * PV_THREADS;
                ln[c] = (c < nc && k < N && loud) ? row[k] : finf;
            }
        }
        const int pc = t & 1, pp = pc ^ 1;
        double* Dc = D + (long)pc * NS;
        const double* Dp = D + (long)pp * NS;
        uint16_t* bk = back + (long)t * NS;
        double mv = inf;
        int mi = PV_NONE;
        const double du = t ? Dp[N] + c_sw : 0.0;        // U as a predecessor of a voiced target
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int k = tid + c * PV_THREADS;
            if (c < nc && k < N) {
                double d;
                if (t == 0) {
                    d = (double)lc[c];
                } else {
                    double best = inf;
                    int arg = lo[c];
                    const double x = lwk[c];
                    // eight predecessors per pass: their sixteen LDS loads are issued together (one wave per SIMD: nothing else hides
                    // the latency), then compared in ascending order
                    int kp = lo[c];
                    const int he = hi[c] + 1;
                    for (; kp + PV_CHUNK <= he; kp += PV_CHUNK) {
                        double dv[PV_CHUNK], lv[PV_CHUNK];
#pragma unroll
                        for (int q = 0; q < PV_CHUNK; ++q) { dv[q] = Dp[kp + q]; lv[q] = lw[kp + q]; }
#pragma unroll
                        for (int q = 0; q < PV_CHUNK; ++q) {
                            const double cand = dv[q] + fabs(x - lv[q]);
                            if (cand < best) { best = cand; arg = kp + q; }
                        }
                    }
                    for (; kp < he; ++kp) {
                        const double cand = Dp[kp] + fabs(x - lw[kp]);
                        if (cand < best) { best = cand; arg = kp; }
                    }
                    if (du < best) { best = du; arg = N; }
                    d = best + (double)lc[c];
                    bk[k] = (uint16_t)arg;
                }
                Dc[k] = d;
                const double cand = d + c_sw;            // this state as a predecessor of U in frame t + 1
                if (cand < mv) { mv = cand; mi = k; }    // (k ascends with c: a later one wins only when strictly smaller)
            }
        }
        t2m_wave_pick(mv, mi, pv_better);
        if (lane == 0) { wv[pc][w] = mv; wi[pc][w] = mi; }
        if (tid == PV_THREADS - 1) {                     // target U: U first, then the voiced predecessors ascending
            if (t == 0) {
                Dc[N] = p.u;
            } else {
                double vv; int vi;
                t2m_combine_picks<PV_WAVES>(wv[pp], wi[pp], vv, vi, pv_better);
                double best = Dp[N] + 0.0;
                int arg = N;
                if (vv < best && vi < N) { best = vv; arg = vi; }
                Dc[N] = best + p.u;
                bk[N] = (uint16_t)arg;
            }
        }
        __syncthreads();      // one barrier per frame: row pc and its wave minima are complete, row pp is free for frame t + 1
    }

    // termination: the first minimum over the voiced states, then U
    const int pl = (n - 1) & 1;
    const double* Dl = D + (long)pl * NS;
    {
        double mv = inf;
        int mi = PV_NONE;
        for (int k = tid; k < N; k += PV_THREADS) {
            const double d = Dl[k];
            if (d < mv) { mv = d; mi = k; }
        }
        t2m_wave_pick(mv, mi, pv_better);
        if (lane == 0) { wv[pl ^ 1][w] = mv; wi[pl ^ 1][w] = mi; }       // (the other parity: last read in front of the last barrier)
    }
    __syncthreads();
    if (tid == 0) {
        double vv; int vi;
        t2m_combine_picks<PV_WAVES>(wv[pl ^ 1], wi[pl ^ 1], vv, vi, pv_better);
        int s = vi < N ? vi : N;
        double best = s < N ? vv : Dl[N];
        if (Dl[N] < best) { best = Dl[N]; s = N; }
        p.cost[b] = best;
        for (int t = n - 1; t >= 0; --t) {               // the walk back: one dependent load per frame
            p.lag[o + t] = s < N ? tau_min + s : 0;
            if (t > 0) s = min((int)back[(long)t * NS + s], N);
        }
    }
    __syncthreads();                                     // the lags of thread 0 are visible to the workgroup
    for (int t = tid; t < n; t += PV_THREADS) {
        const int c = p.lag[o + t];
        float f0 = 0.f, ap = 1.f;
        if (c > 0) {
            const float* r = p.cmnd + (long)b * p.ld_b + (long)t * ldt;
            ap = r[c];
            const float a = r[c - 1], e = r[c + 1];      // (tau_min >= 2 and c < tau_max: both inside the row)
            const float den = a - 2.f * ap + e;
            float off = den > 0.f ? 0.5f * (a - e) / den : 0.f;
            off = fminf(fmaxf(off, -1.f), 1.f);
            f0 = (float)p.sr / ((float)c + off);
        }
        p.f0[o + t] = f0; p.aper[o + t] = ap;
    }
}

__device__ __forceinline__ bool f0_valid(long t, int T, int hop, int S, long n) {
    long s0;
    return t >= 0 && t < T && t2m_frame_valid(t, hop, S, n, &s0);
}

__global__ __launch_bounds__(PV_THREADS) void f0_path_stats_kernel(T2F0PathStats p) {
    __shared__ double redd[7][PV_WAVES];
    __shared__ int redn[4][PV_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(p.path_len[b], 0), p.P);
    double* out = p.out + (long)b * T2_F0_NSTAT;
    if (n == 0) {                                        // (uniform) nothing is read
        if (tid < T2_F0_NSTAT) out[tid] = 0.0;
        return;
    }
    const long na = p.n_a[b] < 0 ? 0 : p.n_a[b], nb = p.n_b[b] < 0 ? 0 : p.n_b[b];
    const int32_t* path = p.path + (long)b * p.P * 2;
    const float* fa = p.f0_a + (long)b * p.Ta;
    const float* fb = p.f0_b + (long)b * p.Tb;
    int cnt[4] = {0, 0, 0, 0};
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = tid; c < n; c += PV_THREADS) {
        const int i = path[2 * c], j = path[2 * c + 1];
        if (!f0_valid(i, p.Ta, p.hop, p.S, na) || !f0_valid(j, p.Tb, p.hop, p.S, nb)) continue;
        const float x = fa[i], y = fb[j];
        const bool va = x > 0.f, vb = y > 0.f;
        ++cnt[0];
        if (va && vb) {
            ++cnt[1];
            const double la = log2((double)x), lb = log2((double)y);
            const double d = 1200.0 * (la - lb);
            s[0] += d; s[1] += d * d; s[2] += la; s[3] += lb; s[4] += la * la; s[5] += lb * lb; s[6] += la * lb;
        } else if (va) {
            ++cnt[2];
        } else if (vb) {
            ++cnt[3];
        }
    }
    t2m_sums_to_thread0(cnt, s, redn, redd);
    if (tid == 0) {
        for (int q = 0; q < 4; ++q) out[q] = (double)cnt[q];
        for (int q = 0; q < 7; ++q) out[4 + q] = s[q];
        out[11] = 0.0;
    }
}

inline bool pv_cost_ok(double v) { return v == v && v - v == 0.0 && v >= 0.0; }      // finite and not negative

}  // namespace

extern "C" int t2_pitch_viterbi(const T2PitchViterbi* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->cmnd && a->power && a->len && a->lw && a->f0 && a->aper && a->lag && a->cost && a->back,
               "t2_pitch_viterbi: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_pitch_viterbi: B outside 1 .. 65535");
    T2_REQUIRE(a->T >= 1 && a->T <= T2_PROSODY_MAX_T, "t2_pitch_viterbi: T outside 1 .. T2_PROSODY_MAX_T (4096)");
    T2_REQUIRE(a->sr >= 1, "t2_pitch_viterbi: sr < 1");
    T2_REQUIRE(a->tau_min >= 2, "t2_pitch_viterbi: tau_min below 2");
    T2_REQUIRE(a->tau_max > a->tau_min + 1, "t2_pitch_viterbi: need tau_max > tau_min + 1");
    const int64_t N = (int64_t)a->tau_max - a->tau_min;
    T2_REQUIRE(N <= T2_PITCH_MAX_STATES, "t2_pitch_viterbi: tau_max - tau_min above T2_PITCH_MAX_STATES (4096)");
    T2_REQUIRE(a->ld_t >= (int64_t)a->tau_max + 1 && (a->B == 1 || a->ld_b >= (int64_t)(a->T - 1) * a->ld_t + a->tau_max + 1),
               "t2_pitch_viterbi: overlapping strides of cmnd: need ld_t >= tau_max + 1, ld_b >= (T-1)*ld_t + tau_max + 1");
    T2_REQUIRE(pv_cost_ok(a->trans_max) && pv_cost_ok(a->u) && pv_cost_ok(a->c_sw),
               "t2_pitch_viterbi: trans_max, u and c_sw must be finite and not negative");
    T2_REQUIRE(a->power_floor == a->power_floor, "t2_pitch_viterbi: power_floor is NaN");
    const size_t bytes = (3 * (size_t)N + 2) * sizeof(double);
    if (N <= 2 * PV_THREADS) {           // the default lag range (323 states) owns two targets per thread
        T2_REQUIRE(t2_allow_lds(pitch_viterbi_kernel<2>, bytes), "t2_pitch_viterbi: LDS request refused");
        hipLaunchKernelGGL(pitch_viterbi_kernel<2>, dim3((unsigned)a->B), dim3(PV_THREADS), bytes, ST, *a);
    } else {
        T2_REQUIRE(t2_allow_lds(pitch_viterbi_kernel<T2_PITCH_MAX_STATES / PV_THREADS>, bytes), "t2_pitch_viterbi: LDS request refused");
        hipLaunchKernelGGL(pitch_viterbi_kernel<T2_PITCH_MAX_STATES / PV_THREADS>, dim3((unsigned)a->B), dim3(PV_THREADS), bytes, ST, *a);
    }
    T2_CHECK_LAUNCH(); return T2_OK;
}

extern "C" int t2_f0_path_stats(const T2F0PathStats* a, void* stream) {
    (void)hipGetLastError();
    T2_REQUIRE(a && a->path && a->path_len && a->f0_a && a->f0_b && a->n_a && a->n_b && a->out, "t2_f0_path_stats: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_f0_path_stats: B outside 1 .. 65535");
    T2_REQUIRE(a->P >= 1 && a->Ta >= 1 && a->Tb >= 1, "t2_f0_path_stats: need P, Ta, Tb >= 1");
    T2_REQUIRE(a->hop >= 1 && a->S >= 1, "t2_f0_path_stats: need hop, S >= 1");
    hipLaunchKernelGGL(f0_path_stats_kernel, dim3((unsigned)a->B), dim3(PV_THREADS), 0, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
