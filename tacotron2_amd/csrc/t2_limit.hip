// Look-ahead true-peak limiter of a padded batch of waveforms (include/tacotron2_amd.h: t2_limit; restated sequentially
// in float64 in tests/limiter_ref.py).  Four launches on one stream, plain, in the style of t2_loudness.hip: no cross-workgroup
// synchronisation, nothing persistent, every sum in a fixed order; the one atomic is an integer maximum, which has no order.
//
//   envelope  grid (tiles of 1024 samples, B), 256 threads: the tile's span, 1024 + 2K floats from the sample tile0 - K on, staged in
//             LDS with zeros outside [0, n) as t2_loudness's peak launch stages it; P of the 1025 samples tile0 - 1 .. tile0 + 1023
//             (t2m_peak4: that launch's taps) goes to LDS and env[i] = max(P[i-1], P[i]) is written.
//   curve     one 256-thread workgroup per row.  It first reads the row's env for in_peak and n_over; a row without a sample above
//             the ceiling gets curve = 1 and is done.  Else the row runs in passes of LM_PASS = 4096 samples:
//               r over the pass and L samples behind it (1 behind n: neutral for a minimum);
//               h by doubling, m_{k+1}[j] = min(m_k[j], m_k[j + 2^k]), between two LDS buffers: with 2^q the largest power of two
//                 <= L + 1,  h[j] = min(m_q[j], m_q[j + L + 1 - 2^q]) - a minimum over exactly j .. j + L whatever the grouping;
//               the release, a * e + (1 - a) in two roundings as the rule states it: thread t runs the 16 samples of its chunk
//                 from e = 1 (thread 0 from the state the pass before left) and publishes d = 1 - e; the chunk ends meet in an
//                 inclusive Hillis-Steele scan of 8 steps,
//                 d[t] = max(d[t], a^(16 2^k) d[t - 2^k]) - e = min(h, 1 - a d) is d = max(1 - h, a d), linear in (max, x) -, the
//                 8 powers formed by the entry in fp64.  The recurrence itself does not reach 1 from below: with e = 1 - k 2^-53 a
//                 step is k' = round(a k), which stops at the largest k with (1 - a) k < 1/2, about tau / 2 ulps under 1, and
//                 every release ends exactly there; a product that is not zero is held at that `stall`, found by the entry with
//                 the recurrence's own arithmetic, so a chunk starts where the sequential rule stands.
//                 Every thread then runs its chunk AGAIN, from 1 - d[t-1], and leaves e in
//                 LDS behind the L values of e the pass before left (the first pass: h[0]);
//               the box sum: a thread adds the L + 1 values of its first sample in ascending index and slides, (s + new) - old,
//                 over the 15 others; curve = (float)(s / (L + 1)); the last L values of e move to the front.
//             LDS, dynamic, with n = LM_PASS + L: e as n + n / 16 + 1 doubles (one double of padding per 16: a thread's chunk
//             starts on its own bank), the scan's two buffers of 256 doubles, two buffers of n floats.  L = 2048, the largest:
//             52 232 + 4 096 + 49 152 = 105 480 bytes of the CU's 160 KB; L = 110 (5 ms at 22 050 Hz): 73 456.
//   apply     the envelope's grid and staging over w = x * curve - one float32 product, the same for a sample in a tile and in its
//             neighbour's span -; the tile writes its own w to y and joins max P into stat[3] through atomicMax on the bits of the
//             value as a double.  A row that is not active is copied: w = x, and its peak is in_peak (the curve launch wrote it).
//   trim      grid (chunks, B): t from stat[3], y *= t where peak_after > c (row-uniform), zeros behind n.
#include <math.h>
#include "t2_measure.hpp"

namespace {

#define LM_THREADS 256
#define LM_WAVES (LM_THREADS / 64)
#define LM_CHUNK 16
#define LM_PASS (LM_THREADS * LM_CHUNK)
#define LM_STEPS 8                 // log2(LM_THREADS)
#define LM_PADE(j) ((j) + ((j) >> 4))
#define LM_TILE 1024
#define LM_TRIM_CHUNK 1024

struct LmPow { double m[LM_STEPS], stall; };       // m[k] = a^(16 * 2^k); stall: where the fp64 release stops short of 1, as 1 - e

size_t lm_curve_lds(int L) {
    const size_t len = (size_t)LM_PASS + (size_t)L;
    return (LM_PADE(len) + 1) * sizeof(double) + 2 * LM_THREADS * sizeof(double) + 2 * len * sizeof(float);
}

// WPEAK 0: the envelope of x.  1: w = x * curve, written to y, and its peak.
template <int WPEAK>
__global__ __launch_bounds__(256) void lim_peak_kernel(T2Limit p) {
    extern __shared__ __attribute__((aligned(16))) float lm_xs[];      // [LM_TILE + 2K] the span, [LM_TILE + 1] P
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (!t2m_count_ok(p.n[b], p.n_max)) return;
    const int64_t n = p.n[b], tile0 = (int64_t)blockIdx.x * LM_TILE;
    if (tile0 >= n) return;                                             // (uniform) behind the row: nothing is read
    const int K = p.K;
    const float* x = p.x + (int64_t)b * p.ldx;
    double* st = p.stat + (int64_t)b * T2_LIMIT_NSTAT;
    if (WPEAK && st[5] == 0.0) {                                        // (uniform) not active: w = x, peak_after = in_peak
        float* y = p.y + (int64_t)b * p.ldy;
        for (int i = tid; i < LM_TILE && tile0 + i < n; i += 256) y[tile0 + i] = x[tile0 + i];
        return;
    }
    const float* curve = p.curve + (int64_t)b * p.ldc;
    float* Ps = lm_xs + LM_TILE + 2 * K;
    const int64_t span0 = tile0 - K;
    for (int i = tid; i < LM_TILE + 2 * K; i += 256) {
        const int64_t g = span0 + i;
        float v = 0.f;
        if (g >= 0 && g < n) {
            v = x[g];
            if (WPEAK) {
                v *= curve[g];
                if (g >= tile0 && g < tile0 + LM_TILE) p.y[(int64_t)b * p.ldy + g] = v;
            }
        }
        lm_xs[i] = v;
    }
    __syncthreads();
    float top = 0.f;
    for (int qq = tid + WPEAK; qq < LM_TILE + 1; qq += 256) {           // (WPEAK: the tile's own samples alone, from qq = 1)
        const int64_t i = tile0 - 1 + qq;                               // P[i]: xr = the sample i - K + 1
        float P = 0.f;
        if (i >= 0 && i < n) {
            const float* xr = lm_xs + qq;
            P = fmaxf(fabsf(xr[K - 1]), t2m_peak4(p.table, K, xr));
        }
        if (WPEAK) top = fmaxf(top, P);
        else Ps[qq] = P;
    }
    if (WPEAK) {
        top = t2_block_max(top, red);
        if (tid == 0) atomicMax(reinterpret_cast<unsigned long long*>(st + 3), (unsigned long long)__double_as_longlong((double)top));
        return;
    }
    __syncthreads();
    float* env = p.env + (int64_t)b * p.lde;
    for (int q = tid; q < LM_TILE && tile0 + q < n; q += 256) env[tile0 + q] = fmaxf(Ps[q], Ps[q + 1]);
}

__global__ __launch_bounds__(LM_THREADS) void lim_curve_kernel(T2Limit p, LmPow pw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_smem[];
    __shared__ double redd[LM_WAVES];
    __shared__ long long redi[LM_WAVES];
    __shared__ float redf[LM_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, L = p.L, len = LM_PASS + L;
    double* st = p.stat + (int64_t)b * T2_LIMIT_NSTAT;
    if (!t2m_count_ok(p.n[b], p.n_max)) {
        if (tid == 0) st[5] = -1.0;
        return;
    }
    double* eb = reinterpret_cast<double*>(lm_smem);                    // [LM_PADE(len) + 1]: e of i at LM_PADE(L + i - p0)
    double* sc = eb + LM_PADE(len) + 1;                                 // [2][LM_THREADS]
    float* ra = reinterpret_cast<float*>(sc + 2 * LM_THREADS);          // [len]
    float* rb = ra + len;                                               // [len]
    const int64_t n = p.n[b];
    const double c = p.ceiling, a = p.a, oma = 1.0 - p.a;
    const float* env = p.env + (int64_t)b * p.lde;
    float* curve = p.curve + (int64_t)b * p.ldc;
    float mx = 0.f;
    long long over = 0;
    for (int64_t i = tid; i < n; i += LM_THREADS) {
        const float v = env[i];
        mx = fmaxf(mx, v);
        over += (double)v > c ? 1 : 0;
    }
    mx = t2m_block_reduce<LM_WAVES>(mx, T2mMax(), redf);
    over = t2m_block_reduce<LM_WAVES>(over, T2mSum(), redi);
    double mn = 1.0;
    if (over == 0) {                                                    // (uniform) s == 1 exactly
        for (int64_t i = tid; i < n; i += LM_THREADS) curve[i] = 1.0f;
    } else {
        int q = 0;
        while ((2 << q) <= L + 1) ++q;                                  // 2^q <= L + 1 < 2^(q+1)
        const int off = L + 1 - (1 << q);
        double carry = 1.0;                                             // e in front of the pass: the same in every thread
        for (int64_t p0 = 0; p0 < n; p0 += LM_PASS) {
            for (int j = tid; j < len; j += LM_THREADS) {
                const int64_t g = p0 + j;
                float r = 1.0f;
                if (g < n) {
                    const double ev = (double)env[g];
                    if (ev > c) r = (float)(c / ev);
                }
                ra[j] = r;
            }
            __syncthreads();
            float* src = ra;
            float* dst = rb;
            for (int k = 0; k < q; ++k) {
                const int d = 1 << k;
                for (int j = tid; j < len; j += LM_THREADS) dst[j] = j + d < len ? fminf(src[j], src[j + d]) : src[j];
                __syncthreads();
                float* t = src; src = dst; dst = t;
            }
            for (int j = tid; j < LM_PASS; j += LM_THREADS) dst[j] = fminf(src[j], src[j + off]);     // j + off + 2^q - 1 = j + L < len
            __syncthreads();
            const float* h = dst;
            if (p0 == 0) {                                              // the limiter is already down when the row starts
                carry = (double)h[0];
                for (int j = tid; j < L; j += LM_THREADS) eb[LM_PADE(j)] = carry;
            }
            float hr[LM_CHUNK];
#pragma unroll
            for (int i = 0; i < LM_CHUNK; ++i) hr[i] = h[tid * LM_CHUNK + i];
            double e = tid == 0 ? carry : 1.0;
#pragma unroll
            for (int i = 0; i < LM_CHUNK; ++i) e = fmin((double)hr[i], __dadd_rn(__dmul_rn(a, e), oma));
            sc[tid] = 1.0 - e;
            __syncthreads();
            int cur = 0;
#pragma unroll
            for (int k = 0; k < LM_STEPS; ++k) {
                const int d = 1 << k;
                const double* s = sc + cur * LM_THREADS;
                double v = s[tid];
                if (tid >= d) {
                    const double back = pw.m[k] * s[tid - d];
                    v = fmax(v, back > 0.0 ? fmax(back, pw.stall) : 0.0);
                }
                sc[(1 - cur) * LM_THREADS + tid] = v;
                __syncthreads();
                cur = 1 - cur;
            }
            e = tid == 0 ? carry : 1.0 - sc[cur * LM_THREADS + tid - 1];
#pragma unroll
            for (int i = 0; i < LM_CHUNK; ++i) {
                e = fmin((double)hr[i], __dadd_rn(__dmul_rn(a, e), oma));
                eb[LM_PADE(L + tid * LM_CHUNK + i)] = e;
            }
            __syncthreads();
            carry = eb[LM_PADE(L + LM_PASS - 1)];
            const int j0 = tid * LM_CHUNK;                              // e[i - L] of the pass's sample j lies at LM_PADE(j)
            double s = 0.0;
            for (int k = 0; k <= L; ++k) s += eb[LM_PADE(j0 + k)];
            for (int i = 0; i < LM_CHUNK; ++i) {
                if (i > 0) s = (s + eb[LM_PADE(j0 + i + L)]) - eb[LM_PADE(j0 + i - 1)];
                const double sv = s / (double)(L + 1);
                if (p0 + j0 + i < n) {
                    curve[p0 + j0 + i] = (float)sv;
                    mn = fmin(mn, sv);
                }
            }
            __syncthreads();
            for (int j = tid; j < L; j += LM_THREADS) eb[LM_PADE(j)] = eb[LM_PADE(LM_PASS + j)];      // (L <= LM_PASS: the two do not overlap)
            __syncthreads();
        }
        mn = t2m_block_reduce<LM_WAVES>(mn, T2mMin(), redd);
    }
    if (tid == 0) {
        st[0] = (double)mx;
        st[1] = (double)over;
        st[2] = mn;
        st[3] = over == 0 ? (double)mx : 0.0;                           // active: the apply launch's maxima meet here
        st[4] = 1.0;
        st[5] = over > 0 ? 1.0 : 0.0;
        st[6] = 0.0;
        st[7] = 0.0;
    }
}

__global__ __launch_bounds__(256) void lim_trim_kernel(T2Limit p) {
    const int b = blockIdx.y;
    if (!t2m_count_ok(p.n[b], p.n_max)) return;
    const int64_t n = p.n[b];
    double* st = p.stat + (int64_t)b * T2_LIMIT_NSTAT;
    const double c = p.ceiling, pk = st[3];
    const bool trimmed = pk > c;                                        // (row-uniform)
    float t = 1.0f;
    if (trimmed) {                                                      // the largest float32 with (double)t * pk <= c: the product is exact in fp64
        t = (float)(c / pk);
        while ((double)t * pk > c) t = nextafterf(t, 0.0f);
        while ((double)nextafterf(t, 2.0f) * pk <= c) t = nextafterf(t, 2.0f);
    }
    float* y = p.y + (int64_t)b * p.ldy;
    for (int64_t c0 = (int64_t)blockIdx.x * LM_TRIM_CHUNK; c0 < p.ldy; c0 += (int64_t)gridDim.x * LM_TRIM_CHUNK) {
#pragma unroll
        for (int j = 0; j < LM_TRIM_CHUNK / 256; ++j) {
            const int64_t i = c0 + threadIdx.x + j * 256;
            if (i >= p.ldy) break;
            if (i >= n) y[i] = 0.f;
            else if (trimmed) y[i] = y[i] * t;
        }
    }
    if (trimmed && blockIdx.x == 0 && threadIdx.x == 0) {               // (the other blocks read stat[3] alone)
        st[4] = (double)t;
        st[5] = 3.0;                                                    // a trimmed row is active
    }
}

}  // namespace

extern "C" int t2_limit(const T2Limit* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->n && a->table && a->env && a->curve && a->y && a->stat, "t2_limit: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_limit: B outside 1 .. 65535");
    T2_REQUIRE(a->n_max >= 0 && a->ldx >= a->n_max, "t2_limit: n_max < 0 or ldx < n_max");
    T2_REQUIRE(a->x || a->n_max == 0, "t2_limit: null");
    T2_REQUIRE(a->lde >= a->n_max && a->ldc >= a->n_max && a->ldy >= a->n_max, "t2_limit: lde, ldc or ldy < n_max");
    T2_REQUIRE(a->K >= 1 && a->K <= T2_LOUD_MAX_K, "t2_limit: K outside 1 .. 4096");
    T2_REQUIRE(a->L >= 1 && a->L <= T2_LIMIT_MAX_L, "t2_limit: L outside 1 .. 2048");
    T2_REQUIRE(a->a > 0.0 && a->a < 1.0, "t2_limit: a not in (0, 1)");
    T2_REQUIRE(a->ceiling > 0.0 && a->ceiling <= 1.7e308, "t2_limit: ceiling not finite or <= 0");
    LmPow pw;
    double m = a->a;
    for (int k = 0; k < 4; ++k) m *= m;                                  // a^16: one chunk
    for (int k = 0; k < LM_STEPS; ++k) {
        pw.m[k] = m;
        m *= m;
    }
    pw.stall = 0.0;
    const double oma = 1.0 - a->a, ulp = 1.0 / 9007199254740992.0;       // 2^-53: the spacing of fp64 in [0.5, 1)
    if (0.5 / oma < 1048576.0)                                          // (a release of up to 2^21 samples; beyond: no hold)
        for (long k = (long)(0.5 / oma) + 2; k > 0; --k) {
            volatile double e = 1.0 - (double)k * ulp, t = a->a * e;    // (volatile: two roundings, as the kernel's)
            volatile double next = t + oma;
            if (next == e) {
                pw.stall = (double)k * ulp;
                break;
            }
        }
    const size_t lds = lm_curve_lds(a->L), span = (size_t)(2 * LM_TILE + 1 + 2 * a->K) * sizeof(float);
    T2_REQUIRE(t2_allow_lds(lim_curve_kernel, lds), "t2_limit: no LDS for the curve launch");
    const int64_t tiles = ((int64_t)a->n_max + LM_TILE - 1) / LM_TILE;
    if (tiles > 0)
        hipLaunchKernelGGL(lim_peak_kernel<0>, dim3((unsigned)tiles, (unsigned)a->B), dim3(256), span, ST, *a);
    hipLaunchKernelGGL(lim_curve_kernel, dim3((unsigned)a->B), dim3(LM_THREADS), lds, ST, *a, pw);
    if (tiles > 0)
        hipLaunchKernelGGL(lim_peak_kernel<1>, dim3((unsigned)tiles, (unsigned)a->B), dim3(256), span, ST, *a);
    if (a->ldy > 0) {
        int64_t chunks = (a->ldy + LM_TRIM_CHUNK - 1) / LM_TRIM_CHUNK;
        chunks = chunks > 4096 ? 4096 : chunks;
        hipLaunchKernelGGL(lim_trim_kernel, dim3((unsigned)chunks, (unsigned)a->B), dim3(256), 0, ST, *a);
    }
    T2_CHECK_LAUNCH(); return T2_OK;
}
