// Programme loudness, true peak and loudness normalisation of a padded batch of waveforms (include/tacotron2_amd.h: t2_loudness;
// DESIGN 5.20; restated in float64 in tests/loudness_ref.py): ITU-R BS.1770-4 for one channel.  Four launches on one stream, plain,
// in the style of t2_join.hip: no cross-workgroup synchronisation, nothing persistent, every sum in a fixed order; the one atomic is an
// integer maximum, which has no order.
//
//   filter  one 256-thread workgroup per row.  The K-weighting is a recurrence along the signal, so a PASS of 8192 samples is cut into
//           256 chunks of 32: thread t filters chunk t through both sections in fp64 from a zero state (thread 0 from the state the
//           pass before left) and publishes its 4 end states.  The cascade without input is linear in those 4 numbers, s' = T s, so the
//           true state behind chunk t is S_t = z_t + T^32 S_{t-1}: an inclusive Hillis-Steele scan of 8 steps, step k adding
//           T^(32 2^k) times the value 2^k chunks back.  The 8 matrices are formed by the entry, in fp64, from the coefficients.
//           Every thread then filters its chunk AGAIN, from S_{t-1}, and leaves y^2 in LDS; one wave per hop adds a hop's stretch of
//           the pass (lane l takes the samples l, l + 64, .., the 64 partial sums meet in a butterfly).  A hop that is cut by the
//           end of a pass carries its partial sum into the next; the last, partial hop of a row is kept for a short row's one block.
//           Filtering twice costs 2 x 32 dependent steps per thread and pass and needs no table of homogeneous responses; what the
//           second run computes IS the sequential recurrence from a carried state.
//           LDS: x 256 x 33 floats (33: a thread's chunk starts on its own bank), y^2 256 x 33 doubles, the scan's two buffers of
//           256 x 4 doubles: 117 760 bytes, dynamic, one workgroup per CU.
//   peak    grid (tiles of 1024 input samples, B), 256 threads: the tile's span, 1023 + 2K floats, staged in LDS with zeros outside
//           [0, n) as t2_resample stages it; a thread forms the 4 phases of 4 samples, each sum t2_resample's - one fmaf per tap in
//           ascending k from 0.0f -, and keeps the largest magnitudes.  The tile's maxima reach stat through atomicMax on the bits of
//           the value as a double: for non-negative numbers the integer order is the numeric one, so any arrival order gives the
//           same bits.  (The filter launch, which comes first on the stream, zeroes the two slots.)
//   gate    one 256-thread workgroup per row over E: the blocks, the two gates, the loudness, the gain.
//   scale   grid (chunks, B): y = x * gain, zeros behind n.  Only with y != NULL.
#include <math.h>
#include "t2_measure.hpp"

namespace {

#define LD_THREADS 256
#define LD_WAVES (LD_THREADS / 64)
#define LD_CHUNK 32
#define LD_PASS (LD_THREADS * LD_CHUNK)
#define LD_STEPS 8                 // log2(LD_THREADS)
#define LD_PAD(j) ((j) + ((j) >> 5))
#define LD_ROWS (LD_THREADS * (LD_CHUNK + 1))
#define LD_FILTER_LDS (LD_ROWS * sizeof(double) + 2 * LD_THREADS * 4 * sizeof(double) + LD_ROWS * sizeof(float))
#define LP_TILE 1024
#define LS_CHUNK 1024

struct LdTrans { double m[LD_STEPS][16]; };     // m[k] = T^(32 * 2^k), row-major, over the state (s1, s2 of the shelf, s1, s2 of the high-pass)

struct LdCoef { double b10, b11, b12, a11, a12, b20, b21, b22, a21, a22; };

// one sample through both sections (the header's rule); s = (s1, s2 of the shelf, s1, s2 of the high-pass)
__device__ __forceinline__ double ld_step(const LdCoef& c, double (&s)[4], double u) {
    const double v = c.b10 * u + s[0];
    s[0] = c.b11 * u - c.a11 * v + s[1];
    s[1] = c.b12 * u - c.a12 * v;
    const double w = c.b20 * v + s[2];
    s[2] = c.b21 * v - c.a21 * w + s[3];
    s[3] = c.b22 * v - c.a22 * w;
    return w;
}

__global__ __launch_bounds__(LD_THREADS) void loud_filter_kernel(T2Loudness p, LdTrans tr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ld_smem[];
    double* ysq = reinterpret_cast<double*>(ld_smem);                   // [LD_ROWS]
    double* sc = ysq + LD_ROWS;                                         // [2][LD_THREADS][4]
    float* xs = reinterpret_cast<float*>(sc + 2 * LD_THREADS * 4);      // [LD_ROWS]
    __shared__ double open[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!t2m_count_ok(p.n[b], p.n_max)) return;
    const int64_t n = p.n[b], H = p.H;
    const float* x = p.x + (int64_t)b * p.ldx;
    double* E = p.E + (int64_t)b * p.lde;
    double* st = p.stat + (int64_t)b * T2_LOUD_NSTAT;
    const LdCoef c = {p.b1[0], p.b1[1], p.b1[2], p.a1[1], p.a1[2], p.b2[0], p.b2[1], p.b2[2], p.a2[1], p.a2[2]};
    double carry[4] = {0.0, 0.0, 0.0, 0.0};                             // the state in front of the pass: the same in every thread
    int par = 0;
    for (int64_t p0 = 0; p0 < n; p0 += LD_PASS, par ^= 1) {
        const int64_t p1 = min(p0 + (int64_t)LD_PASS, n);
        for (int j = tid; j < LD_PASS; j += LD_THREADS) {
            const int64_t g = p0 + j;
            xs[LD_PAD(j)] = g < n ? x[g] : 0.f;
        }
        __syncthreads();
        float xr[LD_CHUNK];
#pragma unroll
        for (int i = 0; i < LD_CHUNK; ++i) xr[i] = xs[tid * (LD_CHUNK + 1) + i];
        double s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = tid == 0 ? carry[q] : 0.0;
#pragma unroll
        for (int i = 0; i < LD_CHUNK; ++i) (void)ld_step(c, s, (double)xr[i]);
#pragma unroll
        for (int q = 0; q < 4; ++q) sc[tid * 4 + q] = s[q];
        __syncthreads();
        int cur = 0;
#pragma unroll
        for (int k = 0; k < LD_STEPS; ++k) {
            const int d = 1 << k;
            const double* src = sc + cur * (LD_THREADS * 4);
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = src[tid * 4 + q];
            if (tid >= d) {
                const double* u = src + (tid - d) * 4;
                const double u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    v[q] += ((tr.m[k][4 * q] * u0 + tr.m[k][4 * q + 1] * u1) + tr.m[k][4 * q + 2] * u2) + tr.m[k][4 * q + 3] * u3;
            }
            double* dst = sc + (1 - cur) * (LD_THREADS * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[tid * 4 + q] = v[q];
            __syncthreads();
            cur = 1 - cur;
        }
        const double* fin = sc + cur * (LD_THREADS * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = tid == 0 ? carry[q] : fin[max(tid - 1, 0) * 4 + q];
#pragma unroll
        for (int q = 0; q < 4; ++q) carry[q] = fin[(LD_THREADS - 1) * 4 + q];
#pragma unroll
        for (int i = 0; i < LD_CHUNK; ++i) {
            const double w = ld_step(c, s, (double)xr[i]);
            ysq[tid * (LD_CHUNK + 1) + i] = w * w;
        }
        __syncthreads();
        for (int64_t h = p0 / H + wave; h <= (p1 - 1) / H; h += LD_THREADS / 64) {
            const int64_t lo = max(h * H, p0), hi = min((h + 1) * H, p1);
            double acc = 0.0;
            for (int64_t i = lo + lane; i < hi; i += 64) {
                const int j = (int)(i - p0);
                acc += ysq[LD_PAD(j)];
            }
            acc = t2_wave_sum_d(acc);
            if (lane == 0) {
                const double v = lo == h * H ? acc : open[par ^ 1] + acc;      // (a hop cut by the pass before: its part comes first)
                if (hi == (h + 1) * H) E[h] = v;
                else open[par] = v;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        st[0] = (n > 0 && n % H != 0) ? open[par ^ 1] : 0.0;           // the partial hop behind the last whole one: the gate launch reads it
        st[2] = 0.0;
        st[3] = 0.0;
    }
}

__global__ __launch_bounds__(256) void loud_peak_kernel(T2Loudness p) {
    extern __shared__ __attribute__((aligned(16))) float lp_xs[];
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (!t2m_count_ok(p.n[b], p.n_max)) return;
    const int64_t n = p.n[b], tile0 = (int64_t)blockIdx.x * LP_TILE;
    if (tile0 >= n) return;                                             // (uniform) behind the row: nothing is read
    const int K = p.K;
    const float* x = p.x + (int64_t)b * p.ldx;
    const int64_t span0 = tile0 - K + 1;
    for (int i = tid; i < LP_TILE - 1 + 2 * K; i += 256) {
        const int64_t g = span0 + i;
        lp_xs[i] = (g >= 0 && g < n) ? x[g] : 0.f;
    }
    __syncthreads();
    float tp = 0.f, sp = 0.f;
#pragma unroll
    for (int j = 0; j < LP_TILE / 256; ++j) {
        const int o = tid + j * 256;
        if (tile0 + o >= n) break;
        const float* xr = lp_xs + o;                                    // the sample of tap -K+1
        sp = fmaxf(sp, fabsf(xr[K - 1]));
        tp = fmaxf(tp, t2m_peak4(p.table, K, xr));
    }
    tp = t2_block_max(tp, red);
    sp = t2_block_max(sp, red);
    if (tid == 0) {
        unsigned long long* st = reinterpret_cast<unsigned long long*>(p.stat + (int64_t)b * T2_LOUD_NSTAT);
        atomicMax(st + 2, (unsigned long long)__double_as_longlong((double)tp));
        atomicMax(st + 3, (unsigned long long)__double_as_longlong((double)sp));
    }
}

__global__ __launch_bounds__(LD_THREADS) void loud_gate_kernel(T2Loudness p) {
    __shared__ double redd[LD_WAVES];
    __shared__ long long redi[LD_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    double* st = p.stat + (int64_t)b * T2_LOUD_NSTAT;
    if (!t2m_count_ok(p.n[b], p.n_max)) {
        if (tid == 0) st[9] = -1.0;
        return;
    }
    const int64_t n = p.n[b], H = p.H, N = 4 * H;
    const double* E = p.E + (int64_t)b * p.lde;
    const bool is_short = n > 0 && n < N;
    const int64_t J = n >= N ? n / H - 3 : (n > 0 ? 1 : 0);
    const double tail = st[0];                                          // (read by all in front of the first barrier; written behind the last)
    auto z = [&](int64_t j) -> double {
        if (is_short) {
            double s = 0.0;
            for (int64_t h = 0; h < n / H; ++h) s += E[h];
            return (s + tail) / (double)n;
        }
        return (((E[j] + E[j + 1]) + E[j + 2]) + E[j + 3]) / (double)N;
    };
    double sum_a = 0.0, zmax = 0.0;
    long long cnt_a = 0;
    for (int64_t j = tid; j < J; j += LD_THREADS) {
        const double zj = z(j);
        zmax = fmax(zmax, zj);
        if (zj > p.abs_gate) { sum_a += zj; ++cnt_a; }
    }
    sum_a = t2m_block_reduce<LD_WAVES>(sum_a, T2mSum(), redd);
    cnt_a = t2m_block_reduce<LD_WAVES>(cnt_a, T2mSum(), redi);
    zmax = t2m_block_reduce<LD_WAVES>(zmax, T2mFmax(), redd);
    const double nan = __builtin_nan("");
    double lufs = nan, rel_lufs = nan, g = 1.0;
    long long cnt_r = 0;
    unsigned flags = is_short ? 1u : 0u;
    if (cnt_a == 0) {
        flags |= 2u;
    } else {                                                            // (uniform: every thread holds the same cnt_a)
        const double thr = 0.1 * (sum_a / (double)cnt_a);
        double sum_r = 0.0;
        for (int64_t j = tid; j < J; j += LD_THREADS) {
            const double zj = z(j);
            if (zj > p.abs_gate && zj > thr) { sum_r += zj; ++cnt_r; }
        }
        sum_r = t2m_block_reduce<LD_WAVES>(sum_r, T2mSum(), redd);
        cnt_r = t2m_block_reduce<LD_WAVES>(cnt_r, T2mSum(), redi);
        lufs = -0.691 + 10.0 * log10(sum_r / (double)cnt_r);            // (cnt_r >= 1: the largest block is above a tenth of the mean)
        rel_lufs = -0.691 + 10.0 * log10(thr);
        if (p.y) {
            g = pow(10.0, (p.target - lufs) / 20.0);
            if (g > p.max_gain) { g = p.max_gain; flags |= 8u; }
            if (g * st[2] > p.ceiling) { g = p.ceiling / st[2]; flags |= 4u; }
        }
    }
    if (tid == 0) {
        st[0] = lufs;
        st[1] = g;
        st[4] = (double)J;
        st[5] = (double)(J - cnt_a);
        st[6] = (double)(cnt_a - cnt_r);
        st[7] = rel_lufs;
        st[8] = J > 0 ? -0.691 + 10.0 * log10(zmax) : nan;
        st[9] = (double)flags;
        p.gain[b] = (float)g;
    }
}

__global__ __launch_bounds__(256) void loud_scale_kernel(T2Loudness p) {
    const int b = blockIdx.y;
    if (!t2m_count_ok(p.n[b], p.n_max)) return;
    const int64_t n = p.n[b];
    const float gain = p.gain[b];
    const float* x = p.x + (int64_t)b * p.ldx;
    float* y = p.y + (int64_t)b * p.ldy;
    for (int64_t c = (int64_t)blockIdx.x * LS_CHUNK; c < p.ldy; c += (int64_t)gridDim.x * LS_CHUNK) {
#pragma unroll
        for (int j = 0; j < LS_CHUNK / 256; ++j) {
            const int64_t i = c + threadIdx.x + j * 256;
            if (i >= p.ldy) break;
            y[i] = i < n ? x[i] * gain : 0.f;
        }
    }
}

void ld_matmul(const double* a, const double* b, double* out) {
    double t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            t[4 * i + j] = s;
        }
    memcpy(out, t, sizeof(t));
}

bool ld_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!(fabs(v[i]) <= 1.7e308)) return false;
    return true;
}

}  // namespace

extern "C" int t2_loudness(const T2Loudness* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->n && a->table && a->E && a->stat && a->gain, "t2_loudness: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_loudness: B outside 1 .. 65535");
    T2_REQUIRE(a->n_max >= 0 && a->ldx >= a->n_max, "t2_loudness: n_max < 0 or ldx < n_max");
    T2_REQUIRE(a->x || a->n_max == 0, "t2_loudness: null");
    T2_REQUIRE(a->H >= 1, "t2_loudness: H < 1");
    T2_REQUIRE(a->lde >= (int64_t)a->n_max / a->H, "t2_loudness: lde < n_max / H");
    T2_REQUIRE(a->K >= 1 && a->K <= T2_LOUD_MAX_K, "t2_loudness: K outside 1 .. 4096");
    T2_REQUIRE(!a->y || a->ldy >= a->n_max, "t2_loudness: ldy < n_max");
    T2_REQUIRE(ld_finite(a->b1, 3) && ld_finite(a->a1, 3) && ld_finite(a->b2, 3) && ld_finite(a->a2, 3),
               "t2_loudness: a coefficient that is not finite");
    T2_REQUIRE(ld_finite(&a->abs_gate, 1) && ld_finite(&a->target, 1), "t2_loudness: abs_gate or target not finite");
    T2_REQUIRE(a->max_gain > 0.0 && a->max_gain <= 1.7e308 && a->ceiling > 0.0 && a->ceiling <= 1.7e308,
               "t2_loudness: max_gain or ceiling not finite or <= 0");
    // the cascade without input, one sample: s' = T s over (s1, s2 of the shelf, s1, s2 of the high-pass)
    const double T[16] = {-a->a1[1], 1.0, 0.0, 0.0,
                          -a->a1[2], 0.0, 0.0, 0.0,
                          a->b2[1] - a->a2[1] * a->b2[0], 0.0, -a->a2[1], 1.0,
                          a->b2[2] - a->a2[2] * a->b2[0], 0.0, -a->a2[2], 0.0};
    LdTrans tr;
    double m[16];
    memcpy(m, T, sizeof(m));
    for (int k = 0; k < 5; ++k) ld_matmul(m, m, m);                      // T^32: one chunk
    for (int k = 0; k < LD_STEPS; ++k) {
        memcpy(tr.m[k], m, sizeof(m));
        ld_matmul(m, m, m);
    }
    T2_REQUIRE(ld_finite(&tr.m[0][0], LD_STEPS * 16), "t2_loudness: an unstable filter (its chunk transition is not finite)");
    T2_REQUIRE(t2_allow_lds(loud_filter_kernel, LD_FILTER_LDS), "t2_loudness: no 115 KB of LDS for the filter launch");
    hipLaunchKernelGGL(loud_filter_kernel, dim3((unsigned)a->B), dim3(LD_THREADS), LD_FILTER_LDS, ST, *a, tr);
    if (a->n_max > 0) {
        const int64_t tiles = ((int64_t)a->n_max + LP_TILE - 1) / LP_TILE;
        hipLaunchKernelGGL(loud_peak_kernel, dim3((unsigned)tiles, (unsigned)a->B), dim3(256),
                           (size_t)(LP_TILE - 1 + 2 * a->K) * sizeof(float), ST, *a);
    }
    hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)a->B), dim3(LD_THREADS), 0, ST, *a);
    if (a->y && a->ldy > 0) {
        int64_t chunks = (a->ldy + LS_CHUNK - 1) / LS_CHUNK;
        chunks = chunks > 4096 ? 4096 : chunks;
        hipLaunchKernelGGL(loud_scale_kernel, dim3((unsigned)chunks, (unsigned)a->B), dim3(256), 0, ST, *a);
    }
    T2_CHECK_LAUNCH(); return T2_OK;
}
