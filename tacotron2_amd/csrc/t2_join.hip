// Joining a padded batch of synthesised pieces into one waveform (include/tacotron2_amd.h: t2_join): each row is trimmed
// on the ruler the corpus was trimmed on (trim_silence of datasets/tts_dataset.py), levelled, faded at both ends and written behind
// its predecessor with a pause of zeros.  Four launches on one stream, plain, in the style of t2_resample.hip: no cross-workgroup
// synchronisation, nothing persistent, no atomics, every sum in a fixed order.
//
//   energy  one WAVE per frame (4 per workgroup), grid (frames / 4, B): lane l adds x[i]^2 for i = lo + l, lo + l + 64, .. in fp64, the
//           64 partial sums meet in a butterfly.  The heavy launch - every sample is read F / H times - and the only one whose grid
//           grows with the length of a row.  Rows with trim = 0 or n < F, and frames behind n / H, leave at once.
//   span    one 1024-thread workgroup per row: e_max, the first and last active frame (integer minima and maxima), then sumsq and peak
//           over the span.  A row without an active frame (all zeros - or top_db = 0, where no frame is above e_max) is EMPTY; that is
//           not trim_silence's answer for the all-zero signal, whose 1e-10 floors keep it whole.
//   plan    one workgroup: the document's RMS, the gains, the ceiling, the exclusive int64 scan of len + pause.  It also refuses the
//           batch: an n[b] outside 0 .. n_max, a negative pause[b] or a total above cap give total = -1, and the last launch then
//           writes nothing (nothing is clamped; the rows that are out of range are never read).
//   write   grid (chunks, B): y[off + i] = x[s0 + i] * (gain * e) - two float multiplications, nothing to contract - and the zeros of
//           the pause.  A shortened fade (len < 2 fade) samples the SAME table, at (2 i + 1) fade / (2 fl).
#include "t2_measure.hpp"

namespace {

#define JN_FRAME_WAVES 4
#define JN_ROW_THREADS 1024
#define JN_ROW_WAVES (JN_ROW_THREADS / 64)
#define JN_CHUNK 1024              // outputs of one workgroup of the write launch per round

__global__ __launch_bounds__(JN_FRAME_WAVES * 64) void join_energy_kernel(T2Join p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * JN_FRAME_WAVES + (threadIdx.x >> 6);
    const int64_t n = p.n[b];
    if (n < p.F || n > p.n_max || f > n / p.H) return;                  // (n < F: the whole row is kept, no frame is needed)
    int64_t lo = f * p.H - p.F / 2, hi = lo + p.F;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const float* x = p.x + (int64_t)b * p.ldx;
    double acc = 0.0;
    for (int64_t i = lo + lane; i < hi; i += 64) {
        const double v = (double)x[i];
        acc += v * v;
    }
    acc = t2_wave_sum_d(acc);
    if (lane == 0) p.energy[(int64_t)b * p.lde + f] = acc;
}

__global__ __launch_bounds__(JN_ROW_THREADS) void join_span_kernel(T2Join p, double factor) {
    __shared__ double redd[JN_ROW_WAVES];
    __shared__ long long redi[JN_ROW_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t s0 = 0, s1 = 0;
    if (t2m_count_ok(p.n[b], p.n_max)) {
        const int64_t n = p.n[b];
        s1 = n;
        if (p.trim && n >= p.F) {
            const double* e = p.energy + (int64_t)b * p.lde;
            const int64_t nfr = n / p.H + 1;
            double m = 0.0;
            for (int64_t f = tid; f < nfr; f += JN_ROW_THREADS) m = fmax(m, e[f]);
            m = t2m_block_reduce<JN_ROW_WAVES>(m, T2mFmax(), redd);
            const double thr = m * factor;
            long long fa = INT64_MAX, fz = -1;
            for (int64_t f = tid; f < nfr; f += JN_ROW_THREADS)
                if (e[f] > thr) { fa = f < fa ? f : fa; fz = f > fz ? f : fz; }
            fa = t2m_block_reduce<JN_ROW_WAVES>(fa, T2mMin(), redi);
            fz = t2m_block_reduce<JN_ROW_WAVES>(fz, T2mMax(), redi);
            if (!(m > 0.0) || fz < 0) {
                s0 = s1 = 0;
            } else {
                s0 = fa * p.H - p.keep;
                s0 = s0 < 0 ? 0 : s0;
                s1 = (fz + 1) * p.H + p.keep;
                s1 = s1 > n ? n : s1;
            }
        }
    }
    const float* x = p.x + (int64_t)b * p.ldx;
    double ss = 0.0, pk = 0.0;
    for (int64_t i = s0 + tid; i < s1; i += JN_ROW_THREADS) {
        const float xv = x[i];
        const double v = (double)xv;
        ss += v * v;
        pk = fmax(pk, fabs(v));
    }
    ss = t2m_block_reduce<JN_ROW_WAVES>(ss, T2mSum(), redd);
    pk = t2m_block_reduce<JN_ROW_WAVES>(pk, T2mFmax(), redd);
    if (tid == 0) {
        p.s0[b] = (int32_t)s0;
        p.len[b] = (int32_t)(s1 - s0);
        p.stat[2 * (int64_t)b] = ss;
        p.stat[2 * (int64_t)b + 1] = pk;
    }
}

__device__ __forceinline__ double jn_gain(const T2Join& p, int b, double rms_doc) {
    const int len = p.len[b];
    const double rms = len > 0 ? sqrt(p.stat[2 * (int64_t)b] / (double)len) : 0.0;
    if (!p.level || !(rms > 0.0)) return 1.0;
    const double g = rms_doc / rms, lo = 1.0 / p.max_gain;
    return g < lo ? lo : g > p.max_gain ? p.max_gain : g;
}

__global__ __launch_bounds__(JN_ROW_THREADS) void join_plan_kernel(T2Join p) {
    __shared__ double redd[JN_ROW_WAVES];
    __shared__ long long redi[JN_ROW_WAVES];
    __shared__ long long sc[2][JN_ROW_THREADS];
    const int tid = threadIdx.x, B = p.B;
    double S = 0.0;
    long long L = 0, bad = 0;
    for (int b = tid; b < B; b += JN_ROW_THREADS) {
        if (!t2m_count_ok(p.n[b], p.n_max) || p.pause[b] < 0) bad = 1;
        S += p.stat[2 * (int64_t)b];
        L += p.len[b];
    }
    S = t2m_block_reduce<JN_ROW_WAVES>(S, T2mSum(), redd);
    L = t2m_block_reduce<JN_ROW_WAVES>(L, T2mSum(), redi);
    bad = t2m_block_reduce<JN_ROW_WAVES>(bad, T2mMax(), redi);
    const double rms_doc = L > 0 ? sqrt(S / (double)L) : 0.0;
    double pk = 0.0;
    for (int b = tid; b < B; b += JN_ROW_THREADS) pk = fmax(pk, jn_gain(p, b, rms_doc) * p.stat[2 * (int64_t)b + 1]);
    pk = t2m_block_reduce<JN_ROW_WAVES>(pk, T2mFmax(), redd);
    const bool limit = p.ceiling > 0.0 && pk > p.ceiling;
    const double scale = limit ? p.ceiling / pk : 1.0;
    for (int b = tid; b < B; b += JN_ROW_THREADS) {
        const double g = jn_gain(p, b, rms_doc);
        p.gain[b] = (float)(limit ? g * scale : g);
    }
    // the exclusive scan of len + pause: thread t owns `per` consecutive rows, their sums meet in a Hillis-Steele scan (integers: any
    // order gives these bits)
    const int per = (B + JN_ROW_THREADS - 1) / JN_ROW_THREADS;
    const int b0 = min(tid * per, B), b1 = min(b0 + per, B);
    long long mine = 0;
    if (!bad)
        for (int b = b0; b < b1; ++b) mine += (long long)p.len[b] + p.pause[b];
    sc[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < JN_ROW_THREADS; d <<= 1) {
        sc[1 - cur][tid] = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
        __syncthreads();
        cur = 1 - cur;
    }
    long long off = sc[cur][tid] - mine;
    const long long total = sc[cur][JN_ROW_THREADS - 1];
    const bool refuse = bad || total > p.cap;
    for (int b = b0; b < b1; ++b) {
        p.off[b] = refuse ? 0 : off;
        if (!refuse) off += (long long)p.len[b] + p.pause[b];
    }
    if (tid == 0) p.total[0] = refuse ? -1 : total;
}

__global__ __launch_bounds__(256) void join_write_kernel(T2Join p) {
    if (p.total[0] < 0) return;
    const int b = blockIdx.y;
    const int64_t len = p.len[b], seg = len + p.pause[b], off = p.off[b];
    const int64_t fl = min((int64_t)p.fade, len / 2);
    const float gain = p.gain[b];
    const float* x = p.x + (int64_t)b * p.ldx + p.s0[b];
    float* y = p.y + off;
    for (int64_t c = (int64_t)blockIdx.x * JN_CHUNK; c < seg; c += (int64_t)gridDim.x * JN_CHUNK) {
#pragma unroll
        for (int j = 0; j < JN_CHUNK / 256; ++j) {
            const int64_t i = c + threadIdx.x + j * 256;
            if (i >= seg || off + i >= p.cap) break;
            if (i >= len) { y[i] = 0.f; continue; }
            float e = 1.0f;
            if (i < fl) e = p.w[((2 * i + 1) * p.fade) / (2 * fl)];
            else if (i >= len - fl) e = p.w[((2 * (len - 1 - i) + 1) * p.fade) / (2 * fl)];
            const float ge = gain * e;
            y[i] = x[i] * ge;
        }
    }
}

}  // namespace

extern "C" int t2_join(const T2Join* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->n && a->pause && a->stat && a->off && a->s0 && a->len && a->gain && a->total, "t2_join: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_join: B outside 1 .. 65535");
    T2_REQUIRE((a->trim == 0 || a->trim == 1) && (a->level == 0 || a->level == 1), "t2_join: trim and level are flags, 0 or 1");
    T2_REQUIRE(a->F >= 2 && a->F % 2 == 0, "t2_join: F < 2 or odd");
    T2_REQUIRE(a->H >= 1, "t2_join: H < 1");
    T2_REQUIRE(a->keep >= 0, "t2_join: keep < 0");
    T2_REQUIRE(a->fade >= 0, "t2_join: fade < 0");
    T2_REQUIRE(a->top_db >= 0.0 && a->top_db <= 1.7e308, "t2_join: top_db negative or not finite");
    T2_REQUIRE(a->max_gain >= 1.0 && a->max_gain <= 1.7e308, "t2_join: max_gain < 1 or not finite");
    T2_REQUIRE(a->ceiling >= 0.0 && a->ceiling <= 1.7e308, "t2_join: ceiling negative or not finite");
    T2_REQUIRE(a->n_max >= 0 && a->ldx >= a->n_max, "t2_join: n_max < 0 or ldx < n_max");
    T2_REQUIRE(a->cap >= 0, "t2_join: cap < 0");
    T2_REQUIRE((a->x || a->n_max == 0) && (a->y || a->cap == 0) && (a->w || a->fade == 0), "t2_join: null");
    T2_REQUIRE(!a->trim || (a->energy && a->lde >= (int64_t)a->n_max / a->H + 1), "t2_join: energy null or lde < n_max / H + 1");
    const double factor = pow(10.0, -a->top_db / 10.0);
    if (a->trim && a->n_max >= a->F) {
        const int64_t blocks = ((int64_t)a->n_max / a->H + 1 + JN_FRAME_WAVES - 1) / JN_FRAME_WAVES;
        hipLaunchKernelGGL(join_energy_kernel, dim3((unsigned)blocks, (unsigned)a->B), dim3(JN_FRAME_WAVES * 64), 0, ST, *a);
    }
    hipLaunchKernelGGL(join_span_kernel, dim3((unsigned)a->B), dim3(JN_ROW_THREADS), 0, ST, *a, factor);
    hipLaunchKernelGGL(join_plan_kernel, dim3(1), dim3(JN_ROW_THREADS), 0, ST, *a);
    if (a->cap > 0) {
        int64_t chunks = ((int64_t)a->n_max + JN_CHUNK - 1) / JN_CHUNK;
        chunks = chunks < 1 ? 1 : chunks > 4096 ? 4096 : chunks;
        hipLaunchKernelGGL(join_write_kernel, dim3((unsigned)chunks, (unsigned)a->B), dim3(256), 0, ST, *a);
    }
    T2_CHECK_LAUNCH(); return T2_OK;
}
