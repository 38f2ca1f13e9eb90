// Sample-rate conversion of a padded batch of signals (include/tacotron2_amd.h: t2_resample): a polyphase FIR for any
// rational ratio U / D, the table of U phase rows of 2K taps designed by the host (tacotron2_amd/datasets/resample.py).  One launch in
// front of the batched log-mel pass, and behind the vocoder in `say --out-sample-rate`; plain, in the style of t2_prosody.hip: no
// cross-workgroup synchronisation, nothing persistent, no atomics.
//
//   ONE 256-thread workgroup per block of RS_BLOCK = 1024 consecutive outputs of one row; thread t owns the outputs m0 + t + 256 j,
//   j = 0 .. 3 - four independent sums per thread, stores coalesced.  The block's input span, (RS_BLOCK - 1) D / U + 2K + 2 samples at
//   most, is staged in LDS once, with zeros for every sample outside [0, n_in[b]) - those are never loaded.  The table stays in global
//   memory: consecutive outputs walk the phases with stride D mod U, so every lane reads ANOTHER row, all 2K taps of it, and a table of
//   21 to 56 KB (147 x 36, 441 x 32 floats) is an L2 resident that would not fit LDS beside the span for the larger ratios.  With K
//   even and the table 16-byte aligned a lane's taps are dwordx4 loads, else dword loads; the ORDER of the sum is the same - tap
//   -K+1 first, K last, one fmaf each - so both forms, and the unstaged one below, give the same bits.
//   A span above RS_MAX_SPAN floats (a ratio below about 1 / 16, or more than 8190 taps per row) is not staged: the same sum with
//   guarded global loads (resample_kernel<.., false>).
//   m D is formed in 64 bits (ten minutes at 48 kHz with D = 320 pass 2^31); i0 and p of an output are one 64-bit division each.
//   Blocks at or behind n_out[b] only write zeros, up to ldy: the log-mel pass wants each row zero-filled behind its utterance.
#include "t2_measure.hpp"

namespace {

#define RS_THREADS 256
#define RS_PER_THREAD 4
#define RS_BLOCK (RS_THREADS * RS_PER_THREAD)
#define RS_MAX_SPAN 16384          // floats of LDS for one block's input span (64 KB)

template <int VEC, bool STAGED>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(T2Resample p) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * RS_BLOCK;
    const int64_t U = p.U, D = p.D, K = p.K;
    int64_t n = p.n_in[b];
    n = n < 0 ? 0 : n;
    int64_t n_out = (n * U + D - 1) / D;
    n_out = n_out > p.n_out_max ? p.n_out_max : n_out;
    float* y = p.y + (int64_t)b * p.ldy;
    const int64_t m_end = min(m0 + (int64_t)RS_BLOCK, p.ldy);          // outputs of this block: [m0, m_end)
    const int64_t m_live = min(m_end, n_out);                           // ... of which [m0, m_live) are sums, the rest zeros
    if (m_live <= m0) {                                                 // (uniform) behind the utterance: nothing is read
        for (int64_t m = m0 + tid; m < m_end; m += RS_THREADS) y[m] = 0.f;
        return;
    }
    const float* x = p.x + (int64_t)b * p.ldx;
    const int64_t span0 = (m0 * D) / U - K + 1;                         // first input sample any output of the block touches
    if (STAGED) {
        const int64_t span1 = ((m_live - 1) * D) / U + K;               // last one
        const int len = (int)(span1 - span0 + 1);                       // <= RS_MAX_SPAN (host)
        for (int i = tid; i < len; i += RS_THREADS) {
            const int64_t g = span0 + i;
            xs[i] = (g >= 0 && g < n) ? x[g] : 0.f;
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < RS_PER_THREAD; ++j) {
        const int64_t m = m0 + tid + (int64_t)j * RS_THREADS;
        if (m >= m_end) break;
        if (m >= m_live) { y[m] = 0.f; continue; }
        const int64_t md = m * D, i0 = md / U;
        const int ph = (int)(md - i0 * U);
        const float* h = p.table + (int64_t)ph * (2 * K);
        const int64_t first = i0 - K + 1;                               // input sample of tap -K+1
        float acc = 0.f;
        if (STAGED) {
            const float* xr = xs + (first - span0);
            if (VEC == 4) {
                for (int k = 0; k < 2 * (int)K; k += 4) {
                    const f32x4 hv = *reinterpret_cast<const f32x4*>(h + k);
                    acc = fmaf(hv[0], xr[k], acc);
                    acc = fmaf(hv[1], xr[k + 1], acc);
                    acc = fmaf(hv[2], xr[k + 2], acc);
                    acc = fmaf(hv[3], xr[k + 3], acc);
                }
            } else {
                for (int k = 0; k < 2 * (int)K; ++k) acc = fmaf(h[k], xr[k], acc);
            }
        } else {
            for (int k = 0; k < 2 * (int)K; ++k) {
                const int64_t g = first + k;
                const float xv = (g >= 0 && g < n) ? x[g] : 0.f;
                acc = fmaf(h[k], xv, acc);
            }
        }
        y[m] = acc;
    }
}

}  // namespace

extern "C" int t2_resample(const T2Resample* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->x && a->n_in && a->y && a->table, "t2_resample: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_resample: B outside 1 .. 65535");
    T2_REQUIRE(a->U >= 1 && a->D >= 1 && a->K >= 1, "t2_resample: need U, D, K >= 1");
    T2_REQUIRE((int64_t)a->U * 2 * (int64_t)a->K <= ((int64_t)1 << 20), "t2_resample: table of U * 2K floats above 2^20");
    T2_REQUIRE(a->n_out_max >= 0, "t2_resample: n_out_max < 0");
    T2_REQUIRE(a->ldy >= a->n_out_max, "t2_resample: ldy < n_out_max");
    if (a->ldy == 0) return T2_OK;
    const int64_t blocks = (a->ldy + RS_BLOCK - 1) / RS_BLOCK;
    T2_REQUIRE(blocks <= 0x7fffffff, "t2_resample: more than 2^31 - 1 blocks of outputs per row");
    const int64_t span = ((int64_t)(RS_BLOCK - 1) * a->D) / a->U + 2 * (int64_t)a->K + 2;
    const dim3 grid((unsigned)blocks, (unsigned)a->B), block(RS_THREADS);
    if (span > RS_MAX_SPAN)
        hipLaunchKernelGGL((resample_kernel<1, false>), grid, block, 0, ST, *a);
    else if (a->K % 2 == 0 && t2_aligned16(a->table))
        hipLaunchKernelGGL((resample_kernel<4, true>), grid, block, (size_t)span * sizeof(float), ST, *a);
    else
        hipLaunchKernelGGL((resample_kernel<1, true>), grid, block, (size_t)span * sizeof(float), ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
