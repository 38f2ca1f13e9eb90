// Spectral subtraction of a stationary bias spectrum from a padded batch of waveforms (include/tacotron2_amd.h: t2_denoise; DESIGN
// 5.22; restated in float64 in tests/denoise_ref.py).  ONE launch, plain, in the style of t2_limit.hip: no cross-workgroup
// synchronisation, nothing persistent, every float sum in a fixed order; the two atomics add integers, which have no order.
//
//   grid (tiles of DN_G = 16 hops = 4096 samples, B), 256 threads.  A workgroup stages the 4096 + 2 * 768 samples its frames touch in
//   LDS, reflected at the row's OWN ends (never a sample at or behind n[b]), runs the frames g0 - 1 .. g0 + 17 that reach its tile one
//   after another - window, forward FFT, gate, inverse FFT, window, add into the LDS output tile: ascending t -, divides by the
//   envelope of the frames that exist and writes its samples once.  The three halo frames are computed again by the neighbouring
//   tile; no frame and no spectrum goes to global memory unless `mag` is asked for.  A frame is counted, and its `mag` row written,
//   by its OWNER alone: the tile with g0 <= t < g0 + 16.
//   The transform: 1024 = 4^5, a radix-4 Stockham autosort FFT of five passes between two complex buffers in LDS (separate re / im
//   planes), one butterfly per thread and pass, twiddles from the host-made table.  Pass k (s = 4^k) reads the elements tid + 256 m
//   and writes q + s (4 p + m), q = tid mod s, p = tid div s: a power-of-two stride in every pass.  Element i lies at
//   DN_SW(i) = i ^ ((i >> 2) & 31): with ds_read_b32 / ds_write_b32 banked (a / 4) mod 32 per 32-lane half, every read and every
//   write of all five passes is conflict-free (plain layout: up to 4-way on the strided writes) and the buffer stays 1024 floats.
//   The real frame rides in the real plane with a zero imaginary plane.
//   LDS, dynamic: span 5632 + out 4096 + window 1024 + twiddles 768 x 2 + two complex buffers 4 x 1024 = 16 384 floats = 64 KB: two
//   workgroups per CU.
//   Element j = tid + 256 m of a frame, and every output sample with o mod 256 == tid, belong to thread tid from the staging of the
//   frame to the last division: the overlap-add needs no barrier of its own.
#include <math.h>
#include "t2_measure.hpp"

namespace {

#define DN_N T2_DENOISE_NFFT
#define DN_HOP T2_DENOISE_HOP
#define DN_G 16
#define DN_TILE (DN_G * DN_HOP)
#define DN_HALO (DN_N / 2 + DN_HOP)
#define DN_SPAN (DN_TILE + 2 * DN_HALO)
#define DN_BINS (DN_N / 2 + 1)
#define DN_TW 768                                   // twiddle indices reach 3 * 255
#define DN_SW(i) ((i) ^ (((i) >> 2) & 31))
#define DN_LDS ((DN_SPAN + DN_TILE + DN_N + 2 * DN_TW + 4 * DN_N) * sizeof(float))

static_assert(DN_N == 1024 && DN_HOP == 256, "five radix-4 passes of 256 butterflies; four frames over a sample");

// x -> y, five passes; the result lies in (yr, yi).  INV: the conjugate twiddles, unnormalised.  Ends behind a barrier.
template <int INV>
__device__ __forceinline__ void dn_fft(float* xr, float* xi, float* yr, float* yi, const float* tw, int tid) {
#pragma unroll
    for (int pass = 0; pass < 5; ++pass) {
        const int ls = 2 * pass, s = 1 << ls, q = tid & (s - 1), p = tid >> ls, e = p << ls;
        const float ar = xr[DN_SW(tid)], ai = xi[DN_SW(tid)], br = xr[DN_SW(tid + 256)], bi = xi[DN_SW(tid + 256)];
        const float cr = xr[DN_SW(tid + 512)], ci = xi[DN_SW(tid + 512)], dr = xr[DN_SW(tid + 768)], di = xi[DN_SW(tid + 768)];
        const float apcr = ar + cr, apci = ai + ci, amcr = ar - cr, amci = ai - ci;
        const float bpdr = br + dr, bpdi = bi + di, bmdr = br - dr, bmdi = bi - di;
        // j (b - d) = (-bmdi, bmdr); forward: y1 = w1 (amc - j bmd), y3 = w3 (amc + j bmd); inverse: the two swapped
        const float sg = INV ? -1.f : 1.f;
        const float u1r = amcr + sg * bmdi, u1i = amci - sg * bmdr, u3r = amcr - sg * bmdi, u3i = amci + sg * bmdr;
        const float u2r = apcr - bpdr, u2i = apci - bpdi;
        const float w1r = tw[2 * e], w1i = -sg * tw[2 * e + 1], w2r = tw[4 * e], w2i = -sg * tw[4 * e + 1];
        const float w3r = tw[6 * e], w3i = -sg * tw[6 * e + 1];
        const int o = q + (p << (ls + 2));
        yr[DN_SW(o)] = apcr + bpdr;
        yi[DN_SW(o)] = apci + bpdi;
        yr[DN_SW(o + s)] = u1r * w1r - u1i * w1i;
        yi[DN_SW(o + s)] = u1r * w1i + u1i * w1r;
        yr[DN_SW(o + 2 * s)] = u2r * w2r - u2i * w2i;
        yi[DN_SW(o + 2 * s)] = u2r * w2i + u2i * w2r;
        yr[DN_SW(o + 3 * s)] = u3r * w3r - u3i * w3i;
        yi[DN_SW(o + 3 * s)] = u3r * w3i + u3i * w3r;
        __syncthreads();
        float* t = xr; xr = yr; yr = t;
        t = xi; xi = yi; yi = t;
    }
}

__global__ __launch_bounds__(256) void denoise_kernel(T2Denoise p) {
    extern __shared__ __attribute__((aligned(16))) float dn_smem[];
    float* span = dn_smem;                          // [DN_SPAN] the samples tile0 - 768 .. tile0 + 4096 + 768, reflected
    float* out = span + DN_SPAN;                    // [DN_TILE]
    float* win = out + DN_TILE;                     // [DN_N]
    float* tw = win + DN_N;                         // [DN_TW][2]
    float* ar = tw + 2 * DN_TW;                     // two complex buffers, DN_SW layout
    float* ai = ar + DN_N;
    float* br = ai + DN_N;
    float* bi = br + DN_N;
    const int b = blockIdx.y, tid = threadIdx.x;
    double* st = p.stat + (int64_t)b * T2_DENOISE_NSTAT;
    if (!t2m_count_ok(p.n[b], p.n_max)) {
        if (blockIdx.x == 0 && tid == 0) st[2] = -1.0;
        return;
    }
    const int n = p.n[b], g0 = (int)blockIdx.x * DN_G;
    const int64_t tile0 = (int64_t)blockIdx.x * DN_TILE;
    const bool is_short = n <= DN_N / 2;                                // no reflection at this length: a copy
    const int F = is_short ? 0 : 1 + n / DN_HOP;
    if (blockIdx.x == 0 && tid == 0) {
        st[0] = (double)F;
        st[2] = is_short ? 1.0 : 0.0;
    }
    const float* x = p.x + (int64_t)b * p.ldx;
    float* y = p.y ? p.y + (int64_t)b * p.ldy : nullptr;
    int t_lo = g0 > 0 ? g0 - 1 : 0, t_hi = g0 + DN_G + 1 < F - 1 ? g0 + DN_G + 1 : F - 1;
    if (tile0 >= n || !y) {                                             // no sample of the row here: the frames this tile owns alone
        t_lo = g0;
        t_hi = g0 + DN_G - 1 < F - 1 ? g0 + DN_G - 1 : F - 1;
    }
    if (t_lo > t_hi) {                                                  // (uniform) a short row, or a tile behind the row's last frame
        if (y)
            for (int o = tid; o < DN_TILE && tile0 + o < p.ldy; o += 256) y[tile0 + o] = tile0 + o < n ? x[tile0 + o] : 0.f;
        return;
    }
    for (int i = tid; i < DN_N; i += 256) win[i] = p.win[i];
    for (int i = tid; i < 2 * DN_TW; i += 256) tw[i] = p.tw[i];
    for (int i = tid; i < DN_SPAN; i += 256) {
        const int64_t g = tile0 - DN_HALO + i;
        float v = 0.f;
        if (g >= -(DN_N / 2) && g < (int64_t)n + DN_N / 2)              // n > 512: both reflections land inside [0, n)
            v = x[g < 0 ? -g : g >= n ? 2 * ((int64_t)n - 1) - g : g];
        span[i] = v;
    }
    for (int o = tid; o < DN_TILE; o += 256) out[o] = 0.f;
    __syncthreads();
    int cnt = 0;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int off = (t - g0 + 1) * DN_HOP;                          // the frame's first sample in span
        const bool owned = t >= g0 && t < g0 + DN_G;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int j = tid + 256 * m;
            ar[DN_SW(j)] = span[off + j] * win[j];
            ai[DN_SW(j)] = 0.f;
        }
        __syncthreads();
        dn_fft<0>(ar, ai, br, bi, tw, tid);
        float* mrow = owned && p.mag ? p.mag + ((int64_t)b * p.f_max + t) * p.ldm : nullptr;
        for (int k = tid; k < DN_BINS; k += 256) {                      // thread 0 also takes the bin 512
            const float re = br[DN_SW(k)], im = bi[DN_SW(k)];
            const float m = sqrtf(__fmaf_rn(re, re, __fmul_rn(im, im)));
            if (mrow) mrow[k] = m;
            if (y) {
                const float thr = __fmul_rn(p.strength, p.bias[k]);
                const float g = m > thr ? __fdiv_rn(m - thr, m) : 0.f;
                if (owned && g == 0.f) ++cnt;
                br[DN_SW(k)] = re * g;
                bi[DN_SW(k)] = im * g;
                if (k > 0 && k < DN_N / 2) {                            // the mirror bin: the real part of the inverse is the real inverse
                    br[DN_SW(DN_N - k)] *= g;
                    bi[DN_SW(DN_N - k)] *= g;
                }
            }
        }
        __syncthreads();
        if (!y) continue;
        dn_fft<1>(br, bi, ar, ai, tw, tid);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int j = tid + 256 * m, o = (t - g0) * DN_HOP - DN_N / 2 + j;
            if (o >= 0 && o < DN_TILE) out[o] += __fmul_rn(__fmul_rn(ar[DN_SW(j)], 1.0f / DN_N), win[j]);
        }
    }
    if (y) {
        cnt = t2m_wave_reduce(cnt, T2mSum());
        if ((tid & 63) == 0 && cnt > 0) {
            atomicAdd(p.gated + b, cnt);
            atomicAdd(st + 1, (double)cnt);                             // (integers below 2^53: exact in any order)
        }
        for (int o = tid; o < DN_TILE && tile0 + o < p.ldy; o += 256) {
            const int64_t i = tile0 + o;
            float v = 0.f;
            if (i < n) {
                const int h = (int)(i >> 8);
                float env = 0.f;
                for (int t = h - 1; t <= h + 2; ++t)                    // the frames over i, ascending; those that exist
                    if (t >= 0 && t < F) {
                        const float w = win[(int)(i - (int64_t)t * DN_HOP) + DN_N / 2];
                        env = __fadd_rn(env, __fmul_rn(w, w));
                    }
                v = __fdiv_rn(out[o], env);
            }
            y[i] = v;
        }
    }
}

}  // namespace

extern "C" int t2_denoise(const T2Denoise* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->n && a->win && a->tw && a->gated && a->stat, "t2_denoise: null");
    T2_REQUIRE(a->y || a->mag, "t2_denoise: y and mag both null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_denoise: B outside 1 .. 65535");
    T2_REQUIRE(a->n_max >= 0 && a->ldx >= a->n_max, "t2_denoise: n_max < 0 or ldx < n_max");
    T2_REQUIRE(a->x || a->n_max == 0, "t2_denoise: null");
    T2_REQUIRE(!a->y || (a->bias && a->ldy >= a->n_max), "t2_denoise: y without bias, or ldy < n_max");
    T2_REQUIRE(a->strength >= 0.f && a->strength <= 3.4e38f, "t2_denoise: strength negative or not finite");
    T2_REQUIRE(!a->mag || (a->ldm >= DN_BINS && a->f_max >= 1 + a->n_max / DN_HOP), "t2_denoise: ldm < 513 or f_max < 1 + n_max / 256");
    T2_REQUIRE(t2_allow_lds(denoise_kernel, DN_LDS), "t2_denoise: no LDS");
    if (hipMemsetAsync(a->gated, 0, (size_t)a->B * sizeof(int32_t), ST) != hipSuccess ||
        hipMemsetAsync(a->stat, 0, (size_t)a->B * T2_DENOISE_NSTAT * sizeof(double), ST) != hipSuccess) {
        T2_CHECK_LAUNCH();
        return T2_ERR_LAUNCH;
    }
    int64_t tiles = (int64_t)a->n_max / DN_TILE + 1;                     // the owner of the last frame, 16 (n_max / 4096) <= n_max / 256
    if (a->y && (a->ldy + DN_TILE - 1) / DN_TILE > tiles) tiles = (a->ldy + DN_TILE - 1) / DN_TILE;
    hipLaunchKernelGGL(denoise_kernel, dim3((unsigned)tiles, (unsigned)a->B), dim3(256), DN_LDS, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
