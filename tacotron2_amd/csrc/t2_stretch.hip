// WSOLA time stretching of a padded batch of waveforms (include/tacotron2_amd.h: t2_stretch; restated in numpy in
// tests/stretch_ref.py).  Each frame's position depends on the choice made for the frame before it, so a row is a chain: one
// 1024-thread workgroup per row, the chain inside the kernel, as in t2_align.hip, t2_dtw.hip, t2_pitch.hip and t2_join.hip.  One launch,
// no cross-workgroup synchronisation, no atomics; every decision is made on integers whose sums are exact in int32, so the order of
// the additions does not matter and two calls - or this kernel and numpy - choose the same offset on every frame.
//
//   peak    max |x[i]| over i < n[b]: a float maximum, exact in any order.
//   chain   frames m = 1 .. M - 1 in turn.  The template (N int16) and the search region (N + 2D int16) are quantised from x into LDS:
//           q = rint(x * 1023 / peak) in fp64, an IEEE division, so numpy gives these bits.  Thread (g, s) scores the FOUR adjacent
//           offsets e = 4g .. 4g + 3 (e = d + D) over the template chunks c = s, s + S, ..: one 16-byte read of 8 template values and
//           three 8-byte reads of the 11 region values under them feed 32 multiply-adds, as 16 packed 16-bit dot instructions
//           (v_dot2_i32_i16; the odd offsets take their pairs from five v_alignbit; DESIGN 9 has what this was chosen over).  The
//           S partial scores of an offset are added
//           by one thread, and a workgroup-wide maximum over the 64-bit key (score << 32 | rank) applies the tie rule: rank =
//           2 (D - |d|) + (d < 0), so the smaller |d| wins, then the negative one.  Every thread holds p_m afterwards.
//   sweep   y[j] = w[Hs + i] x~[p_m + i] + w[i] x~[p_{m+1} - Hs + i] for j = m Hs + i < n_out, two products and one sum in fp32, nothing
//           fused; zeros behind n_out up to ldy.  pos is read back from global memory behind the barrier that ends the chain.
#include "t2_measure.hpp"

namespace {

#define SR_THREADS 1024
#define SR_WAVES (SR_THREADS / 64)
#define SR_T_LEN (T2_STRETCH_MAX_N + 8)                                   // the template, zero padded to whole chunks of 8
#define SR_R_LEN (T2_STRETCH_MAX_N + 2 * T2_STRETCH_MAX_D + 32)          // the region and the zeros a thread's last reads run into

__device__ __forceinline__ short sr_quant(const float* x, int64_t i, int64_t n, double peak) {
    if (i < 0 || i >= n || !(peak > 0.0)) return 0;
    return (short)(int)rint((double)x[i] * 1023.0 / peak);
}

// Two int16 in a dword, the first in the low half.  sr_dot: a.lo * b.lo + a.hi * b.hi + c (v_dot2_i32_i16, no saturation: the whole
// sum is below 2^31); sr_odd: the pair that straddles two neighbouring dwords, (lo.hi, hi.lo).
typedef short sr_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int sr_dot(int a, int b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(sr_short2, a), __builtin_bit_cast(sr_short2, b), c, false);
}
__device__ __forceinline__ int sr_odd(int lo, int hi) { return (int)__builtin_amdgcn_alignbit((unsigned)hi, (unsigned)lo, 16); }

__device__ __forceinline__ float sr_at(const float* x, int64_t i, int64_t n) { return i >= 0 && i < n ? x[i] : 0.f; }

__global__ __launch_bounds__(SR_THREADS) void stretch_kernel(T2Stretch p) {
    __shared__ __attribute__((aligned(16))) short T[SR_T_LEN];
    __shared__ __attribute__((aligned(16))) short R[SR_R_LEN];
    __shared__ int part[4 * SR_THREADS];
    __shared__ long long red[SR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = p.n[b];
    if (!t2m_count_ok(nb, p.n_max)) {                                     // refused, not clamped: the row is neither read nor written
        if (tid == 0) p.n_out[b] = -1;
        return;
    }
    const int64_t n = nb;
    const int N = p.N, Hs = N / 2, D = p.D;
    const int64_t P = p.P, Q = p.Q;
    const int64_t n_out = (n * Q + P - 1) / P;
    const int64_t M = (n_out + Hs - 1) / Hs + 1;
    const float* x = p.x + (int64_t)b * p.ldx;
    int32_t* pos = p.pos + (int64_t)b * p.ldp;
    float* y = p.y + (int64_t)b * p.ldy;

    // ---- peak ----
    float pk = 0.f;
    for (int64_t i = tid; i < n; i += SR_THREADS) pk = fmaxf(pk, fabsf(x[i]));
    const double peak =
        (double)__builtin_bit_cast(float, (int)t2m_block_reduce<SR_WAVES, SR_WAVES>((long long)__builtin_bit_cast(int, pk), T2mMax(), red));
    // (|x| >= 0: the bit patterns of non-negative floats order as integers)

    // ---- chain ----
    const int C = 2 * D + 1, G = (C + 3) / 4, nch = (N + 7) / 8;
    int S = SR_THREADS / G;
    S = S > nch ? nch : S;
    const int g = tid % G, s = tid / G;
    const int r_used = 4 * G + 8 * nch;                                   // one past the last region value any thread reads
    int64_t prev = 0;                                                     // p_{m-1}; p_0 = a_0 = (Q / 2) div Q = 0
    if (tid == 0) pos[0] = 0;
    for (int64_t m = 1; m < M; ++m) {
        const int64_t a = (m * Hs * P + Q / 2) / Q;
        __syncthreads();                                                  // the previous frame's reads of T, R and part are over
        for (int k = tid; k < 8 * nch; k += SR_THREADS) T[k] = k < N ? sr_quant(x, prev + k, n, peak) : (short)0;
        for (int j = tid; j < r_used; j += SR_THREADS) R[j] = j < N + 2 * D ? sr_quant(x, a - Hs - D + j, n, peak) : (short)0;
        __syncthreads();
        if (s < S) {
            int acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
            for (int c = s; c < nch; c += S) {
                const int4 t = *reinterpret_cast<const int4*>(T + 8 * c);          // (t0 t1) (t2 t3) (t4 t5) (t6 t7)
                const int2* rp = reinterpret_cast<const int2*>(R + 4 * g + 8 * c);
                const int2 ra = rp[0], rb = rp[1], rc = rp[2];                      // (r0 r1) (r2 r3) | (r4 r5) (r6 r7) | (r8 r9) (r10 -)
                const int u0 = sr_odd(ra.x, ra.y), u1 = sr_odd(ra.y, rb.x), u2 = sr_odd(rb.x, rb.y), u3 = sr_odd(rb.y, rc.x),
                          u4 = sr_odd(rc.x, rc.y);                                  // (r1 r2) (r3 r4) (r5 r6) (r7 r8) (r9 r10)
                acc0 = sr_dot(t.w, rb.y, sr_dot(t.z, rb.x, sr_dot(t.y, ra.y, sr_dot(t.x, ra.x, acc0))));
                acc1 = sr_dot(t.w, u3, sr_dot(t.z, u2, sr_dot(t.y, u1, sr_dot(t.x, u0, acc1))));
                acc2 = sr_dot(t.w, rc.x, sr_dot(t.z, rb.y, sr_dot(t.y, rb.x, sr_dot(t.x, ra.y, acc2))));
                acc3 = sr_dot(t.w, u4, sr_dot(t.z, u3, sr_dot(t.y, u2, sr_dot(t.x, u1, acc3))));
            }
            int* o = part + (s * G + g) * 4;
            o[0] = acc0; o[1] = acc1; o[2] = acc2; o[3] = acc3;
        }
        __syncthreads();
        long long key = INT64_MIN;
        for (int e = tid; e < C; e += SR_THREADS) {                       // (C <= 2049: at most three offsets per thread)
            int sc = 0;
            for (int ss = 0; ss < S; ++ss) sc += part[ss * 4 * G + e];
            const int d = e - D, rank = 2 * (D - (d < 0 ? -d : d)) + (d < 0 ? 1 : 0);
            const long long k2 = (long long)sc * 4294967296LL + rank;
            key = k2 > key ? k2 : key;
        }
        key = t2m_block_reduce<SR_WAVES, SR_WAVES>(key, T2mMax(), red);
        const int rank = (int)(key & 0xffffffffLL);
        const int ad = D - rank / 2;
        prev = a + ((rank & 1) ? -ad : ad);
        if (tid == 0) pos[m] = (int32_t)prev;
    }
    for (int64_t m = M + tid; m < p.ldp; m += SR_THREADS) pos[m] = 0;
    if (tid == 0) p.n_out[b] = (int32_t)n_out;
    __syncthreads();                                                      // pos[0 .. M) of this row is visible to the workgroup

    // ---- sweep ----
    for (int64_t j = tid; j < p.ldy; j += SR_THREADS) {
        float v = 0.f;
        if (j < n_out) {
            const int m = (int)j / Hs, i = (int)j - m * Hs;              // (n_out <= 2^30)
            const int64_t p0 = pos[m], p1 = pos[m + 1];
            v = __fadd_rn(__fmul_rn(p.w[Hs + i], sr_at(x, p0 + i, n)), __fmul_rn(p.w[i], sr_at(x, p1 - Hs + i, n)));
        }
        y[j] = v;
    }
}

}  // namespace

extern "C" int t2_stretch(const T2Stretch* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->n && a->w && a->pos && a->n_out, "t2_stretch: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_stretch: B outside 1 .. 65535");
    T2_REQUIRE(a->N >= 4 && a->N <= T2_STRETCH_MAX_N && a->N % 2 == 0, "t2_stretch: N outside 4 .. 2048 or odd");
    T2_REQUIRE(a->D >= 0 && a->D <= T2_STRETCH_MAX_D, "t2_stretch: D outside 0 .. 1024");
    T2_REQUIRE(a->P >= 1 && a->Q >= 1 && a->P <= (1 << 20) && a->Q <= (1 << 20) && a->P <= 8 * (int64_t)a->Q && a->Q <= 8 * (int64_t)a->P,
               "t2_stretch: P or Q outside 1 .. 2^20, or a tempo P / Q outside 1/8 .. 8");
    T2_REQUIRE(a->n_max >= 0 && a->n_max <= (1 << 27) && a->ldx >= a->n_max, "t2_stretch: n_max outside 0 .. 2^27 or ldx < n_max");
    const int64_t n_out_max = ((int64_t)a->n_max * a->Q + a->P - 1) / a->P, Hs = a->N / 2;
    T2_REQUIRE(a->ldy >= n_out_max, "t2_stretch: ldy < ceil(n_max Q / P)");
    T2_REQUIRE(a->ldp >= (n_out_max + Hs - 1) / Hs + 1, "t2_stretch: ldp < ceil(ceil(n_max Q / P) / (N / 2)) + 1");
    T2_REQUIRE((a->x || a->n_max == 0) && (a->y || a->ldy == 0), "t2_stretch: null");
    hipLaunchKernelGGL(stretch_kernel, dim3((unsigned)a->B), dim3(SR_THREADS), 0, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
