// Shared pieces of the model-free measurement kernels (t2_align, t2_dtw, t2_join, t2_limit, t2_loudness, t2_pitch, t2_prosody, t2_psola,
// t2_resample, t2_stretch, t2_variance): their reductions, the frame rule and the count rule.  None of it is on the training
// step's path.  Every reduction walks the wave with __shfl_xor at offsets 32, 16, .., 1 and then the waves in order 0 .. NW - 1:
// one fixed association, so float sums keep their bits from launch to launch (t2_wave_sum of t2_common.hpp has another order).
#pragma once
#include "t2_common.hpp"

#define ST ((hipStream_t)stream)

struct T2mSum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct T2mMax { template <typename T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };
struct T2mMin { template <typename T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct T2mFmax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

template <typename T, typename Op>
__device__ __forceinline__ T t2m_wave_reduce(T v, Op op) {              // every lane gets the result
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, T2_WAVE));
    return v;
}

// Over a block of NW waves; red: NW values of LDS.  Every thread gets the result.  UNROLL: how many of the NW - 1 combining steps are
// issued together - all 15 of a 1024-thread block cost 40 VGPRs more, which only a kernel that reduces once per step of a chain
// (t2_stretch: 3 % of its time) gets back.
template <int NW, int UNROLL = 4, typename T, typename Op>
__device__ __forceinline__ T t2m_block_reduce(T v, Op op, T* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = t2m_wave_reduce(v, op);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    T s = red[0];
#pragma unroll UNROLL
    for (int i = 1; i < NW; ++i) s = op(s, red[i]);
    return s;
}

// M accumulators of a block of NW waves summed into v[] of THREAD 0 (other threads keep a wave's sum); red: [M][NW] of LDS.  The
// first function has no barrier: the caller places ONE between the two.
template <int NW, int M, typename T>
__device__ __forceinline__ void t2m_wave_partials(T (&v)[M], T (*red)[NW]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < M; ++q) {
        v[q] = t2m_wave_reduce(v[q], T2mSum());
        if (lane == 0) red[q][w] = v[q];
    }
}
template <int NW, int M, typename T>
__device__ __forceinline__ void t2m_sum_partials(T (&v)[M], const T (*red)[NW]) {
    for (int q = 0; q < M; ++q) {
        T m = 0;
        for (int r = 0; r < NW; ++r) m += red[q][r];
        v[q] = m;
    }
}
template <int NW, int M>
__device__ __forceinline__ void t2m_sums_to_thread0(double (&s)[M], double (*redd)[NW]) {
    t2m_wave_partials(s, redd);
    __syncthreads();
    if (threadIdx.x == 0) t2m_sum_partials(s, redd);
}
// ... with N counts beside them; the counts reach every thread (integers: a few broadcast reads)
template <int NW, int N, int M>
__device__ __forceinline__ void t2m_sums_to_thread0(int (&cnt)[N], double (&s)[M], int (*redn)[NW], double (*redd)[NW]) {
    t2m_wave_partials(cnt, redn);
    t2m_wave_partials(s, redd);
    __syncthreads();
    t2m_sum_partials(cnt, redn);
    if (threadIdx.x == 0) t2m_sum_partials(s, redd);
}

// The best (value, index) of a wave, in every lane; better(ov, oi, v, i): "the other pair replaces mine".  A rule that breaks ties
// by the lower index gives the same pair in any order.
template <typename V, typename Better>
__device__ __forceinline__ void t2m_wave_pick(V& v, int& i, Better better) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const V ov = __shfl_xor(v, o, T2_WAVE);
        const int oi = __shfl_xor(i, o, T2_WAVE);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}
// ... and of NW wave partials, in wave order
template <int NW, typename V, typename Better>
__device__ __forceinline__ void t2m_combine_picks(const V* rv, const int* ri, V& v, int& i, Better better) {
    v = rv[0]; i = ri[0];
#pragma unroll
    for (int r = 1; r < NW; ++r)
        if (better(rv[r], ri[r], v, i)) { v = rv[r]; i = ri[r]; }
}

// The largest magnitude among the 4 values t2_resample writes behind one input sample with U = 4, D = 1 (the true peak of t2_loudness
// and t2_limit): table [4][2K], xr the sample of tap -K+1 in a staged span; one fmaf per tap in ascending k from 0.0f.
__device__ __forceinline__ float t2m_peak4(const float* table, int K, const float* xr) {
    float tp = 0.f;
    for (int ph = 0; ph < 4; ++ph) {
        const float* h = table + (int64_t)ph * (2 * K);
        float acc = 0.f;
        for (int k = 0; k < 2 * K; ++k) acc = fmaf(h[k], xr[k], acc);
        tp = fmaxf(tp, fabsf(acc));
    }
    return tp;
}

// Frame t of hop `hop` and span S is valid when its span [s0, s0 + S), s0 = t hop - S / 2, lies inside the row's n samples.
__device__ __forceinline__ bool t2m_frame_valid(long t, int hop, int S, long n, long* s0_out) {
    const long s0 = t * hop - S / 2;
    *s0_out = s0;
    return s0 >= 0 && s0 + S <= n;
}

// A device-side count is accepted when it lies in 0 .. n_max; a row with another count is refused, not clamped.
__device__ __forceinline__ bool t2m_count_ok(long n, long n_max) { return n >= 0 && n <= n_max; }
