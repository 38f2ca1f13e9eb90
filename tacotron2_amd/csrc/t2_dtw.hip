// Objective scoring of a decode against the recording (include/tacotron2_amd.h: t2_mel_cepstra, t2_dtw): mel-cepstral
// coefficients of log-mel rows, and dynamic time warping between two feature sequences.  An evaluation path - milliseconds per
// batch - so both kernels are plain, in the style of t2_align.hip: no cross-workgroup synchronisation, nothing persistent, no
// atomics to global memory.
//
//   t2_dtw: ONE 256-thread workgroup per pair walks the anti-diagonals i + j = k.  Every cell of diagonal k reads diagonals k-1
//     and k-2 only, so three rotating rows of fp64 D and of int32 path lengths, indexed by i, live in LDS; the block strides over
//     the diagonal's cells, one barrier per diagonal.  d(i, j) is formed on the fly in fp32 from the two feature rows and is
//     independent of D: the distances of diagonal k+1 are computed BEFORE the barrier of diagonal k, so no global load sits
//     between a barrier and the LDS reads that depend on it.  fp64 D: totals reach ~1e5 over a few thousand cells, where an fp32
//     ulp (8e-3) is the size of real decision margins.
#include "t2_measure.hpp"

namespace {

#define DTW_THREADS 256
#define DTW_MAXC (T2_DTW_MAX_T / DTW_THREADS)      // cells of one diagonal a thread can own

__global__ __launch_bounds__(256) void mel_cepstra_kernel(T2MelCeps p) {
    const int b = blockIdx.y;
    const int n = min(max(p.len[b], 0), p.T);
    const long e = (long)blockIdx.x * 256 + threadIdx.x;      // (t, k) of this thread
    const int t = (int)(e / p.K), k = (int)(e % p.K);
    if (t >= n) return;
    const float* x = p.mel + (long)b * p.ld_b + (long)t * p.ld_t;
    const float* w = p.basis + k;
    float s = 0.f;
    for (int m = 0; m < p.M; ++m) s = fmaf(x[m], w[(long)m * p.K], s);
    p.out[(long)b * p.ld_ob + (long)t * p.ld_ot + k] = s;
}

// KT > 0: K is the compile-time KT, the loop unrolls and the 2 K loads of a cell are issued together (one load latency per cell
// instead of K dependent ones); KT = 0: any K at run time.  The same operations in the same order either way.
template <int KT>
__device__ __forceinline__ float dtw_dist(const float* __restrict__ ar, const float* __restrict__ br, int Krt, float scale) {
    const int K = KT ? KT : Krt;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float d = ar[k] - br[k];
        s = fmaf(d, d, s);
    }
    return scale * sqrtf(s);
}

// dynamic LDS: D[3][Ta] doubles, then len[3][Ta] ints; row (k % 3) belongs to diagonal k
template <int KT>
__global__ __launch_bounds__(DTW_THREADS) void dtw_kernel(T2Dtw p) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Ta = p.Ta, Tb = p.Tb, K = p.K;
    double* D = lds;
    int* Ln = reinterpret_cast<int*>(lds + 3 * (long)Ta);
    const int la = min(max(p.len_a[b], 0), Ta), lb = min(max(p.len_b[b], 0), Tb);
    if (la == 0 || lb == 0) {
        if (tid == 0) { p.cost[b] = 0.0; p.path_len[b] = 0; }
        return;
    }
    const float* A = p.a + (long)b * p.ld_ab;
    const float* Bf = p.b + (long)b * p.ld_bb;
    const int64_t lda = p.ld_at, ldb = p.ld_bt;
    const float scale = p.scale;
    uint8_t* back = p.back ? p.back + (long)b * Ta * Tb : nullptr;
    const int nd = la + lb - 1;                          // diagonals
    const int nc = (la + DTW_THREADS - 1) / DTW_THREADS; // cells per thread and diagonal, at most (<= DTW_MAXC: Ta <= T2_DTW_MAX_T)

    float dn[DTW_MAXC];                                  // distances of this thread's cells on the NEXT diagonal
#pragma unroll
    for (int c = 0; c < DTW_MAXC; ++c) {
        const int i = tid + c * DTW_THREADS;
        dn[c] = (c < nc && i == 0) ? dtw_dist<KT>(A, Bf, K, scale) : 0.f;      // diagonal 0 is the cell (0, 0)
    }
    int r0 = 0, r1 = 2, r2 = 1;                          // rows of diagonals k, k-1, k-2
    for (int k = 0; k < nd; ++k) {
        float dc[DTW_MAXC];
#pragma unroll
        for (int c = 0; c < DTW_MAXC; ++c) dc[c] = dn[c];
        // cells of diagonal k+1: i in [max(0, k+1-(lb-1)), min(la-1, k+1)]
#pragma unroll
        for (int c = 0; c < DTW_MAXC; ++c) {
            const int i = tid + c * DTW_THREADS, j = k + 1 - i;
            if (c < nc && k + 1 < nd && i < la && j >= 0 && j < lb) dn[c] = dtw_dist<KT>(A + i * lda, Bf + j * ldb, K, scale);
        }
        double* Dc = D + (long)r0 * Ta;
        const double* D1 = D + (long)r1 * Ta;
        const double* D2 = D + (long)r2 * Ta;
        int* Lc = Ln + (long)r0 * Ta;
        const int* L1 = Ln + (long)r1 * Ta;
        const int* L2 = Ln + (long)r2 * Ta;
#pragma unroll
        for (int c = 0; c < DTW_MAXC; ++c) {
            const int i = tid + c * DTW_THREADS, j = k - i;
            if (c < nc && i < la && j >= 0 && j < lb) {
                double best = 0.0;
                int len = 0;
                uint8_t mv = 0;
                if (i > 0 && j > 0) {
                    best = D2[i - 1]; len = L2[i - 1];
                    const double up = D1[i - 1];
                    if (up < best) { best = up; len = L1[i - 1]; mv = 1; }
                    const double lf = D1[i];
                    if (lf < best) { best = lf; len = L1[i]; mv = 2; }
                } else if (i > 0) {
                    best = D1[i - 1]; len = L1[i - 1]; mv = 1;
                } else if (j > 0) {
                    best = D1[i]; len = L1[i]; mv = 2;
                }
                Dc[i] = best + (double)dc[c];
                Lc[i] = len + 1;
                if (back) back[(long)i * Tb + j] = mv;
            }
        }
        __syncthreads();      // one barrier per diagonal: row r0 is complete, row r2 is free for diagonal k + 1
        const int t = r2; r2 = r1; r1 = r0; r0 = t;
    }
    if (tid == 0) {           // (after the rotation r1 is the row of the last diagonal)
        const int n = Ln[(long)r1 * Ta + la - 1];
        p.cost[b] = D[(long)r1 * Ta + la - 1];
        p.path_len[b] = n;
        if (back && p.path) { // backtrack from (la - 1, lb - 1); the cells are written in forward order
            int32_t* path = p.path + (long)b * (Ta + Tb - 1) * 2;
            int i = la - 1, j = lb - 1;
            for (int s = n - 1; s >= 0 && i >= 0 && j >= 0; --s) {
                path[2 * s] = i;
                path[2 * s + 1] = j;
                const uint8_t mv = back[(long)i * Tb + j];
                if (mv != 2) --i;
                if (mv != 1) --j;
            }
        }
    }
}

}  // namespace

extern "C" int t2_mel_cepstra(const T2MelCeps* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->mel && a->len && a->basis && a->out, "t2_mel_cepstra: null");
    T2_REQUIRE(a->B >= 1 && a->T >= 1 && a->M >= 1, "t2_mel_cepstra: need B, T, M >= 1");
    T2_REQUIRE(a->M <= T2_CEPS_MAX_M, "t2_mel_cepstra: M above T2_CEPS_MAX_M (1024)");
    T2_REQUIRE(a->K >= 1 && a->K <= T2_DTW_MAX_K, "t2_mel_cepstra: K outside 1 .. T2_DTW_MAX_K (32)");
    T2_REQUIRE(a->ld_t >= a->M && (a->B == 1 || a->ld_b >= (int64_t)(a->T - 1) * a->ld_t + a->M),
               "t2_mel_cepstra: overlapping strides of mel: need ld_t >= M, ld_b >= (T-1)*ld_t + M");
    T2_REQUIRE(a->ld_ot >= a->K && (a->B == 1 || a->ld_ob >= (int64_t)(a->T - 1) * a->ld_ot + a->K),
               "t2_mel_cepstra: overlapping strides of out: need ld_ot >= K, ld_ob >= (T-1)*ld_ot + K");
    T2_REQUIRE(a->B <= 65535, "t2_mel_cepstra: B above 65535");
    const unsigned gx = (unsigned)t2_cdiv((long)a->T * a->K, 256);
    hipLaunchKernelGGL(mel_cepstra_kernel, dim3(gx, (unsigned)a->B), dim3(256), 0, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}

extern "C" int t2_dtw(const T2Dtw* a, void* stream) {
    (void)hipGetLastError();
    T2_REQUIRE(a && a->a && a->b && a->len_a && a->len_b && a->cost && a->path_len, "t2_dtw: null");
    T2_REQUIRE(a->B >= 1 && a->Ta >= 1 && a->Tb >= 1, "t2_dtw: need B, Ta, Tb >= 1");
    T2_REQUIRE(a->Ta <= T2_DTW_MAX_T && a->Tb <= T2_DTW_MAX_T, "t2_dtw: Ta or Tb above T2_DTW_MAX_T (4096)");
    T2_REQUIRE(a->K >= 1 && a->K <= T2_DTW_MAX_K, "t2_dtw: K outside 1 .. T2_DTW_MAX_K (32)");
    T2_REQUIRE(a->back || !a->path, "t2_dtw: a path needs the back workspace [B][Ta][Tb]");
    T2_REQUIRE(a->scale == a->scale && a->scale - a->scale == 0.f, "t2_dtw: scale must be finite");
    T2_REQUIRE(a->ld_at >= a->K && (a->B == 1 || a->ld_ab >= (int64_t)(a->Ta - 1) * a->ld_at + a->K),
               "t2_dtw: overlapping strides of a: need ld_at >= K, ld_ab >= (Ta-1)*ld_at + K");
    T2_REQUIRE(a->ld_bt >= a->K && (a->B == 1 || a->ld_bb >= (int64_t)(a->Tb - 1) * a->ld_bt + a->K),
               "t2_dtw: overlapping strides of b: need ld_bt >= K, ld_bb >= (Tb-1)*ld_bt + K");
    const size_t bytes = 3 * (size_t)a->Ta * (sizeof(double) + sizeof(int));
    if (a->K == 13) {          // the default number of coefficients gets the unrolled distance
        T2_REQUIRE(t2_allow_lds(dtw_kernel<13>, bytes), "t2_dtw: LDS request refused");
        hipLaunchKernelGGL(dtw_kernel<13>, dim3((unsigned)a->B), dim3(DTW_THREADS), bytes, ST, *a);
    } else {
        T2_REQUIRE(t2_allow_lds(dtw_kernel<0>, bytes), "t2_dtw: LDS request refused");
        hipLaunchKernelGGL(dtw_kernel<0>, dim3((unsigned)a->B), dim3(DTW_THREADS), bytes, ST, *a);
    }
    T2_CHECK_LAUNCH(); return T2_OK;
}
