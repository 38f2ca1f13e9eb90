// TD-PSOLA pitch change of a padded batch of waveforms (include/tacotron2_amd.h: t2_psola; restated in numpy in
// tests/psola_ref.py).  Every pitch mark depends on the mark before it, so a row is two chains: one 1024-thread workgroup per row, the
// chains inside the kernel, as in t2_stretch.hip.  One launch, no cross-workgroup synchronisation, no atomics; every decision is made on
// integers or on a comparison of input floats, so two calls - or this kernel and numpy - place every mark on the same sample.
//
//   check   the Tb frames of lag and rho the row reads; one bad value refuses the row (n_marks = -1, nothing else written).
//   chain 1 analysis marks, by wave 0.  The signal goes through LDS in pieces of PS_PIECE samples that start at the last mark, with
//           the lags of the piece's frames beside it; the wave places marks while the next search window lies inside the piece (a window
//           ends at most 5120 samples behind the last mark, so every piece places at least one).  A window's maximum is a strided scan
//           per lane and six shuffles over (value, index), the smaller index winning a tie; no workgroup barrier per mark, two per piece.
//   chain 2 synthesis marks, by one thread: int64 fixed point and a pointer into a that only moves forward.  a (up to PS_A_CAP marks)
//           and the effective rho (up to PS_T_CAP frames) are read from LDS, where the piece was; longer rows read global memory.
//   sweep   all threads gather: a binary search for the first grain that can reach sample i (r_j > i - gmax, gmax the row's largest
//           mark spacing), then the grains in ascending j up to r_j >= i + gmax.  Products and sums by __fmul_rn / __fadd_rn, nothing
//           fused, one IEEE division.  a, r and kmap are read back from global memory behind the barrier that ends chain 2.
#include "t2_measure.hpp"

namespace {

#define PS_THREADS 1024
#define PS_PIECE 16384                                                    // samples of one staged piece (64 KB)
#define PS_LAGS (PS_PIECE / 16 + 2)                                       // frames under one piece at the smallest hop, 16
#define PS_A_CAP 12288                                                    // marks and frames chain 2 finds in LDS: together the piece's
#define PS_T_CAP 4096                                                     // 16384 dwords
#define PS_ONE 65536

__global__ __launch_bounds__(PS_THREADS) void psola_kernel(T2Psola p) {
    __shared__ __attribute__((aligned(16))) int buf[PS_PIECE];
    __shared__ int lags[PS_LAGS];
    __shared__ int st[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = p.n[b];
    if (!t2m_count_ok(n, p.n_max)) {                                      // refused, not clamped: the row is neither read nor written
        if (tid == 0) p.n_marks[b] = -1;
        return;
    }
    const int hop = p.hop, U = p.U;
    const int Tb = min(p.T, 1 + n / hop);
    const float* x = p.x + (int64_t)b * p.ldx;
    const int32_t* lag = p.lag + (int64_t)b * p.ldt;
    const int32_t* rho = p.rho + (int64_t)b * p.ldt;
    float* y = p.y + (int64_t)b * p.ldy;
    int32_t* a = p.a + (int64_t)b * p.ldm;
    int32_t* r = p.r + (int64_t)b * p.lds;
    int32_t* kmap = p.kmap + (int64_t)b * p.lds;
    auto tf = [&](int s) { return min((s + hop / 2) / hop, Tb - 1); };   // t(s)

    // ---- check ----
    int bad = 0;
    for (int t = tid; t < Tb; t += PS_THREADS) {
        const int l = lag[t];
        if (l != 0) {
            const int q = rho[t];
            bad |= (l < T2_PSOLA_MIN_LAG || l > T2_PSOLA_MAX_LAG || q < T2_PSOLA_MIN_RHO || q > T2_PSOLA_MAX_RHO) ? 1 : 0;
        }
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) p.n_marks[b] = -1;
        return;
    }

    // ---- chain 1 ----
    float* xs = reinterpret_cast<float*>(buf);
    int cur = 0, k = 0, gmax = 0;                                         // a_k, k and the largest spacing so far: uniform
    if (tid == 0) a[0] = 0;
    for (;;) {
        const int base = cur, t0 = tf(base);
        __syncthreads();                                                  // the piece before, and st, have been read
        for (int i = tid; i < PS_PIECE && base + i < n; i += PS_THREADS) xs[i] = x[base + i];
        for (int i = tid; i < PS_LAGS; i += PS_THREADS) lags[i] = t0 + i < Tb ? lag[t0 + i] : 0;
        __syncthreads();
        if (wave == 0) {
            int done = 0;
            for (;;) {
                int step = lags[tf(cur) - t0];
                step = step ? step : U;
                const int c = cur + step;
                int m = c;
                if (c >= n) { m = n; done = 1; }                          // the terminal mark
                else {
                    if (c >= base + PS_PIECE) break;                      // (the next piece starts at cur)
                    const int pc = lags[tf(c) - t0];
                    if (pc > 0) {
                        const int d = min(pc, step) / 4, lo = c - d, hi = min(c + d, n - 1);
                        if (hi >= base + PS_PIECE) break;
                        float bv = -INFINITY;
                        int bi = INT_MAX;
                        for (int i = lo + lane; i <= hi; i += 64) {
                            const float v = xs[i - base];
                            if (bi == INT_MAX || v > bv) { bv = v; bi = i; }
                        }
                        t2m_wave_pick(bv, bi, [](float ov, int oi, float v, int i) { return ov > v || (ov == v && oi < i); });
                        m = __builtin_amdgcn_readfirstlane(bi);           // (lane 0 scanned lo itself: an index inside the window)
                    }
                }
                if (lane == 0) a[k + 1] = m;
                gmax = max(gmax, m - cur);
                cur = m;
                ++k;
                if (done) break;
            }
            if (lane == 0) { st[0] = cur; st[1] = k; st[2] = done; st[3] = gmax; }
        }
        __syncthreads();
        cur = st[0]; k = st[1]; gmax = st[3];
        if (st[2]) break;
    }
    const int K = k;                                                      // a_K = n
    for (int64_t i = K + 1 + tid; i < p.ldm; i += PS_THREADS) a[i] = 0;

    // ---- chain 2 ----
    int* as = buf;
    int* rs = buf + PS_A_CAP;
    const bool a_in = K + 1 <= PS_A_CAP, r_in = Tb <= PS_T_CAP;
    __syncthreads();                                                      // st has been read; a[0 .. K] is visible to the workgroup
    if (a_in) for (int i = tid; i <= K; i += PS_THREADS) as[i] = a[i];
    if (r_in) for (int t = tid; t < Tb; t += PS_THREADS) rs[t] = lag[t] ? rho[t] : PS_ONE;
    __syncthreads();
    if (tid == 0) {
        auto A = [&](int i) { return a_in ? as[i] : a[i]; };
        int64_t s = 0;
        int rj = 0, kj = 0, kk = 0, j = 0;
        r[0] = 0; kmap[0] = 0;
        for (;;) {
            const int t = tf(rj);
            const int q = r_in ? rs[t] : (lag[t] ? rho[t] : PS_ONE);
            s += ((int64_t)(A(kj + 1) - A(kj)) * q) >> 8;
            const int64_t rn = (s + 128) >> 8;
            ++j;
            if (rn >= n || j >= p.lds - 1) {                              // (the second cannot happen under the entry's bound on lds;
                r[j] = n; kmap[j] = K;                                    // kept so that no bound, right or wrong, writes out of range)
                break;
            }
            const int ri = (int)rn;
            while (kk + 1 <= K - 1 && abs(A(kk + 1) - ri) < abs(A(kk) - ri)) ++kk;    // a tie keeps the smaller k
            r[j] = ri; kmap[j] = kk;
            rj = ri; kj = kk;
        }
        st[0] = j;
    }
    __syncthreads();                                                      // r and kmap [0 .. J] are visible to the workgroup
    const int J = st[0];
    for (int64_t i = J + 1 + tid; i < p.lds; i += PS_THREADS) { r[i] = 0; kmap[i] = 0; }
    if (tid == 0) { p.n_marks[b] = K + 1; p.n_syn[b] = J + 1; }

    // ---- sweep ----
    for (int64_t i64 = tid; i64 < p.ldy; i64 += PS_THREADS) {
        float v = 0.f;
        if (i64 < n) {
            const int i = (int)i64, key = i - gmax;
            int lo = 0, hi = J + 1;                                       // the first j with r_j > i - gmax
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (r[mid] > key) hi = mid; else lo = mid + 1;
            }
            float num = 0.f, den = 0.f;
            for (int j = lo; j <= J; ++j) {
                const int rj = r[j];
                if (rj - i >= gmax) break;
                const int kj = kmap[j], ak = a[kj], e = i - rj;
                float w = 1.f;
                if (e < 0) {
                    if (kj == 0) continue;
                    const int L = ak - a[kj - 1];
                    if (-e >= L) continue;
                    w = p.w[((L + e) * 1024) / L];
                } else if (e > 0) {
                    if (kj == K) continue;
                    const int R = a[kj + 1] - ak;
                    if (e >= R) continue;
                    w = p.w[1024 - (e * 1024) / R];
                }
                num = __fadd_rn(num, __fmul_rn(w, x[ak + e]));            // (e == 0 belongs to a grain with k < K: r_J = n > i)
                den = __fadd_rn(den, w);
            }
            v = __fdiv_rn(num, fmaxf(den, 1.f));
        }
        y[i64] = v;
    }
}

}  // namespace

extern "C" int t2_psola(const T2Psola* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->n && a->lag && a->rho && a->w && a->a && a->r && a->kmap && a->n_marks && a->n_syn, "t2_psola: null");
    T2_REQUIRE(a->B >= 1 && a->B <= 65535, "t2_psola: B outside 1 .. 65535");
    T2_REQUIRE(a->n_max >= 0 && a->n_max <= (1 << 27) && a->ldx >= a->n_max, "t2_psola: n_max outside 0 .. 2^27 or ldx < n_max");
    T2_REQUIRE(a->T >= 1 && a->ldt >= a->T, "t2_psola: T < 1 or ldt < T");
    T2_REQUIRE(a->hop >= 16 && a->hop <= (1 << 20), "t2_psola: hop outside 16 .. 2^20");
    T2_REQUIRE(a->U >= T2_PSOLA_MIN_LAG && a->U <= T2_PSOLA_MAX_LAG, "t2_psola: U outside 16 .. 4096");
    T2_REQUIRE(a->ldy >= a->n_max, "t2_psola: ldy < n_max");
    T2_REQUIRE(a->ldm >= a->n_max / 12 + 2, "t2_psola: ldm < n_max / 12 + 2");
    T2_REQUIRE(a->lds >= a->n_max / 3 + T2_PSOLA_SYN_TAIL, "t2_psola: lds < n_max / 3 + 10256");
    T2_REQUIRE((a->x || a->n_max == 0) && (a->y || a->ldy == 0), "t2_psola: null");
    hipLaunchKernelGGL(psola_kernel, dim3((unsigned)a->B), dim3(PS_THREADS), 0, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
