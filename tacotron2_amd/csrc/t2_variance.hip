// Per-character pitch and energy targets on the character grid of t2_align_durations (include/tacotron2_amd.h:
// t2_char_variance): a pitch track and a log-mel cut at the character boundaries and averaged, with the sums a
// student's normalisation needs.  An export path like t2_align.hip, so the kernel is plain: ONE launch, ONE 256-thread workgroup
// per utterance, no cross-workgroup synchronisation, no atomics, every sum in a fixed order (two calls are bit-identical).
//
//   1. span starts: the prefix sum of max(dur, 0) over n < N_b in int64 (each thread a contiguous chunk, then the 256 chunk
//      totals), stored clipped to F_b.  `consistent` compares the unclipped total with F_b.
//   2. frame pass: p(t) and the voicing bit of every frame t < F_b (one ballot word per 64 frames), and the energy
//      e(t) = sqrt(sum_m exp(2 mel[t][m])) in fp64: 16 lanes per frame, lane l takes m = l, l + 16, ... in order, then a
//      butterfly over the 16 lanes - coalesced 64-byte reads of a mel row, one order of summation.
//   3. interpolation (optional): each thread owns a contiguous chunk of frames; the chunk's first and last voiced frame go to LDS,
//      from which every thread finds the voiced frame before and behind its chunk, then walks its chunk.  Only unvoiced entries of
//      q are written, only voiced ones read: no ordering between threads is needed inside the pass.
//   4. characters: thread n sums q, e and the voicing bits of its span in frame order.
//   5. the per-utterance sums: thread-strided partials, a wave butterfly, the four wave partials in order.
// q and e stay in LDS as doubles between the passes: 2 * 8 * T + 4 * (L + 1) bytes = 80 KB at both caps, plus 4.8 KB of small
// arrays (reduction partials, chunk totals, chunk voicing, voicing bits).
#include "t2_measure.hpp"

namespace {

constexpr int kRed = 32;        // doubles: 8 sums x 4 wave partials
constexpr int kChunks = 256;    // one chunk per thread

__host__ __device__ inline size_t variance_lds_bytes(int T, int L) {
    // red[32] doubles | part[256] int64 | edge[512] int32 | vbits[ceil(T/64)] uint64 | q[T] | e[T] doubles | start[L + 1] int32
    return 8 * (size_t)kRed + 8 * (size_t)kChunks + 4 * (size_t)(2 * kChunks) + 8 * (size_t)((T + 63) / 64) + 16 * (size_t)T +
           4 * (size_t)(L + 1);
}

__global__ __launch_bounds__(256) void char_variance_kernel(T2CharVariance a) {
    extern __shared__ double lds[];
    const int T = a.T, L = a.L, M = a.M;
    double (*red)[4] = reinterpret_cast<double (*)[4]>(lds);
    long long* part = reinterpret_cast<long long*>(lds + kRed);
    int* edge = reinterpret_cast<int*>(lds + kRed + kChunks);                 // [0, 256) first voiced of a chunk, [256, 512) last
    unsigned long long* vbits = reinterpret_cast<unsigned long long*>(lds + kRed + kChunks + kChunks);
    double* q = lds + kRed + 2 * kChunks + (T + 63) / 64;
    double* e = q + T;
    int* start = reinterpret_cast<int*>(e + T);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Nb = min(max(a.chars_len[b], 0), L);
    const int Fb = min(max(a.frames_len[b], 0), T);
    const int32_t* dur = a.dur + (long)b * a.ld_dur;
    float* cp = a.char_pitch + (long)b * L;
    float* ce = a.char_energy + (long)b * L;
    int32_t* cv = a.char_voiced + (long)b * L;
    float* fp = a.frame_pitch ? a.frame_pitch + (long)b * T : nullptr;
    float* fe = a.frame_energy ? a.frame_energy + (long)b * T : nullptr;
    double* stats = a.stats + (long)b * T2_VAR_NSTAT;

    // 1. span starts
    const int cn = (Nb + kChunks - 1) / kChunks;           // characters per thread (<= 16)
    const int n0 = min(tid * cn, Nb), n1 = min(n0 + cn, Nb);
    long long mine = 0;
    for (int n = n0; n < n1; ++n) mine += max(dur[n], 0);
    part[tid] = mine;
    __syncthreads();
    long long before = 0, total = 0;
    for (int i = 0; i < kChunks; ++i) {
        const long long v = part[i];
        before += i < tid ? v : 0;
        total += v;
    }
    for (int n = n0; n < n1; ++n) {
        start[n] = (int)min(before, (long long)Fb);
        before += max(dur[n], 0);
    }
    if (tid == 0) start[Nb] = (int)min(total, (long long)Fb);
    const double consistent = total == (long long)Fb ? 1.0 : 0.0;

    if (Nb == 0 || Fb == 0) {           // (the whole block takes this branch) nothing of f0 or mel is read
        for (int n = tid; n < L; n += 256) { cp[n] = 0.f; ce[n] = 0.f; cv[n] = 0; }
        for (int t = tid; t < Fb; t += 256) {
            if (fp) fp[t] = 0.f;
            if (fe) fe[t] = 0.f;
        }
        if (tid < T2_VAR_NSTAT) stats[tid] = tid == 8 ? consistent : 0.0;
        return;
    }
    const float* f0 = a.f0 + (long)b * a.ld_f0;
    const float* mel = a.mel + (long)b * a.ld_b;

    // 2. frame pass: pitch and voicing (every wave runs every iteration: the ballot needs all 64 lanes) ...
    for (int t0 = 0; t0 < Fb; t0 += 256) {
        const int t = t0 + tid;
        float f = 0.f;
        if (t < Fb) f = f0[t];
        const bool v = f > 0.f;                            // (a NaN is unvoiced)
        const unsigned long long m = __ballot(v);
        if (t < Fb) q[t] = v ? (a.log_pitch ? log((double)f) : (double)f) : 0.0;
        if (lane == 0 && t0 + w * 64 < Fb) vbits[(t0 >> 6) + w] = m;
    }
    // ... and energy: 16 lanes per frame
    {
        const int g = tid >> 4, l = tid & 15;
        for (int t0 = 0; t0 < Fb; t0 += 16) {
            const int t = t0 + g;
            double acc = 0.0;
            if (t < Fb) {
                const float* row = mel + (long)t * a.ld_t;
                for (int m = l; m < M; m += 16) acc += exp(2.0 * (double)row[m]);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
            if (l == 0 && t < Fb) e[t] = sqrt(acc);
        }
    }
    __syncthreads();
#define VOICED(t) ((int)((vbits[(t) >> 6] >> ((t) & 63)) & 1ull))

    // 3. interpolation across the unvoiced frames
    if (a.interpolate) {
        const int cf = (Fb + kChunks - 1) / kChunks;       // frames per thread (<= 16)
        const int c0 = min(tid * cf, Fb), c1 = min(c0 + cf, Fb);
        int first = -1, last = -1;
        for (int t = c0; t < c1; ++t)
            if (VOICED(t)) { if (first < 0) first = t; last = t; }
        edge[tid] = first;
        edge[kChunks + tid] = last;
        __syncthreads();
        int prev = -1, next = -1;                          // the voiced frame before / behind this chunk
        for (int i = tid - 1; i >= 0 && prev < 0; --i) prev = edge[kChunks + i];
        for (int i = tid + 1; i < kChunks && next < 0; ++i) next = edge[i];
        for (int t = c0; t < c1; ++t) {
            if (VOICED(t)) { prev = t; continue; }
            int c = next;
            for (int u = c1 - 1; u > t; --u)
                if (VOICED(u)) c = u;
            double v = 0.0;
            if (prev >= 0 && c >= 0) {
                const double pa = q[prev], pc = q[c];
                v = pa + (pc - pa) * ((double)(t - prev) / (double)(c - prev));
            } else if (prev >= 0) {
                v = q[prev];
            } else if (c >= 0) {
                v = q[c];
            }
            q[t] = v;
        }
        __syncthreads();
    }
    for (int t = tid; t < Fb; t += 256) {
        if (fp) fp[t] = (float)q[t];
        if (fe) fe[t] = (float)e[t];
    }

    // 4. characters: the span's sums in frame order
    int unvoiced_chars = 0;
    for (int n = tid; n < L; n += 256) {
        float pitch = 0.f, energy = 0.f;
        int nv = 0;
        if (n < Nb) {
            const int s0 = start[n], s1 = start[n + 1];
            double sq = 0.0, se = 0.0;
            for (int t = s0; t < s1; ++t) {
                // (interpolate = 0: q is p on the voiced frames and an exact 0 elsewhere - the sum over the span IS the sum over its
                // voiced frames)
                sq += q[t];
                se += e[t];
                nv += VOICED(t);
            }
            const int len = s1 - s0, np = a.interpolate ? len : nv;
            if (np > 0) pitch = (float)(sq / (double)np);
            if (len > 0) energy = (float)(se / (double)len);
            unvoiced_chars += nv == 0;
        }
        cp[n] = pitch; ce[n] = energy; cv[n] = nv;
    }

    // 5. the utterance's sums
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, (double)unvoiced_chars};    // voiced, p, p^2, q, q^2, e, e^2, unvoiced chars
    for (int t = tid; t < Fb; t += 256) {
        const double qt = q[t], et = e[t];
        if (VOICED(t)) { s[0] += 1.0; s[1] += qt; s[2] += qt * qt; }
        s[3] += qt; s[4] += qt * qt;
        s[5] += et; s[6] += et * et;
    }
    t2m_sums_to_thread0(s, red);
    if (tid == 0) {
        stats[0] = (double)Fb;
        for (int k = 0; k < 7; ++k) stats[1 + k] = s[k];
        stats[8] = consistent; stats[9] = s[7];
    }
#undef VOICED
}

}  // namespace

extern "C" int t2_char_variance(const T2CharVariance* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->f0 && a->mel && a->dur && a->chars_len && a->frames_len && a->char_pitch && a->char_energy && a->char_voiced &&
               a->stats, "t2_char_variance: null");
    T2_REQUIRE(a->B >= 1 && a->T >= 1 && a->L >= 1 && a->M >= 1, "t2_char_variance: need B, T, L, M >= 1");
    T2_REQUIRE(a->T <= T2_VAR_MAX_T, "t2_char_variance: T above T2_VAR_MAX_T (4096)");
    T2_REQUIRE(a->L <= T2_VAR_MAX_L, "t2_char_variance: L above T2_VAR_MAX_L (4096)");
    T2_REQUIRE((a->log_pitch == 0 || a->log_pitch == 1) && (a->interpolate == 0 || a->interpolate == 1),
               "t2_char_variance: log_pitch and interpolate must be 0 or 1");
    T2_REQUIRE(a->ld_f0 >= a->T && a->ld_dur >= a->L, "t2_char_variance: need ld_f0 >= T and ld_dur >= L");
    T2_REQUIRE(a->ld_t >= a->M && (a->B == 1 || a->ld_b >= (int64_t)(a->T - 1) * a->ld_t + a->M),
               "t2_char_variance: need ld_t >= M and ld_b >= (T-1)*ld_t + M");
    const size_t bytes = variance_lds_bytes(a->T, a->L);
    T2_REQUIRE(t2_allow_lds(char_variance_kernel, bytes), "t2_char_variance: LDS request refused");
    hipLaunchKernelGGL(char_variance_kernel, dim3((unsigned)a->B), dim3(256), bytes, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
