// Per-character durations from an alignment matrix (include/tacotron2_amd.h: t2_align_durations): how many mel frames each
// input character lasts.  An export path - milliseconds per batch - so the kernel is plain: ONE 256-thread workgroup per
// utterance, no cross-workgroup synchronisation, nothing persistent, no atomics to global memory.
//
//   monotonic (mode 1): the monotonic alignment search of Glow-TTS (Kim et al. 2020) - the best path through
//     la[s][n] = log(max(a, 1e-8)) that starts on the first character, ends on the last and stays or advances by one per
//     decoder step.  The recurrence is sequential in s and parallel in n: two fp64 rows of Q in LDS, the block strides over
//     n, one barrier per step, one predecessor byte per (s, n) to the `back` workspace.  fp64 because Q grows to ~4e4 over
//     a few thousand steps, where an fp32 ulp (4e-3) is the size of real decision margins.
//   argmax (mode 0, and the fall-back of an utterance with fewer steps than characters): one wave per step finds the lowest
//     position of the row's maximum.
// Both modes make the argmax pass (focus rate, agreement with the argmax).  The counts are LDS integers (they reuse the Q
// rows once the recurrence is done); the block writes them out as dur.
#include "t2_measure.hpp"

namespace {

__device__ __forceinline__ double la_of(float a) { return log((double)fmaxf(a, 1e-8f)); }

// dynamic LDS: [0, 64) 8 doubles of wave partials; then mode 1: Q[2][L] doubles, mode 0: L ints.  cnt[L] ints alias Q.
__global__ __launch_bounds__(256) void align_durations_kernel(T2AlignDur a) {
    extern __shared__ double lds[];
    double (*red)[4] = reinterpret_cast<double (*)[4]>(lds);         // [2][4 waves]
    double* Q = lds + 8;
    int* cnt = reinterpret_cast<int*>(lds + 8);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.L, r = a.r;
    const int Nb = min(max(a.chars_len[b], 0), L);
    const long Fcap = (long)r * a.S;
    const int Fb = (int)min((long)max(a.frames_len[b], 0), Fcap);
    const int Sb = (Fb + r - 1) / r;
    int32_t* dur = a.dur + (long)b * a.ld_dur;
    float* stats = a.stats + (long)b * 4;
    if (Nb == 0 || Sb == 0) {
        for (int n = tid; n < L; n += 256) dur[n] = 0;
        if (tid < 4) stats[tid] = 0.f;
        return;
    }
    const float* al = a.align + (long)b * a.ld_b;
    const int64_t lds_ = a.ld_s;
    const bool feasible = Sb >= Nb;
    const bool mono = a.mode == 1 && feasible;
    uint8_t* back = mono ? a.back + (long)b * a.S * L : nullptr;
    const int wlast = Fb - r * (Sb - 1);          // frames of the last step (1 .. r)

    if (mono) {
        // Q[0][0] = la[0][0], Q[0][n > 0] = -inf; Q[s][n] = la[s][n] + max(Q[s-1][n], Q[s-1][n-1]), advance only when strictly better
        const double ninf = -__builtin_inf();
        for (int n = tid; n < Nb; n += 256) {
            Q[n] = n == 0 ? la_of(al[0]) : ninf;
            back[n] = 0;
        }
        __syncthreads();
        for (int s = 1; s < Sb; ++s) {
            const double* Qp = Q + (long)((s - 1) & 1) * L;
            double* Qc = Q + (long)(s & 1) * L;
            const float* row = al + s * lds_;
            uint8_t* brow = back + (long)s * L;
            for (int n = tid; n < Nb; n += 256) {
                const double q0 = Qp[n], q1 = n > 0 ? Qp[n - 1] : ninf;
                const bool adv = q1 > q0;
                Qc[n] = la_of(row[n]) + (adv ? q1 : q0);
                brow[n] = adv ? 1 : 0;
            }
            __syncthreads();      // one barrier per step: row (s & 1) is complete, row ((s - 1) & 1) is free for step s + 1
        }
    }
    // (mono: every thread is past the last barrier of the recurrence - the Q rows are dead, their LDS becomes the counts)
    for (int n = tid; n < Nb; n += 256) cnt[n] = 0;
    __syncthreads();

    // argmax pass, one wave per step: the row's maximum (focus rate) and its lowest position
    double sum[2] = {0.0, 0.0};                    // focus, lasum: lane 0 of every wave adds, the other lanes hold 0
    for (int s = w; s < Sb; s += 4) {
        const float* row = al + s * lds_;
        float v = -__builtin_inff();
        int i = 0x7fffffff;
        for (int n = lane; n < Nb; n += 64) {
            const float x = row[n];
            if (x > v || i == 0x7fffffff) { v = x; i = n; }
        }
        t2m_wave_pick(v, i, [](float ov, int oi, float mv, int mi) {
            return oi != 0x7fffffff && (mi == 0x7fffffff || ov > mv || (ov == mv && oi < mi));
        });
        if (lane == 0) {
            sum[0] += (double)v;
            if (mono) {
                back[(long)s * L + i] |= 2;       // bit 1: this cell is the step's argmax (read by the backtrack below)
            } else {
                atomicAdd(&cnt[i], s < Sb - 1 ? r : wlast);
                sum[1] += la_of(v);
            }
        }
    }
    t2m_sums_to_thread0(sum, red);

    if (tid == 0) {
        double focus = sum[0], lasum = sum[1];
        int agree = Sb;
        if (mono) {               // backtrack from (Sb - 1, Nb - 1)
            agree = 0;
            int n = Nb - 1;
            for (int s = Sb - 1; s >= 0; --s) {
                const uint8_t f = back[(long)s * L + n];
                cnt[n] += s < Sb - 1 ? r : wlast;
                lasum += la_of(al[s * lds_ + n]);
                agree += (f >> 1) & 1;
                n -= f & 1;
            }
        }
        const double inv = 1.0 / (double)Sb;
        stats[0] = (float)(focus * inv);
        stats[1] = (float)(lasum * inv);
        stats[2] = feasible ? 1.f : 0.f;
        stats[3] = (float)((double)agree * inv);
    }
    __syncthreads();
    for (int n = tid; n < L; n += 256) dur[n] = n < Nb ? cnt[n] : 0;
}

}  // namespace

extern "C" int t2_align_durations(const T2AlignDur* a, void* stream) {
    (void)hipGetLastError();   // drop stale sticky errors of other HIP users in this thread: only OUR launches are checked
    T2_REQUIRE(a && a->align && a->chars_len && a->frames_len && a->dur && a->stats, "t2_align_durations: null");
    T2_REQUIRE(a->B >= 1 && a->S >= 1 && a->L >= 1, "t2_align_durations: need B, S, L >= 1");
    T2_REQUIRE(a->L <= T2_ALIGN_MAX_L, "t2_align_durations: L above T2_ALIGN_MAX_L (4096)");
    T2_REQUIRE(a->r >= 1, "t2_align_durations: need r >= 1");
    T2_REQUIRE(a->mode == 0 || a->mode == 1, "t2_align_durations: mode must be 0 (argmax) or 1 (monotonic)");
    T2_REQUIRE(a->mode == 0 || a->back, "t2_align_durations: monotonic mode needs the back workspace [B][S][L]");
    T2_REQUIRE(a->ld_s >= a->L && (a->B == 1 || a->ld_b >= (int64_t)(a->S - 1) * a->ld_s + a->L) && a->ld_dur >= a->L,
               "t2_align_durations: need ld_s >= L, ld_b >= (S-1)*ld_s + L, ld_dur >= L");
    const size_t bytes = 64 + (a->mode == 1 ? 16 : 4) * (size_t)a->L;
    T2_REQUIRE(t2_allow_lds(align_durations_kernel, bytes), "t2_align_durations: LDS request refused");
    hipLaunchKernelGGL(align_durations_kernel, dim3((unsigned)a->B), dim3(256), bytes, ST, *a);
    T2_CHECK_LAUNCH(); return T2_OK;
}
