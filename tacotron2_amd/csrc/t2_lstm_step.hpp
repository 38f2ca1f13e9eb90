// Kernel-side operand blocks of one LSTM cell step (forward and backward) and their host-side checks and conversions from the
// C ABI structs; the kernels that read them are in t2_lstm.hip.
#pragma once
#include "t2_common.hpp"

struct Seg { const float* x; long ldx; const float* w; long ldw; int K; };
struct LstmK {
    int B, H, nseg;
    Seg seg[3];
    const float* wpacked;               // optional: [H/4][NT][64 lanes][4] lane-contiguous weight stream
    const float* pre; long ldpre;
    const float* bias1; const float* bias2;
    const float* c_prev; long ldc_prev;
    const float* drop; long lddrop;
    float* h_out; long ldh;
    float* h_out2; long ldh2;
    float* c_out; long ldc_out;
    float* gates_out; long ldg;
    const int32_t* len; int t;
    const float* xt; long xt_cs;        // x16-tiled input (chunk stride Bp*16 floats) or null
    int xt_rows;                        // tiled rows that exist from this row block's first row (round_up(B_total, 16) - b0)
    float* ht_out; int ht_col0;
    const float* zone_h; long ldzh;     // zoneout masks and the previous h (all null = off)
    const float* zone_c; long ldzc;
    const float* h_prev; long ldhp;
};
struct LstmK2 { LstmK s[2]; };

inline int t2_lstm_check_step(const T2LstmStep& s) {
    T2_REQUIRE(s.B >= 1 && s.H >= 4 && s.H % 4 == 0, "lstm step: need B >= 1 and H % 4 == 0");
    T2_REQUIRE(s.nseg >= 0 && s.nseg <= 3, "lstm step: 0..3 input segments");
    for (int i = 0; i < s.nseg; ++i) {
        T2_REQUIRE(s.seg[i].K % 16 == 0 && s.seg[i].K > 0, "lstm step: segment K must be a multiple of 16");
        T2_REQUIRE(s.seg[i].ldx % 4 == 0 && t2_aligned16(s.seg[i].x), "lstm step: segment x must be 16-byte aligned");
        T2_REQUIRE(s.wpacked || (s.seg[i].ldw % 4 == 0 && t2_aligned16(s.seg[i].w)),
                   "lstm step: segment weights must be 16-byte aligned");
    }
    T2_REQUIRE(s.h_out != nullptr, "lstm step: h_out required");
    T2_REQUIRE((!s.xt && !s.ht_out) || (s.wpacked && s.nseg == 1), "lstm step: x16-tiled operands need the packed single-segment path");
    T2_REQUIRE(!s.xt || t2_aligned16(s.xt), "lstm step: xt must be 16-byte aligned");
    T2_REQUIRE(!s.ht_out || s.ht_col0 >= 0, "lstm step: ht_col0 must be >= 0");
    if (s.zone_h || s.zone_c) {
        T2_REQUIRE(s.h_prev != nullptr, "lstm step: zone masks need h_prev");
        T2_REQUIRE(s.len == nullptr, "lstm step: zone masks do not combine with len");
    }
    return T2_OK;
}

inline void t2_lstm_to_k(const T2LstmStep& s, LstmK& k, int b0, int bn) {
    k.B = bn; k.H = s.H; k.nseg = s.nseg;
    for (int i = 0; i < 3; ++i) {
        k.seg[i].x = (i < s.nseg && s.seg[i].x) ? s.seg[i].x + (long)b0 * s.seg[i].ldx : nullptr;
        k.seg[i].ldx = s.seg[i].ldx; k.seg[i].w = s.seg[i].w; k.seg[i].ldw = s.seg[i].ldw; k.seg[i].K = s.seg[i].K;
    }
    k.wpacked = s.wpacked;
    k.pre = s.pre ? s.pre + (long)b0 * s.ldpre : nullptr; k.ldpre = s.ldpre;
    k.bias1 = s.bias1; k.bias2 = s.bias2;
    k.c_prev = s.c_prev ? s.c_prev + (long)b0 * s.ldc_prev : nullptr; k.ldc_prev = s.ldc_prev;
    k.drop = s.drop ? s.drop + (long)b0 * s.lddrop : nullptr; k.lddrop = s.lddrop;
    k.h_out = s.h_out + (long)b0 * s.ldh; k.ldh = s.ldh;
    k.h_out2 = s.h_out2 ? s.h_out2 + (long)b0 * s.ldh2 : nullptr; k.ldh2 = s.ldh2;
    k.c_out = s.c_out ? s.c_out + (long)b0 * s.ldc_out : nullptr; k.ldc_out = s.ldc_out;
    k.gates_out = s.gates_out ? s.gates_out + (long)b0 * s.ldg : nullptr; k.ldg = s.ldg;
    k.len = s.len ? s.len + b0 : nullptr; k.t = s.t;
    k.xt_cs = (long)((s.B + 15) / 16 * 16) * 16;
    k.xt_rows = (s.B + 15) / 16 * 16 - b0;         // tiled rows that exist from this row block's first row on
    k.xt = s.xt ? s.xt + (long)b0 * 16 : nullptr;
    k.ht_out = s.ht_out ? s.ht_out + (long)b0 * 16 : nullptr; k.ht_col0 = s.ht_col0;
    const bool zoned = s.zone_h || s.zone_c;
    k.zone_h = s.zone_h ? s.zone_h + (long)b0 * s.ldzone_h : nullptr; k.ldzh = s.ldzone_h;
    k.zone_c = s.zone_c ? s.zone_c + (long)b0 * s.ldzone_c : nullptr; k.ldzc = s.ldzone_c;
    k.h_prev = zoned ? s.h_prev + (long)b0 * s.ldh_prev : nullptr; k.ldhp = s.ldh_prev;
}

// Backward step: dx = dgates . W over one or two K segments, then a plain store (epi 0) or the cell's pointwise backward (epi 1).
struct BwdK {
    int B, H, N4;                       // N4 = reduction length (4H of the producing cell)
    const float* dg_next; long lddg;    // [b][N4] or null (no recurrent contribution)
    const float* W; long ldw;           // element (n,u) at W[n*ldw + u]
    const float* dg2; long lddg2; const float* W2; long ldw2; int N2;   // optional second K segment
    const float* wtpacked;              // optional: [ncols/16][NCH][64 lanes][4] lane-contiguous transposed weights
    int ncols;                          // number of output columns u (H for the recurrent path)
    int epi;                            // 0: plain store of dx (+ext), 1: LSTM pointwise backward
    const float* ext1; long ldx1; const float* ext2; long ldx2;
    float* dx_out; long lddx;           // epi 0
    const float* drop; long lddrop;
    const float* gates; long ldgs;
    const float* c_prev; long ldcp; const float* c_cur; long ldcc;
    float* dc; long lddc;
    float* dg_out; long ldgo;
    float* dg_out2; long ldgo2;
    const int32_t* len; int t;
    const float* dgt; long dgt_cs; float* dgt_out;   // x16-tiled dg_next / dg_out (chunk stride Bp*16 floats)
    int off_chain;                      // T2LstmBwdStep.off_chain
    const float* zone_h; long ldzh; const float* zone_c; long ldzc;   // zoneout masks (both null = off)
    float* dhz; long lddhz;             // in/out carry of the zoned share of dh
    unsigned long long* clk;            // diagnostic build: the caller's stamp buffer (event ring, t2_common.hpp) or null
};
struct BwdK2 { BwdK s[2]; };

inline void t2_lstm_to_bk(const T2LstmBwdStep& s, BwdK& k) {
    k.B = s.B; k.H = s.H; k.N4 = s.N4;
    k.dg_next = s.dg_next; k.lddg = s.lddg; k.W = s.W; k.ldw = s.ldw; k.ncols = s.ncols; k.epi = s.epi;
    k.dg2 = s.dg2; k.lddg2 = s.lddg2; k.W2 = s.W2; k.ldw2 = s.ldw2; k.N2 = s.N2; k.dg_out2 = s.dg_out2; k.ldgo2 = s.ldgo2;
    k.wtpacked = s.wtpacked;
    k.ext1 = s.ext1; k.ldx1 = s.ldx1; k.ext2 = s.ext2; k.ldx2 = s.ldx2;
    k.dx_out = s.dx_out; k.lddx = s.lddx; k.drop = s.drop; k.lddrop = s.lddrop;
    k.gates = s.gates; k.ldgs = s.ldgs; k.c_prev = s.c_prev; k.ldcp = s.ldcp; k.c_cur = s.c_cur; k.ldcc = s.ldcc;
    k.dc = s.dc; k.lddc = s.lddc; k.dg_out = s.dg_out; k.ldgo = s.ldgo; k.len = s.len; k.t = s.t;
    k.dgt = s.dgt_next; k.dgt_out = s.dgt_out; k.dgt_cs = (long)((s.B + 15) / 16 * 16) * 16;
    k.off_chain = s.off_chain;
    k.zone_h = s.zone_h; k.ldzh = s.ldzone_h; k.zone_c = s.zone_c; k.ldzc = s.ldzone_c; k.dhz = s.dhz; k.lddhz = s.lddhz;
    k.clk = nullptr;
}

inline int t2_lstm_check_bwd(const T2LstmBwdStep& s) {
    T2_REQUIRE(s.B >= 1 && s.ncols >= 1, "lstm bwd step: empty");
    if (s.dg_next) {
        T2_REQUIRE(s.N4 % 16 == 0 && s.lddg % 4 == 0 && t2_aligned16(s.dg_next), "lstm bwd step: dg_next alignment");
        T2_REQUIRE(s.W != nullptr || s.wtpacked != nullptr, "lstm bwd step: W required with dg_next");
    }
    if (s.dg2) {
        T2_REQUIRE(s.N2 % 16 == 0 && s.lddg2 % 4 == 0 && t2_aligned16(s.dg2) && (s.W2 || s.wtpacked), "lstm bwd step: dg2 alignment");
    }
    if (s.epi == 1) {
        T2_REQUIRE(s.gates && s.c_cur && s.dc && s.dg_out && s.ncols == s.H, "lstm bwd step: epilogue operands");
        if (s.zone_h || s.zone_c) {
            T2_REQUIRE(s.dhz != nullptr, "lstm bwd step: zone masks need the carry dhz");
            T2_REQUIRE(s.len == nullptr, "lstm bwd step: zone masks do not combine with len");
        }
    } else {
        T2_REQUIRE(s.dx_out != nullptr, "lstm bwd step: dx_out required");
        T2_REQUIRE(!s.zone_h && !s.zone_c, "lstm bwd step: zone masks need the cell epilogue (epi = 1)");
    }
    return T2_OK;
}
