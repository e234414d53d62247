// wn_banks.h -- layout and host-side packing of the GEMM-ready weight banks (plain C++17, no HIP: tests/test_banks_host.py builds it with g++).
//
// The fp32 bank IS the packed parameter array of the training step (include/wn_abi.h: wn_train_layout, where the layouts of its sections are
// written down); wn_forward / wn_prime read the same sections.  The bf16 bank holds the matrices of the forward once more as [N][K] row-major
// bf16 (K contiguous: the weights' natural (out, in) layout), for wn_set_forward_precision; the filter/gate matrix of a layer is [2D][k*R], column tap*R + r, tap 0 the oldest.
#ifndef WN_BANKS_H
#define WN_BANKS_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/wn_abi.h"
#include "wn_plan.h"

// the bf16 forms of the forward and the training step need kernel_size 2 and channel counts that are multiples of 32
static inline bool wn_bank_ok(const WnPlan& s) { return s.k == 2 && s.R % 32 == 0 && s.D % 32 == 0 && s.S % 32 == 0 && s.E % 32 == 0 && s.C % 32 == 0; }
// inference (wn_forward / wn_score / wn_prime, fp32 operands) also takes kernel_size 3 and 4: only the filter/gate product reads the taps (wn_fwd_gemm_taps)
static inline bool wn_bank_fwd_ok(const WnPlan& s) {
    return s.k >= 2 && s.k <= 4 && s.R % 32 == 0 && s.D % 32 == 0 && s.S % 32 == 0 && s.E % 32 == 0 && s.C % 32 == 0;
}
// bf16 operands for inference (wn_set_forward_precision): kernel_size 2, and 3 and 4 (wn_fwd_gemm_taps_bf16; wn_forward / wn_score only)
static inline bool wn_bank_fwd_bf16_ok(const WnPlan& s) {
    return s.k >= 2 && s.k <= 4 && s.R % 64 == 0 && s.D % 64 == 0 && s.S % 64 == 0 && s.E % 64 == 0 && s.C % 32 == 0;
}

// the fp32 training step takes the same shapes (kernel_size 3 and 4: wn_fwd_gemm_taps / wn_bwd_gemm_taps; bf16 operands stay kernel_size 2)
static inline bool wn_bank_train_ok(const WnPlan& s) { return wn_bank_fwd_ok(s); }

static inline wn_train_layout wn_bank_layout(const WnPlan& s) {   // offsets in floats
    const int64_t NL = s.NL, R = s.R, D = s.D, S = s.S, E = s.E, C = s.C, k = s.k;
    wn_train_layout t;
    int64_t o = 0;
    t.fg = o; o += NL * k * R * 2 * D;   // (k taps: Wfg^T of a layer is [k*R][2D], tap j -- j = 0 the oldest -- in rows j*R .. (j+1)*R - 1)
    t.bfg = o; o += NL * 2 * D;
    t.res = o; o += NL * D * R;
    t.bres = o; o += NL * R;
    t.skip = o; o += NL * D * S;
    t.bskip = o; o += NL * S;
    t.bskip_total = o; o += S;
    t.w1 = o; o += S * E;
    t.b1 = o; o += E;
    t.w2 = o; o += E * C;
    t.b2 = o; o += C;
    t.start_t = o; o += C * R;   // start_t / start_b: training only (wn_forward / wn_prime read the handle's own copies)
    t.start_b = o; o += R;
    t.total = o;
    return t;
}

// bf16 copies of the forward's matrices, [N][K] row-major, K a multiple of 64; the skip banks grouped per block of G layers: [block][S][G*D]
struct WnBf16Layout {
    size_t fg = 0, res = 0, skip = 0, w1 = 0, w2 = 0, total = 0;   // offsets in bf16 elements
    int G = 1;         // layers per grouped skip product: min(layers, NL)
    bool ok = false;   // R, D, S, E multiples of 64 and G divides NL
};
static inline WnBf16Layout wn_bank_layout_bf16(const WnPlan& s) {
    const size_t NL = s.NL, R = s.R, D = s.D, S = s.S, E = s.E, C = s.C, k = s.k;
    WnBf16Layout t;
    t.G = s.layers < s.NL ? s.layers : s.NL;
    t.ok = s.R % 64 == 0 && s.D % 64 == 0 && s.S % 64 == 0 && s.E % 64 == 0 && s.NL % t.G == 0;
    size_t o = 0;
    t.fg = o; o += NL * 2 * D * k * R;   // (k taps: [NL][2D][k*R])
    t.res = o; o += NL * R * D;
    t.skip = o; o += NL * D * S;
    t.w1 = o; o += E * S;
    t.w2 = o; o += C * E;
    t.total = o;
    return t;
}

static inline void wn_transpose_start(const float* start_w, int R, int C, float* out) {   // (R, C, 1) -> start_conv^T [C][R]
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < C; ++c) out[(size_t)c * R + r] = start_w[(size_t)r * C + c];
}

// B^T [K][N] row-major per layer (see wn_forward.h).  Bias sections stay zero for a model without stack biases.
static inline std::vector<float> wn_pack_bank(const wn_train_layout& o, const WnPlan& s, const wn_weight_ptrs* w) {
    const bool has_bias = s.has_bias != 0;
    const int NL = s.NL, R = s.R, D = s.D, S = s.S, E = s.E, C = s.C, k = s.k;
    std::vector<float> fw((size_t)o.total, 0.f);
    for (int l = 0; l < NL; ++l) {
        float* fg = fw.data() + o.fg + (size_t)l * k * R * 2 * D;
        for (int ch = 0; ch < D; ++ch) {
            const int nf = 64 * (ch / 32) + (ch % 32), ng = nf + 32;  // column order [F(32) | G(32)] per 32-channel group
            for (int tap = 0; tap < k; ++tap)
                for (int r = 0; r < R; ++r) {
                    fg[(size_t)(tap * R + r) * 2 * D + nf] = w->filter_w[(((size_t)l * D + ch) * R + r) * k + tap];
                    fg[(size_t)(tap * R + r) * 2 * D + ng] = w->gate_w[(((size_t)l * D + ch) * R + r) * k + tap];
                }
            if (has_bias) {
                fw[o.bfg + (size_t)l * 2 * D + nf] = w->filter_b[(size_t)l * D + ch];
                fw[o.bfg + (size_t)l * 2 * D + ng] = w->gate_b[(size_t)l * D + ch];
            }
        }
        for (int dch = 0; dch < D; ++dch) {
            for (int r = 0; r < R; ++r) fw[o.res + ((size_t)l * D + dch) * R + r] = w->res_w[((size_t)l * R + r) * D + dch];
            for (int sc = 0; sc < S; ++sc) fw[o.skip + ((size_t)l * D + dch) * S + sc] = w->skip_w[((size_t)l * S + sc) * D + dch];
        }
        if (has_bias) {
            for (int r = 0; r < R; ++r) fw[o.bres + (size_t)l * R + r] = w->res_b[(size_t)l * R + r];
            for (int sc = 0; sc < S; ++sc) {
                fw[o.bskip + (size_t)l * S + sc] = w->skip_b[(size_t)l * S + sc];
                fw[o.bskip_total + sc] += w->skip_b[(size_t)l * S + sc];  // the grouped skip GEMM adds all biases once
            }
        }
    }
    for (int sc = 0; sc < S; ++sc)
        for (int e = 0; e < E; ++e) fw[o.w1 + (size_t)sc * E + e] = w->end1_w[(size_t)e * S + sc];
    for (int e = 0; e < E; ++e) fw[o.b1 + e] = w->end1_b[e];
    for (int e = 0; e < E; ++e)
        for (int c = 0; c < C; ++c) fw[o.w2 + (size_t)e * C + c] = w->end2_w[(size_t)c * E + e];
    for (int c = 0; c < C; ++c) fw[o.b2 + c] = w->end2_b[c];
    wn_transpose_start(w->start_w, R, C, fw.data() + o.start_t);
    if (has_bias) memcpy(fw.data() + o.start_b, w->start_b, (size_t)R * 4);
    return fw;
}

static inline unsigned short wn_bf16_rne(float x) {   // round to nearest even (finite inputs)
    unsigned u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// `fw`: the packed fp32 bank (its filter/gate section is transposed here; the others come from the caller's arrays, which are [N][K] already)
static inline std::vector<unsigned short> wn_pack_bank_bf16(const WnBf16Layout& ob, const wn_train_layout& o, const WnPlan& s, const std::vector<float>& fw,
                                                            const wn_weight_ptrs* w) {
    const int NL = s.NL, R = s.R, D = s.D, S = s.S, E = s.E, C = s.C, G = ob.G, KR = s.k * s.R;
    std::vector<unsigned short> wb(ob.total, 0);
    for (int l = 0; l < NL; ++l) {
        for (int n = 0; n < 2 * D; ++n)  // packed column n of layer l = row n here; k = tap*R + ch
            for (int k = 0; k < KR; ++k)
                wb[ob.fg + ((size_t)l * 2 * D + n) * KR + k] = wn_bf16_rne(fw[o.fg + (size_t)l * KR * 2 * D + (size_t)k * 2 * D + n]);
        for (int r = 0; r < R; ++r)
            for (int dch = 0; dch < D; ++dch) wb[ob.res + ((size_t)l * R + r) * D + dch] = wn_bf16_rne(w->res_w[((size_t)l * R + r) * D + dch]);
        const int blk = l / G, li = l % G;  // skip banks are grouped per block: [block][S][G*D]
        for (int sc = 0; sc < S; ++sc)
            for (int dch = 0; dch < D; ++dch)
                wb[ob.skip + ((size_t)blk * S + sc) * G * D + (size_t)li * D + dch] = wn_bf16_rne(w->skip_w[((size_t)l * S + sc) * D + dch]);
    }
    for (size_t i = 0; i < (size_t)E * S; ++i) wb[ob.w1 + i] = wn_bf16_rne(w->end1_w[i]);
    for (size_t i = 0; i < (size_t)C * E; ++i) wb[ob.w2 + i] = wn_bf16_rne(w->end2_w[i]);
    return wb;
}

#endif  // WN_BANKS_H
