// wn_plan.h -- host-side planner and weight packer + the POD structs shared with the kernel.
//
// The generation engine is a SYSTOLIC CHAIN of persistent workgroups (one per CU):
//
//     L0[c] -> L1[c] -> ... -> L(NL-1)[c] -> HEAD[h] -> back to L0 (sampled index feeds start_conv)
//
// Every layer of the reference's stack (wavenet_model.py:131-165) is owned by P workgroups ("layer
// split"), the two end convs (:167-169) by PA workgroups ("head split").  Each workgroup keeps its slice
// of the fp32 weight banks STATIONARY in its CU's LDS for the whole generate_fast() call, owns the
// dilation queue (wavenet_modules.py:42-77) of its layer, and exchanges only activations with its
// neighbours through 8-byte {tag,value} granules in HBM (MI355X guide: "R2, the data IS the flag").
//
// Split of one layer across its P workgroups (c = 0..P-1, Dc = ceil(D/P) gated channels each):
//   filter/gate (wavenet_model.py:147-151): ROW split  -- WG c computes channels [c*Dc, (c+1)*Dc) of
//       tanh(Wf.[x[t-d];x[t]]) * sigmoid(Wg.[...]); it needs the full layer input x[t] (R floats).
//   residual 1x1 (:164-165) and skip 1x1 (:154-162): K split -- WG c multiplies ITS Dc channels of z into
//       partial sums for all R (resp. S) outputs; the consumer adds the P partials in fixed order c=0..P-1
//       (WG 0's partial also carries the "+ x[t]" residual add and the conv bias).
//   The running skip sum travels down the chain in P independent lanes; the head adds the lanes.
// Head WG h: rows [h*Ec,(h+1)*Ec) of end_conv_1 (+bias, ReLU) then the matching K-slice of end_conv_2,
//   publishing partial logits; every L0 workgroup adds the PA partials, applies regulariser/temperature,
//   softmax + inverse-CDF sampling (or argmax) redundantly and bit-identically, and gathers the
//   start_conv column of the sampled class (wavenet_model.py:127 on a one-hot == column gather).
#ifndef WN_PLAN_H
#define WN_PLAN_H

#include <stdint.h>

#define WN_THREADS 256
#define WN_SAMPLER_GROUPS 16
#define WN_LDS_MAX_BYTES (163840 - 1024) /* 160 KiB per CU on gfx950, minus the static LDS __syncthreads_or() uses */

typedef unsigned long long wn_u64;

// One packed matrix-vector product  out[row] = sum_k W[row][k] * x[k],  rows Nr, reduction K.
// 256 threads; T threads cooperate on a row (T a power of two), each owning J float4 of that row per
// pass; a pass covers 256/T rows.  LDS image: float4 W4[(pass*J + j)*256 + tid] -- every ds_read_b128
// of a wave is lane-linear (conflict-free); thread tid holds row pass*(256/T) + tid/T and the k-range
// 4*(j*T + tid%T) .. +3.  x must provide xlen = J*T*4 floats (zero padded).
struct WnMatvec {
    int32_t Nr, K, T, J, passes;
    int32_t off4;  // offset of the image inside the workgroup's LDS blob, in float4 units
    int32_t xlen;  // floats of x consumed (zero padded tail)
    int32_t n4;    // float4 count of the image = passes*J*256
};

struct WnPlan {
    // model (wavenet_model.py:28-39)
    int32_t layers, blocks, NL, R, D, S, E, C, k, has_bias;
    int32_t n_streams;
    // chain geometry
    int32_t P, PA, Dc, Ec, n_wg;
    int32_t HR;  // replicas of the PA head workgroups (wave-specialised kernel: replica j serves the streams s = j mod HR); 1 elsewhere
    WnMatvec fg, res, skip, end1, end2;
    // LDS layout of a layer workgroup (float offsets; blob first)
    int32_t l_bias_fg, l_bias_res, l_bias_skip;  // inside the blob, valid iff has_bias
    int32_t l_xs, l_fgout, l_z, l_xt, l_skin, l_red, l_smp, l_total;
    // LDS layout of a head workgroup
    int32_t h_b1, h_b2, h_sk, h_ev, h_red, h_total;
    int32_t blob_layer_floats, blob_head_floats;  // multiples of 4
    int32_t lds_floats;                           // max(l_total, h_total)
    int32_t red_floats;
    // device tables / buffers
    const float* blobs;       // layer WG w: blobs + w*blob_layer_floats ; head h: blobs + NL*P*blob_layer + h*blob_head
    const float* start_t;     // [C][R] start_conv.weight transposed: column gather = one contiguous row
    const float* start_b;     // [R] or NULL
    const int32_t* dil;       // [NL] dilation of each layer (wavenet_model.py:70-110)
    const int64_t* ring_off;  // [NL] float offset of the layer's queue rings inside `rings`
    const int32_t* wg_map;    // [n_wg] blockIdx -> chain position
    float* rings;             // layer l, copy c, stream s: ring_off[l] + (c*n_streams+s)*ML*R ; ML=(k-1)*d+1
    wn_u64* gx;               // x' partials   [(NL*P)][n_streams][R]
    wn_u64* gs;               // skip lanes    [(NL*P)][n_streams][S]
    wn_u64* gl;               // partial logits[PA][n_streams][C]
    wn_u64* gi;               // sampled class index per stream [n_streams] (multi-stream kernel: samplers -> L0)
    wn_u64* g0;               // variant 3: layer 0's input, the start_conv row of the sampled class [n_streams][R] (samplers -> L0)
    int32_t n_smp;            // dedicated sampler workgroups (0 in the single-stream kernels)
    int32_t start_in_lds;     // v2 single-stream: layer 0 holds start_conv^T in LDS
    uint32_t* status;         // [8] 0: abort code, 1: chain position, 2: eval, 3: stream, 4: where, 5: residency count, 6-7: the log-probability output pointer (WnRun::logp)
                              // (behind xcc_tab, at word WN_STATUS_FORCED(n_wg): the forced samples' pointer of an armed job -- wn_forced_in, wn_kernel.h)
    uint32_t* xcc_tab;        // [n_wg] XCC id + 1 of every chain position, written by the workgroups at start
    int32_t n_blocks;         // grid size (>= n_wg; blocks mapped to -1 exit at once)
    int32_t allow_plain;      // same-XCD producers may publish with L2-resident (non write-through) stores
    // chain positions: [0, n_lw) layer-role workgroups, then PA * HR head workgroups, then the samplers.  Variant 3: n_lw = NL * P
    // (one layer slice each); variant 4: n_lw stack workgroups of LPW consecutive layers each (wn_kernel_v4.h)
    int32_t n_lw, LPW;
    int64_t head_blob_off;    // float offset of head workgroup 0's weight image inside `blobs` (variants 3 and 4)
};

struct WnRun {
    const int32_t* first;  // [n_streams][n_given]
    int64_t n_given, num_samples, n_eval, t_base;
    float temperature;
    int32_t greedy;
    const float* reg;
    const double* uniforms;
    int32_t* out_idx;
    float* dbg_logits;
    int64_t timeout_ticks;  // wall_clock64 ticks
    long long* prof;        // optional [n_wg][prof_items][4] wall-clock stamps (diagnostics), or NULL
    int32_t prof_items;
    int32_t logp;               // bits 0-1 (WN_RUN_LOGP_MASK): per-sample log-probabilities (wn_set_logprob_output, include/wn_abi.h): 0 = off, else 1 + WN_LOGP_*
                                // (1: of the distribution the draw was made from, 2: of the step's summed logits).  Bit 2 (WN_RUN_FORCED): the job is armed with forced
                                // samples (wn_set_forced_samples).  The former padding word: WnRun keeps its size and every offset.  The pointers do not fit here: the
                                // host puts them into the status block (WnPlan::status) ahead of the launch -- wn_logp_out, wn_forced_in, wn_kernel.h
    const float* stream_temps;  // optional [n_streams]: per-stream temperature (<= 0: that stream is greedy); NULL = `temperature` for all
    int64_t resident_ticks;     // bound of the start-up residency barrier (wn_resident_barrier), wall_clock64 ticks
    // sampling filters (wn_set_sampling, include/wn_abi.h), normalised by the host: 0 = off.  APPENDED: WnRun is the kernels' last argument, so no offset
    // of an existing argument moves, and a zero-filled run means "no filter"
    int32_t top_k;              // 1 .. C-1: keep the classes x_i >= the k-th largest x (ties at the threshold all stay)
    float top_p;                // (0, 1): of those, keep class i iff the mass of the classes with x_j > x_i is < top_p * the survivors' mass
};

#define WN_RUN_LOGP_MASK 3
#define WN_RUN_FORCED 4
// The status block is 8 words, the n_wg words of xcc_tab and, 8-byte aligned behind them, the two words of the forced samples' pointer
#define WN_STATUS_FORCED(n_wg) (8 + (((n_wg) + 1) & ~1))
#define WN_STATUS_WORDS(n_wg) (WN_STATUS_FORCED(n_wg) + 2)

// ---- host-side planner / packer (plain C++; also parsed, unused, in the device pass) ----
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/wn_abi.h"

static inline int wn_pow2floor(int v) { int p = 1; while (p * 2 <= v) p *= 2; return p; }
static inline int wn_pow2ceil(int v) { int p = 1; while (p < v) p *= 2; return p; }
static inline int wn_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int wn_round4(int v) { return (v + 3) & ~3; }
static inline int wn_smp_floats(int C) { return 5 * wn_round4(C) + 8 * WN_SAMPLER_GROUPS + 16; }  // floats of the sampler scratch (wn_kernel.h WnSmp)

static inline WnMatvec wn_make_matvec(int Nr, int K, int off4) {
    WnMatvec m;
    m.Nr = Nr; m.K = K;
    const int K4 = wn_cdiv(K, 4);
    int T = Nr >= WN_THREADS ? 1 : wn_pow2floor(WN_THREADS / Nr);
    const int tmax = wn_pow2ceil(K4);
    if (T > tmax) T = tmax;
    if (T > 64) T = 64;
    m.T = T;
    m.J = wn_cdiv(K4, T);
    m.passes = wn_cdiv(Nr, WN_THREADS / T);
    m.off4 = off4;
    m.xlen = m.J * T * 4;
    m.n4 = m.passes * m.J * WN_THREADS;
    return m;
}

// dst: float image of m (m.n4*4 floats); W(row,k) -> weight or 0 outside the matrix
static inline void wn_pack_matvec(float* dst, const WnMatvec& m, const std::function<float(int, int)>& W) {
    const int rpp = WN_THREADS / m.T;
    for (int p = 0; p < m.passes; ++p)
        for (int j = 0; j < m.J; ++j)
            for (int tid = 0; tid < WN_THREADS; ++tid) {
                const int row = p * rpp + tid / m.T, q = tid % m.T;
                for (int i = 0; i < 4; ++i) {
                    const int kk = (j * m.T + q) * 4 + i;
                    dst[((size_t)(p * m.J + j) * WN_THREADS + tid) * 4 + i] = (row < m.Nr && kk < m.K) ? W(row, kk) : 0.f;
                }
            }
}

// Fills the geometry part of the plan for a given split; returns LDS bytes needed.
static inline int64_t wn_plan_geometry(WnPlan& pl, int P, int PA) {
    pl.P = P; pl.PA = PA; pl.HR = 1;
    pl.Dc = wn_cdiv(pl.D, P);
    pl.Ec = wn_cdiv(pl.E, PA);
    pl.n_wg = pl.NL * P + PA;
    int off4 = 0;
    pl.fg = wn_make_matvec(2 * pl.Dc, pl.k * pl.R, off4); off4 += pl.fg.n4;
    pl.res = wn_make_matvec(pl.R, pl.Dc, off4); off4 += pl.res.n4;
    pl.skip = wn_make_matvec(pl.S, pl.Dc, off4); off4 += pl.skip.n4;
    int o = off4 * 4;
    pl.l_bias_fg = pl.l_bias_res = pl.l_bias_skip = -1;
    if (pl.has_bias) {
        pl.l_bias_fg = o; o += wn_round4(2 * pl.Dc);
        pl.l_bias_res = o; o += wn_round4(pl.R);
        pl.l_bias_skip = o; o += wn_round4(pl.S);
    }
    pl.blob_layer_floats = o;
    int passes = pl.fg.passes;
    if (pl.res.passes > passes) passes = pl.res.passes;
    if (pl.skip.passes > passes) passes = pl.skip.passes;
    // head
    int hoff4 = 0;
    pl.end1 = wn_make_matvec(pl.Ec, pl.S, hoff4); hoff4 += pl.end1.n4;
    pl.end2 = wn_make_matvec(pl.C, pl.Ec, hoff4); hoff4 += pl.end2.n4;
    int ho = hoff4 * 4;
    pl.h_b1 = ho; ho += wn_round4(pl.Ec);
    pl.h_b2 = ho; ho += wn_round4(pl.C);
    pl.blob_head_floats = ho;
    if (pl.end1.passes > passes) passes = pl.end1.passes;
    if (pl.end2.passes > passes) passes = pl.end2.passes;
    pl.red_floats = passes * WN_THREADS;
    // layer scratch
    pl.l_xs = o; o += wn_round4(pl.fg.xlen > pl.k * pl.R ? pl.fg.xlen : pl.k * pl.R);
    pl.l_fgout = o; o += wn_round4(2 * pl.Dc);
    int zlen = pl.res.xlen > pl.skip.xlen ? pl.res.xlen : pl.skip.xlen;
    if (zlen < pl.Dc) zlen = pl.Dc;
    pl.l_z = o; o += wn_round4(zlen);
    pl.l_xt = o; o += wn_round4(pl.R);
    // skin + red double as the sampler scratch of the L0 workgroups (never live at the same time)
    // sampler scratch: lgt,xsm,pp floats (3*C4) + pd doubles (2*C4) + per-group partials (see wn_kernel.h WnSmp)
    const int smp_floats = wn_smp_floats(pl.C);
    pl.l_skin = o;
    pl.l_smp = o;
    int region = wn_round4(pl.S) + pl.red_floats;
    if (region < smp_floats) region = smp_floats;
    pl.l_red = o + wn_round4(pl.S);
    o += region;
    pl.l_total = o;
    // head scratch
    pl.h_sk = ho; ho += wn_round4(pl.end1.xlen > pl.S ? pl.end1.xlen : pl.S);
    pl.h_ev = ho; ho += wn_round4(pl.end2.xlen > pl.Ec ? pl.end2.xlen : pl.Ec);
    pl.h_red = ho; ho += pl.red_floats;
    pl.h_total = ho;
    pl.lds_floats = pl.l_total > pl.h_total ? pl.l_total : pl.h_total;
    return (int64_t)pl.lds_floats * 4;
}

// Chooses (P, PA): the smallest splits whose LDS image fits one CU, within the CU budget.
// forced_P / forced_PA > 0 override.  Returns empty string on success, else a reason.
static inline std::string wn_plan_choose(WnPlan& pl, int n_cu, int forced_P, int forced_PA) {
    int bestP = -1, bestPA = -1;
    const int p_lo = forced_P > 0 ? forced_P : 1, p_hi = forced_P > 0 ? forced_P : pl.D;
    for (int P = p_lo; P <= p_hi; ++P) {
        if (forced_P <= 0 && P > 1 && wn_cdiv(pl.D, P) == wn_cdiv(pl.D, P - 1)) continue;  // same Dc: no gain
        WnPlan t = pl;
        // layer part only depends on P: probe with a head split that certainly fits
        wn_plan_geometry(t, P, pl.E);
        if ((int64_t)t.l_total * 4 <= WN_LDS_MAX_BYTES) { bestP = P; break; }
    }
    if (bestP < 0) return "no layer split fits the 160 KiB LDS of one CU";
    const int a_lo = forced_PA > 0 ? forced_PA : 1, a_hi = forced_PA > 0 ? forced_PA : pl.E;
    for (int PA = a_lo; PA <= a_hi; ++PA) {
        if (forced_PA <= 0 && PA > 1 && wn_cdiv(pl.E, PA) == wn_cdiv(pl.E, PA - 1)) continue;
        WnPlan t = pl;
        wn_plan_geometry(t, bestP, PA);
        if ((int64_t)t.h_total * 4 <= WN_LDS_MAX_BYTES) { bestPA = PA; break; }
    }
    if (bestPA < 0) return "no head split fits the 160 KiB LDS of one CU";
    const int64_t lds = wn_plan_geometry(pl, bestP, bestPA);
    if (lds > WN_LDS_MAX_BYTES) return "LDS image does not fit";
    if (n_cu > 0) {
        const int per_cu = (int)(WN_LDS_MAX_BYTES / lds) > 0 ? (int)(WN_LDS_MAX_BYTES / lds) : 1;
        const int cap = n_cu * (per_cu > 4 ? 4 : per_cu);
        if (pl.n_wg > cap)
            return "the chain needs " + std::to_string(pl.n_wg) + " co-resident workgroups but the device admits only " +
                   std::to_string(cap);
    }
    return std::string();
}

struct WnHostWeights {  // host pointers, reference layout (see include/wn_abi.h wn_weight_ptrs)
    const float *start_w, *start_b, *filter_w, *filter_b, *gate_w, *gate_b, *res_w, *res_b, *skip_w, *skip_b, *end1_w,
        *end1_b, *end2_w, *end2_b;
};

// Builds all per-workgroup LDS images: [NL*P layer blobs][PA head blobs].
static inline void wn_pack_blobs(const WnPlan& pl, const WnHostWeights& w, std::vector<float>& out) {
    const int R = pl.R, D = pl.D, S = pl.S, E = pl.E, C = pl.C, k = pl.k, Dc = pl.Dc, Ec = pl.Ec;
    out.assign((size_t)pl.NL * pl.P * pl.blob_layer_floats + (size_t)pl.PA * pl.blob_head_floats, 0.f);
    for (int l = 0; l < pl.NL; ++l)
        for (int c = 0; c < pl.P; ++c) {
            float* b = out.data() + ((size_t)l * pl.P + c) * pl.blob_layer_floats;
            const float* fw = w.filter_w + (size_t)l * D * R * k;
            const float* gw = w.gate_w + (size_t)l * D * R * k;
            const float* rw = w.res_w + (size_t)l * R * D;
            const float* sw = w.skip_w + (size_t)l * S * D;
            // rows 0..Dc-1: filter channel c*Dc+row ; rows Dc..2Dc-1: gate.  k index kk = tap*R + ch:
            // tap 0 multiplies x[t-(k-1)d] ... tap k-1 multiplies x[t]  (Appendix A item 1)
            wn_pack_matvec(b + (size_t)pl.fg.off4 * 4, pl.fg, [&](int row, int kk) -> float {
                const bool gate = row >= Dc;
                const int ch_out = c * Dc + (gate ? row - Dc : row);
                if (ch_out >= D) return 0.f;
                const int tap = kk / R, ch = kk % R;
                return (gate ? gw : fw)[((size_t)ch_out * R + ch) * k + tap];
            });
            wn_pack_matvec(b + (size_t)pl.res.off4 * 4, pl.res, [&](int row, int kk) -> float {
                const int ch = c * Dc + kk;
                return ch < D ? rw[(size_t)row * D + ch] : 0.f;
            });
            wn_pack_matvec(b + (size_t)pl.skip.off4 * 4, pl.skip, [&](int row, int kk) -> float {
                const int ch = c * Dc + kk;
                return ch < D ? sw[(size_t)row * D + ch] : 0.f;
            });
            if (pl.has_bias) {
                for (int i = 0; i < Dc; ++i) {
                    const int ch = c * Dc + i;
                    b[pl.l_bias_fg + i] = (ch < D && w.filter_b) ? w.filter_b[(size_t)l * D + ch] : 0.f;
                    b[pl.l_bias_fg + Dc + i] = (ch < D && w.gate_b) ? w.gate_b[(size_t)l * D + ch] : 0.f;
                }
                if (c == 0) {  // biases of the K-split convs ride on lane 0 only
                    for (int i = 0; i < R; ++i) b[pl.l_bias_res + i] = w.res_b ? w.res_b[(size_t)l * R + i] : 0.f;
                    for (int i = 0; i < S; ++i) b[pl.l_bias_skip + i] = w.skip_b ? w.skip_b[(size_t)l * S + i] : 0.f;
                }
            }
        }
    for (int h = 0; h < pl.PA; ++h) {
        float* b = out.data() + (size_t)pl.NL * pl.P * pl.blob_layer_floats + (size_t)h * pl.blob_head_floats;
        wn_pack_matvec(b + (size_t)pl.end1.off4 * 4, pl.end1, [&](int row, int kk) -> float {
            const int e = h * Ec + row;
            return e < E ? w.end1_w[(size_t)e * S + kk] : 0.f;
        });
        wn_pack_matvec(b + (size_t)pl.end2.off4 * 4, pl.end2, [&](int row, int kk) -> float {
            const int e = h * Ec + kk;
            return e < E ? w.end2_w[(size_t)row * E + e] : 0.f;
        });
        for (int i = 0; i < Ec; ++i) b[pl.h_b1 + i] = (h * Ec + i < E) ? w.end1_b[h * Ec + i] : 0.f;
        if (h == 0)
            for (int i = 0; i < C; ++i) b[pl.h_b2 + i] = w.end2_b[i];
    }
}

// ---- forms of the wave-specialised kernel (wn_kernel_v3.h), chosen per job by wn_create
// The throughput form pays once the ring holds more tokens than it has stages (one stream per item then runs into the stages' cycle):
// from n_layers + WN_V3_G2_MARGIN streams -- cfg3 (50 layers): 56 streams (895 k against 887 k samples/s; 48: 783 k against 800 k);
// cfg2 (30 layers): 36 (32 streams: 999 k against 956 k, 64: 1.53 M against 0.96 M); cfg1 (10 layers): 16.
#define WN_V3_G2_MARGIN 6
#define WN_V3_ROUND_STREAMS 128   // streams per round when a job exceeds what one chain holds (wn_handle::rounds)
// bit 0: two streams per pipeline item of a layer workgroup (needs an even stream count); bit 1: two replicas of the head
// workgroups.  `pin`: the WN_V3_MODE environment override ("0".."3"), or NULL.
static inline int wn_v3_mode_for(int n_streams, const char* pin, int n_layers = 50) {
    int mode = (n_streams >= n_layers + WN_V3_G2_MARGIN) ? 3 : 0;
    if (pin && pin[0] >= '0' && pin[0] <= '3' && !pin[1]) mode = pin[0] - '0';
    if (n_streams % 2) mode &= ~1;
    if (n_streams < 2) mode = 0;
    return mode;
}
// Skip-lane slot re-use (wn_kernel_v3.h, the skip group's NSLOT): a form of the two-streams-per-item kernel of shapes that have it (`has_form`: cfg3's), taken
// where the chain is throughput bound -- measured crossover on cfg3 (50 layers): 80 streams -2 %, 96 +1 %, 112 +4 %, 128 +6 %, 150 +2.5 %
// (profiles/r05_skip_lane_slots_by_stream_count.txt).  `pin`: the WN_V3_SLOTS environment override ("0" / "4"), or NULL.  Returns the slot count (0 = off).
static inline int wn_v3_slots_for(int n_streams, int mode, bool has_form, const char* pin, int n_layers = 50) {
    if (!has_form || !(mode & 1)) return 0;
    int slots = n_streams >= 2 * n_layers - 4 ? 4 : 0;
    if (pin && (pin[0] == '0' || pin[0] == '4') && !pin[1]) slots = pin[0] - '0';
    if (slots * 2 > n_streams) slots = 0;
    return slots;
}
// sizes of the rounds a job of n_streams > round_max streams runs in: as few rounds as possible, equal within one or two streams,
// even (two streams per pipeline item) wherever streams are left for it, none above round_max
static inline std::vector<int> wn_v3_round_sizes(int n_streams, int round_max) {
    std::vector<int> out;
    const int K = (n_streams + round_max - 1) / round_max;
    int left = n_streams;
    for (int i = 0; i < K; ++i) {
        int n = (left + (K - i) - 1) / (K - i);
        if (n % 2 && n < left && n < round_max) ++n;
        out.push_back(n);
        left -= n;
    }
    return out;
}

// blockIdx -> chain position such that consecutive chain positions share an XCD (block b is observed
// to land on XCD b % 8; a speed-only assumption -- correctness never depends on it).
static inline void wn_make_wg_map(int n_wg, int n_xcd, std::vector<int32_t>& map) {
    map.assign(n_wg, 0);
    std::vector<int> cnt(n_xcd, 0), pre(n_xcd + 1, 0);
    for (int b = 0; b < n_wg; ++b) cnt[b % n_xcd]++;
    for (int x = 0; x < n_xcd; ++x) pre[x + 1] = pre[x] + cnt[x];
    for (int b = 0; b < n_wg; ++b) map[b] = pre[b % n_xcd] + b / n_xcd;
}

// Layer-aligned placement: every layer's P workgroups (and the head's PA) sit on ONE XCD, so that most hand-offs
// stay inside one XCD's L2.  XCD 0 hosts the head, the samplers, the first layers (sampler -> L0 stays local) AND the last layer:
// the last layer's skip lanes -- S granules from each of its P slices, the widest hand-off of the ring -- reach the head without
// crossing an XCD boundary (round 3; the ring crosses as many boundaries as before, the crossing moved to the narrow x' hand-off
// in front of the last layer).
// map[b] = chain position of block b, or -1 (bystander).  Returns false if the layers do not fit that way.
static inline bool wn_make_wg_map_layers(int NL, int P, int PA, int n_smp, int n_xcd, int cu_per_xcd, std::vector<int32_t>& map,
                                         int* n_blocks) {
    if (PA + n_smp > cu_per_xcd) return false;
    // use as FEW XCDs as hold the chain: every XCD boundary the token crosses costs ~0.4 us more than a local hop
    for (int used = 1; used <= n_xcd; ++used) {
        std::vector<std::vector<int>> S(n_xcd);
        for (int h = 0; h < PA + n_smp; ++h) S[0].push_back(NL * P + h);  // head, then samplers
        const int tail = (used > 1 && NL >= 2 && (cu_per_xcd - (int)S[0].size()) / P >= 2) ? 1 : 0;  // the last layer next to the head
        const int body = NL - tail;
        int next = 0;
        for (int x = 0; x < used; ++x) {
            const int cap = (cu_per_xcd - (int)S[x].size()) / P - (x == 0 ? tail : 0);
            const int want = wn_cdiv(body - next, used - x);
            const int take = want < cap ? want : cap;
            for (int l = next; l < next + take; ++l)
                for (int c = 0; c < P; ++c) S[x].push_back(l * P + c);
            next += take;
        }
        if (next < body) continue;
        for (int l = body; l < NL; ++l)
            for (int c = 0; c < P; ++c) S[0].push_back(l * P + c);
        size_t per = 0;
        for (int x = 0; x < n_xcd; ++x) per = S[x].size() > per ? S[x].size() : per;
        *n_blocks = (int)per * n_xcd;
        map.assign(*n_blocks, -1);
        for (int b = 0; b < *n_blocks; ++b)
            if ((size_t)(b / n_xcd) < S[b % n_xcd].size()) map[b] = S[b % n_xcd][b / n_xcd];
        return true;
    }
    return false;
}

// ---- batched products (wn_forward.h): tile mapping and grids
#if defined(__HIPCC__)
#define WN_HD __host__ __device__
#else
#define WN_HD
#endif
// Workgroup -> tile, XCD-aware.  The weight-gradient products are streams over their row operands, and every tile of one row split
// re-reads the split's rows.  Workgroups are dispatched in id order, round-robin over the 8 XCDs (id % 8), each with its own L2: the
// `nshare` tiles of a sharing group are given ids 8 apart and consecutive in time -- same XCD, same moment -- so the group's rows
// come from HBM once and from that L2 afterwards.  Grids are 1-D: 8 * nshare * ceil(ngroups / 8) workgroups; returns false for the
// padding (group >= ngroups).
static inline WN_HD bool wn_tile_of(unsigned id, unsigned nshare, unsigned ngroups, unsigned& group, unsigned& member) {
    const unsigned xcd = id & 7u, slot = id >> 3;
    member = slot % nshare;
    group = (slot / nshare) * 8u + xcd;
    return group < ngroups;
}
// Grid of a weight-gradient product C[Ka][Nb] += A^T B over M rows with tiles of 128 x tile_nb: the rows are split so that about
// `want` workgroups exist (the resident ones), never below 256 rows per split (every split ends with a tile of atomics), in whole
// rounds of 8 splits where there are that many (wn_tile_of puts a split's tiles on one XCD: 25 splits would load one XCD with four
// splits and the others with three), each a multiple of 32 rows.
struct WnTnGrid { int tiles_ka, tiles_nb, splits; long long rows_per_split; unsigned blocks; };
static inline WnTnGrid wn_tn_grid(long long M, int Ka, int Nb, int tile_nb, int want) {
    WnTnGrid g;
    g.tiles_ka = (Ka + 127) / 128; g.tiles_nb = (Nb + tile_nb - 1) / tile_nb;
    const int tiles = g.tiles_ka * g.tiles_nb;
    long long splits = want / tiles > 1 ? want / tiles : 1;
    const long long most = (M + 255) / 256;
    if (splits > most) splits = most;
    if (splits >= 8) splits -= splits % 8;
    if (splits < 1) splits = 1;
    long long rps = (M + splits - 1) / splits;
    rps = (rps + 31) / 32 * 32;
    splits = (M + rps - 1) / rps;
    g.splits = (int)splits; g.rows_per_split = rps;
    g.blocks = 8u * (unsigned)tiles * (unsigned)((splits + 7) / 8);
    return g;
}

// ---- zero padding of channel shapes (wn_create): the cheapest compiled shape that HOLDS the model.  `rows`: the kernel table
// (residual channels, dilation-channel slice, skip channels, end-channel slice, slices per layer); `usable(R, D, S, E)`: the caller's
// check that the padded configuration can be planned (LDS, CU count).  Cost: workgroups on the token's path first (layers x slices +
// head slices), then the arithmetic.  Returns the row's index or -1; the padded counts in out[4] = {R, D, S, E}.
struct WnShapeRow { int R, DC, S, EC, Pm; };
template <class Usable>
static inline int wn_pad_pick(const WnShapeRow* rows, int n_rows, int R, int D, int S, int E, int n_layers, Usable usable, int out[4]) {
    long long best = -1;
    int pick = -1;
    for (int i = 0; i < n_rows; ++i) {
        const WnShapeRow& e = rows[i];
        const int D2 = e.DC * e.Pm, E2 = (E + e.EC - 1) / e.EC * e.EC;
        if (e.R < R || e.S < S || D2 < D || E2 / e.EC > 16) continue;
        if (!usable(e.R, D2, e.S, E2)) continue;
        const long long cost = ((long long)n_layers * e.Pm + E2 / e.EC) * 100000000ll + (long long)e.R * D2 + (long long)e.S * (D2 + E2);
        if (best < 0 || cost < best) { best = cost; pick = i; out[0] = e.R; out[1] = D2; out[2] = e.S; out[3] = E2; }
    }
    return pick;
}

// ---- variant 4 (wn_kernel_v4.h): streams up to which the stacked chain of n_stack workgroups beats variant 3's longer pipeline
static inline int wn_v4_stream_limit(int n_stack) { const int n = (n_stack + 2) / 2; return n < 1 ? 1 : n; }

// ---- the generation chain's planner: (wn_config, CU count, development pins, instantiated shapes) -> everything wn_create derives before its first
// allocation.  Pure host arithmetic (tests/test_chain_plan_host.py runs it without a device; tests/test_gpu_chain_plan.py against wn_get_info).
// One instantiated shape of the wave-specialised kernel (kind 3, wn_kernel_v3.h) or the stacked kernel (kind 4, wn_kernel_v4.h) as numbers: the rows are
// listed in wn_chain_shapes.h, which computes these facts from WnV2Shape / WnV3Lds / WnV4Shape / WnV4Lds.
struct WnChainShape {
    int kind, index;          // 3 / 4; row of the kind's kernel pointer table (wn_runtime.hip, wn_stacked.hip)
    int R, DC, S, EC;         // DC: dilation channels of a layer slice (kind 4: all of them, D); EC: end channels of a head slice
    int Pm;                   // kind 3: slices per layer the kernel is compiled for (its input poll is unrolled over them); kind 4: LPW, layers per workgroup
    int nwl, lanes, nwh;      // weight image of a layer (slice): nwl words for each of `lanes` lanes; of a head slice: nwh words for each of 256
    int has_g2, has_slots;    // kind 3: the two-streams-per-item form and its skip-lane slot re-use form exist
    int lds_pre[2];           // LDS floats in front of the per-stream area of a layer workgroup, by streams per item - 1 ([1]: has_g2)
    int lds_stride;           // ... and per stream there
    int lds_head, lds_smp;    // LDS floats of a head workgroup (its LDS-resident weights) and of a sampler workgroup that holds start_conv^T
};
// The development switches that steer the planner, read once per wn_create (wn_runtime.hip: wn_dev_env): WN_KERNEL, WN_SAMPLERS, WN_V3_MODE and
// WN_V3_SLOTS as given (NULL: unset), WN_CHAINS=1 and WN_NO_LOCAL_STORES=1 as flags.  no_padding has no switch: wn_create sets it (and no_rounds) to plan
// again after the device refused a padded (a rounds) handle.
struct WnPins { const char *kernel, *samplers, *v3_mode, *v3_slots; bool no_rounds, no_local_stores, no_padding; };

static inline int wn_shape_lds_floats(const WnChainShape& e, int ns, int g2) {
    int need = e.lds_pre[g2 && e.has_g2 ? 1 : 0] + ns * e.lds_stride;
    if (e.lds_head > need) need = e.lds_head;
    if (e.lds_smp * 4 <= WN_LDS_MAX_BYTES && e.lds_smp > need) need = e.lds_smp;
    return need;
}
// dedicated sampler workgroups of a multi-stream chain (each serves the streams s = j mod n): 4 by default, WN_SAMPLERS = 1..16 pins
static inline int wn_sampler_count(int n_streams, const char* pin) {
    const int n = pin && atoi(pin) >= 1 && atoi(pin) <= 16 ? atoi(pin) : 4;
    return n_streams < n ? n_streams : n;
}
static inline bool wn_pin_is(const char* pin, const char* v) { return pin && !strcmp(pin, v); }
struct WnChainPick { int row, P, PA; };
// the stacked kernel serves a configuration of an instantiated shape exactly, few streams, no pinned split.  WN_KERNEL = "v3" / "generic" pin another
// kernel, "v4" lifts the stream limit
static inline bool wn_v4_pick(const wn_config& c, int n_cu, const WnPins& pins, const WnChainShape* sh, int n_sh, WnChainPick* out) {
    if (wn_pin_is(pins.kernel, "generic") || wn_pin_is(pins.kernel, "v3")) return false;
    if (c.kernel_size != 2 || c.classes != 256 || c.layer_split > 0 || c.head_split > 0 || c.n_streams < 1 || c.n_streams > 16) return false;
    for (int i = 0; i < n_sh; ++i) {
        const WnChainShape& e = sh[i];
        if (e.kind != 4 || e.R != c.residual_channels || e.DC != c.dilation_channels || e.S != c.skip_channels || c.end_channels % e.EC) continue;
        const int PA = c.end_channels / e.EC, n_stack = wn_cdiv(c.layers * c.blocks, e.Pm);
        if (PA > 16) continue;
        // The stacked chain is a short pipeline (n_stack + 2 stages, each busy ~3 us per item): it saturates at about half a token per stage,
        // beyond that the one-layer-per-workgroup pipeline of variant 3 wins (measured, profiles/r04_v4_vs_v3_streams.txt: cfg2 -- 10 stack
        // workgroups -- up to 6 streams, cfg1 -- 2 -- up to 2, the train_script shape -- 15 -- up to 8).
        if (!wn_pin_is(pins.kernel, "v4") && c.n_streams > wn_v4_stream_limit(n_stack)) continue;
        if (n_stack + PA + wn_sampler_count(c.n_streams, pins.samplers) > n_cu) continue;
        if (wn_shape_lds_floats(e, c.n_streams, 0) * 4 > WN_LDS_MAX_BYTES) continue;
        *out = WnChainPick{i, 1, PA};
        return true;
    }
    return false;
}
// the wave-specialised kernel serves a configuration with ONE chain: an instantiated shape in the split it is compiled for, one CU per workgroup, the
// parked tap-0 sums of all streams fit the LDS next to the activations.  WN_KERNEL = "generic" pins the LDS-resident kernel
static inline bool wn_v3_pick(const wn_config& c, int n_cu, const WnPins& pins, const WnChainShape* sh, int n_sh, WnChainPick* out) {
    if (wn_pin_is(pins.kernel, "generic") || c.kernel_size != 2 || c.classes != 256) return false;
    const int NL = c.layers * c.blocks, n_smp = wn_sampler_count(c.n_streams, pins.samplers);
    for (int i = 0; i < n_sh; ++i) {
        const WnChainShape& e = sh[i];
        if (e.kind != 3 || e.R != c.residual_channels || e.S != c.skip_channels || c.dilation_channels % e.DC || c.end_channels % e.EC) continue;
        const int P = c.dilation_channels / e.DC, PA = c.end_channels / e.EC;
        if (P != e.Pm || PA > 16) continue;
        if ((c.layer_split > 0 && c.layer_split != P) || (c.head_split > 0 && c.head_split != PA)) continue;
        if (NL * P + PA + n_smp > n_cu) continue;
        if (wn_shape_lds_floats(e, c.n_streams, wn_v3_mode_for(c.n_streams, pins.v3_mode, NL) & 1) * 4 > WN_LDS_MAX_BYTES) return false;
        *out = WnChainPick{i, P, PA};
        return true;
    }
    return false;
}

// Zero padding of the channel counts.  Extra residual channels stay 0 for ever (zero rows in start_conv and the residual convs), extra
// dilation channels give tanh(0) * sigmoid(0) = 0, extra skip / end channels give relu(0) = 0 against zero weights: the padded network
// computes the same logits, and every product only gains exact zeros.  So a kernel_size-2, 256-class model whose channel shape is not
// in the table of the wave-specialised kernel (e.g. 48 / 48 / 300 / 200) runs as the cheapest instantiated shape that holds it instead
// of on the generic LDS-resident kernel (last measured 6-13x slower).  Not applied when the caller pins layer_split / head_split.
static inline bool wn_pad_config(const wn_config& c, int n_cu, const WnPins& pins, const WnChainShape* sh, int n_sh, wn_config* padded) {
    if (c.kernel_size != 2 || c.classes != 256 || c.layer_split > 0 || c.head_split > 0 || (c.reserved[0] & WN_CFG_NO_PADDING)) return false;
    wn_config probe = c;
    if (probe.n_streams > WN_V3_ROUND_STREAMS) probe.n_streams = WN_V3_ROUND_STREAMS;
    WnChainPick pk;
    if (wn_v4_pick(probe, n_cu, pins, sh, n_sh, &pk) || wn_v3_pick(probe, n_cu, pins, sh, n_sh, &pk)) return false;   // served as it is
    std::vector<WnShapeRow> rows;
    for (int i = 0; i < n_sh; ++i)
        if (sh[i].kind == 3) rows.push_back(WnShapeRow{sh[i].R, sh[i].DC, sh[i].S, sh[i].EC, sh[i].Pm});
    int dims[4];
    const int pick = wn_pad_pick(rows.data(), (int)rows.size(), c.residual_channels, c.dilation_channels, c.skip_channels, c.end_channels, c.layers * c.blocks,
                                 [&](int R2, int D2, int S2, int E2) {
                                     wn_config p2 = probe;
                                     p2.residual_channels = R2; p2.dilation_channels = D2; p2.skip_channels = S2; p2.end_channels = E2;
                                     return wn_v3_pick(p2, n_cu, pins, sh, n_sh, &pk);
                                 }, dims);
    if (pick < 0) return false;
    *padded = c;
    padded->residual_channels = dims[0]; padded->dilation_channels = dims[1]; padded->skip_channels = dims[2]; padded->end_channels = dims[3];
    return true;
}

// what wn_create refuses before it looks at the device: 0, or the error code (include/wn_abi.h) and the reason
static inline int wn_config_refusal(const wn_config& c, std::string& why) {
    if (c.layers < 1 || c.blocks < 1 || c.dilation_channels < 1 || c.residual_channels < 1 || c.skip_channels < 1 || c.end_channels < 1 || c.classes < 2 || c.n_streams < 1)
        return why = "non-positive dimension in wn_config", WN_E_BADARG;
    if (c.kernel_size < 1) return why = "kernel_size must be >= 1", WN_E_BADARG;
    if (c.layers > 24) return why = "layers > 24 (dilation 2^layers overflows the queue)", WN_E_UNSUPPORTED;
    if (c.layer_split < 0 || c.head_split < 0 || (c.reserved[0] & ~WN_CFG_NO_PADDING) || c.reserved[1] || c.reserved[2])
        return why = "negative split / non-zero reserved field", WN_E_BADARG;
    return WN_OK;
}

struct WnChainPlan {
    wn_config cfg;               // the configuration that was planned: the caller's, or (`padded`) its zero-padded form
    bool padded;
    WnPlan pl;                   // model, geometry, LDS layout, grid; the device pointers stay NULL
    int variant, row;            // 1 = generic LDS-resident kernel, 3 = wave-specialised, 4 = stacked; row of the shapes (-1: generic)
    int v3_mode, v3_slots;       // variant 3: wn_v3_mode_for after its corrections (no such form / no CUs for a second head set); wn_v3_slots_for
    int lds_bytes, gate_need;    // dynamic LDS of the launch; workgroups that stay resident on the fullest XCD
    std::vector<int32_t> dil, wg_map;
    std::vector<int64_t> ring_off, state_off;   // state_off: [NL + 1] canonical rows below layer l's block of a saved stream state (wn_state.inl)
    size_t ring_floats, gx_n, gs_n, gl_n, g0_n, gran_count, blob_floats;
    std::vector<WnChainPlan> rounds;   // a rounds front (more streams than one chain holds): its members' plans; the rest is then member 0's
};

// ONE chain for exactly this configuration.  Returns "" or the reason why no kernel serves it.
static inline std::string wn_chain_plan_one(const wn_config& c, int n_cu, const WnPins& pins, const WnChainShape* sh, int n_sh, WnChainPlan& cp) {
    cp = WnChainPlan();
    cp.cfg = c; cp.variant = 1; cp.row = -1;
    WnPlan& pl = cp.pl;
    pl.layers = c.layers; pl.blocks = c.blocks; pl.NL = c.layers * c.blocks;
    pl.R = c.residual_channels; pl.D = c.dilation_channels; pl.S = c.skip_channels; pl.E = c.end_channels;
    pl.C = c.classes; pl.k = c.kernel_size; pl.has_bias = c.bias ? 1 : 0; pl.n_streams = c.n_streams;
    WnChainPick pk;
    size_t layer_img, head_img;   // floats of one layer-role workgroup's weight image and of one head slice's
    if (wn_v4_pick(c, n_cu, pins, sh, n_sh, &pk) || wn_v3_pick(c, n_cu, pins, sh, n_sh, &pk)) {
        const WnChainShape& e = sh[pk.row];
        cp.variant = e.kind; cp.row = pk.row;
        wn_plan_geometry(pl, pk.P, pk.PA);
        pl.LPW = e.kind == 4 ? e.Pm : 1;
        pl.n_lw = e.kind == 4 ? wn_cdiv(pl.NL, pl.LPW) : pl.NL * pk.P;
        pl.n_smp = wn_sampler_count(c.n_streams, pins.samplers);   // sampling runs on dedicated workgroups (they also feed layer 0)
        pl.n_wg = pl.n_lw + pk.PA + pl.n_smp;
        pl.start_in_lds = e.lds_smp * 4 <= WN_LDS_MAX_BYTES ? 1 : 0;   // the samplers' copy of start_conv^T
        if (e.kind == 3) {
            cp.v3_mode = wn_v3_mode_for(pl.n_streams, pins.v3_mode, pl.NL);
            if (!e.has_g2) cp.v3_mode &= ~1;   // (shapes whose filter/gate slices cannot be halved: one stream per item only)
            if ((cp.v3_mode & 2) && pl.n_wg + pk.PA <= n_cu) { pl.HR = 2; pl.n_wg += pk.PA; }   // a second set of head workgroups
            else cp.v3_mode &= 1;
            cp.v3_slots = wn_v3_slots_for(pl.n_streams, cp.v3_mode, e.has_slots != 0, pins.v3_slots, pl.NL);
        }
        cp.lds_bytes = wn_shape_lds_floats(e, pl.n_streams, cp.v3_mode & 1) * 4;
        // 1-4 streams (8: measured level, profiles/archive/r03_few_stream_lds_queues.txt): the layers' dilation queues live in LDS where they fit (wn_v3_layer)
        if (e.kind == 3 && pl.n_streams <= 4 && !(cp.v3_mode & 1)) cp.lds_bytes = WN_LDS_MAX_BYTES;
        pl.lds_floats = cp.lds_bytes / 4;
        layer_img = (size_t)pl.LPW * e.nwl * e.lanes; head_img = (size_t)e.nwh * 256;
    } else {
        const std::string why = wn_plan_choose(pl, n_cu, c.layer_split, c.head_split);
        if (!why.empty()) return why;
        cp.lds_bytes = (pl.lds_floats + 8) * 4;  // + the fail-flag word (wn_any_failed)
        pl.LPW = 1; pl.n_lw = pl.NL * pl.P;
        layer_img = (size_t)pl.blob_layer_floats; head_img = (size_t)pl.blob_head_floats;
    }
    pl.head_blob_off = (int64_t)((size_t)pl.n_lw * layer_img);
    cp.blob_floats = (size_t)pl.head_blob_off + (size_t)pl.PA * head_img;
    cp.dil.resize(pl.NL); cp.ring_off.resize(pl.NL); cp.state_off.assign(pl.NL + 1, 0);
    int64_t off = 0;
    for (int l = 0; l < pl.NL; ++l) {
        const int d = 1 << (l % pl.layers);  // wavenet_model.py:72,108-110
        const int64_t ML = (int64_t)(pl.k - 1) * d + 1;  // wavenet_model.py:78
        cp.dil[l] = d;
        cp.ring_off[l] = off;
        off += (int64_t)pl.P * pl.n_streams * ML * pl.R;
        cp.state_off[l + 1] = cp.state_off[l] + ML;
    }
    cp.ring_floats = (size_t)off;
    pl.n_blocks = pl.n_wg;
    if (cp.variant >= 3 && n_cu % 8 == 0 && wn_make_wg_map_layers(cp.variant == 4 ? pl.n_lw : pl.NL, pl.P, pl.PA * pl.HR, pl.n_smp, 8, n_cu / 8, cp.wg_map, &pl.n_blocks))
        pl.allow_plain = pins.no_local_stores ? 0 : 1;
    else
        wn_make_wg_map(pl.n_wg, 8, cp.wg_map);
    // what a job keeps RESIDENT per XCD (block b lands on XCD b % 8; padding blocks exit at once and hold nothing)
    int per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int nx = n_cu % 8 == 0 ? 8 : 1;
    for (int b = 0; b < pl.n_blocks; ++b)
        if (cp.wg_map[b] >= 0 && ++per_xcd[b % nx] > cp.gate_need) cp.gate_need = per_xcd[b % nx];
    cp.gx_n = (size_t)pl.n_lw * pl.n_streams * pl.R; cp.gs_n = (size_t)pl.n_lw * pl.n_streams * pl.S; cp.gl_n = (size_t)pl.PA * pl.n_streams * pl.C;
    cp.g0_n = cp.variant >= 3 ? (size_t)pl.n_streams * pl.R : 0;
    cp.gran_count = cp.gx_n + cp.gs_n + cp.gl_n + (size_t)pl.n_streams + cp.g0_n;
    return std::string();
}

// The plan of a handle: the zero-padded form of the model where that gets it onto a register-resident kernel, rounds of up to WN_V3_ROUND_STREAMS
// streams where one chain of the wave-specialised kernel cannot hold the job (its LDS parks a tap-0 sum per stream: cfg3 ~150 streams), one chain otherwise
static inline std::string wn_chain_plan(const wn_config& c, int n_cu, const WnPins& pins, const WnChainShape* sh, int n_sh, WnChainPlan& cp) {
    wn_config eff;
    if (!pins.no_padding && wn_pad_config(c, n_cu, pins, sh, n_sh, &eff)) {
        WnPins unpadded = pins;
        unpadded.no_padding = true;
        if (wn_chain_plan(eff, n_cu, unpadded, sh, n_sh, cp).empty() && cp.variant >= 3) { cp.padded = true; return std::string(); }
    }   // (not the kernel the padding was for: plan the caller's shape instead)
    WnChainPick pk;
    wn_config probe = c;
    probe.n_streams = WN_V3_ROUND_STREAMS;
    if (!pins.no_rounds && c.n_streams > WN_V3_ROUND_STREAMS && !wn_v3_pick(c, n_cu, pins, sh, n_sh, &pk) && wn_v3_pick(probe, n_cu, pins, sh, n_sh, &pk)) {
        std::vector<WnChainPlan> members;
        for (int n : wn_v3_round_sizes(c.n_streams, WN_V3_ROUND_STREAMS)) {
            wn_config part = c;
            part.n_streams = n;
            members.emplace_back();
            if (!wn_chain_plan_one(part, n_cu, pins, sh, n_sh, members.back()).empty() || members.back().variant != 3) { members.clear(); break; }
        }
        if (!members.empty()) {
            cp = members[0];
            cp.cfg = c; cp.pl.n_streams = c.n_streams;
            cp.rounds.swap(members);
            return std::string();
        }
    }
    return wn_chain_plan_one(c, n_cu, pins, sh, n_sh, cp);
}

// ---- which kernel a job runs.  A handle resolves three slots at creation; a job takes the slot of what it needs:
//        needs                                           slot         forms 0 / 1 of variant 3, variant 4     slot re-use form          generic kernel
//        nothing                                         0 product    the product instantiation               the form's one kernel     the kernel
//        stamps (wn_profile_next) or a logits dump       1 diag       the DIAG instantiation                  the form's one kernel     the kernel
//        a sampling filter, log-probabilities, forced    2 extras     the DIAG instantiation                  the filter kernel         the kernel
// (extras outrank stamps: the DIAG instantiations and the filter kernel carry both.)
static inline int wn_kernel_slot(bool stamps_or_dump, bool extras) { return extras ? 2 : (stamps_or_dump ? 1 : 0); }
static inline int wn_job_slot(const WnRun& r) {   // (r.logp carries the log-probability mode and the forced flag)
    return wn_kernel_slot(r.prof != nullptr || r.dbg_logits != nullptr, r.top_k != 0 || r.top_p != 0.f || r.logp != 0);
}
// column of the kernel tables a slot resolves to: 0 = the product instantiation, 1 = the DIAG one, 2 = the slot form's filter kernel
static inline int wn_slot_column(int variant, bool slot_form, int slot) {
    if (variant < 3) return 0;
    if (slot_form) return slot == 2 ? 2 : 0;
    return slot ? 1 : 0;
}

// ---- time geometry of WaveNetModel.forward() (wn_forward / wn_train_*; comment: wn_runtime.hip above wn_forward_geometry)
struct WnFwdGeom { std::vector<long long> a, rows, zlo; };
// dil[l] = dilation of layer l.  Returns "" and fills g, or the reason why the reference has no defined result for clips of L samples.
// kernel_size k: a layer's conv drops its input's first (k - 1) d positions; zlo counts the output rows whose OLDEST tap is a pad zero.
// k = 3, 4 are served from L >= receptive_field + output_length - 1 only (no returned position sees a pad zero: zlo is 0 everywhere);
// shorter clips -- the reference's zero-padding regime, which the k = 2 kernels cover with row windows -- are refused for them.
static inline std::string wn_forward_geometry_host(const int32_t* dil, int NL, long long L, long long out_len, WnFwdGeom& g, int kernel_size = 2) {
    const long long k1 = kernel_size - 1;
    g.a.assign(NL + 1, 0); g.rows.assign(NL + 1, 0); g.zlo.assign(NL, 0);
    if (kernel_size != 2) {
        long long rf = 1;
        for (int l = 0; l < NL; ++l) rf += k1 * dil[l];
        if (L < rf + out_len - 1)
            return "L=" + std::to_string(L) + " is below receptive_field + output_length - 1 = " + std::to_string(rf + out_len - 1) + ": with kernel_size " +
                   std::to_string(kernel_size) + " the matrix-core forward does not serve the reference's zero-padding regime";
    }
    for (int l = 0; l < NL; ++l) {
        const long long d = dil[l], len = L - g.a[l];
        if (len < 1) return "L=" + std::to_string(L) + " leaves layer " + std::to_string(l) + " without input (the reference's conv fails there)";
        const long long pad = (d - len % d) % d, steps = (len + pad) / d;   // per-row length of the dilated layout
        if (steps < k1 + 1) return "L=" + std::to_string(L) + " leaves layer " + std::to_string(l) + " (dilation " + std::to_string(d) + ") no output position";
        if (steps == k1 + 1 && d > 1)
            return "L=" + std::to_string(L) + " gives layer " + std::to_string(l) + " (dilation " + std::to_string(d) + ") a per-row output length of 1: the reference "
                   "skips the skip path's un-dilation there (wavenet_model.py:155) and its shapes no longer match";
        g.a[l + 1] = g.a[l] - pad + k1 * d;
    }
    if (L - g.a[NL] < out_len)
        return "L=" + std::to_string(L) + " yields " + std::to_string(L - g.a[NL]) + " output positions, output_length is " + std::to_string(out_len) +
               " (the reference's view(n * l, c) fails)";
    g.rows[NL] = out_len;
    for (int l = NL - 1; l >= 0; --l) {
        const long long want = g.rows[l + 1] + k1 * dil[l], have = L - g.a[l];
        g.rows[l] = want < have ? want : have;
        const long long z = g.a[l] + k1 * dil[l] - (L - g.rows[l + 1]);
        g.zlo[l] = z > 0 ? z : 0;
    }
    return std::string();
}
// ---- batched priming (wn_forward.inl: wn_prime, wn_prime_shared, wn_prime_ragged).  need[i] = trailing positions of layer i's input that the queues above
// can still see: its own queue's (k - 1) d + 1 columns, and (k - 1) d positions behind what layer i + 1 needs.  need[0] is the receptive field, need[NL] = 0
// (the last layer's output is never consumed).  A stream of n samples computes min(need[i], n) of them.
static inline std::vector<long long> wn_prime_need(const int32_t* dil, int NL, int kernel_size) {
    const long long k1 = kernel_size - 1;
    std::vector<long long> need(NL + 1, 0);
    for (int l = NL - 1; l >= 0; --l) need[l] = need[l + 1] > 0 ? need[l + 1] + k1 * dil[l] : k1 * dil[l] + 1;
    return need;
}
// ---- row plan of the ragged form: batched priming of streams whose prompts differ in length, right-aligned at queue time n.
// Stream s holds n_prime[s] given samples at the times [n - n_prime[s], n); before its start its activations are zero at every layer (rows that are
// never computed, in a workspace that is cleared first).  Table 0 describes the start_conv gather (n_prime[s] rows per stream), table 1 + l the two
// products of layer l (l = 0 .. NL - 2): stream s computes the trailing min(need[l + 1], n_prime[s]) rows.  A table is the prefix
// sums of its streams' row counts, start[0 .. ns] (start[ns] = the product's M); a stream without rows repeats a start.  Row m of a product belongs
// to the LAST stream s with start[s] <= m and stands for the time n - rows_s + (m - start[s]) of that stream (wn_ragged_find, wn_forward.h).
// THIS is what keeps the kernels' addresses inside the workspace: every time lies in [n - n_prime[s], n), every stream in [0, ns).
struct WnRaggedPlan {
    int ns = 0, n_tables = 0;           // n_tables = NL (>= 1)
    long long n = 0;                    // the queue time behind the call
    std::vector<long long> need;        // [NL + 1]
    std::vector<int32_t> start;         // [n_tables][ns + 1]
    std::vector<long long> total;       // [n_tables] = start[t][ns]
    const int32_t* table(int t) const { return start.data() + (size_t)t * (ns + 1); }
    long long rows(int t, int s) const { return (long long)table(t)[s + 1] - table(t)[s]; }
    long long first_time(int t, int s) const { return n - rows(t, s); }
};
// Returns "" and fills p, or why not: a length outside [0, n], or ns * n at / above 2^31 rows (the bound of wn_prime: rows are 32-bit in the kernels).
static inline std::string wn_prime_ragged_plan_host(const int32_t* dil, int NL, int kernel_size, const int64_t* n_prime, int ns, long long n, WnRaggedPlan& p) {
    if (NL < 1 || ns < 1 || n < 0) return "no layers, no streams or a negative queue time";
    for (int s = 0; s < ns; ++s)
        if (n_prime[s] < 0 || n_prime[s] > n) return "stream " + std::to_string(s) + ": length " + std::to_string((long long)n_prime[s]) + " outside [0, " + std::to_string(n) + "]";
    if ((long long)ns * n >= 0x7fffffffll) return "too many rows (n_streams * n must stay below 2^31)";
    p.ns = ns; p.n_tables = NL; p.n = n;
    p.need = wn_prime_need(dil, NL, kernel_size);
    p.start.assign((size_t)NL * (ns + 1), 0);
    p.total.assign(NL, 0);
    for (int t = 0; t < NL; ++t) {
        int32_t* st = p.start.data() + (size_t)t * (ns + 1);
        long long sum = 0;
        for (int s = 0; s < ns; ++s) {
            const long long want = t == 0 ? (long long)n_prime[s] : p.need[t], rows = want < (long long)n_prime[s] ? want : (long long)n_prime[s];
            st[s] = (int32_t)sum;
            sum += rows;   // (<= ns * n < 2^31)
        }
        st[ns] = (int32_t)sum;
        p.total[t] = sum;
    }
    return std::string();
}
// ---- the pass plan: everything wn_prime_pass (wn_forward.inl) does for one handle's streams, as numbers.  Every stream owns Lt = Lp + n rows of the two
// ping-pong activation buffers: Lp = (k - 1) max_d rows of zeros (the oldest tap's reach below time 0), then the times [0, n).  Layer l's queue takes the
// newest fill_cols = min(ML, n) columns of its input; its two products (l < NL - 1) run over M = entries * rows rows:
//   the rectangle (n_prime == NULL, or every length == n):  one batch entry per stream, its trailing rows = min(need[l + 1], n) from t0 = n - rows; z is dense,
//       `rows` high per entry;
//   the ragged form:  ONE batch entry of total[1 + l] rows under the row tables of `ragged` (stream s: its trailing min(need[l + 1], n_prime[s]) rows, at the
//       times from first_time on), t0 = 0; z is addressed by (stream, time) like x, n high.
// Either way every row a product reads or writes lies in [-Lp, n) of its stream, which is what keeps the kernels inside the 2 x + z workspace
// (tests/ragged_cases.py: check_pass_plan).
//
// The APPEND form (wn_prime_append: `append`, the handle's queue time base_time >= 0) runs the same products over the same rows -- rectangle or ragged by the
// same rule -- on queues that hold a history.  The times of the pass stay [0, n): pass time t is the queue time base_time + t, stream s's samples stand at
// [n - n_prime[s], n), and where the other forms read the zero prefix this one reads what the stream's rings held:
//   the history gather of layer l (hist_rows = ML rows per stream, into the buffer that is layer l's input, ahead of layer l's fill and products) copies
//       the rows j = 1 .. ML from ring slot (base_time - j) mod ML to the pass time (n - n_prime[s]) - j; a row below -Lp is dropped (wn_prime_hist_time);
//   the fill takes fill_cols = ML columns -- every slot is rewritten at the new queue time -- into slot (base_time + t) mod ML, t in [n - ML, n) (wn_ring_slot:
//       the modulo of a negative operand done right).
// INVARIANT of the append form, on top of the bounds above: every row that a product or a fill READS was WRITTEN in this pass -- by the start gather, by a
// history gather or by a product of the layer below -- into the buffer it is read from (the buffers ping-pong: layer l + 2 re-uses layer l's, with a history
// region of another size).  The cleared workspace is not what makes an append pass right; the one row the clip at -Lp can drop (j = ML of a layer of the
// largest dilation, in a stream that appends all n rows) is the stream's dead oldest row, which no fill and no product reads (tests/append_cases.py:
// check_append_plan).
struct WnPrimeLayer {
    int ML, fill_cols;
    long long M, entries, rows, t0, z_rows;   // M == 0: no product
    int hist_rows;                            // append form: rows per stream of the history gather (ML); else 0
};
struct WnPrimePlan {
    int ns = 0, NL = 0;
    long long n = 0, Lp = 0, Lt = 0;
    size_t x_floats = 0, z_floats = 0, total_floats = 0;   // one activation buffer, z, and the workspace 2 x + z
    bool rectangle = true;
    bool append = false;                  // the append form; base_time = the queue time the pass starts at (0 in the other forms)
    long long base_time = 0;
    long long start_rows = 0;             // rows of the start_conv gather: the rectangle's ns launches of n rows, or the ragged form's one launch of total[0]
    std::vector<long long> need;          // [NL + 1]
    std::vector<WnPrimeLayer> layer;      // [NL]
    WnRaggedPlan ragged;                  // filled iff !rectangle
};
// The queue time a pass may end at: the generation kernels keep times in 64 bits and a job adds fewer than 2^32 evaluations to them, so below 2^62 nothing
// in their arithmetic (t mod ML, t - d) can overflow.
#define WN_PRIME_APPEND_TIME_MAX (1ll << 62)
// slot of time t (any sign) in a ring of ML rows: the DilatedQueue's t mod ML, mathematically (C's % rounds towards zero)
static inline WN_HD long long wn_ring_slot(long long t, long long ML) { const long long m = t % ML; return m < 0 ? m + ML : m; }
// pass time of history row j (1 = the newest) of a stream that appends n_append of the pass's n rows, or -Lp - 1 ("dropped") below the workspace
static inline WN_HD long long wn_prime_hist_time(long long n, long long n_append, long long j, long long Lp) {
    const long long t = (n - n_append) - j;
    return t < -Lp ? -Lp - 1 : t;
}
// n_prime == NULL: every stream has n samples.  Returns "" and fills p, or why not: the rectangle's "too many rows" (ns * n at / above 2^31), the ragged
// row plan's refusal, or (append) a queue time outside [0, WN_PRIME_APPEND_TIME_MAX - n).
static inline std::string wn_prime_plan_host(const int32_t* dil, int NL, int kernel_size, int R, int D, const int64_t* n_prime, int ns, long long n, WnPrimePlan& p,
                                             bool append = false, long long base_time = 0) {
    if (NL < 1 || ns < 1 || n < 0) return "no layers, no streams or a negative queue time";
    if (append && (base_time < 0 || base_time >= WN_PRIME_APPEND_TIME_MAX - n)) return "the queue time behind the call must stay below 2^62";
    p = WnPrimePlan();
    for (int s = 0; n_prime && s < ns; ++s) p.rectangle = p.rectangle && n_prime[s] == n;
    if (p.rectangle) {
        if ((long long)ns * n >= 0x7fffffffll) return "too many rows";
    } else {
        const std::string why = wn_prime_ragged_plan_host(dil, NL, kernel_size, n_prime, ns, n, p.ragged);
        if (!why.empty()) return why;
    }
    const long long k1 = kernel_size - 1;
    long long max_d = 1;
    for (int l = 0; l < NL; ++l) max_d = dil[l] > max_d ? dil[l] : max_d;
    p.ns = ns; p.NL = NL; p.n = n;
    p.append = append; p.base_time = append ? base_time : 0;
    p.Lp = k1 * max_d; p.Lt = p.Lp + n;
    p.x_floats = (size_t)ns * p.Lt * R; p.z_floats = (size_t)ns * n * D;
    p.total_floats = 2 * p.x_floats + p.z_floats;
    p.start_rows = p.rectangle ? (long long)ns * n : p.ragged.total[0];
    p.need = wn_prime_need(dil, NL, kernel_size);
    p.layer.assign(NL, WnPrimeLayer());
    for (int l = 0; l < NL; ++l) {
        WnPrimeLayer& y = p.layer[l];
        y.ML = (int)(k1 * dil[l]) + 1;
        y.fill_cols = append ? y.ML : (int)(y.ML < n ? y.ML : n);
        y.hist_rows = append ? y.ML : 0;
        if (l == NL - 1) continue;
        if (p.rectangle) {
            y.entries = ns; y.rows = p.need[l + 1] < n ? p.need[l + 1] : n;
            y.t0 = n - y.rows; y.z_rows = y.rows;
        } else {
            y.entries = 1; y.rows = p.ragged.total[1 + l];
            y.t0 = 0; y.z_rows = n;
        }
        y.M = y.entries * y.rows;
    }
    return std::string();
}
// ---- row windows of the k-tap backward's input-gradient product (wn_bwd_gemm_taps, wn_forward.h).  dx_l lives on the rows_out = g.rows[l] trailing rows of a
// clip, [dF|dG] of the layer on the rows_dfg = g.rows[l + 1] trailing ones: output row i (time L - rows_out + i) is row i - shift of dfg.
static inline long long wn_taps_bwd_shift(long long rows_out, long long rows_dfg) { return rows_out - rows_dfg; }
// The row of dfg that view j (tap j, 0 = the oldest) of output row i reads -- dfg(t + (k-1-j) d) --, or -1 where that row does not exist: the view reads as zero there.
static inline long long wn_taps_bwd_src(long long i, long long shift, long long d, int k, int j, long long rows_dfg) {
    const long long r = i - shift + (long long)(k - 1 - j) * d;
    return (r >= 0 && r < rows_dfg) ? r : -1;
}
#endif  // WN_PLAN_H
