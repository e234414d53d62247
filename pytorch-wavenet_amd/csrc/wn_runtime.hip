// wn_runtime.hip -- C ABI of libwn_mi355.so (include/wn_abi.h): handle, planner glue, HIP launch.
//
//   hipcc --offload-arch=gfx950 -shared ... wn_runtime.hip    -> libwn_mi355.so
// One backend: gfx950.  (Host logic above this ABI is tested without a GPU against tests/double, a host-memory test double
// of include/wn_abi.h built on the C oracle -- it shares no code with this file.)
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/wn_abi.h"
#include "wn_banks.h"
#include "wn_kernel.h"
#include "wn_kernel_v3.h"
#include "wn_stacked_table.h"
#include "wn_forward.h"
#include "wn_score.h"
#include "wn_gate.h"
#include "wn_optim.h"

static thread_local char g_err[512] = "";
// Development overrides (WN_KERNEL, WN_V3_MODE, WN_CHAINS, WN_SAMPLERS, WN_NO_LOCAL_STORES) pick another kernel or form than the
// planner would: they exist for A/B runs and for the tests that pin a form, and are IGNORED unless WN_TESTING=1 is set as well -- a
// stray variable in a production environment must not silently change what runs (wn_get_info reports the form that does).
static thread_local int g_dev_env_used = 0;
static thread_local int g_create_depth = 0;  // wn_create is building the member handles of a rounds front
static const char* wn_dev_env(const char* name) {
    const char* t = getenv("WN_TESTING");
    if (!t || t[0] != '1') return nullptr;
    const char* v = getenv(name);
    if (v) g_dev_env_used = 1;
    return v;
}
static bool wn_dev_flag(const char* name) { const char* v = wn_dev_env(name); return v && v[0] == '1'; }   // the on / off switches ("1" = on)

static int wn_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ------------------------------------------------------------------------------------------------ runtime shim
static const char* g_hip_what = "";
static int rt_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    g_hip_what = what;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return WN_E_HIP;
}
static void* rt_malloc(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, n ? n : 1) != hipSuccess) return nullptr;
    return p;
}
static void rt_free(void* p) { if (p) (void)hipFree(p); }
template <class T> static bool rt_grow(T*& p, size_t& have, size_t need, size_t per = 1) {   // a buffer of `need` units that only ever grows (old contents dropped)
    rt_free(p);
    p = (T*)rt_malloc(need * per * sizeof(T));
    have = p ? need : 0;
    return p != nullptr;
}
static int rt_h2d(void* d, const void* h, size_t n) { return rt_hip(hipMemcpy(d, h, n, hipMemcpyHostToDevice), "hipMemcpy H2D"); }
static int rt_d2h(void* h, const void* d, size_t n) { return rt_hip(hipMemcpy(h, d, n, hipMemcpyDeviceToHost), "hipMemcpy D2H"); }
static int rt_memset_async(void* d, int v, size_t n, void* stream) {
    return rt_hip(hipMemsetAsync(d, v, n, (hipStream_t)stream), "hipMemsetAsync");
}
static int rt_sync(void* stream) { return rt_hip(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize"); }

// The persistent kernel: one workgroup per chain position, alive for the whole generate_fast() job.
__global__ __launch_bounds__(WN_THREADS) void wn_generate_kernel(WnPlan p, WnRun r) {
    extern __shared__ __attribute__((aligned(16))) float wn_lds[];
    const int w = p.wg_map[blockIdx.x];
    if (w < 0) return;
    WnCtx cx;
    cx.p = &p; cx.r = &r; cx.lds = wn_lds; cx.w = w; cx.fail = 0;
    cx.t_start = (long long)wall_clock64();
    if (wn_not_resident(cx, wn_lds)) return;   // (every workgroup of the job is resident from here on)
    wn_load_lds(p, w, wn_lds);
    cx.t_start = (long long)wall_clock64();
    const int n_layer_wg = p.NL * p.P;
    if (w < n_layer_wg) {
        const int l = w / p.P, c = w % p.P;
        const long long n_it = r.n_eval + (l == 0 ? 1 : 0);  // L0 runs one sample-only iteration at the end
        const int ML = (p.k - 1) * p.dil[l] + 1;
        int tmod = (int)(r.t_base % ML);  // queue slot of x[t], kept incrementally (a 64-bit modulo is ~100 scalar instructions)
        for (long long e = 0; e < n_it; ++e, tmod = tmod + 1 == ML ? 0 : tmod + 1)
            for (int s = 0; s < p.n_streams; ++s) {
                cx.t_start = (long long)wall_clock64();  // the spin bound is per hand-off wait, not per job
                if (!wn_layer_item(cx, l, c, e, s, tmod)) return;
            }
    } else {
        const int h = w - n_layer_wg;
        for (long long e = 0; e < r.n_eval; ++e)
            for (int s = 0; s < p.n_streams; ++s) {
                cx.t_start = (long long)wall_clock64();
                if (!wn_head_item(cx, h, e, s)) return;
            }
    }
}


// ------------------------------------------------------------------------------------------------ register-resident shapes
// Shapes the wave-specialised kernel (variant 3, wn_kernel_v3.h) is instantiated for: (R, D/P, S, E/PA, P).  Anything else runs on the
// generic LDS-resident kernel above.  (Rounds 1-2 also had 256-thread kernels on these shapes -- "variant 2", one chain or several
// sharing the CUs two by two; round 3 moved every shape to variant 3 and removed them.)
struct WnV2Entry {
    int R, DC, S, EC, nwl, nwh;
    int Pm;  // layer split the kernel is compiled for (its input poll is unrolled over it)
    void (*pack)(const WnPlan& pl, const WnHostWeights& w, std::vector<float>& out);
    // [form]: 0 = one stream per pipeline item of a layer workgroup, 1 = two (wn_v3_mode), 2 = two + skip-lane slot re-use (wn_v3_slots_for); NULL where
    // the shape has no such form
    const void* fn_v3[3];
    const void* fn_v3_diag[3];   // the same forms with the stamps and the logits dump compiled in (DIAG: a job with wn_profile_next or dbg_logits)
    const void* fn_v3_filter;    // form 2 with the sampling filters and the log-probabilities (the forms 0 and 1 have them in fn_v3_diag); NULL where the shape has no form 2
    int (*lds_floats_v3)(int ns, int g2);
    int lds_pre_v3;  // float offset of the per-stream area = what head / sampler workgroups use in front of their own tables
    void (*launch_v3)(int form, bool diag, int grid, size_t lds, hipStream_t st, const WnPlan& p, const WnRun& r);
};

template <class SH>
static void wn_pack_v2(const WnPlan& pl, const WnHostWeights& w, std::vector<float>& out) {
    constexpr int R = SH::R, DC = SH::DC, S = SH::S, EC = SH::EC, T1 = SH::T1, K1 = SH::K1, T2 = SH::T2, K2 = SH::K2, RS = SH::RS,
                  T3 = SH::T3, K3 = SH::K3;
    const int D = pl.D, E = pl.E, P = pl.P, NL = pl.NL;
    out.assign((size_t)NL * P * SH::NWL * 256 + (size_t)pl.PA * SH::NWH * 256, 0.f);
    for (int l = 0; l < NL; ++l)
        for (int c = 0; c < P; ++c) {
            float* img = out.data() + ((size_t)l * P + c) * SH::NWL * 256;
            const float* fw = w.filter_w + (size_t)l * D * R * 2;
            const float* gw = w.gate_w + (size_t)l * D * R * 2;
            const float* rw = w.res_w + (size_t)l * R * D;
            const float* sw = w.skip_w + (size_t)l * S * D;
            for (int tid = 0; tid < 256; ++tid) {
                int j = 0;
                const int kq1 = tid % T1, grp = tid / T1, ch = c * DC + (grp >> 1), gate = grp & 1;
                const float* cw = gate ? gw : fw;
                for (int k = 0; k < K1; ++k) img[(size_t)(j++) * 256 + tid] = cw[((size_t)ch * R + kq1 * K1 + k) * 2 + 1];  // tap 1: x[t]
                for (int k = 0; k < K1; ++k) img[(size_t)(j++) * 256 + tid] = cw[((size_t)ch * R + kq1 * K1 + k) * 2 + 0];  // tap 0: x[t-d]
                const int kq2 = tid % T2, row2 = tid / T2;
                for (int k = 0; k < K2; ++k) img[(size_t)(j++) * 256 + tid] = rw[(size_t)row2 * D + c * DC + kq2 * K2 + k];
                for (int q = 0; q < RS; ++q)
                    for (int k = 0; k < DC; ++k) img[(size_t)(j++) * 256 + tid] = sw[(size_t)(tid + 256 * q) * D + c * DC + k];
                float bfg = 0.f, bres = 0.f;
                if (pl.has_bias) {
                    if (kq1 == 0) bfg = (gate ? w.gate_b : w.filter_b)[(size_t)l * D + ch];
                    if (c == 0 && kq2 == 0) bres = w.res_b[(size_t)l * R + row2];
                }
                img[(size_t)(j++) * 256 + tid] = bfg;
                img[(size_t)(j++) * 256 + tid] = bres;
                for (int q = 0; q < RS; ++q)
                    img[(size_t)(j++) * 256 + tid] = (pl.has_bias && c == 0) ? w.skip_b[(size_t)l * S + tid + 256 * q] : 0.f;
            }
        }
    for (int h = 0; h < pl.PA; ++h) {
        float* img = out.data() + (size_t)NL * P * SH::NWL * 256 + (size_t)h * SH::NWH * 256;
        for (int tid = 0; tid < 256; ++tid) {
            const int kq3 = tid % T3, row3 = tid / T3, e = h * EC + row3;
            int j = 0;
            for (int k = 0; k < K3; ++k) img[(size_t)(j++) * 256 + tid] = w.end1_w[(size_t)e * S + kq3 * K3 + k];
            for (int k = 0; k < EC; ++k) img[(size_t)(j++) * 256 + tid] = w.end2_w[(size_t)tid * E + h * EC + k];
            img[(size_t)(j++) * 256 + tid] = kq3 == 0 ? w.end1_b[e] : 0.f;
            img[(size_t)(j++) * 256 + tid] = h == 0 ? w.end2_b[tid] : 0.f;
        }
    }
}

template <int R, int DC, int S, int EC, int PM, int SK = 0>
static WnV2Entry wn_v2_entry() {
    using SH = WnV2Shape<R, DC, S, EC>;
    WnV2Entry e;
    e.R = R; e.DC = DC; e.S = S; e.EC = EC; e.nwl = SH::NWL; e.nwh = SH::NWH; e.Pm = PM;
    e.pack = wn_pack_v2<SH>;
    e.fn_v3[0] = e.fn_v3[1] = e.fn_v3[2] = nullptr; e.fn_v3_diag[0] = e.fn_v3_diag[1] = e.fn_v3_diag[2] = nullptr; e.fn_v3_filter = nullptr; e.lds_floats_v3 = nullptr; e.launch_v3 = nullptr; e.lds_pre_v3 = 0;
    static_assert(wn_v3_fits<SH, PM>(), "every table entry runs the wave-specialised kernel");
    {
        e.fn_v3[0] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 1, 0, false>;
        e.fn_v3_diag[0] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 1, 0, true>;
        if constexpr (wn_v3_g2_fits<SH>()) {
            e.fn_v3[1] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, 0, false>;
            e.fn_v3_diag[1] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, 0, true>;
        }
        // The slot re-use form exists in ONE instantiation, the one that tests r.prof at run time: its product instantiation measured 7 % SLOWER than the
        // parent's kernel on the jobs the form is for (cfg3 x 128: 1.45 M against 1.57 M; x 96: 1.37 against 1.43), this one 3 % faster (1.61 / 1.47 M) --
        // the form is throughput bound, what the stamps cost is not on its path, and the compiler's schedule of the kernel without them is the worse one
        // (profiles/r12_lean_item_loops.txt).
        // Because unfiltered product jobs run it, its sampler does NOT carry the sampling filters (wn_kernel_v3.h: the kernel is, instruction for instruction,
        // what it was before they existed): a job of this form with a filter set runs wn_generate_kernel_v3m_filter, compiled in the other unit (wn_stacked_table.h).
        if constexpr (wn_v3_g2_fits<SH>() && SK > 0) {
            e.fn_v3[2] = e.fn_v3_diag[2] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, SK, true>;
            static_assert(R == 128 && DC == 32 && S == 512 && EC == 32 && PM == 4 && SK == 4, "the slot form's filter kernel is instantiated for this shape (wn_stacked.hip)");
            e.fn_v3_filter = wn_v3_cfg3_slots_filter_fn();
        }
        e.lds_pre_v3 = WnV3Lds<SH, 1>::pre;
        e.lds_floats_v3 = [](int ns, int g2) {
            int lay = WnV3Lds<SH, 1>::floats(ns);
            if constexpr (wn_v3_g2_fits<SH>()) { if (g2) lay = WnV3Lds<SH, 2>::floats(ns); }
            const int head = WnV3Lds<SH, 1>::pre + (SH::K3 > 100 ? SH::K3 : EC) * 256;  // + the head lanes' LDS-resident weights (wn_v3_head)
            const int smp = WnV3Lds<SH, 1>::pre + 256 * R;    // + start_conv^T in the sampler workgroups (wn_v3_sampler), when it fits
            int need = lay > head ? lay : head;
            if (smp * 4 <= WN_LDS_MAX_BYTES && smp > need) need = smp;
            return need;
        };
        e.launch_v3 = [](int form, bool diag, int grid, size_t lds, hipStream_t st, const WnPlan& p, const WnRun& r) {
            auto go = [&](auto diag_c) {
                constexpr bool DG = decltype(diag_c)::value;
                if constexpr (wn_v3_g2_fits<SH>() && SK > 0) {
                    if (form == 2 && (r.top_k != 0 || r.top_p != 0.f || r.logp != 0)) { wn_v3_cfg3_slots_filter_launch(grid, lds, st, p, r); return; }
                    if (form == 2) { hipLaunchKernelGGL((wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, SK, true>), dim3(grid), dim3(WN_THREADS_V3), lds, st, p, r); return; }
                }
                if constexpr (wn_v3_g2_fits<SH>()) {
                    if (form >= 1) { hipLaunchKernelGGL((wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, 0, DG>), dim3(grid), dim3(WN_THREADS_V3), lds, st, p, r); return; }
                }
                hipLaunchKernelGGL((wn_generate_kernel_v3m<R, DC, S, EC, PM, 1, 0, DG>), dim3(grid), dim3(WN_THREADS_V3), lds, st, p, r);
            };
            if (diag) go(WnBool<true>{}); else go(WnBool<false>{});
        };
    }
    return e;
}

static const std::vector<WnV2Entry>& wn_v2_table() {
    static const std::vector<WnV2Entry> t = {
        wn_v2_entry<128, 32, 512, 32, 4, 4>(),   // cfg3: P=4, PA=8 (a 64-row head slice is the slowest pipeline stage); + the slot re-use form (96 streams and more)
        wn_v2_entry<64, 64, 256, 64, 1>(),    // cfg2: P=1, PA=4
        wn_v2_entry<32, 32, 256, 64, 1>(),    // cfg1: P=1, PA=4
        wn_v2_entry<32, 16, 1024, 32, 2>(),   // train_script.py chaconne shape, split two ways (64 skip weights per lane), PA=16 (end_conv_1 slice in LDS)
        wn_v2_entry<64, 32, 256, 64, 2>(),    // cfg2 split in two (layer_split=2)
        wn_v2_entry<16, 16, 256, 32, 1>(),    // small test shape
        wn_v2_entry<16, 16, 256, 32, 2>(),    // ... and its two-slice form
    };
    return t;
}

// picks an instantiated shape for this model; returns its index or -1
static int wn_v2_choose(const WnPlan& pl, int n_cu, int n_smp, int forced_P, int forced_PA, int* outP, int* outPA) {
    if (pl.k != 2 || pl.C != 256) return -1;
    const std::vector<WnV2Entry>& t = wn_v2_table();
    for (size_t i = 0; i < t.size(); ++i) {
        const WnV2Entry& e = t[i];
        if (e.R != pl.R || e.S != pl.S || pl.D % e.DC || pl.E % e.EC) continue;
        const int P = pl.D / e.DC, PA = pl.E / e.EC;
        if (P != e.Pm || PA > 16) continue;  // the kernel is compiled per layer split
        if ((forced_P > 0 && forced_P != P) || (forced_PA > 0 && forced_PA != PA)) continue;
        if (pl.NL * P + PA + n_smp > n_cu) continue;
        *outP = P; *outPA = PA;
        return (int)i;
    }
    return -1;
}

// dedicated sampler workgroups of a multi-stream chain (each serves the streams s = j mod n): 4 by default
static int wn_sampler_count(int n_streams) {
    int n = 4;
    const char* e = wn_dev_env("WN_SAMPLERS");
    if (e && atoi(e) >= 1 && atoi(e) <= 16) n = atoi(e);
    return n_streams < n ? n_streams : n;
}

// Throughput form of the wave-specialised kernel (bit 0: two streams per pipeline item of a layer workgroup; bit 1: two replicas
// of the head workgroups, each serving every other stream).  One stream per item is the latency-optimal form; with more streams
// than the chain can turn around in one trip the stages' fixed costs per item -- the request round trip, two workgroup barriers,
// the LDS and DPP latencies of the dot products -- bound the throughput, and two streams per item share them (every weight
// operand is used twice) at the price of a longer trip through each stage.  WN_V3_MODE = 0..3 pins a form (A/B runs, tests).
// (the rule itself is host-only arithmetic in wn_plan.h: wn_v3_mode_for, tests/test_plan_host.py)
static int wn_v3_mode(int n_streams, int n_layers) { return wn_v3_mode_for(n_streams, wn_dev_env("WN_V3_MODE"), n_layers); }

// true iff the wave-specialised kernel (variant 3) serves this configuration with ONE chain: an instantiated shape, at least
// two streams, the parked tap-0 sums of all streams fit the LDS next to the activations, one CU per workgroup
static bool wn_v3_applicable(const wn_config* cfg, int n_cu, int* out_vi, int* outP, int* outPA) {
    const char* force = wn_dev_env("WN_KERNEL");  // "generic" pins the LDS-resident kernel (A/B runs, tests)
    if (force && !strcmp(force, "generic")) return false;
    if (cfg->n_streams < WN_V3_MIN_STREAMS) return false;
    WnPlan pl = {};
    pl.layers = cfg->layers; pl.blocks = cfg->blocks; pl.NL = cfg->layers * cfg->blocks;
    pl.R = cfg->residual_channels; pl.D = cfg->dilation_channels; pl.S = cfg->skip_channels; pl.E = cfg->end_channels;
    pl.C = cfg->classes; pl.k = cfg->kernel_size; pl.n_streams = cfg->n_streams;
    const int n_smp = wn_sampler_count(cfg->n_streams);
    int P = 0, PA = 0;
    const int vi = wn_v2_choose(pl, n_cu, n_smp, cfg->layer_split, cfg->head_split, &P, &PA);
    if (vi < 0) return false;
    if (wn_v2_table()[vi].lds_floats_v3(cfg->n_streams, (wn_v3_mode(cfg->n_streams, cfg->layers * cfg->blocks) & 1) && wn_v2_table()[vi].fn_v3[1]) * 4 > WN_LDS_MAX_BYTES) return false;
    if (out_vi) *out_vi = vi;
    if (outP) *outP = P;
    if (outPA) *outPA = PA;
    return true;
}

// true iff the stacked kernel serves this configuration: an instantiated shape exactly, few streams, no pinned split
static bool wn_v4_applicable(const wn_config* cfg, int n_cu, int* out_vi, int* outPA) {
    const char* force = wn_dev_env("WN_KERNEL");  // "v3" / "generic" pin another kernel (A/B runs, tests); "v4" lifts the stream limit
    if (force && (!strcmp(force, "generic") || !strcmp(force, "v3"))) return false;
    const bool forced = force && !strcmp(force, "v4");
    if (cfg->kernel_size != 2 || cfg->classes != 256 || cfg->layer_split > 0 || cfg->head_split > 0) return false;
    if (cfg->n_streams < 1 || cfg->n_streams > 16) return false;
    const std::vector<WnV4Entry>& t = wn_v4_table();
    for (size_t i = 0; i < t.size(); ++i) {
        const WnV4Entry& e = t[i];
        if (e.R != cfg->residual_channels || e.D != cfg->dilation_channels || e.S != cfg->skip_channels || cfg->end_channels % e.EC) continue;
        const int PA = cfg->end_channels / e.EC, NL = cfg->layers * cfg->blocks, n_stack = (NL + e.LPW - 1) / e.LPW;
        if (PA > 16) continue;
        // The stacked chain is a short pipeline (n_stack + 2 stages, each busy ~3 us per item): it saturates at about half a token per stage,
        // beyond that the one-layer-per-workgroup pipeline of variant 3 wins (measured, profiles/r04_v4_vs_v3_streams.txt: cfg2 -- 10 stack
        // workgroups -- up to 6 streams, cfg1 -- 2 -- up to 2, the train_script shape -- 15 -- up to 8).
        if (!forced && cfg->n_streams > wn_v4_stream_limit(n_stack)) continue;
        const int n_smp = wn_sampler_count(cfg->n_streams);
        if (n_stack + PA + n_smp > n_cu) continue;
        if (e.lds_floats(cfg->n_streams) * 4 > WN_LDS_MAX_BYTES) continue;
        if (out_vi) *out_vi = (int)i;
        if (outPA) *outPA = PA;
        return true;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------ handle
struct WnTrainLay {
    long long N, L, out_len;
    std::vector<long long> need;          // need[l] = trailing time steps of layer l's input the loss depends on (and that exist: wn_forward_geometry)
    std::vector<long long> zlo;           // zlo[l] = leading output rows of layer l whose tap x(t - d) is one of the reference's pad zeros
    std::vector<size_t> x, th, sg;        // per layer offsets (floats) into the training workspace
    std::vector<size_t> zb;               // per skip block: Z_b, the block's z matrices side by side -- row (n, t) holds [z_first(n, t) | ... | z_{first+cnt-1}(n, t)] (see wn_train_layout_ws)
    std::vector<long long> zb_rows;       //   rows per batch entry of Z_b (the block's first layer has the most)
    std::vector<size_t> xh;               // bf16 step: the bf16 shadow of x[l] (same shape; offsets in floats, N * L * R / 2 floats each); empty otherwise
    size_t skip, ev, dzg, bskip_total, res_o, skip_o, w1_o, w2_o, fgb0, fgb1, dskip, de, dz, dfg, dfg2, dxa, dxb, colsum_tmp, idx, total;
    size_t dskip_h;                       // bf16 step: the bf16 shadow of dskip (a matrix operand twice per skip block: the dzg product and the skip weight gradient); offset in floats
    size_t bw, bt_fg, bt_res, bt_skip, bt_w1, bt_w2;  // bf16 operand banks (offsets in floats)
    int NL, G, nblk;  // layers; layers per skip block, blocks
    int cnt(int b) const { const int first = b * G; return NL - first < G ? NL - first : G; }   // layers of skip block b (its first: b * G)
    bool bf16;  // the saved forward ran with bf16 operands: so does its backward
};
struct WnDetWs { float* buf = nullptr; size_t floats = 0; };
// What the rounds of a multi-round handle share (wn_load_weights): the chain's weight images, start_conv and the GEMM-ready banks of wn_banks.h
struct WnWeights {
    float *d_blobs = nullptr, *d_start_t = nullptr, *d_start_b = nullptr;
    // batched forward (wn_forward) and training: the fp32 bank, and its bf16 copy [N][K] row-major
    float* d_fw = nullptr; size_t fw_floats = 0; bool fw_ok = false; wn_train_layout fw = {};   // fw_ok: kernel_size 2 shapes (the bf16 banks)
    bool train_ok = false;   // the training step's shapes: kernel_size 2, 3 and 4 (wn_banks.h: wn_bank_train_ok)
    bool fwd_ok = false;   // inference (wn_forward / wn_score / wn_prime): also kernel_size 3 and 4 (wn_banks.h: wn_bank_fwd_ok)
    unsigned short* d_fwb = nullptr; size_t fwb_elems = 0; bool fwb_ok = false; WnBf16Layout fwb;   // fwb_ok: the bf16 bank of a kernel_size 2 model (forward AND training forms)
    bool fwb_taps_ok = false;   // the bf16 bank of a kernel_size 3 or 4 model: wn_forward / wn_score only (WN_PRECISION_BF16_TAPS)
};
struct wn_handle {
    wn_config cfg = {};
    WnPlan plan = {};
    bool have_weights = false;
    bool pending = false;
    bool broken = false;   // rounds front: a launch failed after some rounds had started; the rounds' queue times diverged -> wn_reset
    void* last_stream = nullptr;
    long long t_base = 0;  // evaluations since the last reset
    int n_cu = 0, wall_khz = 0;
    int variant = 1;   // 1 = generic LDS-resident kernel, 3 = wave-specialised register-resident kernel (2: the 256-thread kernels of rounds 1-2, removed), 4 = stacked kernel
    int v2_index = -1; // row of wn_v2_table() / wn_v4_table()
    int lds_bytes = 0;
    int v3_mode = 0;    // variant 3: streams per pipeline item (wn_v3_mode)
    int v3_slots = 0;   // variant 3: skip-lane slots re-used per in-flight item (wn_v3_slots_for; 0 = one slot per stream)
    int dev_overrides = 0;  // a development override was in effect when this handle was planned (wn_dev_env)
    // Zero padding: a channel shape the wave-specialised kernel is not compiled for runs as the next instantiated shape that holds it,
    // its weights padded with zeros (wn_pad_config).  cfg / plan then carry the PADDED channel counts; these are the caller's.
    bool padded = false;
    int user_R = 0, user_D = 0, user_S = 0, user_E = 0;
    int export_R = 0;       // rows wn_export_queue returns (0: plan.R); set on a padded handle and on the member handles of its rounds
    // Rounds: more streams than ONE chain holds (its LDS parks a tap-0 sum per stream: cfg3 ~150 streams) are served in rounds of up to
    // WN_V3_ROUND_STREAMS streams, one round after the other on the caller's stream: this handle is then only a front that routes
    // every call to its member handles (`chains`, one complete engine per round).
    std::vector<wn_handle*> chains;
    std::vector<int> chain_first;  // first stream of round i (chain_first[n] = n_streams)
    bool rounds = false;
    bool shares_weights = false;   // member i > 0 of a rounds front: its weight images, start_conv^T and GEMM banks ARE member 0's (immutable during a
                                   // job, identical for every member -- the image layout depends on the channel shape, not on the stream count): not freed here
    // owned device allocations
    WnWeights w;   // (owned unless shares_weights)
    float* d_rings = nullptr;
    int32_t *d_dil = nullptr, *d_wg_map = nullptr;
    int64_t* d_ring_off = nullptr;
    int64_t* d_state_off = nullptr;   // [NL + 1] canonical rows below layer l's block of a saved stream state (wn_state.inl)
    wn_u64* d_gran = nullptr;
    uint32_t* d_status = nullptr;
    size_t blob_floats = 0, ring_floats = 0, gran_count = 0;
    long long* d_prof = nullptr;
    float* d_ws = nullptr; size_t ws_floats = 0;   // batched forward (wn_forward): a workspace that grows on demand
    int fw_bf16 = 0;                               //   and its operand precision (wn_set_forward_precision); kernel_size 2, shared with the training step
    int fw_bf16_taps = 0;                          //   kernel_size 3 and 4: bf16 operands for wn_forward / wn_score alone (WN_PRECISION_BF16_TAPS)
    int prof_items = 0;      // stamps requested for the next job (0 = off)
    int32_t smp_top_k = 0; float smp_top_p = 0.f;   // sampling filters of every later job (wn_set_sampling; as given: wn_generate normalises the off values)
    float* logp_out = nullptr; int64_t logp_capacity = 0; int32_t logp_mode = 0;   // log-probability output of the NEXT job alone (wn_set_logprob_output; wn_generate consumes it)
    const int32_t* forced_in = nullptr; int64_t forced_capacity = 0;               // forced samples of the NEXT job alone (wn_set_forced_samples; likewise)
    int prof_recorded = 0;   // stamps held in d_prof
    std::vector<int64_t> ring_off;
    std::vector<int32_t> dil;
    float* d_tws = nullptr; size_t tws_floats = 0;  // training workspace (saved activations + backward temporaries)
    float* d_xent = nullptr; size_t xent_rows = 0;  // wn_train_loss: per-row losses
    double* d_score_part = nullptr; size_t score_parts = 0;  // wn_score: one {sum nll, hits, rows} triple per workgroup
    WnTrainLay train = {}; bool train_valid = false;
    // wn_train_backward: the weight-gradient products run on a second stream next to the activation-gradient chain (wn_train.inl)
    hipStream_t side_stream = nullptr;
    std::vector<hipEvent_t> events;
    // deterministic weight / bias gradients (wn_train_set_deterministic; default from WN_DETERMINISTIC=1 at wn_create): partial tiles of the row splits
    // in a workspace per stream + an ordered reduction instead of fp32 atomics (wn_train.inl)
    bool deterministic = false;
    WnDetWs det_ws[2];
    char busid[32] = "";
    // admission of persistent jobs (wn_gate.h)
    std::shared_ptr<WnGateTicket> gate;   // the booking of the job in flight (released by the host function behind the kernel, or in wn_wait)
    int gate_shared = -1, gate_waited_ms = 0;
    int gate_need = 0;   // resident workgroups on the fullest XCD (wn_create)
    int resident_ms = 0; // bound of the last job's residency barrier
    int wg_per_cu = 0;   // workgroups of the job's kernel one CU holds (hipOccupancyMaxActiveBlocksPerMultiprocessor at wn_create)
    long long last_n_eval = 0;   // evaluations the job in flight advances the queues by (rolled back when it never started: WN_E_BUSY)
};
static void wn_free_weights(wn_handle* h) {   // (members i > 0 of a rounds front never free: the allocations are member 0's)
    if (!h->shares_weights) { rt_free(h->w.d_blobs); rt_free(h->w.d_start_t); rt_free(h->w.d_start_b); rt_free(h->w.d_fw); rt_free(h->w.d_fwb); }
}

// The chain kernel a handle runs: its function (for the attribute and occupancy queries of wn_create), its workgroup size, its launch
// (variants 3 and 4 exist twice: the product instantiation and the DIAG one -- wall-clock stamps, logits dump -- that a job with wn_profile_next or
//  dbg_logits or a sampling filter, a log-probability output or forced samples runs; the generic kernel tests at run time)
struct WnChainKernel { const void* fn; int threads; };
static WnChainKernel wn_chain_kernel(const wn_handle* h, bool diag) {
    if (h->variant == 4) return WnChainKernel{diag ? wn_v4_table()[h->v2_index].fn_diag : wn_v4_table()[h->v2_index].fn, WN_THREADS_V4};
    if (h->variant == 3) {
        const WnV2Entry& e = wn_v2_table()[h->v2_index];
        return WnChainKernel{(diag ? e.fn_v3_diag : e.fn_v3)[h->v3_slots ? 2 : (h->v3_mode & 1)], WN_THREADS_V3};
    }
    return WnChainKernel{(const void*)wn_generate_kernel, WN_THREADS};
}
static void wn_chain_launch(const wn_handle* h, hipStream_t st, const WnRun& r) {
    const bool diag = r.prof != nullptr || r.dbg_logits != nullptr || r.top_k != 0 || r.top_p != 0.f || r.logp != 0;   // (the sampling filters, the log-probabilities and the forced fork live in the DIAG samplers: r.logp carries both flags)
    if (h->variant == 4)
        wn_v4_table()[h->v2_index].launch(diag, h->plan.n_blocks, (size_t)h->lds_bytes, st, h->plan, r);
    else if (h->variant == 3)
        wn_v2_table()[h->v2_index].launch_v3(h->v3_slots ? 2 : (h->v3_mode & 1), diag, h->plan.n_blocks, (size_t)h->lds_bytes, st, h->plan, r);
    else
        hipLaunchKernelGGL(wn_generate_kernel, dim3(h->plan.n_blocks), dim3(WN_THREADS), (size_t)h->lds_bytes, st, h->plan, r);
}

// CUs per XCD a job of this handle needs -- the workgroups that stay resident on the fullest XCD (blocks are dispatched round-robin over
// the XCDs; the padding blocks of the layer-aligned placement exit at once and hold nothing) -- and what an XCD has
static void wn_gate_numbers(const wn_handle* h, int* need, int* cap) {
    const int n_xcd = h->n_cu % 8 == 0 ? 8 : 1;
    *cap = h->n_cu / n_xcd;
    *need = h->gate_need > 0 ? h->gate_need : (h->plan.n_blocks + n_xcd - 1) / n_xcd;
}
static void wn_gate_host_release(void* user) {   // runs on the runtime's callback thread once the job's kernel has finished
    std::shared_ptr<WnGateTicket>* t = static_cast<std::shared_ptr<WnGateTicket>*>(user);
    wn_gate_release(*t);
    delete t;
}

extern "C" int wn_abi_version(void) { return WN_ABI_VERSION; }
extern "C" const char* wn_last_error(void) { return g_err; }

extern "C" void wn_destroy(wn_handle* h) {
    if (!h) return;
    if (!h->chains.empty()) {
        for (wn_handle* c : h->chains) wn_destroy(c);
        (void)hipSetDevice(h->cfg.device_id);
        delete h;
        return;
    }
    (void)hipSetDevice(h->cfg.device_id);
    if (h->pending) (void)hipStreamSynchronize((hipStream_t)h->last_stream);
    if (h->side_stream) { (void)hipStreamSynchronize(h->side_stream); (void)hipStreamDestroy(h->side_stream); }
    for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
    wn_gate_release(h->gate);
    wn_free_weights(h);
    rt_free(h->d_rings); rt_free(h->d_dil);
    rt_free(h->d_wg_map); rt_free(h->d_ring_off); rt_free(h->d_state_off); rt_free(h->d_gran); rt_free(h->d_status); rt_free(h->d_prof); rt_free(h->d_ws);
    rt_free(h->d_tws);
    rt_free(h->d_xent);
    rt_free(h->d_score_part);
    rt_free(h->det_ws[0].buf); rt_free(h->det_ws[1].buf);
    delete h;
}

static int wn_create_impl(const wn_config* cfg, wn_handle** out);

// Zero padding of the channel counts.  Extra residual channels stay 0 for ever (zero rows in start_conv and the residual convs), extra
// dilation channels give tanh(0) * sigmoid(0) = 0, extra skip / end channels give relu(0) = 0 against zero weights: the padded network
// computes the same logits, and every product only gains exact zeros.  So a kernel_size-2, 256-class model whose channel shape is not
// in the table of the wave-specialised kernel (e.g. 48 / 48 / 300 / 200) runs as the cheapest instantiated shape that holds it instead
// of on the generic LDS-resident kernel (last measured 6-13x slower).  Not applied when the caller pins layer_split / head_split.
static bool wn_pad_config(const wn_config* cfg, int n_cu, wn_config* padded) {
    if (cfg->kernel_size != 2 || cfg->classes != 256 || cfg->layer_split > 0 || cfg->head_split > 0 || (cfg->reserved[0] & WN_CFG_NO_PADDING)) return false;
    wn_config probe = *cfg;
    if (probe.n_streams > WN_V3_ROUND_STREAMS) probe.n_streams = WN_V3_ROUND_STREAMS;
    if (wn_v4_applicable(&probe, n_cu, nullptr, nullptr) || wn_v3_applicable(&probe, n_cu, nullptr, nullptr, nullptr)) return false;   // served as it is
    std::vector<WnShapeRow> rows;
    for (const WnV2Entry& e : wn_v2_table()) rows.push_back(WnShapeRow{e.R, e.DC, e.S, e.EC, e.Pm});
    int dims[4];
    const int pick = wn_pad_pick(rows.data(), (int)rows.size(), cfg->residual_channels, cfg->dilation_channels, cfg->skip_channels, cfg->end_channels,
                                 cfg->layers * cfg->blocks, [&](int R2, int D2, int S2, int E2) {
                                     wn_config c = probe;
                                     c.residual_channels = R2; c.dilation_channels = D2; c.skip_channels = S2; c.end_channels = E2;
                                     return wn_v3_applicable(&c, n_cu, nullptr, nullptr, nullptr);
                                 }, dims);
    if (pick < 0) return false;
    *padded = *cfg;
    padded->residual_channels = dims[0]; padded->dilation_channels = dims[1]; padded->skip_channels = dims[2]; padded->end_channels = dims[3];
    return true;
}

extern "C" int wn_create(const wn_config* cfg, wn_handle** out) {
    g_err[0] = 0;
    if (!cfg || !out) return wn_fail(WN_E_BADARG, "wn_create: NULL argument");
    *out = nullptr;
    if (!g_create_depth) g_dev_env_used = 0;
    if (!g_create_depth && cfg->layers >= 1 && cfg->blocks >= 1 && cfg->dilation_channels >= 1 && cfg->residual_channels >= 1 && cfg->skip_channels >= 1 &&
        cfg->end_channels >= 1 && cfg->n_streams >= 1 && cfg->layers <= 24) {
        int ndev = 0, n_cu = 0;
        if (hipGetDeviceCount(&ndev) == hipSuccess && cfg->device_id >= 0 && cfg->device_id < ndev &&
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device_id) == hipSuccess) {
            wn_config eff;
            if (wn_pad_config(cfg, n_cu, &eff)) {
                const int rc = wn_create_impl(&eff, out);
                if (rc == WN_OK && (*out)->variant >= 3) {
                    wn_handle* h = *out;
                    h->padded = true;
                    h->user_R = cfg->residual_channels; h->user_D = cfg->dilation_channels; h->user_S = cfg->skip_channels; h->user_E = cfg->end_channels;
                    h->export_R = h->user_R;
                    for (wn_handle* c : h->chains) c->export_R = h->user_R;
                    return WN_OK;
                }
                if (rc == WN_OK) { wn_destroy(*out); *out = nullptr; }   // (not the kernel the padding was for: plan the caller's shape instead)
                g_err[0] = 0;
            }
        }
    }
    return wn_create_impl(cfg, out);
}

static int wn_create_impl(const wn_config* cfg, wn_handle** out) {
    g_err[0] = 0;
    if (!cfg || !out) return wn_fail(WN_E_BADARG, "wn_create: NULL argument");
    *out = nullptr;
    if (cfg->layers < 1 || cfg->blocks < 1 || cfg->dilation_channels < 1 || cfg->residual_channels < 1 ||
        cfg->skip_channels < 1 || cfg->end_channels < 1 || cfg->classes < 2 || cfg->n_streams < 1)
        return wn_fail(WN_E_BADARG, "wn_create: non-positive dimension in wn_config");
    if (cfg->kernel_size < 1) return wn_fail(WN_E_BADARG, "wn_create: kernel_size must be >= 1");
    if (cfg->layers > 24) return wn_fail(WN_E_UNSUPPORTED, "wn_create: layers > 24 (dilation 2^layers overflows the queue)");
    if (cfg->layer_split < 0 || cfg->head_split < 0 || (cfg->reserved[0] & ~WN_CFG_NO_PADDING) || cfg->reserved[1] || cfg->reserved[2])
        return wn_fail(WN_E_BADARG, "wn_create: negative split / non-zero reserved field");
    int n_cu = 256, wall_khz = 100000;
    {
        int ndev = 0;
        int rc = rt_hip(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
        if (rc) return rc;
        if (cfg->device_id < 0 || cfg->device_id >= ndev) return wn_fail(WN_E_BADARG, "wn_create: device_id %d of %d", cfg->device_id, ndev);
        if ((rc = rt_hip(hipSetDevice(cfg->device_id), "hipSetDevice"))) return rc;
        hipDeviceProp_t prop;
        if ((rc = rt_hip(hipGetDeviceProperties(&prop, cfg->device_id), "hipGetDeviceProperties"))) return rc;
        n_cu = prop.multiProcessorCount;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return wn_fail(WN_E_UNSUPPORTED, "wn_create: device %d is %s; this library is built for gfx950 (MI355X) only",
                           cfg->device_id, prop.gcnArchName);
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, cfg->device_id) == hipSuccess && khz > 0) wall_khz = khz;
    }
    char busid[32] = "";
    if (hipDeviceGetPCIBusId(busid, (int)sizeof(busid), cfg->device_id) != hipSuccess || !busid[0]) snprintf(busid, sizeof(busid), "dev%d", cfg->device_id);
    {   // rounds of the wave-specialised chain (see wn_handle::rounds)
        const bool off = wn_dev_flag("WN_CHAINS");
        wn_config probe = *cfg;
        probe.n_streams = WN_V3_ROUND_STREAMS;
        if (!off && cfg->n_streams > WN_V3_ROUND_STREAMS && !wn_v3_applicable(cfg, n_cu, nullptr, nullptr, nullptr) &&
            wn_v3_applicable(&probe, n_cu, nullptr, nullptr, nullptr)) {
            const std::vector<int> sizes = wn_v3_round_sizes(cfg->n_streams, WN_V3_ROUND_STREAMS);
            std::vector<wn_handle*> cs;
            std::vector<int> firsts(1, 0);
            int rc = WN_OK;
            for (size_t i = 0; i < sizes.size() && rc == WN_OK; ++i) {
                wn_config part = *cfg;
                const int n = sizes[i];
                part.n_streams = n;
                wn_handle* c = nullptr;
                ++g_create_depth;
                rc = wn_create(&part, &c);
                --g_create_depth;
                if (rc == WN_OK) {
                    cs.push_back(c);
                    firsts.push_back(firsts.back() + n);
                    if (c->variant != 3) rc = WN_E_UNSUPPORTED;
                }
            }
            if (rc == WN_OK) {
                wn_handle* c0 = cs[0];
                wn_handle* f = new wn_handle();
                f->cfg = *cfg;
                f->plan = c0->plan;
                f->plan.n_streams = cfg->n_streams;
                f->n_cu = n_cu; f->wall_khz = wall_khz; f->variant = c0->variant; f->v2_index = c0->v2_index; f->lds_bytes = c0->lds_bytes;
                f->v3_mode = c0->v3_mode; f->v3_slots = c0->v3_slots;
                f->dil = c0->dil;
                f->chains = cs;
                f->chain_first = firsts;
                f->rounds = true;
                *out = f;
                return WN_OK;
            }
            for (wn_handle* c : cs) wn_destroy(c);
            if (rc != WN_E_UNSUPPORTED) return rc;
            g_err[0] = 0;
        }
    }
    wn_handle* h = new wn_handle();
    h->cfg = *cfg;
    { const char* de = getenv("WN_DETERMINISTIC"); h->deterministic = de && de[0] == '1'; }
    h->n_cu = n_cu; h->wall_khz = wall_khz;
    memcpy(h->busid, busid, sizeof(busid));
    WnPlan& pl = h->plan;
    pl.layers = cfg->layers; pl.blocks = cfg->blocks; pl.NL = cfg->layers * cfg->blocks;
    pl.R = cfg->residual_channels; pl.D = cfg->dilation_channels; pl.S = cfg->skip_channels; pl.E = cfg->end_channels;
    pl.C = cfg->classes; pl.k = cfg->kernel_size; pl.has_bias = cfg->bias ? 1 : 0; pl.n_streams = cfg->n_streams;
    pl.HR = 1;
    {
        int P2 = 0, PA2 = 0;
        int vi3 = -1, vi4 = -1;
        if (wn_v4_applicable(cfg, n_cu, &vi4, &PA2)) {
            const WnV4Entry& ve = wn_v4_table()[vi4];
            h->variant = 4; h->v2_index = vi4;
            wn_plan_geometry(pl, 1, PA2);
            pl.LPW = ve.LPW;
            pl.n_lw = (pl.NL + ve.LPW - 1) / ve.LPW;
            pl.n_smp = wn_sampler_count(cfg->n_streams);
            pl.n_wg = pl.n_lw + PA2 + pl.n_smp;
            pl.start_in_lds = (ve.lds_pre_head + 256 * pl.R) * 4 <= WN_LDS_MAX_BYTES ? 1 : 0;
            h->lds_bytes = ve.lds_floats(pl.n_streams) * 4;
            pl.lds_floats = h->lds_bytes / 4;
        } else if (wn_v3_applicable(cfg, n_cu, &vi3, &P2, &PA2)) {
            h->variant = 3; h->v2_index = vi3;
            wn_plan_geometry(pl, P2, PA2);
            pl.n_smp = wn_sampler_count(cfg->n_streams);  // sampling runs on dedicated workgroups (they also feed layer 0)
            pl.n_wg += pl.n_smp;
            pl.start_in_lds = (wn_v2_table()[vi3].lds_pre_v3 + 256 * pl.R) * 4 <= WN_LDS_MAX_BYTES ? 1 : 0;  // the samplers' copy of start_conv^T
            h->v3_mode = wn_v3_mode(pl.n_streams, pl.NL);
            if (!wn_v2_table()[vi3].fn_v3[1]) h->v3_mode &= ~1;  // (shapes whose filter/gate slices cannot be halved: one stream per item only)
            if ((h->v3_mode & 2) && pl.NL * P2 + 2 * PA2 + pl.n_smp <= n_cu) {  // a second set of head workgroups
                pl.HR = 2;
                pl.n_wg += PA2;
            } else {
                h->v3_mode &= 1;
            }
            h->v3_slots = wn_v3_slots_for(pl.n_streams, h->v3_mode, wn_v2_table()[vi3].fn_v3[2] != nullptr, wn_dev_env("WN_V3_SLOTS"), pl.NL);
            h->lds_bytes = wn_v2_table()[vi3].lds_floats_v3(pl.n_streams, h->v3_mode & 1) * 4;
            if (pl.n_streams <= 4 && !(h->v3_mode & 1)) h->lds_bytes = WN_LDS_MAX_BYTES;  // 1-4 streams (8: measured level, profiles/archive/r03_few_stream_lds_queues.txt): the layers' dilation queues live in LDS where they fit (wn_v3_layer)
            pl.lds_floats = h->lds_bytes / 4;
        }
    }
    if (h->variant == 1) {
        const std::string why = wn_plan_choose(pl, n_cu, cfg->layer_split, cfg->head_split);
        if (!why.empty()) {
            delete h;
            return wn_fail(WN_E_UNSUPPORTED, "wn_create: %s", why.c_str());
        }
        h->lds_bytes = (pl.lds_floats + 8) * 4;  // + the fail-flag word (wn_any_failed)
    }
    // tables
    h->dil.resize(pl.NL); h->ring_off.resize(pl.NL);
    int64_t off = 0;
    for (int l = 0; l < pl.NL; ++l) {
        const int d = 1 << (l % pl.layers);  // wavenet_model.py:72,108-110
        h->dil[l] = d;
        h->ring_off[l] = off;
        const int64_t ML = (int64_t)(pl.k - 1) * d + 1;  // wavenet_model.py:78
        off += (int64_t)pl.P * pl.n_streams * ML * pl.R;
    }
    h->ring_floats = (size_t)off;
    std::vector<int64_t> state_off(pl.NL + 1, 0);
    for (int l = 0; l < pl.NL; ++l) state_off[l + 1] = state_off[l] + (int64_t)(pl.k - 1) * h->dil[l] + 1;
    std::vector<int32_t> wg_map;
    pl.n_blocks = pl.n_wg;
    pl.allow_plain = 0;
    if ((h->variant == 3 || h->variant == 4) && n_cu % 8 == 0 &&
        wn_make_wg_map_layers(h->variant == 4 ? pl.n_lw : pl.NL, pl.P, pl.PA * pl.HR, pl.n_smp, 8, n_cu / 8, wg_map, &pl.n_blocks)) {
        pl.allow_plain = wn_dev_flag("WN_NO_LOCAL_STORES") ? 0 : 1;
    } else {
        wn_make_wg_map(pl.n_wg, 8, wg_map);
    }
    {   // what a job of this handle keeps RESIDENT per XCD (block b lands on XCD b % 8; padding blocks exit at once and hold nothing)
        int per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int nx = n_cu % 8 == 0 ? 8 : 1;
        for (int b = 0; b < pl.n_blocks; ++b)
            if (wg_map[b] >= 0) per_xcd[b % nx]++;
        h->gate_need = 0;
        for (int x = 0; x < nx; ++x) h->gate_need = per_xcd[x] > h->gate_need ? per_xcd[x] : h->gate_need;
    }
    const size_t n_lw = h->variant == 4 ? (size_t)pl.n_lw : (size_t)pl.NL * pl.P;
    const size_t gx_n = n_lw * pl.n_streams * pl.R, gs_n = n_lw * pl.n_streams * pl.S, gl_n = (size_t)pl.PA * pl.n_streams * pl.C;
    const size_t g0_n = h->variant >= 3 ? (size_t)pl.n_streams * pl.R : 0;
    h->gran_count = gx_n + gs_n + gl_n + (size_t)pl.n_streams + g0_n;
    h->blob_floats = n_lw * pl.blob_layer_floats + (size_t)pl.PA * pl.blob_head_floats;
    pl.n_lw = (int32_t)n_lw; pl.head_blob_off = (int64_t)n_lw * pl.blob_layer_floats;
    if (h->variant != 4) pl.LPW = 1;
    if (h->variant == 4) {
        const WnV4Entry& ve = wn_v4_table()[h->v2_index];
        pl.head_blob_off = (int64_t)n_lw * ve.LPW * ve.nwpl * WN_THREADS_V4;
        h->blob_floats = (size_t)pl.head_blob_off + (size_t)pl.PA * ve.nwh * 256;
    }
    if (h->variant == 3) {
        const WnV2Entry& ve = wn_v2_table()[h->v2_index];
        h->blob_floats = n_lw * (size_t)ve.nwl * 256 + (size_t)pl.PA * ve.nwh * 256;
        pl.head_blob_off = (int64_t)n_lw * ve.nwl * 256;
    }
    h->w.d_blobs = (float*)rt_malloc(h->blob_floats * 4);
    h->w.d_start_t = (float*)rt_malloc((size_t)pl.C * pl.R * 4);
    h->w.d_start_b = (float*)rt_malloc((size_t)pl.R * 4);
    h->d_rings = (float*)rt_malloc(h->ring_floats * 4);
    h->d_dil = (int32_t*)rt_malloc((size_t)pl.NL * 4);
    h->d_ring_off = (int64_t*)rt_malloc((size_t)pl.NL * 8);
    h->d_state_off = (int64_t*)rt_malloc((size_t)(pl.NL + 1) * 8);
    h->d_wg_map = (int32_t*)rt_malloc((size_t)pl.n_blocks * 4);
    h->d_gran = (wn_u64*)rt_malloc(h->gran_count * 8);
    h->d_status = (uint32_t*)rt_malloc((size_t)WN_STATUS_WORDS(pl.n_wg) * 4);
    if (!h->w.d_blobs || !h->w.d_start_t || !h->w.d_start_b || !h->d_rings || !h->d_dil || !h->d_ring_off || !h->d_state_off || !h->d_wg_map ||
        !h->d_gran || !h->d_status) {
        const double q_mb = h->ring_floats * 4e-6, g_mb = h->gran_count * 8e-6, w_mb = h->blob_floats * 4e-6;
        wn_destroy(h);
        return wn_fail(WN_E_NOMEM, "wn_create: device allocation failed (queues %.1f MB, hand-off %.1f MB, weights %.1f MB)", q_mb, g_mb, w_mb);
    }
    int rc = 0;
    rc = rc ? rc : rt_h2d(h->d_dil, h->dil.data(), (size_t)pl.NL * 4);
    rc = rc ? rc : rt_h2d(h->d_ring_off, h->ring_off.data(), (size_t)pl.NL * 8);
    rc = rc ? rc : rt_h2d(h->d_state_off, state_off.data(), (size_t)(pl.NL + 1) * 8);
    rc = rc ? rc : rt_h2d(h->d_wg_map, wg_map.data(), (size_t)pl.n_blocks * 4);
    rc = rc ? rc : rt_memset_async(h->d_rings, 0, h->ring_floats * 4, nullptr);
    rc = rc ? rc : rt_memset_async(h->d_status, 0, (size_t)WN_STATUS_WORDS(pl.n_wg) * 4, nullptr);
    rc = rc ? rc : rt_sync(nullptr);
    if (rc) { wn_destroy(h); return rc; }
    pl.blobs = h->w.d_blobs; pl.start_t = h->w.d_start_t; pl.start_b = nullptr;
    pl.dil = h->d_dil; pl.ring_off = h->d_ring_off; pl.wg_map = h->d_wg_map; pl.rings = h->d_rings;
    pl.gx = h->d_gran; pl.gs = h->d_gran + gx_n; pl.gl = h->d_gran + gx_n + gs_n; pl.gi = h->d_gran + gx_n + gs_n + gl_n;
    pl.g0 = pl.gi + pl.n_streams;
    pl.status = h->d_status;
    pl.xcc_tab = h->d_status + 8;
    WnChainKernel ck = wn_chain_kernel(h, false), ck_diag = wn_chain_kernel(h, true);
    if (h->variant == 3 && h->v3_slots) {   // the slot re-use form has ONE kernel for plain and diagnostic jobs and a second one for jobs with a sampling filter
        ck_diag.fn = wn_v2_table()[h->v2_index].fn_v3_filter;
    }
    rc = rt_hip(hipFuncSetAttribute(ck.fn, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes), "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    if (!rc && ck_diag.fn != ck.fn)
        rc = rt_hip(hipFuncSetAttribute(ck_diag.fn, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes), "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    if (rc) { wn_destroy(h); return rc; }
    {   // residency is a requirement, not a hope: what the hardware can keep resident of THIS kernel with THIS much LDS, against what the plan needs per XCD
        int per_cu = 0;   // (of either instantiation: the smaller figure)
        rc = rt_hip(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ck.fn, ck.threads, (size_t)h->lds_bytes), "hipOccupancyMaxActiveBlocksPerMultiprocessor");
        if (!rc && ck_diag.fn != ck.fn) {
            int per_cu_diag = 0;
            rc = rt_hip(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_diag, ck_diag.fn, ck_diag.threads, (size_t)h->lds_bytes), "hipOccupancyMaxActiveBlocksPerMultiprocessor");
            if (per_cu_diag < per_cu) per_cu = per_cu_diag;
        }
        if (rc) { wn_destroy(h); return rc; }
        int need = 0, cap = 0;
        wn_gate_numbers(h, &need, &cap);
        h->wg_per_cu = per_cu;
        if ((long long)per_cu * cap < need) {
            const int n_wg = pl.n_wg;
            wn_destroy(h);
            return wn_fail(WN_E_UNSUPPORTED, "wn_create: the plan keeps %d workgroups resident on one XCD (%d in all), the device holds %d x %d of this kernel there",
                           need, n_wg, cap, per_cu);
        }
    }
    (void)wn_dev_env("WN_NO_FUSED_SCORE");   // (wn_score reads it per call; a handle created under it says so from the start)
    h->dev_overrides = g_dev_env_used;
    *out = h;
    return WN_OK;
}

static int wn_load_weights_impl(wn_handle* h, const wn_weight_ptrs* w);

// the caller's weights copied into zero-filled arrays of the padded shape
static int wn_load_weights_padded(wn_handle* h, const wn_weight_ptrs* w) {
    const WnPlan& pl = h->plan;
    const int R = h->user_R, D = h->user_D, S = h->user_S, E = h->user_E, R2 = pl.R, D2 = pl.D, S2 = pl.S, E2 = pl.E, C = pl.C, NL = pl.NL, k = pl.k;
    // dst[n][a][b] (extents A2, B2, inner run of `in` floats) <- src[n][a][b] (extents A, B)
    auto pad3 = [](const float* src, int n, int A, int B, int A2, int B2, int in) {
        std::vector<float> dst((size_t)n * A2 * B2 * in, 0.f);
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < A; ++a)
                memcpy(dst.data() + (((size_t)i * A2 + a) * B2) * in, src + (((size_t)i * A + a) * B) * in, (size_t)B * in * 4);
        return dst;
    };
    std::vector<float> start_w = pad3(w->start_w, 1, R, C, R2, C, 1);
    std::vector<float> filter_w = pad3(w->filter_w, NL, D, R, D2, R2, k), gate_w = pad3(w->gate_w, NL, D, R, D2, R2, k);
    std::vector<float> res_w = pad3(w->res_w, NL, R, D, R2, D2, 1), skip_w = pad3(w->skip_w, NL, S, D, S2, D2, 1);
    std::vector<float> end1_w = pad3(w->end1_w, 1, E, S, E2, S2, 1), end1_b = pad3(w->end1_b, 1, 1, E, 1, E2, 1);
    std::vector<float> end2_w = pad3(w->end2_w, 1, C, E, C, E2, 1);
    std::vector<float> start_b, filter_b, gate_b, res_b, skip_b;
    wn_weight_ptrs p = *w;
    p.start_w = start_w.data(); p.filter_w = filter_w.data(); p.gate_w = gate_w.data(); p.res_w = res_w.data(); p.skip_w = skip_w.data();
    p.end1_w = end1_w.data(); p.end1_b = end1_b.data(); p.end2_w = end2_w.data();
    if (pl.has_bias) {
        start_b = pad3(w->start_b, 1, 1, R, 1, R2, 1); filter_b = pad3(w->filter_b, NL, 1, D, 1, D2, 1); gate_b = pad3(w->gate_b, NL, 1, D, 1, D2, 1);
        res_b = pad3(w->res_b, NL, 1, R, 1, R2, 1); skip_b = pad3(w->skip_b, NL, 1, S, 1, S2, 1);
        p.start_b = start_b.data(); p.filter_b = filter_b.data(); p.gate_b = gate_b.data(); p.res_b = res_b.data(); p.skip_b = skip_b.data();
    }
    return wn_load_weights_impl(h, &p);   // (the padded arrays are this handle's shape; the handle's state is not touched on the way)
}

extern "C" int wn_load_weights(wn_handle* h, const wn_weight_ptrs* w) {
    g_err[0] = 0;
    if (!h || !w) return wn_fail(WN_E_BADARG, "wn_load_weights: NULL argument");
    if (!w->start_w || !w->filter_w || !w->gate_w || !w->res_w || !w->skip_w || !w->end1_w || !w->end1_b || !w->end2_w || !w->end2_b)
        return wn_fail(WN_E_BADARG, "wn_load_weights: a mandatory weight pointer is NULL");
    if (h->plan.has_bias && (!w->start_b || !w->filter_b || !w->gate_b || !w->res_b || !w->skip_b))
        return wn_fail(WN_E_BADARG, "wn_load_weights: cfg.bias=1 but a stack bias pointer is NULL");
    return h->padded ? wn_load_weights_padded(h, w) : wn_load_weights_impl(h, w);
}

// weights in the handle's own (possibly padded) channel shape; the pointers have been checked
static int wn_load_weights_impl(wn_handle* h, const wn_weight_ptrs* w) {
    if (!h->chains.empty()) {
        // Rounds: ONE copy of the weights.  Member 0 packs and uploads; the others point at its images and banks (round 3 uploaded the
        // weight images, start_conv^T and both GEMM banks into every member: 4 x 120 MB at cfg3 x 512 streams).
        wn_handle* c0 = h->chains[0];
        { int rc = wn_load_weights_impl(c0, w); if (rc) return rc; }
        for (size_t i = 1; i < h->chains.size(); ++i) {
            wn_handle* c = h->chains[i];
            if (c->blob_floats != c0->blob_floats || c->plan.P != c0->plan.P || c->plan.PA != c0->plan.PA || c->variant != c0->variant || c->v2_index != c0->v2_index)
                return wn_fail(WN_E_STATE, "wn_load_weights: the rounds of this handle were planned with different geometries");
            { int rc = rt_hip(hipSetDevice(c->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
            if (c->pending) { int rc = wn_wait(c); if (rc) return rc; }
            wn_free_weights(c);
            c->shares_weights = true;
            c->w = c0->w;
            c->plan.blobs = c0->plan.blobs; c->plan.start_t = c0->plan.start_t; c->plan.start_b = c0->plan.start_b;
            c->have_weights = true;
        }
        h->have_weights = true;
        return WN_OK;
    }
    const WnPlan& pl = h->plan;
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    WnHostWeights hw = {w->start_w, w->start_b, w->filter_w, w->filter_b, w->gate_w, w->gate_b, w->res_w,
                        w->res_b, w->skip_w, w->skip_b, w->end1_w, w->end1_b, w->end2_w, w->end2_b};
    std::vector<float> blobs;
    if (h->variant == 4) wn_v4_table()[h->v2_index].pack(pl, hw, blobs);
    else if (h->variant == 3) wn_v2_table()[h->v2_index].pack(pl, hw, blobs);
    else
        wn_pack_blobs(pl, hw, blobs);
    if (blobs.size() != h->blob_floats) return wn_fail(WN_E_STATE, "wn_load_weights: internal blob size mismatch");
    std::vector<float> st((size_t)pl.C * pl.R);
    wn_transpose_start(w->start_w, pl.R, pl.C, st.data());
    WnWeights& wt = h->w;
    int rc = rt_h2d(wt.d_blobs, blobs.data(), blobs.size() * 4);
    rc = rc ? rc : rt_h2d(wt.d_start_t, st.data(), st.size() * 4);
    if (pl.has_bias) {
        rc = rc ? rc : rt_h2d(wt.d_start_b, w->start_b, (size_t)pl.R * 4);
        h->plan.start_b = wt.d_start_b;
    } else {
        h->plan.start_b = nullptr;
    }
    if (rc) return rc;
    // GEMM-ready banks for wn_forward and the training step (wn_banks.h)
    wt.fw_ok = wn_bank_ok(pl);
    wt.fwd_ok = wn_bank_fwd_ok(pl);
    wt.train_ok = wn_bank_train_ok(pl);
    wt.fwb_ok = false;
    wt.fwb_taps_ok = false;
    if (wt.fwd_ok) {
        wt.fw = wn_bank_layout(pl);
        const std::vector<float> fw = wn_pack_bank(wt.fw, pl, w);
        const size_t o = fw.size();
        if (wt.fw_floats != o) { rt_free(wt.d_fw); wt.d_fw = (float*)rt_malloc(o * 4); wt.fw_floats = o; }
        if (!wt.d_fw) return wn_fail(WN_E_NOMEM, "wn_load_weights: forward weight banks (%.1f MB)", o * 4e-6);
        rc = rt_h2d(wt.d_fw, fw.data(), o * 4);
        if (rc) return rc;
        // bf16 copies for wn_set_forward_precision
        const WnBf16Layout fwb = wn_bank_layout_bf16(pl);
        const bool bank = wn_bank_fwd_bf16_ok(pl) && fwb.ok;
        wt.fwb_ok = bank && pl.k == 2;        // (the bf16 forms of the forward and the training step: kernel_size 2 only)
        wt.fwb_taps_ok = bank && pl.k != 2;   // (kernel_size 3 and 4: the forward alone)
        if (bank) {
            wt.fwb = fwb;
            const std::vector<unsigned short> wb = wn_pack_bank_bf16(fwb, wt.fw, pl, fw, w);
            const size_t ob = wb.size();
            if (wt.fwb_elems != ob) { rt_free(wt.d_fwb); wt.d_fwb = (unsigned short*)rt_malloc(ob * 2); wt.fwb_elems = ob; }
            if (!wt.d_fwb) return wn_fail(WN_E_NOMEM, "wn_load_weights: bf16 forward banks");
            rc = rt_h2d(wt.d_fwb, wb.data(), ob * 2);
            if (rc) return rc;
        }
    }
    h->have_weights = true;
    return WN_OK;
}

extern "C" int wn_reset(wn_handle* h, void* hip_stream) {
    g_err[0] = 0;
    if (!h) return wn_fail(WN_E_BADARG, "wn_reset: NULL handle");
    if (!h->chains.empty()) {
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        for (wn_handle* c : h->chains) { int rc = wn_reset(c, hip_stream); if (rc) return rc; }
        h->t_base = 0;
        h->broken = false;
        return WN_OK;
    }
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    h->t_base = 0;
    return rt_memset_async(h->d_rings, 0, h->ring_floats * 4, hip_stream);
}


extern "C" int wn_generate(wn_handle* h, const wn_generate_args* a) {
    g_err[0] = 0;
    if (!h || !a) return wn_fail(WN_E_BADARG, "wn_generate: NULL argument");
    // the log-probability output (wn_set_logprob_output) and the forced samples (wn_set_forced_samples) armed for THIS call: BOTH are consumed here, ahead
    // of either capacity test, whatever becomes of the call -- a job refused for one of them must not leave the other behind for the next job
    float* const logp_out = h->logp_out;
    const int64_t logp_capacity = h->logp_capacity;
    const int32_t logp_mode = h->logp_mode;
    h->logp_out = nullptr; h->logp_capacity = 0; h->logp_mode = 0;
    const int32_t* const forced_in = h->forced_in;
    const int64_t forced_capacity = h->forced_capacity;
    h->forced_in = nullptr; h->forced_capacity = 0;
    if (logp_out && a->num_samples > 0 && (long long)h->plan.n_streams * (long long)a->num_samples > (long long)logp_capacity)
        return wn_fail(WN_E_BADARG, "wn_generate: the log-probability output holds %lld floats, the job writes %d x %lld; nothing was launched",
                       (long long)logp_capacity, h->plan.n_streams, (long long)a->num_samples);
    if (forced_in && a->num_samples > 0 && (long long)h->plan.n_streams * (long long)a->num_samples > (long long)forced_capacity)
        return wn_fail(WN_E_BADARG, "wn_generate: the forced samples hold %lld values, the job reads %d x %lld; nothing was launched",
                       (long long)forced_capacity, h->plan.n_streams, (long long)a->num_samples);
    if (!h->have_weights) return wn_fail(WN_E_STATE, "wn_generate: wn_load_weights has not been called");
    if (!h->chains.empty()) {   // rounds: member i owns streams [chain_first[i], chain_first[i + 1]); one after the other on the caller's stream
        if (a->n_given < 1 || a->num_samples < 0) return wn_fail(WN_E_BADARG, "wn_generate: n_given must be >= 1 and num_samples >= 0");
        if (!a->first_samples) return wn_fail(WN_E_BADARG, "wn_generate: first_samples is NULL");
        { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        if (h->broken) return wn_fail(WN_E_STATE, "wn_generate: an earlier job failed half way through its rounds; call wn_reset");
        int rc = WN_OK;
        for (size_t i = 0; i < h->chains.size(); ++i) {
            wn_generate_args b = *a;
            const size_t s0 = (size_t)h->chain_first[i];
            b.first_samples = a->first_samples + s0 * (size_t)a->n_given;
            if (a->uniforms) b.uniforms = a->uniforms + s0 * (size_t)a->num_samples;
            if (a->out_idx) b.out_idx = a->out_idx + s0 * (size_t)a->num_samples;
            if (a->dbg_logits) b.dbg_logits = a->dbg_logits + s0 * (size_t)a->num_samples * h->plan.C;
            if (a->stream_temperatures) b.stream_temperatures = a->stream_temperatures + s0;
            if (logp_out) {   // (the member's slice; the whole array's capacity was checked above)
                wn_handle* m = h->chains[i];
                m->logp_out = logp_out + s0 * (size_t)a->num_samples;
                m->logp_capacity = (int64_t)(h->chain_first[i + 1] - h->chain_first[i]) * a->num_samples;
                m->logp_mode = logp_mode;
            }
            if (forced_in) {
                wn_handle* m = h->chains[i];
                m->forced_in = forced_in + s0 * (size_t)a->num_samples;
                m->forced_capacity = (int64_t)(h->chain_first[i + 1] - h->chain_first[i]) * a->num_samples;
            }
            if (i == 0 && h->prof_items > 0) { h->chains[0]->prof_items = h->prof_items; h->prof_items = 0; }
            rc = wn_generate(h->chains[i], &b);
            if (rc) {
                if (i > 0) {  // rounds 0..i-1 are enqueued: drain them, then refuse further jobs until the queues are reset
                    char msg[sizeof(g_err)];
                    memcpy(msg, g_err, sizeof(msg));
                    h->pending = true; h->last_stream = a->hip_stream;
                    (void)wn_wait(h);
                    h->broken = true;
                    memcpy(g_err, msg, sizeof(msg));
                }
                return rc;
            }
        }
        h->pending = true;
        h->last_stream = a->hip_stream;
        h->t_base = h->chains[0]->t_base;
        return WN_OK;
    }
    if (a->n_given < 1 || a->num_samples < 0) return wn_fail(WN_E_BADARG, "wn_generate: n_given must be >= 1 and num_samples >= 0");
    if (!a->first_samples) return wn_fail(WN_E_BADARG, "wn_generate: first_samples is NULL");
    if (a->num_samples > 0 && !a->out_idx) return wn_fail(WN_E_BADARG, "wn_generate: out_idx is NULL");
    if (a->flags != 0 || a->reserved != 0) return wn_fail(WN_E_BADARG, "wn_generate: flags/reserved must be 0");
    const bool greedy = (!(a->temperature > 0.f) && !a->stream_temperatures) || a->uniforms == nullptr;
    const long long n_eval = a->n_given - 1 + a->num_samples;
    if (n_eval + 1 >= 0xFFFFFFFFll || (n_eval + 1) * (long long)h->plan.n_streams >= 0xFFFFFFFFll)   // (re-used slots count pipeline items, not evaluations)
        return wn_fail(WN_E_BADARG, "wn_generate: job too long for 32-bit hand-off tags");
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    if (n_eval == 0) return WN_OK;
    WnRun r;
    memset(&r, 0, sizeof(r));
    r.first = a->first_samples; r.n_given = a->n_given; r.num_samples = a->num_samples; r.n_eval = n_eval;
    r.t_base = h->t_base; r.temperature = a->temperature; r.greedy = greedy ? 1 : 0; r.reg = a->regularizer;
    r.uniforms = a->uniforms; r.out_idx = a->out_idx; r.dbg_logits = a->dbg_logits; r.stream_temps = a->stream_temperatures;
    if (forced_in && a->num_samples > 0) r.logp |= WN_RUN_FORCED;   // (its pointer travels behind xcc_tab; the forced fork lives where the log-probabilities live)
    r.logp |= logp_out ? 1 + logp_mode : 0;   // (the pointer travels in status[6..7], below; an armed job, a greedy one too, runs the instantiation that carries the log-probabilities: wn_chain_launch)
    if (!greedy) {   // (nothing is drawn in a greedy job: no filter applies to it, and unarmed it runs the kernel it always ran)
        r.top_k = h->smp_top_k < h->plan.C ? h->smp_top_k : 0;
        r.top_p = h->smp_top_p < 1.f ? h->smp_top_p : 0.f;
    }
    const long long ms = a->timeout_ms > 0 ? a->timeout_ms : 10000;
    r.timeout_ticks = ms * (long long)h->wall_khz;
    {   // the start-up residency barrier has a bound of its own: a job that finds CUs taken by another kernel starts when they free up
        const char* re = getenv("WN_RESIDENT_TIMEOUT_MS");
        const long long rms = re && atoll(re) > 0 ? atoll(re) : 60000;
        r.resident_ticks = rms * (long long)h->wall_khz;
        h->resident_ms = (int)(rms > 0x7fffffff ? 0x7fffffff : rms);
    }
    {   // CUs this stream may use right now (a CU mask on the stream, or the process-wide one): fewer than the job keeps resident = it could never start
        uint32_t mask[32];
        memset(mask, 0, sizeof(mask));
        if (hipExtStreamGetCUMask((hipStream_t)a->hip_stream, 32, mask) == hipSuccess) {
            int cus = 0;
            for (int i = 0; i < 32; ++i) cus += __builtin_popcount(mask[i]);
            const int per_cu = h->wg_per_cu > 0 ? h->wg_per_cu : 1;
            if (cus > 0 && (long long)cus * per_cu < h->plan.n_wg)
                return wn_fail(WN_E_UNSUPPORTED, "wn_generate: the stream's CU mask leaves %d compute units (%d workgroup%s of this kernel each), the job keeps %d "
                               "workgroups resident; nothing was launched", cus, per_cu, per_cu == 1 ? "" : "s", h->plan.n_wg);
        } else {
            (void)hipGetLastError();
        }
    }
    if (h->prof_items > 0) {
        rt_free(h->d_prof);
        const size_t nb = (size_t)h->plan.n_wg * h->prof_items * 8 * sizeof(long long);
        h->d_prof = (long long*)rt_malloc(nb);
        if (!h->d_prof) return wn_fail(WN_E_NOMEM, "wn_generate: profile buffer");
        int prc = rt_memset_async(h->d_prof, 0, nb, a->hip_stream);
        if (prc) return prc;
        r.prof = h->d_prof; r.prof_items = h->prof_items;
        h->prof_recorded = h->prof_items;
        h->prof_items = 0;
    }
    {   // admission: a persistent job only runs once ALL its workgroups are resident (wn_gate.h)
        wn_gate_release(h->gate);
        h->gate.reset();
        if (!wn_dev_flag("WN_NO_DEVICE_GATE")) {
            int need = 0, cap = 0;
            wn_gate_numbers(h, &need, &cap);
            const char* te = getenv("WN_GATE_TIMEOUT_MS");
            const long long gate_ms = te && atoll(te) > 0 ? atoll(te) : 600000;
            long long waited = 0;
            int shared = 0;
            if (wn_gate_acquire(h->busid, cap, need, a->hip_stream, gate_ms, &h->gate, &waited, &shared))
                return wn_fail(WN_E_TIMEOUT, "wn_generate: device %s stayed booked by other persistent jobs for %lld ms (this job needs %d of %d CUs per XCD); "
                               "nothing was launched", h->busid, waited, need, cap);
            h->gate_shared = shared; h->gate_waited_ms = (int)(waited > 0x7fffffff ? 0x7fffffff : waited);
        }
    }
    // hand-off words restart at tag 1 every call: zero them (and the status word) ahead of the launch
    int rc = rt_memset_async(h->d_gran, 0, h->gran_count * 8, a->hip_stream);
    rc = rc ? rc : rt_memset_async(h->d_status, 0, (size_t)WN_STATUS_WORDS(h->plan.n_wg) * 4, a->hip_stream);   // (the whole block: no pointer of an earlier armed job stays in its tail)
    if (!rc && logp_out) {   // the log-probability output pointer, behind the memset: two 32-bit fills, no host buffer to keep alive (wn_logp_out, wn_kernel.h)
        const unsigned long long bits = (unsigned long long)(uintptr_t)logp_out;
        rc = rt_hip(hipMemsetD32Async((hipDeviceptr_t)(h->d_status + 6), (int)(uint32_t)bits, 1, (hipStream_t)a->hip_stream), "hipMemsetD32Async");
        rc = rc ? rc : rt_hip(hipMemsetD32Async((hipDeviceptr_t)(h->d_status + 7), (int)(uint32_t)(bits >> 32), 1, (hipStream_t)a->hip_stream), "hipMemsetD32Async");
    }
    if (!rc && (r.logp & WN_RUN_FORCED)) {   // the forced samples' pointer, likewise (wn_forced_in, wn_kernel.h)
        const unsigned long long bits = (unsigned long long)(uintptr_t)forced_in;
        uint32_t* at = h->d_status + WN_STATUS_FORCED(h->plan.n_wg);
        rc = rt_hip(hipMemsetD32Async((hipDeviceptr_t)at, (int)(uint32_t)bits, 1, (hipStream_t)a->hip_stream), "hipMemsetD32Async");
        rc = rc ? rc : rt_hip(hipMemsetD32Async((hipDeviceptr_t)(at + 1), (int)(uint32_t)(bits >> 32), 1, (hipStream_t)a->hip_stream), "hipMemsetD32Async");
    }
    if (rc) { wn_gate_release(h->gate); h->gate.reset(); return rc; }
    wn_chain_launch(h, (hipStream_t)a->hip_stream, r);
    rc = rt_hip(hipGetLastError(), "launch wn_generate_kernel");
    if (rc) { wn_gate_release(h->gate); h->gate.reset(); return rc; }
    if (h->gate) {   // the booking goes back the moment the kernel is done (a caller that never waits must not keep the device closed)
        std::shared_ptr<WnGateTicket>* t = new std::shared_ptr<WnGateTicket>(h->gate);
        if (hipLaunchHostFunc((hipStream_t)a->hip_stream, wn_gate_host_release, t) != hipSuccess) { (void)hipGetLastError(); delete t; }  // (wn_wait returns it then)
    }
    h->pending = true;
    h->last_stream = a->hip_stream;
    h->t_base += n_eval;
    h->last_n_eval = n_eval;
    return WN_OK;
}

extern "C" int wn_wait(wn_handle* h) {
    if (!h) return wn_fail(WN_E_BADARG, "wn_wait: NULL handle");
    if (!h->pending) return WN_OK;
    h->pending = false;
    if (!h->chains.empty()) {
        // Every round is a kernel of its own with its own residency barrier: "nothing ran, repeat the call" (WN_E_BUSY) is only true of the JOB when
        // it is true of EVERY round.  A round that gave up while another ran to completion leaves the rounds' queue times apart -- a repeated call
        // would advance the completed rounds twice -- so a mixed outcome closes the handle until wn_reset, like a launch that failed half way.
        int first_rc = WN_OK, n_busy = 0, n_ok = 0;
        char msg[sizeof(g_err)] = "";
        for (wn_handle* c : h->chains) {
            const int rc = wn_wait(c);
            if (rc == WN_E_BUSY) ++n_busy;
            else if (rc == WN_OK) ++n_ok;
            if (rc && (!first_rc || (first_rc == WN_E_BUSY && rc != WN_E_BUSY))) { first_rc = rc; memcpy(msg, g_err, sizeof(msg)); }   // (a hard error outranks BUSY)
        }
        if (!first_rc) return WN_OK;
        if (n_busy == (int)h->chains.size()) {   // no round started: every member rolled its own queue time back, the parent follows
            h->t_base = h->chains[0]->t_base;
            memcpy(g_err, msg, sizeof(msg));
            return WN_E_BUSY;
        }
        h->broken = true;
        if (first_rc == WN_E_BUSY)
            return wn_fail(WN_E_STATE, "wn_generate: %d of the job's %d rounds never became resident (WN_RESIDENT_TIMEOUT_MS) while %d ran: the rounds' queues are "
                           "out of step -- call wn_reset", n_busy, (int)h->chains.size(), n_ok);
        memcpy(g_err, msg, sizeof(msg));
        return first_rc;
    }
    int rc = rt_sync(h->last_stream);
    wn_gate_release(h->gate);
    h->gate.reset();
    if (rc) return rc;
    uint32_t st[8];
    rc = rt_d2h(st, h->d_status, 32);
    if (rc) return rc;
    if (st[0] != 0 && st[4] == 5) {   // WN_W_RESIDENT: the job never started -- no workgroup entered the chain, queues and rings are as they were
        h->t_base -= h->last_n_eval;
        h->last_n_eval = 0;
        return wn_fail(WN_E_BUSY,
                       "wn_generate: only %u of the job's %d workgroups had become resident after %d ms (WN_RESIDENT_TIMEOUT_MS): the device's compute units "
                       "are held by other kernels (or masked); nothing was generated and the queues are unchanged -- the call can be repeated",
                       st[2], h->plan.n_wg, h->resident_ms);
    }
    if (st[0] != 0) {
        static const char* where[] = {"?", "partial logits (head -> L0)", "x partials (layer -> layer)", "skip lane (layer -> layer)",
                                      "skip lanes (last layer -> head)"};
        return wn_fail(WN_E_TIMEOUT,
                       "wn_generate: hand-off wait gave up at chain position %u (eval %u, stream %u) waiting for %s; "
                       "queues are in an undefined state -- call wn_reset",
                       st[1], st[2], st[3], where[st[4] < 5 ? st[4] : 0]);
    }
    return WN_OK;
}

extern "C" int wn_get_info(wn_handle* h, wn_info* out) {
    if (!h || !out) return wn_fail(WN_E_BADARG, "wn_get_info: NULL argument");
    if (!h->chains.empty()) {  // both chains have the same geometry; sizes and workgroups add up
        int rc = wn_get_info(h->chains[0], out);
        if (rc) return rc;
        for (size_t i = 1; i < h->chains.size(); ++i) {
            wn_info ci;
            if ((rc = wn_get_info(h->chains[i], &ci))) return rc;
            out->n_workgroups += ci.n_workgroups; out->queue_bytes += ci.queue_bytes;
            if (!h->chains[i]->shares_weights) out->weight_bytes += ci.weight_bytes;   // (after wn_load_weights the rounds share member 0's)
            out->handoff_bytes += ci.handoff_bytes;
        }
        out->n_chains = (int)h->chains.size();
        for (wn_handle* c : h->chains) if (c->gate_waited_ms > out->gate_waited_ms) out->gate_waited_ms = c->gate_waited_ms;
        return WN_OK;
    }
    const WnPlan& pl = h->plan;
    memset(out, 0, sizeof(*out));
    out->abi_version = WN_ABI_VERSION;
    out->n_layers = pl.NL; out->layer_split = pl.P; out->head_split = pl.PA; out->n_workgroups = pl.n_wg;
    out->lds_bytes = h->lds_bytes; out->n_compute_units = h->n_cu; out->kernel_variant = h->variant;
    out->receptive_field = 1 + pl.blocks * (pl.k - 1) * ((1 << pl.layers) - 1);
    out->weight_bytes = (int64_t)h->blob_floats * 4 + (int64_t)pl.C * pl.R * 4;
    out->queue_bytes = (int64_t)h->ring_floats * 4;
    out->handoff_bytes = (int64_t)h->gran_count * 8;
    out->evals_done = h->t_base;
    out->n_chains = 1;
    out->streams_per_item = (h->variant == 3 && (h->v3_mode & 1)) ? 2 : 1;
    out->head_replicas = pl.HR;
    out->n_samplers = pl.n_smp;
    out->dev_overrides = h->dev_overrides;
    out->layers_per_workgroup = h->variant == 4 ? pl.LPW : 1;
    out->gate_shared = h->gate_shared; out->gate_waited_ms = h->gate_waited_ms;
    { int need = 0, cap = 0; wn_gate_numbers(h, &need, &cap); out->gate_need_per_xcd = need; }
    out->forward_native = (h->have_weights && h->w.fwd_ok) ? 1 : 0;
    out->workgroups_per_cu = h->wg_per_cu; out->resident_timeout_ms = h->resident_ms; out->skip_lane_slots = h->variant == 3 ? h->v3_slots : 0;
    return WN_OK;
}

extern "C" int wn_export_queue(wn_handle* h, int32_t layer, int32_t stream, float* host_data, int32_t* in_pos, int32_t* out_pos) {
    g_err[0] = 0;
    if (!h || !host_data) return wn_fail(WN_E_BADARG, "wn_export_queue: NULL argument");
    if (!h->chains.empty()) {
        if (stream < 0 || stream >= h->plan.n_streams) return wn_fail(WN_E_BADARG, "wn_export_queue: index out of range");
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        size_t i = 0;
        while (stream >= h->chain_first[i + 1]) ++i;
        return wn_export_queue(h->chains[i], layer, stream - h->chain_first[i], host_data, in_pos, out_pos);
    }
    const WnPlan& pl = h->plan;
    if (layer < 0 || layer >= pl.NL || stream < 0 || stream >= pl.n_streams) return wn_fail(WN_E_BADARG, "wn_export_queue: index out of range");
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    const int d = h->dil[layer];
    const int ML = (pl.k - 1) * d + 1;
    std::vector<float> tmp((size_t)ML * pl.R);
    // slice c = 0 holds the layer's queue (all P slices keep identical copies)
    int rc = rt_d2h(tmp.data(), h->d_rings + h->ring_off[layer] + (size_t)stream * ML * pl.R, tmp.size() * 4);
    if (rc) return rc;
    const int R_out = h->export_R ? h->export_R : pl.R;   // (zero padding: the caller's channels are the first ones)
    for (int r = 0; r < R_out; ++r)
        for (int m = 0; m < ML; ++m) host_data[(size_t)r * ML + m] = tmp[(size_t)m * pl.R + r];  // (slot, R) -> (R, max_length)
    if (in_pos) *in_pos = (int32_t)(h->t_base % ML);  // one enqueue + one dequeue per evaluation
    if (out_pos) *out_pos = (int32_t)(h->t_base % ML);
    return WN_OK;
}

// Sampling filters of every later job on the handle (include/wn_abi.h has the contract; the kernels read them from WnRun)
extern "C" int wn_set_sampling(wn_handle* h, int32_t top_k, float top_p) {
    g_err[0] = 0;
    if (!h) return wn_fail(WN_E_BADARG, "wn_set_sampling: NULL handle");
    if (top_k < 0) return wn_fail(WN_E_BADARG, "wn_set_sampling: top_k must be >= 0 (0 and >= classes: off), got %d", (int)top_k);
    if (!(top_p >= 0.f && top_p <= 1.f)) return wn_fail(WN_E_BADARG, "wn_set_sampling: top_p must lie in [0, 1] (0 and 1: off), got %g", (double)top_p);
    for (wn_handle* c : h->chains) { int rc = wn_set_sampling(c, top_k, top_p); if (rc) return rc; }   // (rounds: every member draws with the same filter)
    h->smp_top_k = top_k; h->smp_top_p = top_p;
    return WN_OK;
}

// Per-sample log-probabilities of the NEXT job on the handle (include/wn_abi.h has the contract; wn_generate consumes the arming, the kernels read WnRun)
extern "C" int wn_set_logprob_output(wn_handle* h, float* logp, int64_t capacity, int32_t mode) {
    g_err[0] = 0;
    if (capacity < 0) return wn_fail(WN_E_BADARG, "wn_set_logprob_output: capacity must be >= 0, got %lld", (long long)capacity);
    if (mode != WN_LOGP_SAMPLING && mode != WN_LOGP_MODEL)
        return wn_fail(WN_E_BADARG, "wn_set_logprob_output: mode must be WN_LOGP_SAMPLING (0) or WN_LOGP_MODEL (1), got %d", (int)mode);
    if (!h) return wn_fail(WN_E_BADARG, "wn_set_logprob_output: NULL handle");   // (behind the value checks: those are testable without a device)
    h->logp_out = logp; h->logp_capacity = logp ? capacity : 0; h->logp_mode = logp ? mode : 0;
    return WN_OK;
}

// Forced samples of the NEXT job on the handle (include/wn_abi.h has the contract; wn_generate consumes the arming, the kernels read the status block)
extern "C" int wn_set_forced_samples(wn_handle* h, const int32_t* forced, int64_t capacity) {
    g_err[0] = 0;
    if (capacity < 0) return wn_fail(WN_E_BADARG, "wn_set_forced_samples: capacity must be >= 0, got %lld", (long long)capacity);
    if (!h) return wn_fail(WN_E_BADARG, "wn_set_forced_samples: NULL handle");   // (behind the value check: that one is testable without a device)
    h->forced_in = forced; h->forced_capacity = forced ? capacity : 0;
    return WN_OK;
}

// Diagnostics (not part of the reference surface): wall-clock stamps of the first n_items (eval, stream) steps of
// every workgroup of the NEXT wn_generate, 4 stamps each (start, input staged, x' published, done), 100 MHz ticks.
extern "C" int wn_profile_next(wn_handle* h, int32_t n_items) {
    if (!h || n_items < 0) return wn_fail(WN_E_BADARG, "wn_profile_next: bad argument");
    if (!h->chains.empty()) return wn_profile_next(h->chains[0], n_items);  // stamps of the first chain
    h->prof_items = n_items;
    return WN_OK;
}

extern "C" int wn_profile_read(wn_handle* h, int64_t* host_out, int64_t capacity) {
    if (!h || !host_out) return wn_fail(WN_E_BADARG, "wn_profile_read: NULL argument");
    if (!h->chains.empty()) {
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        return wn_profile_read(h->chains[0], host_out, capacity);
    }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    const int64_t n = (int64_t)h->plan.n_wg * h->prof_recorded * 8;
    if (!h->d_prof || n == 0 || capacity < n) return wn_fail(WN_E_STATE, "wn_profile_read: nothing recorded / buffer too small (%lld)", (long long)n);
    return rt_d2h(host_out, h->d_prof, (size_t)n * 8);
}

#include "wn_forward.inl"
#include "wn_state.inl"
#include "wn_train.inl"
#include "wn_optim.inl"
