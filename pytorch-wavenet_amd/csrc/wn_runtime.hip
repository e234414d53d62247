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
// Kernel pointers of the shapes the wave-specialised kernel (variant 3, wn_kernel_v3.h) is instantiated for: one row per shape of WN_V3_SHAPES
// (wn_chain_shapes.h, where the planner's facts of the same rows are computed).  Anything else runs on the generic LDS-resident kernel above.
// (Rounds 1-2 also had 256-thread kernels on these shapes -- "variant 2", one chain or several sharing the CUs two by two; round 3 moved every
// shape to variant 3 and removed them.)
struct WnV3Kernels {
    void (*pack)(const WnPlan& pl, const WnHostWeights& w, std::vector<float>& out);
    // [form]: 0 = one stream per pipeline item of a layer workgroup, 1 = two (wn_v3_mode_for), 2 = two + skip-lane slot re-use (wn_v3_slots_for); NULL where
    // the shape has no such form
    const void* fn[3];
    const void* fn_diag[3];   // the same forms with the stamps and the logits dump compiled in (DIAG)
    const void* fn_filter;    // form 2 with the sampling filters and the log-probabilities (the forms 0 and 1 have them in fn_diag); NULL where the shape has no form 2
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

template <int R, int DC, int S, int EC, int PM, int SK>
static WnV3Kernels wn_v3_kernels_of() {
    using SH = WnV2Shape<R, DC, S, EC>;
    WnV3Kernels e = {};
    e.pack = wn_pack_v2<SH>;
    e.fn[0] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 1, 0, false>;
    e.fn_diag[0] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 1, 0, true>;
    if constexpr (wn_v3_g2_fits<SH>()) {
        e.fn[1] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, 0, false>;
        e.fn_diag[1] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, 0, true>;
    }
    // The slot re-use form exists in ONE instantiation, the one that tests r.prof at run time: its product instantiation measured 7 % SLOWER than the
    // parent's kernel on the jobs the form is for (cfg3 x 128: 1.45 M against 1.57 M; x 96: 1.37 against 1.43), this one 3 % faster (1.61 / 1.47 M) --
    // the form is throughput bound, what the stamps cost is not on its path, and the compiler's schedule of the kernel without them is the worse one
    // (profiles/r12_lean_item_loops.txt).
    // Because unfiltered product jobs run it, its sampler does NOT carry the sampling filters (wn_kernel_v3.h: the kernel is, instruction for instruction,
    // what it was before they existed): a job of this form with a filter set runs wn_generate_kernel_v3m_filter, compiled in the other unit (wn_stacked_table.h).
    if constexpr (SK > 0) {
        e.fn[2] = e.fn_diag[2] = (const void*)wn_generate_kernel_v3m<R, DC, S, EC, PM, 2, SK, true>;
        static_assert(R == 128 && DC == 32 && S == 512 && EC == 32 && PM == 4 && SK == 4, "the slot form's filter kernel is instantiated for this shape (wn_stacked.hip)");
        e.fn_filter = wn_v3_cfg3_slots_filter_fn();
    }
    return e;
}
static const std::vector<WnV3Kernels>& wn_v3_kernels() {
#define WN_X(R, DC, S, EC, PM, SK) wn_v3_kernels_of<R, DC, S, EC, PM, SK>(),
    static const std::vector<WnV3Kernels> t = {WN_V3_SHAPES(WN_X)};
#undef WN_X
    return t;
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
// The one-shot armings of the NEXT job on a handle: the log-probability output (wn_set_logprob_output) and the forced samples (wn_set_forced_samples)
struct WnArming {
    float* logp_out = nullptr; int64_t logp_capacity = 0; int32_t logp_mode = 0;
    const int32_t* forced_in = nullptr; int64_t forced_capacity = 0;
};
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
    int shape = -1;    // row of wn_chain_shapes() (-1: the generic kernel)
    const void* kern[3] = {nullptr, nullptr, nullptr};   // the chain kernels by wn_kernel_slot (product, diag, extras), resolved at creation (wn_resolve_kernels)
    int threads = 0;   // ... and their workgroup size
    int lds_bytes = 0;
    int v3_mode = 0;    // variant 3: streams per pipeline item (wn_v3_mode_for)
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
    WnArming arm;   // what the NEXT job alone is armed with (wn_generate takes it)
    int prof_recorded = 0;   // stamps held in d_prof
    std::vector<int64_t> ring_off;
    std::vector<int32_t> dil;
    float* d_tws = nullptr; size_t tws_floats = 0;  // training workspace (saved activations + backward temporaries)
    float* d_xent = nullptr; size_t xent_rows = 0;  // wn_train_loss: per-row losses
    double* d_score_part = nullptr; size_t score_parts = 0;  // wn_score: one {sum nll, hits, rows} triple per workgroup
    int32_t* d_ragged = nullptr; size_t ragged_ints = 0;     // wn_prime_ragged: the row tables of all layers, their pinned staging copy, and the event behind
    int32_t* ragged_host = nullptr; hipEvent_t ragged_ev = nullptr;   //   the last upload (the staging copy is rewritten only once that upload has been read)
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

// The chain kernels a handle runs, resolved ONCE at creation into the three slots of wn_kernel_slot (wn_plan.h has the truth table): wn_create sets their
// attributes and checks their occupancy, wn_generate launches the slot of what the job needs (wn_job_slot)
static void wn_resolve_kernels(wn_handle* h) {
    const void* col[3] = {(const void*)wn_generate_kernel, nullptr, nullptr};   // the table's columns: product, DIAG, the slot form's filter kernel
    h->threads = WN_THREADS;
    if (h->variant == 4) {
        const WnV4Kernels& k = wn_v4_kernels()[wn_chain_shapes()[h->shape].index];
        col[0] = k.fn; col[1] = k.fn_diag; h->threads = WN_THREADS_V4;
    } else if (h->variant == 3) {
        const WnV3Kernels& k = wn_v3_kernels()[wn_chain_shapes()[h->shape].index];
        const int form = h->v3_slots ? 2 : (h->v3_mode & 1);
        col[0] = k.fn[form]; col[1] = k.fn_diag[form]; col[2] = k.fn_filter; h->threads = WN_THREADS_V3;
    }
    for (int s = 0; s < 3; ++s) h->kern[s] = col[wn_slot_column(h->variant, h->variant == 3 && h->v3_slots, s)];
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
    rt_free(h->d_ragged);
    if (h->ragged_host) (void)hipHostFree(h->ragged_host);
    if (h->ragged_ev) (void)hipEventDestroy(h->ragged_ev);
    rt_free(h->det_ws[0].buf); rt_free(h->det_ws[1].buf);
    delete h;
}

// wn_create, step 1 validates the configuration (wn_plan.h: wn_config_refusal); step 2: the device (selected on the way)
struct WnDevice { int n_cu = 256, wall_khz = 100000; char busid[32] = ""; };
static int wn_query_device(int device_id, WnDevice* d) {
    int ndev = 0;
    int rc = rt_hip(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    if (rc) return rc;
    if (device_id < 0 || device_id >= ndev) return wn_fail(WN_E_BADARG, "wn_create: device_id %d of %d", device_id, ndev);
    if ((rc = rt_hip(hipSetDevice(device_id), "hipSetDevice"))) return rc;
    hipDeviceProp_t prop;
    if ((rc = rt_hip(hipGetDeviceProperties(&prop, device_id), "hipGetDeviceProperties"))) return rc;
    d->n_cu = prop.multiProcessorCount;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return wn_fail(WN_E_UNSUPPORTED, "wn_create: device %d is %s; this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id) == hipSuccess && khz > 0) d->wall_khz = khz;
    if (hipDeviceGetPCIBusId(d->busid, (int)sizeof(d->busid), device_id) != hipSuccess || !d->busid[0]) snprintf(d->busid, sizeof(d->busid), "dev%d", device_id);
    return WN_OK;
}
// step 3 plans (wn_plan.h: wn_chain_plan, pure) under the development switches, read here once per wn_create
static WnPins wn_read_pins() {
    WnPins p = {};
    p.kernel = wn_dev_env("WN_KERNEL"); p.samplers = wn_dev_env("WN_SAMPLERS"); p.v3_mode = wn_dev_env("WN_V3_MODE"); p.v3_slots = wn_dev_env("WN_V3_SLOTS");
    p.no_rounds = wn_dev_flag("WN_CHAINS"); p.no_local_stores = wn_dev_flag("WN_NO_LOCAL_STORES");
    (void)wn_dev_env("WN_NO_FUSED_SCORE");   // (wn_score reads it per call; a handle created under it says so from the start)
    return p;
}

// steps 4 and 5 for ONE chain: allocate and upload what the plan sizes, resolve the kernels, check their residency
static int wn_build_chain(const WnChainPlan& cp, const WnDevice& dev, wn_handle** out) {
    wn_handle* h = new wn_handle();
    h->cfg = cp.cfg; h->plan = cp.pl;
    { const char* de = getenv("WN_DETERMINISTIC"); h->deterministic = de && de[0] == '1'; }
    h->n_cu = dev.n_cu; h->wall_khz = dev.wall_khz;
    memcpy(h->busid, dev.busid, sizeof(h->busid));
    h->variant = cp.variant; h->shape = cp.row; h->lds_bytes = cp.lds_bytes; h->v3_mode = cp.v3_mode; h->v3_slots = cp.v3_slots; h->gate_need = cp.gate_need;
    h->dil = cp.dil; h->ring_off = cp.ring_off; h->ring_floats = cp.ring_floats; h->gran_count = cp.gran_count; h->blob_floats = cp.blob_floats;
    h->dev_overrides = g_dev_env_used;
    WnPlan& pl = h->plan;
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
        wn_destroy(h);
        return wn_fail(WN_E_NOMEM, "wn_create: device allocation failed (queues %.1f MB, hand-off %.1f MB, weights %.1f MB)", cp.ring_floats * 4e-6,
                       cp.gran_count * 8e-6, cp.blob_floats * 4e-6);
    }
    int rc = 0;
    rc = rc ? rc : rt_h2d(h->d_dil, cp.dil.data(), (size_t)pl.NL * 4);
    rc = rc ? rc : rt_h2d(h->d_ring_off, cp.ring_off.data(), (size_t)pl.NL * 8);
    rc = rc ? rc : rt_h2d(h->d_state_off, cp.state_off.data(), (size_t)(pl.NL + 1) * 8);
    rc = rc ? rc : rt_h2d(h->d_wg_map, cp.wg_map.data(), (size_t)pl.n_blocks * 4);
    rc = rc ? rc : rt_memset_async(h->d_rings, 0, h->ring_floats * 4, nullptr);
    rc = rc ? rc : rt_memset_async(h->d_status, 0, (size_t)WN_STATUS_WORDS(pl.n_wg) * 4, nullptr);
    rc = rc ? rc : rt_sync(nullptr);
    pl.blobs = h->w.d_blobs; pl.start_t = h->w.d_start_t; pl.start_b = nullptr;
    pl.dil = h->d_dil; pl.ring_off = h->d_ring_off; pl.wg_map = h->d_wg_map; pl.rings = h->d_rings;
    pl.gx = h->d_gran; pl.gs = pl.gx + cp.gx_n; pl.gl = pl.gs + cp.gs_n; pl.gi = pl.gl + cp.gl_n; pl.g0 = pl.gi + pl.n_streams;
    pl.status = h->d_status;
    pl.xcc_tab = h->d_status + 8;
    // residency is a requirement, not a hope: what the hardware can keep resident of THESE kernels with THIS much LDS (of the distinct functions among the
    // three slots: the smallest figure), against what the plan needs per XCD
    wn_resolve_kernels(h);
    int per_cu = 0;
    for (int s = 0; s < 3 && !rc; ++s) {
        if ((s > 0 && h->kern[s] == h->kern[0]) || (s > 1 && h->kern[s] == h->kern[1])) continue;
        int n = 0;
        rc = rt_hip(hipFuncSetAttribute(h->kern[s], hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes), "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
        rc = rc ? rc : rt_hip(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, h->kern[s], h->threads, (size_t)h->lds_bytes), "hipOccupancyMaxActiveBlocksPerMultiprocessor");
        if (s == 0 || n < per_cu) per_cu = n;
    }
    if (rc) { wn_destroy(h); return rc; }
    int need = 0, cap = 0;
    wn_gate_numbers(h, &need, &cap);
    h->wg_per_cu = per_cu;
    if ((long long)per_cu * cap < need) {
        wn_destroy(h);
        return wn_fail(WN_E_UNSUPPORTED, "wn_create: the plan keeps %d workgroups resident on one XCD (%d in all), the device holds %d x %d of this kernel there",
                       need, cp.pl.n_wg, cap, per_cu);
    }
    *out = h;
    return WN_OK;
}
// ... and for the plan as a whole: one chain, or the front of a rounds handle over one chain per round (wn_handle::rounds)
static int wn_build_handle(const WnChainPlan& cp, const WnDevice& dev, wn_handle** out) {
    if (cp.rounds.empty()) return wn_build_chain(cp, dev, out);
    wn_handle* f = new wn_handle();
    f->cfg = cp.cfg;
    f->n_cu = dev.n_cu; f->wall_khz = dev.wall_khz; f->variant = cp.variant; f->shape = cp.row; f->lds_bytes = cp.lds_bytes;
    f->v3_mode = cp.v3_mode; f->v3_slots = cp.v3_slots;
    f->dil = cp.dil;
    f->rounds = true;
    f->chain_first.assign(1, 0);
    for (const WnChainPlan& m : cp.rounds) {
        wn_handle* c = nullptr;
        const int rc = wn_build_chain(m, dev, &c);
        if (rc) { wn_destroy(f); return rc; }
        f->chains.push_back(c);
        f->chain_first.push_back(f->chain_first.back() + m.cfg.n_streams);
    }
    f->plan = f->chains[0]->plan;
    f->plan.n_streams = cp.cfg.n_streams;
    *out = f;
    return WN_OK;
}

extern "C" int wn_create(const wn_config* cfg, wn_handle** out) {
    g_err[0] = 0;
    if (!cfg || !out) return wn_fail(WN_E_BADARG, "wn_create: NULL argument");
    *out = nullptr;
    g_dev_env_used = 0;
    std::string why;
    int rc = wn_config_refusal(*cfg, why);
    if (rc) return wn_fail(rc, "wn_create: %s", why.c_str());
    WnDevice dev;
    if ((rc = wn_query_device(cfg->device_id, &dev))) return rc;
    WnPins pins = wn_read_pins();
    const std::vector<WnChainShape>& shapes = wn_chain_shapes();
    for (;;) {
        WnChainPlan cp;
        why = wn_chain_plan(*cfg, dev.n_cu, pins, shapes.data(), (int)shapes.size(), cp);
        if (!why.empty()) return wn_fail(WN_E_UNSUPPORTED, "wn_create: %s", why.c_str());
        rc = wn_build_handle(cp, dev, out);
        if (rc == WN_OK && cp.padded) {   // cfg / plan carry the PADDED channel counts; these are the caller's
            wn_handle* h = *out;
            h->padded = true;
            h->user_R = cfg->residual_channels; h->user_D = cfg->dilation_channels; h->user_S = cfg->skip_channels; h->user_E = cfg->end_channels;
            h->export_R = h->user_R;
            for (wn_handle* c : h->chains) c->export_R = h->user_R;
        }
        // a plan whose handle the device refuses is planned again one step simpler: one chain instead of rounds, then the caller's shape instead of the padded one
        if (rc == WN_E_UNSUPPORTED && !cp.rounds.empty()) pins.no_rounds = true;
        else if (rc != WN_OK && cp.padded) pins.no_padding = true;
        else return rc;
        g_err[0] = 0;
    }
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
            if (c->blob_floats != c0->blob_floats || c->plan.P != c0->plan.P || c->plan.PA != c0->plan.PA || c->variant != c0->variant || c->shape != c0->shape)
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
    if (h->variant == 4) wn_v4_kernels()[wn_chain_shapes()[h->shape].index].pack(pl, hw, blobs);
    else if (h->variant == 3) wn_v3_kernels()[wn_chain_shapes()[h->shape].index].pack(pl, hw, blobs);
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


// ---- the one-shot armings (WnArming).  take: the handle's arming, which the handle then no longer has
static WnArming wn_arming_take(wn_handle* h) { const WnArming a = h->arm; h->arm = WnArming(); return a; }
// check: the armed array holds a value per stream and sample of the job (`fmt`: the refusal, with the capacity, the streams and the samples)
static int wn_arming_check(const void* armed, int64_t capacity, const wn_handle* h, const wn_generate_args* a, const char* fmt) {
    if (!armed || a->num_samples <= 0 || (long long)h->plan.n_streams * (long long)a->num_samples <= (long long)capacity) return WN_OK;
    return wn_fail(WN_E_BADARG, fmt, (long long)capacity, h->plan.n_streams, (long long)a->num_samples);
}
// slice: what a rounds member that owns `n` streams from stream `first` on is armed with (the whole arrays' capacities have been checked)
static WnArming wn_arming_slice(const WnArming& a, size_t first, int n, int64_t num_samples) {
    WnArming m;
    if (a.logp_out) { m.logp_out = a.logp_out + first * (size_t)num_samples; m.logp_capacity = (int64_t)n * num_samples; m.logp_mode = a.logp_mode; }
    if (a.forced_in) { m.forced_in = a.forced_in + first * (size_t)num_samples; m.forced_capacity = (int64_t)n * num_samples; }
    return m;
}
// publish: a pointer into two words of the status block, behind the block's memset on the job's stream: two 32-bit fills, no host buffer to keep alive
static int wn_publish_ptr(uint32_t* at, const void* p, void* stream) {
    const unsigned long long bits = (unsigned long long)(uintptr_t)p;
    const int rc = rt_hip(hipMemsetD32Async((hipDeviceptr_t)at, (int)(uint32_t)bits, 1, (hipStream_t)stream), "hipMemsetD32Async");
    return rc ? rc : rt_hip(hipMemsetD32Async((hipDeviceptr_t)(at + 1), (int)(uint32_t)(bits >> 32), 1, (hipStream_t)stream), "hipMemsetD32Async");
}

extern "C" int wn_generate(wn_handle* h, const wn_generate_args* a) {
    g_err[0] = 0;
    if (!h || !a) return wn_fail(WN_E_BADARG, "wn_generate: NULL argument");
    // what THIS call is armed with is taken here, BOTH armings ahead of either capacity test, whatever becomes of the call -- a job refused for one of them
    // must not leave the other behind for the next job
    const WnArming arm = wn_arming_take(h);
    if (wn_arming_check(arm.logp_out, arm.logp_capacity, h, a, "wn_generate: the log-probability output holds %lld floats, the job writes %d x %lld; nothing was launched") ||
        wn_arming_check(arm.forced_in, arm.forced_capacity, h, a, "wn_generate: the forced samples hold %lld values, the job reads %d x %lld; nothing was launched"))
        return WN_E_BADARG;
    if (!h->have_weights) return wn_fail(WN_E_STATE, "wn_generate: wn_load_weights has not been called");
    if (a->n_given < 1 || a->num_samples < 0) return wn_fail(WN_E_BADARG, "wn_generate: n_given must be >= 1 and num_samples >= 0");
    if (!a->first_samples) return wn_fail(WN_E_BADARG, "wn_generate: first_samples is NULL");
    if (!h->chains.empty()) {   // rounds: member i owns streams [chain_first[i], chain_first[i + 1]); one after the other on the caller's stream
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
            h->chains[i]->arm = wn_arming_slice(arm, s0, h->chain_first[i + 1] - h->chain_first[i], a->num_samples);
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
    if (arm.forced_in && a->num_samples > 0) r.logp |= WN_RUN_FORCED;   // (its pointer travels behind xcc_tab; the forced fork lives where the log-probabilities live)
    r.logp |= arm.logp_out ? 1 + arm.logp_mode : 0;   // (the pointer travels in status[6..7], below; an armed job, a greedy one too, runs the extras slot: wn_job_slot)
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
    if (!rc && arm.logp_out) rc = wn_publish_ptr(h->d_status + 6, arm.logp_out, a->hip_stream);   // (wn_logp_out, wn_kernel.h)
    if (!rc && (r.logp & WN_RUN_FORCED)) rc = wn_publish_ptr(h->d_status + WN_STATUS_FORCED(h->plan.n_wg), arm.forced_in, a->hip_stream);   // (wn_forced_in, wn_kernel.h)
    if (rc) { wn_gate_release(h->gate); h->gate.reset(); return rc; }
    void* args[] = {&h->plan, &r};   // the ONE launch of a chain kernel: the slot of what the job needs
    (void)hipLaunchKernel(h->kern[wn_job_slot(r)], dim3(h->plan.n_blocks), dim3(h->threads), args, (size_t)h->lds_bytes, (hipStream_t)a->hip_stream);
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
    h->arm.logp_out = logp; h->arm.logp_capacity = logp ? capacity : 0; h->arm.logp_mode = logp ? mode : 0;
    return WN_OK;
}

// Forced samples of the NEXT job on the handle (include/wn_abi.h has the contract; wn_generate consumes the arming, the kernels read the status block)
extern "C" int wn_set_forced_samples(wn_handle* h, const int32_t* forced, int64_t capacity) {
    g_err[0] = 0;
    if (capacity < 0) return wn_fail(WN_E_BADARG, "wn_set_forced_samples: capacity must be >= 0, got %lld", (long long)capacity);
    if (!h) return wn_fail(WN_E_BADARG, "wn_set_forced_samples: NULL handle");   // (behind the value check: that one is testable without a device)
    h->arm.forced_in = forced; h->arm.forced_capacity = forced ? capacity : 0;
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
