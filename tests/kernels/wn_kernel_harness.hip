// wn_kernel_harness.hip -- TEST INFRASTRUCTURE ONLY: the product's kernels launched one at a time, every group of kernel-level tests in one library:
//   kh_*   the training-time matrix-core kernels (tests/test_gpu_kernels.py) and the inference kernels -- tap product, score head, ring fill, the
//          small layout kernels (tests/test_gpu_infer_kernels.py)
//   kf_*   the generation chain's two samplers, one draw per workgroup (tests/test_gpu_sampler_kernels.py, tests/test_gpu_sampler_filter_kernels.py), and
//          their log-probability and forced forms (kf_logp_*: tests/test_gpu_logp_kernels.py)
//   kst_*  the gather / scatter of a stream's canonical state (tests/test_gpu_state_kernels.py)
//   kt_*   the k-tap training step's input-gradient product (tests/test_gpu_taps_train_kernels.py)
//   kb_*   the bf16 filter/gate product of kernel_size 3 / 4 (tests/test_gpu_taps_bf16_kernels.py)
//   kp_*   the batched-priming kernels: the ragged products, the ragged start gather, the ring fill at a queue time, the history gather
//          (tests/test_gpu_prime_kernels.py)
//
// The product's runtime unit is included as it is, ONCE, so its own static launchers (wn_launch_nn, wn_launch_tn, wn_launch_colsum, wn_launch_layer,
// wn_launch_bwd_layer, ...) and kernels, with their dispatch conditions, are the code under test: nothing is copied.  The entry points take plain
// scalars and device pointers, zero-fill the argument structs as the product does, launch on the given stream and return hipGetLastError().
// A row map is passed as (base, batch_stride, row_stride, t0).  The signatures are bound in tests/kernel_lib.py; a change of any of them raises
// kh_version.  The product package never loads this library (tests/kernels/build_harness.py).
#include "../../pytorch-wavenet_amd/csrc/wn_runtime.hip"

#define KH_MAP(p) const void *p##_base, long long p##_bs, long long p##_rs, long long p##_t0
#define KH_ROWMAP(p) WnRowMap{reinterpret_cast<const float*>(p##_base), p##_bs, p##_rs, p##_t0}

// deterministic mode: the harness's own partial-tile workspace stands in for a handle's while one launcher runs
static WnDetWs kh_det_ws;
struct KhDet {
    explicit KhDet(int det) { t_tn_det[0] = det ? &kh_det_ws : nullptr; t_tn_det[1] = nullptr; t_tn_side = nullptr; }
    ~KhDet() { t_tn_det[0] = nullptr; }
};

// ---------------------------------------------------------------- the samplers' callers (wrappers: kf_*, below)
// wn_sample_1w<true> (wn_kernel_v3.h; <false>, the product form with the filters off) and wn_sample (wn_kernel.h, with wn_smp_carve) on logits handed
// over bit for bit.  Each kernel does what the sampler's caller does around the call and nothing else: load the row, build the run the sampler reads
// -- zero-filled, `reg`, and the launch's top_k / top_p as wn_generate would have normalised them (0 = off) --, call, store the index.  `greedy` is
// the caller's flag (r.greedy != 0 || !(temp > 0)): the samplers take it as an argument.
#define KF_TAIL 64             // floats behind the planner's sampler scratch that must come back untouched
#define KF_SENT 0x7FC0DEADu    // (tests/kernel_lib.py SENT32)

// one 64-thread workgroup per row, lane l holds the classes 4l .. 4l+3; every lane stores the index it got
template <bool FILTER>
__global__ __launch_bounds__(64) void kf_sample_1w_kernel(int top_k, float top_p, const float* logits, const float* reg, const double* u, const int* greedy,
                                                          const float* temp, int* out) {
    const size_t row = blockIdx.x;
    const int lane = (int)threadIdx.x;
    WnRun r;
    memset(&r, 0, sizeof(r));
    r.reg = reg;
    r.top_k = top_k;
    r.top_p = top_p;
    float logit[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) logit[k] = logits[row * 256 + 4 * lane + k];
    out[row * 64 + lane] = wn_sample_1w<FILTER>(r, logit, lane, u[row], greedy[row] != 0, temp[row]);
}

// one WN_THREADS workgroup per row; dynamic LDS = smp_floats (wn_smp_floats) + KF_TAIL sentinel floats
__global__ __launch_bounds__(WN_THREADS) void kf_sample_generic_kernel(int C, int smp_floats, int top_k, float top_p, const float* logits, const float* reg,
                                                                       const double* u, const int* greedy, const float* temp, int* out, uint32_t* tail) {
    extern __shared__ __attribute__((aligned(16))) float kf_lds[];
    const size_t row = blockIdx.x;
    WnPlan pl;
    memset(&pl, 0, sizeof(pl));
    pl.C = C;
    pl.l_smp = 0;
    WnRun r;
    memset(&r, 0, sizeof(r));
    r.reg = reg;
    r.top_k = top_k;
    r.top_p = top_p;
    WnCtx cx{&pl, &r, kf_lds, 0, 0, 0};
    const WnSmp sm = wn_smp_carve(pl, kf_lds);
    WN_PHASE {
        if (tid < KF_TAIL) reinterpret_cast<uint32_t*>(kf_lds)[smp_floats + tid] = KF_SENT;
        for (int i = tid; i < C; i += WN_THREADS) sm.lgt[i] = logits[row * C + i];
    }
    WN_SYNC();
    wn_sample(cx, sm, u[row], greedy[row] != 0, temp[row]);
    WN_PHASE {
        if (tid == 0) out[row] = sm.iscal[0];
        if (tid < KF_TAIL) tail[row * KF_TAIL + tid] = reinterpret_cast<const uint32_t*>(kf_lds)[smp_floats + tid];
    }
}

// ---- the samplers' log-probability and forced forms (wrappers: kf_logp_*, below; tests/test_gpu_logp_kernels.py)
// wn_sample_1w_lp<true, true> as the item loop of wn_kernel_v3.h calls it: `logp_mode` is r.logp's two low bits (0 = off, 1 = sampling, 2 = model: the forced
// bit does not reach the sampler), `forced` one int32 per row, made wave-uniform and turned into -1 outside [0, 256) as the item loop does.  Every lane
// stores its index and its logp; logp starts as the sentinel's bits, so a mode that must not write it shows.
__global__ __launch_bounds__(64) void kf_logp_1w_kernel(int top_k, float top_p, int logp_mode, const float* logits, const float* reg, const double* u, const int* greedy,
                                                        const float* temp, const int* forced, int* out, uint32_t* logp) {
    const size_t row = blockIdx.x;
    const int lane = (int)threadIdx.x;
    WnRun r;
    memset(&r, 0, sizeof(r));
    r.reg = reg;
    r.top_k = top_k;
    r.top_p = top_p;
    r.logp = logp_mode;
    float logit[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) logit[k] = logits[row * 256 + 4 * lane + k];
    const int f = __builtin_amdgcn_readfirstlane(forced[row]);
    float lp = __uint_as_float(KF_SENT);
    out[row * 64 + lane] = wn_sample_1w_lp<true, true>(r, logit, lane, u[row], greedy[row] != 0, temp[row], lp, (uint32_t)f < 256u ? f : -1);
    logp[row * 64 + lane] = __float_as_uint(lp);
}

// wn_sample, the forced fork, wn_sample_logp -- the order of wn_l0_input (wn_kernel.h).  The LDS set-up and the tail sentinel are kf_sample_generic_kernel's.
// The three lines of the forced fork are RESTATED here, not called (in the product they sit inside wn_l0_input, behind the table's pointer): the product's own
// copy of them stays covered by tests/test_gpu_forced.py.  `status` is a device status block the test fills as wn_publish_ptr would (words 6..7: the output
// pointer, NULL = write nothing); the value of row `row` goes to out[row + at0].  logp_mode 0: wn_sample_logp is not called, as in wn_l0_input.
__global__ __launch_bounds__(WN_THREADS) void kf_logp_generic_kernel(int C, int smp_floats, int top_k, float top_p, int logp_mode, uint32_t* status, long long at0,
                                                                     const float* logits, const float* reg, const double* u, const int* greedy, const float* temp,
                                                                     const int* forced, int* out, uint32_t* tail) {
    extern __shared__ __attribute__((aligned(16))) float kf_lds[];
    const size_t row = blockIdx.x;
    WnPlan pl;
    memset(&pl, 0, sizeof(pl));
    pl.C = C;
    pl.l_smp = 0;
    pl.status = status;
    WnRun r;
    memset(&r, 0, sizeof(r));
    r.reg = reg;
    r.top_k = top_k;
    r.top_p = top_p;
    r.logp = logp_mode;
    WnCtx cx{&pl, &r, kf_lds, 0, 0, 0};
    const WnSmp sm = wn_smp_carve(pl, kf_lds);
    WN_PHASE {
        if (tid < KF_TAIL) reinterpret_cast<uint32_t*>(kf_lds)[smp_floats + tid] = KF_SENT;
        for (int i = tid; i < C; i += WN_THREADS) sm.lgt[i] = logits[row * C + i];
    }
    WN_SYNC();
    const bool is_greedy = greedy[row] != 0;
    wn_sample(cx, sm, u[row], is_greedy, temp[row]);
    WN_PHASE {
        if (tid == 0) {
            const int32_t f = forced[row];
            if ((uint32_t)f < (uint32_t)C) sm.iscal[0] = f;
        }
    }
    WN_SYNC();
    if (logp_mode) wn_sample_logp(cx, sm, is_greedy, row + (size_t)at0);
    WN_SYNC();
    WN_PHASE {
        if (tid == 0) out[row] = sm.iscal[0];
        if (tid < KF_TAIL) tail[row * KF_TAIL + tid] = reinterpret_cast<const uint32_t*>(kf_lds)[smp_floats + tid];
    }
}

// what wn_generate puts into the run: the off values are 0
static int kf_norm_k(int top_k, int C) { return top_k > 0 && top_k < C ? top_k : 0; }
static float kf_norm_p(float top_p) { return top_p > 0.f && top_p < 1.f ? top_p : 0.f; }

extern "C" {

int kh_version() { return 5; }

// One NN product through wn_launch_nn.  bn != NULL: the bf16 forms (B as bf16 [N][ldb]); else fp32 with B^T = bt [K][N] (bt1: rows k >= k_split).
int kh_nn(void* stream, int epi, KH_MAP(a0), KH_MAP(a1), int k_split, int K, const float* bt, const float* bt1, int N, const float* bias,
          KH_MAP(cin), KH_MAP(c), long long M, int rows_per_batch, int relu_a, int relu_c, const float* mask, float* gate_t, float* gate_g,
          KH_MAP(c2), int c2_first_row, int gate_packed, int a_skip_lo0, int a_skip_lo1, int a_skip_hi0, int a_skip_hi1, int cin_skip_lo,
          int a_bf16, int c_bf16, unsigned short* c_h, const unsigned short* bn, const unsigned short* bn1, int ldb) {
    WnGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.a0 = KH_ROWMAP(a0); a.a1 = KH_ROWMAP(a1); a.k_split = k_split; a.K = K;
    a.bt = bt; a.bt1 = bt1; a.N = N; a.bias = bias;
    a.cin = KH_ROWMAP(cin); a.c = KH_ROWMAP(c); a.M = M; a.rows_per_batch = rows_per_batch;
    a.relu_a = relu_a; a.relu_c = relu_c; a.mask = mask; a.gate_t = gate_t; a.gate_g = gate_g;
    a.c2 = KH_ROWMAP(c2); a.c2_first_row = c2_first_row; a.gate_packed = gate_packed;
    a.a_skip_lo[0] = a_skip_lo0; a.a_skip_lo[1] = a_skip_lo1; a.a_skip_hi[0] = a_skip_hi0; a.a_skip_hi[1] = a_skip_hi1; a.cin_skip_lo = cin_skip_lo;
    a.a_bf16 = a_bf16; a.c_bf16 = c_bf16; a.c_h = c_h;
    (void)hipGetLastError();
    wn_launch_nn((hipStream_t)stream, epi, a, bn, bn1, ldb);
    return (int)hipGetLastError();
}

// The forward's fused layer (wn_launch_layer): `a` the filter/gate product (GATE epilogue, bf16 A = the shadow of x in two tap views, c_bf16 z),
// `r` the residual product (bias, cin, c, c_h).  Returns -1 when the launcher declines the shape.
int kh_layer(void* stream, KH_MAP(a0), KH_MAP(a1), int k_split, int K, const unsigned short* bn_fg, const float* bias_fg, KH_MAP(z), long long M,
             int rows_per_batch, float* gate_t, KH_MAP(c2), int c2_first_row, int a_skip_lo0, int a_skip_lo1,
             const unsigned short* bn_res, const float* bias_res, KH_MAP(cin), KH_MAP(x), unsigned short* x_h) {
    WnGemmArgs a, r;
    memset(&a, 0, sizeof(a));
    memset(&r, 0, sizeof(r));
    a.a0 = KH_ROWMAP(a0); a.a1 = KH_ROWMAP(a1); a.k_split = k_split; a.K = K; a.N = 256; a.bias = bias_fg; a.c = KH_ROWMAP(z);
    a.M = M; a.rows_per_batch = rows_per_batch; a.gate_t = gate_t; a.gate_packed = 1; a.c2 = KH_ROWMAP(c2); a.c2_first_row = c2_first_row;
    a.a_skip_lo[0] = a_skip_lo0; a.a_skip_lo[1] = a_skip_lo1; a.a_bf16 = 1; a.c_bf16 = 1;
    r.K = 128; r.N = 128; r.bias = bias_res; r.cin = KH_ROWMAP(cin); r.c = KH_ROWMAP(x); r.c_h = x_h; r.M = M; r.rows_per_batch = rows_per_batch;
    (void)hipGetLastError();
    if (!wn_launch_layer((hipStream_t)stream, a, bn_fg, r, bn_res)) return -1;
    return (int)hipGetLastError();
}

// The backward's fused pair (wn_launch_bwd_layer): `a` the dx product (bf16-stored [dF|dG] in two views, banks bn / bn1 of row length ldb, cin = dx',
// c = dx), `b` the gate-derivative product of the layer below on dx (Wres bank bn_res, packed gates, c2 = dzg, bf16 [dF|dG] out).  -1: declined.
int kh_bwd_layer(void* stream, KH_MAP(a0), KH_MAP(a1), int k_split, int K, const unsigned short* bn, const unsigned short* bn1, int ldb, KH_MAP(cin),
                 KH_MAP(dx), long long M, int rows_per_batch, int a_skip_lo0, int a_skip_lo1, int a_skip_hi0, int a_skip_hi1, int cin_skip_lo,
                 const unsigned short* bn_res, float* gates, KH_MAP(dzg), int c2_first_row, KH_MAP(dfg)) {
    WnGemmArgs a, b;
    memset(&a, 0, sizeof(a));
    memset(&b, 0, sizeof(b));
    a.a0 = KH_ROWMAP(a0); a.a1 = KH_ROWMAP(a1); a.k_split = k_split; a.K = K; a.N = 128; a.cin = KH_ROWMAP(cin); a.c = KH_ROWMAP(dx);
    a.M = M; a.rows_per_batch = rows_per_batch; a.a_bf16 = 1; a.cin_skip_lo = cin_skip_lo;
    a.a_skip_lo[0] = a_skip_lo0; a.a_skip_lo[1] = a_skip_lo1; a.a_skip_hi[0] = a_skip_hi0; a.a_skip_hi[1] = a_skip_hi1;
    b.a0 = a.c; b.a1 = a.c; b.k_split = 128; b.K = 128; b.N = 128; b.c = KH_ROWMAP(dfg); b.M = M; b.rows_per_batch = rows_per_batch;
    b.gate_t = gates; b.gate_packed = 1; b.c2 = KH_ROWMAP(dzg); b.c2_first_row = c2_first_row; b.c_bf16 = 1;
    (void)hipGetLastError();
    if (!wn_launch_bwd_layer((hipStream_t)stream, a, bn, bn1, ldb, b, bn_res)) return -1;
    return (int)hipGetLastError();
}

// One weight-gradient product through wn_launch_tn (bf16: the step's bf16 forms), atomics (det = 0) or deterministic (det = 1).
int kh_tn(void* stream, int det, int bf16, KH_MAP(a), const int32_t* a_idx, KH_MAP(b), int Ka, int Nb, float* c, int ldc, long long M,
          int rows_per_batch, int relu_a, KH_MAP(a1), int ka_split, int a_bf16, int b_bf16, int c_trans, int a_skip_lo) {
    WnGemmTnArgs g;
    memset(&g, 0, sizeof(g));
    g.a = KH_ROWMAP(a); g.a_idx = a_idx; g.b = KH_ROWMAP(b); g.Ka = Ka; g.Nb = Nb; g.c = c; g.ldc = ldc; g.M = M;
    g.rows_per_batch = rows_per_batch; g.relu_a = relu_a; g.a1 = KH_ROWMAP(a1); g.ka_split = ka_split;
    g.a_bf16 = a_bf16; g.b_bf16 = b_bf16; g.c_trans = c_trans; g.a_skip_lo = a_skip_lo;
    (void)hipGetLastError();
    KhDet scope(det);
    wn_launch_tn((hipStream_t)stream, g, bf16 != 0);
    return (int)hipGetLastError();
}

// The split plan wn_launch_tn would use for a plain product of this shape (wn_tn_grid, then the 2 GB window rule): out[0] splits, out[1] rows per split.
void kh_tn_grid(long long M, int Ka, int Nb, int tile_nb, int want, long long* out) {
    const WnTnGrid tg = wn_tn_grid(M, Ka, Nb, tile_nb, want);
    out[0] = tg.splits; out[1] = tg.rows_per_split;
}

int kh_colsum(void* stream, int det, KH_MAP(x), long long M, int rows_per_batch, int N, float* out, int x16) {
    (void)hipGetLastError();
    KhDet scope(det);
    wn_launch_colsum((hipStream_t)stream, KH_ROWMAP(x), M, rows_per_batch, N, out, x16 != 0);
    return (int)hipGetLastError();
}

int kh_tn_reduce(void* stream, const float* part, int n_splits, int Ka, int Nb, float* c, int ldc, int c_trans) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_tn_reduce, dim3((unsigned)(((long long)Ka * Nb / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, n_splits, Ka, Nb, c, ldc, c_trans);
    return (int)hipGetLastError();
}

// wn_bwd_gate<packed> with the launch geometry of wn_train_backward (four channels per thread)
int kh_gate_bwd(void* stream, int packed, const float* dz, const float* th, const float* sg, float* dfg, long long M, int D, const float* dzg, int ldg,
                int rows, int out_len) {
    const unsigned blocks = (unsigned)((M * D / 4 + 255) / 256);
    (void)hipGetLastError();
    if (packed) hipLaunchKernelGGL(wn_bwd_gate<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dz, th, sg, dfg, M, D, dzg, ldg, rows, out_len);
    else hipLaunchKernelGGL(wn_bwd_gate<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dz, th, sg, dfg, M, D, dzg, ldg, rows, out_len);
    return (int)hipGetLastError();
}

// wn_xent_rows + wn_xent_reduce as wn_train_backward launches them (scale = 1 / M); dlogits may be NULL
int kh_xent(void* stream, const float* logits, const long long* targets, long long M, float* row_loss, float* dlogits, float* loss) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_xent_rows, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, targets, M, (float)(1.0 / (double)M), row_loss, dlogits);
    hipLaunchKernelGGL(wn_xent_reduce, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_loss, M, 1.0 / (double)M, loss);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- inference kernels (tests/test_gpu_infer_kernels.py)
// The filter/gate product of kernel_size `taps` = 3 or 4 through wn_launch_taps, its arguments filled as wn_layer_fg_taps fills them (a0 = a1 = the view
// of x(t), k_split = R, K = taps * R), with the epilogue fields wn_forward_run adds (c2) and the saved gates.
int kh_taps(void* stream, int taps, KH_MAP(x), long long tap_rows, long long t_min, int R, const float* bt, int N, const float* bias, KH_MAP(z), long long M,
            int rows_per_batch, KH_MAP(c2), int c2_first_row, float* gate_t, float* gate_g, int gate_packed) {
    WnTapsArgs a;
    memset(&a, 0, sizeof(a));
    a.g.a0 = KH_ROWMAP(x); a.g.a1 = KH_ROWMAP(x); a.g.k_split = R; a.g.K = taps * R; a.g.bt = bt; a.g.N = N; a.g.bias = bias;
    a.g.c = KH_ROWMAP(z); a.g.M = M; a.g.rows_per_batch = rows_per_batch;
    a.g.c2 = KH_ROWMAP(c2); a.g.c2_first_row = c2_first_row; a.g.gate_t = gate_t; a.g.gate_g = gate_g; a.g.gate_packed = gate_packed;
    a.tap_rows = tap_rows; a.t_min = t_min;
    if (taps != 3 && taps != 4) return -1;
    (void)hipGetLastError();
    wn_launch_taps((hipStream_t)stream, taps, a);
    return (int)hipGetLastError();
}

// wn_score_head / wn_score_head_bf16 with the grid of wn_forward_run: one workgroup of 256 per WN_SCORE_TM rows, one fp64 triple of `part` each
int kh_score_head(void* stream, int bf16, const float* skip, long long M, int S, int E, const float* w1t, const float* w2t, const unsigned short* w1h,
                  const unsigned short* w2h, const float* b1, const float* b2, const long long* targets, float* row_nll, int* row_pred, double* part) {
    WnScoreArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.skip = skip; sa.M = M; sa.S = S; sa.E = E; sa.w1t = w1t; sa.w2t = w2t; sa.w1h = w1h; sa.w2h = w2h; sa.b1 = b1; sa.b2 = b2;
    sa.targets = targets; sa.row_nll = row_nll; sa.row_pred = row_pred; sa.part = part;
    const unsigned n_part = (unsigned)((M + WN_SCORE_TM - 1) / WN_SCORE_TM);
    (void)hipGetLastError();
    if (bf16) hipLaunchKernelGGL(wn_score_head_bf16, dim3(n_part), dim3(256), 0, (hipStream_t)stream, sa);
    else hipLaunchKernelGGL(wn_score_head, dim3(n_part), dim3(256), 0, (hipStream_t)stream, sa);
    return (int)hipGetLastError();
}

int kh_score_rows(void* stream, const float* logits, int C, const long long* targets, long long M, float* row_nll, int* row_pred, double* part) {
    const unsigned n_part = (unsigned)((M + WN_SCORE_ROWS_PER_WG - 1) / WN_SCORE_ROWS_PER_WG);
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_score_rows, dim3(n_part), dim3(256), 0, (hipStream_t)stream, logits, C, targets, M, row_nll, row_pred, part);
    return (int)hipGetLastError();
}

int kh_score_reduce(void* stream, const double* part, long long n, double* sums) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_score_reduce, dim3(1), dim3(1024), 0, (hipStream_t)stream, part, n, sums);
    return (int)hipGetLastError();
}

// wn_fill_ring with the grid of wn_prime: one thread per float4 of the `count` newest rows of every stream
int kh_fill_ring(void* stream, const float* x, long long x_batch_stride, float* ring, int R, int ML, int n_streams, int P, long long n_time, int count) {
    const long long work = (long long)n_streams * count * (R / 4);
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_fill_ring, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, x_batch_stride, ring, R, ML, n_streams, P, n_time, count);
    return (int)hipGetLastError();
}

// wn_fwd_start as wn_forward_run / wn_train_forward launch it (xh: the bf16 shadow, may be NULL)
int kh_fwd_start(void* stream, const int32_t* idx, const float* start_t, const float* start_b, float* x, long long rows, int R, unsigned short* xh) {
    const long long work = rows * (R / 4);
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_fwd_start, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, start_t, start_b, x, rows, R, xh);
    return (int)hipGetLastError();
}

int kh_cvt_bf16(void* stream, const float* in, unsigned short* out, long long n) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_cvt_bf16, dim3((unsigned)((n / 2 + 256) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n);
    return (int)hipGetLastError();
}

int kh_cvt_bf16_transposed(void* stream, const float* in, long long in_batch_stride, unsigned short* out, int rows, int cols, int batches) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_cvt_bf16_transposed, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)batches), dim3(256), 0, (hipStream_t)stream,
                       in, in_batch_stride, out, rows, cols);
    return (int)hipGetLastError();
}

int kh_transpose_batched(void* stream, const float* in, long long in_batch_stride, float* out, int rows, int cols, int batches) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_transpose_batched, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)batches), dim3(256), 0, (hipStream_t)stream,
                       in, in_batch_stride, out, rows, cols);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- the samplers (tests/test_gpu_sampler_kernels.py: filter_form 0 and top_k = top_p = 0; tests/test_gpu_sampler_filter_kernels.py)
int kf_smp_floats(int C) { return wn_smp_floats(C); }
int kf_run_bytes() { return (int)sizeof(WnRun); }

// out: rows * 64 indices (one per lane).  filter_form 1: wn_sample_1w<true>, 0: wn_sample_1w<false> (which never looks at top_k / top_p)
int kf_sample_1w(void* stream, int filter_form, int rows, int top_k, float top_p, const float* logits, const float* reg, const double* u, const int* greedy,
                 const float* temp, int* out) {
    if (rows < 1 || top_k < 0 || !(top_p >= 0.f && top_p <= 1.f)) return -1;
    (void)hipGetLastError();
    if (filter_form)
        hipLaunchKernelGGL(kf_sample_1w_kernel<true>, dim3(rows), dim3(64), 0, (hipStream_t)stream, kf_norm_k(top_k, 256), kf_norm_p(top_p), logits, reg, u, greedy, temp, out);
    else
        hipLaunchKernelGGL(kf_sample_1w_kernel<false>, dim3(rows), dim3(64), 0, (hipStream_t)stream, 0, 0.f, logits, reg, u, greedy, temp, out);
    return (int)hipGetLastError();
}

// out: rows indices; tail: rows * 64 words, the floats behind the scratch as they are after the draw.  -1: arguments the scratch is not planned for
int kf_sample_generic(void* stream, int rows, int C, int top_k, float top_p, const float* logits, const float* reg, const double* u, const int* greedy,
                      const float* temp, int* out, uint32_t* tail) {
    if (rows < 1 || C < 1 || C > 4096 || top_k < 0 || !(top_p >= 0.f && top_p <= 1.f)) return -1;
    const int smp_floats = wn_smp_floats(C);
    (void)hipGetLastError();
    hipLaunchKernelGGL(kf_sample_generic_kernel, dim3(rows), dim3(WN_THREADS), (size_t)(smp_floats + KF_TAIL) * sizeof(float), (hipStream_t)stream, C, smp_floats,
                       kf_norm_k(top_k, C), kf_norm_p(top_p), logits, reg, u, greedy, temp, out, tail);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- the samplers' log-probability and forced forms (tests/test_gpu_logp_kernels.py)
// out: rows * 64 indices, logp: rows * 64 words (one of each per lane).  logp_mode: r.logp & WN_RUN_LOGP_MASK, 0 .. 2; forced: one int32 per row
int kf_logp_1w(void* stream, int rows, int top_k, float top_p, int logp_mode, const float* logits, const float* reg, const double* u, const int* greedy,
               const float* temp, const int* forced, int* out, uint32_t* logp) {
    if (rows < 1 || top_k < 0 || !(top_p >= 0.f && top_p <= 1.f) || logp_mode < 0 || logp_mode > 2) return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kf_logp_1w_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, kf_norm_k(top_k, 256), kf_norm_p(top_p), logp_mode, logits, reg, u, greedy, temp,
                       forced, out, logp);
    return (int)hipGetLastError();
}

// out: rows indices; tail: as kf_sample_generic; status: 8 device words, 6..7 the pointer the values go to (row `row` to element row + at0), or NULL
int kf_logp_generic(void* stream, int rows, int C, int top_k, float top_p, int logp_mode, uint32_t* status, long long at0, const float* logits, const float* reg,
                    const double* u, const int* greedy, const float* temp, const int* forced, int* out, uint32_t* tail) {
    if (rows < 1 || C < 1 || C > 4096 || top_k < 0 || !(top_p >= 0.f && top_p <= 1.f) || logp_mode < 0 || logp_mode > 2 || at0 < 0 || !status) return -1;
    const int smp_floats = wn_smp_floats(C);
    (void)hipGetLastError();
    hipLaunchKernelGGL(kf_logp_generic_kernel, dim3(rows), dim3(WN_THREADS), (size_t)(smp_floats + KF_TAIL) * sizeof(float), (hipStream_t)stream, C, smp_floats,
                       kf_norm_k(top_k, C), kf_norm_p(top_p), logp_mode, status, at0, logits, reg, u, greedy, temp, forced, out, tail);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- generation state (tests/test_gpu_state_kernels.py)
// wn_state_gather / wn_state_scatter (csrc/wn_state.inl) on rings the test makes up, through the product's own launchers (which choose the float4 or the
// scalar kernel).  The tables (ring offsets, canonical row offsets, dilations) are DEVICE arrays the test uploads, as wn_create does.

// 1 iff the launchers take the float4 kernels for this geometry and state pointer
int kst_vec(int R, int R_own, const float* state) {
    WnStateGeom g = {};
    g.R = R; g.R_own = R_own;
    return wn_state_vec(g, state) ? 1 : 0;
}

int kst_gather(void* stream, const int64_t* ring_off, const int64_t* row_off, const int32_t* dil, int NL, int k, int R, int R_own, int n_streams, int P,
               long long rows, const float* rings, long long t, int s, float* state) {
    if (NL < 1 || s < 0 || s >= n_streams || R_own > R || rows < 1) return -1;
    const WnStateGeom g{ring_off, row_off, dil, NL, k, R, R_own, n_streams, P};
    (void)hipGetLastError();
    wn_state_launch_gather((hipStream_t)stream, g, rows, rings, t, s, state);
    return (int)hipGetLastError();
}

int kst_scatter(void* stream, const int64_t* ring_off, const int64_t* row_off, const int32_t* dil, int NL, int k, int R, int R_own, int n_streams, int P,
                long long rows, float* rings, long long t, int s0, int count, const float* state) {
    if (NL < 1 || s0 < 0 || count < 1 || s0 + count > n_streams || R_own > R || rows < 1) return -1;
    const WnStateGeom g{ring_off, row_off, dil, NL, k, R, R_own, n_streams, P};
    (void)hipGetLastError();
    wn_state_launch_scatter((hipStream_t)stream, g, rows, rings, t, s0, count, state);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- the k-tap input-gradient product (tests/test_gpu_taps_train_kernels.py)
// wn_launch_taps_bwd -> wn_bwd_gemm_taps<3>, <4>.  The argument struct is filled field by field as wn_layer_dx_taps (csrc/wn_forward.inl) fills it, with
// every quantity that function derives passed in instead, so that the kernel's row windows can be driven apart from the training step's geometry.

// dx = (cin on the rows >= cin_skip_lo of an entry) + sum_j a(t + (taps-1-j) tap_rows) . B_j: `a` = the view of [dF|dG](t) (rows of two_d floats that
// exist for t in [t_lo, t_hi)), B_j = bt + j * bt_tap_stride, [two_d][N].  -1: not a kernel size of the launcher.
int kt_bwd_taps(void* stream, int taps, KH_MAP(a), long long tap_rows, long long t_lo, long long t_hi, int two_d, const float* bt, long long bt_tap_stride, int N,
                KH_MAP(cin), int cin_skip_lo, KH_MAP(c), long long M, int rows_per_batch) {
    WnTapsBwdArgs x;
    memset(&x, 0, sizeof(x));
    x.g.a0 = KH_ROWMAP(a); x.g.a1 = KH_ROWMAP(a); x.g.k_split = two_d; x.g.K = taps * two_d; x.g.bt = bt; x.g.N = N;
    x.g.cin = KH_ROWMAP(cin); x.g.cin_skip_lo = cin_skip_lo; x.g.c = KH_ROWMAP(c); x.g.M = M; x.g.rows_per_batch = rows_per_batch;
    x.tap_rows = tap_rows; x.t_lo = t_lo; x.t_hi = t_hi; x.bt_tap_stride = bt_tap_stride;
    if (taps != 3 && taps != 4) return -1;
    (void)hipGetLastError();
    wn_launch_taps_bwd((hipStream_t)stream, taps, x);
    return (int)hipGetLastError();
}

// The same product with its arguments built by the training step's own helper (wn_layer_dx_taps): dense [dF|dG] of rows_dfg rows per entry, dx and dx'
// on the rows_out trailing rows of clips of L rows of R floats (dxin == NULL: the last layer's form, no addend).
int kt_layer_dx(void* stream, int taps, int R, int D, const float* dfg, long long rows_dfg, long long rows_out, long long d, const float* btT, long long tap_stride,
                const float* dxin, float* dx, long long L, long long n) {
    if (taps != 3 && taps != 4) return -1;
    WnPlan pl;
    memset(&pl, 0, sizeof(pl));
    pl.R = R; pl.D = D; pl.k = taps;
    const WnTapsBwdArgs x = wn_layer_dx_taps(pl, dfg, rows_dfg, rows_out, d, btT, tap_stride, dxin ? wn_rows(dxin, L, R, L - rows_out) : WnRowMap{nullptr, 0, 0, 0},
                                             wn_rows(dx, L, R, L - rows_out), n);
    (void)hipGetLastError();
    wn_launch_taps_bwd((hipStream_t)stream, taps, x);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- the bf16 tap product (tests/test_gpu_taps_bf16_kernels.py)
// wn_launch_taps_bf16 -> wn_fwd_gemm_taps_bf16<3 | 4, 4 | 8>, its arguments filled as kh_taps fills them.

// z = gate([x(t - (taps-1) tap_rows) | ... | x(t)] . B^T + bias): x fp32 rows of R floats, B = bn, bf16 [N][taps * R].  -1: not a kernel size of the launcher.
int kb_taps_bf16(void* stream, int taps, KH_MAP(x), long long tap_rows, long long t_min, int R, const unsigned short* bn, int N, const float* bias, KH_MAP(z),
                 long long M, int rows_per_batch, KH_MAP(c2), int c2_first_row) {
    WnTapsArgs a;
    memset(&a, 0, sizeof(a));
    a.g.a0 = KH_ROWMAP(x); a.g.a1 = KH_ROWMAP(x); a.g.k_split = R; a.g.K = taps * R; a.g.N = N; a.g.bias = bias;
    a.g.c = KH_ROWMAP(z); a.g.M = M; a.g.rows_per_batch = rows_per_batch;
    a.g.c2 = KH_ROWMAP(c2); a.g.c2_first_row = c2_first_row;
    a.tap_rows = tap_rows; a.t_min = t_min;
    if (taps != 3 && taps != 4) return -1;
    (void)hipGetLastError();
    wn_launch_taps_bf16((hipStream_t)stream, taps, a, bn);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- batched priming (tests/test_gpu_prime_kernels.py)
// The kernels wn_prime_pass (csrc/wn_forward.inl) launches for the ragged and the append forms, with the fields and the grid expressions it uses.  A row
// table is passed as (start, n_streams, t_end): start = the prefix sums of the streams' row counts, a DEVICE array of n_streams + 1 ints.

// wn_launch_nn(st, epi, a, nullptr, nullptr, 0, &rg) -> wn_fwd_gemm_ragged<GATE | PLAIN>: what wn_layer_fg (a0 = x(t - d), a1 = x(t), k_split = R) and
// wn_layer_res (a0 = a1 = z, cin = x(t)) fill, rows_per_batch = M as one entry of the table's total.  -1: an epilogue the ragged kernels do not have.
int kp_nn_ragged(void* stream, int epi, KH_MAP(a0), KH_MAP(a1), int k_split, int K, const float* bt, int N, const float* bias, KH_MAP(cin), KH_MAP(c), long long M,
                 const int32_t* start, int n_streams, int t_end) {
    WnGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.a0 = KH_ROWMAP(a0); a.a1 = KH_ROWMAP(a1); a.k_split = k_split; a.K = K; a.bt = bt; a.N = N; a.bias = bias;
    a.cin = KH_ROWMAP(cin); a.c = KH_ROWMAP(c); a.M = M; a.rows_per_batch = (int)M;
    const WnRagged rg{start, n_streams, t_end};
    if (epi != WN_EPI_GATE && epi != WN_EPI_PLAIN) return -1;
    (void)hipGetLastError();
    wn_launch_nn((hipStream_t)stream, epi, a, nullptr, nullptr, 0, &rg);
    return (int)hipGetLastError();
}

// wn_launch_taps(st, taps, a, &rg) -> wn_fwd_gemm_taps_ragged<3 | 4>, filled as wn_layer_fg_taps fills it (t_min = the first row in front of a stream's
// time 0 that exists: -Lp).  -1: not a kernel size of the launcher.
int kp_taps_ragged(void* stream, int taps, KH_MAP(x), long long tap_rows, long long t_min, int R, const float* bt, int N, const float* bias, KH_MAP(c), long long M,
                   const int32_t* start, int n_streams, int t_end) {
    WnTapsArgs a;
    memset(&a, 0, sizeof(a));
    a.g.a0 = KH_ROWMAP(x); a.g.a1 = KH_ROWMAP(x); a.g.k_split = R; a.g.K = taps * R; a.g.bt = bt; a.g.N = N; a.g.bias = bias;
    a.g.c = KH_ROWMAP(c); a.g.M = M; a.g.rows_per_batch = (int)M;
    a.tap_rows = tap_rows; a.t_min = t_min;
    const WnRagged rg{start, n_streams, t_end};
    if (taps != 3 && taps != 4) return -1;
    (void)hipGetLastError();
    wn_launch_taps((hipStream_t)stream, taps, a, &rg);
    return (int)hipGetLastError();
}

// wn_fwd_start_ragged with the grid of wn_prime_pass: one thread per float4 of the table's `rows` rows (no launch for an empty table)
int kp_fwd_start_ragged(void* stream, const int32_t* idx, long long idx_stride, const float* start_t, const float* start_b, float* x, long long x_stream_stride,
                        const int32_t* start, int n_streams, int t_end, long long rows, int R) {
    const long long work = rows * (R / 4);
    const WnRagged rg{start, n_streams, t_end};
    (void)hipGetLastError();
    if (work > 0)
        hipLaunchKernelGGL(wn_fwd_start_ragged, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, idx_stride, start_t, start_b, x, x_stream_stride,
                           rg, rows, R);
    return (int)hipGetLastError();
}

// wn_fill_ring_at with the grid of wn_prime_pass: one thread per float4 of the `count` newest rows of every stream (x_batch_stride 0: the shared form)
int kp_fill_ring_at(void* stream, const float* x, long long x_batch_stride, float* ring, int R, int ML, int n_streams, int P, long long n_time, int count,
                    long long t_base) {
    const long long work = (long long)n_streams * count * (R / 4);
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_fill_ring_at, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, x_batch_stride, ring, R, ML, n_streams, P, n_time, count, t_base);
    return (int)hipGetLastError();
}

// wn_prime_gather_history with the grid of wn_prime_pass: one thread per float4 of the ML history rows of every stream.  start == NULL: the rectangle form
// (every stream appends n_time rows); else table 0 of the row tables, {start, n_streams, n_time}.
int kp_gather_history(void* stream, const float* ring, int R, int ML, int n_streams, float* x, long long x_batch_stride, long long Lp, long long n_time,
                      long long t_base, const int32_t* start) {
    const long long work = (long long)n_streams * ML * (R / 4);
    const WnRagged rg = start ? WnRagged{start, n_streams, (int)n_time} : WnRagged{nullptr, 0, 0};
    (void)hipGetLastError();
    hipLaunchKernelGGL(wn_prime_gather_history, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ring, R, ML, n_streams, x, x_batch_stride, Lp, n_time,
                       t_base, rg);
    return (int)hipGetLastError();
}

void kh_release() {
    rt_free(kh_det_ws.buf);
    kh_det_ws.buf = nullptr;
    kh_det_ws.floats = 0;
}

}  // extern "C"
