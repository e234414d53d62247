// wn_kernel_harness.hip -- TEST INFRASTRUCTURE ONLY: the product's kernels launched one at a time: the training-time matrix-core kernels
// (tests/test_gpu_kernels.py) and the inference kernels -- tap product, score head, ring fill, the small layout kernels (tests/test_gpu_infer_kernels.py).
//
// The product's runtime unit is included as it is, so its own static launchers (wn_launch_nn, wn_launch_tn, wn_launch_colsum, wn_launch_layer,
// wn_launch_bwd_layer) and kernels, with their dispatch conditions, are the code under test: nothing is copied.  The entry points take plain
// scalars and device pointers, zero-fill the argument structs as the product does, launch on the given stream and return hipGetLastError().
// A row map is passed as (base, batch_stride, row_stride, t0).  The product package never loads this library (tests/kernels/build_harness.py).
#include "../../pytorch-wavenet_amd/csrc/wn_runtime.hip"

#define KH_MAP(p) const void *p##_base, long long p##_bs, long long p##_rs, long long p##_t0
#define KH_ROWMAP(p) WnRowMap{reinterpret_cast<const float*>(p##_base), p##_bs, p##_rs, p##_t0}

// deterministic mode: the harness's own partial-tile workspace stands in for a handle's while one launcher runs
static WnDetWs kh_det_ws;
struct KhDet {
    explicit KhDet(int det) { t_tn_det[0] = det ? &kh_det_ws : nullptr; t_tn_det[1] = nullptr; t_tn_side = nullptr; }
    ~KhDet() { t_tn_det[0] = nullptr; }
};

extern "C" {

int kh_version() { return 2; }

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

void kh_release() {
    rt_free(kh_det_ws.buf);
    kh_det_ws.buf = nullptr;
    kh_det_ws.floats = 0;
}

}  // extern "C"
