// wn_kernel_harness.hip -- TEST INFRASTRUCTURE ONLY: the training-time matrix-core kernels launched one at a time (tests/test_gpu_kernels.py).
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

int kh_version() { return 1; }

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

void kh_release() {
    rt_free(kh_det_ws.buf);
    kh_det_ws.buf = nullptr;
    kh_det_ws.floats = 0;
}

}  // extern "C"
