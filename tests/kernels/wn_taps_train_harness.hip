// wn_taps_train_harness.hip -- TEST INFRASTRUCTURE ONLY: the k-tap training step's input-gradient product (wn_bwd_gemm_taps<3>, <4>) launched one
// product at a time through its own launcher (tests/test_gpu_taps_train_kernels.py).  Like wn_kernel_harness.hip it includes the product's runtime
// unit as it is: wn_launch_taps_bwd and the kernels are the code under test, nothing is copied.  The argument struct is zero-filled and filled field
// by field as wn_layer_dx_taps (csrc/wn_forward.inl) fills it, with every quantity that function derives passed in instead, so that the kernel's row
// windows can be driven apart from the training step's geometry.  A row map is (base, batch_stride, row_stride, t0).  The product package never
// loads this library (tests/kernels/build_taps_train_harness.py).
#include "../../pytorch-wavenet_amd/csrc/wn_runtime.hip"

#define KT_MAP(p) const void *p##_base, long long p##_bs, long long p##_rs, long long p##_t0
#define KT_ROWMAP(p) WnRowMap{reinterpret_cast<const float*>(p##_base), p##_bs, p##_rs, p##_t0}

extern "C" {

int kt_version() { return 1; }

// dx = (cin on the rows >= cin_skip_lo of an entry) + sum_j a(t + (taps-1-j) tap_rows) . B_j: `a` = the view of [dF|dG](t) (rows of two_d floats that
// exist for t in [t_lo, t_hi)), B_j = bt + j * bt_tap_stride, [two_d][N].  -1: not a kernel size of the launcher.
int kt_bwd_taps(void* stream, int taps, KT_MAP(a), long long tap_rows, long long t_lo, long long t_hi, int two_d, const float* bt, long long bt_tap_stride, int N,
                KT_MAP(cin), int cin_skip_lo, KT_MAP(c), long long M, int rows_per_batch) {
    WnTapsBwdArgs x;
    memset(&x, 0, sizeof(x));
    x.g.a0 = KT_ROWMAP(a); x.g.a1 = KT_ROWMAP(a); x.g.k_split = two_d; x.g.K = taps * two_d; x.g.bt = bt; x.g.N = N;
    x.g.cin = KT_ROWMAP(cin); x.g.cin_skip_lo = cin_skip_lo; x.g.c = KT_ROWMAP(c); x.g.M = M; x.g.rows_per_batch = rows_per_batch;
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

}  // extern "C"
