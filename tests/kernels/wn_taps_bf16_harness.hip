// wn_taps_bf16_harness.hip -- TEST INFRASTRUCTURE ONLY: the bf16 filter/gate product of kernel_size 3 / 4 (wn_fwd_gemm_taps_bf16<3 | 4, 4 | 8>) launched
// one product at a time through its own launcher (tests/test_gpu_taps_bf16_kernels.py).  Like wn_kernel_harness.hip it includes the product's runtime
// unit as it is: wn_launch_taps_bf16 and the kernels are the code under test, nothing is copied.  The argument struct is zero-filled and filled as
// wn_layer_fg_taps (csrc/wn_forward.inl) fills it (a0 = a1 = the view of x(t), k_split = R, K = taps * R), with the epilogue fields wn_forward_run
// adds (c2).  A row map is (base, batch_stride, row_stride, t0).  The product package never loads this library (tests/kernels/build_taps_bf16_harness.py).
#include "../../pytorch-wavenet_amd/csrc/wn_runtime.hip"

#define KB_MAP(p) const void *p##_base, long long p##_bs, long long p##_rs, long long p##_t0
#define KB_ROWMAP(p) WnRowMap{reinterpret_cast<const float*>(p##_base), p##_bs, p##_rs, p##_t0}

extern "C" {

int kb_version() { return 1; }

// z = gate([x(t - (taps-1) tap_rows) | ... | x(t)] . B^T + bias): x fp32 rows of R floats, B = bn, bf16 [N][taps * R].  -1: not a kernel size of the launcher.
int kb_taps_bf16(void* stream, int taps, KB_MAP(x), long long tap_rows, long long t_min, int R, const unsigned short* bn, int N, const float* bias, KB_MAP(z),
                 long long M, int rows_per_batch, KB_MAP(c2), int c2_first_row) {
    WnTapsArgs a;
    memset(&a, 0, sizeof(a));
    a.g.a0 = KB_ROWMAP(x); a.g.a1 = KB_ROWMAP(x); a.g.k_split = R; a.g.K = taps * R; a.g.N = N; a.g.bias = bias;
    a.g.c = KB_ROWMAP(z); a.g.M = M; a.g.rows_per_batch = rows_per_batch;
    a.g.c2 = KB_ROWMAP(c2); a.g.c2_first_row = c2_first_row;
    a.tap_rows = tap_rows; a.t_min = t_min;
    if (taps != 3 && taps != 4) return -1;
    (void)hipGetLastError();
    wn_launch_taps_bf16((hipStream_t)stream, taps, a, bn);
    return (int)hipGetLastError();
}

}  // extern "C"
