// wn_state_harness.hip -- TEST INFRASTRUCTURE ONLY: the two kernels that move a stream's canonical state out of and into the dilation rings
// (csrc/wn_state.inl: wn_state_gather, wn_state_scatter), alone, on rings the test makes up (tests/test_gpu_state_kernels.py).  Like the other harnesses
// it includes the product's runtime unit as it is; the wrappers fill the geometry struct and go through the product's own launchers (which choose the
// float4 or the scalar kernel).  The tables (ring offsets, canonical row offsets, dilations) are DEVICE arrays the test uploads, as wn_create does.  The
// product package never loads this library (tests/kernels/build_state_harness.py).
#include "../../pytorch-wavenet_amd/csrc/wn_runtime.hip"

extern "C" {

int kst_version() { return 1; }

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

}  // extern "C"
