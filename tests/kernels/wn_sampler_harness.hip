// wn_sampler_harness.hip -- TEST INFRASTRUCTURE ONLY: the two samplers of the generation chain, one draw per workgroup, on logits handed over bit for
// bit (tests/test_gpu_sampler_kernels.py).  Like wn_kernel_harness.hip it includes the product's runtime unit as it is: wn_sample (wn_kernel.h, with
// wn_smp_carve) and wn_sample_1w (wn_kernel_v3.h, with the wave helpers of wn_chain_regs.h) are the code under test, nothing is copied.  Each wrapper
// does what the sampler's caller does around the call and nothing else: load the row, build the zero-filled run / plan the sampler reads (`reg`, `C`,
// `l_smp`), call, store the index.  `greedy` is the caller's flag (r.greedy != 0 || !(temp > 0)): the samplers take it as an argument.  The product
// package never loads this library (tests/kernels/build_sampler_harness.py).
#include "../../pytorch-wavenet_amd/csrc/wn_runtime.hip"

#define KS_TAIL 64             // floats behind the planner's sampler scratch that must come back untouched
#define KS_SENT 0x7FC0DEADu    // (tests/test_gpu_kernels.py SENT32)

// one 64-thread workgroup per row, lane l holds the classes 4l .. 4l+3; EVERY lane stores the index it got (the caller gathers its piece of the
// start_conv row with it: the result has to be wave-uniform)
__global__ __launch_bounds__(64) void ks_sample_1w_kernel(const float* logits, const float* reg, const double* u, const int* greedy, const float* temp, int* out) {
    const size_t row = blockIdx.x;
    const int lane = (int)threadIdx.x;
    WnRun r;
    memset(&r, 0, sizeof(r));
    r.reg = reg;
    float logit[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) logit[k] = logits[row * 256 + 4 * lane + k];
    out[row * 64 + lane] = wn_sample_1w(r, logit, lane, u[row], greedy[row] != 0, temp[row]);
}

// one WN_THREADS workgroup per row; dynamic LDS = smp_floats (what the planner reserves for the scratch: wn_smp_floats) + KS_TAIL sentinel floats
__global__ __launch_bounds__(WN_THREADS) void ks_sample_generic_kernel(int C, int smp_floats, const float* logits, const float* reg, const double* u, const int* greedy,
                                                                       const float* temp, int* out, uint32_t* tail) {
    extern __shared__ __attribute__((aligned(16))) float ks_lds[];
    const size_t row = blockIdx.x;
    WnPlan pl;
    memset(&pl, 0, sizeof(pl));
    pl.C = C;
    pl.l_smp = 0;
    WnRun r;
    memset(&r, 0, sizeof(r));
    r.reg = reg;
    WnCtx cx{&pl, &r, ks_lds, 0, 0, 0};
    const WnSmp sm = wn_smp_carve(pl, ks_lds);
    WN_PHASE {
        if (tid < KS_TAIL) reinterpret_cast<uint32_t*>(ks_lds)[smp_floats + tid] = KS_SENT;
        for (int i = tid; i < C; i += WN_THREADS) sm.lgt[i] = logits[row * C + i];
    }
    WN_SYNC();
    wn_sample(cx, sm, u[row], greedy[row] != 0, temp[row]);
    WN_PHASE {
        if (tid == 0) out[row] = sm.iscal[0];
        if (tid < KS_TAIL) tail[row * KS_TAIL + tid] = reinterpret_cast<const uint32_t*>(ks_lds)[smp_floats + tid];
    }
}

extern "C" {

int ks_version() { return 1; }
int ks_smp_floats(int C) { return wn_smp_floats(C); }

// out: rows * 64 indices (one per lane)
int ks_sample_1w(void* stream, int rows, const float* logits, const float* reg, const double* u, const int* greedy, const float* temp, int* out) {
    if (rows < 1) return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ks_sample_1w_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, logits, reg, u, greedy, temp, out);
    return (int)hipGetLastError();
}

// out: rows indices; tail: rows * 64 words, the floats behind the scratch as they are after the draw.  -1: a class count the scratch is not planned for
int ks_sample_generic(void* stream, int rows, int C, const float* logits, const float* reg, const double* u, const int* greedy, const float* temp, int* out,
                      uint32_t* tail) {
    if (rows < 1 || C < 1 || C > 4096) return -1;
    const int smp_floats = wn_smp_floats(C);
    (void)hipGetLastError();
    hipLaunchKernelGGL(ks_sample_generic_kernel, dim3(rows), dim3(WN_THREADS), (size_t)(smp_floats + KS_TAIL) * sizeof(float), (hipStream_t)stream, C, smp_floats,
                       logits, reg, u, greedy, temp, out, tail);
    return (int)hipGetLastError();
}

}  // extern "C"
