// wn_sampler_filter_harness.hip -- TEST INFRASTRUCTURE ONLY: the two samplers of the generation chain with the sampling filters (wn_set_sampling), one
// draw per workgroup, on logits handed over bit for bit (tests/test_gpu_sampler_filter_kernels.py).  Like wn_sampler_harness.hip it includes the
// product's runtime unit as it is: wn_sample_1w<true> (wn_kernel_v3.h; <false>, the product form, for the comparison with the filter off) and wn_sample
// (wn_kernel.h) are the code under test, nothing is copied.  The wrappers build the run the samplers read -- zero-filled, `reg`, and the launch's
// top_k / top_p as wn_generate would have normalised them (0 = off) -- call, and store the index.  The product package never loads this library
// (tests/kernels/build_sampler_filter_harness.py).
#include "../../pytorch-wavenet_amd/csrc/wn_runtime.hip"

#define KF_TAIL 64             // floats behind the planner's sampler scratch that must come back untouched
#define KF_SENT 0x7FC0DEADu    // (tests/test_gpu_kernels.py SENT32)

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

// what wn_generate puts into the run: the off values are 0
static int kf_norm_k(int top_k, int C) { return top_k > 0 && top_k < C ? top_k : 0; }
static float kf_norm_p(float top_p) { return top_p > 0.f && top_p < 1.f ? top_p : 0.f; }

extern "C" {

int kf_version() { return 1; }
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

}  // extern "C"
