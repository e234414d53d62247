// wn_stacked_table.h -- the table of instantiated stacked-layer kernels (variant 4, wn_kernel_v4.h), shared by the two translation units of the
// library: wn_stacked.hip DEFINES the table (kernel instantiations, weight packers, launchers), wn_runtime.hip plans and launches through it.
// Why two translation units (round 6): the library's persistent chains are compiled with -mllvm -align-all-nofallthru-blocks=6 (build.py: +0.5 % on the
// 64-stream headline), a per-translation-unit switch -- and the stacked kernels LOSE 1.2-1.3 % with it (same-box A/B of one source, three passes:
// cfg2 x 1 48.9 k with / 49.5 k without, cfg1 x 1 131.5 k / 133.1 k: profiles/r06_small_shape_regression_ab.txt).  They get a unit of their own, built without it.
#ifndef WN_STACKED_TABLE_H
#define WN_STACKED_TABLE_H

#include <hip/hip_runtime.h>

#include <vector>

#include "wn_plan.h"

#ifndef WN_THREADS_V4
#define WN_THREADS_V4 512   // threads of a stack workgroup (wn_kernel_v4.h)
#endif

// Shapes the stacked kernel (wn_kernel_v4.h: LPW consecutive layers per 512-thread workgroup) is instantiated for: (R, D, S, E / PA, LPW).
// LPW is what one CU's register file holds next to the working set: cfg2 60 registers per layer and lane (tap 0 lives in LDS), cfg1 32,
// the train_script.py shape 83 (its 1024 skip rows).
struct WnV4Entry {
    int R, D, S, EC, LPW, nwpl, nwh;
    void (*pack)(const WnPlan& pl, const WnHostWeights& w, std::vector<float>& out);
    const void* fn;        // the product instantiation
    const void* fn_diag;   // ... and the one with the stamps and the logits dump (a job with wn_profile_next or dbg_logits)
    int (*lds_floats)(int ns);
    int lds_pre_head;   // float offset of the head / sampler workgroups' own tables (WnV3Lds<SH>::pre)
    void (*launch)(bool diag, int grid, size_t lds, hipStream_t st, const WnPlan& p, const WnRun& r);
};

const std::vector<WnV4Entry>& wn_v4_table();

// One kernel of the wave-specialised family lives in wn_stacked.hip too: the slot re-use form of cfg3 WITH the sampling filters
// (wn_kernel_v3.h: wn_generate_kernel_v3m_filter<128, 32, 512, 32, 4, 2, 4>).  In wn_runtime.hip it would be a second caller of the layer role that form's
// own kernel instantiates, and that alone moves the instruction stream of that kernel -- the one unfiltered jobs of 96 streams and more run, whose
// schedule is sensitive (wn_runtime.hip: wn_v2_entry).  Here it is the role's only caller, and the other unit compiles as if it did not exist.
const void* wn_v3_cfg3_slots_filter_fn();
void wn_v3_cfg3_slots_filter_launch(int grid, size_t lds, hipStream_t st, const WnPlan& p, const WnRun& r);

#endif  // WN_STACKED_TABLE_H
