// wn_stacked_table.h -- the table of instantiated stacked-layer kernels (variant 4, wn_kernel_v4.h), shared by the two translation units of the
// library: wn_stacked.hip DEFINES the table (kernel instantiations, weight packers), wn_runtime.hip launches through it.
// Why two translation units (round 6): the library's persistent chains are compiled with -mllvm -align-all-nofallthru-blocks=6 (build.py: +0.5 % on the
// 64-stream headline), a per-translation-unit switch -- and the stacked kernels LOSE 1.2-1.3 % with it (same-box A/B of one source, three passes:
// cfg2 x 1 48.9 k with / 49.5 k without, cfg1 x 1 131.5 k / 133.1 k: profiles/r06_small_shape_regression_ab.txt).  They get a unit of their own, built without it.
#ifndef WN_STACKED_TABLE_H
#define WN_STACKED_TABLE_H

#include <hip/hip_runtime.h>

#include <vector>

#include "wn_chain_shapes.h"
#include "wn_plan.h"

#ifndef WN_THREADS_V4
#define WN_THREADS_V4 512   // threads of a stack workgroup (wn_kernel_v4.h)
#endif

// The stacked kernels' pointer table: one row per shape of WN_V4_SHAPES (wn_chain_shapes.h, where the planner's facts of the same rows are computed)
struct WnV4Kernels {
    void (*pack)(const WnPlan& pl, const WnHostWeights& w, std::vector<float>& out);
    const void* fn;        // the product instantiation
    const void* fn_diag;   // ... and the one with the stamps and the logits dump
};
const std::vector<WnV4Kernels>& wn_v4_kernels();

// One kernel of the wave-specialised family lives in wn_stacked.hip too: the slot re-use form of cfg3 WITH the sampling filters
// (wn_kernel_v3.h: wn_generate_kernel_v3m_filter<128, 32, 512, 32, 4, 2, 4>).  In wn_runtime.hip it would be a second caller of the layer role that form's
// own kernel instantiates, and that alone moves the instruction stream of that kernel -- the one unfiltered jobs of 96 streams and more run, whose
// schedule is sensitive (wn_runtime.hip: wn_v3_kernels_of).  Here it is the role's only caller, and the other unit compiles as if it did not exist.
const void* wn_v3_cfg3_slots_filter_fn();

#endif  // WN_STACKED_TABLE_H
