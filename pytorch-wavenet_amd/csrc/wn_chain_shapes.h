// wn_chain_shapes.h -- the instantiated shapes of the generation chain's register-resident kernels, listed ONCE.  The kernel pointer tables of the two
// translation units (wn_runtime.hip: variant 3, wn_stacked.hip: variant 4 -- wn_stacked_table.h says why two) and the planner's table of facts
// (wn_plan.h: WnChainShape) are generated from these lists; so are the rows of the planner tests.  The lists are plain preprocessor text; the facts below
// need the device headers but name no kernel, so a host-only harness that includes this file links without device code.  Anything that is not listed
// runs on the generic LDS-resident kernel (or zero-padded into a listed shape: wn_pad_config).
#ifndef WN_CHAIN_SHAPES_H
#define WN_CHAIN_SHAPES_H

// The wave-specialised kernel (wn_kernel_v3.h): X(R, D / P, S, E / PA, P, skip-lane slots of the slot re-use form or 0)
#define WN_V3_SHAPES(X)                                                                                                                                  \
    X(128, 32, 512, 32, 4, 4) /* cfg3: P=4, PA=8 (a 64-row head slice is the slowest pipeline stage); + the slot re-use form (96 streams and more) */   \
    X(64, 64, 256, 64, 1, 0)  /* cfg2: P=1, PA=4 */                                                                                                      \
    X(32, 32, 256, 64, 1, 0)  /* cfg1: P=1, PA=4 */                                                                                                      \
    X(32, 16, 1024, 32, 2, 0) /* train_script.py chaconne shape, split two ways (64 skip weights per lane), PA=16 (end_conv_1 slice in LDS) */           \
    X(64, 32, 256, 64, 2, 0)  /* cfg2 split in two (layer_split=2) */                                                                                    \
    X(16, 16, 256, 32, 1, 0)  /* small test shape */                                                                                                     \
    X(16, 16, 256, 32, 2, 0)  /* ... and its two-slice form */
// The stacked kernel (wn_kernel_v4.h: LPW consecutive layers per 512-thread workgroup): X(R, D, S, E / PA, LPW).  LPW is what one CU's register file
// holds next to the working set: cfg2 60 registers per layer and lane (tap 0 lives in LDS), cfg1 32, the train_script.py shape 83 (its 1024 skip rows).
#define WN_V4_SHAPES(X)                                                                                                 \
    X(64, 64, 256, 64, 3)  /* cfg2 (BASELINE configs[1]): 10 stack workgroups */                                        \
    X(32, 32, 256, 64, 5)  /* cfg1 (configs[0]): 2 */                                                                   \
    X(32, 32, 1024, 32, 2) /* train_script.py:17-25, the reference's only trained model shape: 15 */

#if defined(__HIPCC__)
#include "wn_kernel_v4.h"

template <int R, int DC, int S, int EC, int PM, int SK>
static WnChainShape wn_v3_shape_facts(int index) {
    using SH = WnV2Shape<R, DC, S, EC>;
    static_assert(wn_v3_fits<SH, PM>(), "every listed shape runs the wave-specialised kernel");
    static_assert(SK == 0 || wn_v3_g2_fits<SH>(), "the slot re-use form is a two-streams-per-item form");
    WnChainShape e = {};
    e.kind = 3; e.index = index; e.R = R; e.DC = DC; e.S = S; e.EC = EC; e.Pm = PM;
    e.nwl = SH::NWL; e.lanes = 256; e.nwh = SH::NWH;
    e.has_g2 = wn_v3_g2_fits<SH>() ? 1 : 0; e.has_slots = SK > 0 ? 1 : 0;
    e.lds_pre[0] = e.lds_pre[1] = WnV3Lds<SH, 1>::pre;
    if constexpr (wn_v3_g2_fits<SH>()) e.lds_pre[1] = WnV3Lds<SH, 2>::pre;
    e.lds_stride = 256;                                                              // WnV3Lds::floats
    e.lds_head = WnV3Lds<SH, 1>::pre + (SH::K3 > 100 ? SH::K3 : EC) * 256;           // + the head lanes' LDS-resident weights (wn_v3_head)
    e.lds_smp = WnV3Lds<SH, 1>::pre + 256 * R;                                       // + start_conv^T in the sampler workgroups (wn_v3_sampler), when it fits
    return e;
}
template <int R, int D, int S, int EC, int LPW>
static WnChainShape wn_v4_shape_facts(int index) {
    using V = WnV4Shape<R, D, S>;
    using SH = WnV2Shape<R, D, S, EC>;   // (head and sampler workgroups are variant 3's)
    WnChainShape e = {};
    e.kind = 4; e.index = index; e.R = R; e.DC = D; e.S = S; e.EC = EC; e.Pm = LPW;
    e.nwl = V::NWPL; e.lanes = WN_THREADS_V4; e.nwh = SH::NWH;
    e.lds_pre[0] = e.lds_pre[1] = WnV4Lds<V, LPW>::pre;
    e.lds_stride = LPW * 2 * D;                                                      // WnV4Lds::floats
    e.lds_head = WnV3Lds<SH, 1>::pre + (SH::K3 > 100 ? SH::K3 : EC) * 256;
    e.lds_smp = WnV3Lds<SH, 1>::pre + 256 * R;
    return e;
}
// the facts of every listed shape: variant 3's rows, then variant 4's (`index`: the row within its kind)
static const std::vector<WnChainShape>& wn_chain_shapes() {
    static const std::vector<WnChainShape> t = [] {
        std::vector<WnChainShape> v;
        int i3 = 0, i4 = 0;
#define WN_X(R, DC, S, EC, PM, SK) v.push_back(wn_v3_shape_facts<R, DC, S, EC, PM, SK>(i3++));
        WN_V3_SHAPES(WN_X)
#undef WN_X
#define WN_X(R, D, S, EC, LPW) v.push_back(wn_v4_shape_facts<R, D, S, EC, LPW>(i4++));
        WN_V4_SHAPES(WN_X)
#undef WN_X
        return v;
    }();
    return t;
}
#endif  // __HIPCC__
#endif  // WN_CHAIN_SHAPES_H
