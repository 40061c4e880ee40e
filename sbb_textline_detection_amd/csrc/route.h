// route.h -- private, host only, no HIP call, on top of ctx.h: which kernel family runs a plan op.  THE one statement of the rule: launch_op
// (forward.hip) dispatches on it, region_plan_levels (pages.hip) builds the kind of owned-region table the routed kernel takes, and
// tests/test_route_cpu.py holds it to a restatement of the rule over every combination of the knobs, on the CPU.
#pragma once

#include "ctx.h"

namespace sbbseg {

// One value per kernel family.  The precision pair of a family (launch_block_x3 / launch_bottleneck, launch_dec_halo_x3 / _f16, the x3 field
// of stem_pool and the 1x1 pairs) is the family's launch function's business, and so is what depends on the call instead of the plan: split-K,
// the owned-region table, tile map and class-minor walk of the generic conv.
enum Route {
    kRouteNone = 0,         // launches nothing: another op's launch writes this op's output (Op::absorbed_by)
    kRouteBlockFused,       // bottleneck_fused* / block_x3
    kRouteBlockParts,       // ... as the three convs it replaces, each by its own route
    kRouteStem,             // stem_conv_pairs
    kRouteStemPool,         // stem_pool_x3: the max-pool behind the stem too
    kRouteDirect64,         // conv3x3_c64_direct
    kRouteC3ER,             // conv3_expand_reduce: the 3x3 conv in front of the pair too
    kRouteExpandReduce,     // expand_reduce_x3: the next block's reduce conv too
    kRouteDecHalo,          // dec_halo_x3 / dec_halo_f16
    kRouteConv,             // conv_igemm_mfma (generic; split-K or not)
    kRoutePool,             // maxpool_kernel
    kRouteTail,
    kRouteHead,
};

// A pure function of the op's plan facts (type, d_stem_wfrag, d_d64_wfrag, d_halo_wfrag, fused_*, absorbed_by) and the handle's A/B knobs
// (sbbseg_debug_set_conv_variant).
inline Route route_of(const sbbseg_ctx* c, const Op& op)
{
    // an absorbed op never restates its absorber's condition: it launches nothing exactly when the absorber takes the route that writes it
    // (an absorber is never absorbed itself: sbbseg_finalize's passes skip such ops)
    if (op.absorbed_by >= 0) {
        const Op& by = c->ops[op.absorbed_by];
        const Route r = route_of(c, by);
        const bool is_conv3 = op.type == kConv && by.conv.fused_conv3 >= 0 && &c->ops[by.conv.fused_conv3] == &op;
        const bool written = op.type == kPool ? r == kRouteStemPool            // the stem's pool
                             : is_conv3       ? r == kRouteC3ER                // the 3x3 conv in front of an expand conv
                                              : r == kRouteC3ER || r == kRouteExpandReduce;      // the reduce conv behind it
        if (written) return kRouteNone;
    }
    switch (op.type) {
    // (deliberately no look at the tile-family variants: they are knobs of the plan's convs, and a fused block is none -- bit 18 takes it
    // apart, and the variants then reach its parts)
    case kBlock: return c->unfuse_blocks ? kRouteBlockParts : kRouteBlockFused;
    case kPool: return kRoutePool;
    case kTail: return kRouteTail;
    case kHead: return kRouteHead;
    case kConv: break;
    }
    const ConvOp& co = op.conv;
    if (c->conv_variant & 3) return kRouteConv;         // tile-family variants 1-3 of conv_igemm_mfma: every conv runs there
    if (co.d_stem_wfrag) return co.fused_pool >= 0 && !c->unfuse_stem_pool ? kRouteStemPool : kRouteStem;
    if (co.d_d64_wfrag) return kRouteDirect64;
    if (co.fused_reduce >= 0 && !c->no_expand_reduce) return co.fused_conv3 >= 0 && !c->no_c3er ? kRouteC3ER : kRouteExpandReduce;
    if (co.d_halo_wfrag && !c->no_dec_halo) return kRouteDecHalo;
    return kRouteConv;
}

}  // namespace sbbseg
