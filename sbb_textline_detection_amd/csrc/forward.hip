// forward.hip -- the forward pass over n patches whose input forms are filled: every plan op's launch (launch_op: a dispatch on route.h's
// route_of to one function per kernel family), the plan loop with its per-op accounting and profiling events (run_plan), and the profiling
// entry points that read them.
#include <stdlib.h>
#include <string.h>

#include "conv_choice.h"
#include "exec.h"
#include "route.h"

using namespace sbbseg;

namespace {

int get_event(sbbseg_ctx* c, hipEvent_t* e)
{
    if (!c->free_events.empty()) {
        *e = c->free_events.back();
        c->free_events.pop_back();
        return 0;
    }
    HIPCHK(hipEventCreate(e));
    return 0;
}

// ---- forward pass over n patches whose input forms are already filled -------------------------
// One function per kernel family (route.h): each fills its family's parameter struct and launches it.

int launch_block(sbbseg_ctx* c, Op& op, int n)
{
    const BlockOp& bo = op.block;
    BlockParams bp;
    bp.x = c->tensors[bo.x_tensor].buf; bp.n = n; bp.H = bo.H; bp.W = bo.W; bp.proj = bo.proj; bp.pq = c->block_pq ? 1 : 0;
    bp.w1 = bo.d_w1; bp.w2 = op.parts[1].conv.d_d64_wfrag; bp.w3 = bo.d_w3;
    bp.s1 = op.parts[0].conv.d_scale; bp.b1 = op.parts[0].conv.d_shift;
    bp.s2 = op.parts[1].conv.d_scale; bp.b2 = op.parts[1].conv.d_shift;
    bp.s3 = op.parts[2].conv.d_scale; bp.b3 = op.parts[2].conv.d_shift;
    bp.out = c->tensors[bo.out_tensor].data();
    bp.wmul1 = bo.wmul[0]; bp.wmul2 = bo.wmul[1]; bp.wmul3 = bo.wmul[2];
#ifdef SBBSEG_PROBES
    { static const int blk_dbg = getenv("SBBSEG_BLOCK_DBG") ? atoi(getenv("SBBSEG_BLOCK_DBG")) : 0; bp.dbg = blk_dbg; }
#endif
    if (c->precision == kF16X3) HIPCHK(launch_block_x3(bp, c->num_cus, c->stream, &op.last));
    else {
        if (c->dump_blocks) {         // the parts stay alive, so the plan tensors of a and b exist
            bp.dump_a = c->tensors[op.parts[0].conv.d.out_tensor].data();
            bp.dump_b = c->tensors[op.parts[1].conv.d.out_tensor].data();
        }
        HIPCHK(launch_bottleneck(bp, c->precision, c->num_cus, c->stream, &op.last));
    }
    return 0;
}

// the stem alone, or (with_pool) the stem and the max-pool behind it in one launch
int launch_stem_route(sbbseg_ctx* c, Op& op, int n, bool with_pool)
{
    const ConvOp& co = op.conv;
    const Tensor& st = c->tensors[co.d.src[0].tensor];
    StemParams sp;
    sp.pairs = st.buf; sp.PHt = st.H; sp.PWt = st.W; sp.n = n; sp.Ho = co.Ho; sp.Wo = co.Wo;
    sp.wfrag = co.d_stem_wfrag; sp.scale = co.d_scale; sp.shift = co.d_shift; sp.relu = co.d.relu; sp.wmul = co.wmul_cls[0];
    sp.out = c->tensors[co.d.out_tensor].data();
    if (!with_pool) {
        HIPCHK(launch_stem(sp, c->precision, c->num_cus, c->stream, &op.last));
        return 0;
    }
    const PoolOp& po = c->ops[co.fused_pool].pool;
    sp.pool_out = c->tensors[po.dst].data(); sp.pool_scale = po.d_pre_scale; sp.pool_shift = po.d_pre_shift;
    sp.pool_relu = po.pre_relu; sp.pool_Ho = po.Ho; sp.pool_Wo = po.Wo;
    sp.x3 = c->precision == kF16X3;
    HIPCHK(launch_stem_pool_x3(sp, c->num_cus, c->stream, &op.last));
    return 0;
}

int launch_direct64_route(sbbseg_ctx* c, Op& op, int n)
{
    const ConvOp& co = op.conv;
    const Tensor& st = c->tensors[co.d.src[0].tensor];
    Direct64Params dp;
    dp.src = st.buf; dp.n = n; dp.H = st.H; dp.W = st.W; dp.wfrag = co.d_d64_wfrag;
    dp.scale = co.d_scale; dp.shift = co.d_shift; dp.relu = co.d.relu; dp.out = c->tensors[co.d.out_tensor].data();
    dp.wmul = co.wmul_cls[0];
    HIPCHK(launch_direct64(dp, c->precision, c->num_cus, c->stream, &op.last));
    return 0;
}

// the expand conv's launch computes the block's 3x3 conv in front of it and the next block's reduce conv behind it too
int launch_c3er(sbbseg_ctx* c, Op& op, int n)
{
    const ConvOp& co = op.conv;
    const ConvOp& ro = c->ops[co.fused_reduce].conv;
    const ConvOp& k3 = c->ops[co.fused_conv3].conv;
    const Tensor& ta = c->tensors[k3.d.src[0].tensor];
    C3ERParams cp;
    cp.a = ta.buf; cp.x = c->tensors[co.d.residual_tensor].buf;
    cp.y = c->tensors[co.d.out_tensor].buf; cp.a2 = c->tensors[ro.d.out_tensor].buf;
    cp.n = n; cp.H = ta.H; cp.W = ta.W; cp.C = co.d.src[0].channels; cp.x3 = c->precision == kF16X3;
    cp.w2frag = co.d_c3_w2; cp.w3frag = co.d_er_w3; cp.w1frag = co.d_er_w1;
    cp.s2 = k3.d_scale; cp.h2 = k3.d_shift; cp.s3 = co.d_scale; cp.h3 = co.d_shift; cp.s1 = ro.d_scale; cp.h1 = ro.d_shift;
    cp.wmul2 = k3.wmul_cls[0]; cp.wmul3 = co.wmul_cls[0]; cp.wmul1 = ro.wmul_cls[0];
    cp.k0 = co.d_c3_k0;
    HIPCHK(launch_conv3_expand_reduce(cp, c->num_cus, c->stream, &op.last));
    return 0;
}

// the expand conv's launch writes the next block's reduce conv too
int launch_expand_reduce(sbbseg_ctx* c, Op& op, int n)
{
    const ConvOp& co = op.conv;
    const ConvOp& ro = c->ops[co.fused_reduce].conv;
    ExpRedParams ep;
    ep.b = c->tensors[co.d.src[0].tensor].buf; ep.x = c->tensors[co.d.residual_tensor].buf;
    ep.y = c->tensors[co.d.out_tensor].buf; ep.a2 = c->tensors[ro.d.out_tensor].buf;
    ep.M = n * co.Ho * co.Wo; ep.C = co.d.src[0].channels; ep.x3 = c->precision == kF16X3;
    ep.w3frag = co.d_er_w3; ep.w1frag = co.d_er_w1;
    ep.s3 = co.d_scale; ep.h3 = co.d_shift; ep.s1 = ro.d_scale; ep.h1 = ro.d_shift;
    ep.wmul3 = co.wmul_cls[0]; ep.wmul1 = ro.wmul_cls[0];
    ep.dbg = 0;
#ifdef SBBSEG_PROBES
    { static const int er_dbg = getenv("SBBSEG_ER_DBG") ? atoi(getenv("SBBSEG_ER_DBG")) : 0; ep.dbg = er_dbg; }
#endif
    HIPCHK(launch_expand_reduce_x3(ep, c->num_cus, c->stream, &op.last));
    return 0;
}

int launch_dec_halo(sbbseg_ctx* c, Op& op, int n)
{
    const ConvOp& co = op.conv;
    const Tensor& s0 = c->tensors[co.d.src[0].tensor];
    DecHaloParams hp;
    hp.src0 = s0.buf; hp.skip = c->tensors[co.d.src[1].tensor].buf; hp.PH = s0.H; hp.PW = s0.W; hp.n = n;
    hp.wfrag = co.d_halo_wfrag; hp.taps = co.d_halo_taps; hp.scale = co.d_scale; hp.shift = co.d_shift;
    for (int q = 0; q < 4; ++q) hp.wmul[q] = co.wmul_cls[q];
    hp.relu = co.d.relu; hp.out = c->tensors[co.d.out_tensor].data();
    // owned-region launch (region.h): the chunk's tile table -- region_plan_levels asked route_of too, so the level's table is of that kind
    if (c->rr.on && op.region_level >= 0) { hp.ttab = c->rr.tab[op.region_level]; hp.n_tab = c->rr.total[op.region_level]; }
    if (c->precision == kF16X3) HIPCHK(launch_dec_halo_x3(hp, c->num_cus, c->stream, &op.last));
    else HIPCHK(launch_dec_halo_f16(hp, c->num_cus, c->stream, &op.last));
    return 0;
}

// conv_igemm_mfma.  The form of the launch -- tile, gather, tile walk, owned-region table, split-K -- is choose_conv's (conv_choice.h); here
// ConvParams is filled from the op and that form.
int launch_generic_conv(sbbseg_ctx* c, Op& op, int n, uint8_t* d_labels, float* d_probs)
{
    const ConvOp& co = op.conv;
    const int region_entries = conv_region_entries(c, op);
    const ConvForm form = choose_conv(c, co, n, region_entries, conv_env());
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.n_src = co.d.n_src;
    for (int s = 0; s < co.d.n_src; ++s) {
        const Tensor& t = c->tensors[co.d.src[s].tensor];
        SrcDesc& sd = p.src[s];
        sd.base = t.buf;
        sd.PH = t.H; sd.PW = t.W;
        sd.pix_bytes = conv_src_pix_bytes(c, t);
        sd.lo_off = c->planes == 2 ? split_group(t.C) * c->elem : 64;       // split mode: hi -> lo inside a channel group
        sd.shift = co.d.src[s].up_shift;
        sd.lim_y = t.H << sd.shift; sd.lim_x = t.W << sd.shift;
        sd.ksteps = co.ksteps[s];
        sd.sy_shift = co.d.src[s].stride_y == 2; sd.sx_shift = co.d.src[s].stride_x == 2;
        sd.bytes = (uint32_t)conv_src_bytes(c, t, n);
        sd.tap_lo_y = co.tap_lo[s][0]; sd.tap_lo_x = co.tap_lo[s][1];
    }
    p.fast_gather = form.fast_gather;
    p.ktab = co.d_ktab; p.kstep = co.d_kstep; p.half_stages = (c->conv_variant & 16) ? 1 : 0;
    p.variant = c->conv_variant & 3; p.persist_blocks = (c->conv_variant & 4) ? 0 : c->num_cus;
    p.M = n * co.Ho * co.Wo;
    p.variant_flags = form.variant_flags;
#ifdef SBBSEG_PROBES
    { static const int probe_local = getenv("SBBSEG_CONV_PROBE_LOCAL") ? atoi(getenv("SBBSEG_CONV_PROBE_LOCAL")) : 0; if (probe_local) p.variant_flags |= 32; }
    { static const int probe_whot = getenv("SBBSEG_CONV_PROBE_WHOT") ? atoi(getenv("SBBSEG_CONV_PROBE_WHOT")) : 0; if (probe_whot) p.variant_flags |= 64; }
#endif
    p.tile_map = form.tile_map; p.cls_minor = form.cls_minor;
    p.w = co.d_w; p.Ktot = co.Ktot; p.total_ksteps = co.total_ksteps;
    p.Ho = co.Ho; p.Wo = co.Wo;
    p.TH = co.TH; p.TW = co.TW; p.osy = co.d.out_stride_y; p.osx = co.d.out_stride_x;
    p.ooy = co.d.out_off_y; p.oox = co.d.out_off_x;
    p.n_cls = co.n_cls;
    for (int q = 0; q < 4; ++q) {
        p.w_cls[q] = co.d_w_cls[q]; p.kstep_cls[q] = co.d_kstep_cls[q]; p.ktab_cls[q] = co.d_ktab_cls[q]; p.fgstep_cls[q] = co.d_fgstep_cls[q];
        p.ooy_cls[q] = co.ooy_cls[q]; p.oox_cls[q] = co.oox_cls[q]; p.wmul_cls[q] = co.wmul_cls[q];
    }
    p.head_classes = co.d.head_classes; p.head_w = co.d_head_w; p.head_scale = co.d_head_scale;
    p.head_shift = co.d_head_shift; p.labels = d_labels; p.probs = d_probs;
    p.cout = co.d.cout; p.scale = co.d_scale; p.shift = co.d_shift;
    p.out = co.d.out_tensor >= 0 ? c->tensors[co.d.out_tensor].data() : nullptr;
    p.residual = co.d.residual_tensor >= 0 ? c->tensors[co.d.residual_tensor].data() : nullptr;
    p.raw_out = co.d.raw_out_tensor >= 0 ? c->tensors[co.d.raw_out_tensor].data() : nullptr;
    p.raw_scale = co.d_rscale; p.raw_shift = co.d_rshift; p.relu = co.d.relu;
    // owned-region launch of a decoder level (region.h): the chunk's table replaces the walk over the whole output grid; a level whose table
    // is withheld runs whole and counts as whole
    if (form.table) { p.rmap = c->rr.tab[op.region_level]; p.M = region_entries; }
    else if (region_entries >= 0) c->last_exec_frac = 1.0;
    if (form.ks_shift > 0) {
        const size_t split_elems = (size_t)n * p.TH * p.TW * p.cout;
        if (ensure(c, c->ks_ws, (split_elems << form.ks_shift) * sizeof(float))) return 1;
        p.ks_shift = form.ks_shift; p.ks_ws = c->ks_ws.p; p.ks_split_elems = (long)split_elems;
    }
    HIPCHK(launch_conv(p, form, c->precision, c->stream, &op.last));
    if (form.ks_shift > 0)
        HIPCHK(launch_splitk_finish(c->ks_ws.p, 1 << form.ks_shift, p.ks_split_elems, (long)n * p.TH * p.TW, p.cout, p.scale, p.shift, p.residual,
                                    p.relu, p.out, c->precision, c->stream));
    return 0;
}

int launch_pool(sbbseg_ctx* c, Op& op, int n)
{
    const PoolOp& po = op.pool;
    const Tensor& s = c->tensors[po.src];
    HIPCHK(launch_maxpool(s.data(), c->tensors[po.dst].data(), n, s.H, s.W, s.C, po.k, po.stride, po.Ho, po.Wo,
                          po.d_pre_scale, po.d_pre_shift, po.pre_relu, c->precision, c->stream, &op.last));
    return 0;
}

int launch_tail_route(sbbseg_ctx* c, Op& op, int n, uint8_t* d_labels, float* d_probs)
{
    const TailOp& to = op.tail;
    const Tensor& s0 = c->tensors[to.src0];
    TailParams tp;
    tp.src0 = s0.buf; tp.img = c->tensors[to.img].buf; tp.PH = s0.H; tp.PW = s0.W; tp.n = n;
    tp.wfrag = to.d_wfrag; tp.scale = to.d_scale; tp.shift = to.d_shift; tp.classes = to.classes;
    tp.head_w = to.d_head_w; tp.head_scale = to.d_head_scale; tp.head_shift = to.d_head_shift;
    tp.labels = d_labels; tp.probs = d_probs;
    if (c->rr.on && op.region_level >= 0) { tp.ttab = c->rr.tab[op.region_level]; tp.n_tab = c->rr.total[op.region_level]; }
    HIPCHK(launch_tail(tp, c->precision, c->num_cus, c->stream, &op.last));
    return 0;
}

int launch_head_route(sbbseg_ctx* c, Op& op, int n, uint8_t* d_labels, float* d_probs)
{
    const HeadOp& ho = op.head;
    const Tensor& s = c->tensors[ho.src];
    HeadParams hp;
    hp.src = s.data(); hp.cin = ho.cin; hp.classes = ho.classes; hp.M = n * s.H * s.W;
    hp.w = ho.d_w; hp.scale = ho.d_scale; hp.shift = ho.d_shift;
    hp.labels = d_labels; hp.probs = d_probs;
    HIPCHK(launch_head(hp, c->precision, c->stream, &op.last));
    return 0;
}

int launch_op(sbbseg_ctx* c, Op& op, int n, uint8_t* d_labels, float* d_probs)
{
    op.last = LaunchRec{};            // (sbbseg_debug_op_launch: an op that returns below without a launch reports family NONE)
    // an owned-region level (a decoder conv or the tail) none of whose pixels any patch of the chunk keeps
    if (c->rr.on && op.region_level >= 0 && c->rr.total[op.region_level] == 0) return 0;
    switch (route_of(c, op)) {
    case kRouteNone: return 0;        // written by its absorber's launch
    case kRouteBlockFused: return launch_block(c, op, n);
    case kRouteBlockParts:
        for (auto& part : op.parts)
            if (launch_op(c, part, n, d_labels, d_probs)) return 1;
        op.last = op.parts.back().last;
        return 0;
    case kRouteStem: return launch_stem_route(c, op, n, false);
    case kRouteStemPool: return launch_stem_route(c, op, n, true);
    case kRouteDirect64: return launch_direct64_route(c, op, n);
    case kRouteC3ER: return launch_c3er(c, op, n);
    case kRouteExpandReduce: return launch_expand_reduce(c, op, n);
    case kRouteDecHalo: return launch_dec_halo(c, op, n);
    case kRouteConv: return launch_generic_conv(c, op, n, d_labels, d_probs);
    case kRoutePool: return launch_pool(c, op, n);
    case kRouteTail: return launch_tail_route(c, op, n, d_labels, d_probs);
    case kRouteHead: return launch_head_route(c, op, n, d_labels, d_probs);
    }
    return 0;
}

}  // namespace

namespace sbbseg {

int resolve_pending(sbbseg_ctx* c)
{
    if (c->pending.empty()) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto& pe : c->pending) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, pe.a, pe.b));
        Op& op = c->ops[pe.op];
        op.prof_ms += ms;
        op.prof_launches += 1;
        op.prof_patches += pe.patches;
        op.prof_exec_patches += pe.exec;
        c->free_events.push_back(pe.a);
        c->free_events.push_back(pe.b);
    }
    c->pending.clear();
    return 0;
}

int run_plan(sbbseg_ctx* c, int n, uint8_t* d_labels, float* d_probs)
{
    c->forwards += n;
    for (size_t i = 0; i < c->ops.size(); ++i) {
        Op& op = c->ops[i];
        hipEvent_t ea = nullptr, eb = nullptr;
        if (c->profiling) {
            if (get_event(c, &ea) || get_event(c, &eb)) return 1;
            HIPCHK(hipEventRecord(ea, c->stream));
        }
        c->last_exec_frac = (c->rr.on && op.region_level >= 0) ? c->rr.frac[op.region_level] : 1.0;
        if (launch_op(c, op, n, d_labels, d_probs)) return 1;
        const double exec = n * c->last_exec_frac;
        op.exec_patches += exec;
        if (c->profiling) {
            HIPCHK(hipEventRecord(eb, c->stream));
            c->pending.push_back({(int)i, ea, eb, n, exec});
        }
    }
    return 0;
}

int fill_ingest(sbbseg_ctx* c, IngestParams& ip)
{
    memset(&ip, 0, sizeof(ip));
    REQUIRE(c->form_tensor[SBBSEG_INPUT_C8] >= 0, "plan has no C8 input form");
    const Tensor& c8 = c->tensors[c->form_tensor[SBBSEG_INPUT_C8]];
    ip.H = c->in_H; ip.W = c->in_W; ip.lut = c->d_lut; ip.c8 = c8.data();
    if (c->form_tensor[SBBSEG_INPUT_PAIRS] >= 0) {
        const Tensor& pr = c->tensors[c->form_tensor[SBBSEG_INPUT_PAIRS]];
        ip.pairs = pr.data(); ip.pad = pr.pad; ip.pairs_w = pr.W;
    }
    return 0;
}

}  // namespace sbbseg

extern "C" {

// ------------------------------------------------------------------------------------- profiling
int sbbseg_profile_enable(sbbseg_ctx* c, int enable)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (resolve_pending(c)) return 1;
    c->profiling = enable != 0;
    return 0;
    API_END
}

int sbbseg_profile_reset(sbbseg_ctx* c)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (resolve_pending(c)) return 1;
    for (auto& op : c->ops) { op.prof_ms = 0; op.prof_launches = 0; op.prof_patches = 0; op.exec_patches = 0; op.prof_exec_patches = 0; }
    return 0;
    API_END
}

int sbbseg_op_executed(sbbseg_ctx* c, int op, double* exec_patches, double* timed_exec_patches)
{
    API_BEGIN
    REQUIRE(c && op >= 0 && op < (int)c->ops.size(), "op index out of range");
    if (resolve_pending(c)) return 1;
    if (exec_patches) *exec_patches = c->ops[op].exec_patches;
    if (timed_exec_patches) *timed_exec_patches = c->ops[op].prof_exec_patches;
    return 0;
    API_END
}

int sbbseg_profile_get(sbbseg_ctx* c, int op, double* total_ms, int64_t* launches, int64_t* patches)
{
    API_BEGIN
    REQUIRE(c && op >= 0 && op < (int)c->ops.size(), "op index out of range");
    if (resolve_pending(c)) return 1;
    if (total_ms) *total_ms = c->ops[op].prof_ms;
    if (launches) *launches = c->ops[op].prof_launches;
    if (patches) *patches = c->ops[op].prof_patches;
    return 0;
    API_END
}

}  // extern "C"
