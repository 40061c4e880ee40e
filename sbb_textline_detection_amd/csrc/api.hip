// api.hip -- host side of libsbbseg: the C ABI declared in include/sbbseg.h, less plan building (plan_build.hip) and the stage glue
// (stage_glue.hip; all three sit on ctx.h).
//
// Holds the execution plan the Python planner builds (tensors + fused ops), owns all device
// memory, and drives the per-page pipeline
//   ingest (u8 -> LUT -> bf16 tiles)  ->  fused conv plan  ->  head (softmax/argmax)  ->  stitch
// that replaces the reference's per-patch Python loop (main.py:225-380).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>

#include <dlfcn.h>

#include "ctx.h"

using namespace sbbseg;

namespace sbbseg {

thread_local std::string g_err;
thread_local int g_err_kind = kErrOther;
int g_alloc_fail_countdown = 0;

int set_error(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    g_err_kind = kErrOther;
    return 1;
}

int dmalloc(sbbseg_ctx* c, void** p, size_t bytes)
{
    HIPCHK(hipMalloc(p, bytes));
    c->device_bytes += bytes;
    return 0;
}

int ensure(sbbseg_ctx* c, void** p, size_t* cap, size_t bytes)
{
    if (*cap >= bytes) return 0;
    if (*p) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(*p));
        c->device_bytes -= *cap;
        *p = nullptr; *cap = 0;
    }
    if (dmalloc(c, p, bytes)) return 1;
    *cap = bytes;
    return 0;
}

int check_ready(sbbseg_ctx* c)
{
    REQUIRE(c != nullptr, "null handle");
    REQUIRE(c->finalized, "plan not finalized");
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

}  // namespace sbbseg

namespace {

int margin_of(int W) { return (int)(0.1 * (double)W); }   // main.py:233  int(0.1 * img_width_model)

// per-axis tiles exactly as main.py:246-281: count = ceil(extent/mid); origin t*mid clamped inward
int axis_tiles(int extent, int tile, int margin, std::vector<int>& origin)
{
    const int mid = tile - 2 * margin;
    if (mid <= 0 || extent < tile) return -1;
    const int n = (extent + mid - 1) / mid;
    origin.resize(n);
    for (int t = 0; t < n; ++t) {
        int d = t * mid;
        if (d + tile > extent) d = extent - tile;
        origin[t] = d;
    }
    return n;
}

// owner table of one axis (closed form of the crop + overwrite order, main.py:294-364)
void axis_owner(int extent, int tile, int margin, const std::vector<int>& origin, std::vector<int>& own)
{
    own.assign(extent, 0);
    const int n = (int)origin.size();
    for (int t = 0; t < n; ++t) {
        const int lo = origin[t] + (t == 0 ? 0 : margin);
        const int hi = origin[t] + (t == n - 1 ? tile : tile - margin);
        for (int q = lo; q < hi; ++q) own[q] = (t << 16) | (q - origin[t]);
    }
}

// cv2.resize(..., INTER_NEAREST) index rule [EXT OpenCV resizeNN]: min(floor(dst * (1/(dst_len/src_len))), src_len-1)
void nearest_map(int src_len, int dst_len, std::vector<int>& m)
{
    m.resize(dst_len);
    const double inv = 1.0 / ((double)dst_len / (double)src_len);
    for (int i = 0; i < dst_len; ++i) {
        int s = (int)std::floor(i * inv);
        m[i] = s < src_len - 1 ? s : src_len - 1;
    }
}

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

// the 224 x 224 decoder conv takes the LDS-resident-halo kernel (dec_halo_x3 / dec_halo_f16) -- also decides which table an
// owned-region chunk builds for that level (tile origins vs class-grid pixels)
bool runs_dec_halo(const sbbseg_ctx* c, const ConvOp& co) { return co.d_halo_wfrag && !c->no_dec_halo && !(c->conv_variant & 3); }

// ---- forward pass over n patches whose input forms are already filled -------------------------
int launch_op(sbbseg_ctx* c, Op& op, int n, uint8_t* d_labels, float* d_probs)
{
        op.last = LaunchRec{};            // (sbbseg_debug_op_launch: an op that returns below without a launch reports family NONE)
        if (op.type == kBlock) {
            if (c->unfuse_blocks) {
                for (auto& part : op.parts)
                    if (launch_op(c, part, n, d_labels, d_probs)) return 1;
                op.last = op.parts.back().last;
                return 0;
            }
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
            else HIPCHK(launch_bottleneck(bp, c->precision, c->num_cus, c->stream, &op.last));
        } else if (op.type == kConv) {
            const ConvOp& co = op.conv;
            if (co.fused_into_expand && !c->no_expand_reduce && !(c->conv_variant & 3)) return 0;      // written by the expand conv's launch (expand_reduce_x3)
            if (co.fused_into_c3 && !c->no_c3er && !c->no_expand_reduce && !(c->conv_variant & 3)) return 0;     // computed by the expand conv's launch (conv3_expand_reduce)
            ConvParams p;
            p.ks_shift = 0; p.ks_ws = nullptr; p.ks_split_elems = 0;
            memset(&p, 0, sizeof(p));
            p.n_src = co.d.n_src;
            // (short-K layers keep the plain gather: the per-tile mask set-up costs them 1-10 %; from ~9 K-steps on the fast
            // gather wins 2-10 %, profiles/r02_experiments.md)
            bool fg = co.d_fgstep_cls[0] && !c->plain_gather;
            for (int s = 0; s < co.d.n_src; ++s) {
                const Tensor& t = c->tensors[co.d.src[s].tensor];
                SrcDesc& sd = p.src[s];
                sd.base = t.buf;
                sd.PH = t.H; sd.PW = t.W;
                sd.pix_bytes = t.C * c->elem * c->planes;
                sd.lo_off = c->planes == 2 ? split_group(t.C) * c->elem : 64;       // split mode: hi -> lo inside a channel group
                sd.shift = co.d.src[s].up_shift;
                sd.lim_y = t.H << sd.shift; sd.lim_x = t.W << sd.shift;
                sd.ksteps = co.ksteps[s];
                sd.sy_shift = co.d.src[s].stride_y == 2; sd.sx_shift = co.d.src[s].stride_x == 2;
                const size_t bytes = kZeroHeaderBytes + t.elems_per_patch * (size_t)n * c->elem * c->planes;
                sd.bytes = (uint32_t)bytes;
                // fast gather: bit 31 of a lane offset marks an out-of-bounds tap, so every real offset must stay below 2^31
                sd.tap_lo_y = co.tap_lo[s][0]; sd.tap_lo_x = co.tap_lo[s][1];
                if (bytes + (size_t)kFgBiasPixels(t.W) * sd.pix_bytes >= ((size_t)1 << 31)) fg = false;
            }
            p.fast_gather = fg ? (co.fg_pointwise ? 2 : 1) : 0;
            p.ktab = co.d_ktab; p.kstep = co.d_kstep; p.half_stages = (c->conv_variant & 16) ? 1 : 0;
            p.variant = c->conv_variant & 3; p.persist_blocks = (c->conv_variant & 4) ? 0 : c->num_cus;
            p.M = n * co.Ho * co.Wo;
            p.variant_flags = ((c->conv_variant & 64) ? 1 : 0) | ((c->conv_variant & 128) ? 2 : 0) | (c->ph8 ? 4 : 0);
#ifdef SBBSEG_PROBES
            { static const int probe_local = getenv("SBBSEG_CONV_PROBE_LOCAL") ? atoi(getenv("SBBSEG_CONV_PROBE_LOCAL")) : 0; if (probe_local) p.variant_flags |= 32; }
            { static const int probe_whot = getenv("SBBSEG_CONV_PROBE_WHOT") ? atoi(getenv("SBBSEG_CONV_PROBE_WHOT")) : 0; if (probe_whot) p.variant_flags |= 64; }
#endif
            // XCD-grouped walk for single-class layers: measured neutral-to-slower (it removes the n_ct-fold
            // re-fetch of the pixel operand, but those layers are not bound by fetch bytes) -> opt-in, bit 5
            // (split mode: on by default -- twice the pixel bytes; +0.7 % page throughput in two runs, profiles/r03_experiments.md)
            // (SBBSEG_PSHARE_MAX_MB: weight-matrix size up to which the pixel-sharing walk is taken; round 6 experiment -- the K >= 768 merge / reduce
            //  convs of stages 4 / 5 and dec0 re-fetch their pixel operand once per channel tile under map 0: PMC FETCH = n_ct x the input)
            static const size_t pshare_max = (size_t)(getenv("SBBSEG_PSHARE_MAX_MB") ? atoi(getenv("SBBSEG_PSHARE_MAX_MB")) : 2) << 20;
            p.tile_map = (((c->conv_variant & 32) || c->precision == kF16X3) && !(c->conv_variant & 8) && (c->conv_variant & 4) == 0 && co.d.cout > conv_tile_bc(co.d.cout) && p.M >= 256 * 128 &&
                          (size_t)co.cout_pad * co.Ktot * c->elem <= pshare_max) ? 1 : 0;
            if (p.tile_map == 1 && co.n_cls == 1 && co.Ktot <= c->contig_max_k) p.tile_map = 2;
            p.w = co.d_w; p.Ktot = co.Ktot; p.total_ksteps = co.total_ksteps;
            p.Ho = co.Ho; p.Wo = co.Wo; p.M = n * co.Ho * co.Wo;
            p.TH = co.TH; p.TW = co.TW; p.osy = co.d.out_stride_y; p.osx = co.d.out_stride_x;
            p.ooy = co.d.out_off_y; p.oox = co.d.out_off_x;
            p.n_cls = co.n_cls;
            p.cls_minor = 0;
            if (co.n_cls > 1 && (co.n_cls & (co.n_cls - 1)) == 0 && !(c->conv_variant & 8) && !(c->conv_variant & 4) &&
                (size_t)co.cout_pad * co.Ktot * c->elem <= ((size_t)16 << 20)) {     // (dec1/dec2 too: fetch -30 / -53 %, time unchanged)
                p.cls_minor = 1;      // small weights: let the classes share their source pixels in one L2
                p.tile_map = c->ranged_walk ? 3 : 1;
            }
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
            // owned-region launch of a decoder level (region.h): the chunk's table replaces the walk over the whole output grid
            const int rlv = c->rr.on ? op.region_level : -1;
            if (rlv >= 0 && c->rr.total[rlv] == 0) return 0;                         // (no patch of the chunk keeps anything)
            if (rlv >= 0 && c->rr.kind[rlv] == 1) {
                // the pixel table is read by the fast-gather form of conv_igemm_mfma, 2-stage whole-K-step tiles only (what every decoder conv
                // runs by default); under an A/B knob that takes the level elsewhere it is launched whole -- a superset, same results
                if (p.fast_gather && !p.half_stages && p.variant != 2 && !(p.variant_flags & 4)) { p.rmap = c->rr.tab[rlv]; p.M = c->rr.total[rlv]; }
                else c->last_exec_frac = 1.0;
            }
            if (co.d_stem_wfrag && !(c->conv_variant & 3)) {
                const Tensor& st = c->tensors[co.d.src[0].tensor];
                StemParams sp;
                sp.pairs = st.buf; sp.PHt = st.H; sp.PWt = st.W; sp.n = n; sp.Ho = co.Ho; sp.Wo = co.Wo;
                sp.wfrag = co.d_stem_wfrag; sp.scale = co.d_scale; sp.shift = co.d_shift; sp.relu = co.d.relu; sp.wmul = co.wmul_cls[0];
                sp.out = c->tensors[co.d.out_tensor].data();
                if (co.fused_pool >= 0 && !c->unfuse_stem_pool) {
                    const PoolOp& po = c->ops[co.fused_pool].pool;
                    sp.pool_out = c->tensors[po.dst].data(); sp.pool_scale = po.d_pre_scale; sp.pool_shift = po.d_pre_shift;
                    sp.pool_relu = po.pre_relu; sp.pool_Ho = po.Ho; sp.pool_Wo = po.Wo;
                    sp.x3 = c->precision == kF16X3;
                    HIPCHK(launch_stem_pool_x3(sp, c->num_cus, c->stream, &op.last));
                } else
                    HIPCHK(launch_stem(sp, c->precision, c->num_cus, c->stream, &op.last));
            } else if (co.d_d64_wfrag && !(c->conv_variant & 3)) {
                const Tensor& st = c->tensors[co.d.src[0].tensor];
                Direct64Params dp;
                dp.src = st.buf; dp.n = n; dp.H = st.H; dp.W = st.W; dp.wfrag = co.d_d64_wfrag;
                dp.scale = co.d_scale; dp.shift = co.d_shift; dp.relu = co.d.relu; dp.out = c->tensors[co.d.out_tensor].data();
                dp.wmul = co.wmul_cls[0];
                HIPCHK(launch_direct64(dp, c->precision, c->num_cus, c->stream, &op.last));
            } else if (co.fused_reduce >= 0 && !c->no_expand_reduce && !(c->conv_variant & 3)) {
                const ConvOp& ro = c->ops[co.fused_reduce].conv;
                if (co.fused_conv3 >= 0 && !c->no_c3er) {
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
            } else if (runs_dec_halo(c, co)) {
                const Tensor& s0 = c->tensors[co.d.src[0].tensor];
                DecHaloParams hp;
                hp.src0 = s0.buf; hp.skip = c->tensors[co.d.src[1].tensor].buf; hp.PH = s0.H; hp.PW = s0.W; hp.n = n;
                hp.wfrag = co.d_halo_wfrag; hp.taps = co.d_halo_taps; hp.scale = co.d_scale; hp.shift = co.d_shift;
                for (int q = 0; q < 4; ++q) hp.wmul[q] = co.wmul_cls[q];
                hp.relu = co.d.relu; hp.out = c->tensors[co.d.out_tensor].data();
                if (rlv >= 0) { hp.ttab = c->rr.tab[rlv]; hp.n_tab = c->rr.total[rlv]; }
                if (c->precision == kF16X3) HIPCHK(launch_dec_halo_x3(hp, c->num_cus, c->stream, &op.last));
                else HIPCHK(launch_dec_halo_f16(hp, c->num_cus, c->stream, &op.last));
            } else {
                // One patch through a long-K conv = 2-32 tiles of 100-400 K-steps at ~1 us a step on as many CUs: the whole-image branch
                // (extract_page's border model, 1 forward per page) splits the K range over the idle CUs -- up to 16 blocks per tile, each
                // at least 4 K-steps, fp32 partial sums added in split order by splitk_finish.  Only there: a split launch differs from
                // the unsplit one in the last bits, and seam 2 / the patch paths promise batch-size-independent results.
                int ks = 0;
                if (c->ksplit_now && n == 1 && c->precision != kF32 && p.fast_gather && conv_tile_bc(p.cout) == 128 && !p.raw_out && !p.head_classes &&
                    p.out && p.cout % 8 == 0 &&
                    ((p.n_cls == 1 && p.osy == 1 && p.osx == 1 && p.ooy == 0 && p.oox == 0 && p.TH == p.Ho && p.TW == p.Wo) ||
                     (p.n_cls == 4 && p.osy == 2 && p.osx == 2 && p.TH == 2 * p.Ho && p.TW == 2 * p.Wo))) {
                    const long tiles = (long)p.n_cls * ((p.M + 127) / 128) * ((p.cout + 127) / 128);
                    while (ks < 4 && (tiles << (ks + 1)) <= 512 && p.total_ksteps % (2 << ks) == 0 && (p.total_ksteps >> (ks + 1)) >= 4) ++ks;
                }
                if (ks > 0) {
                    const size_t split_elems = (size_t)n * p.TH * p.TW * p.cout;
                    if (ensure(c, (void**)&c->d_ks_ws, &c->ks_ws_cap, (split_elems << ks) * sizeof(float))) return 1;
                    p.ks_shift = ks; p.ks_ws = c->d_ks_ws; p.ks_split_elems = (long)split_elems; p.tile_map = 0; p.cls_minor = 0;
                    HIPCHK(launch_conv(p, c->precision, c->stream, &op.last));
                    HIPCHK(launch_splitk_finish(c->d_ks_ws, 1 << ks, (long)split_elems, (long)n * p.TH * p.TW, p.cout, p.scale, p.shift, p.residual,
                                                p.relu, p.out, c->precision, c->stream));
                } else {
                    HIPCHK(launch_conv(p, c->precision, c->stream, &op.last));
                }
            }
        } else if (op.type == kPool) {
            const PoolOp& po = op.pool;
            // written by the stem's launch (stem_pool_x3) -- under exactly the condition that sends the stem there (launch_op, kConv)
            if (po.fused_into_stem && !c->unfuse_stem_pool && !(c->conv_variant & 3)) return 0;
            const Tensor& s = c->tensors[po.src];
            HIPCHK(launch_maxpool(s.data(), c->tensors[po.dst].data(), n, s.H, s.W, s.C, po.k, po.stride, po.Ho, po.Wo,
                                  po.d_pre_scale, po.d_pre_shift, po.pre_relu, c->precision, c->stream, &op.last));
        } else if (op.type == kTail) {
            const TailOp& to = op.tail;
            const Tensor& s0 = c->tensors[to.src0];
            TailParams tp;
            tp.src0 = s0.buf; tp.img = c->tensors[to.img].buf; tp.PH = s0.H; tp.PW = s0.W; tp.n = n;
            tp.wfrag = to.d_wfrag; tp.scale = to.d_scale; tp.shift = to.d_shift; tp.classes = to.classes;
            tp.head_w = to.d_head_w; tp.head_scale = to.d_head_scale; tp.head_shift = to.d_head_shift;
            tp.labels = d_labels; tp.probs = d_probs;
            if (c->rr.on && op.region_level >= 0) {
                if (c->rr.total[op.region_level] == 0) return 0;
                tp.ttab = c->rr.tab[op.region_level]; tp.n_tab = c->rr.total[op.region_level];
            }
            HIPCHK(launch_tail(tp, c->precision, c->num_cus, c->stream, &op.last));
        } else {
            const HeadOp& ho = op.head;
            const Tensor& s = c->tensors[ho.src];
            HeadParams hp;
            hp.src = s.data(); hp.cin = ho.cin; hp.classes = ho.classes; hp.M = n * s.H * s.W;
            hp.w = ho.d_w; hp.scale = ho.d_scale; hp.shift = ho.d_shift;
            hp.labels = d_labels; hp.probs = d_probs;
            HIPCHK(launch_head(hp, c->precision, c->stream, &op.last));
        }
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

// activation buffers and stream of lane L become the ones run_plan / fill_ingest see
struct LaneScope {
    sbbseg_ctx* c; hipStream_t saved;
    LaneScope(sbbseg_ctx* c_, int lane) : c(c_), saved(c_->stream)
    {
        if (lane == 1) {
            for (auto& t : c->tensors) t.buf = t.lane_buf[1];
            c->stream = c->lane_stream;
        }
    }
    ~LaneScope()
    {
        for (auto& t : c->tensors) t.buf = t.lane_buf[0];
        c->stream = saved;
    }
};

// A pooled list of n_tiles tiles, cut into launches: run_chunk(lane, first, nb) queues tiles [first, first + nb) on lane `lane`.
template <typename F>
int run_chunked(sbbseg_ctx* c, int n_tiles, F&& run_chunk)
{
    // chunks of equal size (108 tiles at max_batch 70 -> 54 + 54, not 70 + 38): launches shrink evenly.
    // (Profiling runs every launch alone on one lane: its chunks are capped at the size a LANE's launch has in normal operation -- half a
    // chunk -- so that the per-op times describe the launches the product runs, partial last rounds of the persistent grids included.)
    const int chunk_cap = (c->profiling && c->lanes == 2 && c->lane1_batch > 0 && c->max_batch >= 4 * kMinLaneTiles) ? (c->max_batch + 1) / 2 : c->max_batch;
    const int n_chunks = (n_tiles + chunk_cap - 1) / chunk_cap;
    const int chunk = n_chunks ? (n_tiles + n_chunks - 1) / n_chunks : 0;
    bool forked = false;
    for (int done = 0; done < n_tiles; done += chunk) {
        const int nb = n_tiles - done < chunk ? n_tiles - done : chunk;
        const bool two = c->lane1_batch > 0 && c->lanes == 2 && !c->profiling && nb >= 2 * kMinLaneTiles;
        if (!two) {
            if (forked) {                                       // (a one-lane chunk behind two-lane ones: lane 1 first)
                HIPCHK(hipEventRecord(c->ev_join, c->lane_stream));
                HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
                forked = false;
            }
            if (run_chunk(0, done, nb)) return 1;               // (not forked here: a fork in front was joined above)
            continue;
        }
        const int na = (nb + 1) / 2, nb2 = nb - na;            // nb2 <= lane1_batch
        // The lanes fork ONCE per tile range and join once behind its last chunk (round 5): a lane's halves of consecutive chunks follow each
        // other on the lane's own stream and buffers, nothing of one lane depends on the other.  (Up to round 4 every chunk forked and joined:
        // the lane that finished its half first waited for the other one -- 7-10 % of the timed region had ONE kernel in flight,
        // profiles/r05_timeline_gaps.txt.)
        if (!forked) {
            HIPCHK(hipEventRecord(c->ev_fork, c->stream));     // page / threshold / earlier ranges are ordered before
            HIPCHK(hipStreamWaitEvent(c->lane_stream, c->ev_fork, 0));
            forked = true;
        }
        // (a failure from here on must still join the lanes: earlier chunks of this range are in flight on lane_stream, unordered against
        //  whatever the caller does next on the handle's stream -- stitch, reuse of d_tile_labels, destroy)
        auto join_on_error = [&]() -> int {
            if (hipEventRecord(c->ev_join, c->lane_stream) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_join, 0) != hipSuccess)
                (void)hipStreamSynchronize(c->lane_stream);
            (void)hipGetLastError();
            return 1;
        };
        if (run_chunk(0, done, na)) return join_on_error();
        if (run_chunk(1, done + na, nb2)) return join_on_error();           // (starting lane 1 later -- after lane 0's op k -- measured 3-14 % slower)
    }
    if (forked) {
        HIPCHK(hipEventRecord(c->ev_join, c->lane_stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
    return 0;
}

// device label plane [pix] -> host buffer, as one plane or as the reference's three identical channels
int labels_to_host(sbbseg_ctx* c, void* host, size_t pix)
{
    if (c->label_channels == 3) {
        if (ensure(c, (void**)&c->d_page_labels3, &c->page_labels3_cap, (pix + 3) / 4 * 12)) return 1;
        HIPCHK(launch_replicate3(c->d_page_labels, c->d_page_labels3, pix, c->stream));
        HIPCHK(hipMemcpyAsync(host, c->d_page_labels3, pix * 3, hipMemcpyDeviceToHost, c->stream));
    } else {
        HIPCHK(hipMemcpyAsync(host, c->d_page_labels, pix, hipMemcpyDeviceToHost, c->stream));
    }
    return 0;
}

// ---- RCCL, loaded at run time: libsbbseg has no link-time dependency on librccl (it must load on a box without it, and
// on the CPU-only build container); the sharded path's one collective is the all-gather of u8 label maps
struct RcclUniqueId { char internal[128]; };                  // = ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES 128)
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(RcclUniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclUniqueId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mutex;                                      // (handles on distinct devices may be driven from distinct threads)
int rccl_load()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.lib) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    REQUIRE(h, "librccl not found (tried librccl.so.1, librccl.so, /opt/rocm/lib/librccl.so.1): %s", dlerror());
    RcclApi a;
    a.GetUniqueId = (int (*)(RcclUniqueId*))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void**, int, RcclUniqueId, int))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    a.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    a.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllGather || !a.GetErrorString) {
        dlclose(h);
        return set_error("librccl lacks an expected symbol (ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather)");
    }
    a.lib = h;
    g_rccl = a;
    return 0;
}
#define RCCLCHK(expr)                                                                              \
    do {                                                                                           \
        const int r_ = (expr);                                                                     \
        if (r_ != 0) return set_error("%s failed: %s", #expr, g_rccl.GetErrorString(r_));          \
    } while (0)

void comm_release(sbbseg_ctx* c)
{
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    c->comm = nullptr; c->comm_rank = 0; c->comm_world = 1;
}

}  // namespace

// =================================================================================================
extern "C" {

const char* sbbseg_last_error(void) { return g_err.c_str(); }
int sbbseg_abi_version(void) { return SBBSEG_ABI_VERSION; }

int sbbseg_device_count(int* count)
{
    API_BEGIN
    REQUIRE(count, "null count");
    HIPCHK(hipGetDeviceCount(count));
    return 0;
    API_END
}

int sbbseg_create(int device, int precision, sbbseg_ctx** out)
{
    API_BEGIN
    REQUIRE(out, "null out");
    REQUIRE(precision == SBBSEG_PREC_BF16 || precision == SBBSEG_PREC_F32 || precision == SBBSEG_PREC_F16 || precision == SBBSEG_PREC_F16X3,
            "bad precision %d", precision);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    REQUIRE(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
            "libsbbseg is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
    sbbseg_ctx* c = new sbbseg_ctx();
    c->device = device;
    c->precision = precision;
    c->elem = precision == SBBSEG_PREC_F32 ? 4 : 2;
    c->planes = is_split(precision) ? 2 : 1;
    c->num_cus = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    // The second lane's stream is created in ANOTHER PRIORITY CLASS than the handle's own stream.  HIP multiplexes streams onto a few
    // hardware queues per priority class (GPU_MAX_HW_QUEUES, default 4, dealt round robin): when a handle's two streams land on the
    // same queue its lanes serialise behind each other's barrier packets -- measured 26.4 ms instead of 22.9 ms per 108-tile page on the
    // SECOND handle of a process (the fourth with 8 queues, none of five with 16: tools/handle_order_probe.py, profiles/r04_experiments.md
    // section 10); configs[2]'s layout stage was that handle.  Queues of different priority classes are never shared.
    // SBBSEG_LANE_PRIORITY: -1 (default) = the device's highest priority, 0 = same class as the own stream (the old behaviour), 1 = lowest
    {
        int least = 0, greatest = 0, want = -1;
        if (const char* v = getenv("SBBSEG_LANE_PRIORITY")) want = atoi(v);
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        const int prio = want < 0 ? greatest : want > 0 ? least : 0;
        e = prio != 0 ? hipStreamCreateWithPriority(&c->lane_stream, hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(&c->lane_stream, hipStreamNonBlocking);
        c->lane_prio = prio; c->prio_least = least; c->prio_greatest = greatest;
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) {
        sbbseg_destroy(c);
        return set_error("lane stream/event creation failed: %s", hipGetErrorString(e));
    }
    if (const char* v = getenv("SBBSEG_DEDUPE")) c->dedupe = v[0] != '0';
    if (const char* v = getenv("SBBSEG_KSPLIT")) c->ksplit = v[0] != '0';
    if (const char* v = getenv("SBBSEG_OWNED_REGIONS")) c->owned_mode = v[0] == '0' ? 0 : (v[0] == '2' ? 2 : 1);
    *out = c;
    return 0;
    API_END
}

int sbbseg_destroy(sbbseg_ctx* c)
{
    API_BEGIN
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->lane_stream) (void)hipStreamSynchronize(c->lane_stream);
    for (auto& t : c->tensors) {
        (void)hipFree(t.lane_buf[0]);
        (void)hipFree(t.lane_buf[1]);
    }
    std::vector<Op*> all_ops;
    for (auto& op : c->ops) {
        all_ops.push_back(&op);
        for (auto& part : op.parts) all_ops.push_back(&part);
    }
    for (Op* opp : all_ops) {
        Op& op = *opp;
        (void)hipFree(op.block.d_w1); (void)hipFree(op.block.d_w3);
        for (int q = 0; q < 4; ++q) (void)hipFree(op.conv.d_fgstep_cls[q]);
        (void)hipFree(op.conv.d_ktab); (void)hipFree(op.conv.d_kstep); (void)hipFree(op.conv.d_w); (void)hipFree(op.conv.d_scale); (void)hipFree(op.conv.d_shift);
        (void)hipFree(op.conv.d_rscale); (void)hipFree(op.conv.d_rshift);
        (void)hipFree(op.conv.d_head_w); (void)hipFree(op.conv.d_head_scale); (void)hipFree(op.conv.d_head_shift); (void)hipFree(op.conv.d_stem_wfrag); (void)hipFree(op.conv.d_d64_wfrag);
        (void)hipFree(op.conv.d_halo_wfrag); (void)hipFree(op.conv.d_halo_taps);
        (void)hipFree(op.conv.d_er_w3); (void)hipFree(op.conv.d_er_w1);
        (void)hipFree(op.conv.d_c3_w2); (void)hipFree(op.conv.d_c3_k0);
        for (int q = 1; q < 4; ++q) { (void)hipFree(op.conv.d_w_cls[q]); (void)hipFree(op.conv.d_kstep_cls[q]); (void)hipFree(op.conv.d_ktab_cls[q]); }
        (void)hipFree(op.head.d_w); (void)hipFree(op.head.d_scale); (void)hipFree(op.head.d_shift);
        (void)hipFree(op.pool.d_pre_scale); (void)hipFree(op.pool.d_pre_shift);
        (void)hipFree(op.tail.d_wfrag); (void)hipFree(op.tail.d_scale); (void)hipFree(op.tail.d_shift); (void)hipFree(op.tail.d_head_w);
        (void)hipFree(op.tail.d_head_scale); (void)hipFree(op.tail.d_head_shift);
    }
    (void)hipFree(c->d_lut); (void)hipFree(c->d_hist); (void)hipFree(c->d_tile_xy); (void)hipFree(c->d_batch_labels); (void)hipFree(c->d_probs); (void)hipFree(c->d_xin); (void)hipFree(c->d_ks_ws);
    (void)hipFree(c->d_page); (void)hipFree(c->d_page_labels); (void)hipFree(c->d_page_labels3); (void)hipFree(c->d_tile_labels);
    (void)hipFree(c->d_own_x); (void)hipFree(c->d_own_y); (void)hipFree(c->d_map); (void)hipFree(c->d_wmap);
    (void)hipFree(c->d_views); (void)hipHostFree(c->h_views);
    if (c->ev_views) (void)hipEventDestroy(c->ev_views);
    (void)hipFree(c->d_deskew);
    (void)hipFree(c->d_cc_bg); (void)hipFree(c->d_cc_roots); (void)hipFree(c->d_rdk); (void)hipFree(c->d_pstat); (void)hipFree(c->d_line_tab);
    (void)hipFree(c->d_lsplit); (void)hipFree(c->d_line_w);
    for (int lane = 0; lane < 2; ++lane)
        for (int L = 0; L < kRegionMaxLevels; ++L) (void)hipFree(c->d_rtab[lane][L]);
    (void)hipFree(c->d_run_page); (void)hipFree(c->d_run_mask); (void)hipFree(c->d_run_a); (void)hipFree(c->d_run_b);
    for (auto& ub : c->user_bufs) (void)hipFree(ub.first);
    for (int k = 0; k < 2; ++k) {
        (void)hipHostFree(c->pp_h_in[k]); (void)hipHostFree(c->pp_h_out[k]);
        (void)hipFree(c->pp_d_in[k]); (void)hipFree(c->pp_d_out[k]); (void)hipFree(c->pp_d_out3[k]);
        if (c->pp_in[k]) (void)hipEventDestroy(c->pp_in[k]);
        if (c->pp_comp[k]) (void)hipEventDestroy(c->pp_comp[k]);
        if (c->pp_out[k]) (void)hipEventDestroy(c->pp_out[k]);
    }
    comm_release(c);
    if (c->copy_in) (void)hipStreamDestroy(c->copy_in);
    if (c->copy_out) (void)hipStreamDestroy(c->copy_out);
    (void)hipFree(c->d_morph_a); (void)hipFree(c->d_morph_b); (void)hipFree(c->d_cc_parent); (void)hipFree(c->d_cc_count); (void)hipFree(c->d_cc_aux); (void)hipFree(c->d_cc_list); (void)hipFree(c->d_cc_small);
    for (auto& pe : c->pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto e : c->free_events) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->lane_stream) (void)hipStreamDestroy(c->lane_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    delete c;
    return 0;
    API_END
}

int sbbseg_set_stream(sbbseg_ctx* c, void* hip_stream)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (resolve_pending(c)) return 1;
    // NULL is a real stream (the legacy default stream torch uses unless told otherwise)
    c->stream = hip_stream == SBBSEG_OWN_STREAM ? c->own_stream : (hipStream_t)hip_stream;
    // a caller's stream of the lane stream's own priority class could share its hardware queue (see sbbseg_create): move the lane
    // stream to the other end of the range
    int up = 0;
    if (hip_stream != SBBSEG_OWN_STREAM && hip_stream && c->lane_prio != 0 && c->prio_least != c->prio_greatest &&
        hipStreamGetPriority((hipStream_t)hip_stream, &up) == hipSuccess && up == c->lane_prio) {
        const int other = c->lane_prio == c->prio_greatest ? c->prio_least : c->prio_greatest;
        hipStream_t ns = nullptr;
        if (other != 0 && hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, other) == hipSuccess) {
            HIPCHK(hipStreamSynchronize(c->lane_stream));
            HIPCHK(hipStreamDestroy(c->lane_stream));
            c->lane_stream = ns;
            c->lane_prio = other;
        } else (void)hipGetLastError();
    }
    return 0;
    API_END
}

int sbbseg_set_lanes(sbbseg_ctx* c, int lanes)
{
    API_BEGIN
    REQUIRE(c && (lanes == 1 || lanes == 2), "lanes must be 1 or 2");
    REQUIRE(!(c->finalized && lanes == 2 && c->lane1_batch == 0), "the second lane was not allocated at finalize (lanes was 1 or max_batch < 16)");
    c->lanes = lanes;
    return 0;
    API_END
}

int sbbseg_set_label_channels(sbbseg_ctx* c, int channels)
{
    API_BEGIN
    REQUIRE(c && (channels == 1 || channels == 3), "label channels must be 1 or 3");
    c->label_channels = channels;
    return 0;
    API_END
}

int sbbseg_set_dedupe(sbbseg_ctx* c, int on)
{
    API_BEGIN
    REQUIRE(c && (on == 0 || on == 1), "dedupe must be 0 or 1");
    c->dedupe = on != 0;
    return 0;
    API_END
}

int sbbseg_set_owned_regions(sbbseg_ctx* c, int mode)
{
    API_BEGIN
    REQUIRE(c && mode >= 0 && mode <= 2, "mode: 0 = off, 1 = fused page paths, 2 = tile-range entry points too");
    c->owned_mode = mode;
    return 0;
    API_END
}

int sbbseg_owned_region_info(sbbseg_ctx* c, int* mode, int* levels)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (mode) *mode = c->owned_mode;
    if (levels) *levels = c->finalized ? c->region_levels : 0;
    return 0;
    API_END
}

int sbbseg_debug_owned_range(int extent, int tile, int margin, int n_tiles, int t, int* lo, int* hi)
{
    API_BEGIN
    REQUIRE(lo && hi && tile > 2 * margin && margin >= 0 && extent >= tile && n_tiles >= 1 && t >= 0 && t < n_tiles, "bad arguments");
    const RegionAxis a = {extent, tile, margin, tile - 2 * margin, n_tiles};
    region_own(a, t, *lo, *hi);
    return 0;
    API_END
}

int sbbseg_debug_region_rows(int extent, int tile, int margin, int n_tiles, int t, int levels, const int32_t* level_size, int32_t* lo_hi)
{
    API_BEGIN
    REQUIRE(lo_hi && level_size && levels >= 1 && levels <= kRegionMaxLevels && tile > 2 * margin && margin >= 0 && extent >= tile && n_tiles >= 1 &&
            t >= 0 && t < n_tiles, "bad arguments");
    const RegionAxis a = {extent, tile, margin, tile - 2 * margin, n_tiles};
    int lo, hi;
    region_own(a, t, lo, hi);
    lo_hi[0] = lo; lo_hi[1] = hi;
    for (int k = 1; k < levels; ++k) {
        region_down(lo, hi, level_size[k]);
        lo_hi[2 * k] = lo; lo_hi[2 * k + 1] = hi;
    }
    return 0;
    API_END
}

int sbbseg_debug_poison_activations(sbbseg_ctx* c, int byte_value)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    HIPCHK(hipDeviceSynchronize());
    for (auto& t : c->tensors) {
        if (t.is_input_form) continue;                     // (their zero borders are part of the form)
        for (int lane = 0; lane < 2; ++lane) {
            if (!t.lane_buf[lane]) continue;
            const size_t n = t.elems_per_patch * (size_t)(lane == 0 ? c->max_batch : c->lane1_batch) * c->elem * c->planes;
            HIPCHK(hipMemset(t.lane_buf[lane] + kZeroHeaderBytes, byte_value & 255, n));
        }
    }
    if (c->d_tile_labels) HIPCHK(hipMemset(c->d_tile_labels, byte_value & 255, c->tile_labels_cap));
    // the split-K partial sums too: a split that a later pass does not write must not find the last pass's (equal) value there
    if (c->d_ks_ws) HIPCHK(hipMemset(c->d_ks_ws, byte_value & 255, c->ks_ws_cap));
    HIPCHK(hipDeviceSynchronize());
    return 0;
    API_END
}

int sbbseg_set_ksplit(sbbseg_ctx* c, int on)
{
    API_BEGIN
    REQUIRE(c && (on == 0 || on == 1), "ksplit must be 0 or 1");
    c->ksplit = on != 0;
    return 0;
    API_END
}

int sbbseg_synchronize(sbbseg_ctx* c)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

// ----------------------------------------------------------------------------------------- queries
int sbbseg_model_info(sbbseg_ctx* c, int* H, int* W, int* classes, int* max_batch)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (H) *H = c->in_H;
    if (W) *W = c->in_W;
    if (classes) *classes = c->classes;
    if (max_batch) *max_batch = c->max_batch;
    return 0;
    API_END
}

int sbbseg_num_ops(sbbseg_ctx* c, int* n)
{
    API_BEGIN
    REQUIRE(c && n, "bad arguments");
    *n = (int)c->ops.size();
    return 0;
    API_END
}

int sbbseg_op_info(sbbseg_ctx* c, int op, char* name, int name_len, double* flops_per_patch, double* min_bytes_per_patch)
{
    API_BEGIN
    REQUIRE(c && op >= 0 && op < (int)c->ops.size(), "op index out of range");
    if (name && name_len > 0) snprintf(name, name_len, "%s", c->ops[op].name.c_str());
    if (flops_per_patch) *flops_per_patch = c->ops[op].flops;
    if (min_bytes_per_patch) *min_bytes_per_patch = c->ops[op].min_bytes;
    return 0;
    API_END
}

int sbbseg_op_issued_flops(sbbseg_ctx* c, int op, double* issued_flops_per_patch)
{
    API_BEGIN
    REQUIRE(c && op >= 0 && op < (int)c->ops.size() && issued_flops_per_patch, "op index out of range");
    *issued_flops_per_patch = c->ops[op].issued_flops;
    return 0;
    API_END
}

int sbbseg_device_bytes(sbbseg_ctx* c, size_t* bytes)
{
    API_BEGIN
    REQUIRE(c && bytes, "bad arguments");
    *bytes = c->device_bytes;
    return 0;
    API_END
}

// -------------------------------------------------------------------------------------- seam 2
int sbbseg_predict(sbbseg_ctx* c, const float* x_nhwc, int n, float* probs_nhwc)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(x_nhwc && probs_nhwc && n >= 0, "bad arguments");
    const size_t per_in = (size_t)c->in_H * c->in_W * 3, per_out = (size_t)c->in_H * c->in_W * c->classes;
    if (!c->d_xin && dmalloc(c, (void**)&c->d_xin, per_in * c->max_batch * sizeof(float))) return 1;
    if (!c->d_probs && dmalloc(c, (void**)&c->d_probs, per_out * c->max_batch * sizeof(float))) return 1;
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    for (int done = 0; done < n; done += c->max_batch) {
        const int nb = n - done < c->max_batch ? n - done : c->max_batch;
        HIPCHK(hipMemcpyAsync(c->d_xin, x_nhwc + done * per_in, per_in * nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_ingest_f32(c->d_xin, nb, c->in_H, c->in_W, ip.c8, ip.pairs, ip.pad, ip.pairs_w, c->precision, c->stream));
        if (run_plan(c, nb, c->d_batch_labels, c->d_probs)) return 1;
        HIPCHK(hipMemcpyAsync(probs_nhwc + done * per_out, c->d_probs, per_out * nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
    API_END
}

// -------------------------------------------------------------------------------------- seam 1
int sbbseg_tile_grid(int Hp, int Wp, int H, int W, int32_t* tile_xy, int capacity, int* nxf, int* nyf)
{
    API_BEGIN
    alloc_check();
    std::vector<int> ox, oy;
    const int margin = margin_of(W);
    const int nx = axis_tiles(Wp, W, margin, ox), ny = axis_tiles(Hp, H, margin, oy);
    REQUIRE_GEOMETRY(nx > 0 && ny > 0, "page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)", Hp, Wp, H, W);
    if (nxf) *nxf = nx;
    if (nyf) *nyf = ny;
    if (tile_xy) {
        REQUIRE(capacity >= nx * ny, "tile_xy capacity %d < %d tiles", capacity, nx * ny);
        for (int i = 0; i < nx; ++i)               // x outer, y inner: main.py:259-260
            for (int j = 0; j < ny; ++j) {
                tile_xy[2 * (i * ny + j)] = ox[i];
                tile_xy[2 * (i * ny + j) + 1] = oy[j];
            }
    }
    return 0;
    API_END
}

int sbbseg_nearest_map(int src_len, int dst_len, int32_t* map)
{
    API_BEGIN
    REQUIRE(src_len > 0 && dst_len > 0 && map, "bad arguments");
    alloc_check();
    std::vector<int> m;
    nearest_map(src_len, dst_len, m);
    for (int i = 0; i < dst_len; ++i) map[i] = m[i];
    return 0;
    API_END
}

int sbbseg_segment_tiles_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, const int32_t* tile_xy, int n_tiles,
                             void* d_tile_labels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && tile_xy && d_tile_labels && n_tiles >= 0, "bad arguments");
    for (int t = 0; t < n_tiles; ++t)
        REQUIRE(tile_xy[2 * t] >= 0 && tile_xy[2 * t] + c->in_W <= Wp && tile_xy[2 * t + 1] >= 0 && tile_xy[2 * t + 1] + c->in_H <= Hp,
                "tile %d at (%d,%d) leaves the %dx%d page", t, tile_xy[2 * t], tile_xy[2 * t + 1], Hp, Wp);
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = (const uint8_t*)d_page_hwc; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = Hp; ip.src_Wp = Wp; ip.tile_xy = c->d_tile_xy;
    const size_t per = (size_t)c->in_H * c->in_W;
    for (int done = 0; done < n_tiles; done += c->max_batch) {
        const int nb = n_tiles - done < c->max_batch ? n_tiles - done : c->max_batch;
        // explicit origin lists are the slow, general form: the table is re-used per chunk, so wait
        // for the previous chunk's ingest before overwriting it (the grid form below needs no table)
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(c->d_tile_xy, tile_xy + 2 * done, sizeof(int) * 2 * nb, hipMemcpyHostToDevice));
        ip.n_tiles = nb;
        HIPCHK(launch_ingest_u8(ip, c->precision, c->stream));
        if (run_plan(c, nb, (uint8_t*)d_tile_labels + done * per, nullptr)) return 1;
    }
    return 0;
    API_END
}

// Tile grid of the FUSED page paths: the reference's grid (sbbseg_tile_grid) minus the repeated last tile of an axis whose last two
// origins coincide (at most the last two can: three equal origins would need 2 * mid < tile - mid).  Origins are still
// min(t * mid, extent - tile) for t < n', so the ingest kernel's closed form holds on the smaller grid; the dropped tile's pixels
// [origin + margin, origin + tile) are exactly what tile n' - 1 pastes as the new last tile (axis_owner with dedupe).
static int fused_grid(const sbbseg_ctx* c, int Hp, int Wp, bool dedupe, int* nx, int* ny)
{
    if (sbbseg_tile_grid(Hp, Wp, c->in_H, c->in_W, nullptr, 0, nx, ny)) return 1;
    if (!dedupe) return 0;
    const int margin = margin_of(c->in_W);
    std::vector<int> o;
    if (axis_tiles(Wp, c->in_W, margin, o) >= 2 && o[o.size() - 1] == o[o.size() - 2]) --*nx;
    if (axis_tiles(Hp, c->in_H, margin, o) >= 2 && o[o.size() - 1] == o[o.size() - 2]) --*ny;
    return 0;
}

// ---- what the pooled tile paths share (tile_range_impl: pages of one size; sbbseg_segment_views_dev: views of any size) ----
// the plan's side of the owned-region geometry: levels, table kinds, output sizes (the page's side -- axes, grid -- is the caller's)
static void region_plan_levels(const sbbseg_ctx* c, RegionGeom& rg)
{
    rg.n_levels = c->region_levels;
    for (int L = 0; L < c->region_levels; ++L) {
        const Op& lop = c->ops[c->region_op[L]];
        if (L == 0) { rg.kind[L] = 0; rg.Rh[L] = c->in_H; rg.Rw[L] = c->in_W; rg.align_x[L] = 16; }
        else {
            const Tensor& to = c->tensors[lop.conv.d.out_tensor];
            rg.kind[L] = runs_dec_halo(c, lop.conv) ? 0 : 1;
            rg.Rh[L] = to.H; rg.Rw[L] = to.W; rg.align_x[L] = 2;
        }
    }
}

// level L's table of the chunk of nb patches lane `lane` is about to run: `total` entries as the host counted them -> c->rr; the lane's buffer
// holds the largest table a full batch can need
static int region_level_table(sbbseg_ctx* c, int lane, const RegionGeom& rg, int L, int nb, long total)
{
    const size_t batch_cap = (size_t)(lane == 0 ? c->max_batch : c->lane1_batch);
    const size_t need = 4 * (rg.kind[L] ? 4 * batch_cap * (size_t)(rg.Rh[L] / 2) * (size_t)(rg.Rw[L] / 2)
                                         : batch_cap * (size_t)(rg.Rh[L] / 16 + 1) * (size_t)(rg.Rw[L] / 16 + 1));
    if (c->rtab_cap[lane][L] < need) {
        HIPCHK(hipDeviceSynchronize());                  // (first use / a kind switched by an A/B knob: rare)
        if (c->d_rtab[lane][L]) { HIPCHK(hipFree(c->d_rtab[lane][L])); c->device_bytes -= c->rtab_cap[lane][L]; c->d_rtab[lane][L] = nullptr; c->rtab_cap[lane][L] = 0; }
        if (dmalloc(c, (void**)&c->d_rtab[lane][L], need)) return 1;
        c->rtab_cap[lane][L] = need;
    }
    RegionRun& rr = c->rr;
    rr.kind[L] = rg.kind[L]; rr.total[L] = (int)total; rr.tab[L] = c->d_rtab[lane][L];
    rr.frac[L] = (double)total * (rg.kind[L] ? 4.0 : 256.0) / ((double)nb * rg.Rh[L] * rg.Rw[L]);
    return 0;
}
struct RegionOff { sbbseg_ctx* c; ~RegionOff() { c->rr.on = false; } };

// Tiles [first_tile, first_tile + n_tiles) of the tile list of `n_pages` equally sized pages (page-major: tile g = page g / tpp,
// grid index g % tpp) -> d_tile_labels[g - first_tile].  Chunks of <= max_batch tiles may span pages: big launches fill the chip's
// persistent grids better than one page's 70 tiles (profiles/r02_experiments.md).
// `owned`: the decoder of every tile is launched over the region the page stitch keeps of it (+ the halo the levels above need) only
// (region.h) -- d_tile_labels is then defined on the owned regions, which is all stitch_impl reads.
static int tile_range_impl(sbbseg_ctx* c, const void* const* d_pages, int n_pages, int src_Hp, int src_Wp, const int* d_map_y, const int* d_map_x,
                           int Hp, int Wp, int first_tile, int n_tiles, void* d_tile_labels, const int* d_bin_thr = nullptr, bool dedupe = false,
                           bool owned = false)
{
    REQUIRE(d_pages && n_pages >= 1 && d_tile_labels && first_tile >= 0 && n_tiles >= 0, "bad arguments");
    for (int k = 0; k < n_pages; ++k) REQUIRE(d_pages[k], "null page pointer (page %d)", k);
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, dedupe, &nx, &ny)) return 1;
    const int tpp = nx * ny;
    REQUIRE((long)first_tile + n_tiles <= (long)tpp * n_pages, "tile range [%d,%d) exceeds the %d tiles of the %d page(s)", first_tile,
            first_tile + n_tiles, tpp * n_pages, n_pages);
    const int margin = margin_of(c->in_W);
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = (const uint8_t*)d_pages[0]; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = src_Hp; ip.src_Wp = src_Wp; ip.tile_xy = nullptr;
    ip.map_y = d_map_y; ip.map_x = d_map_x; ip.bin_thr = d_bin_thr;
    ip.grid_nyf = ny; ip.grid_mid_x = c->in_W - 2 * margin; ip.grid_mid_y = c->in_H - 2 * margin;
    const size_t per = (size_t)c->in_H * c->in_W;
    const size_t act = (size_t)c->elem * c->planes;          // bytes per stored element
    // owned-region launches: the page geometry in closed form; the tables of a chunk are built on its lane's stream in front of its forward
    const bool regions = owned && c->region_levels > 0 && c->max_batch <= kRegionMaxPatches;
    RegionGeom rg;
    memset(&rg, 0, sizeof(rg));
    if (regions) {
        rg.ax = {Wp, c->in_W, margin, c->in_W - 2 * margin, nx};
        rg.ay = {Hp, c->in_H, margin, c->in_H - 2 * margin, ny};
        rg.tpp = tpp; rg.ny = ny;
        region_plan_levels(c, rg);
    }
    auto setup_regions = [&](int lane, int g_first, int nb) -> int {       // (inside the lane's scope: c->stream is the lane's stream)
        RegionBuildParams bp;
        memset(&bp, 0, sizeof(bp));
        bp.g = rg; bp.g0 = g_first; bp.nb = nb;
        for (int L = 0; L < rg.n_levels; ++L) {
            long total = 0;
            for (int q = 0; q < nb; ++q) {
                const int local = (g_first + q) % tpp, i = local / ny, j = local - i * ny;
                total += region_entries(rg, i, j, L);
            }
            if (region_level_table(c, lane, rg, L, nb, total)) return 1;
            bp.out[L] = c->d_rtab[lane][L]; bp.total[L] = (int)total;
        }
        HIPCHK(launch_region_build(bp, c->stream));
        c->rr.on = true;
        return 0;
    };
    auto run_chunk = [&](int lane, int first, int nb) -> int {
        LaneScope scope(c, lane);
        RegionOff roff{c};
        if (regions && setup_regions(lane, first_tile + first, nb)) return 1;
        IngestParams lp = ip;
        if (fill_ingest(c, lp)) return 1;          // (input-form pointers of this lane)
        char* const c8_base = (char*)lp.c8;
        char* const pairs_base = (char*)lp.pairs;
        const size_t c8_tile = per * 8 * act, pairs_tile = lp.pairs ? (size_t)(c->in_H + 2 * lp.pad) * lp.pairs_w * 8 * act : 0;
        lp.Hp = ip.Hp; lp.Wp = ip.Wp; lp.src_Hp = ip.src_Hp; lp.src_Wp = ip.src_Wp; lp.tile_xy = nullptr;
        lp.map_y = ip.map_y; lp.map_x = ip.map_x; lp.bin_thr = ip.bin_thr;
        lp.grid_nyf = ip.grid_nyf; lp.grid_mid_x = ip.grid_mid_x; lp.grid_mid_y = ip.grid_mid_y;
        for (int done = 0; done < nb;) {            // one ingest launch per page the chunk touches
            const int g = first_tile + first + done, pg = g / tpp, local = g - pg * tpp;
            const int run = nb - done < tpp - local ? nb - done : tpp - local;
            lp.page = (const uint8_t*)d_pages[pg];
            lp.grid_first = local;
            lp.n_tiles = run;
            lp.c8 = c8_base + (size_t)done * c8_tile;
            lp.pairs = pairs_base ? pairs_base + (size_t)done * pairs_tile : nullptr;
            HIPCHK(launch_ingest_u8(lp, c->precision, c->stream));
            done += run;
        }
        return run_plan(c, nb, (uint8_t*)d_tile_labels + first * per, nullptr);
    };
    return run_chunked(c, n_tiles, run_chunk);
}

int sbbseg_segment_tile_range_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int first_tile, int n_tiles,
                                  void* d_tile_labels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return tile_range_impl(c, &d_page_hwc, 1, Hp, Wp, nullptr, nullptr, Hp, Wp, first_tile, n_tiles, d_tile_labels, nullptr, false, c->owned_mode >= 2);
    API_END
}

static int prepare_owner(sbbseg_ctx* c, int Hp, int Wp, bool dedupe)
{
    if (c->own_Hp == Hp && c->own_Wp == Wp && c->own_dedupe == dedupe) return 0;
    alloc_check();
    std::vector<int> ox, oy, own_x, own_y;
    const int margin = margin_of(c->in_W);
    int nx = axis_tiles(Wp, c->in_W, margin, ox), ny = axis_tiles(Hp, c->in_H, margin, oy);
    REQUIRE_GEOMETRY(nx > 0 && ny > 0, "page %dx%d is smaller than the model input", Hp, Wp);
    if (dedupe) {                              // (fused_grid: the repeated last tile of an axis is not computed)
        if (nx >= 2 && ox[nx - 1] == ox[nx - 2]) ox.resize(--nx);
        if (ny >= 2 && oy[ny - 1] == oy[ny - 2]) oy.resize(--ny);
    }
    axis_owner(Wp, c->in_W, margin, ox, own_x);
    axis_owner(Hp, c->in_H, margin, oy, own_y);
    const size_t need = sizeof(int) * (size_t)(Hp > Wp ? Hp : Wp);
    if (c->own_cap < need) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->d_own_x) { HIPCHK(hipFree(c->d_own_x)); HIPCHK(hipFree(c->d_own_y)); c->device_bytes -= 2 * c->own_cap; }
        c->d_own_x = c->d_own_y = nullptr;
        if (dmalloc(c, (void**)&c->d_own_x, need) || dmalloc(c, (void**)&c->d_own_y, need)) return 1;
        c->own_cap = need;
    }
    HIPCHK(hipStreamSynchronize(c->stream));   // tables may still be in use by an earlier stitch
    HIPCHK(hipMemcpy(c->d_own_x, own_x.data(), sizeof(int) * Wp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_own_y, own_y.data(), sizeof(int) * Hp, hipMemcpyHostToDevice));
    c->own_Hp = Hp; c->own_Wp = Wp; c->own_nyf = ny; c->own_dedupe = dedupe;
    return 0;
}

static int stitch_impl(sbbseg_ctx* c, const void* d_tile_labels, int Hp, int Wp, void* d_labels_hw, bool dedupe)
{
    REQUIRE(d_tile_labels && d_labels_hw, "bad arguments");
    if (prepare_owner(c, Hp, Wp, dedupe)) return 1;
    HIPCHK(launch_stitch((const uint8_t*)d_tile_labels, c->in_H, c->in_W, c->d_own_x, c->d_own_y, c->own_nyf, Hp, Wp,
                         (uint8_t*)d_labels_hw, c->stream));
    return 0;
}

int sbbseg_stitch_dev(sbbseg_ctx* c, const void* d_tile_labels, int Hp, int Wp, void* d_labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return stitch_impl(c, d_tile_labels, Hp, Wp, d_labels_hw, false);      // tile labels in the reference's call order
    API_END
}

int sbbseg_segment_page_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, void* d_labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, c->dedupe, &nx, &ny)) return 1;
    if (ensure(c, (void**)&c->d_tile_labels, &c->tile_labels_cap, (size_t)nx * ny * c->in_H * c->in_W)) return 1;
    if (tile_range_impl(c, &d_page_hwc, 1, Hp, Wp, nullptr, nullptr, Hp, Wp, 0, nx * ny, c->d_tile_labels, nullptr, c->dedupe, c->owned_mode >= 1)) return 1;
    return stitch_impl(c, c->d_tile_labels, Hp, Wp, d_labels_hw, c->dedupe);
    API_END
}

int sbbseg_segment_pages_dev(sbbseg_ctx* c, int n_pages, const void* const* d_pages_hwc, int Hp, int Wp, void* const* d_labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_pages >= 1 && d_pages_hwc && d_labels_hw, "bad arguments");
    for (int k = 0; k < n_pages; ++k) REQUIRE(d_pages_hwc[k] && d_labels_hw[k], "null page / label pointer (page %d)", k);
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, c->dedupe, &nx, &ny)) return 1;
    const size_t per = (size_t)c->in_H * c->in_W, tpp = (size_t)nx * ny;
    // Pages are pooled in GROUPS whose tile count is a whole number of chunks where that is possible with few pages
    // (lcm(tiles per page, max_batch)), else about eight chunks: the tile-label scratch stays bounded by the group, not
    // by the caller's page count (64 pages of 4000x3000 would otherwise hold 1.4 GB of tile labels at once), and no
    // chunk is cut short except the very last.  Groups run back to back on the handle's stream (stream order protects the
    // scratch buffer that every group reuses).
    size_t a = tpp, b = (size_t)c->max_batch;
    while (b) { const size_t t = a % b; a = b; b = t; }                 // a = gcd
    size_t G = (size_t)c->max_batch / a;                                 // pages per group with G * tpp = lcm
    if (G > 32) G = (8 * (size_t)c->max_batch + tpp - 1) / tpp;
    if (G < 1) G = 1;
    if (G > (size_t)n_pages) G = (size_t)n_pages;
    REQUIRE(tpp * G < (size_t)1 << 30, "page group of %zu tiles is too large", tpp * G);
    if (ensure(c, (void**)&c->d_tile_labels, &c->tile_labels_cap, tpp * G * per)) return 1;
    for (size_t g0 = 0; g0 < (size_t)n_pages; g0 += G) {
        const size_t np = g0 + G <= (size_t)n_pages ? G : (size_t)n_pages - g0;
        if (tile_range_impl(c, d_pages_hwc + g0, (int)np, Hp, Wp, nullptr, nullptr, Hp, Wp, 0, (int)(tpp * np), c->d_tile_labels, nullptr, c->dedupe, c->owned_mode >= 1)) return 1;
        for (size_t k = 0; k < np; ++k)
            if (stitch_impl(c, c->d_tile_labels + k * tpp * per, Hp, Wp, d_labels_hw[g0 + k], c->dedupe)) return 1;
    }
    return 0;
    API_END
}

// do_prediction(patches=True) for several HOST pages of one size, pipelined in groups of as many pages as fill a chunk:
// while group g runs on the handle's stream, the caller's thread stages group g+1 into pinned memory and starts its upload on
// a copy stream, and the label planes of group g-1 come back on another.  Results equal n_pages sbbseg_segment_page calls.
int sbbseg_segment_pages(sbbseg_ctx* c, int n_pages, const uint8_t* const* pages_hwc, int Hp, int Wp, uint8_t* const* labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_pages >= 1 && pages_hwc && labels_hw, "bad arguments");
    for (int k = 0; k < n_pages; ++k) REQUIRE(pages_hwc[k] && labels_hw[k], "null page / label pointer (page %d)", k);
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)", Hp, Wp, c->in_H, c->in_W);
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, c->dedupe, &nx, &ny)) return 1;
    const size_t pix = (size_t)Hp * Wp, in_b = pix * 3, ch = c->label_channels == 3 ? 3 : 1, out_b = pix * ch;
    const size_t out3_b = (pix + 3) / 4 * 12;                          // launch_replicate3 writes whole 12-byte groups
    int G = c->max_batch / (nx * ny);
    G = G < 1 ? 1 : (G > n_pages ? n_pages : G);
    if (!c->pp_ready) {                                                   // set LAST: a failed creation is retried by the next call
        if (!c->copy_in) HIPCHK(hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
        if (!c->copy_out) HIPCHK(hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            if (!c->pp_in[k]) HIPCHK(hipEventCreateWithFlags(&c->pp_in[k], hipEventDisableTiming));
            if (!c->pp_comp[k]) HIPCHK(hipEventCreateWithFlags(&c->pp_comp[k], hipEventDisableTiming));
            if (!c->pp_out[k]) HIPCHK(hipEventCreateWithFlags(&c->pp_out[k], hipEventDisableTiming));
        }
        c->pp_ready = true;
    }
    HIPCHK(hipStreamSynchronize(c->stream));                            // (buffers below may be re-allocated)
    // Every buffer has its own capacity in the units it was allocated in; a capacity is zeroed BEFORE its buffers are
    // freed and set only after all of them exist again, so a failed allocation leaves "nothing allocated", not a stale size.
    auto host_pair = [&](uint8_t* (&h)[2], size_t* cap, size_t bytes) -> int {
        if (*cap >= bytes) return 0;
        *cap = 0;
        for (int k = 0; k < 2; ++k) { (void)hipHostFree(h[k]); h[k] = nullptr; }
        for (int k = 0; k < 2; ++k) HIPCHK(hipHostMalloc((void**)&h[k], bytes, hipHostMallocDefault));
        *cap = bytes;
        return 0;
    };
    auto dev_pair = [&](uint8_t* (&d)[2], size_t* cap, size_t bytes) -> int {
        if (*cap >= bytes) return 0;
        const size_t old = *cap;
        *cap = 0;
        for (int k = 0; k < 2; ++k)
            if (d[k]) { (void)hipFree(d[k]); d[k] = nullptr; c->device_bytes -= old; }
        for (int k = 0; k < 2; ++k)
            if (dmalloc(c, (void**)&d[k], bytes)) return 1;
        *cap = bytes;
        return 0;
    };
    if (host_pair(c->pp_h_in, &c->pp_hin_cap, G * in_b)) return 1;
    if (dev_pair(c->pp_d_in, &c->pp_in_cap, G * in_b)) return 1;
    if (host_pair(c->pp_h_out, &c->pp_hout_cap, G * out_b)) return 1;
    if (dev_pair(c->pp_d_out, &c->pp_out_cap, G * (pix + 4))) return 1;   // one u8 plane (+4 bytes slack) per page, whatever label_channels is
    if (ch == 3 && dev_pair(c->pp_d_out3, &c->pp_out3_cap, G * out3_b)) return 1;
    const int n_groups = (n_pages + G - 1) / G;
    auto group_pages = [&](int g) { return g * G + G <= n_pages ? G : n_pages - g * G; };
    auto drain = [&](int g) -> int {                                      // labels of group g: staging -> caller
        const int slot = g & 1;
        HIPCHK(hipEventSynchronize(c->pp_out[slot]));
        for (int k = 0; k < group_pages(g); ++k) memcpy(labels_hw[g * G + k], c->pp_h_out[slot] + (size_t)k * out_b, out_b);
        return 0;
    };
    alloc_check();
    std::vector<const void*> d_pages(G);
    std::vector<void*> d_labels(G);
    for (int g = 0; g < n_groups; ++g) {
        const int slot = g & 1, np = group_pages(g);
        if (g >= 2 && drain(g - 2)) return 1;                             // frees this slot's staging and device buffers
        for (int k = 0; k < np; ++k) memcpy(c->pp_h_in[slot] + (size_t)k * in_b, pages_hwc[g * G + k], in_b);
        HIPCHK(hipMemcpyAsync(c->pp_d_in[slot], c->pp_h_in[slot], (size_t)np * in_b, hipMemcpyHostToDevice, c->copy_in));
        HIPCHK(hipEventRecord(c->pp_in[slot], c->copy_in));
        HIPCHK(hipStreamWaitEvent(c->stream, c->pp_in[slot], 0));
        for (int k = 0; k < np; ++k) {
            d_pages[k] = c->pp_d_in[slot] + (size_t)k * in_b;
            d_labels[k] = c->pp_d_out[slot] + (size_t)k * (pix + 4);
        }
        if (sbbseg_segment_pages_dev(c, np, d_pages.data(), Hp, Wp, d_labels.data())) return 1;
        const uint8_t* d_src = c->pp_d_out[slot];
        size_t d_stride = pix + 4;
        if (ch == 3) {
            for (int k = 0; k < np; ++k)
                HIPCHK(launch_replicate3(c->pp_d_out[slot] + (size_t)k * (pix + 4), c->pp_d_out3[slot] + (size_t)k * out3_b, pix, c->stream));
            d_src = c->pp_d_out3[slot];
            d_stride = out3_b;
        }
        HIPCHK(hipEventRecord(c->pp_comp[slot], c->stream));
        HIPCHK(hipStreamWaitEvent(c->copy_out, c->pp_comp[slot], 0));
        for (int k = 0; k < np; ++k)
            HIPCHK(hipMemcpyAsync(c->pp_h_out[slot] + (size_t)k * out_b, d_src + (size_t)k * d_stride, out_b, hipMemcpyDeviceToHost, c->copy_out));
        HIPCHK(hipEventRecord(c->pp_out[slot], c->copy_out));
    }
    for (int g = n_groups >= 2 ? n_groups - 2 : 0; g < n_groups; ++g)
        if (drain(g)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_segment_page(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, uint8_t* labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw, "bad arguments");
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)", Hp, Wp, c->in_H, c->in_W);
    const size_t pix = (size_t)Hp * Wp;
    if (ensure(c, (void**)&c->d_page, &c->page_cap, pix * 3)) return 1;
    if (ensure(c, (void**)&c->d_page_labels, &c->page_labels_cap, pix + 4)) return 1;
    HIPCHK(hipMemcpyAsync(c->d_page, page_hwc, pix * 3, hipMemcpyHostToDevice, c->stream));
    if (sbbseg_segment_page_dev(c, c->d_page, Hp, Wp, c->d_page_labels)) return 1;
    if (labels_to_host(c, labels_hw, pix)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_segment_page_scaled(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, uint8_t* labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw && Hs > 0 && Ws > 0, "bad arguments");
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "scaled page %dx%d is smaller than the model input %dx%d", Hp, Wp, c->in_H, c->in_W);
    const size_t spix = (size_t)Hs * Ws, pix = (size_t)Hp * Wp;
    if (ensure(c, (void**)&c->d_page, &c->page_cap, spix * 3)) return 1;
    if (ensure(c, (void**)&c->d_page_labels, &c->page_labels_cap, pix + 4)) return 1;
    std::vector<int> my, mx;
    nearest_map(Hs, Hp, my);               // scaled row -> stored row   (main.py:214 -> 112-113)
    nearest_map(Ws, Wp, mx);
    if (ensure(c, (void**)&c->d_map, &c->map_cap, sizeof(int) * (size_t)(Hp + Wp))) return 1;
    c->map_key[0] = 0;                     // (d_map is rewritten below: the crop path's cached maps are gone)
    int* d_my = c->d_map; int* d_mx = d_my + Hp;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(d_my, my.data(), sizeof(int) * Hp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_mx, mx.data(), sizeof(int) * Wp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpyAsync(c->d_page, page_hwc, spix * 3, hipMemcpyHostToDevice, c->stream));
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, c->dedupe, &nx, &ny)) return 1;
    if (ensure(c, (void**)&c->d_tile_labels, &c->tile_labels_cap, (size_t)nx * ny * c->in_H * c->in_W)) return 1;
    const void* pg_ = c->d_page;
    if (tile_range_impl(c, &pg_, 1, Hs, Ws, d_my, d_mx, Hp, Wp, 0, nx * ny, c->d_tile_labels, nullptr, c->dedupe, c->owned_mode >= 1)) return 1;
    if (stitch_impl(c, c->d_tile_labels, Hp, Wp, c->d_page_labels, c->dedupe)) return 1;
    if (labels_to_host(c, labels_hw, pix)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_otsu_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int* d_threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && d_threshold && Hp > 0 && Wp > 0, "bad arguments");
    HIPCHK(launch_otsu((const uint8_t*)d_page_hwc, Wp, Hp, Wp, nullptr, nullptr, c->d_hist, d_threshold, c->num_cus, c->stream));
    return 0;
    API_END
}

int sbbseg_segment_tile_range_bin_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int first_tile, int n_tiles,
                                      const int* d_threshold, void* d_tile_labels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_threshold, "bad arguments");
    return tile_range_impl(c, &d_page_hwc, 1, Hp, Wp, nullptr, nullptr, Hp, Wp, first_tile, n_tiles, d_tile_labels, d_threshold, false, c->owned_mode >= 2);
    API_END
}

int sbbseg_segment_page_otsu(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, uint8_t* labels_hw,
                             int* threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw && Hs > 0 && Ws > 0, "bad arguments");
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "page %dx%d is smaller than the model input %dx%d", Hp, Wp, c->in_H, c->in_W);
    const size_t spix = (size_t)Hs * Ws, pix = (size_t)Hp * Wp;
    const bool scaled = Hs != Hp || Ws != Wp;
    if (ensure(c, (void**)&c->d_page, &c->page_cap, spix * 3)) return 1;
    if (ensure(c, (void**)&c->d_page_labels, &c->page_labels_cap, pix + 4)) return 1;
    int *d_my = nullptr, *d_mx = nullptr;
    if (scaled) {
        std::vector<int> my, mx;
        nearest_map(Hs, Hp, my);           // scaled row -> stored row   (main.py:214 -> 112-113)
        nearest_map(Ws, Wp, mx);
        if (ensure(c, (void**)&c->d_map, &c->map_cap, sizeof(int) * (size_t)(Hp + Wp))) return 1;
        c->map_key[0] = 0;
        d_my = c->d_map; d_mx = d_my + Hp;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(d_my, my.data(), sizeof(int) * Hp, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_mx, mx.data(), sizeof(int) * Wp, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpyAsync(c->d_page, page_hwc, spix * 3, hipMemcpyHostToDevice, c->stream));
    int* d_thr = (int*)(c->d_hist + 256);
    HIPCHK(launch_otsu(c->d_page, Ws, Hp, Wp, d_my, d_mx, c->d_hist, d_thr, c->num_cus, c->stream));
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, c->dedupe, &nx, &ny)) return 1;
    if (ensure(c, (void**)&c->d_tile_labels, &c->tile_labels_cap, (size_t)nx * ny * c->in_H * c->in_W)) return 1;
    const void* pg_ = c->d_page;
    if (tile_range_impl(c, &pg_, 1, Hs, Ws, d_my, d_mx, Hp, Wp, 0, nx * ny, c->d_tile_labels, d_thr, c->dedupe, c->owned_mode >= 1)) return 1;
    if (stitch_impl(c, c->d_tile_labels, Hp, Wp, c->d_page_labels, c->dedupe)) return 1;
    if (labels_to_host(c, labels_hw, pix)) return 1;
    int thr = 0;
    HIPCHK(hipMemcpyAsync(&thr, d_thr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (threshold) *threshold = thr;
    return 0;
    API_END
}

// The patch stages of run() on the CROPPED page (main.py:2061-2102: extract_page's croped_page goes to extract_text_regions and
// textline_contours): the crop box lives in the coordinates of the page as upscaled to Hp x Wp, the stored image is Hs x Ws.
// Rescale, crop and (binarise != 0) otsu_copy are all index arithmetic in the tile gather: row r / column q of the crop read
// stored row map_y[cy + r] / column map_x[cx + q]; the Otsu histogram is taken over exactly those pixels (channel 0).
int sbbseg_segment_crop_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hs, int Ws, int Hp, int Wp, int cx, int cy, int cw, int ch,
                            int binarise, void* d_labels_hw, int* d_threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && d_labels_hw && Hs > 0 && Ws > 0 && Hp > 0 && Wp > 0, "bad arguments");
    REQUIRE(cx >= 0 && cy >= 0 && cw > 0 && ch > 0 && cx + cw <= Wp && cy + ch <= Hp, "crop box {%d,%d,%d,%d} leaves the %dx%d page", cx, cy, cw, ch, Hp, Wp);
    REQUIRE_GEOMETRY(ch >= c->in_H && cw >= c->in_W, "cropped page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)",
            ch, cw, c->in_H, c->in_W);
    if (c->map_key[0] != Hs || c->map_key[1] != Ws || c->map_key[2] != Hp || c->map_key[3] != Wp || !c->d_map) {
        std::vector<int> my, mx;
        nearest_map(Hs, Hp, my);           // scaled row -> stored row   (main.py:214 -> 112-113); identity when Hs == Hp
        nearest_map(Ws, Wp, mx);
        if (ensure(c, (void**)&c->d_map, &c->map_cap, sizeof(int) * (size_t)(Hp + Wp))) return 1;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(c->d_map, my.data(), sizeof(int) * Hp, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_map + Hp, mx.data(), sizeof(int) * Wp, hipMemcpyHostToDevice));
        c->map_key[0] = Hs; c->map_key[1] = Ws; c->map_key[2] = Hp; c->map_key[3] = Wp;
    }
    const int* d_my = c->d_map + cy;
    const int* d_mx = c->d_map + Hp + cx;
    int* d_thr = nullptr;
    if (binarise) {
        d_thr = d_threshold ? d_threshold : (int*)(c->d_hist + 256);
        HIPCHK(launch_otsu((const uint8_t*)d_page_hwc, Ws, ch, cw, d_my, d_mx, c->d_hist, d_thr, c->num_cus, c->stream));
    }
    int nx = 0, ny = 0;
    if (fused_grid(c, ch, cw, c->dedupe, &nx, &ny)) return 1;
    if (ensure(c, (void**)&c->d_tile_labels, &c->tile_labels_cap, (size_t)nx * ny * c->in_H * c->in_W)) return 1;
    if (tile_range_impl(c, &d_page_hwc, 1, Hs, Ws, d_my, d_mx, ch, cw, 0, nx * ny, c->d_tile_labels, d_thr, c->dedupe, c->owned_mode >= 1)) return 1;
    return stitch_impl(c, c->d_tile_labels, ch, cw, d_labels_hw, c->dedupe);
    API_END
}

int sbbseg_segment_crop(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, int cx, int cy, int cw, int ch,
                        int binarise, uint8_t* labels_hw, int* threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw && Hs > 0 && Ws > 0 && cw > 0 && ch > 0, "bad arguments");
    const size_t spix = (size_t)Hs * Ws, pix = (size_t)ch * cw;
    if (ensure(c, (void**)&c->d_page, &c->page_cap, spix * 3)) return 1;
    if (ensure(c, (void**)&c->d_page_labels, &c->page_labels_cap, pix + 4)) return 1;
    HIPCHK(hipMemcpyAsync(c->d_page, page_hwc, spix * 3, hipMemcpyHostToDevice, c->stream));
    if (sbbseg_segment_crop_dev(c, c->d_page, Hs, Ws, Hp, Wp, cx, cy, cw, ch, binarise, c->d_page_labels, nullptr)) return 1;
    if (labels_to_host(c, labels_hw, pix)) return 1;
    int thr = 0;
    if (binarise) HIPCHK(hipMemcpyAsync(&thr, (int*)(c->d_hist + 256), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (threshold) *threshold = thr;
    return 0;
    API_END
}

// The per-call tables of the many-view entry points (sbbseg_segment_views_dev, sbbseg_segment_whole_views_dev): c->h_views (pinned) and
// c->d_views hold at least `bytes`, and the staging may be rewritten (the previous call's upload has read it).
static int views_staging(sbbseg_ctx* c, size_t bytes)
{
    if (c->views_copy_pending) {                               // (the previous call's upload still reads the staging)
        HIPCHK(hipEventSynchronize(c->ev_views));
        c->views_copy_pending = false;
    }
    if (!c->ev_views) HIPCHK(hipEventCreateWithFlags(&c->ev_views, hipEventDisableTiming));
    if (c->h_views_cap < bytes) {
        c->h_views_cap = 0;
        (void)hipHostFree(c->h_views); c->h_views = nullptr;
        const size_t cap = bytes + bytes / 2;
        HIPCHK(hipHostMalloc(&c->h_views, cap, hipHostMallocDefault));
        c->h_views_cap = cap;
    }
    if (c->views_cap < bytes && ensure(c, &c->d_views, &c->views_cap, bytes + bytes / 2)) return 1;
    return 0;
}

// ---- many views in one call: tiles of differently sized pages and crops share launches (include/sbbseg.h) ----
// Per call: the view table (region.h ViewRec), a fallback threshold int per view and the nearest maps of the rescaled views are laid out in
// pinned staging and go up in one asynchronous copy; per group of views (about eight chunks of tiles, which bounds the tile-label scratch):
// the pooled tile list through run_chunked -- one ingest and one region-table launch per lane-chunk -- and one stitch launch.
int sbbseg_segment_views_dev(sbbseg_ctx* c, int n_views, const sbbseg_view* views)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_views >= 1, "n_views %d < 1", n_views);
    REQUIRE(views, "null view array");
    alloc_check();
    const int margin = margin_of(c->in_W);
    const size_t per = (size_t)c->in_H * c->in_W;
    struct Group { int v0, v1, tiles; unsigned blocks; };
    struct MapAt { int src, dst, off; };
    std::vector<ViewRec> recs(n_views);
    std::vector<Group> groups;
    std::vector<MapAt> map_at;
    std::vector<int> maps, one;
    auto map_offset = [&](int src, int dst) -> int {          // (the views of one document share their maps)
        for (const MapAt& m : map_at)
            if (m.src == src && m.dst == dst) return m.off;
        nearest_map(src, dst, one);        // scaled row -> stored row   (main.py:214 -> 112-113)
        map_at.push_back({src, dst, (int)maps.size()});
        maps.insert(maps.end(), one.begin(), one.end());
        return map_at.back().off;
    };
    const int group_cap = 8 * c->max_batch;
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_view& v = views[k];
        REQUIRE(v.d_page_hwc && v.d_labels_hw, "view %d: null page / label pointer", k);
        REQUIRE(v.Hs > 0 && v.Ws > 0 && v.Hp > 0 && v.Wp > 0, "view %d: bad page size %dx%d (stored %dx%d)", k, v.Hp, v.Wp, v.Hs, v.Ws);
        REQUIRE(v.cx >= 0 && v.cy >= 0 && v.cw > 0 && v.ch > 0 && (long)v.cx + v.cw <= v.Wp && (long)v.cy + v.ch <= v.Hp,
                "view %d: crop box {%d,%d,%d,%d} leaves the %dx%d page", k, v.cx, v.cy, v.cw, v.ch, v.Hp, v.Wp);
        REQUIRE_GEOMETRY(v.ch >= c->in_H && v.cw >= c->in_W, "view %d: cropped page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)",
                k, v.ch, v.cw, c->in_H, c->in_W);
        ViewRec& r = recs[k];
        memset(&r, 0, sizeof(r));
        if (fused_grid(c, v.ch, v.cw, c->dedupe, &r.nx, &r.ny)) return 1;
        r.page = (const uint8_t*)v.d_page_hwc; r.labels = (uint8_t*)v.d_labels_hw; r.src_Wp = v.Ws; r.cw = v.cw; r.ch = v.ch;
        r.n_tiles = r.nx * r.ny;
        REQUIRE(r.n_tiles < 1 << 30, "view %d: %d x %d tiles are too many", k, r.nx, r.ny);
        r.mapped = v.Hs != v.Hp || v.Ws != v.Wp;
        r.my = r.mapped ? map_offset(v.Hs, v.Hp) + v.cy : v.cy;
        r.mx = r.mapped ? map_offset(v.Ws, v.Wp) + v.cx : v.cx;
        if (groups.empty() || groups.back().tiles + r.n_tiles > group_cap) groups.push_back({k, k, 0, 0u});
        Group& g = groups.back();
        r.first = g.tiles; r.blk_first = g.blocks;
        const size_t blocks = ((size_t)v.ch * v.cw + 255) / 256;
        REQUIRE(g.blocks + blocks < (size_t)1 << 31, "view %d: the group's label planes are too large for one stitch launch", k);
        g.v1 = k + 1; g.tiles += r.n_tiles; g.blocks += (unsigned)blocks;
    }
    size_t most = 0;
    for (const Group& g : groups) most = most > (size_t)g.tiles ? most : (size_t)g.tiles;
    // one buffer: [n_views] ViewRec | [n_views] int thresholds (views that bring no device int of their own) | maps
    const size_t thr_at = sizeof(ViewRec) * (size_t)n_views, maps_at = thr_at + sizeof(int) * (size_t)n_views;
    const size_t bytes = maps_at + sizeof(int) * maps.size();
    if (views_staging(c, bytes)) return 1;
    if (ensure(c, (void**)&c->d_tile_labels, &c->tile_labels_cap, most * per)) return 1;
    const ViewRec* d_recs = (const ViewRec*)c->d_views;
    int* d_thr = (int*)((char*)c->d_views + thr_at);
    const int* d_maps = (const int*)((char*)c->d_views + maps_at);
    for (int k = 0; k < n_views; ++k) recs[k].thr = views[k].binarise ? (views[k].d_threshold ? views[k].d_threshold : d_thr + k) : nullptr;
    memcpy(c->h_views, recs.data(), thr_at);
    memset((char*)c->h_views + thr_at, 0, maps_at - thr_at);
    if (!maps.empty()) memcpy((char*)c->h_views + maps_at, maps.data(), sizeof(int) * maps.size());
    HIPCHK(hipMemcpyAsync(c->d_views, c->h_views, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_views, c->stream));
    c->views_copy_pending = true;
    c->d_views_thr = d_thr;
    for (int k = 0; k < n_views; ++k) {                        // otsu_copy over exactly the crop's pixels (channel 0), view by view
        const ViewRec& r = recs[k];
        if (!r.thr) continue;
        const uint8_t* pg = r.mapped ? r.page : r.page + ((size_t)r.my * r.src_Wp + r.mx) * 3;
        HIPCHK(launch_otsu(pg, r.src_Wp, r.ch, r.cw, r.mapped ? d_maps + r.my : nullptr, r.mapped ? d_maps + r.mx : nullptr, c->d_hist,
                           (int*)r.thr, c->num_cus, c->stream));
    }
    const bool regions = c->owned_mode >= 1 && c->region_levels > 0 && c->max_batch <= kRegionMaxPatches;
    RegionViewsBuildParams bp;
    memset(&bp, 0, sizeof(bp));
    if (regions) region_plan_levels(c, bp.g);
    bp.tile_h = c->in_H; bp.tile_w = c->in_W; bp.margin = margin;
    for (const Group& g : groups) {
        const ViewRec* gv = recs.data() + g.v0;
        const int nv = g.v1 - g.v0;
        auto run_chunk = [&](int lane, int first, int nb) -> int {
            LaneScope scope(c, lane);
            RegionOff roff{c};
            if (regions) {                                     // the chunk's tables, on the lane's stream in front of its forward
                RegionViewsBuildParams lp = bp;
                lp.views = d_recs + g.v0; lp.n_views = nv; lp.g0 = first; lp.nb = nb;
                for (int L = 0; L < lp.g.n_levels; ++L) {
                    long total = 0;
                    for (int q = 0, w = view_find(nv, (unsigned)first, [&](int m) { return (unsigned)gv[m].first; }); q < nb; ++q) {
                        while (first + q >= gv[w].first + gv[w].n_tiles) ++w;
                        const int local = first + q - gv[w].first, i = local / gv[w].ny, j = local - i * gv[w].ny;
                        total += region_entries(lp.g, view_axis_x(gv[w], c->in_W, margin), view_axis_y(gv[w], c->in_H, margin), i, j, L);
                    }
                    if (region_level_table(c, lane, lp.g, L, nb, total)) return 1;
                    lp.out[L] = c->d_rtab[lane][L]; lp.total[L] = (int)total;
                }
                HIPCHK(launch_region_build_views(lp, c->stream));
                c->views_launches += 1;
                c->rr.on = true;
            }
            IngestParams fp;
            if (fill_ingest(c, fp)) return 1;                  // (input-form pointers of this lane)
            IngestViewsParams ip;
            memset(&ip, 0, sizeof(ip));
            ip.views = d_recs + g.v0; ip.maps = d_maps; ip.n_views = nv; ip.g0 = first; ip.n_tiles = nb;
            ip.H = c->in_H; ip.W = c->in_W; ip.margin = margin; ip.lut = fp.lut; ip.c8 = fp.c8; ip.pairs = fp.pairs; ip.pad = fp.pad; ip.pairs_w = fp.pairs_w;
            HIPCHK(launch_ingest_views(ip, c->precision, c->stream));
            c->views_launches += 1;
            return run_plan(c, nb, c->d_tile_labels + (size_t)first * per, nullptr);
        };
        if (run_chunked(c, g.tiles, run_chunk)) return 1;
        HIPCHK(launch_stitch_views(c->d_tile_labels, c->in_H, c->in_W, margin, d_recs + g.v0, nv, g.blocks, c->stream));
        c->views_launches += 1;
    }
    return 0;
    API_END
}

int sbbseg_segment_views(sbbseg_ctx* c, int n_views, const sbbseg_view* views_host_pointers, int* thresholds)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_views >= 1, "n_views %d < 1", n_views);
    REQUIRE(views_host_pointers, "null view array");
    alloc_check();
    std::vector<sbbseg_view> dv(views_host_pointers, views_host_pointers + n_views);
    std::vector<size_t> page_at(n_views), plane_at(n_views);
    size_t page_bytes = 0, plane_bytes = 0, most_pix = 0;
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_view& v = dv[k];
        REQUIRE(v.d_page_hwc && v.d_labels_hw, "view %d: null page / label pointer", k);
        REQUIRE(v.Hs > 0 && v.Ws > 0 && v.cw > 0 && v.ch > 0, "view %d: bad page or crop size", k);
        int same = 0;
        while (same < k && dv[same].d_page_hwc != v.d_page_hwc) ++same;
        if (same < k) {
            REQUIRE(dv[same].Hs == v.Hs && dv[same].Ws == v.Ws, "view %d: the page of view %d with another stored size", k, same);
            page_at[k] = page_at[same];
        } else {
            page_at[k] = page_bytes;
            page_bytes += ((size_t)v.Hs * v.Ws * 3 + 15) & ~(size_t)15;
        }
        const size_t pix = (size_t)v.ch * v.cw;
        plane_at[k] = plane_bytes;
        plane_bytes += (pix + 4 + 15) & ~(size_t)15;
        most_pix = most_pix > pix ? most_pix : pix;
    }
    if (ensure(c, (void**)&c->d_page, &c->page_cap, page_bytes)) return 1;
    if (ensure(c, (void**)&c->d_page_labels, &c->page_labels_cap, plane_bytes)) return 1;
    if (c->label_channels == 3 && ensure(c, (void**)&c->d_page_labels3, &c->page_labels3_cap, (most_pix + 3) / 4 * 12)) return 1;
    for (int k = 0; k < n_views; ++k) {
        int same = 0;
        while (dv[same].d_page_hwc != dv[k].d_page_hwc) ++same;
        if (same == k)
            HIPCHK(hipMemcpyAsync(c->d_page + page_at[k], views_host_pointers[k].d_page_hwc, (size_t)dv[k].Hs * dv[k].Ws * 3, hipMemcpyHostToDevice, c->stream));
    }
    for (int k = 0; k < n_views; ++k) {                        // (after the search above: it compares the caller's host pointers)
        dv[k].d_page_hwc = c->d_page + page_at[k];
        dv[k].d_labels_hw = c->d_page_labels + plane_at[k];
        dv[k].d_threshold = nullptr;
    }
    if (sbbseg_segment_views_dev(c, n_views, dv.data())) {
        (void)hipStreamSynchronize(c->stream);                 // (the uploads read the caller's pages)
        return 1;
    }
    for (int k = 0; k < n_views; ++k) {
        const size_t pix = (size_t)dv[k].ch * dv[k].cw;
        const uint8_t* plane = c->d_page_labels + plane_at[k];
        if (c->label_channels == 3) {
            HIPCHK(launch_replicate3(plane, c->d_page_labels3, pix, c->stream));
            HIPCHK(hipMemcpyAsync(views_host_pointers[k].d_labels_hw, c->d_page_labels3, pix * 3, hipMemcpyDeviceToHost, c->stream));
        } else {
            HIPCHK(hipMemcpyAsync(views_host_pointers[k].d_labels_hw, plane, pix, hipMemcpyDeviceToHost, c->stream));
        }
    }
    std::vector<int> thr(n_views, 0);
    HIPCHK(hipMemcpyAsync(thr.data(), c->d_views_thr, sizeof(int) * (size_t)n_views, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (thresholds)
        for (int k = 0; k < n_views; ++k) thresholds[k] = dv[k].binarise ? thr[k] : 0;
    return 0;
    API_END
}

int sbbseg_debug_axis_owner(int extent, int tile, int margin, int n_tiles, int32_t* own)
{
    API_BEGIN
    REQUIRE(own && tile > 2 * margin && margin >= 0 && extent >= tile && n_tiles >= 1, "bad arguments");
    const RegionAxis a = {extent, tile, margin, tile - 2 * margin, n_tiles};
    for (int q = 0; q < extent; ++q) own[q] = region_owner(a, q);
    return 0;
    API_END
}

int sbbseg_segment_whole(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int out_h, int out_w, uint8_t* labels_out)
{
    API_BEGIN
    return sbbseg_segment_whole_scaled(c, page_hwc, Hp, Wp, Hp, Wp, out_h, out_w, labels_out);
    API_END
}

// do_prediction(patches=False) on the page as upscaled to Hs x Ws: the page comes from host memory (page_hwc) or is already on the
// device (d_page_in); the label plane lands in c->d_page_labels and, if labels_out is given, in host memory too -- or, with d_dst, in that
// device buffer alone (labels_out is then NULL).
static int whole_scaled_impl(sbbseg_ctx* c, const uint8_t* page_hwc, const void* d_page_in, int Hp, int Wp, int Hs, int Ws, int out_h, int out_w,
                             uint8_t* labels_out, void* d_dst = nullptr)
{
    const size_t pix = (size_t)Hp * Wp, opix = (size_t)out_h * out_w;
    if (!d_page_in && ensure(c, (void**)&c->d_page, &c->page_cap, pix * 3)) return 1;
    if (!d_dst && ensure(c, (void**)&c->d_page_labels, &c->page_labels_cap, opix + 4)) return 1;
    const size_t need = sizeof(int) * (size_t)(c->in_H + c->in_W + out_h + out_w);
    const bool cached = c->d_wmap && c->wmap_cap >= need && c->wmap_key[0] == Hp && c->wmap_key[1] == Wp && c->wmap_key[2] == Hs &&
                        c->wmap_key[3] == Ws && c->wmap_key[4] == out_h && c->wmap_key[5] == out_w;
    if (!cached) {                         // the four gather tables depend on the sizes only: built and uploaded once per geometry
        std::vector<int> my, mx, oy, ox;
        nearest_map(Hs, c->in_H, my);      // model row  -> row of the page do_prediction was handed (main.py:371)
        nearest_map(Ws, c->in_W, mx);
        if (Hs != Hp || Ws != Wp) {        // that page is itself the nearest-upscaled stored image (main.py:214): compose
            std::vector<int> sy, sx;
            nearest_map(Hp, Hs, sy);       // scaled row -> stored row
            nearest_map(Wp, Ws, sx);
            for (auto& v : my) v = sy[v];
            for (auto& v : mx) v = sx[v];
        }
        nearest_map(c->in_H, out_h, oy);   // output row -> model row  (main.py:378)
        nearest_map(c->in_W, out_w, ox);
        if (ensure(c, (void**)&c->d_wmap, &c->wmap_cap, need)) return 1;
        c->wmap_key[0] = 0;
        int* d_my = c->d_wmap; int* d_mx = d_my + c->in_H; int* d_oy = d_mx + c->in_W; int* d_ox = d_oy + out_h;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(d_my, my.data(), sizeof(int) * c->in_H, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_mx, mx.data(), sizeof(int) * c->in_W, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_oy, oy.data(), sizeof(int) * out_h, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ox, ox.data(), sizeof(int) * out_w, hipMemcpyHostToDevice));
        c->wmap_key[0] = Hp; c->wmap_key[1] = Wp; c->wmap_key[2] = Hs; c->wmap_key[3] = Ws; c->wmap_key[4] = out_h; c->wmap_key[5] = out_w;
    }
    int* d_my = c->d_wmap; int* d_mx = d_my + c->in_H; int* d_oy = d_mx + c->in_W; int* d_ox = d_oy + out_h;
    if (!d_page_in) HIPCHK(hipMemcpyAsync(c->d_page, page_hwc, pix * 3, hipMemcpyHostToDevice, c->stream));
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = d_page_in ? (const uint8_t*)d_page_in : c->d_page; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = Hp; ip.src_Wp = Wp; ip.tile_xy = nullptr; ip.n_tiles = 1;
    ip.whole = 1; ip.map_y = d_my; ip.map_x = d_mx;
    HIPCHK(launch_ingest_u8(ip, c->precision, c->stream));
    {
        struct KsplitScope {               // reset on every way out (a throwing run_plan included): later n == 1 launches must not split
            sbbseg_ctx* c;
            explicit KsplitScope(sbbseg_ctx* c_) : c(c_) { c->ksplit_now = c->ksplit; }
            ~KsplitScope() { c->ksplit_now = false; }
        } scope(c);
        if (run_plan(c, 1, c->d_batch_labels, nullptr)) return 1;
    }
    HIPCHK(launch_resize_labels(c->d_batch_labels, c->in_H, c->in_W, d_oy, d_ox, out_h, out_w, d_dst ? (uint8_t*)d_dst : c->d_page_labels, c->stream));
    if (labels_out) {
        if (labels_to_host(c, labels_out, opix)) return 1;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int sbbseg_segment_whole_scaled(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws, int out_h, int out_w,
                                uint8_t* labels_out)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_out && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0 && out_h > 0 && out_w > 0, "bad arguments");
    return whole_scaled_impl(c, page_hwc, nullptr, Hp, Wp, Hs, Ws, out_h, out_w, labels_out);
    API_END
}

// ---- the whole-image branch for many pages in shared launches (include/sbbseg.h): one patch per view, chunks of <= max_batch patches one
// after the other on the handle's stream.  Per call the view table (internal.h WholeViewRec) and every view's four nearest maps -- the
// composed model -> page -> stored maps and the output -> model maps of whole_scaled_impl, shared between views of equal geometry -- go up
// in one asynchronous copy; per chunk one ingest and one label-resize launch.  n_views == 1 is whole_scaled_impl itself (split-K as the
// handle has it); from two views on nothing splits: ksplit_now is only ever set inside whole_scaled_impl.
static int check_whole_views(int n_views, const sbbseg_whole_view* views, bool planes_required)
{
    REQUIRE(n_views >= 1, "n_views %d < 1", n_views);
    REQUIRE(views, "null view array");
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_whole_view& v = views[k];
        REQUIRE(v.d_page_hwc && (v.d_labels_out || !planes_required), "view %d: null page / label pointer", k);
        REQUIRE(v.stored_h > 0 && v.stored_w > 0 && v.page_h > 0 && v.page_w > 0 && v.out_h > 0 && v.out_w > 0,
                "view %d: bad size (stored %dx%d, page %dx%d, labels %dx%d)", k, v.stored_h, v.stored_w, v.page_h, v.page_w, v.out_h, v.out_w);
    }
    return 0;
}

static int whole_views_impl(sbbseg_ctx* c, int n_views, const sbbseg_whole_view* views)
{
    if (check_whole_views(n_views, views, true)) return 1;
    if (n_views == 1) {
        const sbbseg_whole_view& v = views[0];
        if (whole_scaled_impl(c, nullptr, v.d_page_hwc, v.stored_h, v.stored_w, v.page_h, v.page_w, v.out_h, v.out_w, nullptr, v.d_labels_out)) return 1;
        c->whole_launches += 2;
        return 0;
    }
    alloc_check();
    // chunks of equal size, as run_chunked cuts a tile list (9 views at max_batch 4: 3 + 3 + 3)
    const int n_chunks = (n_views + c->max_batch - 1) / c->max_batch, chunk = (n_views + n_chunks - 1) / n_chunks;
    struct MapAt { int a, b, m, off; };
    std::vector<MapAt> map_at;
    std::vector<int> maps, one, two;
    auto map_offset = [&](int stored, int page, int model) -> int {       // model index -> stored index; page = 0: destination index -> model index
        for (const MapAt& m : map_at)
            if (m.a == stored && m.b == page && m.m == model) return m.off;
        if (page == 0) nearest_map(model, stored, one);                   // (a = the destination length here: main.py:378)
        else {
            nearest_map(page, model, one);                                // model row -> row of the page do_prediction was handed (main.py:371)
            if (page != stored) {                                         // ... itself the nearest-upscaled stored image (main.py:214): compose
                nearest_map(stored, page, two);
                for (auto& q : one) q = two[q];
            }
        }
        map_at.push_back({stored, page, model, (int)maps.size()});
        maps.insert(maps.end(), one.begin(), one.end());
        return map_at.back().off;
    };
    std::vector<WholeViewRec> recs(n_views);
    std::vector<unsigned> chunk_blocks(n_chunks, 0u);
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_whole_view& v = views[k];
        WholeViewRec& r = recs[k];
        memset(&r, 0, sizeof(r));
        r.page = (const uint8_t*)v.d_page_hwc; r.out = (uint8_t*)v.d_labels_out; r.stored_w = v.stored_w; r.out_h = v.out_h; r.out_w = v.out_w;
        r.my = map_offset(v.stored_h, v.page_h, c->in_H); r.mx = map_offset(v.stored_w, v.page_w, c->in_W);
        r.oy = map_offset(v.out_h, 0, c->in_H); r.ox = map_offset(v.out_w, 0, c->in_W);
        r.lead = (unsigned)((uintptr_t)v.d_labels_out & 15);
        unsigned& blocks = chunk_blocks[k / chunk];
        r.blk_first = blocks;
        const size_t nb = ((size_t)r.lead + (size_t)v.out_h * v.out_w + kResizeViewsBlockBytes - 1) / kResizeViewsBlockBytes;
        REQUIRE(blocks + nb < (size_t)1 << 31, "view %d: the chunk's label planes are too large for one resize launch", k);
        blocks += (unsigned)nb;
    }
    const size_t maps_at = sizeof(WholeViewRec) * (size_t)n_views, bytes = maps_at + sizeof(int) * maps.size();
    if (views_staging(c, bytes)) return 1;
    memcpy(c->h_views, recs.data(), maps_at);
    memcpy((char*)c->h_views + maps_at, maps.data(), sizeof(int) * maps.size());
    HIPCHK(hipMemcpyAsync(c->d_views, c->h_views, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_views, c->stream));
    c->views_copy_pending = true;
    const WholeViewRec* d_recs = (const WholeViewRec*)c->d_views;
    const int* d_maps = (const int*)((char*)c->d_views + maps_at);
    for (int q = 0, first = 0; first < n_views; ++q, first += chunk) {
        const int nb = n_views - first < chunk ? n_views - first : chunk;
        IngestParams fp;
        if (fill_ingest(c, fp)) return 1;
        IngestWholeViewsParams ip;
        memset(&ip, 0, sizeof(ip));
        ip.views = d_recs + first; ip.maps = d_maps; ip.n_views = nb; ip.H = c->in_H; ip.W = c->in_W;
        ip.lut = fp.lut; ip.c8 = fp.c8; ip.pairs = fp.pairs; ip.pad = fp.pad; ip.pairs_w = fp.pairs_w;
        HIPCHK(launch_ingest_whole_views(ip, c->precision, c->stream));
        if (run_plan(c, nb, c->d_batch_labels, nullptr)) return 1;              // (ksplit_now is false: no launch splits, whatever nb is)
        HIPCHK(launch_resize_labels_views(c->d_batch_labels, c->in_H, c->in_W, d_recs + first, d_maps, nb, chunk_blocks[q], c->stream));
        c->whole_launches += 2;
    }
    return 0;
}

int sbbseg_segment_whole_views_dev(sbbseg_ctx* c, int n_views, const sbbseg_whole_view* views)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return whole_views_impl(c, n_views, views);
    API_END
}

// ---- device buffers for callers that have no device runtime of their own (the reference's environment is Keras/TF, not PyTorch):
// what run() keeps resident across its three stages -- the stored page, the border mask, the region map, the textline map -- lives in
// buffers the library hands out.  They belong to the handle that allocated them (sbbseg_destroy frees what is left) but any handle of
// the same device may read and write them.
int sbbseg_device_alloc(sbbseg_ctx* c, size_t bytes, void** d_ptr)
{
    API_BEGIN
    REQUIRE(c != nullptr && d_ptr != nullptr && bytes > 0, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    alloc_check();
    void* p = nullptr;
    c->user_bufs.reserve(c->user_bufs.size() + 1);
    if (dmalloc(c, &p, bytes)) return 1;
    c->user_bufs.push_back({p, bytes});
    *d_ptr = p;
    return 0;
    API_END
}

int sbbseg_device_free(sbbseg_ctx* c, void* d_ptr)
{
    API_BEGIN
    REQUIRE(c != nullptr, "null handle");
    if (!d_ptr) return 0;
    for (size_t i = 0; i < c->user_bufs.size(); ++i)
        if (c->user_bufs[i].first == d_ptr) {
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipDeviceSynchronize());            // DEVICE-wide on purpose: any handle on the device may use the buffer (sbbseg.h), so
                                                       // other handles' streams may still be reading it; a free is not a hot-path call
            HIPCHK(hipFree(d_ptr));
            c->device_bytes -= c->user_bufs[i].second;
            c->user_bufs.erase(c->user_bufs.begin() + (long)i);
            return 0;
        }
    return set_error("sbbseg_device_free: %p was not allocated by this handle", d_ptr);
    API_END
}

// host -> device / device -> host on the handle's stream; both return when the copy is complete, so the buffer may be handed to
// another handle (another stream) right away.
int sbbseg_upload(sbbseg_ctx* c, void* d_dst, const void* src, size_t bytes)
{
    API_BEGIN
    REQUIRE(c != nullptr && d_dst && src, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_download(sbbseg_ctx* c, void* dst, const void* d_src, size_t bytes)
{
    API_BEGIN
    REQUIRE(c != nullptr && dst && d_src, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

// a u8 label plane [pixels] on the device -> host memory, as one plane or as the three identical channels do_prediction returns
// (main.py:366; replicated on the device, sbbseg_set_label_channels is not consulted)
int sbbseg_download_labels(sbbseg_ctx* c, uint8_t* dst, const void* d_labels_hw, size_t pixels, int channels)
{
    API_BEGIN
    REQUIRE(c != nullptr && dst && d_labels_hw && pixels > 0 && (channels == 1 || channels == 3), "bad arguments (channels: 1 or 3)");
    HIPCHK(hipSetDevice(c->device));
    if (channels == 3) {
        if (ensure(c, (void**)&c->d_page_labels3, &c->page_labels3_cap, (pixels + 3) / 4 * 12)) return 1;
        HIPCHK(launch_replicate3((const uint8_t*)d_labels_hw, c->d_page_labels3, pixels, c->stream));
        HIPCHK(hipMemcpyAsync(dst, c->d_page_labels3, pixels * 3, hipMemcpyDeviceToHost, c->stream));
    } else {
        HIPCHK(hipMemcpyAsync(dst, d_labels_hw, pixels, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_extract_page_box(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws, uint8_t* mask_out, int32_t* box_xywh,
                            int64_t* pixels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && box_xywh && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0, "bad arguments");
    // border model on the (virtually) upscaled page, result at the upscaled size (main.py:384-392) ...  (mask_out == NULL: the mask --
    // a local of extract_page in the reference -- stays on the device)
    if (whole_scaled_impl(c, page_hwc, nullptr, Hp, Wp, Hs, Ws, Hs, Ws, mask_out)) return 1;
    // ... whose label plane is still in d_page_labels: threshold, dilate x 6, largest component, bounding box (main.py:394-404)
    return sbbseg_page_box_dev(c, c->d_page_labels, Hs, Ws, box_xywh, pixels);
    API_END
}

int sbbseg_extract_page_box_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int Hs, int Ws, void* d_mask_out, int32_t* box_xywh,
                                int64_t* pixels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && box_xywh && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0, "bad arguments");
    if (whole_scaled_impl(c, nullptr, d_page_hwc, Hp, Wp, Hs, Ws, Hs, Ws, nullptr)) return 1;
    if (d_mask_out) HIPCHK(hipMemcpyAsync(d_mask_out, c->d_page_labels, (size_t)Hs * Ws, hipMemcpyDeviceToDevice, c->stream));
    return sbbseg_page_box_dev(c, c->d_page_labels, Hs, Ws, box_xywh, pixels);
    API_END
}

// extract_page's model + glue for many pages: the border forwards at batch width (whole_views_impl), then the box search plane by plane.
int sbbseg_extract_page_boxes_dev(sbbseg_ctx* c, int n_pages, const sbbseg_whole_view* views, int32_t* boxes_xywh, int64_t* pixels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(boxes_xywh, "bad arguments");
    if (check_whole_views(n_pages, views, false)) return 1;
    alloc_check();
    std::vector<sbbseg_whole_view> v(views, views + n_pages);
    std::vector<size_t> at(n_pages, 0);
    size_t scratch = 0;
    for (int k = 0; k < n_pages; ++k) {
        REQUIRE(v[k].out_h == v[k].page_h && v[k].out_w == v[k].page_w, "view %d: the mask %dx%d must have the page's size %dx%d", k, v[k].out_h, v[k].out_w,
                v[k].page_h, v[k].page_w);
        REQUIRE((size_t)v[k].page_h * v[k].page_w < ((size_t)1 << 31), "view %d: mask too large for 32-bit pixel indices", k);
        if (v[k].d_labels_out) continue;
        at[k] = scratch;
        scratch += ((size_t)v[k].page_h * v[k].page_w + 15) & ~(size_t)15;
    }
    if (scratch && ensure(c, (void**)&c->d_page_labels, &c->page_labels_cap, scratch + 16)) return 1;      // (the masks nobody asked for)
    for (int k = 0; k < n_pages; ++k)
        if (!v[k].d_labels_out) v[k].d_labels_out = c->d_page_labels + at[k];
    if (whole_views_impl(c, n_pages, v.data())) return 1;
    for (int k = 0; k < n_pages; ++k) {                        // main.py:394-404 per plane; an empty mask: {0, 0, 0, 0} / 0
        int64_t px = 0;
        if (sbbseg_page_box_dev(c, v[k].d_labels_out, v[k].page_h, v[k].page_w, boxes_xywh + 4 * k, &px)) return 1;
        if (pixels) pixels[k] = px;
    }
    return 0;
    API_END
}

// ---- the model-running part of run() (main.py:2056-2107) in ONE call: the stored page is uploaded once and stays in device memory for
// all three stages, the border mask and the region map never leave the device between their model and their glue.
//   extract_page (main.py:2061, 384-437)            border model on the page as upscaled to Hs x Ws, dilate x 6, largest contour, box;
//                                                   outside the reference's try: an error here is the call's error
//   extract_text_regions (2072, 439-454)            layout model on the Otsu'd CROP, erode x 3 / dilate x 4 (2074-2075); a failure --
//                                                   e.g. a crop smaller than the model input, main.py:278-285 -- is "no regions" (2089-2091)
//   get_text_region_contours_and_boxes (2083, 2096) existence only: the textline model runs when a contour would be kept
//   textline_contours (2102, 490-503)               textline model on the crop
int sbbseg_run_page(sbbseg_ctx* border, sbbseg_ctx* layout, sbbseg_ctx* textline, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws,
                    int channels, uint8_t* page_mask_out, uint8_t* regions_out, uint8_t* textlines_out, sbbseg_run_info* info)
{
    API_BEGIN
    if (check_ready(border) || check_ready(layout) || check_ready(textline)) return 1;
    REQUIRE(page_hwc && info && regions_out && textlines_out && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0 && (channels == 1 || channels == 3), "bad arguments");
    REQUIRE(border->device == layout->device && border->device == textline->device, "the three handles must live on one device");
    memset(info, 0, sizeof(*info));
    const size_t spix = (size_t)Hp * Wp, pix = (size_t)Hs * Ws;
    if (ensure(border, (void**)&border->d_run_page, &border->run_page_cap, spix * 3)) return 1;
    if (page_mask_out && ensure(border, (void**)&border->d_run_mask, &border->run_mask_cap, pix)) return 1;
    HIPCHK(hipMemcpyAsync(border->d_run_page, page_hwc, spix * 3, hipMemcpyHostToDevice, border->stream));      // the one upload of the page
    int64_t pixels = 0;
    if (sbbseg_extract_page_box_dev(border, border->d_run_page, Hp, Wp, Hs, Ws, page_mask_out ? border->d_run_mask : nullptr, info->box_xywh, &pixels)) return 1;
    info->box_pixels = pixels;                                  // (extract_page_box_dev has synchronised the border handle's stream)
    REQUIRE(pixels > 0, "attempt to get argmax of an empty sequence (the border model found no page: main.py:399-401 raises here)");
    if (page_mask_out && sbbseg_download_labels(border, page_mask_out, border->d_run_mask, pix, channels)) return 1;
    const int x = info->box_xywh[0], y = info->box_xywh[1], w = info->box_xywh[2], h = info->box_xywh[3];
    const size_t cpix = (size_t)w * h;
    // A failed stage: wait for whatever it had queued (its kernels read border->d_run_page and the handle's d_run_a / d_run_b, which the next
    // call overwrites / may reallocate), then decide what the failure is.  Only a crop that cannot hold one model input -- what makes the
    // reference's own loop raise inside its bare try / except (main.py:278-281 under 2069-2091 / 2152-2157) -- degrades to "no regions" /
    // "no lines"; a device or allocation error fails the call with its message in sbbseg_last_error(): a fault must not look like an empty page.
    auto stage_failed = [&](sbbseg_ctx* h) -> bool {          // true: a geometry failure (swallowed, as the reference swallows it)
        const std::string msg = g_err;
        const int kind = g_err_kind;
        (void)hipStreamSynchronize(h->stream);
        if (h->lane_stream) (void)hipStreamSynchronize(h->lane_stream);
        (void)hipGetLastError();
        g_err = msg; g_err_kind = kind;
        return kind == kErrGeometry;
    };
    // layout stage + its post-processing: the reference's bare try / except (main.py:2069-2091)
    int present = 0;
    bool ok = false;
    do {
        if (ensure(layout, (void**)&layout->d_run_a, &layout->run_a_cap, cpix + 4) || ensure(layout, (void**)&layout->d_run_b, &layout->run_b_cap, cpix + 4)) break;
        int* d_thr = (int*)(layout->d_hist + 256);
        if (sbbseg_segment_crop_dev(layout, border->d_run_page, Hp, Wp, Hs, Ws, x, y, w, h, 1, layout->d_run_a, d_thr)) break;
        if (sbbseg_morph_dev(layout, layout->d_run_a, h, w, SBBSEG_MORPH_ERODE, 5, 3, layout->d_run_b)) break;          // main.py:2074
        if (sbbseg_morph_dev(layout, layout->d_run_b, h, w, SBBSEG_MORPH_DILATE, 5, 4, layout->d_run_b)) break;         // main.py:2075
        if (sbbseg_text_regions_present_dev(layout, layout->d_run_b, h, w, 1, 0.00001, &present)) break;                 // main.py:2083, 2096
        if (sbbseg_download(layout, &info->otsu_threshold, d_thr, sizeof(int))) break;
        if (sbbseg_download_labels(layout, regions_out, layout->d_run_b, cpix, channels)) break;
        info->regions_ok = 1;
        ok = true;
    } while (0);
    if (!ok && !stage_failed(layout)) return 1;
    info->text_present = info->regions_ok ? present : 0;
    if (info->text_present) {                                  // main.py:2096-2107; a failure = the outer except (2152-2157): no lines
        ok = false;
        do {
            if (ensure(textline, (void**)&textline->d_run_a, &textline->run_a_cap, cpix + 4)) break;
            if (sbbseg_segment_crop_dev(textline, border->d_run_page, Hp, Wp, Hs, Ws, x, y, w, h, 0, textline->d_run_a, nullptr)) break;
            if (sbbseg_download_labels(textline, textlines_out, textline->d_run_a, cpix, 1)) break;
            info->textlines_ok = 1;
            ok = true;
        } while (0);
        if (!ok && !stage_failed(textline)) return 1;
    }
    return 0;
    API_END
}

// ---- sbbseg_run_page for many pages: the stored pages go up once, the border forwards run at batch width, the layout and textline models
// take all pages' crops in one sbbseg_segment_views_dev call each; masks, region maps and textline maps stay on the device between their
// model and their glue.  What run() swallows for a page -- a crop that cannot hold a model input -- is decided by geometry before the
// pooled call; any failure of a library call is a device or allocation error and fails the whole call.
int sbbseg_run_pages(sbbseg_ctx* border, sbbseg_ctx* layout, sbbseg_ctx* textline, int n_pages, sbbseg_run_page_io* pages, int channels)
{
    API_BEGIN
    if (check_ready(border) || check_ready(layout) || check_ready(textline)) return 1;
    REQUIRE(n_pages >= 1 && pages && (channels == 1 || channels == 3), "bad arguments");
    REQUIRE(border->device == layout->device && border->device == textline->device, "the three handles must live on one device");
    alloc_check();
    std::vector<size_t> page_at(n_pages), mask_at(n_pages), crop_at(n_pages, 0);
    size_t page_bytes = 0, mask_bytes = 0, crop_bytes = 0;
    for (int k = 0; k < n_pages; ++k) {
        sbbseg_run_page_io& pg = pages[k];
        REQUIRE(pg.page_hwc && pg.regions_out && pg.textlines_out && pg.Hp > 0 && pg.Wp > 0 && pg.Hs > 0 && pg.Ws > 0, "page %d: bad arguments", k);
        memset(&pg.info, 0, sizeof(pg.info));
        pg.status = 0;
        page_at[k] = page_bytes; page_bytes += ((size_t)pg.Hp * pg.Wp * 3 + 15) & ~(size_t)15;
        mask_at[k] = mask_bytes; mask_bytes += ((size_t)pg.Hs * pg.Ws + 15) & ~(size_t)15;
    }
    if (ensure(border, (void**)&border->d_run_page, &border->run_page_cap, page_bytes)) return 1;
    if (ensure(border, (void**)&border->d_run_mask, &border->run_mask_cap, mask_bytes)) return 1;
    // A failed step: wait for whatever is queued (uploads read the caller's pages, kernels read buffers the next call may reallocate)
    auto failed = [&](sbbseg_ctx* h) -> int {
        const std::string msg = g_err;
        const int kind = g_err_kind;
        (void)hipStreamSynchronize(h->stream);
        if (h->lane_stream) (void)hipStreamSynchronize(h->lane_stream);
        (void)hipGetLastError();
        g_err = msg; g_err_kind = kind;
        return 1;
    };
    std::vector<sbbseg_whole_view> wv(n_pages);
    std::vector<int32_t> boxes(4 * (size_t)n_pages);
    std::vector<int64_t> px(n_pages);
    for (int k = 0; k < n_pages; ++k) {
        const sbbseg_run_page_io& pg = pages[k];
        if (hipMemcpyAsync(border->d_run_page + page_at[k], pg.page_hwc, (size_t)pg.Hp * pg.Wp * 3, hipMemcpyHostToDevice, border->stream) != hipSuccess) {
            set_error("upload of page %d failed", k);
            return failed(border);
        }
        wv[k] = {border->d_run_page + page_at[k], pg.Hp, pg.Wp, pg.Hs, pg.Ws, pg.Hs, pg.Ws, border->d_run_mask + mask_at[k]};
    }
    if (sbbseg_extract_page_boxes_dev(border, n_pages, wv.data(), boxes.data(), px.data())) return failed(border);
    HIPCHK(hipStreamSynchronize(border->stream));              // the hand-over: the other two handles read the pages from here on
    for (int k = 0; k < n_pages; ++k) {
        sbbseg_run_page_io& pg = pages[k];
        memcpy(pg.info.box_xywh, &boxes[4 * (size_t)k], sizeof(pg.info.box_xywh));
        pg.info.box_pixels = px[k];
        if (px[k] <= 0) { pg.status = 1; continue; }            // main.py:399-401 raises for this page: nothing else of it is written
        if (pg.page_mask_out && sbbseg_download_labels(border, pg.page_mask_out, border->d_run_mask + mask_at[k], (size_t)pg.Hs * pg.Ws, channels)) return failed(border);
        crop_at[k] = crop_bytes;
        crop_bytes += ((size_t)pg.info.box_xywh[2] * pg.info.box_xywh[3] + 4 + 15) & ~(size_t)15;
    }
    auto fits = [](const sbbseg_ctx* h, const sbbseg_run_page_io& pg) { return pg.info.box_xywh[3] >= h->in_H && pg.info.box_xywh[2] >= h->in_W; };
    auto crop_view = [&](const sbbseg_run_page_io& pg, int k, int binarise) -> sbbseg_view {
        const int32_t* b = pg.info.box_xywh;
        return {border->d_run_page + page_at[k], pg.Hp, pg.Wp, pg.Hs, pg.Ws, b[0], b[1], b[2], b[3], binarise, layout->d_run_a + crop_at[k], nullptr};
    };
    // layout stage (main.py:2069-2091): every page that has a box and whose crop holds one input of the layout model
    std::vector<int> todo;
    std::vector<sbbseg_view> lv;
    for (int k = 0; k < n_pages; ++k)
        if (pages[k].status == 0 && fits(layout, pages[k])) todo.push_back(k);
    if (todo.empty()) return 0;
    if (ensure(layout, (void**)&layout->d_run_a, &layout->run_a_cap, crop_bytes) || ensure(layout, (void**)&layout->d_run_b, &layout->run_b_cap, crop_bytes)) return 1;
    for (int k : todo) lv.push_back(crop_view(pages[k], k, 1));
    if (sbbseg_segment_views_dev(layout, (int)lv.size(), lv.data())) return failed(layout);
    std::vector<int> thr(lv.size(), 0);
    if (sbbseg_download(layout, thr.data(), layout->d_views_thr, sizeof(int) * lv.size())) return failed(layout);
    for (size_t q = 0; q < todo.size(); ++q) {
        const int k = todo[q];
        sbbseg_run_page_io& pg = pages[k];
        const int w = pg.info.box_xywh[2], h = pg.info.box_xywh[3];
        uint8_t* raw = layout->d_run_a + crop_at[k];
        uint8_t* clean = layout->d_run_b + crop_at[k];
        int present = 0;
        if (sbbseg_morph_dev(layout, raw, h, w, SBBSEG_MORPH_ERODE, 5, 3, clean) ||                                         // main.py:2074
            sbbseg_morph_dev(layout, clean, h, w, SBBSEG_MORPH_DILATE, 5, 4, clean) ||                                      // main.py:2075
            sbbseg_text_regions_present_dev(layout, clean, h, w, 1, 0.00001, &present) ||                                   // main.py:2083, 2096
            sbbseg_download_labels(layout, pg.regions_out, clean, (size_t)w * h, channels)) return failed(layout);
        pg.info.otsu_threshold = thr[q];
        pg.info.regions_ok = 1;
        pg.info.text_present = present;
    }
    // textline stage (main.py:2096-2107), on the pages the gate let through.  Its planes take the place of the raw layout maps: every
    // download above has waited for the layout handle's stream, nothing reads them any more.
    todo.clear(); lv.clear();
    for (int k = 0; k < n_pages; ++k)
        if (pages[k].info.text_present && fits(textline, pages[k])) todo.push_back(k);
    if (todo.empty()) return 0;
    for (int k : todo) lv.push_back(crop_view(pages[k], k, 0));
    if (sbbseg_segment_views_dev(textline, (int)lv.size(), lv.data())) return failed(textline);
    for (int k : todo) {
        sbbseg_run_page_io& pg = pages[k];
        if (sbbseg_download_labels(textline, pg.textlines_out, layout->d_run_a + crop_at[k], (size_t)pg.info.box_xywh[2] * pg.info.box_xywh[3], 1)) return failed(textline);
        pg.info.textlines_ok = 1;
    }
    return 0;
    API_END
}

// ----------------------------------------------------------------------------------------- debug
int sbbseg_debug_ingest(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, const int32_t* tile_xy, int n_tiles,
                        int form, float* out, size_t out_floats)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && tile_xy && out && n_tiles >= 1 && n_tiles <= c->max_batch, "bad arguments (n_tiles <= max_batch)");
    REQUIRE(form == SBBSEG_INPUT_C8 || form == SBBSEG_INPUT_PAIRS, "unknown form");
    REQUIRE(c->form_tensor[form] >= 0, "plan does not use input form %d", form);
    const Tensor& t = c->tensors[c->form_tensor[form]];
    const size_t n = t.elems_per_patch * n_tiles;
    REQUIRE(out_floats >= n, "output buffer too small (%zu < %zu)", out_floats, n);
    const size_t pix = (size_t)Hp * Wp;
    if (ensure(c, (void**)&c->d_page, &c->page_cap, pix * 3)) return 1;
    HIPCHK(hipMemcpyAsync(c->d_page, page_hwc, pix * 3, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(c->d_tile_xy, tile_xy, sizeof(int) * 2 * n_tiles, hipMemcpyHostToDevice));
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = c->d_page; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = Hp; ip.src_Wp = Wp; ip.tile_xy = c->d_tile_xy; ip.n_tiles = n_tiles;
    HIPCHK(launch_ingest_u8(ip, c->precision, c->stream));
    float* d_tmp = nullptr;
    HIPCHK(hipMalloc((void**)&d_tmp, n * sizeof(float)));
    hipError_t e = c->planes == 2 ? launch_split_to_f32(t.data(), d_tmp, n / t.C, t.C, c->stream)
                                  : launch_to_f32(t.data(), d_tmp, n, c->precision, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_tmp, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_tmp);
    HIPCHK(e);
    if (c->planes == 2 && form == SBBSEG_INPUT_C8)      // (the hi plane's slots 4..6 repeat lo(ch 0..2) for the fused tail: not channels)
        for (size_t i = 0; i < n; i += 8)
            for (int ch = 3; ch < 8; ++ch) out[i + ch] = 0.f;
    return 0;
    API_END
}

int sbbseg_debug_read_tensor(sbbseg_ctx* c, int tensor_id, int n, float* out, size_t out_floats)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(tensor_id >= 0 && tensor_id < (int)c->tensors.size() && out && n >= 1 && n <= c->max_batch, "bad arguments");
    const Tensor& t = c->tensors[tensor_id];
    const size_t cnt = t.elems_per_patch * n;
    REQUIRE(out_floats >= cnt, "output buffer too small (%zu < %zu)", out_floats, cnt);
    float* d_tmp = nullptr;
    HIPCHK(hipMalloc((void**)&d_tmp, cnt * sizeof(float)));
    hipError_t e = c->planes == 2 ? launch_split_to_f32(t.data(), d_tmp, cnt / t.C, t.C, c->stream)
                                  : launch_to_f32(t.data(), d_tmp, cnt, c->precision, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_tmp, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_tmp);
    HIPCHK(e);
    if (c->planes == 2 && t.is_input_form && t.form == SBBSEG_INPUT_C8)      // (see sbbseg_debug_ingest)
        for (size_t i = 0; i < cnt; i += 8)
            for (int ch = 3; ch < 8; ++ch) out[i + ch] = 0.f;
    return 0;
    API_END
}

int sbbseg_debug_op_launch(sbbseg_ctx* c, int op, int32_t* out, int cap)
{
    API_BEGIN
    REQUIRE(c && out && cap >= 0 && op >= 0 && op < (int)c->ops.size(), "op index out of range");
    const LaunchRec& r = c->ops[op].last;
    const int rec[kLaunchRecInts] = {r.family, r.bp, r.bc, r.stages, r.fast_gather, r.tile_map, r.cls_minor, r.table, r.n_tiles, r.grid,
                                     r.res_epilogue, r.persistent, r.residual};
    static_assert(kLaunchRecInts == SBBSEG_LAUNCH_INTS, "sbbseg.h documents the record");
    for (int i = 0; i < cap && i < kLaunchRecInts; ++i) out[i] = rec[i];
    return 0;
    API_END
}

int sbbseg_debug_tensor_period_mismatches(sbbseg_ctx* c, int tensor_id, int n, int period, int64_t* count, int64_t* first)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(tensor_id >= 0 && tensor_id < (int)c->tensors.size() && count && first && period >= 1 && n >= period && n <= c->max_batch, "bad arguments");
    const Tensor& t = c->tensors[tensor_id];
    const size_t stride = t.elems_per_patch * (size_t)c->elem * c->planes;          // bytes of one stored patch
    REQUIRE(stride % 16 == 0, "patch stride %zu is not a multiple of 16 bytes", stride);
    unsigned long long h_res[2] = {0ull, ~0ull};
    unsigned long long* d_res = nullptr;
    HIPCHK(hipMalloc((void**)&d_res, sizeof(h_res)));
    hipError_t e = hipMemcpyAsync(d_res, h_res, sizeof(h_res), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_period_mismatches(t.data(), stride * period, stride * (size_t)(n - period), d_res, c->num_cus, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_res, d_res, sizeof(h_res), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_res);
    HIPCHK(e);
    *count = (int64_t)h_res[0];
    *first = h_res[0] ? (int64_t)h_res[1] : -1;
    return 0;
    API_END
}

int sbbseg_debug_inject_alloc_failure(int nth_check)
{
    API_BEGIN
    REQUIRE(nth_check >= 0, "nth_check must be >= 0 (0 disarms)");
    g_alloc_fail_countdown = nth_check;
    return 0;
    API_END
}

// ------------------------------------------------------------------------------ multi-GPU: the one collective, on RCCL
int sbbseg_comm_unique_id(char* id128)
{
    API_BEGIN
    REQUIRE(id128, "bad arguments");
    if (rccl_load()) return 1;
    RcclUniqueId id;
    RCCLCHK(g_rccl.GetUniqueId(&id));
    memcpy(id128, id.internal, sizeof(id.internal));
    return 0;
    API_END
}

int sbbseg_comm_init(sbbseg_ctx* c, int rank, int world, const char* id128)
{
    API_BEGIN
    REQUIRE(c && id128 && world >= 1 && rank >= 0 && rank < world, "bad arguments (rank %d of %d)", rank, world);
    HIPCHK(hipSetDevice(c->device));
    if (rccl_load()) return 1;
    comm_release(c);
    RcclUniqueId id;
    memcpy(id.internal, id128, sizeof(id.internal));
    void* comm = nullptr;
    RCCLCHK(g_rccl.CommInitRank(&comm, world, id, rank));
    c->comm = comm; c->comm_rank = rank; c->comm_world = world;
    return 0;
    API_END
}

int sbbseg_comm_info(sbbseg_ctx* c, int* rank, int* world)
{
    API_BEGIN
    REQUIRE(c && rank && world, "bad arguments");
    *rank = c->comm_rank; *world = c->comm ? c->comm_world : 0;
    return 0;
    API_END
}

int sbbseg_comm_destroy(sbbseg_ctx* c)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    comm_release(c);
    return 0;
    API_END
}

int sbbseg_allgather_labels_dev(sbbseg_ctx* c, const void* d_send, size_t bytes_per_rank, void* d_recv)
{
    API_BEGIN
    REQUIRE(c && d_send && d_recv, "bad arguments");
    REQUIRE(c->comm, "no communicator: call sbbseg_comm_init first");
    HIPCHK(hipSetDevice(c->device));
    if (bytes_per_rank == 0) return 0;
    RCCLCHK(g_rccl.AllGather(d_send, d_recv, bytes_per_rank, /* ncclUint8 */ 1, c->comm, c->stream));
    return 0;
    API_END
}

int sbbseg_debug_counter(sbbseg_ctx* c, int which, int64_t* value)
{
    API_BEGIN
    REQUIRE(c && value && which >= 0 && which <= 4, "unknown counter %d (0 = exact host contour rankings, 1 = patches run through the plan, 2 = kernels queued by the line-mask calls, 3 = ingest / region-table / stitch kernels queued by sbbseg_segment_views_dev, 4 = ingest / label-resize kernels queued by the whole-views calls)", which);
    *value = which == 0 ? (int64_t)c->host_contour_calls : which == 1 ? (int64_t)c->forwards : which == 2 ? (int64_t)c->line_launches : which == 3 ? c->views_launches : c->whole_launches;
    return 0;
    API_END
}

int sbbseg_debug_set_conv_variant(sbbseg_ctx* c, int variant)
{
    API_BEGIN
    REQUIRE(c && variant >= 0 && variant <= 0x3ffffff, "variant: bits 0-1 = 0 auto | 1 4-wave/2-stage | 2 8-wave/3-stage; bit 2 = one block per tile (non-persistent); bit 3 = no XCD-grouped tile walk; bit 4 = half-K-step stages; bit 5 = XCD-grouped walk on single-class layers; bit 6 = drain epilogue stores; bit 7 = half-line epilogue stores; bits 8-15 = contiguous-run K limit / 64; bit 16 = 8-phase schedule on the 256x256 tile; bit 17 = plain gather everywhere; bit 18 = fused bottleneck blocks run as their three convs; bit 19 = XCD-contiguous walk for grouped launches; bit 20 = one-group form of the fused block kernel; bit 21 = extract_page ranks contours on the host always; bit 22 = stem and max-pool as two launches; bit 23 = the 224 x 224 decoder conv on the generic kernel; bit 24 = expand + next reduce 1x1 convs as two launches");
    c->conv_variant = variant & 0xff;
    c->ph8 = (variant >> 16) & 1;
    c->plain_gather = (variant >> 17) & 1;
    c->unfuse_blocks = (variant >> 18) & 1;
    c->ranged_walk = (variant >> 19) & 1;
    c->block_pq = !((variant >> 20) & 1);
    c->force_host_contours = (variant >> 21) & 1;
    c->unfuse_stem_pool = (variant >> 22) & 1;
    c->no_dec_halo = (variant >> 23) & 1;
    c->no_expand_reduce = (variant >> 24) & 1;
    c->no_c3er = (variant >> 25) & 1;
    if ((variant >> 8) & 0xff) c->contig_max_k = ((variant >> 8) & 0xff) * 64;
    return 0;
    API_END
}

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
