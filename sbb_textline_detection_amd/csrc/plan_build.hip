// plan_build.hip -- host side of libsbbseg's plan building: the C ABI entry points (include/sbbseg.h) the planner calls in execution
// order -- input forms, tensors, convs, max-pool, tail, head -- and sbbseg_finalize, which fuses what the dedicated kernels take in one
// launch, attaches their tables and allocates the activation buffers.  Nothing here runs per page.  What a kernel reads as weights is
// laid out by wpack.h (host only, checked on the CPU); this unit checks arguments, recognises the fusions and uploads (ctx.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "ctx.h"
#include "wpack.h"

using namespace sbbseg;

extern "C" {

int sbbseg_set_input(sbbseg_ctx* c, int H, int W, int channels)
{
    API_BEGIN
    REQUIRE(c && !c->finalized, "bad handle / already finalized");
    REQUIRE(H > 0 && W > 0 && channels == 3, "input must be HxWx3 (got %dx%dx%d)", H, W, channels);
    c->in_H = H; c->in_W = W; c->in_C = channels;
    return 0;
    API_END
}

int sbbseg_input_form(sbbseg_ctx* c, int form, int pad, int* tensor_id)
{
    API_BEGIN
    REQUIRE(c && !c->finalized && tensor_id, "bad handle / already finalized");
    REQUIRE(c->in_H > 0, "sbbseg_set_input first");
    REQUIRE(form == SBBSEG_INPUT_C8 || form == SBBSEG_INPUT_PAIRS, "unknown input form %d", form);
    if (c->form_tensor[form] >= 0) {
        REQUIRE(c->tensors[c->form_tensor[form]].pad == pad, "input form %d requested with different pad", form);
        *tensor_id = c->form_tensor[form];
        return 0;
    }
    Tensor t;
    t.is_input_form = true; t.form = form; t.pad = pad; t.C = 8;
    if (form == SBBSEG_INPUT_C8) {
        REQUIRE(pad == 0, "C8 form takes pad 0");
        t.H = c->in_H; t.W = c->in_W;
    } else {
        REQUIRE(pad >= 0, "negative pad");
        t.H = c->in_H + 2 * pad; t.W = (c->in_W + 2 * pad + 1) / 2;
    }
    t.elems_per_patch = (size_t)t.H * t.W * t.C;
    c->tensors.push_back(t);
    c->form_tensor[form] = (int)c->tensors.size() - 1;
    *tensor_id = c->form_tensor[form];
    return 0;
    API_END
}

int sbbseg_add_tensor(sbbseg_ctx* c, int H, int W, int C, int* tensor_id)
{
    API_BEGIN
    REQUIRE(c && !c->finalized && tensor_id, "bad handle / already finalized");
    REQUIRE(H > 0 && W > 0 && C > 0 && C % 8 == 0, "tensor %dx%dx%d: channels must be a positive multiple of 8", H, W, C);
    Tensor t;
    t.H = H; t.W = W; t.C = C;
    t.elems_per_patch = (size_t)H * W * C;
    c->tensors.push_back(t);
    *tensor_id = (int)c->tensors.size() - 1;
    return 0;
    API_END
}

int sbbseg_add_conv(sbbseg_ctx* c, const sbbseg_conv_desc* d, const float* w_src0, const float* w_src1,
                    const float* scale, const float* shift, const float* raw_scale, const float* raw_shift,
                    const float* head_w, const float* head_scale, const float* head_shift)
{
    API_BEGIN
    REQUIRE(c && !c->finalized && d && w_src0 && scale && shift, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    AllocScope uploads(c->mem);                  // a failing return below frees what the call uploaded
    REQUIRE(d->n_src == 1 || d->n_src == 2, "n_src must be 1 or 2");
    REQUIRE(d->n_src == 1 || w_src1, "second source needs its weights");
    REQUIRE(d->cout > 0 && d->cout % 8 == 0, "cout %d must be a positive multiple of 8", d->cout);
    REQUIRE(d->out_h > 0 && d->out_w > 0 && d->out_stride_y >= 1 && d->out_stride_x >= 1 && d->out_off_y >= 0 &&
            d->out_off_x >= 0, "bad output grid / placement");
    const int ntens = (int)c->tensors.size();
    for (int s = 0; s < d->n_src; ++s) {
        const sbbseg_conv_src& cs = d->src[s];
        REQUIRE(cs.tensor >= 0 && cs.tensor < ntens, "conv source tensor %d undefined", cs.tensor);
        const Tensor& t = c->tensors[cs.tensor];
        REQUIRE(cs.channels > 0 && ((cs.channels + 7) / 8) * 8 <= t.C, "conv source takes %d channels of a %d-channel tensor", cs.channels, t.C);
        REQUIRE(cs.kh > 0 && cs.kw > 0, "bad kernel size");
        REQUIRE((cs.stride_y == 1 || cs.stride_y == 2) && (cs.stride_x == 1 || cs.stride_x == 2), "strides must be 1 or 2");
        REQUIRE(cs.up_shift == 0 || cs.up_shift == 1, "up_shift must be 0 or 1");
        REQUIRE(!(cs.up_shift && (cs.off_y || cs.off_x)), "offset and upsampling cannot be combined");
        // the last window must start inside the logical input
        const int lh = (t.H << cs.up_shift) + cs.off_y, lw = (t.W << cs.up_shift) + cs.off_x;
        REQUIRE((d->out_h - 1) * cs.stride_y - cs.pad_top < lh && (d->out_w - 1) * cs.stride_x - cs.pad_left < lw,
                "conv geometry: output grid %dx%d does not fit source %d (%dx%d logical)", d->out_h, d->out_w, s, lh, lw);
    }
    REQUIRE(d->out_tensor >= 0 || d->raw_out_tensor >= 0 || d->head_classes > 0, "conv without outputs");
    int TH = -1, TW = -1;
    for (int which = 0; which < 3; ++which) {
        const int id = which == 0 ? d->out_tensor : which == 1 ? d->raw_out_tensor : d->residual_tensor;
        if (id < 0) continue;
        REQUIRE(id < ntens, "conv output/residual tensor %d undefined", id);
        const Tensor& t = c->tensors[id];
        REQUIRE(t.C == d->cout, "conv output tensor has %d channels, cout is %d", t.C, d->cout);
        if (TH < 0) { TH = t.H; TW = t.W; }
        REQUIRE(t.H == TH && t.W == TW, "conv outputs differ in size");
    }
    if (d->head_classes > 0) {
        REQUIRE(c->precision != kF32, "fused head is a 16-bit-mode feature (the fp32 check path runs the head as its own op)");
        REQUIRE(d->cout == 32 && d->head_classes <= 4 && head_w && head_scale && head_shift, "fused head needs cout == 32, <= 4 classes and its weights");
        // several convs may carry the same head (the parity classes of the last decoder conv)
        REQUIRE(c->classes == 0 || (c->fused_heads > 0 && c->classes == d->head_classes), "plan already has a head");
        if (TH < 0) { TH = c->in_H; TW = c->in_W; }
        REQUIRE(TH == c->in_H && TW == c->in_W, "fused head runs at input resolution");
    }
    REQUIRE((d->out_h - 1) * d->out_stride_y + d->out_off_y < TH && (d->out_w - 1) * d->out_stride_x + d->out_off_x < TW,
            "output placement leaves the %dx%d tensor", TH, TW);

    Op op;
    op.type = kConv;
    ConvOp& co = op.conv;
    co.d = *d;
    co.Ho = d->out_h; co.Wo = d->out_w; co.TH = TH; co.TW = TW;
    const int bc = c->precision != kF32 ? 256 : 4;          // pad weight rows for the widest channel tile any variant uses
    co.cout_pad = ((d->cout + bc - 1) / bc) * bc;

    // contraction order, slot table and K-step records: conv_ktable (wpack.h)
    alloc_check();
    const bool split = is_split(c->precision);
    static const bool grouped_taps = !(getenv("SBBSEG_TAP_ORDER") && getenv("SBBSEG_TAP_ORDER")[0] == '0');
    const int src_C[2] = {c->tensors[d->src[0].tensor].C, d->n_src == 2 ? c->tensors[d->src[1].tensor].C : 0};
    const ConvKTable kt = conv_ktable(*d, src_C, c->precision, grouped_taps);
    double geo_macs = 0;
    for (int s = 0; s < d->n_src; ++s) {
        co.ksteps[s] = kt.ksteps_src[s];
        geo_macs += (double)d->src[s].kh * d->src[s].kw * d->src[s].channels;
    }
    co.total_ksteps = kt.total_ksteps;
    co.Ktot = co.total_ksteps * kBK;
    REQUIRE((size_t)co.cout_pad * co.Ktot * c->elem < (size_t)3 << 30, "weight matrix too large");
    const float* const w_src[2] = {w_src0, w_src1};
    float wpre = 1.f;                                        // split mode: the conv's power-of-two weight pre-scale (split_prescale)
    if (split) {
        float wmax = 0.f;
        for (int s = 0; s < d->n_src; ++s) wmax = max_abs(w_src[s], (size_t)d->src[s].kh * d->src[s].kw * d->src[s].channels * d->cout, wmax);
        REQUIRE(std::isfinite(wmax), "%s: non-finite weights", "conv");
        wpre = split_prescale(wmax);
        co.wmul_cls[0] = 1.f / wpre;
    }
    if (c->precision != kF32) {
        if (upload(c, (uint16_t**)&co.d_w, conv_pack_matrix<uint16_t>(kt, *d, w_src, c->precision, co.cout_pad, wpre))) return 1;
    } else {
        if (upload(c, (float**)&co.d_w, conv_pack_matrix<float>(kt, *d, w_src, c->precision, co.cout_pad, wpre))) return 1;
    }
    if (upload(c, &co.d_ktab, kt.ktab) || upload(c, &co.d_kstep, kt.ksteps)) return 1;
    memcpy(co.tap_lo, kt.tap_lo, sizeof(co.tap_lo));
    memcpy(co.tap_hi, kt.tap_hi, sizeof(co.tap_hi));
    co.fg_ok = kt.fg_ok;
    co.h_ksteps_cls[0] = kt.ksteps;
    std::vector<float> pad_s(co.cout_pad, 0.f), pad_b(co.cout_pad, 0.f);
    memcpy(pad_s.data(), scale, sizeof(float) * d->cout);
    memcpy(pad_b.data(), shift, sizeof(float) * d->cout);
    if (upload(c, &co.d_scale, pad_s.data(), pad_s.size()) || upload(c, &co.d_shift, pad_b.data(), pad_b.size())) return 1;
    if (d->raw_out_tensor >= 0) {
        REQUIRE(raw_scale && raw_shift, "raw output needs raw_scale/raw_shift");
        memcpy(pad_s.data(), raw_scale, sizeof(float) * d->cout);
        memcpy(pad_b.data(), raw_shift, sizeof(float) * d->cout);
        if (upload(c, &co.d_rscale, pad_s.data(), pad_s.size()) || upload(c, &co.d_rshift, pad_b.data(), pad_b.size())) return 1;
    }
    co.h_epi.assign(scale, scale + d->cout);
    co.h_epi.insert(co.h_epi.end(), shift, shift + d->cout);
    if (d->head_classes > 0) {
        co.h_epi.insert(co.h_epi.end(), head_w, head_w + (size_t)d->cout * d->head_classes);
        co.h_epi.insert(co.h_epi.end(), head_scale, head_scale + d->head_classes);
        co.h_epi.insert(co.h_epi.end(), head_shift, head_shift + d->head_classes);
    }
    if (d->head_classes > 0) {
        if (upload(c, &co.d_head_w, head_w, (size_t)d->cout * d->head_classes) ||
            upload(c, &co.d_head_scale, head_scale, d->head_classes) || upload(c, &co.d_head_shift, head_shift, d->head_classes))
            return 1;
        c->classes = d->head_classes;
        c->fused_heads += 1;
    }
    int cin_total = 0;
    for (int s = 0; s < d->n_src; ++s) cin_total += d->src[s].channels;
    char nm[128];
    snprintf(nm, sizeof(nm), "conv%dx%d_c%dto%d_%dx%d%s%s%s%s", d->src[0].kh, d->src[0].kw, cin_total, d->cout, d->out_h, d->out_w,
             d->n_src == 2 ? "_cat" : "", d->src[0].up_shift ? "_up" : "",
             (d->out_stride_y > 1 || d->out_stride_x > 1) ? (std::string("_par") + char('0' + d->out_off_y) + char('0' + d->out_off_x)).c_str() : "",
             d->head_classes > 0 ? "_head" : "");
    op.name = nm;
    const double macs = d->algorithmic_macs > 0 ? d->algorithmic_macs : (double)d->out_h * d->out_w * d->cout * geo_macs;
    op.flops = 2.0 * macs;
    op.issued_flops = 2.0 * d->out_h * d->out_w * d->cout * (double)co.total_ksteps * (split ? 32 * 3 : kBK);
    double bytes = 0;
    for (int s = 0; s < d->n_src; ++s) {
        const Tensor& t = c->tensors[d->src[s].tensor];
        bytes += (double)t.H * t.W * ((d->src[s].channels + 7) / 8 * 8) * c->elem * c->planes / (d->out_stride_y * d->out_stride_x);
    }
    const double ob = (double)d->out_h * d->out_w * d->cout * c->elem * c->planes;
    bytes += (d->out_tensor >= 0 ? ob : 0) + (d->raw_out_tensor >= 0 ? ob : 0) + (d->residual_tensor >= 0 ? ob : 0);
    op.min_bytes = bytes;
    co.d_w_cls[0] = co.d_w; co.d_kstep_cls[0] = co.d_kstep; co.d_ktab_cls[0] = co.d_ktab;
    co.ooy_cls[0] = d->out_off_y; co.oox_cls[0] = d->out_off_x;

    // the network stem (7 rows x 4 two-pixel granules on the PAIRS form -> 64 channels) has its own kernel
    {
        const sbbseg_conv_src& cs = d->src[0];
        const Tensor& st = c->tensors[cs.tensor];
        const bool plain16 = c->precision == kF16 || c->precision == kBF16;     // the dedicated kernels read the one-plane layout
        if ((plain16 || split) && d->n_src == 1 && st.is_input_form && st.form == SBBSEG_INPUT_PAIRS &&
            cs.channels == 8 && cs.kh == 7 && cs.kw == 4 && cs.stride_y == 2 && cs.stride_x == 1 && cs.pad_top == 0 && cs.pad_left == 0 &&
            cs.up_shift == 0 && cs.off_y == 0 && cs.off_x == 0 && d->cout == 64 && d->out_h % 16 == 0 && d->out_w % 16 == 0 &&
            st.H >= 2 * d->out_h + 5 && st.W >= d->out_w + 3 &&
            d->residual_tensor < 0 && d->raw_out_tensor < 0 && d->head_classes == 0 && d->out_tensor >= 0 && d->out_stride_y == 1 &&
            d->out_stride_x == 1 && d->out_off_y == 0 && d->out_off_x == 0 && TH == d->out_h && TW == d->out_w) {
            std::vector<uint16_t> frag;          // [7 ky][4 mi] fragments, k = the 4 two-pixel granules x 8 values of kernel row ky; split mode: hi block, lo block
            weight_frags(frag, c->precision, wpre, w_src0, 7 * 32, 64, false);
            if (upload(c, &co.d_stem_wfrag, frag)) return 1;
            op.name = "stem_" + op.name;
        }
        // 3x3 / stride 1 / pad 1, 64 -> 64 channels: direct conv on an LDS halo tile, weights in registers
        if ((plain16 || split) && d->n_src == 1 && !st.is_input_form && st.C == 64 && cs.channels == 64 &&
            cs.kh == 3 && cs.kw == 3 && cs.stride_y == 1 && cs.stride_x == 1 && cs.pad_top == 1 && cs.pad_left == 1 && cs.up_shift == 0 &&
            cs.off_y == 0 && cs.off_x == 0 && d->cout == 64 && d->out_h == st.H && d->out_w == st.W && d->residual_tensor < 0 &&
            d->raw_out_tensor < 0 && d->head_classes == 0 && d->out_tensor >= 0 && d->out_stride_y == 1 && d->out_stride_x == 1 &&
            d->out_off_y == 0 && d->out_off_x == 0 && TH == d->out_h && TW == d->out_w) {
            std::vector<uint16_t> frag;          // [9 taps][2 kk][4 mi] fragments, k = tap * 64 + input channel; split mode: hi block, lo block
            weight_frags(frag, c->precision, wpre, w_src0, 9 * 64, 64, false);
            if (upload(c, &co.d_d64_wfrag, frag)) return 1;
            op.name = "direct_" + op.name;
        }
        // small pointwise convs keep their weights on the host until sbbseg_finalize: candidates for bottleneck fusion
        bool pw = (plain16 || split) && d->head_classes == 0 && d->raw_out_tensor < 0 && (d->cout == 64 || d->cout == 256) && d->out_stride_y == 1 &&
                  d->out_stride_x == 1 && d->out_off_y == 0 && d->out_off_x == 0 && TH == d->out_h && TW == d->out_w;
        for (int s2 = 0; pw && s2 < d->n_src; ++s2) {
            const sbbseg_conv_src& q = d->src[s2];
            const Tensor& qt = c->tensors[q.tensor];
            pw = q.kh == 1 && q.kw == 1 && q.stride_y == 1 && q.stride_x == 1 && q.pad_top == 0 && q.pad_left == 0 && q.up_shift == 0 &&
                 q.off_y == 0 && q.off_x == 0 && (q.channels == 64 || q.channels == 256) && q.channels == qt.C && !qt.is_input_form &&
                 qt.H == d->out_h && qt.W == d->out_w;
        }
        if (pw) {
            co.h_w[0].assign(w_src0, w_src0 + (size_t)d->src[0].channels * d->cout);
            if (d->n_src == 2) co.h_w[1].assign(w_src1, w_src1 + (size_t)d->src[1].channels * d->cout);
        }
    }

    // Output-placement siblings (same sources, taps geometry and outputs, only padding / placement
    // offset / weights differ -- the parity classes of one decoder conv) run as ONE launch: bigger
    // grids (the 256x256 tiles become usable on the small-M layers) and 4x fewer launches.
    if (c->precision != kF32 && !c->ops.empty() && c->ops.back().type == kConv && !(c->conv_variant & 16)) {
        Op& prev = c->ops.back();
        ConvOp& pc = prev.conv;
        bool same = pc.n_cls < 4 && pc.d.n_src == d->n_src && pc.d.cout == d->cout && pc.d.out_tensor == d->out_tensor &&
                    pc.d.relu == d->relu && pc.d.residual_tensor < 0 && d->residual_tensor < 0 && pc.d.raw_out_tensor < 0 &&
                    d->raw_out_tensor < 0 && pc.d.out_h == d->out_h && pc.d.out_w == d->out_w &&
                    pc.d.out_stride_y == d->out_stride_y && pc.d.out_stride_x == d->out_stride_x &&
                    (d->out_stride_y > 1 || d->out_stride_x > 1) && pc.d.head_classes == d->head_classes &&
                    pc.total_ksteps == co.total_ksteps && pc.ksteps[0] == co.ksteps[0] &&
                    pc.h_epi == co.h_epi;       // the merged launch applies class 0's BN / head constants to every class
        for (int s = 0; same && s < d->n_src; ++s) {
            const sbbseg_conv_src &x = pc.d.src[s], &y = d->src[s];
            same = x.tensor == y.tensor && x.channels == y.channels && x.kh == y.kh && x.kw == y.kw && x.stride_y == y.stride_y &&
                   x.stride_x == y.stride_x && x.up_shift == y.up_shift && x.off_y == y.off_y && x.off_x == y.off_x;
        }
        if (same) {
            const int q = pc.n_cls++;
            pc.fg_ok = pc.fg_ok && co.fg_ok;
            pc.h_ksteps_cls[q] = co.h_ksteps_cls[0];
            for (int s2 = 0; s2 < 2; ++s2)
                for (int a = 0; a < 2; ++a) {
                    pc.tap_lo[s2][a] = std::min(pc.tap_lo[s2][a], co.tap_lo[s2][a]);
                    pc.tap_hi[s2][a] = std::max(pc.tap_hi[s2][a], co.tap_hi[s2][a]);
                }
            pc.d_w_cls[q] = co.d_w; pc.d_kstep_cls[q] = co.d_kstep; pc.d_ktab_cls[q] = co.d_ktab;
            pc.ooy_cls[q] = d->out_off_y; pc.oox_cls[q] = d->out_off_x; pc.wmul_cls[q] = co.wmul_cls[0];
            for (void* p : {(void*)co.d_scale, (void*)co.d_shift, (void*)co.d_head_w, (void*)co.d_head_scale, (void*)co.d_head_shift})
                (void)c->mem.release(p);         // (class 0's serve)
            uploads.commit();
            prev.flops += op.flops;
            prev.issued_flops += op.issued_flops;
            prev.min_bytes += op.min_bytes;
            const size_t pos = prev.name.find("_par");
            if (pos != std::string::npos) prev.name = prev.name.substr(0, pos) + "_par4" + (d->head_classes > 0 ? "_head" : "");
            return 0;
        }
    }
    c->ops.push_back(op);
    uploads.commit();
    return 0;
    API_END
}

int sbbseg_add_maxpool(sbbseg_ctx* c, int src_tensor, int dst_tensor, int k, int stride, const float* pre_scale,
                       const float* pre_shift, int pre_relu)
{
    API_BEGIN
    REQUIRE(c && !c->finalized, "bad handle / already finalized");
    const int ntens = (int)c->tensors.size();
    REQUIRE(src_tensor >= 0 && src_tensor < ntens && dst_tensor >= 0 && dst_tensor < ntens, "maxpool tensors undefined");
    const Tensor& s = c->tensors[src_tensor];
    const Tensor& t = c->tensors[dst_tensor];
    const int Ho = (s.H - k) / stride + 1, Wo = (s.W - k) / stride + 1;
    REQUIRE(t.H == Ho && t.W == Wo && t.C == s.C, "maxpool output should be %dx%dx%d", Ho, Wo, s.C);
    AllocScope uploads(c->mem);
    Op op;
    op.type = kPool;
    op.pool.src = src_tensor; op.pool.dst = dst_tensor; op.pool.k = k; op.pool.stride = stride; op.pool.Ho = Ho; op.pool.Wo = Wo;
    if (pre_scale) {
        REQUIRE(pre_shift, "pre_scale needs pre_shift");
        HIPCHK(hipSetDevice(c->device));
        if (upload(c, &op.pool.d_pre_scale, pre_scale, s.C) || upload(c, &op.pool.d_pre_shift, pre_shift, s.C)) return 1;
        op.pool.pre_relu = pre_relu;
    }
    char nm[64];
    snprintf(nm, sizeof(nm), "maxpool%dx%d_s%d_c%d_%dx%d", k, k, stride, s.C, Ho, Wo);
    op.name = nm;
    op.flops = 0;
    op.min_bytes = ((double)s.H * s.W + (double)Ho * Wo) * s.C * c->elem * c->planes;
    c->ops.push_back(op);
    uploads.commit();
    return 0;
    API_END
}

int sbbseg_add_tail(sbbseg_ctx* c, int src0_tensor, int img_c8_tensor, const float* w_src0, const float* w_img,
                    const float* scale, const float* shift, int classes, const float* head_w, const float* head_scale,
                    const float* head_shift, double algorithmic_macs)
{
    API_BEGIN
    REQUIRE(c && !c->finalized && w_src0 && w_img && scale && shift && head_w && head_scale && head_shift, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    REQUIRE(c->precision == kF16 || c->precision == kBF16 || c->precision == kF16X3, "the fused tail is a 16-bit-mode kernel");
    const bool split = c->precision == kF16X3;
    const int ntens = (int)c->tensors.size();
    REQUIRE(src0_tensor >= 0 && src0_tensor < ntens && img_c8_tensor >= 0 && img_c8_tensor < ntens, "tail tensors undefined");
    const Tensor& s0 = c->tensors[src0_tensor];
    const Tensor& im = c->tensors[img_c8_tensor];
    REQUIRE(s0.C == 64, "fused tail needs a 64-channel upsampled source (got %d)", s0.C);
    REQUIRE(im.is_input_form && im.form == SBBSEG_INPUT_C8, "fused tail needs the C8 input form as second source");
    REQUIRE(2 * s0.H == c->in_H && 2 * s0.W == c->in_W && c->in_H % 16 == 0 && c->in_W % 16 == 0, "fused tail: geometry");
    REQUIRE(classes >= 1 && classes <= 4 && c->classes == 0, "fused tail: 1..4 classes, one head per plan");
    const int CO = 32, KS = split ? kTailSplitKSteps : kTailKSteps;
    // pre-summed fp32 weights first; then 16-bit (plain modes) or hi | lo after the power-of-two pre-scale, scale divided by the pre-scale
    // (see sbbseg_add_conv)
    const std::vector<float> pre = tail_presum(split, w_src0, w_img);
    std::vector<float> scale_v(scale, scale + CO);
    float wpre = 1.f;
    if (split) {
        const float wmax = max_abs(pre.data(), pre.size());
        REQUIRE(std::isfinite(wmax), "%s: non-finite weights", "tail");
        wpre = split_prescale(wmax);
        for (float& v : scale_v) v /= wpre;
    }
    AllocScope uploads(c->mem);
    Op op;
    op.type = kTail;
    op.tail.src0 = src0_tensor; op.tail.img = img_c8_tensor; op.tail.classes = classes;
    std::vector<uint16_t> frag;                  // per class [KS][2 kk][2 mi] fragments; split mode: per class hi block, lo block
    for (int q = 0; q < 4; ++q) weight_frags(frag, c->precision, wpre, &pre[(size_t)q * KS * 64 * CO], KS * 64, CO, false);
    if (upload(c, (uint16_t**)&op.tail.d_wfrag, frag) || upload(c, &op.tail.d_scale, scale_v.data(), CO) ||
        upload(c, &op.tail.d_shift, shift, CO) || upload(c, &op.tail.d_head_w, head_w, (size_t)CO * classes) ||
        upload(c, &op.tail.d_head_scale, head_scale, classes) || upload(c, &op.tail.d_head_shift, head_shift, classes))
        return 1;
    char nm[96];
    snprintf(nm, sizeof(nm), "tail_conv3x3_c67to32_up_cat_head%d_%dx%d", classes, c->in_H, c->in_W);
    op.name = nm;
    op.flops = 2.0 * (algorithmic_macs > 0 ? algorithmic_macs : (double)c->in_H * c->in_W * CO * (9.0 * 67 + classes));
    op.issued_flops = 2.0 * c->in_H * c->in_W * CO * (double)(KS * kBK) * (split ? 3 : 1);
    op.min_bytes = (double)s0.H * s0.W * 64 * c->elem * c->planes + (double)c->in_H * c->in_W * (8 * c->elem * c->planes + 1);
    c->classes = classes;
    c->ops.push_back(op);
    uploads.commit();
    return 0;
    API_END
}

int sbbseg_add_head(sbbseg_ctx* c, int src_tensor, int cin, int classes, const float* w, const float* scale,
                    const float* shift)
{
    API_BEGIN
    REQUIRE(c && !c->finalized && w && scale && shift, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    REQUIRE(src_tensor >= 0 && src_tensor < (int)c->tensors.size(), "head source undefined");
    const Tensor& s = c->tensors[src_tensor];
    REQUIRE(cin == s.C && cin <= 64, "head cin %d must equal the source channels (%d) and be <= 64", cin, s.C);
    REQUIRE(classes >= 1 && classes <= 8, "head supports 1..8 classes (got %d)", classes);
    REQUIRE(s.H == c->in_H && s.W == c->in_W, "head runs at input resolution");
    REQUIRE(c->classes == 0, "plan already has a head");
    AllocScope uploads(c->mem);
    Op op;
    op.type = kHead;
    op.head.src = src_tensor; op.head.cin = cin; op.head.classes = classes;
    if (upload(c, &op.head.d_w, w, (size_t)cin * classes) || upload(c, &op.head.d_scale, scale, classes) ||
        upload(c, &op.head.d_shift, shift, classes))
        return 1;
    char nm[64];
    snprintf(nm, sizeof(nm), "head1x1_c%dto%d_softmax_argmax", cin, classes);
    op.name = nm;
    op.flops = 2.0 * s.H * s.W * cin * classes;
    op.issued_flops = 0;           // plain FMA kernel, no MFMA
    op.min_bytes = (double)s.H * s.W * (cin * c->elem * c->planes + 1);
    c->classes = classes;
    c->ops.push_back(op);
    uploads.commit();
    return 0;
    API_END
}

// ---- fast gather tables (conv_igemm_mfma<..., FG>): for every conv whose K-steps are all regular, whose sources are not
// upsampled and whose taps span at most 4 x 4 offsets per source (over all merged classes), one FgStepRec per K-step.
// Short-K layers keep the plain gather (the per-tile mask set-up costs them 1-10 %; from ~9 K-steps on the fast gather
// wins 2-10 %, profiles/r02_experiments.md), and so do the split mode's 64-channel tiles (+13 % time there).
static int build_fast_gather_tables(sbbseg_ctx* c)
{
    if (const char* e = getenv("SBBSEG_FG_POINTWISE_MIN")) c->fg_pointwise_min_ksteps = atoi(e);
    if (const char* e = getenv("SBBSEG_FG_MIN")) c->fg_min_ksteps = atoi(e);
    std::vector<ConvOp*> convs;
    for (Op& op : c->ops) {
        if (op.type == kConv) convs.push_back(&op.conv);
        for (Op& part : op.parts)
            if (part.type == kConv) convs.push_back(&part.conv);
    }
    for (ConvOp* cop : convs) {
        ConvOp& co = *cop;
        bool pointwise = true;                             // every tap (0, 0): no bounds masks to set up
        for (int s = 0; s < co.d.n_src; ++s)
            pointwise = pointwise && co.tap_lo[s][0] == 0 && co.tap_hi[s][0] == 0 && co.tap_lo[s][1] == 0 && co.tap_hi[s][1] == 0 &&
                        co.d.src[s].pad_top == 0 && co.d.src[s].pad_left == 0 && co.d.src[s].off_y == 0 && co.d.src[s].off_x == 0;
        co.fg_pointwise = pointwise;
        const int min_ksteps = pointwise ? c->fg_pointwise_min_ksteps : c->fg_min_ksteps;
        // fast gather on the split mode's 64-channel tiles too: +13 % time under round 2's [C hi][C lo] layout, -11 % (dec4 3.25 ->
        // 2.89 ms) with the interleaved groups of round 3; SBBSEG_FG_X3_SMALL=0 turns it off (A/B)
        static const bool x3_small = !(getenv("SBBSEG_FG_X3_SMALL") && getenv("SBBSEG_FG_X3_SMALL")[0] == '0');
        if (!co.fg_ok || c->precision == kF32 || co.total_ksteps < min_ksteps || (c->precision == kF16X3 && co.d.cout < 128 && !x3_small)) continue;
        bool ok = true;
        for (int s = 0; s < co.d.n_src; ++s)
            ok = ok && co.d.src[s].up_shift == 0 && co.tap_hi[s][0] - co.tap_lo[s][0] <= 3 && co.tap_hi[s][1] - co.tap_lo[s][1] <= 3 &&
                 co.tap_lo[s][0] >= -8 && co.tap_lo[s][1] >= -8;
        if (!ok) continue;
        for (int q = 0; q < co.n_cls; ++q) {
            const std::vector<KStepRec>& ks = co.h_ksteps_cls[q];
            std::vector<FgStepRec> fg(ks.size());
            for (size_t t = 0; t < ks.size(); ++t) {
                const int s = (int)t < co.ksteps[0] ? 0 : 1;
                const Tensor& tt = c->tensors[co.d.src[s].tensor];
                const long pixb = (long)tt.C * c->elem * c->planes, rowb = (long)tt.W * pixb;
                const long soff = ks[t].dy * rowb + ks[t].dx * pixb + ks[t].coff + (long)kFgBiasPixels(tt.W) * pixb;
                REQUIRE(soff >= 0 && soff < ((long)1 << 31), "fast gather: scalar offset out of range");
                fg[t].soff = (uint32_t)soff;
                fg[t].tapbit = s * 16 + (ks[t].dy - co.tap_lo[s][0]) * 4 + (ks[t].dx - co.tap_lo[s][1]);
                fg[t].pad_[0] = fg[t].pad_[1] = 0;
            }
            if (upload(c, &co.d_fgstep_cls[q], fg.data(), fg.size())) return 1;
        }
    }
    return 0;
}

// how many ops of the plan read `tensor` (a fused block reads its input; its parts' tensors are internal to it)
static int readers(const sbbseg_ctx* c, int tensor)
{
    int nrd = 0;
    for (const Op& o : c->ops) {
        if (o.type == kConv) {
            for (int s = 0; s < o.conv.d.n_src; ++s) nrd += o.conv.d.src[s].tensor == tensor;
            nrd += o.conv.d.residual_tensor == tensor;
        } else if (o.type == kPool) nrd += o.pool.src == tensor;
        else if (o.type == kHead) nrd += o.head.src == tensor;
        else if (o.type == kTail) nrd += (o.tail.src0 == tensor) + (o.tail.img == tensor);
        else if (o.type == kBlock) nrd += o.block.x_tensor == tensor;
    }
    return nrd;
}

// ---- bottleneck fusion: [1x1 CIN->64, ReLU] -> [3x3 64->64 direct, ReLU] -> [1x1 -> 256 (+ shortcut), ReLU] at one resolution,
// the two 64-channel tensors in between read by nobody else  ==>  one kBlock op (bottleneck_fused).  The three convs
// stay alive as its parts.  SBBSEG_FUSE_BLOCKS=0 keeps the plan unfused (per-layer tests read the intermediate tensors).
static int fuse_bottlenecks(sbbseg_ctx* c)
{
    const char* env = getenv("SBBSEG_FUSE_BLOCKS");
    const bool split = c->precision == kF16X3;
    if ((env && env[0] == '0') || !(c->precision == kF16 || c->precision == kBF16 || split)) return 0;
    for (size_t i = 0; i + 2 < c->ops.size(); ++i) {
        if (c->ops[i].type != kConv || c->ops[i + 1].type != kConv || c->ops[i + 2].type != kConv) continue;
        const ConvOp &A = c->ops[i].conv, &B = c->ops[i + 1].conv, &C = c->ops[i + 2].conv;
        if (A.h_w[0].empty() || C.h_w[0].empty() || !B.d_d64_wfrag) continue;
        if (A.d.n_src != 1 || A.d.cout != 64 || !A.d.relu || A.d.residual_tensor >= 0 || A.n_cls != 1 || !B.d.relu || !C.d.relu || C.d.cout != 256 ||
            C.n_cls != 1 || A.d.out_tensor < 0 || B.d.out_tensor < 0 || C.d.out_tensor < 0)
            continue;
        const int X = A.d.src[0].tensor, T1 = A.d.out_tensor, T2 = B.d.out_tensor, cin = A.d.src[0].channels;
        if (B.d.src[0].tensor != T1 || readers(c, T1) != 1 || readers(c, T2) != 1 || T1 == X || T2 == X || C.d.out_tensor == X) continue;
        int proj = -1, b_src = 0;
        if (C.d.n_src == 1 && C.d.src[0].tensor == T2 && C.d.residual_tensor == X && cin == 256) proj = 0;
        else if (C.d.n_src == 2 && C.d.residual_tensor < 0 && cin == 64 &&
                 ((C.d.src[0].tensor == T2 && C.d.src[1].tensor == X) || (C.d.src[1].tensor == T2 && C.d.src[0].tensor == X))) {
            proj = 1;
            b_src = C.d.src[0].tensor == T2 ? 0 : 1;
        }
        if (proj < 0) continue;
        const Tensor& xt = c->tensors[X];
        Op blk;
        blk.type = kBlock;
        blk.block.x_tensor = X; blk.block.out_tensor = C.d.out_tensor; blk.block.cin = cin; blk.block.proj = proj;
        blk.block.H = xt.H; blk.block.W = xt.W;
        // W1 / W3 as MFMA A fragments.  Split mode: each conv's own power-of-two pre-scale (ConvOp::wmul_cls[0] = 2^-s), and W3 in the conv's
        // own K order, source 0, then source 1 (block_x3 adds up the same way); plain modes: b's K-steps first, then the block input's
        const int first = split ? 0 : b_src;
        std::vector<uint16_t> f1, f3;        // W1 [cin / 32 kk][4 mi], W3 [2 | 4 kk][16 mi] fragments; split mode: [kk][mi][hi | lo]
        weight_frags(f1, c->precision, 1.f / A.wmul_cls[0], A.h_w[0].data(), cin, 64, true);
        weight_frags(f3, c->precision, 1.f / C.wmul_cls[0], C.h_w[first].data(), 64, 256, true);
        if (proj) weight_frags(f3, c->precision, 1.f / C.wmul_cls[0], C.h_w[1 - first].data(), 64, 256, true);
        if (split) {
            blk.block.wmul[0] = A.wmul_cls[0]; blk.block.wmul[1] = B.wmul_cls[0]; blk.block.wmul[2] = C.wmul_cls[0];
            if (proj) blk.block.proj = b_src == 0 ? 1 : 2;         // 1: K order [b, x]; 2: [x, b]
        }
        if (upload(c, &blk.block.d_w1, f1) || upload(c, &blk.block.d_w3, f3)) return 1;
        char nm[96];
        snprintf(nm, sizeof(nm), "block%s_c%dto64to256_%dx%d", proj ? "_proj" : "", cin, xt.H, xt.W);
        blk.name = nm;
        for (int k = 0; k < 3; ++k) {
            blk.flops += c->ops[i + k].flops;
            blk.issued_flops += c->ops[i + k].issued_flops;
        }
        blk.min_bytes = (double)xt.H * xt.W * (cin + 256) * c->elem * c->planes;        // x read once, y written once
        blk.parts.assign(c->ops.begin() + i, c->ops.begin() + i + 3);
        c->ops.erase(c->ops.begin() + i, c->ops.begin() + i + 3);
        c->ops.insert(c->ops.begin() + i, std::move(blk));
    }
    return 0;
}

// ---- owned-region chain (region.h): the fused tail and, below it, every decoder conv of the form
//   four output-parity classes of conv3x3([nearest-x2 upsampling of the level below, skip]) -> this level
// whose output is read by the level above only.  Level 0 = the tail (network output), level k = the conv k steps below.  A level's rows
// are the rows above dilated by one and halved (region_down), which is exact when class (py, px) reads rows {py - 1, py} / columns
// {px - 1, px} of the level below -- checked here on the K-step records; anything else (unfused heads, fp32 handles, Conv2DTranspose
// decoders whose classes read other taps) leaves the chain short or empty and those ops run whole.
static void find_region_chain(sbbseg_ctx* c)
{
    c->region_levels = 0;
    for (auto& op : c->ops) op.region_level = -1;
    if (c->precision == kF32 || c->ops.empty() || c->ops.back().type != kTail) return;
    if (c->max_batch > kRegionMaxPatches || c->in_H > 2 * kRegionMaxCoord || c->in_W > 2 * kRegionMaxCoord || (c->in_H & 15) || (c->in_W & 15)) return;
    int level = 0;
    c->region_op[0] = (int)c->ops.size() - 1;
    c->ops.back().region_level = 0;
    int below = c->ops.back().tail.src0;              // the tensor the level above upsamples
    {
        const Tensor& t = c->tensors[below];
        if (2 * t.H != c->in_H || 2 * t.W != c->in_W) { c->ops.back().region_level = -1; return; }
    }
    c->region_levels = 1;
    while (level + 1 < kRegionMaxLevels) {
        int oi = -1;
        for (size_t i = 0; i < c->ops.size(); ++i)
            if (c->ops[i].type == kConv && c->ops[i].conv.d.out_tensor == below) oi = oi < 0 ? (int)i : -2;
        if (oi < 0 || readers(c, below) != 1) break;
        const ConvOp& co = c->ops[oi].conv;
        const sbbseg_conv_desc& d = co.d;
        const Tensor& to = c->tensors[below];
        if (co.n_cls != 4 || d.n_src != 2 || d.out_stride_y != 2 || d.out_stride_x != 2 || d.residual_tensor >= 0 || d.raw_out_tensor >= 0 ||
            d.head_classes > 0 || d.src[0].stride_y != 1 || d.src[0].stride_x != 1 || d.src[0].up_shift != 0 || d.src[0].off_y || d.src[0].off_x ||
            to.H != 2 * co.Ho || to.W != 2 * co.Wo || co.TH != to.H || co.TW != to.W || !co.fg_ok)
            break;
        const Tensor& t0 = c->tensors[d.src[0].tensor];
        if (t0.H != co.Ho || t0.W != co.Wo || t0.is_input_form) break;
        bool ok = true;
        int seen = 0;
        for (int q = 0; q < 4 && ok; ++q) {
            const int py = co.ooy_cls[q], px = co.oox_cls[q];
            ok = (py == 0 || py == 1) && (px == 0 || px == 1);
            seen |= 1 << (py * 2 + px);
            const int ks0 = co.ksteps[0];
            ok = ok && (int)co.h_ksteps_cls[q].size() >= ks0;
            for (int t = 0; t < ks0 && ok; ++t) {
                const KStepRec& r = co.h_ksteps_cls[q][t];
                ok = !r.irregular && (r.dy == py - 1 || r.dy == py) && (r.dx == px - 1 || r.dx == px);
            }
        }
        if (!ok || seen != 15) break;
        ++level;
        c->region_op[level] = oi;
        c->ops[oi].region_level = level;
        c->region_levels = level + 1;
        below = d.src[0].tensor;
    }
}

// split mode: the decoder conv at 224 x 224 -- four merged parity classes of  conv3x3([up2(128 ch @ 112 x 112), 64 ch @ 224 x 224]) -> 64 ch
// -- runs dec_halo_x3 (source halos resident in LDS, dec_halo_x3.hip) on the classes' OWN packed weights and K-step order:
// the rows of every class matrix are read back and re-laid as MFMA A fragments.  Conv-variant bit 23 keeps the generic kernel.
static int attach_dec_halo_tables(sbbseg_ctx* c)
{
    // (plain fp16 mode: dec_halo_f16.hip -- K-steps of 64 channels: 2 x 4 + 9 of them, fragments of the two k-halves in place of hi | lo)
    const bool x3 = c->precision == kF16X3;
    const int n0 = x3 ? 16 : 8, n1 = x3 ? 18 : 9, nsteps = n0 + n1;
    for (size_t i = 0; (x3 || c->precision == kF16) && i < c->ops.size(); ++i) {
        Op& op = c->ops[i];
        if (op.type != kConv) continue;
        ConvOp& co = op.conv;
        const sbbseg_conv_desc& d = co.d;
        if (co.n_cls != 4 || d.n_src != 2 || d.cout != 64 || co.ksteps[0] != n0 || co.ksteps[1] != n1 || !co.fg_ok || d.residual_tensor >= 0 ||
            d.raw_out_tensor >= 0 || d.head_classes > 0 || d.out_tensor < 0 || d.out_stride_y != 2 || d.out_stride_x != 2)
            continue;
        const Tensor &t0 = c->tensors[d.src[0].tensor], &t1 = c->tensors[d.src[1].tensor], &to = c->tensors[d.out_tensor];
        if (t0.C != 128 || d.src[0].channels != 128 || t1.C != 64 || d.src[1].channels != 64 || d.src[0].stride_y != 1 || d.src[0].stride_x != 1 ||
            d.src[0].up_shift != 0 || d.src[1].stride_y != 2 || d.src[1].stride_x != 2 || t0.is_input_form || t1.is_input_form ||
            t1.H != 2 * t0.H || t1.W != 2 * t0.W || to.H != t1.H || to.W != t1.W || d.out_h != t0.H || d.out_w != t0.W || (t0.H & 7) || (t0.W & 7))
            continue;
        // class q must be the output parity (q >> 1, q & 1) -- the kernel's wave <-> class map -- and its taps must stay inside the halos
        bool ok = true;
        std::vector<int> taps(4 * 16, 0);
        for (int q = 0; q < 4 && ok; ++q) {
            ok = co.ooy_cls[q] == (q >> 1) && co.oox_cls[q] == (q & 1) && (int)co.h_ksteps_cls[q].size() == nsteps;
            for (int t = 0; t < nsteps && ok; ++t) {
                const KStepRec& r = co.h_ksteps_cls[q][t];
                const int g = t < n0 ? t >> 2 : (t - n0) / 9, ti = t < n0 ? t & 3 : (t - n0) % 9;
                ok = !r.irregular && r.coff == g * 128;                                   // channel group g of the stored pixel
                if (t < n0) ok = ok && r.dy >= -1 && r.dy <= 1 && r.dx >= -1 && r.dx <= 1;             // halo row i + dy + 1 in [0, 9]
                else ok = ok && r.dy >= -1 && r.dy <= 2 && r.dx >= -1 && r.dx <= 2;                    // halo row 2 i + dy + 1 in [0, 17]
                const int word = (r.dy & 255) | ((r.dx & 255) << 8);
                const int slot = q * 16 + (t < n0 ? ti : 4 + ti);
                if (g == 0) taps[slot] = word;
                else ok = ok && taps[slot] == word;                                       // every group walks the same taps
            }
        }
        if (!ok) continue;
        alloc_check();
        std::vector<uint16_t> mat((size_t)64 * co.Ktot), frag;         // [4 classes][K-steps][4 row blocks][hi | lo] fragments
        for (int q = 0; q < 4; ++q) {
            HIPCHK(hipMemcpy(mat.data(), co.d_w_cls[q], mat.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));     // packed rows 0..63
            matrix_frags(frag, mat.data(), co.Ktot, 0, 4, nsteps);
        }
        if (upload(c, &co.d_halo_wfrag, frag) || upload(c, &co.d_halo_taps, taps)) return 1;
    }
    return 0;
}

// split and plain fp16 modes, encoder stages 3 / 4: an identity block's last 1x1 conv (C -> 4C, + residual, ReLU) directly followed by the next block's
// first 1x1 conv (4C -> C, stride 1, ReLU) -> one launch writes both outputs (expand_reduce_x3.hip: y is contracted from LDS instead
// of being read back).  Both matrices are read back and re-laid as MFMA A fragments.  Conv-variant bit 24 keeps two launches.
static int fuse_expand_reduce(sbbseg_ctx* c)
{
    const bool x3 = c->precision == kF16X3;
    const int kch = x3 ? 32 : 64;                                  // channels per K-step (plain fp16: two k-halves in place of hi | lo)
    auto pointwise = [&](const ConvOp& co, int cin, int cout) -> bool {
        const sbbseg_conv_desc& d = co.d;
        if (co.n_cls != 1 || d.n_src != 1 || d.cout != cout || d.src[0].channels != cin || d.src[0].kh != 1 || d.src[0].kw != 1 ||
            d.src[0].stride_y != 1 || d.src[0].stride_x != 1 || d.src[0].pad_top || d.src[0].pad_left || d.src[0].up_shift || d.src[0].off_y ||
            d.src[0].off_x || !d.relu || d.raw_out_tensor >= 0 || d.head_classes > 0 || d.out_tensor < 0 || d.out_stride_y != 1 || d.out_stride_x != 1 ||
            d.out_off_y || d.out_off_x || co.d_stem_wfrag || co.d_d64_wfrag || co.d_halo_wfrag || co.total_ksteps != cin / kch ||
            co.Ktot != cin * (x3 ? 2 : 1) || co.cout_pad < cout || (int)co.h_ksteps_cls[0].size() != cin / kch)
            return false;
        const Tensor& t = c->tensors[d.src[0].tensor];
        if (t.C != cin || t.is_input_form || t.H != d.out_h || t.W != d.out_w) return false;
        for (int k = 0; k < cin / kch; ++k) {
            const KStepRec& r = co.h_ksteps_cls[0][k];
            if (r.irregular || r.dy || r.dx || r.coff != k * 128) return false;     // K-step k = channel group k of the stored pixel
        }
        return true;
    };
    for (size_t i = 0; (x3 || c->precision == kF16) && i + 1 < c->ops.size(); ++i) {
        if (c->ops[i].type != kConv || c->ops[i + 1].type != kConv) continue;
        ConvOp& e = c->ops[i].conv;
        ConvOp& r = c->ops[i + 1].conv;
        const int C = e.d.src[0].channels;
        if ((C != 128 && C != 256) || !pointwise(e, C, 4 * C) || !pointwise(r, 4 * C, C)) continue;
        if (e.d.residual_tensor < 0 || r.d.residual_tensor >= 0 || r.d.src[0].tensor != e.d.out_tensor || c->ops[i].absorbed_by >= 0) continue;
        const Tensor &tx = c->tensors[e.d.residual_tensor], &ty = c->tensors[e.d.out_tensor], &ta = c->tensors[r.d.out_tensor];
        if (tx.C != 4 * C || tx.H != ty.H || tx.W != ty.W || ty.C != 4 * C || ty.H != e.d.out_h || ty.W != e.d.out_w || ta.C != C ||
            ta.H != ty.H || ta.W != ty.W || tx.is_input_form)
            continue;
        alloc_check();
        std::vector<uint16_t> m3((size_t)e.cout_pad * e.Ktot), m1((size_t)r.cout_pad * r.Ktot);
        HIPCHK(hipMemcpy(m3.data(), e.d_w, m3.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(m1.data(), r.d_w, m1.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
        // expand: [4C / 256 chunks][C / kch K-steps][8 waves x 2 row blocks][hi | lo] -- a chunk is 256 rows;
        // reduce: [4C / 256 chunks x 256 / kch K-steps][8 waves x C / 128 row blocks][hi | lo] -- chunk j contracts y channels 256 j ..
        std::vector<uint16_t> f3, f1;
        for (int j = 0; j < C / 64; ++j) matrix_frags(f3, m3.data(), e.Ktot, j * 16, 16, C / kch);
        matrix_frags(f1, m1.data(), r.Ktot, 0, C / 16, 4 * C / kch);
        if (upload(c, &e.d_er_w3, f3) || upload(c, &e.d_er_w1, f1)) return 1;
        e.fused_reduce = (int)(i + 1);
        c->ops[i + 1].absorbed_by = (int)i;
    }
    return 0;
}

// Round 6, stage 3 (C = 128; H, W multiples of 8): the identity block's 3x3 conv in front of such a pair joins the launch
// (conv3_expand_reduce.hip: b stays in LDS).  The conv's packed rows are re-laid as A fragments in ITS K-step order, the taps and
// channel groups of the K-steps go along as a table.  Conv-variant bit 25 keeps the 3x3 conv's own launch.
static int fuse_conv3_expand_reduce(sbbseg_ctx* c)
{
    const bool x3 = c->precision == kF16X3;
    const int kch = x3 ? 32 : 64;                                  // channels per K-step, as in fuse_expand_reduce
    const char* envfb = getenv("SBBSEG_FUSE_BLOCKS");          // (= 0: "keep every plan tensor materialised" -- the per-layer tests; b would not be)
    const bool c3er = !(envfb && envfb[0] == '0');
    for (size_t i = 1; (x3 || c->precision == kF16) && c3er && i < c->ops.size(); ++i) {
        if (c->ops[i].type != kConv || c->ops[i - 1].type != kConv) continue;
        ConvOp& e = c->ops[i].conv;
        ConvOp& k3 = c->ops[i - 1].conv;
        if (e.fused_reduce < 0) continue;
        const int C = e.d.src[0].channels;
        const sbbseg_conv_desc& d = k3.d;
        const int ks0 = 9 * C / kch;
        if (C != 128 || k3.n_cls != 1 || d.n_src != 1 || d.cout != C || d.src[0].channels != C || d.src[0].kh != 3 || d.src[0].kw != 3 ||
            d.src[0].stride_y != 1 || d.src[0].stride_x != 1 || d.src[0].pad_top != 1 || d.src[0].pad_left != 1 || d.src[0].up_shift || d.src[0].off_y ||
            d.src[0].off_x || !d.relu || d.residual_tensor >= 0 || d.raw_out_tensor >= 0 || d.head_classes > 0 || d.out_tensor != e.d.src[0].tensor ||
            d.out_stride_y != 1 || d.out_stride_x != 1 || d.out_off_y || d.out_off_x || k3.d_stem_wfrag || k3.d_d64_wfrag || k3.d_halo_wfrag ||
            c->ops[i - 1].absorbed_by >= 0 || k3.fused_reduce >= 0 || k3.total_ksteps != ks0 || k3.Ktot != ks0 * 64 || k3.cout_pad < C ||
            (int)k3.h_ksteps_cls[0].size() != ks0 || readers(c, d.out_tensor) != 1)
            continue;
        const Tensor &ta = c->tensors[d.src[0].tensor], &tb = c->tensors[d.out_tensor];
        if (ta.C != C || ta.is_input_form || ta.H != d.out_h || ta.W != d.out_w || tb.H != ta.H || tb.W != ta.W || (ta.H & 7) || (ta.W & 7)) continue;
        std::vector<int> k0(ks0);
        bool ok = true;
        for (int t = 0; t < ks0 && ok; ++t) {
            const KStepRec& r = k3.h_ksteps_cls[0][t];
            ok = !r.irregular && r.dy >= -1 && r.dy <= 1 && r.dx >= -1 && r.dx <= 1 && r.coff >= 0 && r.coff % 128 == 0 && r.coff / 128 < C / kch;
            k0[t] = (r.dy & 255) | ((r.dx & 255) << 8) | ((r.coff / 128) << 16);
        }
        if (!ok) continue;
        alloc_check();
        std::vector<uint16_t> m2((size_t)k3.cout_pad * k3.Ktot);
        HIPCHK(hipMemcpy(m2.data(), k3.d_w, m2.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
        std::vector<uint16_t> f2;                // [ks0 K-steps][8 waves x C / 128 row blocks][hi | lo]
        matrix_frags(f2, m2.data(), k3.Ktot, 0, C / 16, ks0);
        if (upload(c, &e.d_c3_w2, f2) || upload(c, &e.d_c3_k0, k0)) return 1;
        e.fused_conv3 = (int)(i - 1);
        c->ops[i - 1].absorbed_by = (int)i;
    }
    return 0;
}

// split and plain fp16 modes: the stem (dedicated kernel, raw output only) directly followed by the 3x3 / stride-2 max-pool of that tensor with an
// affine on every tap (bn_conv1 + ReLU) -> one launch writes both tensors (stem_pool_x3.hip); conv-variant bit 22 keeps two launches
static void fuse_stem_pool(sbbseg_ctx* c)
{
    // (plain fp16 mode: the one-plane form stem_pool<false> is bit-identical too but no faster than the two launches -- 0.53 against
    // 0.26 + 0.29 ms per 140 patches: with one MFMA per product the pool stage is most of the kernel -- so it is opt-in: SBBSEG_STEM_POOL_F16=1)
    const char* env16 = getenv("SBBSEG_STEM_POOL_F16");
    const bool on = c->precision == kF16X3 || (c->precision == kF16 && env16 && env16[0] == '1');
    for (size_t i = 0; on && i + 1 < c->ops.size(); ++i) {
        Op& a = c->ops[i];
        Op& b = c->ops[i + 1];
        if (a.type != kConv || !a.conv.d_stem_wfrag || b.type != kPool) continue;
        const PoolOp& po = b.pool;
        const Tensor& f1 = c->tensors[a.conv.d.out_tensor];
        if (po.src != a.conv.d.out_tensor || po.k != 3 || po.stride != 2 || !po.d_pre_scale || f1.C != 64 || (f1.H & 15) || (f1.W & 15) ||
            po.Ho != f1.H / 2 - 1 || po.Wo != f1.W / 2 - 1)
            continue;
        a.conv.fused_pool = (int)(i + 1);
        b.absorbed_by = (int)i;
    }
}

int sbbseg_finalize(sbbseg_ctx* c, int max_batch)
{
    API_BEGIN
    REQUIRE(c && !c->finalized, "bad handle / already finalized");
    HIPCHK(hipSetDevice(c->device));
    if (fuse_bottlenecks(c)) return 1;
    if (build_fast_gather_tables(c)) return 1;
    if (attach_dec_halo_tables(c)) return 1;
    if (fuse_expand_reduce(c)) return 1;
    if (fuse_conv3_expand_reduce(c)) return 1;          // (after fuse_expand_reduce: it extends the pairs that pass marked)
    fuse_stem_pool(c);
    REQUIRE(max_batch >= 1, "max_batch must be >= 1");
    REQUIRE(c->classes > 0 && !c->ops.empty(), "plan must contain a head (head op or a conv with a fused head)");
    c->max_batch = max_batch;
    find_region_chain(c);
    for (auto& t : c->tensors) {
        const size_t bytes = kZeroHeaderBytes + t.elems_per_patch * max_batch * c->elem * c->planes + 256;
        REQUIRE(bytes < ((size_t)1 << 32), "tensor %dx%dx%d x batch %d exceeds the 4 GiB gather window", t.H, t.W, t.C, max_batch);
        if (dmalloc(c, (void**)&t.lane_buf[0], bytes)) return 1;
        t.buf = t.lane_buf[0];
        // input forms rely on their zero borders / zero channels; headers must be zero for every tensor
        HIPCHK(hipMemset(t.buf, 0, t.is_input_form ? bytes : (size_t)kZeroHeaderBytes));
    }
    c->lane1_batch = (c->lanes == 2 && max_batch >= 2 * kMinLaneTiles) ? (max_batch + 1) / 2 : 0;
    if (c->lane1_batch)
        for (auto& t : c->tensors) {
            const size_t bytes = kZeroHeaderBytes + t.elems_per_patch * c->lane1_batch * c->elem * c->planes + 256;
            if (dmalloc(c, (void**)&t.lane_buf[1], bytes)) return 1;
            HIPCHK(hipMemset(t.lane_buf[1], 0, t.is_input_form ? bytes : (size_t)kZeroHeaderBytes));
        }
    // a 3x3 conv that conv3_expand_reduce computes never writes its output tensor: give the buffers a defined content (zeros) -- the debug
    // read-back of a plan tensor and the tests that compare whole plans then see the same bytes in every run
    for (const Op& op : c->ops)
        if (op.type == kConv && op.conv.fused_conv3 >= 0) {
            Tensor& t = c->tensors[c->ops[op.conv.fused_conv3].conv.d.out_tensor];        // (= the expand conv's source: fuse_conv3_expand_reduce)
            for (int lane = 0; lane < 2; ++lane)
                if (t.lane_buf[lane])
                    HIPCHK(hipMemset(t.lane_buf[lane], 0, kZeroHeaderBytes + t.elems_per_patch * (size_t)(lane == 0 ? max_batch : c->lane1_batch) * c->elem * c->planes));
        }
    float lut[256];
    for (int v = 0; v < 256; ++v) lut[v] = (float)((double)v / 255.0);   // main.py:239 in f64, then Keras' f32 feed
    if (upload(c, &c->d_lut, lut, 256)) return 1;
    if (dmalloc(c, (void**)&c->d_hist, 257 * sizeof(unsigned))) return 1;
    if (dmalloc(c, (void**)&c->d_tile_xy, sizeof(int) * 2 * max_batch)) return 1;
    if (dmalloc(c, (void**)&c->d_batch_labels, (size_t)max_batch * c->in_H * c->in_W)) return 1;
    HIPCHK(hipDeviceSynchronize());
    c->finalized = true;
    return 0;
    API_END
}

}  // extern "C"
