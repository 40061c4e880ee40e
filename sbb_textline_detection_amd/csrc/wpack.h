// wpack.h -- private, host only, no HIP call: how fp32 weights become what the kernels read.  plan_build.hip uploads what these functions
// return; tests/test_wpack_cpu.py compiles the header into a host program of its own and holds every form to tests/wpack_ref.py.
//   * the 16-bit roundings: half16 (plain modes), split_prescale + split16 (split mode: hi | lo of the pre-scaled weight)
//   * an MFMA A fragment = 64 lanes x 8 halves; lane l holds row (l & 15) of a 16-row block and k = (l >> 4) * 8 .. + 7 of a 32-wide K slice
//       frag_from_matrix  / matrix_frags: slices of a packed [rows][Ktot] conv matrix (its rows already are in conv_row_channel order)
//       frag_from_weights / weight_frags: straight from fp32 weights [K][cout], rows in conv_row_channel order
//       tail_presum: the fused tail's pre-summed weights, which weight_frags then rounds
//   * conv_ktable / conv_pack_matrix: the contraction order of conv_igemm_mfma and the packed [cout_pad][Ktot] matrix in that order
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "internal.h"

namespace sbbseg {

inline float max_abs(const float* w, size_t n, float wmax = 0.f)
{
    for (size_t i = 0; i < n; ++i) wmax = std::fmax(wmax, std::fabs(w[i]));
    return wmax;
}

// split mode: one power-of-two pre-scale per conv brings the largest |w| (finite: the caller checks) into [256, 512), so that the lo
// halves of all weights within 2^12 of it are normal fp16 numbers; the epilogue multiplies `scale` by 2^-s (exact)
inline float split_prescale(float wmax)
{
    if (!(wmax > 0.f)) return 1.f;
    int ex = 0;
    (void)std::frexp(wmax, &ex);                     // wmax = m * 2^ex, m in [0.5, 1)
    int sexp = 9 - ex;                               // wmax * 2^sexp in [256, 512)
    sexp = sexp > 60 ? 60 : (sexp < -60 ? -60 : sexp);
    return std::ldexp(1.f, sexp);
}

struct SplitHalf { uint16_t hi, lo; };
inline SplitHalf split16(float v, float wpre)
{
    const float sv = v * wpre;                       // exact (power of two)
    const uint16_t hb = f32_to_f16_rne(sv);
    return {hb, f32_to_f16_rne(sv - (float)__builtin_bit_cast(_Float16, hb))};
}
inline uint16_t half16(int precision, float v) { return precision == kF16 ? f32_to_f16_rne(v) : f32_to_bf16_rne(v); }

// dst[64 lanes][8] <- rows row_block * 16 .. + 15 of mat[rows][Ktot], K elements kstep * 64 + lo * 32 .. + 31
// (split mode: lo = the hi | lo plane of a 32-channel K-step; plain fp16: the k-half of a 64-channel K-step)
inline void frag_from_matrix(uint16_t* dst, const uint16_t* mat, size_t Ktot, int row_block, int kstep, int lo)
{
    for (int l = 0; l < 64; ++l) {
        const uint16_t* src = mat + (size_t)(row_block * 16 + (l & 15)) * Ktot + (size_t)kstep * 64 + lo * 32 + (l >> 4) * 8;
        for (int e = 0; e < 8; ++e) dst[l * 8 + e] = src[e];
    }
}

// hi[64 lanes][8] <- w(conv_row_channel(row_block * 16 + (l & 15), cout), (l >> 4) * 8 + e), k = 0 .. 31 being the caller's K slice.
// Plain modes: one rounding into `hi` (`lo`, `wpre` unused); split mode: hi | lo of w * wpre into `hi` and `lo`.
template <class W>
inline void frag_from_weights(int precision, float wpre, uint16_t* hi, uint16_t* lo, int row_block, int cout, W&& w)
{
    for (int l = 0; l < 64; ++l) {
        const int o = conv_row_channel(row_block * 16 + (l & 15), cout);
        for (int e = 0; e < 8; ++e) {
            const float v = w(o, (l >> 4) * 8 + e);
            if (is_split(precision)) {
                const SplitHalf s = split16(v, wpre);
                hi[l * 8 + e] = s.hi;
                lo[l * 8 + e] = s.lo;
            } else {
                hi[l * 8 + e] = half16(precision, v);
            }
        }
    }
}

// Appends the [K / 32 slices][cout / 16 row blocks] fragments of w[K][cout] (k = slice * 32 + ...).  Split mode (wpre = the conv's
// power-of-two pre-scale): `interleaved` ? each fragment's hi, then its lo : the whole block of hi fragments, then the block of lo fragments
inline void weight_frags(std::vector<uint16_t>& out, int precision, float wpre, const float* w, int K, int cout, bool interleaved)
{
    const size_t n = (size_t)(K / 32) * (cout / 16), P = is_split(precision) ? 2 : 1, base = out.size();
    out.resize(base + n * P * 512);
    for (int ks = 0; ks < K / 32; ++ks)
        for (int mi = 0; mi < cout / 16; ++mi) {
            const size_t f = (size_t)ks * (cout / 16) + mi;
            uint16_t* hi = &out[base + (interleaved ? f * P : f) * 512];
            uint16_t* lo = P == 2 ? hi + (interleaved ? 1 : n) * 512 : hi;
            frag_from_weights(precision, wpre, hi, lo, mi, cout, [&](int o, int k) { return w[(size_t)(ks * 32 + k) * cout + o]; });
        }
}

// Appends the [ksteps][n_rb row blocks from rb0][hi | lo] fragments of a packed matrix (hi | lo: the planes of a split K-step / the k-halves
// of a plain fp16 one) -- how every fused kernel streams the rows of the conv it replaces, K-step by K-step in that conv's own order
inline void matrix_frags(std::vector<uint16_t>& out, const uint16_t* mat, size_t Ktot, int rb0, int n_rb, int ksteps)
{
    const size_t base = out.size();
    out.resize(base + (size_t)ksteps * n_rb * 2 * 512);
    for (int t = 0; t < ksteps; ++t)
        for (int rb = 0; rb < n_rb; ++rb)
            for (int lo = 0; lo < 2; ++lo) frag_from_matrix(&out[base + (((size_t)t * n_rb + rb) * 2 + lo) * 512], mat, Ktot, rb0 + rb, t, lo);
}

// The fused tail's weights before rounding: the 3x3 taps that hit the same source pixel of the upsampled src0 pre-summed in fp32, per output parity class
// q = (py, px): [4 q][KS K-steps][64 k][32 cout].  K-steps 0-3 = the class's 2 x 2 taps of src0 (k = channel), then the 9 image taps:
// plain modes two K-steps, one tap per k-group of 8 (3 channels used); split mode ONE K-step, two taps per k-group, 4 channels each
// (3 used) -- see dec_tail_fused_x3ps.  w_src0: [3][3][64][32], w_img: [3][3][3][32].  The fragments are weight_frags of each class's [KS * 64][32]
constexpr int kTailSplitKSteps = 5;
inline std::vector<float> tail_presum(bool split, const float* w_src0, const float* w_img)
{
    static const int taps[2][2][2] = {{{0, 0}, {1, 2}}, {{0, 1}, {2, 2}}};   // [parity][t] -> first,last ky summed
    const int C0 = 64, CO = 32, KS = split ? kTailSplitKSteps : kTailKSteps;
    std::vector<float> pre((size_t)4 * KS * 64 * CO, 0.f);
    for (int q = 0; q < 4; ++q) {
        const int py = q >> 1, px = q & 1;
        for (int ks = 0; ks < KS; ++ks)
            for (int k = 0; k < 64; ++k)
                for (int o = 0; o < CO; ++o) {
                    float v = 0.f;
                    if (ks < 4) {
                        const int ty = ks >> 1, tx = ks & 1;
                        for (int ky = taps[py][ty][0]; ky <= taps[py][ty][1]; ++ky)
                            for (int kx = taps[px][tx][0]; kx <= taps[px][tx][1]; ++kx)
                                v += w_src0[((size_t)(ky * 3 + kx) * C0 + k) * CO + o];
                    } else {
                        const int t = split ? k >> 2 : (ks - 4) * 8 + (k >> 3), ch = split ? k & 3 : k & 7;
                        if (t < 9 && ch < 3) v = w_img[((size_t)t * 3 + ch) * CO + o];
                    }
                    pre[(((size_t)q * KS + ks) * 64 + k) * CO + o] = v;
                }
    }
    return pre;
}
// ---- conv_igemm_mfma's contraction order: source-major, then 64-channel group, then tap (ky,kx), then the group's
// 8-channel granules.  Keeping the taps of one channel group ADJACENT makes the shifted re-reads
// of the same pixel rows hit in L2 (measured with tap-outer order: dec1 fetched 2.5 GB per
// launch for 70 MB of input).  Each source's segment is padded to whole K-steps (64) with
// out-of-bounds ("zero") granules.  Tap offsets carry the source's padding and placement offset.
// Split mode (kF16X3): a K-step is 32 channels (4 granules) of one tap; its slots 0-3 are those granules' "hi"
// halves, slots 4-7 the "lo" halves of the same channels (lo plane of the stored pixel, lo half of the weight).
struct ConvKTable {
    std::vector<KTabEntry> ktab;          // slot table: 8 entries per K-step (what the kernels index)
    std::vector<KStepRec> ksteps;         // one record per K-step
    int ksteps_src[2] = {0, 0}, total_ksteps = 0;
    int tap_lo[2][2] = {{127, 127}, {127, 127}}, tap_hi[2][2] = {{-127, -127}, {-127, -127}};      // [source][y|x]
    bool fg_ok = true;                    // every K-step regular
    struct KRef { int s, ky, kx, c0; };   // per slot: source (-1 = K padding), tap, first channel (split mode: slots 4-7 repeat slots 0-3)
    std::vector<KRef> kref;
};

// src_C: channels of the source tensors as stored.  grouped_taps: see the tap order below (SBBSEG_TAP_ORDER, read by the caller).
inline ConvKTable conv_ktable(const sbbseg_conv_desc& d, const int* src_C, int precision, bool grouped_taps)
{
    ConvKTable kt;
    const bool split = is_split(precision);
    const int elem = precision == kF32 ? 4 : 2;
    const int gps = split ? 4 : kGranulesPerStep;            // channel granules per K-step
    std::vector<KTabEntry> lin;                              // granule list in contraction order (hi halves in split mode)
    std::vector<ConvKTable::KRef> lref;
    for (int s = 0; s < d.n_src; ++s) {
        const sbbseg_conv_src& cs = d.src[s];
        const int g8 = (cs.channels + 7) / 8;
        // Tap order inside a channel group.  A 3x3 stride-2 source (the skip tensor of a parity-split decoder conv) is walked parity
        // set by parity set -- (0,0) (0,2) (2,0) (2,2) | (0,1) (2,1) | (1,0) (1,2) | (1,1): taps of one set read the SAME source pixels
        // (shifted by one output step), so their K-steps, now adjacent, find the lines of the previous step in L2; in row-major
        // order the next touch of a line came 2 or 6 K-steps later, after 4-12 MB of other gathers had passed through the XCD's
        // 4 MB L2 (PMC: dec4 fetched 4.4x its input).  SBBSEG_TAP_ORDER=0: row-major (A/B).  Only the order of the sum changes.
        std::vector<int> tap_order;
        if (grouped_taps && cs.kh == 3 && cs.kw == 3 && cs.stride_y == 2 && cs.stride_x == 2) tap_order = {0, 2, 6, 8, 1, 7, 3, 5, 4};
        else
            for (int t = 0; t < cs.kh * cs.kw; ++t) tap_order.push_back(t);
        const size_t first = lin.size();
        for (int cg = 0; cg < g8; cg += gps)
            for (int ti = 0; ti < cs.kh * cs.kw; ++ti) {
                const int ky = tap_order[ti] / cs.kw, kx = tap_order[ti] % cs.kw;
                for (int g = cg; g < g8 && g < cg + gps; ++g) {
                    KTabEntry e;
                    e.dy = (int16_t)(ky - cs.pad_top - cs.off_y);
                    e.dx = (int16_t)(kx - cs.pad_left - cs.off_x);
                    // byte offset of the granule's 8 channels inside the stored pixel (split mode: of their hi halves, in the
                    // interleaved [group hi | group lo] layout, internal.h)
                    e.coff = split ? split_hi_elem(src_C[s], g * 8) * elem : g * 8 * elem;
                    lin.push_back(e);
                    lref.push_back({s, ky, kx, g * 8});
                }
            }
        const int granules = (int)(lin.size() - first), ks = (granules + gps - 1) / gps;
        lin.resize(first + (size_t)ks * gps, KTabEntry{16000, 0, 0});
        lref.resize(lin.size(), {-1, 0, 0, 0});
        kt.ksteps_src[s] = ks;
        kt.total_ksteps += ks;
    }
    kt.ktab.resize((size_t)kt.total_ksteps * kGranulesPerStep);
    kt.kref.resize(kt.ktab.size());
    for (int t = 0; t < kt.total_ksteps; ++t)
        for (int g = 0; g < kGranulesPerStep; ++g) {
            const size_t li = (size_t)t * gps + (split ? (g & 3) : g), ki = (size_t)t * kGranulesPerStep + g;
            kt.ktab[ki] = lin[li];
            kt.kref[ki] = lref[li];
            if (split && g >= 4 && lref[li].s >= 0) kt.ktab[ki].coff += split_group(src_C[lref[li].s]) * elem;      // the group's lo halves
        }
    kt.ksteps.resize(kt.total_ksteps);
    for (int t = 0; t < kt.total_ksteps; ++t) {
        const KTabEntry* e = &kt.ktab[(size_t)t * kGranulesPerStep];
        const ConvKTable::KRef* kr = &kt.kref[(size_t)t * kGranulesPerStep];
        KStepRec r;
        r.dy = e[0].dy; r.dx = e[0].dx; r.coff = e[0].coff; r.irregular = 0; r.pad_ = 0;
        for (int g = 1; g < kGranulesPerStep; ++g) {
            // regular: one tap, channel-consecutive granules; in split mode slots 4-7 are slots 0-3 moved to the lo plane
            // (same distance for every step of a source: SrcDesc::lo_off)
            int want = e[0].coff + 16 * g;
            if (split) {
                const int lo_off = kr[0].s >= 0 ? split_group(src_C[kr[0].s]) * elem : 0;
                want = e[0].coff + 16 * (g & 3) + (g >> 2) * lo_off;
                if (kr[0].s < 0 || kr[g].s != kr[0].s) r.irregular = 1;
            }
            if (e[g].dy != e[0].dy || e[g].dx != e[0].dx || e[g].coff != want) r.irregular = 1;
        }
        if (precision == kF32) r.irregular = 1;     // the fp32 check kernel only walks the granule table
        if (r.irregular) kt.fg_ok = false;
        const int sidx = t < kt.ksteps_src[0] ? 0 : 1;
        kt.tap_lo[sidx][0] = std::min(kt.tap_lo[sidx][0], (int)r.dy); kt.tap_hi[sidx][0] = std::max(kt.tap_hi[sidx][0], (int)r.dy);
        kt.tap_lo[sidx][1] = std::min(kt.tap_lo[sidx][1], (int)r.dx); kt.tap_hi[sidx][1] = std::max(kt.tap_hi[sidx][1], (int)r.dx);
        kt.ksteps[t] = r;
    }
    return kt;
}

// pack weights [cout_pad][Ktot] in kt's order: one source pointer per K element (null = K padding), then row by row in
// blocks of 64 K elements -- writes are contiguous, the 64 source lines of a block stay in cache across
// neighbouring output channels (the column-by-column form of this loop took 0.6 s of a model's load time).
// T = uint16_t: rows in conv_row_channel order, each element half16 or the slot's half of split16(., wpre); T = float (fp32 mode): as given.
// w_src[s]: float32 [kh][kw][channels][cout] of source s.
template <class T>
inline std::vector<T> conv_pack_matrix(const ConvKTable& kt, const sbbseg_conv_desc& d, const float* const* w_src, int precision, int cout_pad, float wpre)
{
    const int Ktot = kt.total_ksteps * kBK;
    std::vector<const float*> ksrc((size_t)Ktot, nullptr);
    for (size_t g = 0; g < kt.kref.size(); ++g) {
        const ConvKTable::KRef& r = kt.kref[g];
        if (r.s < 0) continue;
        const sbbseg_conv_src& cs = d.src[r.s];
        for (int q = 0; q < 8 && r.c0 + q < cs.channels; ++q)
            ksrc[g * 8 + q] = w_src[r.s] + ((size_t)(r.ky * cs.kw + r.kx) * cs.channels + r.c0 + q) * d.cout;
    }
    std::vector<int> row_ch(cout_pad);
    for (int row = 0; row < cout_pad; ++row) row_ch[row] = precision != kF32 ? conv_row_channel(row, d.cout) : row;
    std::vector<T> dst((size_t)cout_pad * Ktot);              // (zeros: the rows of the channel padding stay as they are)
    // split mode: slots 4-7 of a K-step hold the same weights as slots 0-3 -- one split16 gives out[k] and out[k + 32]
    const int kw = is_split(precision) ? kBK / 2 : kBK;
    auto pack = [&](auto put) {                               // (one instance per rounding: the choice stays out of the inner loop)
        for (int kb = 0; kb < Ktot; kb += kBK) {
            const float* const* ks = &ksrc[kb];
            for (int row = 0; row < cout_pad; ++row) {
                const int o = row_ch[row];
                if (o >= d.cout) continue;
                T* out = dst.data() + (size_t)row * Ktot + kb;
                for (int k = 0; k < kw; ++k) put(out + k, ks[k] ? ks[k][o] : 0.f);
            }
        }
    };
    if (precision == kF32) pack([](T* out, float v) { *out = (T)v; });
    else if (is_split(precision)) pack([wpre](T* out, float v) { const SplitHalf s = split16(v, wpre); out[0] = (T)s.hi; out[kBK / 2] = (T)s.lo; });
    else if (precision == kF16) pack([](T* out, float v) { *out = (T)f32_to_f16_rne(v); });
    else pack([](T* out, float v) { *out = (T)f32_to_bf16_rne(v); });
    return dst;
}

}  // namespace sbbseg
