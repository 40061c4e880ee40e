// conv_choice.h -- private, host only, no HIP call, on top of ctx.h: the form of one conv_igemm_mfma launch (route.h's kRouteConv) -- tile,
// gather, tile walk, owned-region table, split-K.  THE one statement of the rule: launch_generic_conv (forward.hip) fills ConvParams from the
// chosen form, launch_conv (kernels.hip) maps its tile to a template instantiation, and tests/test_conv_choice_cpu.py holds choose_conv to a
// restatement of the three places that used to decide it, on the CPU.  ConvForm and ConvTileForm themselves are in internal.h (kernels.hip reads
// them without ctx.h).
#pragma once

#include <stdlib.h>

#include "ctx.h"

namespace sbbseg {

// The environment's A/B thresholds of the rule.  A K threshold of 0 in a *_res256_mink switches that rule off.
struct ConvEnv {
    int f16_res256_mink = 256;      // SBBSEG_F16_RES256_MINK: plain modes, residual layers on the 256 x 256 tile from this K on (-3..-4 % each,
                                    //   profiles/r05_experiments.md section 13; the K = 128 expand of stage 3 loses 1.5 %: left out)
    int f16_t256_mink = 384;        // SBBSEG_F16_T256_MINK: plain modes, 256 x 256 from this K on (384: the stage-3 projection merge, 0.40 -> 0.31 ms)
    int x3_res256_mink = 256;       // SBBSEG_X3_RES256_MINK: split mode, residual layers (the expand convs expand_reduce does not take) on 256 x 256: the
                                    //   pixel operand is re-read by half as many channel tiles, the residual is read in the epilogue (section 12)
    int x3_t256_mink = 768;         // SBBSEG_X3_T256_MINK: split mode, 256 x 256 from this K on (768: the stage-3 projection merge, 0.79 -> 0.68 ms)
    int x3_t512_mink = 2048;        // SBBSEG_X3_T512_MINK: split mode, 512 x 128 from this K on
    size_t pshare_max = (size_t)2 << 20;    // SBBSEG_PSHARE_MAX_MB: weight bytes up to which a single-class layer takes the pixel-sharing walk
                                    //   (beyond it the K >= 768 convs of stages 4 / 5 re-fetch their pixels once per channel tile under map 0)
    bool split_issue = true;        // SBBSEG_SPLIT_ISSUE=0: plain 16-bit modes, bit 3 of ConvParams::variant_flags
};

// read once per process
inline const ConvEnv& conv_env()
{
    static const ConvEnv env = [] {
        ConvEnv e;
        const auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        e.f16_res256_mink = num("SBBSEG_F16_RES256_MINK", e.f16_res256_mink);
        e.f16_t256_mink = num("SBBSEG_F16_T256_MINK", e.f16_t256_mink);
        e.x3_res256_mink = num("SBBSEG_X3_RES256_MINK", e.x3_res256_mink);
        e.x3_t256_mink = num("SBBSEG_X3_T256_MINK", e.x3_t256_mink);
        e.x3_t512_mink = num("SBBSEG_X3_T512_MINK", e.x3_t512_mink);
        e.pshare_max = (size_t)num("SBBSEG_PSHARE_MAX_MB", 2) << 20;
        const char* si = getenv("SBBSEG_SPLIT_ISSUE");
        e.split_issue = !(si && si[0] == '0');
        return e;
    }();
    return env;
}

// bytes of a source's buffer a launch of n patches has in use (SrcDesc::bytes), and of one stored pixel
inline size_t conv_src_bytes(const sbbseg_ctx* c, const Tensor& t, int n) { return kZeroHeaderBytes + t.elems_per_patch * (size_t)n * c->elem * c->planes; }
inline int conv_src_pix_bytes(const sbbseg_ctx* c, const Tensor& t) { return t.C * c->elem * c->planes; }

// entries of the pixel table the chunk's owned-region run (region.h) offers this op's launch, or -1: no such level
inline int conv_region_entries(const sbbseg_ctx* c, const Op& op)
{
    const int rlv = c->rr.on ? op.region_level : -1;
    return rlv >= 0 && c->rr.kind[rlv] == 1 ? c->rr.total[rlv] : -1;
}

// A pure function of the op's plan facts (`co`, and H, W, C and elems_per_patch of its source tensors), the handle's knobs (precision, elem,
// planes; sbbseg_debug_set_conv_variant's conv_variant, ph8, plain_gather, ranged_walk, contig_max_k; the whole-image branch's ksplit_now), the
// call (n patches; region_entries: see conv_region_entries) and the environment's thresholds.  conv_variant: bits 0-1 = variants 1-3, bit 2 =
// one block per tile, bit 3 = plain walks, bit 4 = half-K-step stages, bit 5 = the pixel-sharing walk in the plain modes.
inline ConvForm choose_conv(const sbbseg_ctx* c, const ConvOp& co, int n, int region_entries, const ConvEnv& env)
{
    ConvForm f{};
    const bool x3 = c->precision == kF16X3;
    const int variant = c->conv_variant & 3;
    const bool one_block_per_tile = c->conv_variant & 4, plain_walk = c->conv_variant & 8, half_stages = c->conv_variant & 16;
    const int cout = co.d.cout, bc = conv_tile_bc(cout);
    const bool residual = co.d.residual_tensor >= 0;

    // ---- gather.  Fast gather is off under bit 17, without tables, and where a source buffer plus its bias reaches 2^31 bytes (bit 31 of a
    // lane offset marks an out-of-bounds tap); pointwise ops get the value 2.  (plan_build keeps short-K layers off the tables: the per-tile
    // mask set-up costs them 1-10 %, from ~9 K-steps on the fast gather wins 2-10 %, profiles/r02_experiments.md)
    bool fast = co.d_fgstep_cls[0] && !c->plain_gather;
    bool wide_pixels = true;                // every source has at least 128 bytes per pixel (regular K-steps of >= 64 channels)
    for (int s = 0; s < co.d.n_src; ++s) {
        const Tensor& t = c->tensors[co.d.src[s].tensor];
        const int pix_bytes = conv_src_pix_bytes(c, t);
        if (conv_src_bytes(c, t, n) + (size_t)kFgBiasPixels(t.W) * pix_bytes >= ((size_t)1 << 31)) fast = false;
        if (pix_bytes < 128) wide_pixels = false;
    }
    f.fast_gather = fast ? (co.fg_pointwise ? 2 : 1) : 0;
    // SBBSEG_SPLIT_ISSUE=0 sets bit 3 in the plain modes only
    f.variant_flags = ((c->conv_variant & 64) ? 1 : 0) | ((c->conv_variant & 128) ? 2 : 0) | (c->ph8 ? 4 : 0) | (!env.split_issue && !x3 ? 8 : 0);

    // ---- tile walk.  KNOWN QUIRK, kept: the walk is chosen from the whole-grid M = n * Ho * Wo, before a region table replaces M.
    // The XCD-grouped pixel-sharing walk for single-class layers is opt-in (bit 5) in the plain modes -- measured neutral-to-slower: it removes
    // the n_ct-fold re-fetch of the pixel operand, but those layers are not bound by fetch bytes -- and the default in the split mode (twice the
    // pixel bytes; +0.7 % page throughput, profiles/r03_experiments.md).
    const int whole_M = n * co.Ho * co.Wo;
    const size_t weight_bytes = (size_t)co.cout_pad * co.Ktot * c->elem;
    f.tile_map = ((c->conv_variant & 32) || x3) && !plain_walk && !one_block_per_tile && cout > bc && whole_M >= 256 * 128 && weight_bytes <= env.pshare_max ? 1 : 0;
    if (f.tile_map == 1 && co.n_cls == 1 && co.Ktot <= c->contig_max_k) f.tile_map = 2;
    // class-minor then overrides it to 1, or to 3 with bit 19: small weights, the classes of a pixel tile share their source pixels in one L2
    // (dec1 / dec2 too: fetch -30 / -53 %, time unchanged)
    if (co.n_cls > 1 && (co.n_cls & (co.n_cls - 1)) == 0 && !plain_walk && !one_block_per_tile && weight_bytes <= ((size_t)16 << 20)) {
        f.cls_minor = 1;
        f.tile_map = c->ranged_walk ? 3 : 1;
    }

    // ---- owned-region table (region.h): read by the fast-gather form, 2-stage whole-K-step tiles only -- what every decoder conv runs by
    // default.  Withheld whenever bit 4, variant 2 or bit 16 is set, even where the tile finally taken has a fast-gather form (32-channel tiles
    // under bit 4, any tile but 256 x 256 under bit 16, 256 x 256 where the 8-phase conditions fail): the level then runs whole -- a superset,
    // same results -- and counts as whole.
    f.table = region_entries >= 0 && f.fast_gather && !half_stages && variant != 2 && !c->ph8;
    const int M = f.table ? region_entries : whole_M;

    // ---- split-K.  One patch through a long-K conv = 2-32 tiles of 100-400 K-steps at ~1 us a step on as many CUs: the whole-image branch
    // (1 forward per page) splits the K range over the idle CUs -- up to 16 blocks per 128 x 128 tile, each at least 4 K-steps, fp32 partial sums
    // added in split order by splitk_finish.  Only there: a split launch differs from the unsplit one in the last bits, and the patch paths
    // promise batch-size-independent results.  It forces tile_map = 0 and cls_minor = 0.
    const bool whole_tensor = co.n_cls == 1 && co.d.out_stride_y == 1 && co.d.out_stride_x == 1 && co.d.out_off_y == 0 && co.d.out_off_x == 0 &&
                              co.TH == co.Ho && co.TW == co.Wo;
    const bool four_parities = co.n_cls == 4 && co.d.out_stride_y == 2 && co.d.out_stride_x == 2 && co.TH == 2 * co.Ho && co.TW == 2 * co.Wo;
    if (c->ksplit_now && n == 1 && c->precision != kF32 && f.fast_gather && bc == 128 && co.d.raw_out_tensor < 0 && !co.d.head_classes &&
        co.d.out_tensor >= 0 && cout % 8 == 0 && (whole_tensor || four_parities)) {
        const long tiles = (long)co.n_cls * ((M + 127) / 128) * ((cout + 127) / 128);
        int ks = 0;
        while (ks < 4 && (tiles << (ks + 1)) <= 512 && co.total_ksteps % (2 << ks) == 0 && (co.total_ksteps >> (ks + 1)) >= 4) ++ks;
        f.ks_shift = ks;
    }
    if (f.ks_shift > 0) {
        f.tile_map = 0; f.cls_minor = 0;
        f.tile = kTile128x128; f.fg = 1;
        return f;
    }

    // ---- tile.  Measured on MI355X (profiles/r01_conv_variants.md): with two 4-wave blocks per CU the 2-stage tiles already hide the staging
    // latency; the 8-wave tiles (128 x 64 wave tiles: LDS bytes per MFMA x0.75, L2 bytes per MFMA x0.5) win on long-K layers that still give
    // every CU a block -- 200 tiles -- while short-K / HBM-bound layers and small grids stay on the 4-wave tiles.
    const long t256 = (long)co.n_cls * ((M + 255) / 256) * (cout / 256);
    const long t512 = (long)co.n_cls * ((M + 511) / 512) * ((cout + 127) / 128);
    const bool fits256 = bc == 128 && cout % 256 == 0;
    const int dflt = bc == 128 ? kTile128x128 : bc == 64 ? kTile256x64 : kTile256x32;
    int tile = -1;
    if (x3) {
        // split mode: the 4-wave tiles at 2 blocks per CU by default (3 MFMAs per product for the same LDS bytes: the matrix pipe fills first).
        // Bit 4 and variants 2 and 3 mean nothing here; the residual rule and the auto rule apply at variant 0 only.
        if (variant == 0 && fits256 && residual && env.x3_res256_mink > 0 && co.Ktot >= env.x3_res256_mink && t256 >= 200) tile = kTile256x256;
        else if (variant == 0 && bc == 128 && !residual && cout % 256 == 0 && co.Ktot >= env.x3_t256_mink && t256 >= 200) tile = kTile256x256;
        else if (variant == 0 && bc == 128 && !residual && co.Ktot >= env.x3_t512_mink && t512 >= 200) tile = kTile512x128;
        else tile = dflt;
    } else {
        // the 8-phase form runs only under all of: bit 16, at least 2 K-steps, no half stages, no region table, >= 128 bytes per source pixel
        // (the condition the kernel's comments call ph8_ok)
        const bool ph8 = c->ph8 && co.total_ksteps >= 2 && !half_stages && !f.table && wide_pixels;
        const int big256 = ph8 ? kTile256x256Ph8 : kTile256x256;
        // bit 4 is looked at before variant 3, and falls through for 32-channel tiles
        if (half_stages && bc != 32)
            tile = bc == 64 ? kTile256x64Half : fits256 && !residual && co.Ktot >= 512 && t256 >= 200 ? kTile256x256Half : kTile128x128Half;
        // variant 3 forces the 8-wave 2-stage tiles: 512 x 128 where cout % 256 != 0; 32-channel tiles fall through to the default ladder
        else if (variant == 3 && bc != 32) tile = bc == 64 ? kTile512x64 : fits256 ? big256 : kTile512x128;
        // the residual rule (never 8-phase) and the auto rule apply at variant 0 only
        else if (variant == 0 && fits256 && residual && env.f16_res256_mink > 0 && co.Ktot >= env.f16_res256_mink && t256 >= 200) tile = kTile256x256;
        else if (variant == 0 && bc == 128 && !residual && cout % 256 == 0 && co.Ktot >= env.f16_t256_mink && t256 >= 200) tile = big256;
        else if (variant == 0 && bc == 128 && !residual && co.Ktot >= 1024 && t512 >= 200) tile = kTile512x128;
        // variant 2 means the 3-stage tiles (5-25 % slower on every layer: opt-in only)
        else if (variant == 2) tile = bc == 128 ? kTile256x128S3 : bc == 64 ? kTile256x64S3 : kTile256x32S3;
        else tile = dflt;
    }
    f.tile = tile;
    // (a table is only handed to a tile with a fast-gather form: its rule above excludes bit 4, variant 2 and bit 16)
    f.fg = f.fast_gather && conv_tile_has_fg(kConvTileDims[tile]);
    return f;
}

}  // namespace sbbseg
