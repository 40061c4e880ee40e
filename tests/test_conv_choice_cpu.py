"""csrc/conv_choice.h -- the form of one conv_igemm_mfma launch: tile, gather, tile walk, owned-region table, split-K -- without a GPU.

A small host program includes the header, builds synthetic conv ops and source tensors by hand (no HIP call; the table pointers are dummies
that nothing dereferences) and prints ``choose_conv`` over a sweep of op facts x knobs x calls x environment thresholds.  The program is
built with the address and undefined-behaviour sanitizers (a stand-alone host program: nothing is preloaded).  Every line carries its own
inputs, so the expectation below does not depend on how the program enumerates them.

The sweep is held to ``parent_form``: a restatement, ladder by ladder, of the three places that decided the form before the header existed
(csrc/forward.hip launch_generic_conv; csrc/kernels.hip launch_conv, launch_conv_16, launch_conv_x3, ph8_ok, launch_conv_t at 9dd1a7e) --
including their error returns, which the sweep must never reach.  It is written from that code, not from the header: it fills the fields of
ConvParams the launchers read, then walks the launchers' ladders down to the template arguments of the instantiation they call."""
import collections
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
BF16, F32, F16, F16X3 = 0, 1, 2, 3                # csrc/internal.h enum Precision
MODES = {F16: "f16", BF16: "bf16", F16X3: "x3"}

Op = collections.namedtuple("Op", "cout cout_pad Ktot total_ksteps n_cls Ho Wo TH TW osy osx ooy oox residual raw_out out head_classes "
                                  "has_fg pointwise n_src H0 W0 C0 epp0 H1 W1 C1 epp1")
Env = collections.namedtuple("Env", "f16_res256 f16_t256 x3_res256 x3_t256 x3_t512 pshare_max split_issue")
Case = collections.namedtuple("Case", "op env precision conv_variant ph8 plain_gather ranged_walk contig_max_k ksplit_now n region")
Form = collections.namedtuple("Form", "tile fg fast_gather ks_shift tile_map cls_minor table variant_flags")
DEFAULT_ENV = Env(256, 384, 256, 768, 2048, 2 << 20, 1)

# conv_igemm_mfma<BP, BC, WP, WC, NS, F16, GS, PH8, X3, FG, KS> as kernels.hip instantiates it: (BP, BC, WP, WC, NS, GS, PH8) per tile form,
# x the precision mode, the gather and split-K
TILES_16 = [(128, 128, 2, 2, 2, 8, 0), (256, 256, 2, 4, 2, 8, 0), (256, 256, 2, 4, 2, 8, 1), (512, 128, 4, 2, 2, 8, 0), (512, 64, 8, 1, 2, 8, 0),
            (256, 128, 4, 2, 3, 8, 0), (256, 64, 8, 1, 3, 8, 0), (256, 32, 8, 1, 3, 8, 0), (256, 64, 4, 1, 2, 8, 0), (256, 32, 4, 1, 2, 8, 0),
            (256, 256, 2, 4, 4, 4, 0), (128, 128, 2, 2, 4, 4, 0), (256, 64, 4, 1, 4, 4, 0)]
TILES_X3 = [(128, 128, 2, 2, 2, 8, 0), (256, 256, 2, 4, 2, 8, 0), (512, 128, 4, 2, 2, 8, 0), (256, 64, 4, 1, 2, 8, 0), (256, 32, 4, 1, 2, 8, 0)]
WITH_FG = [t for t in TILES_16 if t[4] == 2 and t[5] == 8 and not t[6]]
SYMBOLS = ({(t, m, 0, 0) for m in ("f16", "bf16") for t in TILES_16} | {(t, m, 1, 0) for m in ("f16", "bf16") for t in WITH_FG}
           | {(t, "x3", fg, 0) for t in TILES_X3 for fg in (0, 1)} | {(TILES_16[0], m, 1, 1) for m in MODES.values()})

_PROBE = r"""
#include "conv_choice.h"
#include <cstdio>
using namespace sbbseg;

struct Facts { ConvOp co; std::vector<Tensor> tensors; };
static std::vector<Facts> g_ops;
static std::vector<ConvEnv> g_envs;
static FgStepRec g_fg[1];                        // table pointer: non-null, never dereferenced

// one source of C channels on an H x W grid; the op's output grid is Ho x Wo inside a TH x TW tensor
static Facts& add_op(int cout, int Ktot, int n_cls, int Ho, int Wo, bool residual, int C0 = 256, int C1 = 0)
{
    g_ops.emplace_back();
    Facts& f = g_ops.back();
    ConvOp& co = f.co;
    co.d.cout = cout; co.cout_pad = (cout + conv_tile_bc(cout) - 1) / conv_tile_bc(cout) * conv_tile_bc(cout);
    co.Ktot = Ktot; co.total_ksteps = Ktot / kBK; co.n_cls = n_cls; co.Ho = Ho; co.Wo = Wo;
    const int step = n_cls == 4 ? 2 : 1;
    co.TH = Ho * step; co.TW = Wo * step; co.d.out_stride_y = co.d.out_stride_x = step;
    co.d.residual_tensor = residual ? 2 : -1; co.d.raw_out_tensor = -1; co.d.out_tensor = 3;
    co.d_fgstep_cls[0] = g_fg;
    co.d.n_src = C1 ? 2 : 1;
    f.tensors.resize(4);
    for (int s = 0; s < co.d.n_src; ++s) {
        Tensor& t = f.tensors[s];
        t.H = Ho; t.W = Wo; t.C = s ? C1 : C0; t.elems_per_patch = (size_t)t.H * t.W * t.C;
        co.d.src[s].tensor = s;
    }
    return f;
}

static void print_case(size_t op, size_t env, sbbseg_ctx& k, int n, int region)
{
    k.tensors = g_ops[op].tensors;
    const ConvForm f = choose_conv(&k, g_ops[op].co, n, region, g_envs[env]);
    printf("S %zu %zu %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %d\n", op, env, k.precision, k.conv_variant, (int)k.ph8, (int)k.plain_gather,
           (int)k.ranged_walk, k.contig_max_k, (int)k.ksplit_now, n, region, f.tile, f.fg, f.fast_gather, f.ks_shift, f.tile_map, f.cls_minor, f.table,
           f.variant_flags);
}

// a handle built by hand: only the knobs choose_conv reads are set.  bits: 0-3 = conv variant bits 2-5, 4 = bit 16, 5 = bit 17, 6 = bit 19,
// 7 = bits 8-15 (K limit 512)
static sbbseg_ctx g_ctx;
static sbbseg_ctx& knobs(int precision, int variant, int bits)
{
    sbbseg_ctx& k = g_ctx;
    k.ksplit_now = false;
    k.precision = precision; k.planes = precision == kF16X3 ? 2 : 1; k.elem = 2;
    k.conv_variant = variant | ((bits & 15) << 2);
    k.ph8 = bits & 16; k.plain_gather = bits & 32; k.ranged_walk = bits & 64; k.contig_max_k = (bits & 128) ? 512 : 0;
    return k;
}

int main()
{
    for (int t = 0; t < kConvTiles; ++t) {
        const ConvTileDims d = kConvTileDims[t];
        printf("T %d %d %d %d %d %d %d %d\n", t, d.bp, d.bc, d.wp, d.wc, d.ns, d.gs, (int)d.ph8);
    }
    // ---- the facts sweep: every cout class x K on each side of 256, 384, 512, 768, 1024, 2048 x residual, on a 28 x 28 grid
    const int couts[] = {32, 64, 128, 384, 256, 512};
    const int Ks[] = {64, 192, 256, 320, 384, 448, 512, 704, 768, 960, 1024, 1280, 1984, 2048, 2112};
    for (int cout : couts)
        for (int K : Ks)
            for (int res = 0; res < 2; ++res) add_op(cout, K, 1, 28, 28, res);
    const size_t n_facts = g_ops.size();
    // ---- the core ops, crossed with every knob
    add_op(256, 1024, 1, 28, 28, false, 256, 64);                     // two sources, long K
    add_op(512, 512, 1, 28, 28, true);                                // the residual rule
    add_op(128, 1280, 4, 14, 14, false, 256, 64);                     // four parity classes, 20 K-steps: split 4, not 8
    add_op(256, 2048, 4, 28, 28, false, 512);
    add_op(128, 576, 2, 28, 28, false);                               // two classes, 9 K-steps: never split
    add_op(128, 384, 3, 28, 28, false);                               // three classes: no class-minor walk
    add_op(64, 576, 1, 56, 56, false, 32);                            // a 64-byte-per-pixel source
    add_op(256, 1152, 1, 28, 28, false, 256, 32);                     // ... as the second source of a 256-channel tile
    add_op(256, 64, 1, 28, 28, false);                                // one K-step
    add_op(256, 1536, 1, 28, 28, false).co.fg_pointwise = true;       // pointwise: fast gather 2; 24 K-steps
    add_op(256, 1024, 1, 28, 28, false).co.d_fgstep_cls[0] = nullptr; // no fast-gather tables
    { ConvOp& co = add_op(32, 576, 1, 56, 56, false, 64).co; co.d.head_classes = 4; }
    add_op(256, 1024, 1, 28, 28, false).co.d.raw_out_tensor = 1;      // a raw output: never split
    add_op(256, 1024, 1, 28, 28, false).co.d.out_tensor = -1;
    { ConvOp& co = add_op(256, 1024, 1, 28, 28, false).co; co.d.out_off_y = 1; }                    // placed: not the whole tensor
    { ConvOp& co = add_op(2048, 4096, 4, 14, 14, false, 1024).co; (void)co; }                      // weights of exactly 16 MB
    add_op(2048, 4160, 4, 14, 14, false, 1024);                       // ... and beyond
    add_op(512, 2048, 1, 28, 28, false);                              // weights of exactly 2 MB (plain modes)
    add_op(1024, 1088, 1, 28, 28, false);                             // ... just beyond
    add_op(136, 1024, 1, 28, 28, false);                              // cout % 8 == 0, no multiple of the tile
    add_op(256, 4096, 1, 28, 28, false);                              // 64 K-steps on 14 tiles: 16 splits
    // a buffer that reaches 2^31 bytes with its bias at n = 1 in the plain modes, and the one a pixel short of it
    for (int short_by = 0; short_by < 2; ++short_by) {
        Facts& f = add_op(256, 1024, 1, 28, 28, false);
        const size_t bias = (size_t)kFgBiasPixels(28) * 256 * 2;
        f.tensors[0].elems_per_patch = (((size_t)1 << 31) - kZeroHeaderBytes - bias) / 2 - short_by;
    }
    for (size_t i = 0; i < g_ops.size(); ++i) {
        const ConvOp& co = g_ops[i].co;
        const Tensor *a = &g_ops[i].tensors[0], *b = &g_ops[i].tensors[1];
        printf("O %zu %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d %d %d %zu\n", i, co.d.cout, co.cout_pad, co.Ktot,
               co.total_ksteps, co.n_cls, co.Ho, co.Wo, co.TH, co.TW, co.d.out_stride_y, co.d.out_stride_x, co.d.out_off_y, co.d.out_off_x,
               (int)(co.d.residual_tensor >= 0), (int)(co.d.raw_out_tensor >= 0), (int)(co.d.out_tensor >= 0), co.d.head_classes,
               (int)(co.d_fgstep_cls[0] != nullptr), (int)co.fg_pointwise, co.d.n_src, a->H, a->W, a->C, a->elems_per_patch, b->H, b->W, b->C,
               b->elems_per_patch);
    }
    // ---- environments: the defaults, then each threshold moved once
    g_envs.emplace_back();
    { ConvEnv e; e.f16_res256_mink = 0; g_envs.push_back(e); }
    { ConvEnv e; e.f16_t256_mink = 1024; g_envs.push_back(e); }
    { ConvEnv e; e.x3_res256_mink = 1024; g_envs.push_back(e); }
    { ConvEnv e; e.x3_t256_mink = 384; g_envs.push_back(e); }
    { ConvEnv e; e.x3_t512_mink = 1024; g_envs.push_back(e); }
    { ConvEnv e; e.pshare_max = (size_t)1 << 20; g_envs.push_back(e); }
    { ConvEnv e; e.split_issue = false; g_envs.push_back(e); }
    for (size_t i = 0; i < g_envs.size(); ++i) {
        const ConvEnv& e = g_envs[i];
        printf("E %zu %d %d %d %d %d %zu %d\n", i, e.f16_res256_mink, e.f16_t256_mink, e.x3_res256_mink, e.x3_t256_mink, e.x3_t512_mink, e.pshare_max,
               (int)e.split_issue);
    }
    const int precisions[] = {(int)kF16, (int)kBF16, (int)kF16X3};
    // n: one patch; 41 / 42 patches of 784 pixels = M on each side of 256 x 128; 64 / 65 = 196 / 200 pixel tiles of 256; 130: 200 tiles of 512
    const int ns[] = {1, 2, 41, 42, 64, 65, 130};
    const int single_bits[] = {0, 1, 2, 4, 8, 16, 32, 64, 128};
    for (size_t op = 0; op < n_facts; ++op)
        for (int precision : precisions) {
            for (int variant = 0; variant < 4; ++variant)
                for (int bits : single_bits)
                    for (int n : ns) {
                        sbbseg_ctx& k = knobs(precision, variant, bits);
                        print_case(op, 0, k, n, -1);
                        if (n == 1) { k.ksplit_now = true; print_case(op, 0, k, n, -1); k.ksplit_now = false; }
                        if (n == 65) { print_case(op, 0, k, n, 3000); print_case(op, 0, k, n, 60000); }
                    }
            for (size_t env = 1; env < g_envs.size(); ++env)
                for (int n : {42, 65, 130}) print_case(op, env, knobs(precision, 0, 0), n, -1);
        }
    for (size_t op = n_facts; op < g_ops.size(); ++op)
        for (int precision : precisions)
            for (int variant = 0; variant < 4; ++variant)
                for (int bits = 0; bits < 256; ++bits) {
                    sbbseg_ctx& k = knobs(precision, variant, bits);
                    print_case(op, 0, k, 65, -1);
                    print_case(op, 0, k, 65, 3000);
                    print_case(op, 0, k, 1, -1);
                    k.ksplit_now = true;
                    print_case(op, 0, k, 1, -1);
                    print_case(op, 0, k, 1, 500);
                    print_case(op, 0, k, 2, -1);
                }
    return 0;
}
"""


def conv_tile_bc(cout):
    return 128 if cout >= 128 else (64 if cout > 32 else 32)


class ParentError(Exception):
    """a launcher of the parent returned hipErrorInvalidValue"""


def parent_params(c, op, env):
    """launch_generic_conv (forward.hip at the parent), statement by statement: the fields of ConvParams the launchers read."""
    cv, x3 = c.conv_variant, c.precision == F16X3
    elem, planes = 2, 2 if x3 else 1
    p = {}
    fg = bool(op.has_fg) and not c.plain_gather
    p["pix_bytes"] = []
    for H, W, C, epp in ((op.H0, op.W0, op.C0, op.epp0), (op.H1, op.W1, op.C1, op.epp1))[:op.n_src]:
        pix_bytes = C * elem * planes
        p["pix_bytes"].append(pix_bytes)
        nbytes = 256 + epp * c.n * elem * planes
        if nbytes + (8 * W + 8) * pix_bytes >= 1 << 31:
            fg = False
    p["fast_gather"] = (2 if op.pointwise else 1) if fg else 0
    p["half_stages"] = 1 if cv & 16 else 0
    p["variant"] = cv & 3
    p["M"] = c.n * op.Ho * op.Wo
    p["variant_flags"] = (1 if cv & 64 else 0) | (2 if cv & 128 else 0) | (4 if c.ph8 else 0)
    wbytes = op.cout_pad * op.Ktot * elem
    p["tile_map"] = 1 if (((cv & 32) or x3) and not (cv & 8) and (cv & 4) == 0 and op.cout > conv_tile_bc(op.cout) and p["M"] >= 256 * 128
                          and wbytes <= env.pshare_max) else 0
    if p["tile_map"] == 1 and op.n_cls == 1 and op.Ktot <= c.contig_max_k:
        p["tile_map"] = 2
    p["cls_minor"] = 0
    if op.n_cls > 1 and (op.n_cls & (op.n_cls - 1)) == 0 and not (cv & 8) and not (cv & 4) and wbytes <= 16 << 20:
        p["cls_minor"] = 1
        p["tile_map"] = 3 if c.ranged_walk else 1
    p["rmap"] = 0
    if c.region >= 0:
        if p["fast_gather"] and not p["half_stages"] and p["variant"] != 2 and not (p["variant_flags"] & 4):
            p["rmap"], p["M"] = 1, c.region
    ks = 0
    if (c.ksplit_now and c.n == 1 and c.precision != F32 and p["fast_gather"] and conv_tile_bc(op.cout) == 128 and not op.raw_out
            and not op.head_classes and op.out and op.cout % 8 == 0
            and ((op.n_cls == 1 and op.osy == 1 and op.osx == 1 and op.ooy == 0 and op.oox == 0 and op.TH == op.Ho and op.TW == op.Wo)
                 or (op.n_cls == 4 and op.osy == 2 and op.osx == 2 and op.TH == 2 * op.Ho and op.TW == 2 * op.Wo))):
        tiles = op.n_cls * ((p["M"] + 127) // 128) * ((op.cout + 127) // 128)
        while ks < 4 and (tiles << (ks + 1)) <= 512 and op.total_ksteps % (2 << ks) == 0 and (op.total_ksteps >> (ks + 1)) >= 4:
            ks += 1
    p["ks_shift"] = ks
    if ks > 0:
        p["tile_map"] = p["cls_minor"] = 0
    return p


def parent_launch(c, op, env, p):
    """launch_conv and below (kernels.hip at the parent) -> ((BP, BC, WP, WC, NS, GS, PH8), FG, KS) of the instantiation launched."""
    cout, Ktot, M, n_cls, residual = op.cout, op.Ktot, p["M"], op.n_cls, op.residual
    bc = conv_tile_bc(cout)

    def launch_conv_t(BP, BC, WP, WC, NS, GS=8, PH8=0):
        if not PH8 and GS == 8 and NS == 2 and p["fast_gather"]:
            return (BP, BC, WP, WC, NS, GS, PH8), 1, 0
        if p["rmap"]:
            raise ParentError("an owned-region table for a tile without a fast-gather form")
        return (BP, BC, WP, WC, NS, GS, PH8), 0, 0

    def split_k():
        if bc != 128 or not p["fast_gather"] or p["tile_map"] != 0 or p["cls_minor"] or (op.total_ksteps & ((1 << p["ks_shift"]) - 1)):
            raise ParentError("a split-K launch the caller should not have asked for")
        return (128, 128, 2, 2, 2, 8, 0), 1, 1

    def ph8_ok():
        if not (p["variant_flags"] & 4) or op.total_ksteps < 2 or p["half_stages"] or p["rmap"]:
            return False
        return all(b >= 128 for b in p["pix_bytes"])

    t256 = n_cls * ((M + 255) // 256) * (cout // 256)
    t512 = n_cls * ((M + 511) // 512) * ((cout + 127) // 128)
    if c.precision == F16X3:                                      # launch_conv_x3
        if p["ks_shift"] > 0:
            return split_k()
        if (p["variant"] == 0 and bc == 128 and residual and env.x3_res256 > 0 and cout % 256 == 0 and Ktot >= env.x3_res256 and t256 >= 200):
            return launch_conv_t(256, 256, 2, 4, 2)
        if p["variant"] == 0 and bc == 128 and not residual:
            if cout % 256 == 0 and Ktot >= env.x3_t256 and t256 >= 200:
                return launch_conv_t(256, 256, 2, 4, 2)
            if Ktot >= env.x3_t512 and t512 >= 200:
                return launch_conv_t(512, 128, 4, 2, 2)
        if bc == 128:
            return launch_conv_t(128, 128, 2, 2, 2)
        if bc == 64:
            return launch_conv_t(256, 64, 4, 1, 2)
        return launch_conv_t(256, 32, 4, 1, 2)
    # launch_conv_16
    variant = p["variant"]
    big = variant == 2
    if p["ks_shift"] > 0:
        return split_k()
    if p["half_stages"]:
        if bc == 128 and not residual and cout % 256 == 0 and Ktot >= 512 and t256 >= 200:
            return launch_conv_t(256, 256, 2, 4, 4, GS=4)
        if bc == 128:
            return launch_conv_t(128, 128, 2, 2, 4, GS=4)
        if bc == 64:
            return launch_conv_t(256, 64, 4, 1, 4, GS=4)
    if variant == 3:
        if bc == 128 and cout % 256 == 0:
            return launch_conv_t(256, 256, 2, 4, 2, PH8=1) if ph8_ok() else launch_conv_t(256, 256, 2, 4, 2)
        if bc == 128:
            return launch_conv_t(512, 128, 4, 2, 2)
        if bc == 64:
            return launch_conv_t(512, 64, 8, 1, 2)
    if (variant == 0 and bc == 128 and residual and env.f16_res256 > 0 and cout % 256 == 0 and Ktot >= env.f16_res256 and t256 >= 200):
        return launch_conv_t(256, 256, 2, 4, 2)
    if variant == 0 and bc == 128 and not residual:
        if cout % 256 == 0 and Ktot >= env.f16_t256 and t256 >= 200:
            return launch_conv_t(256, 256, 2, 4, 2, PH8=1) if ph8_ok() else launch_conv_t(256, 256, 2, 4, 2)
        if Ktot >= 1024 and t512 >= 200:
            return launch_conv_t(512, 128, 4, 2, 2)
    if bc == 128:
        return launch_conv_t(256, 128, 4, 2, 3) if big else launch_conv_t(128, 128, 2, 2, 2)
    if bc == 64:
        return launch_conv_t(256, 64, 8, 1, 3) if big else launch_conv_t(256, 64, 4, 1, 2)
    return launch_conv_t(256, 32, 8, 1, 3) if big else launch_conv_t(256, 32, 4, 1, 2)


def parent_form(c, op, env):
    """-> (tile dims, FG, fast_gather, ks_shift, tile_map, cls_minor, table, variant_flags as the kernel gets them)"""
    p = parent_params(c, op, env)
    dims, fg, ks = parent_launch(c, op, env, p)
    flags = p["variant_flags"] | (8 if c.precision != F16X3 and not env.split_issue else 0)        # launch_conv: SBBSEG_SPLIT_ISSUE, plain modes
    assert ks == (p["ks_shift"] > 0)
    return dims, fg, p["fast_gather"], p["ks_shift"], p["tile_map"], p["cls_minor"], p["rmap"], flags


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("conv_choice")
    (d / "probe.cpp").write_text(_PROBE)
    # conv_choice.h is host only: it must compile without the device pass and run without the HIP runtime being called
    res = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-3000:]              # (a sanitizer report ends the program with a status)
    tiles, ops, envs, cases = {}, {}, {}, []
    for line in out.stdout.splitlines():
        kind, *f = line.replace(":", " ").split()
        v = [int(x) for x in f]
        if kind == "T":
            tiles[v[0]] = tuple(v[1:])
        elif kind == "O":
            ops[v[0]] = Op(*v[1:])
        elif kind == "E":
            envs[v[0]] = Env(*v[1:])
        else:
            cases.append((Case(*v[:11]), Form(*v[11:])))
    return tiles, ops, envs, cases


def test_header_is_host_only():
    text = open(os.path.join(CSRC, "conv_choice.h")).read()
    assert re.findall(r'#\s*include\s+"([^"]+)"', text) == ["ctx.h"]
    for word in ("HIPCHK", "REQUIRE", "hipMemcpy", "hipMalloc", "hipLaunch", "<<<"):
        assert word not in text, word


def test_the_tile_table_is_the_thirteen_instantiated_forms(sweep):
    tiles = sweep[0]
    assert sorted(tiles) == list(range(13)) and sorted(tiles.values()) == sorted(TILES_16) and len(SYMBOLS) == 51


def test_forms_match_the_parent_ladders(sweep):
    tiles, ops, envs, cases = sweep
    assert envs[0] == DEFAULT_ENV
    bad = []
    for c, got in cases:
        op, env = ops[c.op], envs[c.env]
        want = parent_form(c, op, env)                            # (raises where the parent's launchers would have returned an error)
        have = (tiles[got.tile],) + tuple(got[1:])
        if have != want:
            bad.append((c, op, have, want))
    assert not bad, (len(bad), bad[:4])


def test_the_sweep_is_complete(sweep):
    tiles, ops, envs, cases = sweep
    assert len(cases) > 100000
    seen = lambda f: {f(c, ops[c.op], envs[c.env], g) for c, g in cases}
    # the knobs, crossed
    assert seen(lambda c, o, e, g: (c.precision, c.conv_variant & 3, (c.conv_variant >> 2) & 15, c.ph8, c.plain_gather, c.ranged_walk, c.contig_max_k > 0)) \
        >= {(p, v, b, a, g_, r, k) for p in MODES for v in range(4) for b in range(16) for a in (0, 1) for g_ in (0, 1) for r in (0, 1) for k in (False, True)}
    assert seen(lambda c, o, e, g: (c.ksplit_now, c.n == 1, c.region >= 0)) >= {(1, True, False), (1, True, True), (0, True, False), (0, False, True), (0, False, False)}
    # the op facts: both sides of every comparison in the rule
    assert seen(lambda c, o, e, g: o.cout) >= {32, 64, 128, 384, 256, 512}
    for k in (256, 384, 512, 768, 1024, 2048):
        assert seen(lambda c, o, e, g: (o.Ktot >= k, o.Ktot >= k - 64)) >= {(False, False), (True, True), (False, True)}, k
    t256 = lambda c, o: o.n_cls * -(-c.n * o.Ho * o.Wo // 256) * (o.cout // 256)
    t512 = lambda c, o: o.n_cls * -(-c.n * o.Ho * o.Wo // 512) * -(-o.cout // 128)
    assert seen(lambda c, o, e, g: (o.cout % 256 == 0 and t256(c, o) >= 200, o.cout % 256 == 0 and 0 < t256(c, o) < 200)) >= {(True, False), (False, True)}
    assert seen(lambda c, o, e, g: t512(c, o) >= 200) == {True, False}
    assert seen(lambda c, o, e, g: c.n * o.Ho * o.Wo >= 256 * 128) == {True, False}
    wb = lambda o: o.cout_pad * o.Ktot * 2
    assert seen(lambda c, o, e, g: (wb(o) < 2 << 20, wb(o) == 2 << 20, wb(o) > 2 << 20)) >= {(True, False, False), (False, True, False), (False, False, True)}
    assert seen(lambda c, o, e, g: (o.n_cls, wb(o) == 16 << 20, wb(o) > 16 << 20)) >= {(4, True, False), (4, False, True), (4, False, False)}
    assert seen(lambda c, o, e, g: o.n_cls) >= {1, 2, 4} and seen(lambda c, o, e, g: o.residual) == {0, 1}
    assert seen(lambda c, o, e, g: (c.precision != F16X3 and min(o.C0, o.C1 or o.C0) * 2 == 64, c.ph8)) >= {(True, 1)}
    assert seen(lambda c, o, e, g: o.total_ksteps == 1) == {True, False}
    assert seen(lambda c, o, e, g: (c.ksplit_now, g.ks_shift, o.total_ksteps % (2 << g.ks_shift) != 0)) >= {(1, 2, True), (1, 0, True)}
    edge = lambda c, o: 256 + o.epp0 * c.n * 2 * (2 if c.precision == F16X3 else 1) + (8 * o.W0 + 8) * o.C0 * 2 * (2 if c.precision == F16X3 else 1)
    assert seen(lambda c, o, e, g: (edge(c, o) == 1 << 31, g.fast_gather)) >= {(True, 0)}
    assert seen(lambda c, o, e, g: ((1 << 31) - edge(c, o) in (1, 2), g.fast_gather)) >= {(True, 1)}
    # every environment threshold moves some choice: the same case under the defaults and under the moved value
    by_case = {}
    for c, g in cases:
        by_case.setdefault(c._replace(env=0), {})[c.env] = g
    moved = {e for forms in by_case.values() for e, g in forms.items() if 0 in forms and g != forms[0]}
    assert moved == set(envs) - {0}, sorted(set(envs) - {0} - moved)
    # the forms
    mode = lambda c: MODES[c.precision]
    assert seen(lambda c, o, e, g: g.tile if c.precision != F16X3 else -1) >= set(range(13))
    assert {tiles[t] for t in seen(lambda c, o, e, g: g.tile if c.precision == F16X3 else 0)} == set(TILES_X3)
    assert seen(lambda c, o, e, g: g.fast_gather) == {0, 1, 2}
    assert seen(lambda c, o, e, g: (c.precision == F16X3, g.ks_shift > 0)) >= {(True, True), (False, True)}
    assert seen(lambda c, o, e, g: g.ks_shift) == {0, 1, 2, 3, 4}
    assert seen(lambda c, o, e, g: g.tile_map) == {0, 1, 2, 3} and seen(lambda c, o, e, g: (g.table, c.region >= 0)) >= {(1, True), (0, True), (0, False)}
    reached = seen(lambda c, o, e, g: (tiles[g.tile], mode(c), g.fg, int(g.ks_shift > 0)))
    assert reached == SYMBOLS, (sorted(reached - SYMBOLS), sorted(SYMBOLS - reached))


def test_what_the_sweep_pins(sweep):
    """the corners of the parent's rule that nothing else states, on the header's own output"""
    tiles, ops, envs, cases = sweep
    for c, g in cases:
        o = ops[c.op]
        dims = tiles[g.tile]
        half, variant = c.conv_variant & 16, c.conv_variant & 3
        if c.region >= 0:                                        # withheld under bit 4, variant 2, bit 16 -- whatever tile is finally taken
            assert g.table == int(bool(g.fast_gather) and not half and variant != 2 and not c.ph8), (c, g)
        if g.table:                                              # a table goes to a fast-gather instantiation only
            assert g.fg == 1
        assert g.fg == int(g.fast_gather > 0 and (g.ks_shift > 0 or (dims[4] == 2 and dims[5] == 8 and not dims[6]))), (c, g)
        if g.ks_shift:
            assert (g.tile_map, g.cls_minor, dims) == (0, 0, TILES_16[0]) and c.ksplit_now and c.n == 1
        if dims[6]:                                              # the 8-phase form
            assert c.ph8 and o.total_ksteps >= 2 and not half and not g.table and c.precision != F16X3 and min(o.C0, o.C1 or o.C0) * 2 >= 128
        if c.precision == F16X3:                                 # bit 4, variant 2 and variant 3 choose no tile in the split mode
            assert dims in TILES_X3
        if c.plain_gather or not o.has_fg:
            assert g.fast_gather == 0
        if o.pointwise and g.fast_gather:
            assert g.fast_gather == 2
        assert bool(g.variant_flags & 8) == (not envs[c.env].split_issue and c.precision != F16X3)
