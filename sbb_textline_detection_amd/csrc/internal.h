// internal.h -- structures shared by the host side (api.hip, forward.hip, pages.hip, whole.hip, comm.hip, plan_build.hip, stage_glue.hip and contour_glue.hip
// through ctx.h; wpack.h) and the gfx950 kernel units (kernels.hip and the other *.hip around it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sbbseg.h"

namespace sbbseg {

// Every activation buffer starts with a zeroed header; gather lanes that fall into padding (conv
// zero padding, one_side_pad, K padding) read their 16 bytes from offset 0 of the buffer instead
// of branching -- global_load_lds cannot predicate per lane.
constexpr int kZeroHeaderBytes = 256;
constexpr int kBK = 64;               // contraction elements per K-step (8 granules of 8 bf16 = 16 B)
constexpr int kGranulesPerStep = 8;

struct SrcDesc {
    const char* base;     // buffer start (zero header first, data at +kZeroHeaderBytes)
    int PH, PW;           // stored (physical) height / width per patch
    int pix_bytes;        // bytes per stored pixel (channels * elem size)
    int shift;            // nearest upsampling log2 (0|1)
    int lim_y, lim_x;     // PH << shift, PW << shift
    int ksteps;           // K-steps contributed by this source
    int sy_shift, sx_shift; // log2 of this source's input step per output step (stride 1|2); the
                          // source's padding and placement offset are folded into the tap table
    int lo_off;           // byte distance from slot 0-3's granules to slot 4-7's inside a K-step: 64 (the next four
                          // 8-channel granules) in the plain modes; channels * 2 in the split mode (the "lo" plane
                          // of the same 32 channels, see kF16X3)
    uint32_t bytes;       // bytes of the buffer in use (header + the launch's patches): num_records of the fast gather
    int tap_lo_y, tap_lo_x; // fast gather: smallest tap offset of this source over all K-steps / classes (its taps span <= 4 x 4)
};

// one entry per 16-byte granule of the contraction axis
struct KTabEntry {
    int16_t dy, dx;       // tap offset minus the source's placement offset
    int32_t coff;         // byte offset of the granule inside the stored pixel
};

// one record per K-step, read through the scalar cache.  Regular step: all 8 granules share the tap
// (dy,dx) and are channel-consecutive (coff + 16*g).  Irregular: per-granule KTabEntry applies.
struct KStepRec {
    int16_t dy, dx;
    int32_t coff;
    int32_t irregular;
    int32_t pad_;
};

// fast gather (ConvParams::fast_gather): the table handed to the kernel in place of the KStepRec table, same stride.
// A source's buffer resource starts kFgBiasPixels(PW) pixels before the buffer, so `soff` is never negative.
struct FgStepRec {
    uint32_t soff;        // dy * row bytes + dx * pixel bytes + channel byte offset + kFgBiasPixels(PW) * pixel bytes
    int32_t tapbit;       // source * 16 + (dy - tap_lo_y) * 4 + (dx - tap_lo_x): bit of this tap in a row's out-of-bounds mask
    int32_t pad_[2];
};
__host__ __device__ constexpr int kFgBiasPixels(int PW) { return 8 * PW + 8; }   // covers taps down to (-8, -8)

struct ConvParams {
    SrcDesc src[2];
    int n_src;
    const KStepRec* kstep;    // [total_ksteps]
    int variant;              // 0 = auto tile choice, 1 = force 4-wave/2-stage, 2 = force 8-wave/3-stage
    int half_stages;          // A/B: half-K-step LDS stages in a 4-deep ring
    int variant_flags;        // A/B switches: bit 0 = drain the epilogue stores before the next barrier, bit 1 = half-line epilogue stores (old behaviour), bit 2 = 8-phase schedule on the 256x256 tile
    int tile_map;             // 0 = channel tile per XCD (big weights), 1 = pixel tiles grouped per XCD (small weights)
    int persist_blocks;       // CUs of the device (persistent grid = resident blocks); 0 = one block per tile
    const KTabEntry* ktab;    // [total_ksteps * 8]
    const void* w;            // packed [cout_pad][Ktot] (bf16) -- K order = ktab order
    int Ktot;                 // total_ksteps * 64
    int total_ksteps;
    int M;                    // batch * Ho * Wo output pixels of THIS op's output grid
    int Ho, Wo;
    // placement of the op's output grid inside the output tensor(s): tensor[y*osy+ooy][x*osx+oox]
    // (1,1,0,0 = the whole tensor; the parity-split decoder convs write every second pixel)
    int TH, TW, osy, osx, ooy, oox;
    int cout;                 // real output channels (multiple of 8)
    const float* scale;       // [cout_pad]
    const float* shift;
    void* out;                // data pointer (header skipped), [M][cout]; may be null
    const void* residual;     // same shape as out, or null
    void* raw_out;            // or null
    const float* raw_scale;
    const float* raw_shift;
    int relu;
    // output-placement classes sharing all geometry (the four parity classes of a decoder conv run as
    // ONE launch): class q has its own weights / tap tables / placement offset; class 0 = the fields above
    int n_cls;
    int cls_minor;            // tile order: 0 = class-major, 1 = classes of a pixel tile adjacent (needs tile_map 1)
    const void* w_cls[4];
    const KStepRec* kstep_cls[4];
    const KTabEntry* ktab_cls[4];
    int ooy_cls[4], oox_cls[4];
    // fused head (cout == 32 tiles only): 1x1 conv + BN + softmax + argmax on the fp32 epilogue values
    float wmul_cls[4];        // per-class multiplier of `scale` (split mode: 2^-s of the power-of-two weight pre-scale; else 1)
    int head_classes;         // 0 = none
    const float* head_w;      // [cout][classes]
    const float* head_scale;  // [classes]
    const float* head_shift;
    uint8_t* labels;          // [n][TH][TW]
    float* probs;             // [n][TH][TW][classes] or null
    uint32_t howo_magic, howo_shift, wo_magic, wo_shift, nct_magic, nct_shift;   // FastDiv pairs for Ho * Wo, Wo and the number of
                                                           // channel tiles, filled by the launcher (kernels.hip)
    const FgStepRec* fgstep_cls[4];   // fast gather: per-class tables read in place of kstep / kstep_cls (class 0 = entry 0)
    int fast_gather;          // every K-step regular, each source's taps within a 4 x 4 window, no upsampling source, buffers < 2 GiB:
                              // run the FG form of conv_igemm_mfma (kernels.hip)
    // split-K (one-patch launches of the whole-image branch, 16-bit and split modes): 2^ks_shift blocks share a tile's K-steps, each writes its fp32
    // partial sums (x the class's power-of-two weight scale) to ks_ws[split][output pixel][cout]; splitk_finish adds them in split order
    // and runs the epilogue.  0 = off
    int ks_shift;
    float* ks_ws;
    long ks_split_elems;      // floats per split = output pixels of the tensor x cout
    // owned-region launch (region.h): the output grid is not walked whole -- pixel index m of class q is the rmap[q * M + m]-th entry of a
    // per-launch table of (patch, oy, ox) triples (kRegionCode) that lists, patch by patch, only the class-grid pixels the page stitch
    // will keep plus the halo the later decoder levels need; M = entries per class.  null = the whole grid (m = (n * Ho + oy) * Wo + ox)
    const uint32_t* rmap;
};

// fused network tail: 3x3 conv over [nearest-x2-upsampled src0 (64 ch), image C8 (3 ch)] -> 32 ch
// -> BN/ReLU -> 1x1 head -> softmax -> argmax, one launch, nothing but labels (and optional
// probabilities) written.  See dec_tail_fused in dec_tail.hip.
struct TailParams {
    const char* src0;         // buffer start (zero header), [n][PH][PW][64] 16-bit
    const char* img;          // buffer start (zero header), C8 form [n][2PH][2PW][8] (split mode: hi slots 4..6 repeat lo 0..2)
    int PH, PW;               // src0 size; output is 2PH x 2PW
    int n;                    // patches
    const void* wfrag;        // [4 parities][6 K-steps][2 kk][2 mi][64 lanes] x 16 bytes, MFMA A-fragment order (split mode: per parity
                              // [hi | lo][5 K-steps][2 kk][2 mi][64 lanes], the image taps packed two to a k-group: sbbseg_add_tail)
    const float* scale;       // [32]
    const float* shift;
    int classes;              // <= 4
    const float* head_w;      // [32][classes]
    const float* head_scale;
    const float* head_shift;
    uint8_t* labels;          // [n][2PH][2PW]
    float* probs;             // [n][2PH][2PW][classes] or null
    // owned-region launch (region.h): the launch walks `n_tab` 16 x 16 output tiles listed in ttab (kRegionCode: patch, tile origin / 2)
    // instead of every tile of every patch; null = all tiles
    const uint32_t* ttab = nullptr;
    int n_tab = 0;
};

// Network stem: 7x7 stride-2 conv on the image in the PAIRS input form (7 rows x 4 two-pixel granules
// of 8 values) -> 64 channels, per-channel affine (+ ReLU), 16-bit NHWC.  See stem_conv_pairs.
struct StemParams {
    const char* pairs;        // buffer start (zero header), [n][PHt][PWt][8] 16-bit
    int PHt, PWt;             // padded rows, two-pixel granules per row
    int n;                    // patches
    int Ho, Wo;               // output size, multiples of 16
    const void* wfrag;        // [7 ky][4 mi][64 lanes] x 16 bytes, MFMA A-fragment order, rows = conv_row_channel
                              // (split mode: that block twice -- hi fragments, then lo fragments of the pre-scaled weights)
    const float* scale;       // [64]
    const float* shift;
    int relu;
    float wmul;               // multiplier of `scale` (split mode: 2^-s of the weight pre-scale; else 1)
    void* out;                // data pointer [n][Ho][Wo][64]
    // stem_pool_x3 (stem_pool_x3.hip): the 3x3 / stride-2 / valid max-pool over ReLU(pool_scale * f1 + pool_shift) written by the same launch
    void* pool_out = nullptr; // data pointer [n][pool_Ho][pool_Wo][64], or null (plain stem)
    const float* pool_scale = nullptr;      // [64] the affine maxpool_kernel applies to every tap (bn_conv1)
    const float* pool_shift = nullptr;
    int pool_relu = 0;
    int pool_Ho = 0, pool_Wo = 0;
    int x3 = 1;               // stem_pool: 1 = split mode (hi | lo planes), 0 = plain fp16
};

// 3x3 stride-1 'same' conv, 64 -> 64 channels (the ResNet stage-2 bottleneck convs), as a direct conv on an
// LDS halo tile with the weights resident in registers.  See conv3x3_c64_direct.
struct Direct64Params {
    const char* src;          // buffer start (zero header), [n][H][W][64] 16-bit
    int n, H, W;
    const void* wfrag;        // [9 taps][2 kk][4 mi][64 lanes] x 16 bytes, MFMA A-fragment order, rows = conv_row_channel;
                              // split mode: that block twice (hi fragments, then lo fragments of the pre-scaled weights)
    const float* scale;       // [64]
    const float* shift;
    int relu;
    float wmul;               // multiplier of `scale` (split mode: 2^-s of the power-of-two weight pre-scale; else 1)
    void* out;                // data pointer [n][H][W][64] (split mode: [64 hi][64 lo] per pixel)
};

// Split mode (kF16X3) pixel layout (round 3): a stored pixel of C channels is a sequence of channel GROUPS of G = min(C, 32)
// channels, each group = [G hi halves][G lo halves] -- for C >= 32 one 128-byte line per group, which is exactly what a split K-step
// (32 channels of one tap, hi and lo) reads.  (Round 2 stored [C hi][C lo]: a K-step then touched two half-used lines per pixel,
// doubling the L2 footprint of every gather and fetching every line twice -- PMC: 2-6x the unique bytes on the decoder launches.)
#if defined(__HIPCC__)
#define SBBSEG_HD __host__ __device__
#else
#define SBBSEG_HD
#endif
SBBSEG_HD inline int split_group(int C) { return C < 32 ? C : 32; }                      // channels per group = distance (in halves) hi -> lo
SBBSEG_HD inline int split_hi_elem(int C, int ch)                                         // index (in halves) of channel ch's hi half inside the pixel
{
    const int G = split_group(C);
    return (ch / G) * 2 * G + (ch % G);
}

// One ResNet bottleneck block at 64 internal channels (1x1 -> 3x3 -> 1x1 + shortcut) as ONE launch.  See bottleneck_fused.
struct BlockParams {
    const char* x;            // buffer start (zero header), [n][H][W][CIN] 16-bit; CIN = 256 (identity) | 64 (projection)
    int n, H, W;
    int proj;                 // 0: y = ReLU(BN(W3 b) + x);  1: y = ReLU(BN(W3 [b, x]))  (shortcut conv folded by the planner)
    int pq;                   // 1: bottleneck_fused_pq (producer / consumer wave groups), 0: bottleneck_fused
    const void* w1;           // [CIN/32 kk][4 mi][64 lanes] x 16 bytes, MFMA A-fragment order, rows = conv_row_channel
    const void* w2;           // [9 taps][2 kk][4 mi][64 lanes] x 16 bytes (Direct64Params::wfrag)
    const void* w3;           // [2|4 kk][16 mi][64 lanes] x 16 bytes; projection: kk 0-1 contract b, kk 2-3 contract x
    const float *s1, *b1;     // [64]  scale / shift after the first 1x1
    const float *s2, *b2;     // [64]  ... after the 3x3
    const float *s3, *b3;     // [256] ... after the last 1x1 (before the residual add)
    void* out;                // data pointer [n][H][W][256]
    // split mode (block_x3_identity, block_x3.hip): w1 = [8 kk][4 mi][hi | lo][64 lanes] x 16 B, w3 = [2 kk][16 mi][hi | lo][64 lanes] x 16 B,
    // w2 = [hi | lo][9][2][4 mi][64 lanes] x 16 B, every conv's weights pre-scaled by a power of two; wmulN = 2^-s undoes it in sN
    float wmul1 = 1.f, wmul2 = 1.f, wmul3 = 1.f;
    int dbg = 0;              // timing probes (SBBSEG_BLOCK_DBG; results are WRONG with any bit set): 1 = LDS rows rotated by 1 slot per row on the WRITE side only
    // conv variant bit 26 (16-bit modes only; null otherwise): data pointers [n][H][W][64] of the plan tensors of a and b.  Non-null selects the
    // DUMP instantiation of bottleneck_fused*, which also stores what phases A and B pack for the pixels inside the image (tests/test_gpu_steps_blocks.py)
    void* dump_a = nullptr;
    void* dump_b = nullptr;
};

// The decoder conv at 224 x 224 in the split mode with LDS-resident source halos (dec_halo_x3.hip): the grouped launch of the four
// output-parity classes of  conv3x3([up2(src0: 128 ch), skip: 64 ch]) -> 64 ch  as ONE direct kernel on 16 x 16 output tiles.
struct DecHaloParams {
    const char* src0;         // buffer start (zero header), [n][PH][PW][128] split layout (512 B per pixel)
    const char* skip;         // buffer start (zero header), [n][2 PH][2 PW][64] split layout (256 B per pixel)
    int PH, PW, n;
    const void* wfrag;        // [4 classes][34 K-steps][4 row blocks][hi | lo][64 lanes] x 16 B: MFMA A fragments of the classes' packed weights
    const int* taps;          // [4 classes][16]: the class's 4 src0 taps, then its 9 skip taps, in K-step order: (dy & 255) | (dx & 255) << 8
    const float* scale;       // [64]
    const float* shift;
    float wmul[4];            // per class: 2^-s of its power-of-two weight pre-scale
    int relu;
    void* out;                // data pointer [n][2 PH][2 PW][64] split layout
    const uint32_t* ttab = nullptr;      // owned-region launch: see TailParams
    int n_tab = 0;
};

// Split mode, stages 3 / 4 of the encoder: the last 1x1 conv of an identity bottleneck block (C -> 4C, BN, + residual, ReLU) and the first
// 1x1 conv of the next block (4C -> C, BN, ReLU) in one launch (expand_reduce_x3.hip): y is written once and contracted from LDS.
struct ExpRedParams {
    const char* b;            // buffer start (zero header), [M][C] split layout: the expand's input
    const char* x;            // buffer start (zero header), [M][4C]: the residual
    char* y;                  // buffer start (zero header), [M][4C]: the expand's output
    char* a2;                 // buffer start (zero header), [M][C]: the reduce's output
    int M;                    // pixels (patches x H x W)
    int C;                    // 128 | 256
    int x3;                   // 1: split mode (hi | lo planes); 0: plain fp16 (the fragment pairs are the two k-halves of a 64-channel K-step)
    const void* w3frag;       // [4C / 256 chunks][C / 32 K-steps][8 waves][2 row blocks][hi | lo][64 lanes] x 16 B: A fragments of the expand's packed rows
    const void* w1frag;       // [4C / 256 chunks][8 K-steps][8 waves][C / 128 row blocks][hi | lo][64 lanes] x 16 B: ... of the reduce's
    const float *s3, *h3;     // [4C] scale / shift of the expand
    const float *s1, *h1;     // [C]  ... of the reduce
    float wmul3, wmul1;       // 2^-s of the power-of-two weight pre-scales
    int dbg;                  // timing probes (SBBSEG_ER_DBG; results are WRONG with any bit set): 1 = one weight block, 2 = y stores dropped, 4 = x reads dropped
};

// Encoder stage 3: an identity block's 3x3 conv + its last 1x1 conv + the next block's first 1x1 conv in one launch
// (conv3_expand_reduce.hip): b = ReLU(BN(W2 * a)) lives in LDS only.
struct C3ERParams {
    const char* a;            // buffer start (zero header), [n][H][W][C]: the 3x3 conv's input
    const char* x;            // buffer start (zero header), [n][H][W][4C]: the residual
    char* y;                  // buffer start (zero header), [n][H][W][4C]
    char* a2;                 // buffer start (zero header), [n][H][W][C]: the reduce's output
    int n, H, W;              // H, W multiples of 8
    int C;                    // 128
    int x3;                   // 1: split mode; 0: plain fp16
    const void* w2frag;       // [9 C / KCH K-steps][8 waves][C / 128 row blocks][hi | lo][64 lanes] x 16 B: A fragments of the 3x3 conv's packed rows, its K order
    const void* w3frag;       // as ExpRedParams
    const void* w1frag;
    const float *s2, *h2;     // [C] scale / shift of the 3x3 conv
    const float *s3, *h3;     // [4C]
    const float *s1, *h1;     // [C]
    float wmul2, wmul3, wmul1;
    const int* k0;            // device [9 C / KCH]: the 3x3 conv's K-steps in its own order: (dy & 255) | (dx & 255) << 8 | channel group << 16
};

struct HeadParams {
    const void* src;          // [M][cin] activations (data pointer)
    int cin;                  // <= 64, multiple of 8
    int classes;              // <= 8
    int M;
    const float* w;           // [cin][classes]
    const float* scale;       // [classes]
    const float* shift;
    uint8_t* labels;          // [M]
    float* probs;             // [M][classes] or null
};

struct IngestParams {
    const uint8_t* page;      // [src_Hp][src_Wp][3] u8 (device)
    int Hp, Wp;               // size of the (virtual) page the tile grid lives on
    int src_Hp, src_Wp;       // size of the stored page (== Hp, Wp unless a nearest-resize map is given)
    int whole;                // 1: one patch = the whole page resized to the model input (maps indexed by model coords)
    const int* tile_xy;       // device [n][2] explicit origins, or null = closed-form grid below
    int grid_first, grid_nyf; // grid mode: tile t = grid_first + local index; i = t / nyf, j = t % nyf
    int grid_mid_x, grid_mid_y; //   origin = min(i*mid_x, Wp-W), min(j*mid_y, Hp-H)   (main.py:262-281)
    int n_tiles;
    int H, W;                 // model input size
    const float* lut;         // [256] float32(v / 255.0)
    void* c8;                 // data pointer of the C8 form  [n][H][W][8]
    void* pairs;              // data pointer of the PAIRS form [n][H+2p][PWp][8]; may be null
    int pad, pairs_w;         // p, ceil((W+2p)/2)
    const int* map_y;         // optional nearest-resize gather tables (whole-image branch) or null
    const int* map_x;
    const int* bin_thr;       // device int: binarise channel 0 at this (Otsu) threshold into all 3 channels, or null
};

// kF16X3: error-compensated fp16 ("split") mode.  Every activation and weight v is carried as two fp16 numbers
// hi = fp16(v), lo = fp16(v - hi) (about 22 significant bits together); a product is three MFMAs
// (hi*hi + hi*lo + lo*hi, fp32 accumulate), the dropped lo*lo term is ~2^-22 relative.  Activations are stored
// per pixel as [C hi][C lo] (4 bytes per element), weights per 32-channel K-step as [32 hi][32 lo] after a
// power-of-two pre-scale that keeps their lo parts out of the fp16 subnormal range.
enum Precision { kBF16 = 0, kF32 = 1, kF16 = 2, kF16X3 = 3 };

// Timing probes that make a kernel compute WRONG results on purpose (every pixel gather an L2 hit, one weight block, stores dropped ...)
// exist only in probe builds (`python -m sbb_textline_detection_amd._build --probes`: -DSBBSEG_PROBES, a separate library under
// tools/probes/bin/); in the shipped library the conditions below are the constant `false` and the environment variables that used to
// switch them (SBBSEG_CONV_PROBE_LOCAL / _WHOT, SBBSEG_BLOCK_DBG, SBBSEG_ER_DBG) are not read at all.
#ifdef SBBSEG_PROBES
#define SBBSEG_PROBE(cond) (cond)
#else
#define SBBSEG_PROBE(cond) (false)
#endif
inline bool is_split(int precision) { return precision == kF16X3; }

// What the last launch of a plan op used (sbbseg_debug_op_launch; the field order is the order of the ints it returns, the family numbers are
// SBBSEG_LAUNCH_* of sbbseg.h).  Every launcher fills the record it is handed where it sizes its grid -- plain host stores into the Op, nothing
// is read back from the device and nothing waits.  persistent = 1: the grid is sized by the CU count and a block loops over the work items
// b, b + G, ... or over a run of them; 0: one block per fixed slice of the output, no loop to carry state through.
struct LaunchRec {
    int family = 0;
    int bp = 0, bc = 0, stages = 0;       // conv_igemm_mfma: pixels x channels of the tile, LDS stages; the direct kernels: output pixels of a work item, channels, 1
    int fast_gather = 0, tile_map = 0, cls_minor = 0;       // conv_igemm_mfma only (ConvParams)
    int table = 0;                        // an owned-region table was passed (ConvParams::rmap, ttab)
    int n_tiles = 0, grid = 0;            // work items of the launch, blocks launched
    int res_epilogue = 0;                 // conv_igemm_mfma with a residual: 1 = read in the epilogue, 0 = prefetched with the last K-step (or no residual)
    int persistent = 0;
    int residual = 0;                     // the launch adds a stored residual
};
constexpr int kLaunchRecInts = 13;
static_assert(sizeof(LaunchRec) == kLaunchRecInts * sizeof(int), "sbbseg_debug_op_launch copies the record as ints");
inline void launch_rec(LaunchRec* r, int family, int bp, int bc, int stages, int n_tiles, int grid, int persistent, int table = 0, int residual = 0)
{
    if (!r) return;
    *r = LaunchRec{};
    r->family = family; r->bp = bp; r->bc = bc; r->stages = stages; r->n_tiles = n_tiles; r->grid = grid; r->persistent = persistent;
    r->table = table; r->residual = residual;
}

// Raise a kernel's dynamic LDS limit to `bytes`, once per device: the attribute belongs to the device's copy of the kernel, so the caller keeps
// one flag array per kernel (`static bool done[64] = {}` at the call site) and the current device selects the flag.  THE one call of
// hipFuncSetAttribute in the library.
inline hipError_t dynamic_lds_once(const void* kernel, int bytes, bool (&done)[64])
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (done[dev & 63]) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done[dev & 63] = true;
    return e;
}

// The tile forms conv_igemm_mfma is instantiated in: one value per (BP, BC, WP, WC, NS, GS, PH8).  conv_choice.h picks one per launch,
// launch_conv (kernels.hip) maps it to the instantiation; the split mode has the five forms marked x3.
enum ConvTileForm {
    kTile128x128 = 0,       // 4 waves, 2 blocks per CU: the default of 128-channel tiles; the split-K launches (x3)
    kTile256x256,           // 8 waves, wave tile 128 px x 64 ch (x3)
    kTile256x256Ph8,        // ... on the staggered 8-phase schedule (conv variant bit 16)
    kTile512x128,           // 8 waves (x3)
    kTile512x64,            // 8 waves, forced by variant 3 only
    kTile256x128S3,         // variant 2: the 8-wave 3-stage tiles
    kTile256x64S3,
    kTile256x32S3,
    kTile256x64,            // 4 waves: the default of 64-channel tiles (x3)
    kTile256x32,            // ... of 32-channel tiles (x3)
    kTile256x256Half,       // conv variant bit 4: half-K-step stages in a 4-deep ring
    kTile128x128Half,
    kTile256x64Half,
    kConvTiles
};
struct ConvTileDims { int bp, bc, wp, wc, ns, gs; bool ph8; };
constexpr ConvTileDims kConvTileDims[kConvTiles] = {
    {128, 128, 2, 2, 2, 8, false}, {256, 256, 2, 4, 2, 8, false}, {256, 256, 2, 4, 2, 8, true}, {512, 128, 4, 2, 2, 8, false},
    {512, 64, 8, 1, 2, 8, false},  {256, 128, 4, 2, 3, 8, false}, {256, 64, 8, 1, 3, 8, false}, {256, 32, 8, 1, 3, 8, false},
    {256, 64, 4, 1, 2, 8, false},  {256, 32, 4, 1, 2, 8, false},  {256, 256, 2, 4, 4, 4, false}, {128, 128, 2, 2, 4, 4, false},
    {256, 64, 4, 1, 4, 4, false}};
// a fast-gather instantiation exists only for whole-K-step, 2-stage, non-8-phase tiles (the others keep the plain gather)
constexpr bool conv_tile_has_fg(const ConvTileDims& d) { return d.ns == 2 && d.gs == 8 && !d.ph8; }

// The form of one conv_igemm_mfma launch, chosen by conv_choice.h's choose_conv -- here, because kernels.hip reads it without ctx.h.
struct ConvForm {
    int tile;             // ConvTileForm (split-K: kTile128x128)
    int fg;               // 1: the fast-gather instantiation runs
    int fast_gather;      // ConvParams::fast_gather: 0 = plain gather, 1 = masked fast gather, 2 = pointwise (no masks)
    int ks_shift;         // split-K: 2^ks_shift blocks per tile; 0 = off
    int tile_map, cls_minor;      // ConvParams
    int table;            // 1: the owned-region level's pixel table is handed over (ConvParams::rmap, M = its entries)
    int variant_flags;    // ConvParams::variant_flags, but for the probe bits
};

// launchers, by the unit that defines them ---------------------------------------------------
// kernels.hip
hipError_t launch_conv(const ConvParams& p, const ConvForm& form, int precision, hipStream_t s, LaunchRec* rec = nullptr);
hipError_t launch_splitk_finish(const float* ws, int splits, long split_elems, long pixels, int cout, const float* scale, const float* shift,
                                const void* residual, int relu, void* out, int precision, hipStream_t s);
// dec_tail.hip, stem.hip, direct64.hip, bottleneck.hip
hipError_t launch_tail(const TailParams& p, int precision, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);
hipError_t launch_stem(const StemParams& p, int precision, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);
hipError_t launch_direct64(const Direct64Params& p, int precision, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);
constexpr int kTailKSteps = 6;      // 4 taps x 64 channels of src0 + 2 steps for the 9 image taps
hipError_t launch_bottleneck(const BlockParams& p, int precision, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);
// the split-mode and fused units
hipError_t launch_dec_halo_x3(const DecHaloParams& p, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);     // split mode: dec4 with LDS-resident halos (dec_halo_x3.hip)
hipError_t launch_dec_halo_f16(const DecHaloParams& p, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);    // ... plain fp16 mode (dec_halo_f16.hip)
hipError_t launch_conv3_expand_reduce(const C3ERParams& p, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);   // 3x3 + expand + next reduce (conv3_expand_reduce.hip)
hipError_t launch_expand_reduce_x3(const ExpRedParams& p, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);   // split mode: expand + next reduce 1x1 (expand_reduce_x3.hip)
hipError_t launch_stem_pool_x3(const StemParams& p, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);      // split mode: stem + max-pool in one launch (stem_pool_x3.hip)
hipError_t launch_block_x3(const BlockParams& p, int num_cus, hipStream_t s, LaunchRec* rec = nullptr);      // split mode, identity blocks (block_x3.hip)
// pixel_ops.hip
hipError_t launch_maxpool(const void* src, void* dst, int n, int H, int W, int C, int k, int stride,
                          int Ho, int Wo, const float* pre_scale, const float* pre_shift, int pre_relu,
                          int precision, hipStream_t s, LaunchRec* rec = nullptr);
hipError_t launch_head(const HeadParams& p, int precision, hipStream_t s, LaunchRec* rec = nullptr);
hipError_t launch_ingest_u8(const IngestParams& p, int precision, hipStream_t s);
hipError_t launch_ingest_f32(const float* x, int n, int H, int W, void* c8, void* pairs, int pad,
                             int pairs_w, int precision, hipStream_t s);
hipError_t launch_stitch(const uint8_t* tile_labels, int H, int W, const int* own_x, const int* own_y,
                         int nyf, int Hp, int Wp, uint8_t* out, hipStream_t s);
// sbbseg_segment_views_dev: tiles [g0, g0 + n_tiles) of a group's pooled tile list (region.h ViewRec) -> both input forms, in one launch;
// the group's label planes out of its tile labels, in one launch (every owner in closed form: region_owner)
struct ViewRec;
struct IngestViewsParams {
    const ViewRec* views;     // the group's views
    const int* maps;          // the call's nearest maps, concatenated
    int n_views, g0, n_tiles;
    int H, W, margin;         // model input size, int(0.1 * W)
    const float* lut;
    void* c8;
    void* pairs;
    int pad, pairs_w;
};
hipError_t launch_ingest_views(const IngestViewsParams& p, int precision, hipStream_t s);
hipError_t launch_stitch_views(const uint8_t* tile_labels, int H, int W, int margin, const ViewRec* views, int n_views, unsigned n_blocks, hipStream_t s);
hipError_t launch_resize_labels(const uint8_t* labels, int H, int W, const int* map_y, const int* map_x,
                                int out_h, int out_w, uint8_t* out, hipStream_t s);
// sbbseg_segment_whole_views_dev: one patch per view (the whole-image branch, main.py:368-380).  Patch p of a chunk is view v0 + p of the
// call's table; its pixel (y, x) reads stored pixel (maps[my + y], maps[mx + x]) (the composed model -> page -> stored nearest maps) and
// pixel (y, x) of its label plane reads label (maps[oy + y], maps[ox + x]) of the patch's H x W label map.
struct WholeViewRec {
    const uint8_t* page;      // stored page [stored_h][stored_w][3]
    uint8_t* out;             // label plane [out_h][out_w], any alignment
    int stored_w;
    int my, mx, oy, ox;       // offsets of the view's four maps in the call's map array
    int out_h, out_w;
    unsigned lead;            // out & 15: bytes between the 16-byte line the plane starts in and the plane
    unsigned blk_first;       // label resize: first block of the view among its chunk's (prefix sum of ceil((lead + out_h * out_w) / 4096))
};
struct IngestWholeViewsParams {
    const WholeViewRec* views;    // the chunk's views
    const int* maps;
    int n_views;                  // = patches of the launch
    int H, W;
    const float* lut;
    void* c8;
    void* pairs;
    int pad, pairs_w;
};
hipError_t launch_ingest_whole_views(const IngestWholeViewsParams& p, int precision, hipStream_t s);
constexpr int kResizeViewsBlockBytes = 256 * 16;      // plane bytes a block of resize_labels_views_kernel covers: 16 per lane
hipError_t launch_resize_labels_views(const uint8_t* labels, int H, int W, const WholeViewRec* views, const int* maps, int n_views, unsigned n_blocks,
                                      hipStream_t s);
hipError_t launch_replicate3(const uint8_t* src, uint8_t* dst, size_t n, hipStream_t s);
hipError_t launch_to_f32(const void* src, float* dst, size_t n, int precision, hipStream_t s);
hipError_t launch_period_mismatches(const void* data, size_t shift_bytes, size_t tail_bytes, unsigned long long* res, int num_cus, hipStream_t s);   // sbbseg_debug_tensor_period_mismatches
hipError_t launch_split_to_f32(const void* src, float* dst, size_t npix, int C, hipStream_t s);   // [pix][C hi][C lo] -> [pix][C]
// page_glue.hip
hipError_t launch_otsu(const uint8_t* page, int src_Wp, int Hp, int Wp, const int* map_y, const int* map_x,
                       unsigned* hist, int* thr, int num_cus, hipStream_t s);
// stage glue: iterated 5x5 erode / dilate as one separable clipped min / max filter; largest 8-connected component
hipError_t launch_morph(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int H, int W, int radius, int is_max, int binarize, hipStream_t s);
constexpr int kCcMaxRivals = 250;    // rival roots sbbseg_page_box_dev gets back from the device (more: the host scans the label plane)
hipError_t launch_largest_contour(const uint8_t* mask, int H, int W, int* parent, int* count, int* area2, int* bx0, int* by0, int* bx1,
                                  int* by1, unsigned long long* d_best, int* d_out, hipStream_t s);
// the roots of the components without a parent (RETR_TREE), after launch_largest_contour on the same plane
hipError_t launch_parentless_roots(const uint8_t* mask, uint8_t* inv, int H, int W, const int* parent, int* bg, int* touch, const int* area2,
                                   const int* bx0, const int* by0, const int* bx1, const int* by1, int* d_n, int* list, int cap, hipStream_t s);
hipError_t launch_deskew_profiles(const uint8_t* mask, int H, int W, int S, int top, int left, const double* minv, const float* cubic,
                                  int n_angles, int* counts, hipStream_t s);
// the outer contour polygons of listed roots of a labelled plane (contours.hip, contour_walk.h): one wave per candidate
struct ContourCand { int root, x0, y0, x1, y1, lower2; };     // launch_parentless_roots' record: root, box, lower bound of the doubled area
struct ContourRec {           // what the counting launch leaves per candidate
    long long area2;          // exact doubled area of the outer contour
    int n_points, status;     // CHAIN_APPROX_SIMPLE points; kContourOk or why the walk ended early (contour_walk.h)
    int x, y, w, h;           // cv2.boundingRect of the contour
};
struct ContourParams {
    const int* parent;        // label plane: root per foreground pixel, -1 elsewhere
    int H, W;
    const ContourCand* cand;  // [n_cand] in the order of the result
    int n_cand;
    int lds_limit;            // bytes: a bit map beyond it takes the global form
    ContourRec* rec;          // [n_cand], written by the counting launch
    const int* slot;          // [n_cand] writing launch: the candidate's contour, or -1
    const long long* point_off;   // [contours + 1] writing launch: first point of every contour
    int32_t* points;          // [points][2] x, y; nullptr = the counting launch
};
struct ContourPackParams {
    const ContourRec* rec;
    int n_cand, filter;       // filter: keep contours of at least three points whose area lies in [lo, hi] (main.py:82-88); 0: keep all
    double lo, hi;
    int* slot;                // [n_cand]
    int32_t* boxes;           // [contours][4] x, y, w, h
    long long* area2;         // [contours]
    long long* point_off;     // [contours + 1]
    long long* totals;        // [4] contours, points, candidates whose walk failed, the first such candidate's status
};
hipError_t launch_contour_all_roots(const int* parent, const int* bx0, const int* by0, const int* bx1, const int* by1, long n, int* d_n,
                                    ContourCand* list, int cap, hipStream_t s);
hipError_t launch_contour_trace(const ContourParams& p, bool any_lds, bool any_global, hipStream_t s);      // 1 launch per form in use
hipError_t launch_contour_pack(const ContourPackParams& q, hipStream_t s);
// batched per-region deskew profiles (region_deskew.hip): crop + erode every box of a label plane, then rotate-and-project all
// (region, angle, row) of a sweep in one launch
struct DeskewRegion {
    int x, y, w, h;           // the box on the plane
    int S, top, left;         // side of the zero square (int(1.4 * max(h, w))), placement of the crop inside it (main.py:1613-1619)
    int clip;                 // 1: the crop keeps a margin of at least one pixel to the square's edges (the analytic x span is valid)
    long long crop_off;       // first byte of the eroded crop in the packed crop buffer
    long long count_off;      // first int of the region's [n_angles][S] counts
    int block0;               // first block of the region in the profile launch
    int row_groups;           // blocks per angle: ceil(S / kRegionDeskewRows)
};
constexpr int kRegionDeskewRows = 8;      // destination rows per block of region_deskew_profile_kernel (a wave per row, two rounds)
// the label plane a region is cropped from, one record per region beside its DeskewRegion: the boxes of one call may lie on many planes
struct DeskewPlane {
    const uint8_t* base;      // [H][W] label plane (device), dense
    int W, H;                 // H: for the host's box checks only
};
struct RegionDeskewParams {
    const DeskewPlane* planes;// [n_regions] the plane of every region (read by the row pass of the crops only)
    const DeskewRegion* geom; // [n_regions]
    int n_regions, n_angles, radius;
    long long total_pix;      // sum of w * h
    const double* minv;       // [n_regions][n_angles][6] inverse affine maps
    const float* cubic;       // [32][4]
    uint8_t* tmp;             // [total_pix] row pass of the erosion
    uint8_t* crops;           // [total_pix] eroded crops, packed
    int* counts;              // packed row counts
    int total_blocks;
};
hipError_t launch_region_deskew_crops(const RegionDeskewParams& p, hipStream_t s);
hipError_t launch_region_deskew_profiles(const RegionDeskewParams& p, hipStream_t s);
// deskewed text-line masks and their projections for every box of a page (region_lines.hip, line_mask.h): OPEN / CLOSE of the packed
// eroded crops * 255, the fixed-point bicubic rotation by the region's own slope onto the crop's own h x w, != 0, row and column sums
struct LineRegion {
    int w, h;
    long long crop_off;       // first byte of the region in the packed crop / mask buffers
    int row_off, col_off;     // first int of the region's row sums / column sums
    int block0;               // first block of the region in the warp launch
    int pad;
};
constexpr int kRegionLineRows = 8;        // destination rows per block of region_line_warp_kernel (a wave per row, two rounds)
struct RegionLinesParams {
    const LineRegion* geom;   // [n_regions]
    int n_regions;
    long long total_pix;      // sum of w * h
    int total_cols;           // sum of w
    int total_blocks;
    const double* minv;       // [n_regions][6] inverse affine maps
    const int16_t* itab;      // [32][32][16] fixed-point bicubic weights (line_mask_weights)
    uint8_t* a;               // packed scratch
    uint8_t* b;               // packed: the eroded crops on entry, the opened / closed crops (0 / 255) after the morphology
    uint8_t* mask;            // packed dst (0 / 1)
    int* rows;                // packed row sums
    int* cols;                // packed column sums
};
hipError_t launch_region_line_morph(const RegionLinesParams& p, hipStream_t s);      // 6 launches: b -> ... -> b
hipError_t launch_region_line_masks(const RegionLinesParams& p, hipStream_t s);      // 2 launches: warp + row sums, column sums
constexpr int kRegionLineLaunches = 8;    // of the two calls above, whatever n_regions is
// the 1-D statistic of every (region, angle) profile of a sweep and the winner per region (profile_stats.hip, profile_stat.h)
constexpr int kProfileLdsSamples = 2048;  // longest profile whose smoothed forms stay in LDS; longer ones use ProfileStatParams::workspace
struct ProfileRegion {
    long long count_off;      // first int of the region's [n_angles][S] counts
    long long ws_off;         // S > kProfileLdsSamples: first double of the region's [n_angles][2 S + 40] workspace
    int S, pad;
};
struct ProfileStatParams {
    const int32_t* counts;    // packed row counts (device)
    const ProfileRegion* regions;
    int n_regions, n_angles;
    const double* weights;    // [radius + 1] half Gaussian kernel
    int radius;
    double multiplier;
    double* workspace;
    double* spread;           // [n_regions][n_angles]
    uint8_t* state;           // [n_regions][n_angles]: 0 appended, 1 skipped, 2 exception
    int32_t* winner;          // [n_regions]
    double* smooth;           // null, or (sbbseg_debug_profile_statistics) z of every profile, packed like counts
    double* below;            // null, or (the same) [n_regions][n_angles]: what deep_level returned
};
hipError_t launch_profile_statistics(const ProfileStatParams& p, bool any_long, hipStream_t s);
// out[i] = soft_div(a[i], b[i]) (op 0) or soft_sqrt(a[i]) (op 1) of profile_stat.h on the device (sbbseg_debug_soft_arith)
hipError_t launch_soft_arith(int op, const double* a, const double* b, long long n, double* out, hipStream_t s);
// the text lines of every region from its row or column sums (line_split.hip, line_split.h): one wave per region
struct LineSplitRegion {
    long long prof_off;       // first int of the region's profile
    long long ws_off;         // n > kProfileLdsSamples: first byte of the region's line_work_bytes(n) workspace
    int n, other, vertical;   // samples of the profile, the other extent of dst, 1 = seperate_lines_vertical
    int line_off;             // first line of the region in the packed outputs
    double rot[6];            // cos, -sin, sin, cos (main.py:524), M[0, 2], M[1, 2] (main.py:519-521)
};
struct LineSplitParams {
    const int32_t* profiles;  // packed profiles (device)
    const LineSplitRegion* regions;
    int n_regions, sigma_max;
    const double* weights;    // half kernels of sigma = 2 .. sigma_max
    const long long* weight_off;
    unsigned char* workspace;
    int32_t* info;            // [n_regions][kLineInfoInts]
    int32_t* pts;             // [lines][3] peak, point_up, point_down
    int32_t* box;             // [lines][4][2]
    int32_t* rot;             // [lines][4][2]
};
hipError_t launch_line_split(const LineSplitParams& p, bool any_long, hipStream_t s);      // 1 launch, 2 with a profile beyond kProfileLdsSamples
// the reading order of a page's text regions (order.hip, order.h)
struct OrderParams {
    const uint8_t* plane;     // [H][W] textline plane, or null: row_sums are given
    int H, W;
    const double* weights;    // [radius + 1] half Gaussian kernel of sigma 8
    int radius;               // kOrderRadius
    const int32_t* points;    // [points][2] x, y, packed in contour order
    const long long* point_off;       // [n + 1]
    int n;                    // contours
    int32_t* row_sums;        // [H]
    double* smooth;           // [H + 80] workspace: the smoothed, flipped profile
    int32_t* n_edges;         // [1]
    int32_t* edges;           // [order_edge_capacity(H)]
    double* moments;          // [n][3] m00, m10, m01
    double* centroids;        // [n][2] cx, cy
    int32_t* serial;          // [n] 1: the contour's sums were redone in float64, serially
    int32_t* sorted_index;    // [n]
    int32_t* order;           // [n]
    int32_t* band;            // [n]
};
hipError_t launch_row_sums(const OrderParams& p, hipStream_t s);                 // 1 launch
hipError_t launch_order_edges(const OrderParams& p, hipStream_t s);              // 1 launch
hipError_t launch_contour_moments(const OrderParams& p, hipStream_t s);          // 1 launch
hipError_t launch_order_rank(const OrderParams& p, hipStream_t s);               // 1 launch
constexpr int kOrderLaunches = 4;         // of a whole reading-order call, whatever n and H are
// the x extents of the text lines of every region from its filled, rotated contour (line_extent.hip, line_extent.h)
struct ExtentRegion {
    long long win_off;        // first point of the region's winner in ExtentParams::winner (second scan pass, extents)
    long long mark_off;       // global form of the scan: first word of the region's two mark planes in ExtentParams::marks
    int ox, oy, w, h;         // the box
    int src_off, dst_off;     // first word of the filled bit map / of threshrot's bit map (box + ring) in ExtentParams::bits
    int block0;               // first work item (8 rows) of the fill and warp kernels
    int line_off, vertical;   // first line of the region in the packed line tables; 1 = |slope| > 45
    int pad;
    double minv[6];           // rotate_image's inverse map for the box
    double rot[6];            // cos, -sin, sin, cos, x_d, y_d as sbbseg_line_split_dev takes them
    double step;              // w / 999.0 (np.linspace's step; divided on the host)
};
struct ExtentParams {
    const ExtentRegion* regions;
    int n_regions, total_blocks, total_lines, lds_limit;
    const int32_t* points;    // [points][2] the rings, page coordinates
    const long long* point_off;       // [n_regions + 1]
    uint32_t* bits;
    uint32_t* marks;
    const int64_t* wtab;      // [kExtentTabEntries] float32 bicubic products * 2^34
    int32_t* rec;             // [n_regions][kExtentRecInts]
    int32_t* winner;          // [points][2]; null in the counting pass of the scan
    const int32_t* info;      // [n_regions][kLineInfoInts] as sbbseg_line_split_dev wrote them
    const int32_t* lines;     // [total_lines][3] peak, point_up, point_down
    int32_t* extent;          // [total_lines][2]
    int32_t* box;             // [total_lines][4][2] rewritten corners
    int32_t* rot;             // [total_lines][4][2]
};
hipError_t launch_extent_masks(const ExtentParams& p, hipStream_t s);                               // 2 launches: fill, warp + threshold
hipError_t launch_extent_scan(const ExtentParams& p, bool any_lds, bool any_global, hipStream_t s);  // 1 launch per form in use
hipError_t launch_extent_lines(const ExtentParams& p, hipStream_t s);                                // 1 launch

// channel-tile width the bf16 conv kernel uses for `cout` (weights are padded to it)
inline int conv_tile_bc(int cout) { return cout >= 128 ? 128 : (cout > 32 ? 64 : 32); }
// Channel stored in packed weight row `row` (16-bit modes).  Inside each wave tile of WCH channels
// (64, or 32 when the channel tile is 32) MFMA row block mi, row rho is given channel
// (mi>>1)*32 + (rho>>2)*8 + (mi&1)*4 + (rho&3): see the epilogue of conv_igemm_mfma.
inline int conv_row_channel(int row, int cout)
{
    const int wch = conv_tile_bc(cout) == 32 ? 32 : 64;
    const int base = (row / wch) * wch, t = row % wch;
    const int mi = t >> 4, rho = t & 15;
    return base + (mi >> 1) * 32 + (rho >> 2) * 8 + (mi & 1) * 4 + (rho & 3);
}
int set_error(const char* fmt, ...);   // fills sbbseg_last_error() (thread-local), returns 1
// host conversions f32 -> 16 bits, round to nearest even (device twins: device_prims.h)
inline uint16_t f32_to_bf16_rne(float f)
{
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline uint16_t f32_to_f16_rne(float f)
{
    f = f > 65504.f ? 65504.f : (f < -65504.f ? -65504.f : f);
    _Float16 h = (_Float16)f;
    return __builtin_bit_cast(uint16_t, h);
}
float bf16_to_f32(uint16_t h);

}  // namespace sbbseg
