// kernels.hip -- the implicit-GEMM convolution of libsbbseg on gfx950 (MI355X, CDNA4) and its dispatch.
//
// Hot kernel: conv_igemm_mfma -- im2col-free implicit-GEMM convolution on MFMA.
//   D[channel][pixel] = sum_k W[channel][k] * X[pixel][k]     (v_mfma_f32_16x16x32_{f16,bf16}, fp32 acc)
//   * the contraction axis k walks (source, channel group, tap) in 16-byte granules; nearest x2 upsampling, channel
//     concat of two sources, zero padding and the one_side_pad shift are address arithmetic in the gather -- no tensor
//     is materialised
//   * operands go HBM/L2 -> LDS with 16-byte LDS-DMA loads (lane-linear LDS image, XOR-swizzled through the *source*
//     granule choice), double buffered: `buffer_load ... lds` with the tap displacement in the scalar offset and
//     out-of-bounds taps zero-filled by the hardware (fast gather), or `global_load_lds` with per-lane address
//     arithmetic (plain gather: irregular K-steps, upsampling sources, short-K layers)
//   * MFMA "A" operand = weights, "B" = pixels, so a lane ends up with consecutive channels of one pixel: 16-byte NHWC
//     epilogue stores; BN scale/shift, residual add and ReLU are applied in fp32 registers
//   * X3 = the split-fp16 (label-exact) mode: hi + lo operands, three MFMAs per product.
// Also here: conv_naive_f32 (the fp32 mode) and splitk_finish.  (The host conversions f32 -> 16 bits and the row order conv_row_channel
// are inline in internal.h: the host-only packer wpack.h needs them without this unit.)
// The other kernel families have a unit each: dec_tail.hip, stem.hip, direct64.hip, bottleneck.hip (direct kernels on LDS halo
// tiles where an output tile has few channels), pixel_ops.hip (ingest, max-pool, head, stitch, resize) and page_glue.hip (Otsu,
// morphology, components, deskew profiles); the primitives they share are in device_prims.h.
#include "device_prims.h"

namespace sbbseg {

float bf16_to_f32(uint16_t h) { uint32_t u = (uint32_t)h << 16; return __builtin_bit_cast(float, u); }

// split mode: add 8 consecutive channels of one stored pixel (hi halves at src, lo halves `plane` elements behind; cf. store_split8)
__device__ inline void add_split8(const uint16_t* src, int plane, float (&y)[8])
{
    const h8_t h = *(const h8_t*)src, l = *(const h8_t*)(src + plane);
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = __fadd_rn(y[q], __fadd_rn((float)h[q], (float)l[q]));      // hi + lo is exact in fp32; one rounding, never fused
}

// ------------------------------------------------------------------------------------------------
// conv_igemm_mfma  (16-bit operands: bf16 or fp16, fp32 accumulate)
// ------------------------------------------------------------------------------------------------
template <int BP, int BC, int WP, int WC, int NS, int GS = 8>
struct ConvTile {
    // GS = 16-byte granules of the contraction axis per LDS stage: 8 (a whole 64-element K-step) or 4
    // (half a K-step: twice as many, half as big stages -> deeper prefetch in the same LDS)
    static constexpr int kWaves = WP * WC;
    static constexpr int kThreads = 64 * kWaves;
    static constexpr int kRowBytes = GS * 16;
    static constexpr int kRowsPerInstr = 64 / GS;             // rows one global_load_lds wave-instruction fills
    static constexpr int kStagesPerKStep = 8 / GS;
    static constexpr int kWPX = BP / WP;          // pixels per wave tile
    static constexpr int kWCH = BC / WC;          // channels per wave tile
    static constexpr int kNI = kWPX / 16;
    static constexpr int kMI = kWCH / 16;
    static constexpr int kPLoads = BP / (kRowsPerInstr * kWaves);   // global_load_lds per thread per stage, pixels
    static constexpr int kWRows = BC > kRowsPerInstr * kWaves ? BC : kRowsPerInstr * kWaves;   // weight rows staged (>= one
                                                  // row group per wave, so every wave issues the same number of loads)
    static constexpr int kWLoads = kWRows / (kRowsPerInstr * kWaves);   // ... weights
    static constexpr int kLoads = kPLoads + kWLoads;
    static constexpr int kStageBytes = (BP + kWRows) * kRowBytes;
    static constexpr int kLdsBytes = NS * kStageBytes;
    static constexpr int kBlocksPerCU = (kWaves == 4 && 3 * kLdsBytes <= 160 * 1024) ? 3 : (kWaves == 4 && 2 * kLdsBytes <= 160 * 1024) ? 2 : 1;
    // the residual of the tile being finished is prefetched into registers with its last K-step (else the epilogue reads it): the tiles whose
    // epilogue registers leave room -- in the split mode (two planes) the 128 x 128 tile only
    static constexpr bool prefetches_residual(bool x3) { return (kMI / 2) * kNI <= 8 && (!x3 || (BP == 128 && BC == 128)); }
    static_assert(GS == 8 || GS == 4, "stage = whole or half K-step");
    static_assert(BP % (kRowsPerInstr * kWaves) == 0 && kWRows % (kRowsPerInstr * kWaves) == 0, "tile rows must split over the waves");
    static_assert(kMI % 2 == 0, "epilogue pairs MFMA row blocks");
};

// blocks per CU a tile family is sized for (LDS budget) -> min waves per SIMD for __launch_bounds__
constexpr int conv_blocks_per_cu(int bp, int bc, int wp, int wc, int ns, int gs)
{
    const int waves = wp * wc;
    const int rpi = 64 / gs;
    const int wrows = bc > rpi * waves ? bc : rpi * waves;
    const int lds = ns * (bp + wrows) * gs * 16;
    if (waves != 4) return 1;
    return 3 * lds <= 160 * 1024 ? 3 : (2 * lds <= 160 * 1024 ? 2 : 1);
}

// n / d for n < 2^31 with a host-made (magic, shift) pair (FastDiv, internal.h): one v_mul_hi_u32 + shift instead of the
// ~40-instruction division sequence -- setup_rows divides twice per staged row, which on short-K tiles rivals the MFMA time
__device__ inline int fast_div(int n, uint32_t magic, uint32_t shift)
{
    const uint32_t q = magic ? __umulhi((uint32_t)n, magic) : (uint32_t)n;
    return (int)(q >> shift);
}

// Pipeline: NS LDS stages, stage s+D (D = NS-1) is issued while stage s is multiplied.  Blocks are
// PERSISTENT: block b walks tiles b, b+G, b+2G, ... and the stage stream runs straight across tile
// boundaries, so the first K-step of the next tile is in flight while the current tile finishes its
// MFMAs and runs its epilogue -- short-K layers (1x1 convs, K = 64..512) otherwise spend most of
// their time filling and draining a 1-4 step pipeline.
// K-step descriptors come through the scalar cache (uniform address in the constant address space
// -> s_load, lgkmcnt): no VGPR-destination VMEM load sits in the steady-state loop.
// X3 = the split mode (internal.h, kF16X3): a K-step is 32 channels of one tap staged as slots 0-3 = "hi" halves,
// slots 4-7 = "lo" halves (same LDS image, same staging code: only the source offset of slots 4-7 differs, SrcDesc::lo_off);
// three MFMAs per product; outputs are split again in the epilogue and stored as [C hi][C lo] per pixel.
// FG = the fast gather (ConvParams::fast_gather): every staged row keeps a per-source byte offset and a bit mask of its
// out-of-bounds taps, set up once per tile; a K-step's tap/channel displacement is wave-uniform and rides in the buffer
// load's scalar offset, an out-of-bounds tap sets bit 31 of the lane offset (past num_records -> the load writes zeros
// to LDS, tools/probes/buffer_lds_oob_probe.hip).  Two VALU ops per load instead of ~18: on the long-K tiles the
// address arithmetic of the plain gather costs 20-25 % of the loop (tools/probes/mfma_loop_probe.hip).
// KS = split-K (ConvParams::ks_shift): tile index = tile * 2^ks_shift + split; split s walks K-steps [s * nt, (s + 1) * nt) of the tile and stores
// fp32 partial sums instead of running the epilogue.  A launch of 2-32 tiles of 100-400 K-steps (one patch) leaves most CUs idle for ~1 us per
// K-step; results of a split launch differ from the unsplit one in the last bits (association), so only the whole-image branch uses it.
template <int BP, int BC, int WP, int WC, int NS, bool F16, int GS = 8, bool PH8 = false, bool X3 = false, bool FG = false, bool KS = false>
__global__ __launch_bounds__(64 * WP * WC, (conv_blocks_per_cu(BP, BC, WP, WC, NS, GS) * (WP * WC) / 4))
void conv_igemm_mfma(const ConvParams p)
{
    static_assert(!X3 || (F16 && GS == 8 && !PH8), "split mode: fp16 halves, whole-K-step stages, plain loop");
    static_assert(!KS || (FG && BP == 128 && BC == 128 && NS == 2 && GS == 8 && !PH8), "split-K: the 128 x 128 tile on the fast gather");
    static_assert(!FG || !PH8, "the 8-phase schedule keeps the plain gather");
    constexpr int PL = X3 ? 2 : 1;                       // 16-bit planes per stored activation element
    using T = ConvTile<BP, BC, WP, WC, NS, GS>;
    constexpr int RPI = T::kRowsPerInstr, RB = T::kRowBytes, SPK = T::kStagesPerKStep;
    constexpr int NW = T::kWaves;
    constexpr int D = NS - 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave / WC, wc = wave % WC;

    const int n_ct = (p.cout + BC - 1) / BC;
    const int n_pt1 = (p.M + BP - 1) / BP;              // pixel tiles of ONE placement class
    // class-minor order (small weights): the classes of one pixel tile are adjacent and, with the XCD-
    // grouped walk, on the same XCD -- they read the same source pixels, which then come from one L2.
    // Pixel tiles are padded to a multiple of 8 per class there (padding tiles are fully masked).
    const int n_pt1e = p.cls_minor ? (n_pt1 + 7) & ~7 : n_pt1;
    const int n_tiles = (p.n_cls * n_ct * n_pt1e) << (KS ? p.ks_shift : 0);
    const int G = gridDim.x;
    const int nt_full = p.total_ksteps;
    const int nt = KS ? nt_full >> p.ks_shift : nt_full;       // K-steps this block walks per tile
    auto split_of = [&](int tile) __attribute__((always_inline)) -> int { return KS ? tile & ((1 << p.ks_shift) - 1) : 0; };
    // Tile walk of this (persistent) block.  map 0: tiles b, b+G, ... (channel tile fastest): every
    // XCD keeps ONE channel-tile's weight slab hot -- right when the weights dwarf the L2.
    // map 1 (small weight matrices): XCD x = b % 8 owns pixel tiles x, x+8, ...; its blocks walk them
    // channel tile fastest, so the n_ct channel tiles of one pixel tile run on the SAME XCD back to
    // back and the pixel operand is fetched into that L2 once instead of once per XCD.
    const int n_pt = p.n_cls * n_pt1e;                  // "extended" pixel tiles (class x pixel tile)
    auto decode = [&](int tile, int& ctile, int& cls, int& ptile) __attribute__((always_inline)) {
        if constexpr (KS) tile >>= p.ks_shift;
        const int e = fast_div(tile, p.nct_magic, p.nct_shift);
        ctile = tile - e * n_ct;
        if (p.cls_minor) {                              // (n_cls is 1, 2 or 4)
            const int lg = 3 + (p.n_cls >> 1);
            const int grp = e >> lg, r = e & ((1 << lg) - 1);
            cls = r >> 3;
            ptile = grp * 8 + (r & 7);
        } else if (p.n_cls > 1) {
            cls = e / n_pt1;
            ptile = e - cls * n_pt1;
        } else {
            cls = 0;
            ptile = e;
        }
    };
    // map 2 (short-K layers): as map 1, but every block owns a CONTIGUOUS run of its XCD's list, so the
    // channel tiles of one pixel tile run back to back in the SAME block.  Blocks of a short-K layer
    // march in lockstep; under map 1 the sibling blocks miss on the same pixel rows at the same moment
    // and the rows are fetched from HBM once per channel tile (PMC: fetch = n_ct x the input tensor).
    // map 3 (grouped launches): XCD x owns a CONTIGUOUS range of the extended pixel tiles (whole groups of 8 pixel tiles x
    // classes), its blocks walk that range together: the four classes of a pixel tile AND its neighbours above / below
    // meet in one L2, so the halo rows between consecutive pixel tiles are fetched from HBM once, not once per XCD.
    const bool pshare = p.tile_map >= 1 && (G & 7) == 0;
    const bool contig = p.tile_map == 2;
    const bool ranged = p.tile_map == 3 && pshare;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, GX = G >> 3;
    const int unit = 8 * p.n_cls, n_units = n_pt / unit;          // (n_pt is a multiple of 8 * n_cls under cls_minor)
    const int e_lo = ranged ? (int)((long long)xcd * n_units / 8) * unit : 0;
    const int e_hi = ranged ? (int)((long long)(xcd + 1) * n_units / 8) * unit : 0;
    const int xcd_tiles = ranged ? (e_hi - e_lo) * n_ct : pshare ? ((n_pt - xcd + 7) >> 3) * n_ct : 0;
    const int run_lo = contig ? (int)((long long)slot * xcd_tiles / GX) : 0;
    const int run_hi = contig ? (int)((long long)(slot + 1) * xcd_tiles / GX) : 0;
    const int my_tiles = !pshare ? (n_tiles - (int)blockIdx.x + G - 1) / G
                         : contig ? run_hi - run_lo
                                  : (slot < xcd_tiles ? (xcd_tiles - slot + GX - 1) / GX : 0);
    auto tile_at = [&](int q) __attribute__((always_inline)) -> int {
        if (!pshare) return blockIdx.x + q * G;
        const int li = contig ? run_lo + q : slot + q * GX;
        const int lq = fast_div(li, p.nct_magic, p.nct_shift), lr = li - lq * n_ct;
        if (ranged) return (e_lo + lq) * n_ct + lr;
        return (lq * 8 + xcd) * n_ct + lr;
    };
    const int nts = nt * SPK;                           // LDS stages per tile
    const int total = my_tiles * nts;                   // stages this block walks

    // one global_load_lds wave-instruction fills RPI rows x GS granules; the LDS image is lane-linear,
    // the XOR swizzle is applied through the SOURCE granule each lane fetches.  Row r keeps granule g
    // at slot g ^ swz(r): swz = r & 7 for 128-byte rows, {0,2,3,1}[(r >> 2) & 3] for 64-byte rows
    // (both brute-forced conflict-free for the four 16-lane groups of ds_read_b128).
    const int lrow = lane / GS;                         // row inside the instruction's row group
    const int lswz = GS == 8 ? lrow : ((0x78 >> (2 * ((lrow >> 2) & 3))) & 3);
    const int gsrc = (lane % GS) ^ lswz;                // source granule (within the stage) this lane fetches
    const int HoWo = p.Ho * p.Wo;
    // output-grid pixel index inside one patch -> (oy, ox): row-major, a pixel tile = a strip of BP consecutive pixels
    auto decode_yx = [&](int rem, int& oy, int& ox) __attribute__((always_inline)) {
        oy = fast_div(rem, p.wo_magic, p.wo_shift);
        ox = rem - oy * p.Wo;
    };
    // pixel index m of class `cls` -> (patch, oy, ox) on the op's output grid.  Owned-region launches (ConvParams::rmap, region.h) look the
    // triple up in the launch's table -- the grid is walked only where the page stitch keeps the result (plus the later levels' halo);
    // the table of a parity class is the one of its placement offset
    // (fast-gather kernels only -- every decoder conv takes them; the plain-gather tiles have no registers for the lookup and the host
    //  never hands them a table: launch_op)
    auto decode_m = [&](int m, int cls, int& n, int& oy, int& ox) __attribute__((always_inline)) {
        if (FG && p.rmap) {
            const int slot = p.n_cls > 1 ? p.ooy_cls[cls] * 2 + p.oox_cls[cls] : 0;
            const uint32_t code = p.rmap[(size_t)slot * (size_t)p.M + (size_t)m];
            n = (int)(code >> 22); oy = (int)((code >> 11) & 2047u); ox = (int)(code & 2047u);
        } else {
            n = fast_div(m, p.howo_magic, p.howo_shift);
            decode_yx(m - n * HoWo, oy, ox);
        }
    };

    // both sources' descriptors live in SGPRs for the whole kernel
    const SrcDesc sd0 = p.src[0];
    const SrcDesc sd1 = p.n_src > 1 ? p.src[1] : p.src[0];
    const int ks0 = p.n_src > 1 ? sd0.ksteps : nt_full;
    const uint32_t img0 = (uint32_t)(sd0.PH * sd0.PW * sd0.pix_bytes), img1 = (uint32_t)(sd1.PH * sd1.PW * sd1.pix_bytes);
    // load-side class state (weights, tap tables), switched in setup_rows
    const char* wbase = (const char*)p.w;
    const __attribute__((address_space(4))) int* kstep_tab =
        (const __attribute__((address_space(4))) int*)(uintptr_t)(FG ? (const void*)p.fgstep_cls[0] : (const void*)p.kstep);
    const KTabEntry* ktab = p.ktab;

    // ---- load side: rows of the tile being STAGED (runs D steps ahead of the compute side)
    // plain gather: output coords (oy, ox, n) of the staged rows.  Fast gather: r_oy = byte offset of the row's centre tap
    // in source 0, r_ox = the same in source 1, r_n = mask of out-of-bounds taps (bit src*16 + (dy-tap_lo_y)*4 + (dx-tap_lo_x)).
    int r_oy[T::kPLoads], r_ox[T::kPLoads], r_n[T::kPLoads];
    uint32_t w_off[T::kWLoads];
    // fast gather: buffer resources.  A source's resource starts fg_bias bytes BEFORE its buffer so that the scalar
    // offset (tap displacement + fg_bias) is never negative.
    const uint32_t fg_bias0 = (uint32_t)(kFgBiasPixels(sd0.PW) * sd0.pix_bytes), fg_bias1 = (uint32_t)(kFgBiasPixels(sd1.PW) * sd1.pix_bytes);
    // bytes from a source row's first granule to the granule this lane fetches
    auto lane_part = [&](const SrcDesc& sd) __attribute__((always_inline)) -> uint32_t {
        return X3 ? (uint32_t)((gsrc & 3) * 16 + (gsrc >> 2) * sd.lo_off) : (uint32_t)(gsrc * 16);
    };
    auto oob_mask = [&](const SrcDesc& sd, int oy, int ox) __attribute__((always_inline)) -> uint32_t {
        const int cy = oy << sd.sy_shift, cx = ox << sd.sx_shift;
        uint32_t xm = 0, m = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) xm |= ((unsigned)(cx + b + sd.tap_lo_x) < (unsigned)sd.lim_x) ? 0u : (1u << b);
#pragma unroll
        for (int a = 0; a < 4; ++a) m |= (((unsigned)(cy + a + sd.tap_lo_y) < (unsigned)sd.lim_y) ? xm : 0xfu) << (4 * a);
        return m;
    };
    auto setup_rows = [&](int tile) __attribute__((always_inline)) {
        int ctile, cls, ptile;
        decode(tile, ctile, cls, ptile);
        if (p.n_cls > 1) {
            wbase = (const char*)p.w_cls[cls];
            kstep_tab = (const __attribute__((address_space(4))) int*)(uintptr_t)(FG ? (const void*)p.fgstep_cls[cls] : (const void*)p.kstep_cls[cls]);
            ktab = p.ktab_cls[cls];
        }
        if constexpr (FG && !X3) {              // (the split-mode tiles have no registers to spare for it: every lane does every row)
            // The 8 lanes of an LDS row (lane & 7 = granule) stage the same kPLoads pixel rows: lane g works out row j = g
            // only, and the group shares the results through ds_bpermute -- instead of every lane repeating all kPLoads
            // rows (~75 VALU ops each; on a 17-K-step decoder tile that was a quarter of the wave's MFMA time).
            static_assert(T::kPLoads <= 8 && RPI == 8, "one row per lane of the 8-lane group");
            const int g8 = lane & 7;
            int my_a = 0, my_b = 0, my_c = -1;              // row past M: every tap out of bounds -> zero rows
            const int mm = ptile * BP + ((g8 < T::kPLoads ? g8 : 0) * NW + wave) * RPI + lrow;
            if (g8 < T::kPLoads && mm < p.M) {
                int n, oy, ox;
                decode_m(mm, cls, n, oy, ox);
                my_a = (int)((uint32_t)n * img0 + (uint32_t)(((oy << sd0.sy_shift) * sd0.PW + (ox << sd0.sx_shift)) * sd0.pix_bytes) +
                             (uint32_t)kZeroHeaderBytes);
                // (fast_gather == 2: every tap is (0, 0) -- pointwise convs -- and in bounds for every real row)
                uint32_t inv = p.fast_gather == 2 ? 0u : oob_mask(sd0, oy, ox);
                if (p.n_src > 1) {
                    my_b = (int)((uint32_t)n * img1 + (uint32_t)(((oy << sd1.sy_shift) * sd1.PW + (ox << sd1.sx_shift)) * sd1.pix_bytes) +
                                 (uint32_t)kZeroHeaderBytes);
                    if (p.fast_gather != 2) inv |= oob_mask(sd1, oy, ox) << 16;
                }
                my_c = (int)inv;
            }
#pragma unroll
            for (int j = 0; j < T::kPLoads; ++j) {
                const int srcl4 = ((lane & ~7) | j) << 2;          // ds_bpermute takes the source lane's byte address
                r_n[j] = __builtin_amdgcn_ds_bpermute(srcl4, my_c);
                r_oy[j] = __builtin_amdgcn_ds_bpermute(srcl4, my_a) + gsrc * 16;      // + lane_part (plain modes: the lane's granule)
                r_ox[j] = __builtin_amdgcn_ds_bpermute(srcl4, my_b) + gsrc * 16;
            }
        }
#pragma unroll
        for (int j = 0; j < T::kPLoads; ++j) {
            const int m = ptile * BP + (j * NW + wave) * RPI + lrow;
            if constexpr (FG && !X3) {
                (void)m;
            } else if constexpr (FG) {
                if (m < p.M) {
                    // (timing probe, variant flag bit 5 / SBBSEG_CONV_PROBE_LOCAL=1: every staged row gathers from the first 1 024 output pixels'
                    //  neighbourhood -- real data, but L2-resident: what the loop does when no pixel load misses.  Results are wrong.)
                    const int mg = SBBSEG_PROBE(p.variant_flags & 32) ? (m & 1023) : m;
                    int n, oy, ox;
                    decode_m(mg, cls, n, oy, ox);
                    r_oy[j] = (int)((uint32_t)n * img0 + (uint32_t)(((oy << sd0.sy_shift) * sd0.PW + (ox << sd0.sx_shift)) * sd0.pix_bytes) +
                                    lane_part(sd0) + (uint32_t)kZeroHeaderBytes);
                    uint32_t inv = p.fast_gather == 2 ? 0u : oob_mask(sd0, oy, ox);
                    if (p.n_src > 1) {
                        r_ox[j] = (int)((uint32_t)n * img1 + (uint32_t)(((oy << sd1.sy_shift) * sd1.PW + (ox << sd1.sx_shift)) * sd1.pix_bytes) +
                                        lane_part(sd1) + (uint32_t)kZeroHeaderBytes);
                        if (p.fast_gather != 2) inv |= oob_mask(sd1, oy, ox) << 16;
                    } else {
                        r_ox[j] = 0;
                    }
                    r_n[j] = (int)inv;
                } else {
                    r_oy[j] = 0;
                    r_ox[j] = 0;
                    r_n[j] = -1;                            // every tap out of bounds -> zero rows
                }
            } else if (m < p.M) {
                int n, oy, ox;
                decode_m(m, cls, n, oy, ox);
                r_oy[j] = oy;
                r_ox[j] = ox;
                r_n[j] = n;
            } else {
                r_oy[j] = -(1 << 20);                   // always out of bounds -> zero granule
                r_ox[j] = 0;
                r_n[j] = 0;
            }
        }
#pragma unroll
        for (int j = 0; j < T::kWLoads; ++j)
            w_off[j] = (uint32_t)((ctile * BC + min((j * NW + wave) * RPI + lrow, BC - 1)) * p.Ktot + gsrc * 8) * 2u;
    };

    int l_t = 0, l_h = 0, l_q = 0, issued = 0;          // load side: K-step, stage inside it, tile
    int l_end = nt;                                     // (split-K: the K-step behind this split's range)
    int rec_yx = kstep_tab[0], rec_coff = kstep_tab[1], rec_irr = kstep_tab[2];   // record of the NEXT stage issued
    auto issue = [&](int buf) __attribute__((always_inline)) {
        const int t = l_t;
        const bool s1 = t >= ks0;
        char* lds_p = smem + buf * T::kStageBytes;
        char* lds_w = lds_p + BP * RB;
        if constexpr (FG) {
            // the fast gather's K-step records (FgStepRec, built by the host) hold the wave-uniform part of the address --
            // tap displacement + channel offset + the resource's bias -- and the tap's bit in the rows' out-of-bounds masks
            const uint32_t soff = (uint32_t)rec_yx + (uint32_t)(X3 ? 0 : l_h * GS * 16);
            const int tapbit = rec_coff;
            auto rows = [&](const char* rbase, uint32_t nrec, const int (&voff)[T::kPLoads]) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < T::kPLoads; ++j) {
                    const uint32_t oob = (uint32_t)__builtin_amdgcn_sbfe(r_n[j], tapbit, 1);      // 0 or ~0
                    const uint32_t off = (oob & 0x80000000u) | (uint32_t)voff[j];
                    buffer_load_lds16(rbase, nrec, (LDS_AS void*)(lds_p + (j * NW + wave) * 1024), off, soff);
                }
            };
            if (s1) rows(sd1.base - fg_bias1, sd1.bytes + fg_bias1, r_ox); else rows(sd0.base - fg_bias0, sd0.bytes + fg_bias0, r_oy);
            // (timing probe, variant flag bit 6 / SBBSEG_CONV_PROBE_WHOT=1: the weight rows of every K-step come from the tile's first sixteen
            //  K-steps -- an L2-resident 32-64 KB per channel tile.  Results are wrong.)
            const uint32_t woff = (uint32_t)((SBBSEG_PROBE(p.variant_flags & 64) ? (t & 15) : t) * (kBK * 2) + l_h * GS * 16);
#pragma unroll
            for (int j = 0; j < T::kWLoads; ++j)
                buffer_load_lds16(wbase, 0x7fffffffu, (LDS_AS void*)(lds_w + (j * NW + wave) * 1024), w_off[j], woff);
        } else {
        const char* base = s1 ? sd1.base : sd0.base;
        const int rowbytes = s1 ? sd1.PW * sd1.pix_bytes : sd0.PW * sd0.pix_bytes;
        const int pixb = s1 ? sd1.pix_bytes : sd0.pix_bytes;
        const uint32_t img = s1 ? img1 : img0;
        const int sh = s1 ? sd1.shift : sd0.shift;
        const int ssy = s1 ? sd1.sy_shift : sd0.sy_shift, ssx = s1 ? sd1.sx_shift : sd0.sx_shift;
        const unsigned lim_y = s1 ? sd1.lim_y : sd0.lim_y, lim_x = s1 ? sd1.lim_x : sd0.lim_x;
        const int gfull = l_h * GS + gsrc;                     // granule inside the 64-element K-step
        int dy = (int)(short)(rec_yx & 0xffff), dx = rec_yx >> 16;
        // slots 4-7 sit lo_off bytes behind slots 0-3: 64 in the plain modes (= gfull * 16), the lo plane in split mode
        int coff = rec_coff + (X3 ? (gfull & 3) * 16 + (gfull >> 2) * (s1 ? sd1.lo_off : sd0.lo_off) : gfull * 16) + kZeroHeaderBytes;
        if (rec_irr) {                                         // granules of this step differ in tap
            const KTabEntry e = ktab[t * kGranulesPerStep + gfull];
            dy = e.dy; dx = e.dx; coff = e.coff + kZeroHeaderBytes;
        }
#pragma unroll
        for (int j = 0; j < T::kPLoads; ++j) {
            const int uy = (r_oy[j] << ssy) + dy;           // dy/dx carry tap - pad - placement offset
            const int ux = (r_ox[j] << ssx) + dx;
            const bool ok = ((unsigned)uy < lim_y) & ((unsigned)ux < lim_x);
            const int yy = uy >> sh, xx = ux >> sh;
            // yy, xx < 2^12 and rowbytes, pixb < 2^24: 24-bit multiplies are exact (full-rate VALU)
            uint32_t off = (uint32_t)r_n[j] * img + __umul24(yy, rowbytes) + __umul24(xx, pixb) + (uint32_t)coff;
            off = ok ? off : 0u;
            // (a non-temporal policy on these loads was measured 5-35 % slower: the tap re-reads live in L2)
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(base + off),
                                             (LDS_AS void*)(lds_p + (j * NW + wave) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < T::kWLoads; ++j) {
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(wbase + w_off[j] + (uint32_t)(t * (kBK * 2) + l_h * GS * 16)),
                                             (LDS_AS void*)(lds_w + (j * NW + wave) * 1024), 16, 0, 0);
        }
        }
        // advance the load side; crossing into the next tile re-derives the gather rows
        ++issued;
        if (++l_h == SPK) {
            l_h = 0;
            if (++l_t == (KS ? l_end : nt)) {
                l_t = 0;
                if (++l_q < my_tiles) {
                    setup_rows(tile_at(l_q));
                    if constexpr (KS) l_t = split_of(tile_at(l_q)) * nt;
                }
                if constexpr (KS) l_end = l_t + nt;
            }
            rec_yx = kstep_tab[l_t * 4 + 0]; rec_coff = kstep_tab[l_t * 4 + 1]; rec_irr = kstep_tab[l_t * 4 + 2];
        }
    };

    f4_t acc[T::kMI][T::kNI];
#pragma unroll
    for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
        for (int ni = 0; ni < T::kNI; ++ni) acc[mi][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};

    // LDS read offsets: row r, granule g lives at r*128 + ((g ^ (r & 7)) * 16)
    const int frow = lane & 15;
    const int fg = lane >> 4;
    const int fswz = GS == 8 ? (frow & 7) : ((0x78 >> (2 * ((frow >> 2) & 3))) & 3);
    const int rd_k0 = frow * RB + (((0 + fg) ^ fswz) << 4);
    const int rd_k1 = frow * RB + (((4 + fg) ^ fswz) << 4);        // second k-half of a whole-K-step stage (GS == 8)
    const int p_rd = (wp * T::kWPX) * RB;
    const int w_rd = BP * RB + (wc * T::kWCH) * RB;

    // ---- epilogue of one finished tile.  Weight rows are packed in the order conv_row_channel()
    // gives, so the two MFMA row blocks (2s, 2s+1) of a lane hold 8 CONSECUTIVE channels of one
    // pixel: 16-byte NHWC stores / residual loads, 64 contiguous bytes per pixel per instruction.
    // linear pixel index inside the output tensor(s) for output-grid pixel m (placement: see ConvParams)
    const bool placed = (p.osy != 1) | (p.osx != 1) | (p.ooy != 0) | (p.oox != 0) | (p.TH != p.Ho) | (p.TW != p.Wo) | (p.n_cls > 1) | (FG && p.rmap != nullptr);
    auto out_pixel = [&](int m, int cls) __attribute__((always_inline)) -> int {
        if (!placed) return m;
        int n, oy, ox;
        decode_m(m, cls, n, oy, ox);
        const int ooy = p.n_cls > 1 ? p.ooy_cls[cls] : p.ooy, oox = p.n_cls > 1 ? p.oox_cls[cls] : p.oox;
        return (n * p.TH + oy * p.osy + ooy) * p.TW + ox * p.osx + oox;
    };

    // residual tile of the tile being finished: requested BEFORE its last K-step's MFMAs so the HBM
    // round trip hides under them
    // (big wave tiles cannot spare the registers; the split mode's hi + lo pairs fit beside the 128x128 tile's 187 registers only)
    constexpr bool kPrefetchRes = T::prefetches_residual(X3);
    uint4 res[kPrefetchRes ? T::kMI / 2 : 1][kPrefetchRes ? T::kNI : 1];
    uint4 res_lo[kPrefetchRes && X3 ? T::kMI / 2 : 1][kPrefetchRes && X3 ? T::kNI : 1];      // split mode: the lo halves
    auto prefetch_residual = [&](int tile) __attribute__((always_inline)) {
        int ctile, cls, ptile;
        decode(tile, ctile, cls, ptile);
#pragma unroll
        for (int ni = 0; ni < T::kNI; ++ni) {
            const int m = ptile * BP + wp * T::kWPX + ni * 16 + frow;
            const int opix = m < p.M ? out_pixel(m, cls) : 0;
#pragma unroll
            for (int s2 = 0; s2 < T::kMI / 2; ++s2) {
                const int c0 = ctile * BC + wc * T::kWCH + s2 * 32 + fg * 8;
                if constexpr (kPrefetchRes) {
                    if (c0 < p.cout && m < p.M) {
                        const uint16_t* rp = (const uint16_t*)p.residual + (size_t)opix * (p.cout * PL) + (X3 ? split_hi_elem(p.cout, c0) : c0);
                        res[s2][ni] = *(const uint4*)rp;
                        if constexpr (X3) res_lo[s2][ni] = *(const uint4*)(rp + split_group(p.cout));
                    }
                }
            }
        }
    };

    // epilogue constants of the tile being finished, requested like the residual BEFORE the next
    // stage's loads are issued: vmcnt retires in order, so a load issued in the epilogue itself would
    // only return after the whole next stage has landed -- one extra round trip per tile on short-K layers
    constexpr bool kPrefetchConst = (T::kMI / 2) * T::kNI <= 8;
    float csc[kPrefetchConst ? T::kMI / 2 : 1][8], csh[kPrefetchConst ? T::kMI / 2 : 1][8];
    auto prefetch_consts = [&](int tile) __attribute__((always_inline)) {
        int ctile, cls, ptile;
        decode(tile, ctile, cls, ptile);
#pragma unroll
        for (int s2 = 0; s2 < T::kMI / 2; ++s2) {
            const int c0 = ctile * BC + wc * T::kWCH + s2 * 32 + fg * 8;
            if constexpr (kPrefetchConst) {
                if (c0 < p.cout) {
                    *(float4*)&csc[s2][0] = *(const float4*)(p.scale + c0);
                    *(float4*)&csc[s2][4] = *(const float4*)(p.scale + c0 + 4);
                    *(float4*)&csh[s2][0] = *(const float4*)(p.shift + c0);
                    *(float4*)&csh[s2][4] = *(const float4*)(p.shift + c0 + 4);
                    if constexpr (X3) {                          // undo the class's power-of-two weight pre-scale (exact)
                        const float wm = p.wmul_cls[cls];
#pragma unroll
                        for (int q = 0; q < 8; ++q) csc[s2][q] *= wm;
                    }
                }
            }
        }
    };

    // ---- epilogue of one finished tile.  Weight rows are packed in the order conv_row_channel()
    // gives, so the two MFMA row blocks (2s, 2s+1) of a lane hold 8 CONSECUTIVE channels of one
    // pixel: 16-byte NHWC stores / residual loads, 64 contiguous bytes per pixel per instruction.
    // Returns true when this wave issued EXACTLY kEpiStores (x2 with a raw copy) store instructions:
    // a full interior tile with a plain 16-bit output.  The caller may then leave those stores in
    // flight behind a counted wait (vmcnt retires loads and stores in issue order on gfx9-family
    // parts, and the staging loads were issued before the stores).
    auto epilogue = [&](int tile) __attribute__((always_inline)) -> bool {
        int ctile, cls, ptile;
        decode(tile, ctile, cls, ptile);
        if constexpr (KS) {
            // this split's partial sums, scaled by the class's power-of-two weight multiplier (exact), at the FINAL pixel index of the
            // output tensor: splitk_finish_x3 is then a plain elementwise pass over [pixels][cout]
            float* ws = p.ks_ws + (size_t)split_of(tile) * (size_t)p.ks_split_elems;
            const float wm = p.wmul_cls[cls];
#pragma unroll
            for (int ni = 0; ni < T::kNI; ++ni) {
                const int m = ptile * BP + wp * T::kWPX + ni * 16 + frow;
                if (m < p.M) {
                    const size_t o = (size_t)out_pixel(m, cls) * p.cout;
#pragma unroll
                    for (int s2 = 0; s2 < T::kMI / 2; ++s2) {
                        const int c0 = ctile * BC + wc * T::kWCH + s2 * 32 + fg * 8;
                        if (c0 < p.cout) {
                            const f4_t a = acc[2 * s2][ni], b = acc[2 * s2 + 1][ni];
                            *(float4*)(ws + o + c0) = make_float4(a[0] * wm, a[1] * wm, a[2] * wm, a[3] * wm);
                            *(float4*)(ws + o + c0 + 4) = make_float4(b[0] * wm, b[1] * wm, b[2] * wm, b[3] * wm);
                        }
                    }
                }
            }
#pragma unroll
            for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                for (int ni = 0; ni < T::kNI; ++ni) acc[mi][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};
            return false;
        }
        const bool full = (ptile * BP + (wp + 1) * T::kWPX <= p.M) && (ctile * BC + (wc + 1) * T::kWCH <= p.cout) &&
                          p.out != nullptr && !(BC == 32 && p.head_classes > 0);
        int opix[T::kNI];
#pragma unroll
        for (int ni = 0; ni < T::kNI; ++ni) {
            const int m = ptile * BP + wp * T::kWPX + ni * 16 + frow;
            opix[ni] = m < p.M ? out_pixel(m, cls) : -1;
        }
        if constexpr (T::kMI % 4 == 0 && !X3) {
            // Full interior tile: whole-line stores.  A lane holds 8 channels of pixel `frow` from row-block
            // pair s2 (A) and from pair s2+1 (B); lanes frow and frow^8 swap "B of the low pixel" against
            // "A of the high pixel" (one DPP row rotate), after which each store instruction writes 8
            // pixels x 128 contiguous, line-aligned bytes instead of 16 pixels x 64 (half lines).
            if (full && !p.raw_out && !(p.variant_flags & 2)) {
                const bool hi = (frow & 8) != 0;
#pragma unroll
                for (int sp = 0; sp < T::kMI / 4; ++sp) {
                    const int cA = ctile * BC + wc * T::kWCH + sp * 64 + fg * 8;
                    const int cst = cA + (hi ? 32 : 0);
                    float sc[2][8], sh[2][8];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if constexpr (kPrefetchConst) {
#pragma unroll
                            for (int q = 0; q < 8; ++q) { sc[h][q] = csc[sp * 2 + h][q]; sh[h][q] = csh[sp * 2 + h][q]; }
                        } else {
                            *(float4*)&sc[h][0] = *(const float4*)(p.scale + cA + h * 32);
                            *(float4*)&sc[h][4] = *(const float4*)(p.scale + cA + h * 32 + 4);
                            *(float4*)&sh[h][0] = *(const float4*)(p.shift + cA + h * 32);
                            *(float4*)&sh[h][4] = *(const float4*)(p.shift + cA + h * 32 + 4);
                        }
                    }
#pragma unroll
                    for (int ni = 0; ni < T::kNI; ++ni) {
                        uint4 r[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int s2 = sp * 2 + h;
                            float y[8];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                y[q] = __builtin_fmaf(acc[2 * s2][ni][q], sc[h][q], sh[h][q]);
                                y[4 + q] = __builtin_fmaf(acc[2 * s2 + 1][ni][q], sc[h][4 + q], sh[h][4 + q]);
                            }
                            if (p.residual) {
                                uint4 rr;
                                if constexpr (kPrefetchRes) rr = res[s2][ni];
                                else rr = *(const uint4*)((const uint16_t*)p.residual + (size_t)opix[ni] * p.cout + cA + h * 32);
                                y[0] += unpack_lo<F16>(rr.x); y[1] += unpack_hi<F16>(rr.x);
                                y[2] += unpack_lo<F16>(rr.y); y[3] += unpack_hi<F16>(rr.y);
                                y[4] += unpack_lo<F16>(rr.z); y[5] += unpack_hi<F16>(rr.z);
                                y[6] += unpack_lo<F16>(rr.w); y[7] += unpack_hi<F16>(rr.w);
                            }
                            if (p.relu) {
#pragma unroll
                                for (int q = 0; q < 8; ++q) y[q] = fmaxf(y[q], 0.f);
                            }
                            r[h].x = pack2<F16>(y[0], y[1]); r[h].y = pack2<F16>(y[2], y[3]);
                            r[h].z = pack2<F16>(y[4], y[5]); r[h].w = pack2<F16>(y[6], y[7]);
                        }
                        uint4 give, recv;
                        give.x = hi ? r[0].x : r[1].x; give.y = hi ? r[0].y : r[1].y;
                        give.z = hi ? r[0].z : r[1].z; give.w = hi ? r[0].w : r[1].w;
                        recv.x = row_ror8(give.x); recv.y = row_ror8(give.y);
                        recv.z = row_ror8(give.z); recv.w = row_ror8(give.w);
                        const int o_other = (int)row_ror8((uint32_t)opix[ni]);
                        const int pix0 = hi ? o_other : opix[ni], pix1 = hi ? opix[ni] : o_other;
                        uint4 st0, st1;
                        st0.x = hi ? recv.x : r[0].x; st0.y = hi ? recv.y : r[0].y;
                        st0.z = hi ? recv.z : r[0].z; st0.w = hi ? recv.w : r[0].w;
                        st1.x = hi ? r[1].x : recv.x; st1.y = hi ? r[1].y : recv.y;
                        st1.z = hi ? r[1].z : recv.z; st1.w = hi ? r[1].w : recv.w;
                        *(uint4*)((uint16_t*)p.out + (size_t)pix0 * p.cout + cst) = st0;
                        *(uint4*)((uint16_t*)p.out + (size_t)pix1 * p.cout + cst) = st1;
                    }
                }
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < T::kNI; ++ni) acc[mi][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};
                return true;
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < T::kMI / 2; ++s2) {
            const int c0 = ctile * BC + wc * T::kWCH + s2 * 32 + fg * 8;
            if (c0 < p.cout) {
                float sc[8], sh[8], rsc[8], rsh[8];
                if constexpr (kPrefetchConst) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) { sc[q] = csc[s2][q]; sh[q] = csh[s2][q]; }
                } else {
                    *(float4*)&sc[0] = *(const float4*)(p.scale + c0);
                    *(float4*)&sc[4] = *(const float4*)(p.scale + c0 + 4);
                    *(float4*)&sh[0] = *(const float4*)(p.shift + c0);
                    *(float4*)&sh[4] = *(const float4*)(p.shift + c0 + 4);
                    if constexpr (X3) {
#pragma unroll
                        for (int q = 0; q < 8; ++q) sc[q] *= p.wmul_cls[cls];
                    }
                }
                if (p.raw_out) {
                    *(float4*)&rsc[0] = *(const float4*)(p.raw_scale + c0);
                    *(float4*)&rsc[4] = *(const float4*)(p.raw_scale + c0 + 4);
                    *(float4*)&rsh[0] = *(const float4*)(p.raw_shift + c0);
                    *(float4*)&rsh[4] = *(const float4*)(p.raw_shift + c0 + 4);
                    if constexpr (X3) {
#pragma unroll
                        for (int q = 0; q < 8; ++q) rsc[q] *= p.wmul_cls[cls];
                    }
                }
#pragma unroll
                for (int ni = 0; ni < T::kNI; ++ni) {
                    float v[8], y[8];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { v[q] = acc[2 * s2][ni][q]; v[4 + q] = acc[2 * s2 + 1][ni][q]; }
#pragma unroll
                    for (int q = 0; q < 8; ++q) y[q] = __builtin_fmaf(v[q], sc[q], sh[q]);
                    // element offset of the pixel's channel group; the split mode stores [C hi][C lo] per pixel
                    const size_t o = (size_t)(opix[ni] < 0 ? 0 : opix[ni]) * (p.cout * PL) + (X3 ? split_hi_elem(p.cout, c0) : c0);
                    const int lo_d = split_group(p.cout);                  // (split mode: halves from a group's hi to its lo part)
                    if (opix[ni] >= 0) {
                        if (p.raw_out) {
                            float rv[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) rv[q] = v[q] * rsc[q] + rsh[q];
                            if constexpr (X3) store_split8((uint16_t*)p.raw_out + o, lo_d, rv);
                            else {
                                uint4 r;
                                r.x = pack2<F16>(rv[0], rv[1]); r.y = pack2<F16>(rv[2], rv[3]);
                                r.z = pack2<F16>(rv[4], rv[5]); r.w = pack2<F16>(rv[6], rv[7]);
                                *(uint4*)((uint16_t*)p.raw_out + o) = r;
                            }
                        }
                        if (p.residual) {
                            if constexpr (X3 && kPrefetchRes) {
                                const h8_t h = __builtin_bit_cast(h8_t, res[s2][ni]), l = __builtin_bit_cast(h8_t, res_lo[s2][ni]);
#pragma unroll
                                for (int q = 0; q < 8; ++q) y[q] = __fadd_rn(y[q], __fadd_rn((float)h[q], (float)l[q]));      // (= add_split8)
                            } else if constexpr (X3) add_split8((const uint16_t*)p.residual + o, lo_d, y);
                            else {
                                uint4 rr;
                                if constexpr (kPrefetchRes) rr = res[s2][ni];
                                else rr = *(const uint4*)((const uint16_t*)p.residual + o);
                                y[0] += unpack_lo<F16>(rr.x); y[1] += unpack_hi<F16>(rr.x);
                                y[2] += unpack_lo<F16>(rr.y); y[3] += unpack_hi<F16>(rr.y);
                                y[4] += unpack_lo<F16>(rr.z); y[5] += unpack_hi<F16>(rr.z);
                                y[6] += unpack_lo<F16>(rr.w); y[7] += unpack_hi<F16>(rr.w);
                            }
                        }
                    }
                    if (p.relu) {
#pragma unroll
                        for (int q = 0; q < 8; ++q) y[q] = fmaxf(y[q], 0.f);
                    }
                    if (p.out && opix[ni] >= 0) {
                        if constexpr (X3) store_split8((uint16_t*)p.out + o, lo_d, y);
                        else {
                            uint4 r;
                            r.x = pack2<F16>(y[0], y[1]); r.y = pack2<F16>(y[2], y[3]);
                            r.z = pack2<F16>(y[4], y[5]); r.w = pack2<F16>(y[6], y[7]);
                            *(uint4*)((uint16_t*)p.out + o) = r;
                        }
                    }
                    if constexpr (BC == 32) {
                        // fused head: the 32 channels of a pixel sit in the 4 lanes {frow + 16*fg}; each
                        // lane contracts its 8 fp32 channels, two xor-shuffles add the partial logits
                        // (no 16-bit rounding between the last conv and the softmax)
                        if (p.head_classes > 0) {
                            float logit[4];
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                float a = 0.f;
                                if (c < p.head_classes) {
#pragma unroll
                                    for (int q = 0; q < 8; ++q) a = fmaf(y[q], p.head_w[(c0 + q) * p.head_classes + c], a);
                                }
                                a += __shfl_xor(a, 16);
                                a += __shfl_xor(a, 32);
                                logit[c] = a;
                            }
                            if (fg == 0 && opix[ni] >= 0) {
                                float mx = -3.0e38f;
#pragma unroll
                                for (int c = 0; c < 4; ++c)
                                    if (c < p.head_classes) { logit[c] = logit[c] * p.head_scale[c] + p.head_shift[c]; mx = fmaxf(mx, logit[c]); }
                                float pr[4], sum = 0.f;
#pragma unroll
                                for (int c = 0; c < 4; ++c)
                                    if (c < p.head_classes) { pr[c] = expf(logit[c] - mx); sum += pr[c]; }
                                int best = 0;
                                float bestp = -1.f;
#pragma unroll
                                for (int c = 0; c < 4; ++c)
                                    if (c < p.head_classes) {
                                        pr[c] = pr[c] / sum;
                                        if (pr[c] > bestp) { bestp = pr[c]; best = c; }      // first maximum wins (np.argmax)
                                        if (p.probs) p.probs[(size_t)opix[ni] * p.head_classes + c] = pr[c];
                                    }
                                p.labels[opix[ni]] = (uint8_t)best;
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
            for (int ni = 0; ni < T::kNI; ++ni) acc[mi][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};
        return full;
    };
    constexpr int kEpiStores = (T::kMI / 2) * T::kNI;             // store instructions per wave per output tensor

    if constexpr (PH8) {
        // ============================================================================================
        // 8-phase schedule (256 x 256 tile, 8 waves as 2 x 4, two K-steps = 8 phases per turn of the ring).
        // A K-step is staged as FOUR half-tiles of 16 KB -- W0/W1 = the two 32-channel halves of every
        // wave column, P0/P1 = the two 64-pixel halves of every wave row -- and a half-tile is restaged
        // (with the data of K-step k+2) as soon as both wave groups have taken their fragments from it,
        // not when the whole stage is spent: 5-6 phases of lead time instead of 4 in the same 128 KB.
        // Each phase = [fragment reads + one half-tile issued + counted vmcnt] barrier [16 MFMAs] barrier;
        // waves 4-7 run one barrier behind waves 0-3, so one group's memory half overlaps the other's
        // matrix half on every SIMD.
        //   phase of K-step k :   1            2            3            4
        //   fragments read    :   W0 P0        W1           P1           -
        //   quadrant (W,P)    :   (0,0)        (1,0)        (1,1)        (0,1)
        //   half-tile issued  :   W1(k+1)      P1(k+1)      W0(k+2)      P0(k+2)
        // ============================================================================================
        static_assert(BP == 256 && BC == 256 && WP == 2 && WC == 4 && NS == 2 && GS == 8, "8-phase schedule is built for the 256x256 tile");
        if (my_tiles == 0) return;
        const int total_k = my_tiles * nt;                       // K-steps this block walks
        constexpr int kHalf = 16384;
        // ---- load side
        int q_oy[4], q_ox[4], q_n[4];                            // P rows of this thread: [h*2 + i]
        uint32_t q_w[4];                                         // W rows: [g*2 + i]
        auto setup8 = [&](int tile) __attribute__((always_inline)) {
            int ctile, cls, ptile;
            decode(tile, ctile, cls, ptile);
            if (p.n_cls > 1) {
                wbase = (const char*)p.w_cls[cls];
                kstep_tab = (const __attribute__((address_space(4))) int*)(uintptr_t)p.kstep_cls[cls];
                ktab = p.ktab_cls[cls];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rho = ((j & 1) * 8 + wave) * 8 + lrow;            // row inside the half-tile
                const int m = ptile * BP + (rho >> 6) * 128 + (j >> 1) * 64 + (rho & 63);
                if (m < p.M) {
                    // (no owned-region table on this schedule: ph8_ok() keeps launches with a table off it -- the lookup's registers spill here)
                    const int n = fast_div(m, p.howo_magic, p.howo_shift);
                    const int rem = m - n * HoWo;
                    int oy, ox;
                    decode_yx(rem, oy, ox);
                    q_oy[j] = oy; q_ox[j] = ox; q_n[j] = n;
                } else {
                    q_oy[j] = -(1 << 20); q_ox[j] = 0; q_n[j] = 0;
                }
                const int crow = (rho >> 5) * 64 + (j >> 1) * 32 + (rho & 31);
                q_w[j] = (uint32_t)((ctile * BC + min(crow, BC - 1)) * p.Ktot + gsrc * 8) * 2u;
            }
        };
        int i_t = 0, i_q = 0, i_k = 0;                           // issue side: K-step in tile, tile, K-step overall
        int r8_yx = 0, r8_coff = 0;
        auto load_rec = [&]() __attribute__((always_inline)) {
            r8_yx = kstep_tab[i_t * 4 + 0]; r8_coff = kstep_tab[i_t * 4 + 1];
        };
        // one half-tile of K-step i_k: part 0 = W0, 1 = P0, 2 = W1, 3 = P1 (issued in this order)
        auto issue_part = [&](int part, bool checked = true) __attribute__((always_inline)) {
            if (checked && i_k >= total_k) return;
            char* half = smem + (i_k & 1) * (4 * kHalf) + ((part & 1) ? 2 * kHalf : 0) + (part >> 1) * kHalf;
            if (!(part & 1)) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(wbase + q_w[(part >> 1) * 2 + i] + (uint32_t)(i_t * (kBK * 2))),
                                                     (LDS_AS void*)(half + (i * 8 + wave) * 1024), 16, 0, 0);
            } else {
                const bool s1 = i_t >= ks0;
                const char* base = s1 ? sd1.base : sd0.base;
                const int rowbytes = s1 ? sd1.PW * sd1.pix_bytes : sd0.PW * sd0.pix_bytes;
                const int pixb = s1 ? sd1.pix_bytes : sd0.pix_bytes;
                const uint32_t img = s1 ? img1 : img0;
                const int sh = s1 ? sd1.shift : sd0.shift;
                const int ssy = s1 ? sd1.sy_shift : sd0.sy_shift, ssx = s1 ? sd1.sx_shift : sd0.sx_shift;
                const unsigned lim_y = s1 ? sd1.lim_y : sd0.lim_y, lim_x = s1 ? sd1.lim_x : sd0.lim_x;
                const int dy = (int)(short)(r8_yx & 0xffff), dx = r8_yx >> 16;
                const int coff = r8_coff + gsrc * 16 + kZeroHeaderBytes;
                // (irregular K-steps -- 8-channel sources -- never reach this schedule: ph8_ok())
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int j = (part >> 1) * 2 + i;
                    const int uy = (q_oy[j] << ssy) + dy, ux = (q_ox[j] << ssx) + dx;
                    const bool ok = ((unsigned)uy < lim_y) & ((unsigned)ux < lim_x);
                    const int yy = uy >> sh, xx = ux >> sh;
                    uint32_t off = (uint32_t)q_n[j] * img + __umul24(yy, rowbytes) + __umul24(xx, pixb) + (uint32_t)coff;
                    off = ok ? off : 0u;
                    __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(base + off), (LDS_AS void*)(half + (i * 8 + wave) * 1024), 16, 0, 0);
                }
            }
            if (part == 3) {                                     // K-step complete: advance
                ++i_k;
                if (++i_t == nt) {
                    i_t = 0;
                    ++i_q;
                    if (!checked || i_q < my_tiles) setup8(tile_at(i_q));
                }
                if (!checked || i_k < total_k) load_rec();
            }
        };
        // ---- read side
        const int fsw0 = (((0 + fg) ^ (frow & 7)) << 4), fsw1 = (((4 + fg) ^ (frow & 7)) << 4);
        const int a_row = (wc * 32 + frow) * 128, b_row = (wp * 64 + frow) * 128;
        bf16x8_t aw[2][2][2], bp[4][2];                          // [g][m2][kk], [n4][kk]
        auto read_w = [&](const char* buf, int g) __attribute__((always_inline)) {
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2) {
                aw[g][m2][0] = *(const bf16x8_t*)(buf + g * kHalf + a_row + m2 * 2048 + fsw0);
                aw[g][m2][1] = *(const bf16x8_t*)(buf + g * kHalf + a_row + m2 * 2048 + fsw1);
            }
        };
        auto read_p = [&](const char* buf, int h) __attribute__((always_inline)) {
#pragma unroll
            for (int n4 = 0; n4 < 4; ++n4) {
                bp[n4][0] = *(const bf16x8_t*)(buf + (2 + h) * kHalf + b_row + n4 * 2048 + fsw0);
                bp[n4][1] = *(const bf16x8_t*)(buf + (2 + h) * kHalf + b_row + n4 * 2048 + fsw1);
            }
        };
        auto quad = [&](int g, int h) __attribute__((always_inline)) {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                    for (int n4 = 0; n4 < 4; ++n4)
                        acc[g * 2 + m2][h * 4 + n4] = mfma16<F16>(aw[g][m2][kk], bp[n4][kk], acc[g * 2 + m2][h * 4 + n4]);
            __builtin_amdgcn_s_setprio(0);
        };
        // after this phase's issue: everything but the 4 youngest half-tiles (8 loads) has landed; once the
        // stream has ended the count no longer says anything -> drain
        auto phase_wait = [&](bool checked = true) __attribute__((always_inline)) {
            if (!checked || i_k < total_k) wait_vmcnt<8>();
            else wait_vmcnt<0>();
        };

        // ---- prologue: K-step 0 complete and W0, P0 of K-step 1 issued; K-step 0's first halves landed
        setup8(tile_at(0));
        load_rec();
        issue_part(0); issue_part(1); issue_part(2); issue_part(3);
        issue_part(0); issue_part(1);
        phase_wait();
        __builtin_amdgcn_s_barrier();
        if (wave >= 4) __builtin_amdgcn_s_barrier();             // second group runs one barrier behind

        int c_t8 = 0, c_q8 = 0;
        // one K-step = four phases; `checked` = the stream may end inside this K-step (last two K-steps only):
        // the steady-state body carries no end-of-stream branches -- the memory half of a phase has to be short
        auto kstep8 = [&](int k, bool checked) __attribute__((always_inline)) {
            const char* buf = smem + (k & 1) * (4 * kHalf);
            // phase 1
            read_w(buf, 0); read_p(buf, 0);
            issue_part(2, checked);
            phase_wait(checked);
            __builtin_amdgcn_s_barrier();
            quad(0, 0);
            __builtin_amdgcn_s_barrier();
            // phase 2
            read_w(buf, 1);
            issue_part(3, checked);
            phase_wait(checked);
            __builtin_amdgcn_s_barrier();
            quad(1, 0);
            __builtin_amdgcn_s_barrier();
            // phase 3
            read_p(buf, 1);
            issue_part(0, checked);
            phase_wait(checked);
            __builtin_amdgcn_s_barrier();
            quad(1, 1);
            __builtin_amdgcn_s_barrier();
            // phase 4
            issue_part(1, checked);
            phase_wait(checked);
            __builtin_amdgcn_s_barrier();
            quad(0, 1);
            if (++c_t8 == nt) {                                  // tile finished
                epilogue(tile_at(c_q8));
                c_t8 = 0;
                ++c_q8;
            }
            __builtin_amdgcn_s_barrier();
        };
        int k8 = 0;
        for (; k8 + 2 < total_k; ++k8) kstep8(k8, false);
        for (; k8 < total_k; ++k8) kstep8(k8, true);
        if (wave < 4) __builtin_amdgcn_s_barrier();              // balance the second group's extra barrier
        return;
    }

    // ---- prologue: D stages in flight, stage 0 landed
    if (total == 0) return;
    setup_rows(tile_at(0));
    if constexpr (KS) { l_t = split_of(tile_at(0)) * nt; l_end = l_t + nt; }
    rec_yx = kstep_tab[l_t * 4 + 0]; rec_coff = kstep_tab[l_t * 4 + 1]; rec_irr = kstep_tab[l_t * 4 + 2];     // (the first tile's class may not be class 0)
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < total) issue(d);
    if (D >= 2 && total >= D) wait_vmcnt<T::kLoads*(D >= 2 ? D - 1 : 0)>();     // stage 0 landed, D-1 stages stay in flight
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();

    int cur = 0, nxt = D % NS, c_t = 0, c_q = 0;
    for (int s = 0; s < total; ++s) {
        if (c_t == nts - 1) {                               // last stage of a tile: its epilogue inputs go first
            if (kPrefetchConst) prefetch_consts(tile_at(c_q));
            if (kPrefetchRes && p.residual) prefetch_residual(tile_at(c_q));
        }
        // 8-wave tiles of the plain 16-bit modes: waves NW/2.. (the SIMD partners of waves 0..NW/2-1) issue the next stage's loads in
        // the MIDDLE of the K-step, after their first half's MFMAs -- a stage's DMA issue costs a wave several hundred cycles in which
        // it feeds no MFMAs; issued by all eight waves right after the barrier those cycles coincided on every SIMD.  f16: dec3 -8.6 %,
        // 128 -> 128 3x3 -6 %, dec1 / dec2 on 256 x 256 tiles -1.5 % (+1.1 % and +0.75 % throughput).  The split mode's 512 x 128 tile
        // gains the same 8 % per launch but has no register left for the second call site (one VGPR spilled) and its 256 x 256 tile
        // loses 1-3 %: plain modes only.  (variant flag bit 3 = off)
        constexpr bool kSplitIssue = !X3 && NW == 8 && !PH8 && NS == 2;
        const bool late_issue = kSplitIssue && wave >= NW / 2 && !(p.variant_flags & 8);
        if (!late_issue && issued < total) issue(nxt);
        const char* sb = smem + cur * T::kStageBytes;
        if constexpr (X3 && T::kNI >= 8) {
            // issue() has just requested the NEXT stage's K-step record through the scalar cache (s_load: lgkmcnt, may return out of order).
            // With it pending the compiler must wait lgkmcnt(0) -- for ALL sixteen fragment requests below -- in front of the first MFMA; a use
            // it can see makes it wait for the record HERE (a few dozen cycles, scalar cache hit), after which the fragment waits are counted.
            asm volatile("" ::"s"(rec_yx), "s"(rec_coff), "s"(rec_irr));
        }
        if constexpr (X3) {
            // split mode: slots 0-3 hold the hi halves of the stage's 32 channels, slots 4-7 the lo halves (rd_k0 / rd_k1
            // address exactly these).  value = hi + lo on both operands: w*x ~= wl*xh + wh*xl + wh*xh, small terms first.
            // Three sweeps over the wave tile keep MFMAs on the same accumulator 16 instructions apart.
            // Wide wave tiles (8 pixel blocks) take the pixel fragments in two halves: the fragments of a stage do not all fit
            // beside 128 accumulator registers.
            if constexpr (T::kNI >= 8) {
                // Wide wave tiles (8 pixel blocks: the 8-wave 256 x 256 and 512 x 128 tiles): phases of NQ pixel blocks, the pixel fragments of
                // phase i + 1 requested BEFORE the MFMAs of phase i (register double buffer: two sets of NQ hi + NQ lo fragments = the
                // registers one set of four blocks took).  Left to itself hipcc loads every fragment right in front of its first MFMA --
                // a dozen `s_waitcnt lgkmcnt(0)` per K-step, each exposing an LDS round trip to the matrix pipe.
                // Request order at the head of the K-step = the order of use: the first sweep (wl x xh) needs 4 + NQ fragments, not all 16 --
                // LDS returns in order, all eight waves ask at once behind the barrier (16 KB each: ~1 000 cycles of the LDS pipe for the
                // whole burst), and the matrix pipe idles until a wave's first operands are there.
                // (Per accumulator the order of its three MFMAs is unchanged: same bits.)
                constexpr int NQ = 2;
                constexpr int NPH = T::kNI / NQ;
                bf16x8_t ah[T::kMI], al[T::kMI];
                bf16x8_t bh[2][NQ], bl[2][NQ];
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi) al[mi] = *(const bf16x8_t*)(sb + w_rd + mi * 16 * RB + rd_k1);
#pragma unroll
                for (int q = 0; q < NQ; ++q) bh[0][q] = *(const bf16x8_t*)(sb + p_rd + q * 16 * RB + rd_k0);
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi) ah[mi] = *(const bf16x8_t*)(sb + w_rd + mi * 16 * RB + rd_k0);
#pragma unroll
                for (int q = 0; q < NQ; ++q) bl[0][q] = *(const bf16x8_t*)(sb + p_rd + q * 16 * RB + rd_k1);
                auto load_b = [&](int ph, bf16x8_t (&dh)[NQ], bf16x8_t (&dl)[NQ]) __attribute__((always_inline)) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        dh[q] = *(const bf16x8_t*)(sb + p_rd + (ph * NQ + q) * 16 * RB + rd_k0);
                        dl[q] = *(const bf16x8_t*)(sb + p_rd + (ph * NQ + q) * 16 * RB + rd_k1);
                    }
                };
#pragma unroll
                for (int ph = 0; ph < NPH; ++ph) {
                    if (ph + 1 < NPH) {
                        load_b(ph + 1, bh[(ph + 1) & 1], bl[(ph + 1) & 1]);
                        __builtin_amdgcn_sched_barrier(0);          // (the requests stay in FRONT of this phase's MFMAs)
                    }
#pragma unroll
                    for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                        for (int q = 0; q < NQ; ++q) acc[mi][ph * NQ + q] = mfma16<true>(al[mi], bh[ph & 1][q], acc[mi][ph * NQ + q]);
#pragma unroll
                    for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                        for (int q = 0; q < NQ; ++q) acc[mi][ph * NQ + q] = mfma16<true>(ah[mi], bl[ph & 1][q], acc[mi][ph * NQ + q]);
#pragma unroll
                    for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                        for (int q = 0; q < NQ; ++q) acc[mi][ph * NQ + q] = mfma16<true>(ah[mi], bh[ph & 1][q], acc[mi][ph * NQ + q]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                bf16x8_t ah[T::kMI], al[T::kMI];
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi) {
                    ah[mi] = *(const bf16x8_t*)(sb + w_rd + mi * 16 * RB + rd_k0);
                    al[mi] = *(const bf16x8_t*)(sb + w_rd + mi * 16 * RB + rd_k1);
                }
                bf16x8_t bh[T::kNI], bl[T::kNI];
#pragma unroll
                for (int q = 0; q < T::kNI; ++q) {
                    bh[q] = *(const bf16x8_t*)(sb + p_rd + q * 16 * RB + rd_k0);
                    bl[q] = *(const bf16x8_t*)(sb + p_rd + q * 16 * RB + rd_k1);
                }
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                    for (int q = 0; q < T::kNI; ++q) acc[mi][q] = mfma16<true>(al[mi], bh[q], acc[mi][q]);
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                    for (int q = 0; q < T::kNI; ++q) acc[mi][q] = mfma16<true>(ah[mi], bl[q], acc[mi][q]);
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                    for (int q = 0; q < T::kNI; ++q) acc[mi][q] = mfma16<true>(ah[mi], bh[q], acc[mi][q]);
            }
        } else {
            // The K-step's MFMAs run in phases of (k-half kk, group of <= 4 pixel blocks); the LDS
            // fragments of phase i+1 are requested BEFORE the MFMAs of phase i (register double
            // buffer).  hipcc on its own emits "all ds_reads, lgkmcnt(0), all MFMAs" per k-half, which
            // leaves the matrix pipe idle while all 8 waves of the block read LDS in lockstep.
            constexpr int NIH = T::kNI >= 8 ? T::kNI / 2 : T::kNI;     // pixel blocks per phase
            constexpr int NH = T::kNI / NIH;
            constexpr int NP = (GS / 4) * NH;                      // k-halves per stage x pixel-block groups
            bf16x8_t a[2][T::kMI], b[2][NIH];
            auto load_a = [&](int kk, bf16x8_t (&dst)[T::kMI]) __attribute__((always_inline)) {
                const int rd = kk ? rd_k1 : rd_k0;
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi) dst[mi] = *(const bf16x8_t*)(sb + w_rd + mi * 16 * RB + rd);
            };
            auto load_b = [&](int kk, int h, bf16x8_t (&dst)[NIH]) __attribute__((always_inline)) {
                const int rd = kk ? rd_k1 : rd_k0;
#pragma unroll
                for (int q = 0; q < NIH; ++q) dst[q] = *(const bf16x8_t*)(sb + p_rd + (h * NIH + q) * 16 * RB + rd);
            };
            load_a(0, a[0]);
            load_b(0, 0, b[0]);
#pragma unroll
            for (int ph = 0; ph < NP; ++ph) {
                const int kk = ph / NH, h = ph % NH;
                if (ph + 1 < NP) {
                    const int nkk = (ph + 1) / NH, nh = (ph + 1) % NH;
                    if (nh == 0) load_a(nkk, a[nkk & 1]);
                    load_b(nkk, nh, b[(ph + 1) & 1]);
                }
#pragma unroll
                for (int mi = 0; mi < T::kMI; ++mi)
#pragma unroll
                    for (int q = 0; q < NIH; ++q)
                        acc[mi][h * NIH + q] = mfma16<F16>(a[kk & 1][mi], b[ph & 1][q], acc[mi][h * NIH + q]);
                if constexpr (kSplitIssue) {
                    if (ph == NP / 2 - 1 && late_issue && issued < total) issue(nxt);
                }
            }
        }
        bool tile_done = false, counted = false;
        if (++c_t == nts) {                                 // tile finished: its stores overlap the
            counted = epilogue(tile_at(c_q));               // next tile's first stage(s), already in flight
            c_t = 0;
            ++c_q;
            tile_done = true;
        }
        if (s + 1 < total) {
            // stage s+1 must have landed; later issued stages stay in flight across the barrier, and
            // so do the stores of a tile that just finished (they are younger than every staging
            // load): a short-K layer otherwise pays a load AND a store round trip per tile, in series.
            constexpr int kAhead = T::kLoads * (D >= 2 ? D - 1 : 0);
            const bool ring_full = D < 2 || s + D < total;          // D-1 younger stages really are in flight
            if (tile_done) {
                if (counted && ring_full && !(p.variant_flags & 1)) {
                    if (p.raw_out) wait_vmcnt<kAhead + 2 * PL * kEpiStores>();      // (split mode: a hi and a lo store per group)
                    else wait_vmcnt<kAhead + PL * kEpiStores>();
                } else wait_vmcnt<0>();
            } else if (D >= 2 && ring_full) wait_vmcnt<kAhead>();
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
        }
        cur = cur + 1 == NS ? 0 : cur + 1;
        nxt = nxt + 1 == NS ? 0 : nxt + 1;
    }
}

// ------------------------------------------------------------------------------------------------
// conv_naive_f32 -- SBBSEG_PREC_F32 handles only: same gather table, plain fp32 FMA.  Slow on
// purpose-free grounds: it exists to separate plumbing errors from bf16 rounding in parity tests.
// One thread = one pixel x 4 channels.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_naive_f32(const ConvParams p)
{
    const int cgroups = p.cout / 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p.M * cgroups) return;
    const int m = (int)(idx / cgroups);
    const int c0 = (int)(idx - (long)m * cgroups) * 4;
    const int HoWo = p.Ho * p.Wo;
    const int n = m / HoWo;
    const int rem = m - n * HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* w = (const float*)p.w;
    int t = 0;
    for (int s = 0; s < p.n_src; ++s) {
        const SrcDesc sd = p.src[s];
        const int iy0 = oy << sd.sy_shift, ix0 = ox << sd.sx_shift;
        for (int ks = 0; ks < sd.ksteps; ++ks, ++t) {
            for (int g = 0; g < kGranulesPerStep; ++g) {
                const KTabEntry e = p.ktab[t * kGranulesPerStep + g];
                const int uy = iy0 + e.dy, ux = ix0 + e.dx;
                if (!(((unsigned)uy < (unsigned)sd.lim_y) & ((unsigned)ux < (unsigned)sd.lim_x))) continue;
                const int yy = uy >> sd.shift, xx = ux >> sd.shift;
                const float* xp = (const float*)(sd.base + kZeroHeaderBytes +
                                                 (size_t)((n * sd.PH + yy) * sd.PW + xx) * sd.pix_bytes + e.coff);
                const int k0 = (t * kGranulesPerStep + g) * 8;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float xv = xp[q];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = fmaf(xv, w[(size_t)(c0 + c) * p.Ktot + k0 + q], acc[c]);
                }
            }
        }
    }
    const size_t opix = (size_t)(n * p.TH + oy * p.osy + p.ooy) * p.TW + ox * p.osx + p.oox;
    const size_t o = opix * p.cout + c0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (p.raw_out) ((float*)p.raw_out)[o + c] = acc[c] * p.raw_scale[c0 + c] + p.raw_shift[c0 + c];
        if (p.out) {
            float y = acc[c] * p.scale[c0 + c] + p.shift[c0 + c];
            if (p.residual) y += ((const float*)p.residual)[o + c];
            if (p.relu) y = fmaxf(y, 0.f);
            ((float*)p.out)[o + c] = y;
        }
    }
}

// (magic, shift) with n / d == umulhi(n, magic) >> shift for every 0 <= n < 2^31; magic == 0: d is a power of two, n >> shift
static void make_fast_div(uint32_t d, uint32_t* magic, uint32_t* shift)
{
    if (d == 0) d = 1;
    uint32_t s2 = 0;
    while ((1u << (s2 + 1)) <= d && s2 < 31) ++s2;              // 2^s2 <= d < 2^(s2+1)
    if ((d & (d - 1)) == 0) { *magic = 0; *shift = s2; return; }
    const unsigned long long num = 1ull << (32 + s2);
    *magic = (uint32_t)((num + d - 1) / d);                       // ceil(2^(32+s2) / d), in (2^31, 2^32)
    *shift = s2;
}

template <int BP, int BC, int WP, int WC, int NS, bool F16, int GS, bool PH8, bool X3, bool FG, bool KS = false>
static hipError_t launch_conv_impl(const ConvParams& p, hipStream_t s, LaunchRec* rec)
{
    using T = ConvTile<BP, BC, WP, WC, NS, GS>;
    static bool attr_done[64] = {};
    const hipError_t e = dynamic_lds_once((const void*)conv_igemm_mfma<BP, BC, WP, WC, NS, F16, GS, PH8, X3, FG, KS>, T::kLdsBytes, attr_done);
    if (e != hipSuccess) return e;
    const int n_ct = (p.cout + BC - 1) / BC;
    const int n_pt = (p.M + BP - 1) / BP;
    const int n_tiles = (p.n_cls * n_ct * (p.cls_minor ? (n_pt + 7) & ~7 : n_pt)) << (KS ? p.ks_shift : 0);
    // persistent grid: as many blocks as are resident at once (2 per CU for the 4-wave tiles, 1 for
    // the 8-wave ones); p.persist_blocks == 0 -> one block per tile (A/B)
    const int resident = p.persist_blocks > 0 ? p.persist_blocks * T::kBlocksPerCU : n_tiles;
    int grid = n_tiles < resident ? n_tiles : resident;
    if (p.tile_map >= 1) grid = (grid + 7) & ~7;          // the XCD-grouped walk needs a multiple of 8 blocks
    if (rec) {
        launch_rec(rec, KS ? SBBSEG_LAUNCH_CONV_SPLITK : SBBSEG_LAUNCH_CONV_IGEMM, BP, BC, NS, n_tiles, grid, p.persist_blocks > 0, p.rmap != nullptr, p.residual != nullptr);
        rec->fast_gather = FG ? p.fast_gather : 0; rec->tile_map = p.tile_map; rec->cls_minor = p.cls_minor;
        rec->res_epilogue = p.residual && !KS && !T::prefetches_residual(X3);
    }
    ConvParams q = p;
    make_fast_div((uint32_t)(p.Ho * p.Wo), &q.howo_magic, &q.howo_shift);
    make_fast_div((uint32_t)p.Wo, &q.wo_magic, &q.wo_shift);
    make_fast_div((uint32_t)n_ct, &q.nct_magic, &q.nct_shift);
    hipLaunchKernelGGL((conv_igemm_mfma<BP, BC, WP, WC, NS, F16, GS, PH8, X3, FG, KS>), dim3(grid), dim3(T::kThreads), T::kLdsBytes, s, q);
    return hipGetLastError();
}

// One tile form in one precision mode: its fast-gather instantiation where the form has one and the launch takes it, else the plain gather's.
template <int BP, int BC, int WP, int WC, int NS, int GS, bool PH8, bool F16, bool X3>
static hipError_t launch_conv_tile(const ConvParams& p, const ConvForm& f, hipStream_t s, LaunchRec* rec)
{
    if constexpr (conv_tile_has_fg({BP, BC, WP, WC, NS, GS, PH8})) {
        if (f.fg) return launch_conv_impl<BP, BC, WP, WC, NS, F16, GS, PH8, X3, true>(p, s, rec);
    }
    return launch_conv_impl<BP, BC, WP, WC, NS, F16, GS, PH8, X3, false>(p, s, rec);
}

// ConvTileForm -> template arguments, checked against kConvTileDims (internal.h) at compile time
#define SBBSEG_CONV_TILE(T, BP, BC, WP, WC, NS, GS, PH8)                                                                                         \
    case T: {                                                                                                                                    \
        constexpr ConvTileDims d = kConvTileDims[T];                                                                                             \
        static_assert(d.bp == BP && d.bc == BC && d.wp == WP && d.wc == WC && d.ns == NS && d.gs == GS && d.ph8 == PH8, #T);                     \
        return launch_conv_tile<BP, BC, WP, WC, NS, GS, PH8, F16, X3>(p, f, s, rec);                                                             \
    }

// the plain 16-bit modes: all 13 tile forms (here and below in the order the ladders they replace named them: the instantiations keep their
// order in the code object)
template <bool F16>
static hipError_t launch_conv_form_16(const ConvParams& p, const ConvForm& f, hipStream_t s, LaunchRec* rec)
{
    constexpr bool X3 = false;
    if (p.ks_shift > 0) return launch_conv_impl<128, 128, 2, 2, 2, F16, 8, false, X3, true, true>(p, s, rec);
    switch (f.tile) {
    SBBSEG_CONV_TILE(kTile256x256Half, 256, 256, 2, 4, 4, 4, false)
    SBBSEG_CONV_TILE(kTile128x128Half, 128, 128, 2, 2, 4, 4, false)
    SBBSEG_CONV_TILE(kTile256x64Half, 256, 64, 4, 1, 4, 4, false)
    SBBSEG_CONV_TILE(kTile256x256Ph8, 256, 256, 2, 4, 2, 8, true)
    SBBSEG_CONV_TILE(kTile256x256, 256, 256, 2, 4, 2, 8, false)
    SBBSEG_CONV_TILE(kTile512x128, 512, 128, 4, 2, 2, 8, false)
    SBBSEG_CONV_TILE(kTile512x64, 512, 64, 8, 1, 2, 8, false)
    SBBSEG_CONV_TILE(kTile256x128S3, 256, 128, 4, 2, 3, 8, false)
    SBBSEG_CONV_TILE(kTile128x128, 128, 128, 2, 2, 2, 8, false)
    SBBSEG_CONV_TILE(kTile256x64S3, 256, 64, 8, 1, 3, 8, false)
    SBBSEG_CONV_TILE(kTile256x64, 256, 64, 4, 1, 2, 8, false)
    SBBSEG_CONV_TILE(kTile256x32S3, 256, 32, 8, 1, 3, 8, false)
    SBBSEG_CONV_TILE(kTile256x32, 256, 32, 4, 1, 2, 8, false)
    }
    return hipErrorInvalidValue;
}

// the split mode: the five forms choose_conv takes there
static hipError_t launch_conv_form_x3(const ConvParams& p, const ConvForm& f, hipStream_t s, LaunchRec* rec)
{
    constexpr bool F16 = true, X3 = true;
    if (p.ks_shift > 0) return launch_conv_impl<128, 128, 2, 2, 2, F16, 8, false, X3, true, true>(p, s, rec);
    switch (f.tile) {
    SBBSEG_CONV_TILE(kTile256x256, 256, 256, 2, 4, 2, 8, false)
    SBBSEG_CONV_TILE(kTile512x128, 512, 128, 4, 2, 2, 8, false)
    SBBSEG_CONV_TILE(kTile128x128, 128, 128, 2, 2, 2, 8, false)
    SBBSEG_CONV_TILE(kTile256x64, 256, 64, 4, 1, 2, 8, false)
    SBBSEG_CONV_TILE(kTile256x32, 256, 32, 4, 1, 2, 8, false)
    }
    return hipErrorInvalidValue;
}
#undef SBBSEG_CONV_TILE

// Second half of a split-K launch: partial sums of the 2^ks_shift splits added in split order, then the conv's epilogue -- scale / shift,
// residual, ReLU, store -- on 8 channels of one pixel per thread.  MODE 0 = split mode ([32 hi][32 lo] channel groups), 1 = fp16, 2 = bf16.
template <int MODE>
__global__ __launch_bounds__(256) void splitk_finish(const float* __restrict__ ws, int splits, long split_elems, long n_groups, int cout,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const uint16_t* __restrict__ residual, int relu, uint16_t* __restrict__ out)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const int cg = cout >> 3;
    const long pix = g / cg;
    const int c0 = (int)(g - pix * cg) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* src = ws + pix * cout + c0;
    for (int s = 0; s < splits; ++s) {
        const float4 a = *(const float4*)(src + (size_t)s * split_elems), b = *(const float4*)(src + (size_t)s * split_elems + 4);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = __builtin_fmaf(v[q], scale[c0 + q], shift[c0 + q]);
    if constexpr (MODE == 0) {
        const size_t o = (size_t)pix * (cout * 2) + split_hi_elem(cout, c0);
        const int lo_d = split_group(cout);
        if (residual) add_split8(residual + o, lo_d, y);
        if (relu) {
#pragma unroll
            for (int q = 0; q < 8; ++q) y[q] = fmaxf(y[q], 0.f);
        }
        store_split8(out + o, lo_d, y);
    } else {
        constexpr bool F16 = MODE == 1;
        const size_t o = (size_t)pix * cout + c0;
        if (residual) {                                         // (the same additions, in the same order, as conv_igemm_mfma's epilogue)
            const uint4 rr = *(const uint4*)(residual + o);
            y[0] += unpack_lo<F16>(rr.x); y[1] += unpack_hi<F16>(rr.x);
            y[2] += unpack_lo<F16>(rr.y); y[3] += unpack_hi<F16>(rr.y);
            y[4] += unpack_lo<F16>(rr.z); y[5] += unpack_hi<F16>(rr.z);
            y[6] += unpack_lo<F16>(rr.w); y[7] += unpack_hi<F16>(rr.w);
        }
        if (relu) {
#pragma unroll
            for (int q = 0; q < 8; ++q) y[q] = fmaxf(y[q], 0.f);
        }
        uint4 r;
        r.x = pack2<F16>(y[0], y[1]); r.y = pack2<F16>(y[2], y[3]);
        r.z = pack2<F16>(y[4], y[5]); r.w = pack2<F16>(y[6], y[7]);
        *(uint4*)(out + o) = r;
    }
}

hipError_t launch_splitk_finish(const float* ws, int splits, long split_elems, long pixels, int cout, const float* scale, const float* shift,
                                const void* residual, int relu, void* out, int precision, hipStream_t s)
{
    const long n_groups = pixels * (cout / 8);
    const dim3 grid((unsigned)((n_groups + 255) / 256));
    if (precision == kF16X3)
        hipLaunchKernelGGL(splitk_finish<0>, grid, dim3(256), 0, s, ws, splits, split_elems, n_groups, cout, scale, shift, (const uint16_t*)residual, relu, (uint16_t*)out);
    else if (precision == kF16)
        hipLaunchKernelGGL(splitk_finish<1>, grid, dim3(256), 0, s, ws, splits, split_elems, n_groups, cout, scale, shift, (const uint16_t*)residual, relu, (uint16_t*)out);
    else
        hipLaunchKernelGGL(splitk_finish<2>, grid, dim3(256), 0, s, ws, splits, split_elems, n_groups, cout, scale, shift, (const uint16_t*)residual, relu, (uint16_t*)out);
    return hipGetLastError();
}

// the launch of conv_choice.h's chosen form (kF32 handles: conv_naive_f32, whatever the form)
hipError_t launch_conv(const ConvParams& p, const ConvForm& form, int precision, hipStream_t s, LaunchRec* rec)
{
    if (precision == kF16X3) return launch_conv_form_x3(p, form, s, rec);
    if (precision == kF32) {
        const long total = (long)p.M * (p.cout / 4);
        launch_rec(rec, SBBSEG_LAUNCH_CONV_NAIVE_F32, 256, 4, 1, (int)((total + 255) / 256), (int)((total + 255) / 256), 0, 0, p.residual != nullptr);
        hipLaunchKernelGGL(conv_naive_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
        return hipGetLastError();
    }
    return precision == kF16 ? launch_conv_form_16<true>(p, form, s, rec) : launch_conv_form_16<false>(p, form, s, rec);
}

}  // namespace sbbseg
