// dec_tail.hip -- the network's last decoder conv and head in one launch: dec_tail_fused (16-bit modes) and dec_tail_fused_x3ps (split mode).
#include "tile_walk.h"

namespace sbbseg {

// ------------------------------------------------------------------------------------------------
// dec_tail_fused -- the network's last decoder conv and head in one kernel.
//
//   y   = ReLU(BN(conv3x3([up2(src0: 64 ch @ H/2 x W/2), image: 3 ch @ H x W])))     32 channels, fp32
//   out = argmax(softmax(BN(conv1x1(y))))                                            u8 label per pixel
//
// The generic implicit-GEMM kernel is address-bound here (32 output channels: 16 MFMAs per 256
// gathered rows).  This kernel is a direct conv on LDS-staged tiles instead:
//   * a block owns a 16x16 output tile; its 10x10 src0 halo tile (128 B per pixel) and 18x18
//     image halo tile (16 B per pixel) are copied to LDS once with global_load_lds (double
//     buffered across the persistent tile loop) -- every source pixel is fetched once, not 4-9 x
//   * the four waves are the four output-parity classes (py,px): for a fixed parity the 3x3 taps
//     on the upsampled src0 collapse to 2x2 taps with pre-summed weights (planner.py), so each
//     wave runs 4 K-steps of 64 channels on its 8x8 sub-grid + 2 K-steps for the 9 image taps
//   * the wave's weights (6 K-steps x 32 channels) live in 96 VGPRs in MFMA A-fragment order for
//     the whole kernel; only pixel fragments are read from LDS (ds_read_b128, XOR-swizzled rows)
//   * epilogue in registers: scale/shift/ReLU in fp32, the head's 32-channel contraction with two
//     xor-shuffles, softmax, argmax; labels are assembled in LDS and stored as 16-byte rows.
// ------------------------------------------------------------------------------------------------
constexpr int kTailSrcRowPx = 16;                       // LDS row stride of the src0 halo tile (10 used): stride = 0 mod 8
constexpr int kTailSrcBytes = 10 * kTailSrcRowPx * 128;      // 20 KB
constexpr int kTailImgRowPx = 32;                       // LDS row stride of the image halo tile (18 used)
constexpr int kTailImgBytes = 18 * kTailImgRowPx * 16;       // 9 KB
constexpr int kTailBufBytes = kTailSrcBytes + kTailImgBytes;
constexpr int kTailConstBytes = 32 * 8 * 4;                  // per channel: scale, shift, head_w[NC] (row of 4 or 8 floats)
constexpr int kTailLdsBytes = 2 * kTailBufBytes + 256 + 64 + kTailConstBytes;  // + label tile + zero granule + constants

template <bool F16, int NC>
__global__ __launch_bounds__(256, 2) void dec_tail_fused(const TailParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lbl_tile = smem + 2 * kTailBufBytes;                 // [16][16] u8
    char* zero_gran = lbl_tile + 256;                          // 16 zero bytes (image taps 9..15)
    float* cst = (float*)(zero_gran + 64);                     // [32 channels][8]: scale, shift, head_w[0..3]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int py = wave >> 1, px = wave & 1;
    const int frow = lane & 15, fg = lane >> 4;

    const int H = 2 * p.PH, W = 2 * p.PW;
    const int tiles_x = W / 16, tiles_y = H / 16;
    const int tiles_per_patch = tiles_x * tiles_y;
    // owned-region launch (TailParams::ttab, region.h): the tiles are the table's entries -- (patch, output origin / 2), x origins multiples
    // of 16 (label rows are stored 16 bytes at a time) -- instead of every 16 x 16 tile of every patch
    const int n_tiles = p.ttab ? p.n_tab : p.n * tiles_per_patch;
    const __attribute__((address_space(4))) uint32_t* ttab = (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)p.ttab;
    auto tile_origin = [&](int tile, int& n, int& y0, int& x0) __attribute__((always_inline)) {
        if (ttab) {
            const uint32_t code = ttab[tile];
            n = (int)(code >> 22); y0 = (int)((code >> 11) & 2047u) * 2; x0 = (int)(code & 2047u) * 2;
        } else {
            n = tile / tiles_per_patch;
            const int rem = tile - n * tiles_per_patch;
            const int ty = rem / tiles_x;
            y0 = ty * 16;
            x0 = (rem - ty * tiles_x) * 16;
        }
    };
    // XCD-contiguous walk (tile_walk.h; grid = a multiple of 8 blocks): XCD x = block % 8 owns a contiguous eighth of the tiles, so the
    // halo pixels neighbouring tiles share are fetched into one L2 once instead of once per XCD (a round-robin walk
    // re-fetched them from HBM: 1.8x the input bytes, L2 hit rate 2 %)
    const XcdWalk walk = xcd_walk(n_tiles, blockIdx, gridDim);
    const int my_tiles = walk.my_tiles;
    if (my_tiles <= 0) return;
    auto tile_at = [&](int it) __attribute__((always_inline)) -> int { return walk.tile_at(it); };
    if (tid < 4) ((uint32_t*)zero_gran)[tid] = 0u;
    constexpr int CR = NC <= 2 ? 4 : 8;                        // floats per constant row
    if (tid < 32) {                                            // epilogue constants stay in LDS (VGPRs hold the weights)
        // channel c = fg*8+q lives in row q*4+fg: the four fg lanes groups of one read hit different banks
        float* row = cst + ((tid & 7) * 4 + (tid >> 3)) * CR;
        row[0] = p.scale[tid];
        row[1] = p.shift[tid];
        for (int c = 0; c < CR - 2; ++c) row[2 + c] = c < p.classes ? p.head_w[tid * p.classes + c] : 0.f;
    }

    // ---- this wave's weights, resident in registers
    bf16x8_t wf[kTailKSteps * 4];
    {
        const uint4* src = (const uint4*)p.wfrag + (size_t)(wave * kTailKSteps * 4) * 64 + lane;
#pragma unroll
        for (int f = 0; f < kTailKSteps * 4; ++f) wf[f] = __builtin_bit_cast(bf16x8_t, src[(size_t)f * 64]);
    }
    float hsc[NC], hsh[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { hsc[c] = c < p.classes ? p.head_scale[c] : 0.f; hsh[c] = c < p.classes ? p.head_shift[c] : 0.f; }

    // ---- LDS read offsets (per lane, tile independent): a fragment read then costs no address arithmetic (the kernel is VALU-issue
    // bound at two blocks per CU: 353 of its 858 vector instructions per tile were these).  Pixel block ni of this lane sits at
    //   src0:  hp = hp0 + ni * 32 (+ tap: (ks >> 1) * 16 + (ks & 1)); slot of granule kk * 4 + fg = (kk * 4 + fg) ^ ((hp0 + (ks & 1)) & 7)
    //   image: pixel ib0 + ni * 128 (+ tap offset of this lane's k-group; taps 9..15 carry zero weights: any finite pixel will do)
    const int hp0 = ((frow >> 3) + py) * kTailSrcRowPx + (frow & 7) + px;
    int src_t[2][2];                                           // [kk][ks & 1]
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int e = 0; e < 2; ++e) src_t[kk][e] = hp0 * 128 + (((kk * 4 + fg) ^ ((hp0 + e) & 7)) << 4);
    const int ib0 = (2 * (frow >> 3) + py) * kTailImgRowPx + 2 * (frow & 7) + px;
    int img_t[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int t = s * 8 + kk * 4 + fg;
            img_t[s][kk] = (ib0 + (t < 9 ? (t / 3) * kTailImgRowPx + (t % 3) : 0)) * 16;
        }

    auto issue_tile = [&](int tile, int buf) __attribute__((always_inline)) {
        int n, y0, x0;
        tile_origin(tile, n, y0, x0);
        char* lds_src = smem + buf * kTailBufBytes;
        char* lds_img = lds_src + kTailSrcBytes;
        // src0 halo: 10 rows x 16 px (10 needed) x 8 granules = 20 wave-instructions of 8 px
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int ii = wave + 4 * j;
            const int r = ii >> 1, c = (ii & 1) * 8 + (lane >> 3);
            const int g = (lane & 7) ^ (lane >> 3);                       // (hp & 7) == (c & 7) == lane >> 3
            const int Y = (y0 >> 1) - 1 + r, X = (x0 >> 1) - 1 + c;
            const bool ok = ((unsigned)Y < (unsigned)p.PH) & ((unsigned)X < (unsigned)p.PW) & (c < 10);
            uint32_t off = (uint32_t)((n * p.PH + Y) * p.PW + X) * 128u + (uint32_t)(g * 16 + kZeroHeaderBytes);
            off = ok ? off : 0u;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(p.src0 + off), (LDS_AS void*)(lds_src + ii * 1024), 16, 0, 0);
        }
        // image halo: 18 rows x 32 px (18 needed) x 16 B = 9 wave-instructions of 2 rows
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ii = wave + 4 * j;
            if (ii < 9) {
                const int r = ii * 2 + (lane >> 5), c = lane & 31;
                const int Y = y0 - 1 + r, X = x0 - 1 + c;
                const bool ok = ((unsigned)Y < (unsigned)H) & ((unsigned)X < (unsigned)W) & (c < 18);
                uint32_t off = (uint32_t)((n * H + Y) * W + X) * 16u + (uint32_t)kZeroHeaderBytes;
                off = ok ? off : 0u;
                __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(p.img + off), (LDS_AS void*)(lds_img + ii * 1024), 16, 0, 0);
            }
        }
    };

    issue_tile(tile_at(0), 0);
    for (int it = 0; it < my_tiles; ++it) {
        const int tile = tile_at(it);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                        // tile `it` landed; everyone is done with tile it-1
        if (it + 1 < my_tiles) issue_tile(tile_at(it + 1), (it + 1) & 1);

        const char* lds_src = smem + (it & 1) * kTailBufBytes;
        const char* lds_img = lds_src + kTailSrcBytes;
        f4_t acc[2][4];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};

        // 12 half-K-steps: 0..7 = src0 (K-step ks = tap (ty,tx) of the parity's 2x2 window, 64 channels,
        // two k-halves), 8..11 = image (two K-steps, one 16-byte granule per tap).  The pixel fragments
        // of step h+1 are requested before the MFMAs of step h (explicit register double buffer: the
        // LDS latency otherwise sits exposed in front of every group of 8 MFMAs).
        auto load_b = [&](int h, bf16x8_t (&b)[4]) __attribute__((always_inline)) {
            if (h < 8) {
                const int ks = h >> 1, kk = h & 1;
                const char* a = lds_src + src_t[kk][ks & 1];
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) b[ni] = *(const bf16x8_t*)(a + (ni * 32 + (ks >> 1) * kTailSrcRowPx + (ks & 1)) * 128);
            } else {
                const char* a = lds_img + img_t[(h - 8) >> 1][(h - 8) & 1];
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) b[ni] = *(const bf16x8_t*)(a + ni * 128 * 16);
            }
        };
        bf16x8_t b0[4], b1[4];
        load_b(0, b0);
#pragma unroll
        for (int h = 0; h < 12; h += 2) {
            load_b(h + 1, b1);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    acc[mi][ni] = mfma16<F16>(wf[h * 2 + mi], b0[ni], acc[mi][ni]);
            if (h + 2 < 12) load_b(h + 2, b0);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    acc[mi][ni] = mfma16<F16>(wf[(h + 1) * 2 + mi], b1[ni], acc[mi][ni]);
        }

        // ---- epilogue: BN/ReLU, head, softmax, argmax
        int n, ty0, tx0;
        tile_origin(tile, n, ty0, tx0);
        // (channel constants are read once per tile -- q outer, the four pixel blocks inner -- not once per pixel block)
        float lg[4][NC];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int c = 0; c < NC; ++c) lg[ni][c] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float* row = cst + (q * 4 + fg) * CR;
            const float4 c0 = *(const float4*)row;                                // scale, shift, hw0, hw1
            float2 c1 = make_float2(0.f, 0.f);
            if constexpr (NC > 2) c1 = *(const float2*)(row + 4);                 // hw2, hw3
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const float v = q < 4 ? acc[0][ni][q] : acc[1][ni][q - 4];
                const float yq = fmaxf(v * c0.x + c0.y, 0.f);
                lg[ni][0] = fmaf(yq, c0.z, lg[ni][0]);
                if constexpr (NC > 1) lg[ni][1] = fmaf(yq, c0.w, lg[ni][1]);
                if constexpr (NC > 2) {
                    lg[ni][2] = fmaf(yq, c1.x, lg[ni][2]);
                    lg[ni][3] = fmaf(yq, c1.y, lg[ni][3]);
                }
            }
        }
        // k-group reduction as a two-step butterfly: lane (frow, fg) ends up with the logits of pixel block ni = fg, pixel frow -- the
        // softmax runs once on 64 lanes instead of four times on 16 (the sums associate as before: own + fg^1, then + fg^2)
        {
            const bool o1 = fg & 1, o2 = fg & 2;
            float logit[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float k0 = (o1 ? lg[1][c] : lg[0][c]) + __shfl_xor(o1 ? lg[0][c] : lg[1][c], 16);
                const float k1 = (o1 ? lg[3][c] : lg[2][c]) + __shfl_xor(o1 ? lg[2][c] : lg[3][c], 16);
                const float a = (o2 ? k1 : k0) + __shfl_xor(o2 ? k0 : k1, 32);
                logit[c] = a * hsc[c] + hsh[c];
            }
            float mx = -3.0e38f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < p.classes) mx = fmaxf(mx, logit[c]);
            float pr[NC], sum = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) { pr[c] = c < p.classes ? expf(logit[c] - mx) : 0.f; sum += pr[c]; }
            int best = 0;
            float bestp = -1.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < p.classes) {
                    pr[c] = pr[c] / sum;
                    if (pr[c] > bestp) { bestp = pr[c]; best = c; }              // first maximum wins (np.argmax)
                }
            const int i = fg * 16 + frow;
            const int oy = 2 * (i >> 3) + py, ox = 2 * (i & 7) + px;             // inside the 16x16 tile
            lbl_tile[oy * 16 + ox] = (char)best;
            if (p.probs) {
                float* dst = p.probs + ((size_t)(n * H + ty0 + oy) * W + tx0 + ox) * p.classes;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < p.classes) dst[c] = pr[c];
            }
        }
        __syncthreads();
        if (tid < 16)
            *(uint4*)(p.labels + (size_t)(n * H + ty0 + tid) * W + tx0) = *(const uint4*)(lbl_tile + tid * 16);
    }
}

// ------------------------------------------------------------------------------------------------
// dec_tail_fused_x3ps -- the same tail in the split mode (kF16X3): three MFMAs per product (lo*hi, hi*lo, hi*hi), everything after
// the accumulators as in dec_tail_fused.  The generic kernel needs 5.1 ms per 140 patches for this layer (32 output channels:
// 24 MFMAs per 288 staged rows).
//   * tile = 16 x 16 output pixels, one block of EIGHT waves per CU: wave = (output-parity class, half of the 32 output channels);
//     its weights are hi + lo fragments in registers (80 VGPRs), two waves share a SIMD
//   * src0 halo: 10 x 10 pixels (rows of 16) x 256 B ([32 hi][32 lo][32 hi][32 lo]); pixel hp keeps granule g at slot
//     (g + 2 hp) & 15.  A 16-lane group of ds_read_b128 holds two k-groups (fg = a, a + 1) of eight pixels each whose hp are eight
//     consecutive residues: the rotation sends one k-group to the eight even slots and the other to the eight odd ones (an XOR
//     swizzle collided two-way in every group: PMC SQ_LDS_BANK_CONFLICT 86 %)
//   * image halo: 18 x 18 pixels x 16 B.  In the split mode the C8 input form keeps lo(ch 0..2) a second time in the unused
//     channel slots 4..6 of its hi plane (write_split_input), so the first granule of a pixel is [h0 h1 h2 0 | l0 l1 l2 0]: one
//     16-byte load fetches both planes, a k-group of 8 is TWO taps x 4 channel slots, and the nine image taps take 2 half-K-steps
//     (K = 36 of 64) instead of the 4 of one-tap-per-granule (K = 72 of 128): 120 instead of 144 MFMAs per wave and tile.
//     LDS row y = 32 units of 16 B; pixel x sits at unit ((x >> 1) + 12 (x & 1) + 16 - 4 (y & 3)) & 31 (brute-forced over this
//     family: 1.31 LDS cycles per conflict-free cycle on the image reads, which are 12 of 76 reads per wave and tile)
// ------------------------------------------------------------------------------------------------
constexpr int kT3SrcBytes = 10 * 16 * 256;              // 40 KB: 10 rows x 16 pixels (10 used) x 256 B
constexpr int kT3ImgBytes = 18 * 32 * 16;               // 9 KB: 18 rows x 32 units (18 used) x 16 B
constexpr int kT3BufBytes = kT3SrcBytes + kT3ImgBytes;
constexpr int kT3HalfSteps = 10;                        // 4 taps x 64 channels of src0 = 8 half-K-steps of 32, + 2 for the 9 image taps

// The two waves of every SIMD run half a tile out of phase.  With all eight waves loading, multiplying and running the epilogue at
// the same moments (round 3's first eight-wave form) the three parts simply added up (tools/probes/tail_probe.hip, 140 patches:
// tile loads alone 0.64 ms, MFMAs alone 1.23, epilogue alone 0.83; all of it 2.48).
// Here the group A = waves 0-3 (channel half 0) does   main loop(t) -> tile loads(t+1) -> BN / ReLU / partial logits(t) -> part[t & 1],
// and the group B = waves 4-7 (channel half 1) does    label store(t-2), epilogue(t-1) incl. softmax, main loop(t)
// between two consecutive block barriers.  Wave w and wave w + 4 share a SIMD (waves go to SIMDs round-robin), so while A's wave
// keeps the MFMA pipe busy B's wave issues the address arithmetic, the DMA loads and the epilogue VALU work, and the other way
// round in the second half of the step.  B finishes the pixels (A's partial logits come through LDS, written one step earlier).
// The k-group reduction is a two-step butterfly that leaves ONE pixel per lane (pixel block ni = fg), so the softmax runs once on
// 64 lanes instead of four times on 16.
constexpr int kT3PsPartBytes = 2 * 4 * 64 * 4 * 4;        // [step parity][4 pixel parities][64 lanes][<= 4 classes] partial logits
constexpr int kT3PsLdsBytes = 2 * kT3BufBytes + 2 * 256 + kTailConstBytes + kT3PsPartBytes;
static_assert(kT3PsLdsBytes <= 160 * 1024, "x3 tail: LDS");

template <int NC>
__global__ __launch_bounds__(512, 2) void dec_tail_fused_x3ps(const TailParams p)
{
    constexpr bool F16 = true;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lbl_tile = smem + 2 * kT3BufBytes;                   // [2][16][16] u8
    float* cst = (float*)(lbl_tile + 2 * 256);                 // [32 channels][CR]: scale, shift, head_w
    float* part = (float*)((char*)cst + kTailConstBytes);      // [2][4 parities][64 lanes][NC]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int par = wave & 3, mh = wave >> 2;                  // parity class; channel half = wave group (A = 0, B = 1)
    const int py = par >> 1, px = par & 1;
    const int frow = lane & 15, fg = lane >> 4;

    const int H = 2 * p.PH, W = 2 * p.PW;
    const int tiles_x = W / 16, tiles_y = H / 16;
    const int tiles_per_patch = tiles_x * tiles_y;
    // owned-region launch (TailParams::ttab): see dec_tail_fused
    const int n_tiles = p.ttab ? p.n_tab : p.n * tiles_per_patch;
    const __attribute__((address_space(4))) uint32_t* ttab = (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)p.ttab;
    auto tile_origin = [&](int tile, int& n, int& y0, int& x0) __attribute__((always_inline)) {
        if (ttab) {
            const uint32_t code = ttab[tile];
            n = (int)(code >> 22); y0 = (int)((code >> 11) & 2047u) * 2; x0 = (int)(code & 2047u) * 2;
        } else {
            n = tile / tiles_per_patch;
            const int rem = tile - n * tiles_per_patch;
            const int ty = rem / tiles_x;
            y0 = ty * 16;
            x0 = (rem - ty * tiles_x) * 16;
        }
    };
    // XCD-contiguous walk, as in the other tail kernels
    const XcdWalk walk = xcd_walk(n_tiles, blockIdx, gridDim);
    const int my_tiles = walk.my_tiles;
    if (my_tiles <= 0) return;
    auto tile_at = [&](int it) __attribute__((always_inline)) -> int { return walk.tile_at(it); };
    constexpr int CR = NC <= 2 ? 4 : 8;
    if (tid < 32) {
        float* row = cst + ((tid & 7) * 4 + (tid >> 3)) * CR;
        row[0] = p.scale[tid];
        row[1] = p.shift[tid];
        for (int c = 0; c < CR - 2; ++c) row[2 + c] = c < p.classes ? p.head_w[tid * p.classes + c] : 0.f;
    }

    // ---- this wave's weights: [plane hi|lo][half-K-step 10] fragments of row block mh (wfrag = per class [hi | lo][10][mi 2])
    constexpr int NH = kT3HalfSteps;
    bf16x8_t whi[NH], wlo[NH];
    {
        const uint4* src = (const uint4*)p.wfrag + (size_t)(par * 2 * NH * 2) * 64 + lane;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            whi[h] = __builtin_bit_cast(bf16x8_t, src[(size_t)(h * 2 + mh) * 64]);
            wlo[h] = __builtin_bit_cast(bf16x8_t, src[(size_t)(NH * 2 + h * 2 + mh) * 64]);
        }
    }
    __syncthreads();                                           // (cst written)
    float4 kc0[4];                                             // this wave's channel constants: [q] = scale, shift, hw0, hw1 of channel fg * 8 + mh * 4 + q
    float2 kc1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float* row = cst + ((mh * 4 + q) * 4 + fg) * CR;
        kc0[q] = *(const float4*)row;
        kc1[q] = make_float2(0.f, 0.f);
        if constexpr (NC > 2) kc1[q] = *(const float2*)(row + 4);
    }
    float hsc[NC], hsh[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { hsc[c] = c < p.classes ? p.head_scale[c] : 0.f; hsh[c] = c < p.classes ? p.head_shift[c] : 0.f; }

    // Tile-invariant LDS read offsets, so that a fragment read costs no address arithmetic.  Pixel block ni of this lane sits at
    //   src0:  hp = hp0 + ni * 32 (+ tap: (ks >> 1) * 16 + (ks & 1)),  slot of granule G = (G + 2 hp) & 15 = (s0 + D) & 15 with
    //          s0 = (fg + 2 hp0) & 15 per lane and D = kk * 4 + 8 * lo + 2 * (ks & 1) known at compile time (even: 8 table entries);
    //   image: row 4 ni + yb (the rotation depends on y & 3 only), tap t = 8 s2 + 2 fg + j of image half-step s2, j = 0 / 1.
    // Everything that depends on ni / ks is a multiple of 256 (2048) bytes and rides in the instruction's immediate offset.
    const int hp0 = ((frow >> 3) + py) * 16 + (frow & 7) + px;
    const int s0 = (fg + 2 * hp0) & 15;
    int src_t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) src_t[e] = hp0 * 256 + (((s0 + 2 * e) & 15) << 4);
    int img_t[3];                                              // [s2 = 0: j = 0, 1][s2 = 1: j = 0]
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int t0 = (e >> 1) * 8 + 2 * fg + (e & 1);
        const int t = t0 < 9 ? t0 : 1;                         // taps 9..15 do not exist: zero weights, any finite pixel will do
        const int yb = 2 * (frow >> 3) + py + t / 3, x = 2 * (frow & 7) + px + t % 3;
        img_t[e] = yb * 512 + ((((x >> 1) + 12 * (x & 1) + 16 - 4 * (yb & 3)) & 31) << 4);
    }

    // Halo loads (group A): wave `par` issues the src0 pieces ii = par + 4 j (j = 0..9: halo row j, halo columns 4 par .. 4 par + 3) and
    // the image pieces q = par + 4 j (< 9).  `buffer_load ... lds` with a per-tile resource (this patch's image, one pixel of
    // bias so that the lane part is never negative): the lane offset of a src0 piece does not depend on j or on the tile, the row
    // rides in the scalar offset, and anything outside the image sets bit 31 of the lane offset (past num_records: the hardware
    // writes zeros).  ~3 vector instructions per piece instead of the ~20 of per-lane global addresses.
    const int c_src = par * 4 + (lane >> 4);                   // halo column of this lane's src0 pixel
    const uint32_t voff_src = (uint32_t)(c_src * 256 + ((((lane & 15) - 2 * c_src) & 15) << 4));      // slot s of pixel hp holds granule (s - 2 hp) & 15
    // image piece q: lane l fills unit l & 31 of halo row 2 q + (l >> 5); (2 q) & 3 = 2 (par & 1) for every piece of this wave
    const int img_v = ((lane & 31) - (16 - 4 * ((2 * par + (lane >> 5)) & 3))) & 31;
    const bool img_xok = img_v < 9 || (img_v >= 12 && img_v < 21);
    const int img_x = img_v < 9 ? 2 * img_v : 2 * (img_v - 12) + 1;
    const uint32_t voff_img = (uint32_t)(((lane >> 5) * W + img_x) * 32);
    const uint32_t src_img_bytes = (uint32_t)(p.PH * p.PW) * 256u, img_img_bytes = (uint32_t)(H * W) * 32u;
    auto issue_src = [&](int n, int y0, int x0, int buf) __attribute__((always_inline)) {           // group A: ten pieces per wave
        char* lds_src = smem + buf * kT3BufBytes;
        const char* sbase = p.src0 + kZeroHeaderBytes - 256 + (size_t)n * src_img_bytes;
        const uint32_t vs = ((unsigned)((x0 >> 1) - 1 + c_src) < (unsigned)p.PW && c_src < 10) ? voff_src : 0x80000000u;
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const int Y = (y0 >> 1) - 1 + j;
            const bool yok = (unsigned)Y < (unsigned)p.PH;
            const uint32_t soff = yok ? (uint32_t)(Y * p.PW + (x0 >> 1)) * 256u : 0u;
            buffer_load_lds16(sbase, src_img_bytes + 256u, (LDS_AS void*)(lds_src + (par + 4 * j) * 1024), yok ? vs : 0x80000000u, soff);
        }
    };
    auto issue_img = [&](int n, int y0, int x0, int buf) __attribute__((always_inline)) {           // group B: two or three pieces per wave
        char* lds_img = smem + buf * kT3BufBytes + kT3SrcBytes;
        // image: piece q = par + 4 j (< 9) = halo rows 2 q, 2 q + 1 (32 units each); one row + one pixel of bias
        const char* ibase = p.img + kZeroHeaderBytes + (size_t)n * img_img_bytes - (size_t)(W + 1) * 32;
        const uint32_t vi = (img_xok && (unsigned)(x0 - 1 + img_x) < (unsigned)W) ? voff_img : 0x80000000u;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = par + 4 * j;
            if (q < 9) {
                const bool yok = (unsigned)(y0 - 1 + 2 * q + (lane >> 5)) < (unsigned)H;
                buffer_load_lds16(ibase, img_img_bytes + (uint32_t)(W + 1) * 32u, (LDS_AS void*)(lds_img + q * 1024), yok ? vi : 0x80000000u,
                                  (uint32_t)((y0 + 2 * q) * W + x0) * 32u);
            }
        }
    };

    f4_t acc[4];
    auto main_loop = [&](int it) __attribute__((always_inline)) {
        const char* lds_src = smem + (it & 1) * kT3BufBytes;
        const char* lds_img = lds_src + kT3SrcBytes;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[ni] = (f4_t){0.f, 0.f, 0.f, 0.f};
        const char* sb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) sb[e] = lds_src + src_t[e];
        auto load_b = [&](int h, bf16x8_t (&bh)[4], bf16x8_t (&bl)[4]) __attribute__((always_inline)) {
            if (h < 8) {
                const int ks = h >> 1, kk = h & 1;
                const int dh = (kk * 8 + 2 * (ks & 1)) & 15, dl = (kk * 8 + 4 + 2 * (ks & 1)) & 15;      // src0 pixel: [32 hi][32 lo][32 hi][32 lo]
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const int k = (ni * 32 + (ks >> 1) * 16 + (ks & 1)) * 256;      // immediate offset
                    bh[ni] = *(const bf16x8_t*)(sb[dh >> 1] + k);
                    bl[ni] = *(const bf16x8_t*)(sb[dl >> 1] + k);
                }
            } else {
                // image pixel = [h0 h1 h2 0 | l0 l1 l2 0]: the k-group is two taps; half-step 9 has tap 8 only (its second tap
                // multiplies zero weights: the first one's registers do)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const uint4 r0 = *(const uint4*)(lds_img + img_t[(h - 8) * 2] + ni * 2048);
                    const uint4 r1 = h == 8 ? *(const uint4*)(lds_img + img_t[1] + ni * 2048) : r0;
                    bh[ni] = __builtin_bit_cast(bf16x8_t, make_uint4(r0.x, r0.y, r1.x, r1.y));
                    bl[ni] = __builtin_bit_cast(bf16x8_t, make_uint4(r0.z, r0.w, r1.z, r1.w));
                }
            }
        };
        auto mac = [&](int h, const bf16x8_t (&bh)[4], const bf16x8_t (&bl)[4]) __attribute__((always_inline)) {
            // three sweeps over the four accumulators (small terms first)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[ni] = mfma16<F16>(wlo[h], bh[ni], acc[ni]);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[ni] = mfma16<F16>(whi[h], bl[ni], acc[ni]);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[ni] = mfma16<F16>(whi[h], bh[ni], acc[ni]);
        };
        bf16x8_t b0h[4], b0l[4], b1h[4], b1l[4];
        load_b(0, b0h, b0l);
#pragma unroll
        for (int h = 0; h < NH; h += 2) {
            load_b(h + 1, b1h, b1l);
            mac(h, b0h, b0l);
            if (h + 2 < NH) load_b(h + 2, b0h, b0l);
            mac(h + 1, b1h, b1l);
        }
    };
    // BN / ReLU / head on this wave's 16 channels, then the k-group butterfly: lane (frow, fg) ends up with the partial logits of
    // pixel block ni = fg, pixel frow
    auto partial_logits = [&](float (&tot)[NC]) __attribute__((always_inline)) {
        float lg[4][NC];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int c = 0; c < NC; ++c) lg[ni][c] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 c0 = kc0[q];                                             // scale, shift, hw0, hw1
            const float2 c1 = kc1[q];                                             // hw2, hw3
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const float yq = fmaxf(acc[ni][q] * c0.x + c0.y, 0.f);
                lg[ni][0] = fmaf(yq, c0.z, lg[ni][0]);
                if constexpr (NC > 1) lg[ni][1] = fmaf(yq, c0.w, lg[ni][1]);
                if constexpr (NC > 2) {
                    lg[ni][2] = fmaf(yq, c1.x, lg[ni][2]);
                    lg[ni][3] = fmaf(yq, c1.y, lg[ni][3]);
                }
            }
        }
        const bool o1 = fg & 1, o2 = fg & 2;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            // step 1 (partner fg ^ 1): keep the pixel blocks of this lane's parity, hand over the other two
            const float k0 = (o1 ? lg[1][c] : lg[0][c]) + __shfl_xor(o1 ? lg[0][c] : lg[1][c], 16);      // block 0 + (fg & 1)
            const float k1 = (o1 ? lg[3][c] : lg[2][c]) + __shfl_xor(o1 ? lg[2][c] : lg[3][c], 16);      // block 2 + (fg & 1)
            // step 2 (partner fg ^ 2)
            tot[c] = (o2 ? k1 : k0) + __shfl_xor(o2 ? k0 : k1, 32);
        }
    };
    // group B: finish tile `it` (its accumulators are still in this wave's registers; A's half came through part[it & 1])
    auto finish = [&](int it) __attribute__((always_inline)) {
        float tot[NC];
        partial_logits(tot);
        const float* pa = part + (((it & 1) * 4 + par) * 64 + lane) * NC;
        float logit[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) logit[c] = (pa[c] + tot[c]) * hsc[c] + hsh[c];
        float mx = -3.0e38f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < p.classes) mx = fmaxf(mx, logit[c]);
        float pr[NC], sum = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { pr[c] = c < p.classes ? expf(logit[c] - mx) : 0.f; sum += pr[c]; }
        int best = 0;
        float bestp = -1.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < p.classes) {
                pr[c] = pr[c] / sum;
                if (pr[c] > bestp) { bestp = pr[c]; best = c; }
            }
        const int i = fg * 16 + frow;
        const int oy = 2 * (i >> 3) + py, ox = 2 * (i & 7) + px;
        lbl_tile[(it & 1) * 256 + oy * 16 + ox] = (char)best;
        if (p.probs) {
            int n, ty0, tx0;
            tile_origin(tile_at(it), n, ty0, tx0);
            float* dst = p.probs + ((size_t)(n * H + ty0 + oy) * W + tx0 + ox) * p.classes;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < p.classes) dst[c] = pr[c];
        }
    };
    auto store_labels = [&](int it) __attribute__((always_inline)) {       // (wave 4, after the barrier that follows finish(it))
        if (wave == 4 && lane < 16) {
            int n, ty0, tx0;
            tile_origin(tile_at(it), n, ty0, tx0);
            *(uint4*)(p.labels + (size_t)(n * H + ty0 + lane) * W + tx0) = *(const uint4*)(lbl_tile + (it & 1) * 256 + lane * 16);
        }
    };

    if (mh == 0) {
        int n, y0, x0;
        tile_origin(tile_at(0), n, y0, x0);
        issue_src(n, y0, x0, 0); issue_img(n, y0, x0, 0);
    }
    for (int it = 0; it < my_tiles; ++it) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (mh == 1) {
            if (it >= 2) store_labels(it - 2);
            if (it >= 1) finish(it - 1);
        }
        main_loop(it);
        if (mh == 0) {
            // all of the next tile's halo pieces (before the epilogue: more time to land).  Moving the image pieces to group B --
            // before or after its epilogue -- made B the longer group: a piece costs its wave 200-400 cycles there
            if (it + 1 < my_tiles) {
                int n, y0, x0;
                tile_origin(tile_at(it + 1), n, y0, x0);
                issue_src(n, y0, x0, (it + 1) & 1); issue_img(n, y0, x0, (it + 1) & 1);
            }
            float tot[NC];
            partial_logits(tot);
            float* pa = part + (((it & 1) * 4 + par) * 64 + lane) * NC;
#pragma unroll
            for (int c = 0; c < NC; ++c) pa[c] = tot[c];
        }
    }
    __syncthreads();
    if (mh == 1) {
        if (my_tiles >= 2) store_labels(my_tiles - 2);
        finish(my_tiles - 1);
    }
    __syncthreads();
    if (mh == 1) store_labels(my_tiles - 1);
}

hipError_t launch_tail(const TailParams& p, int precision, int num_cus, hipStream_t s, LaunchRec* rec)
{
    const int n_tiles = p.ttab ? p.n_tab : p.n * (p.PH / 8) * (p.PW / 8);
    if (n_tiles <= 0) return hipSuccess;
    const int grid = xcd_grid(n_tiles, 2 * num_cus);
    launch_rec(rec, SBBSEG_LAUNCH_TAIL, 16 * 16, 32, 1, n_tiles, grid, 1, p.ttab != nullptr);
    auto go = [&](auto kern) -> hipError_t {
        static bool attr_done[64] = {};                         // (one per kernel: the lambda is instantiated per `kern`)
        hipError_t e = dynamic_lds_once((const void*)kern, kTailLdsBytes, attr_done);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), kTailLdsBytes, s, p);
        return hipSuccess;
    };
    hipError_t e;
    if (precision == kF16X3) {
        const int grid3 = xcd_grid(n_tiles, num_cus);
        if (rec) rec->grid = grid3;
        auto gops = [&](auto kern) -> hipError_t {
            static bool attr_done[64] = {};
            hipError_t e8 = dynamic_lds_once((const void*)kern, kT3PsLdsBytes, attr_done);
            if (e8 != hipSuccess) return e8;
            hipLaunchKernelGGL(kern, dim3(grid3), dim3(512), kT3PsLdsBytes, s, p);
            return hipSuccess;
        };
        e = p.classes <= 2 ? gops(dec_tail_fused_x3ps<2>) : gops(dec_tail_fused_x3ps<4>);
        if (e != hipSuccess) return e;
        return hipGetLastError();
    }
    if (precision == kF16) e = p.classes <= 2 ? go(dec_tail_fused<true, 2>) : go(dec_tail_fused<true, 4>);
    else e = p.classes <= 2 ? go(dec_tail_fused<false, 2>) : go(dec_tail_fused<false, 4>);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace sbbseg
