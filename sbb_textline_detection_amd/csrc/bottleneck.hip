// bottleneck.hip -- a whole stage-2 ResNet bottleneck block per launch in the 16-bit modes: bottleneck_fused and its two-group form
// bottleneck_fused_pq.  (The split mode's block is block_x3.hip.)
#include "tile_walk.h"

namespace sbbseg {

// ------------------------------------------------------------------------------------------------
// bottleneck_fused -- one whole ResNet stage-2 bottleneck block per launch (three of them at 111x111 in the sbb nets):
//
//   a = ReLU(BN(conv1x1(x, CIN -> 64)))              phase A, on the 10 x 18 halo of an 8 x 16 output tile
//   b = ReLU(BN(conv3x3(a, 64 -> 64)))               phase B, from the halo tile in LDS (as conv3x3_c64_direct)
//   y = ReLU(BN(conv1x1(b, 64 -> 256)) + x)          phase C, identity block (CIN = 256)
//   y = ReLU(BN(conv1x1([b, x], 128 -> 256)))        phase C, projection block (CIN = 64; the planner has folded the
//                                                    shortcut conv into one contraction over [b, x])
//
// Run as three launches these layers are HBM-bound and move the 256-channel tensor four times per block (read for
// the first 1x1, residual read + write in the last) plus the 64-channel tensors four times; fused, x is read once
// (halo overlap from L2) and y written once.  What a CU has to do per tile is small next to that traffic (~300 MFMAs
// per wave), so the kernel is built for memory-level parallelism, not for MFMA rate: ONE block of four waves per CU
// (up to 512 VGPRs per lane), the x fragments of the NEXT tile are requested into registers before the current tile's
// phases run, and the fragments of the inner pixels double as the residual of phase C (the MFMA B-operand layout --
// pixel = lane & 15, 8 channels per lane -- is exactly the layout of the epilogue's 16-byte channel groups).
//   * halo pixel order: n-tiles 0-7 = the 8 inner rows (16 pixels each), n-tiles 8-11 = the 52 border pixels (+12
//     dummies).  Wave w owns inner rows 2w, 2w+1 and border tile 8+w in phases A and C, and the 16 output channels
//     of MFMA row block w in phase B (its 9 x 2 weight fragments live in 72 VGPRs).
//   * W1 and W3 stay in LDS for the whole kernel (A-fragment order, linear 16-byte reads); a (halo, 192 rows x 128 B)
//     and b (128 rows x 128 B) are XOR-swizzled rows; halo pixels outside the image are ZERO (the 3x3 conv pads a, not x).
//   * tiles are walked so that every XCD owns one contiguous range of them: vertical halo neighbours share an L2.
//   * DUMP (conv variant bit 26, the step check of tests/test_gpu_steps_blocks.py; never a product launch): what phase A packs for the
//     lane's two inner pixels and what phase B packs also go to the plan tensors of a and b (BlockParams::dump_a / dump_b, the [n][H][W][64]
//     layout the three-conv route writes), under the in-image predicate of phase C's store.  The halo copies of a are not stored: b's
//     reference is built from the dumped a, so a halo that disagrees with its neighbour's inner pixels puts b over its bound.
//     bottleneck_fused_pq's P waves have no register for a second store of a group next to its LDS store (the identity block's product
//     instantiation uses 253 of 256), so its DUMP form stores the same groups where they are read back: a from phase B's centre-tap read
//     of each inner pixel, b from LDS behind B2 in the 16-byte groups the Q waves read for phase C; it also requests the next tile's x
//     behind phase B instead of behind phase A.  No DUMP instantiation may spill (tests/test_build_resources.py).
// ------------------------------------------------------------------------------------------------
constexpr int kBlkHaloW = 18;
constexpr int kBlkABytes = 192 * 128;                           // a: 180 halo rows (+12 dummy rows)
constexpr int kBlkBBytes = 128 * 128;                           // b: 8 x 16 pixels
constexpr int kBlkCstBytes = (4 * 64 + 2 * 256) * 4;            // s1, b1, s2, b2 [64]; s3, b3 [256]
constexpr int block_lds_bytes(int cin, bool proj) { return (cin / 32) * 4 * 1024 + (proj ? 4 : 2) * 16 * 1024 + kBlkABytes + kBlkBBytes + kBlkCstBytes; }

// DUMP: the start of the 16 pixels (x0 .. x0 + 15) of row oy of patch n in the plan tensor of a or b, [n][H][W][64] 16-bit = 128 bytes a pixel.
// Wave-uniform, so it costs scalar registers only; a lane adds dump_lane = frow * 128 + fg * 16 (its pixel and 8-channel group) and the
// uniform byte offset of the 32-channel group it is packing.
__device__ __attribute__((always_inline)) inline char* dump_row(void* base, int n, int H, int W, int oy, int x0)
{
    return (char*)base + (((size_t)n * H + oy) * W + x0) * 128;
}

template <bool F16, int CIN, bool PROJ, bool DUMP>
__global__ __launch_bounds__(256, 1) void bottleneck_fused(const BlockParams p)
{
    static_assert((CIN == 256 && !PROJ) || (CIN == 64 && PROJ), "identity blocks read 256 channels, the projection block 64");
    constexpr int KA = CIN / 32;                                // K-steps (32 channels) of phase A
    constexpr int KC = PROJ ? 4 : 2;                            // K-steps of phase C
    constexpr int PIXB = CIN * 2;                               // bytes per stored x pixel
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_w1 = smem;
    char* lds_w3 = lds_w1 + KA * 4 * 1024;
    char* lds_a = lds_w3 + KC * 16 * 1024;
    char* lds_b = lds_a + kBlkABytes;
    float* cst = (float*)(lds_b + kBlkBBytes);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fg = lane >> 4;
    const int dump_lane = frow * 128 + fg * 16;                 // (DUMP only)
    const int tiles_x = (p.W + 15) / 16, tiles_y = (p.H + 7) / 8;
    const int tiles_per_patch = tiles_x * tiles_y;
    const int n_tiles = p.n * tiles_per_patch;
    // XCD-contiguous walk (tile_walk.h): XCD x = block % 8 owns a contiguous eighth of the tiles
    const XcdWalk walk = xcd_walk(n_tiles, blockIdx, gridDim);
    const int my_tiles = walk.my_tiles;
    if (my_tiles <= 0) return;

    // ---- one-time: weights and constants to LDS, this wave's 3x3 fragments to registers
    for (int i = tid; i < KA * 4 * 64; i += 256) ((uint4*)lds_w1)[i] = ((const uint4*)p.w1)[i];
    for (int i = tid; i < KC * 16 * 64; i += 256) ((uint4*)lds_w3)[i] = ((const uint4*)p.w3)[i];
    if (tid < 64) {
        cst[tid] = p.s1[tid]; cst[64 + tid] = p.b1[tid]; cst[128 + tid] = p.s2[tid]; cst[192 + tid] = p.b2[tid];
    }
    cst[256 + tid] = p.s3[tid]; cst[512 + tid] = p.b3[tid];
    bf16x8_t wf[9][2];                                          // [tap][kk], MFMA row block `wave`
    {
        const uint4* src = (const uint4*)p.w2 + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) wf[t][kk] = __builtin_bit_cast(bf16x8_t, src[(size_t)((t * 2 + kk) * 4 + wave) * 64]);
    }

    // ---- this lane's three halo pixels (fixed per kernel): (hy, hx) and the LDS row hr = hy * 18 + hx
    int hy[3], hx[3], hr[3];
#pragma unroll
    for (int j = 0; j < 2; ++j) { hy[j] = 2 * wave + j + 1; hx[j] = frow + 1; hr[j] = hy[j] * kBlkHaloW + hx[j]; }
    {
        const int bi = wave * 16 + frow;                       // border pixel index
        int y, x;
        if (bi < 18) { y = 0; x = bi; }
        else if (bi < 36) { y = 9; x = bi - 18; }
        else if (bi < 44) { y = 1 + (bi - 36); x = 0; }
        else if (bi < 52) { y = 1 + (bi - 44); x = 17; }
        else { y = 10; x = bi - 52; }                           // dummies: rows 180..191, never inside the image
        hy[2] = y; hx[2] = x; hr[2] = y * kBlkHaloW + x;
    }

    bool inimg[3];
    uint32_t xoff[3];
    auto locate = [&](int tile, bool (&in)[3], uint32_t (&off)[3]) __attribute__((always_inline)) {
        const int n = tile / tiles_per_patch;
        const int rem = tile - n * tiles_per_patch;
        const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int Y = ty * 8 - 1 + hy[j], X = tx * 16 - 1 + hx[j];
            in[j] = ((unsigned)Y < (unsigned)p.H) & ((unsigned)X < (unsigned)p.W) & (hy[j] < 10);
            // (pixels outside the image read the start of the buffer: finite or not, their column is replaced by zeros)
            off[j] = in[j] ? (uint32_t)((n * p.H + Y) * p.W + X) * (uint32_t)PIXB + (uint32_t)(kZeroHeaderBytes + fg * 16) : 0u;
        }
    };
    bf16x8_t xcur[3][KA], xnext[3][KA];
    auto fetch = [&](const uint32_t (&off)[3], bf16x8_t (&dst)[3][KA]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int kk = 0; kk < KA; ++kk) dst[j][kk] = *(const bf16x8_t*)(p.x + off[j] + kk * 64);
    };

    auto tile_at = [&](int it) __attribute__((always_inline)) -> int { return walk.tile_at(it); };
    locate(tile_at(0), inimg, xoff);
    fetch(xoff, xcur);
    __syncthreads();                                            // weights / constants visible

    for (int it = 0; it < my_tiles; ++it) {
        const int tile = tile_at(it);
        bool in_next[3];
        uint32_t off_next[3];
        if (it + 1 < my_tiles) {                                // the next tile's x: in flight across all three phases
            locate(tile_at(it + 1), in_next, off_next);
            fetch(off_next, xnext);
        }
        int dn = 0, dty = 0, dtx = 0;                           // DUMP: patch and tile origin of this tile
        if constexpr (DUMP) {
            dn = tile / tiles_per_patch;
            const int rem = tile - dn * tiles_per_patch;
            dty = rem / tiles_x; dtx = rem - dty * tiles_x;
        }

        // ---- phase A: a[halo pixel][64] = ReLU(s1 * (W1 . x) + b1), zero outside the image
        {
            f4_t acc[4][3];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[mi][j] = (f4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KA; ++kk) {
                bf16x8_t wa[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) wa[mi] = *(const bf16x8_t*)(lds_w1 + (kk * 4 + mi) * 1024 + lane * 16);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[mi][j] = mfma16<F16>(wa[mi], xcur[j][kk], acc[mi][j]);
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int c0 = s2 * 32 + fg * 8;
                float sc[8], sh[8];
                *(float4*)&sc[0] = *(const float4*)(cst + c0); *(float4*)&sc[4] = *(const float4*)(cst + c0 + 4);
                *(float4*)&sh[0] = *(const float4*)(cst + 64 + c0); *(float4*)&sh[4] = *(const float4*)(cst + 64 + c0 + 4);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    float y[8];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        y[q] = fmaxf(acc[2 * s2][j][q] * sc[q] + sh[q], 0.f);
                        y[4 + q] = fmaxf(acc[2 * s2 + 1][j][q] * sc[4 + q] + sh[4 + q], 0.f);
                    }
                    uint4 r;
                    r.x = pack2<F16>(y[0], y[1]); r.y = pack2<F16>(y[2], y[3]); r.z = pack2<F16>(y[4], y[5]); r.w = pack2<F16>(y[6], y[7]);
                    if (!inimg[j]) r = make_uint4(0u, 0u, 0u, 0u);
                    *(uint4*)(lds_a + hr[j] * 128 + (((s2 * 4 + fg) ^ (hr[j] & 7)) << 4)) = r;
                    if constexpr (DUMP) {
                        if (j < 2) {                            // the lane's inner pixels: rows 2w, 2w+1 of the tile, column frow
                            const int oy = dty * 8 + 2 * wave + j;
                            if (oy < p.H && dtx * 16 + frow < p.W)
                                *(uint4*)(dump_row(p.dump_a, dn, p.H, p.W, oy, dtx * 16) + s2 * 64 + dump_lane) = r;
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---- phase B: b[pixel][16 channels of row block `wave`] = ReLU(s2 * conv3x3(a) + b2)
        {
            const int sB = wave >> 1, half = wave & 1;
            const int cB = sB * 32 + fg * 8 + half * 4;
            const float4 sc = *(const float4*)(cst + 128 + cB), sh = *(const float4*)(cst + 192 + cB);
#pragma unroll
            for (int g4 = 0; g4 < 2; ++g4) {                   // four output rows at a time: independent accumulator chains
                f4_t acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = (f4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = (g4 * 4 + i + t / 3) * kBlkHaloW + frow + t % 3;
                            const bf16x8_t bq = *(const bf16x8_t*)(lds_a + row * 128 + (((kk * 4 + fg) ^ (row & 7)) << 4));
                            acc[i] = mfma16<F16>(wf[t][kk], bq, acc[i]);
                        }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = (g4 * 4 + i) * 16 + frow;
                    uint2 r;
                    r.x = pack2<F16>(fmaxf(acc[i][0] * sc.x + sh.x, 0.f), fmaxf(acc[i][1] * sc.y + sh.y, 0.f));
                    r.y = pack2<F16>(fmaxf(acc[i][2] * sc.z + sh.z, 0.f), fmaxf(acc[i][3] * sc.w + sh.w, 0.f));
                    *(uint2*)(lds_b + row * 128 + (((sB * 4 + fg) ^ (row & 7)) << 4) + half * 8) = r;
                    if constexpr (DUMP) {
                        const int oy = dty * 8 + g4 * 4 + i;
                        if (oy < p.H && dtx * 16 + frow < p.W)
                            *(uint2*)(dump_row(p.dump_b, dn, p.H, p.W, oy, dtx * 16) + sB * 64 + half * 8 + dump_lane) = r;
                    }
                }
            }
        }
        __syncthreads();

        // ---- phase C: y[inner rows 2w, 2w+1][256] = ReLU(s3 * (W3 . [b, x?]) + b3 (+ x)), 32 channels at a time
        {
            const int n = tile / tiles_per_patch;
            const int rem = tile - n * tiles_per_patch;
            const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
            const int ox = tx * 16 + frow;
            bf16x8_t bf[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int row = (2 * wave + j) * 16 + frow;
                    bf[j][kk] = *(const bf16x8_t*)(lds_b + row * 128 + (((kk * 4 + fg) ^ (row & 7)) << 4));
                }
#pragma unroll
            for (int s3 = 0; s3 < 8; ++s3) {
                f4_t acc[2][2];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[m][j] = (f4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        const bf16x8_t wa = *(const bf16x8_t*)(lds_w3 + (kk * 16 + 2 * s3 + m) * 1024 + lane * 16);
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            bf16x8_t bq;
                            if constexpr (PROJ) bq = kk < 2 ? bf[j][kk & 1] : xcur[j][kk & 1];
                            else bq = bf[j][kk & 1];
                            acc[m][j] = mfma16<F16>(wa, bq, acc[m][j]);
                        }
                    }
                const int c0 = s3 * 32 + fg * 8;
                float sc[8], sh[8];
                *(float4*)&sc[0] = *(const float4*)(cst + 256 + c0); *(float4*)&sc[4] = *(const float4*)(cst + 256 + c0 + 4);
                *(float4*)&sh[0] = *(const float4*)(cst + 512 + c0); *(float4*)&sh[4] = *(const float4*)(cst + 512 + c0 + 4);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float y[8];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        y[q] = acc[0][j][q] * sc[q] + sh[q];
                        y[4 + q] = acc[1][j][q] * sc[4 + q] + sh[4 + q];
                    }
                    if constexpr (!PROJ) {                      // the residual: this lane's x fragment of K-step s3 = channels c0 .. c0+7
                        const uint4 rv = __builtin_bit_cast(uint4, xcur[j][s3 % KA]);
                        y[0] += unpack_lo<F16>(rv.x); y[1] += unpack_hi<F16>(rv.x); y[2] += unpack_lo<F16>(rv.y); y[3] += unpack_hi<F16>(rv.y);
                        y[4] += unpack_lo<F16>(rv.z); y[5] += unpack_hi<F16>(rv.z); y[6] += unpack_lo<F16>(rv.w); y[7] += unpack_hi<F16>(rv.w);
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) y[q] = fmaxf(y[q], 0.f);
                    uint4 r;
                    r.x = pack2<F16>(y[0], y[1]); r.y = pack2<F16>(y[2], y[3]); r.z = pack2<F16>(y[4], y[5]); r.w = pack2<F16>(y[6], y[7]);
                    const int oy = ty * 8 + 2 * wave + j;
                    if (oy < p.H && ox < p.W)
                        *(uint4*)((uint16_t*)p.out + (((size_t)n * p.H + oy) * p.W + ox) * 256 + c0) = r;
                }
            }
        }

        if (it + 1 < my_tiles) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                inimg[j] = in_next[j];
#pragma unroll
                for (int kk = 0; kk < KA; ++kk) xcur[j][kk] = xnext[j][kk];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// bottleneck_fused_pq -- the same block with its phases split over two groups of four waves (one of each per SIMD):
//   P ("producer") waves run phases A and B of tile i:  x halo -> a (LDS) -> b (LDS, double buffered)
//   Q ("consumer") waves run phase C of tile i-1:        b, x -> y
// In the one-group kernel a wave's MFMA, VALU (epilogues) and LDS work serialise (one wave per SIMD); here the MFMA / LDS-
// heavy phases of one tile overlap the VALU / store-heavy phase of the previous one.  Two block-wide barriers per iteration:
// after phase A (a visible to the P waves; Q has done the first half of its channel groups) and at the end (b[i & 1]
// complete, b[(i-1) & 1] and a free).  P requests the next tile's x right after phase A into the registers that phase just
// freed; Q reads its inner-pixel x (the residual; the projection block's second operand) itself, one tile ahead.
// ------------------------------------------------------------------------------------------------
constexpr int block_pq_lds_bytes(int cin, bool proj) { return block_lds_bytes(cin, proj) + kBlkBBytes; }

template <bool F16, int CIN, bool PROJ, bool DUMP>
__global__ __launch_bounds__(512, 1) void bottleneck_fused_pq(const BlockParams p)
{
    static_assert((CIN == 256 && !PROJ) || (CIN == 64 && PROJ), "identity blocks read 256 channels, the projection block 64");
    constexpr int KA = CIN / 32;
    constexpr int KC = PROJ ? 4 : 2;
    constexpr int PIXB = CIN * 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_w1 = smem;
    char* lds_w3 = lds_w1 + KA * 4 * 1024;
    char* lds_a = lds_w3 + KC * 16 * 1024;
    char* lds_b = lds_a + kBlkABytes;                           // two buffers of kBlkBBytes
    float* cst = (float*)(lds_b + 2 * kBlkBBytes);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_q = wave8 >= 4;
    const int wave = wave8 & 3;                                 // index inside the group
    const int frow = lane & 15, fg = lane >> 4;
    const int tiles_x = (p.W + 15) / 16, tiles_y = (p.H + 7) / 8;
    const int tiles_per_patch = tiles_x * tiles_y;
    const int n_tiles = p.n * tiles_per_patch;
    const XcdWalk walk = xcd_walk(n_tiles, blockIdx, gridDim);
    const int my_tiles = walk.my_tiles;
    if (my_tiles <= 0) return;
    auto tile_at = [&](int it) __attribute__((always_inline)) -> int { return walk.tile_at(it); };

    for (int i = tid; i < KA * 4 * 64; i += 512) ((uint4*)lds_w1)[i] = ((const uint4*)p.w1)[i];
    for (int i = tid; i < KC * 16 * 64; i += 512) ((uint4*)lds_w3)[i] = ((const uint4*)p.w3)[i];
    if (tid < 64) {
        cst[tid] = p.s1[tid]; cst[64 + tid] = p.b1[tid]; cst[128 + tid] = p.s2[tid]; cst[192 + tid] = p.b2[tid];
    }
    if (tid < 256) { cst[256 + tid] = p.s3[tid]; cst[512 + tid] = p.b3[tid]; }

    if (!is_q) {
        // =============================================== P: phases A and B ===============================================
        bf16x8_t wf[9][2];
        {
            const uint4* src = (const uint4*)p.w2 + lane;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) wf[t][kk] = __builtin_bit_cast(bf16x8_t, src[(size_t)((t * 2 + kk) * 4 + wave) * 64]);
        }
        int hy[3], hx[3], hr[3];
#pragma unroll
        for (int j = 0; j < 2; ++j) { hy[j] = 2 * wave + j + 1; hx[j] = frow + 1; hr[j] = hy[j] * kBlkHaloW + hx[j]; }
        {
            const int bi = wave * 16 + frow;
            int y, x;
            if (bi < 18) { y = 0; x = bi; }
            else if (bi < 36) { y = 9; x = bi - 18; }
            else if (bi < 44) { y = 1 + (bi - 36); x = 0; }
            else if (bi < 52) { y = 1 + (bi - 44); x = 17; }
            else { y = 10; x = bi - 52; }
            hy[2] = y; hx[2] = x; hr[2] = y * kBlkHaloW + x;
        }
        bool inimg[3];
        uint32_t xoff[3];
        auto locate = [&](int tile) __attribute__((always_inline)) {
            const int n = tile / tiles_per_patch;
            const int rem = tile - n * tiles_per_patch;
            const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int Y = ty * 8 - 1 + hy[j], X = tx * 16 - 1 + hx[j];
                inimg[j] = ((unsigned)Y < (unsigned)p.H) & ((unsigned)X < (unsigned)p.W) & (hy[j] < 10);
                xoff[j] = inimg[j] ? (uint32_t)((n * p.H + Y) * p.W + X) * (uint32_t)PIXB + (uint32_t)(kZeroHeaderBytes + fg * 16) : 0u;
            }
        };
        bf16x8_t xf[3][KA];
        auto fetch = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int kk = 0; kk < KA; ++kk) xf[j][kk] = *(const bf16x8_t*)(p.x + xoff[j] + kk * 64);
        };
        locate(tile_at(0));
        fetch();
        __syncthreads();                                        // weights / constants visible (all eight waves)

        for (int it = 0; it <= my_tiles; ++it) {
            bool in_cur[3] = {inimg[0], inimg[1], inimg[2]};
            if constexpr (DUMP) {
                // b of tile it - 1, complete since B2: the 16-byte groups of this wave's rows 2w, 2w+1 exactly as the Q waves read them for phase C
                // (a second store of phase B's 8-byte groups costs registers that wave does not have, above; here the accumulators are dead)
                if (it >= 1) {
                    const int tile = tile_at(it - 1);
                    const int pn = tile / tiles_per_patch;
                    const int rem = tile - pn * tiles_per_patch;
                    const int pty = rem / tiles_x, ptx = rem - pty * tiles_x;
                    const char* pb = lds_b + ((it - 1) & 1) * kBlkBBytes;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int oy = pty * 8 + 2 * wave + j;
                        if (oy < p.H && ptx * 16 + frow < p.W) {
                            int lane_now = lane;
                            asm volatile("" : "+v"(lane_now));  // (opaque copy: the addresses below are worked out here per tile, not held in registers across the phases)
                            const int row = (2 * wave + j) * 16 + (lane_now & 15);
#pragma unroll
                            for (int kk = 0; kk < 2; ++kk)
                                *(uint4*)(dump_row(p.dump_b, pn, p.H, p.W, oy, ptx * 16) + kk * 64 + ((lane_now & 15) * 128 + (lane_now >> 4) * 16)) =
                                    *(const uint4*)(pb + row * 128 + (((kk * 4 + (lane_now >> 4)) ^ (row & 7)) << 4));
                        }
                    }
                }
            }
            if (it < my_tiles) {
                // ---- phase A of tile `it`, 32 output channels (two MFMA row blocks) at a time: 24 accumulator registers
                // instead of 48 -- with 96 registers of x fragments and 72 of 3x3 weights this wave has no more to give
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    f4_t acc[2][3];
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int j = 0; j < 3; ++j) acc[m][j] = (f4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kk = 0; kk < KA; ++kk) {
                        bf16x8_t wa[2];
#pragma unroll
                        for (int m = 0; m < 2; ++m) wa[m] = *(const bf16x8_t*)(lds_w1 + (kk * 4 + 2 * s2 + m) * 1024 + lane * 16);
#pragma unroll
                        for (int m = 0; m < 2; ++m)
#pragma unroll
                            for (int j = 0; j < 3; ++j) acc[m][j] = mfma16<F16>(wa[m], xf[j][kk], acc[m][j]);
                    }
                    const int c0 = s2 * 32 + fg * 8;
                    float sc[8], sh[8];
                    *(float4*)&sc[0] = *(const float4*)(cst + c0); *(float4*)&sc[4] = *(const float4*)(cst + c0 + 4);
                    *(float4*)&sh[0] = *(const float4*)(cst + 64 + c0); *(float4*)&sh[4] = *(const float4*)(cst + 64 + c0 + 4);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        float y[8];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            y[q] = fmaxf(acc[0][j][q] * sc[q] + sh[q], 0.f);
                            y[4 + q] = fmaxf(acc[1][j][q] * sc[4 + q] + sh[4 + q], 0.f);
                        }
                        uint4 r;
                        r.x = pack2<F16>(y[0], y[1]); r.y = pack2<F16>(y[2], y[3]); r.z = pack2<F16>(y[4], y[5]); r.w = pack2<F16>(y[6], y[7]);
                        if (!in_cur[j]) r = make_uint4(0u, 0u, 0u, 0u);
                        *(uint4*)(lds_a + hr[j] * 128 + (((s2 * 4 + fg) ^ (hr[j] & 7)) << 4)) = r;
                    }
                }
                if (!DUMP && it + 1 < my_tiles) {               // x of the next tile into the registers phase A just freed
                    locate(tile_at(it + 1));
                    fetch();
                }
            }
            __syncthreads();                                    // B1: a visible
            if (it < my_tiles) {
                // ---- phase B of tile `it` -> b[it & 1]
                char* bb = lds_b + (it & 1) * kBlkBBytes;
                int dn = 0, dty = 0, dtx = 0;                   // DUMP: patch and tile origin of tile `it`
                if constexpr (DUMP) {
                    const int tile = tile_at(it);
                    dn = tile / tiles_per_patch;
                    const int rem = tile - dn * tiles_per_patch;
                    dty = rem / tiles_x; dtx = rem - dty * tiles_x;
                }
                const int sB = wave >> 1, half = wave & 1;
                const int cB = sB * 32 + fg * 8 + half * 4;
                const float4 sc = *(const float4*)(cst + 128 + cB), sh = *(const float4*)(cst + 192 + cB);
#pragma unroll
                for (int g4 = 0; g4 < 2; ++g4) {
                    f4_t acc[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = (f4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int row = (g4 * 4 + i + t / 3) * kBlkHaloW + frow + t % 3;
                                const bf16x8_t bq = *(const bf16x8_t*)(lds_a + row * 128 + (((kk * 4 + fg) ^ (row & 7)) << 4));
                                acc[i] = mfma16<F16>(wf[t][kk], bq, acc[i]);
                                if constexpr (DUMP) {
                                    // the centre tap of output row g4 * 4 + i IS a's inner pixel (that row, column frow), channel group kk * 4 + fg:
                                    // what phase A packed, as phase B reads it (phase A itself has no register left for a second store, above).
                                    // All four waves read it; the one that owns the row in phase A stores it
                                    if (t == 4 && wave == ((g4 * 4 + i) >> 1)) {
                                        const int oy = dty * 8 + g4 * 4 + i;
                                        if (oy < p.H && dtx * 16 + frow < p.W)
                                            *(uint4*)(dump_row(p.dump_a, dn, p.H, p.W, oy, dtx * 16) + kk * 64 + (frow * 128 + fg * 16)) = __builtin_bit_cast(uint4, bq);
                                    }
                                }
                            }
                        __builtin_amdgcn_sched_barrier(0);      // (keeps later taps' reads from being hoisted: registers)
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = (g4 * 4 + i) * 16 + frow;
                        uint2 r;
                        r.x = pack2<F16>(fmaxf(acc[i][0] * sc.x + sh.x, 0.f), fmaxf(acc[i][1] * sc.y + sh.y, 0.f));
                        r.y = pack2<F16>(fmaxf(acc[i][2] * sc.z + sh.z, 0.f), fmaxf(acc[i][3] * sc.w + sh.w, 0.f));
                        *(uint2*)(bb + row * 128 + (((sB * 4 + fg) ^ (row & 7)) << 4) + half * 8) = r;
                    }
                }
            }
            if constexpr (DUMP) {
                // the dump stores of phase B take registers this wave does not have while the next tile's x is in flight (the P waves' budget,
                // above): here that request goes out behind phase B.  Later, not different: in_cur was taken at the top of the iteration
                if (it + 1 < my_tiles) {
                    locate(tile_at(it + 1));
                    fetch();
                }
            }
            __syncthreads();                                    // B2: b[it & 1] complete; a and b[(it-1) & 1] free
        }
    } else {
        // =============================================== Q: phase C ===============================================
        // inner-pixel x of this wave's two output rows (2w, 2w+1): residual (identity) / second operand (projection)
        bf16x8_t xq[2][KA], xq_next[2][KA];
        auto fetch_q = [&](int tile, bf16x8_t (&dst)[2][KA]) __attribute__((always_inline)) {
            const int n = tile / tiles_per_patch;
            const int rem = tile - n * tiles_per_patch;
            const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int Y = ty * 8 + 2 * wave + j, X = tx * 16 + frow;
                const bool in = (Y < p.H) & (X < p.W);
                const uint32_t off = in ? (uint32_t)((n * p.H + Y) * p.W + X) * (uint32_t)PIXB + (uint32_t)(kZeroHeaderBytes + fg * 16) : 0u;
#pragma unroll
                for (int kk = 0; kk < KA; ++kk) dst[j][kk] = *(const bf16x8_t*)(p.x + off + kk * 64);
            }
        };
        fetch_q(tile_at(0), xq_next);
        __syncthreads();                                        // weights / constants visible (all eight waves)

        for (int it = 0; it <= my_tiles; ++it) {
            const bool work = it >= 1;
            const int tile = work ? tile_at(it - 1) : 0;
            const int n = tile / tiles_per_patch;
            const int rem = tile - n * tiles_per_patch;
            const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
            const int ox = tx * 16 + frow;
            bf16x8_t bf[2][2];
            if (work) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int kk = 0; kk < KA; ++kk) xq[j][kk] = xq_next[j][kk];
                const char* bb = lds_b + ((it - 1) & 1) * kBlkBBytes;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        const int row = (2 * wave + j) * 16 + frow;
                        bf[j][kk] = *(const bf16x8_t*)(bb + row * 128 + (((kk * 4 + fg) ^ (row & 7)) << 4));
                    }
            }
            if (it < my_tiles) fetch_q(tile_at(it), xq_next);   // one tile ahead
            auto channel_groups = [&](int s_lo, int s_hi) __attribute__((always_inline)) {
#pragma unroll
                for (int s3 = s_lo; s3 < s_hi; ++s3) {
                    f4_t acc[2][2];
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[m][j] = (f4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                        for (int m = 0; m < 2; ++m) {
                            const bf16x8_t wa = *(const bf16x8_t*)(lds_w3 + (kk * 16 + 2 * s3 + m) * 1024 + lane * 16);
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                bf16x8_t bq;
                                if constexpr (PROJ) bq = kk < 2 ? bf[j][kk & 1] : xq[j][kk & 1];
                                else bq = bf[j][kk & 1];
                                acc[m][j] = mfma16<F16>(wa, bq, acc[m][j]);
                            }
                        }
                    const int c0 = s3 * 32 + fg * 8;
                    float sc[8], sh[8];
                    *(float4*)&sc[0] = *(const float4*)(cst + 256 + c0); *(float4*)&sc[4] = *(const float4*)(cst + 256 + c0 + 4);
                    *(float4*)&sh[0] = *(const float4*)(cst + 512 + c0); *(float4*)&sh[4] = *(const float4*)(cst + 512 + c0 + 4);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        float y[8];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            y[q] = acc[0][j][q] * sc[q] + sh[q];
                            y[4 + q] = acc[1][j][q] * sc[4 + q] + sh[4 + q];
                        }
                        if constexpr (!PROJ) {
                            const uint4 rv = __builtin_bit_cast(uint4, xq[j][s3 % KA]);
                            y[0] += unpack_lo<F16>(rv.x); y[1] += unpack_hi<F16>(rv.x); y[2] += unpack_lo<F16>(rv.y); y[3] += unpack_hi<F16>(rv.y);
                            y[4] += unpack_lo<F16>(rv.z); y[5] += unpack_hi<F16>(rv.z); y[6] += unpack_lo<F16>(rv.w); y[7] += unpack_hi<F16>(rv.w);
                        }
#pragma unroll
                        for (int q = 0; q < 8; ++q) y[q] = fmaxf(y[q], 0.f);
                        uint4 r;
                        r.x = pack2<F16>(y[0], y[1]); r.y = pack2<F16>(y[2], y[3]); r.z = pack2<F16>(y[4], y[5]); r.w = pack2<F16>(y[6], y[7]);
                        const int oy = ty * 8 + 2 * wave + j;
                        if (oy < p.H && ox < p.W)
                            *(uint4*)((uint16_t*)p.out + (((size_t)n * p.H + oy) * p.W + ox) * 256 + c0) = r;
                    }
                    __builtin_amdgcn_sched_barrier(0);          // (keeps later groups' weight reads from being hoisted: registers)
                }
            };
            if (work) channel_groups(0, 4);
            __syncthreads();                                    // B1
            if (work) channel_groups(4, 8);
            __syncthreads();                                    // B2
        }
    }
}

// One instantiation per (precision, block kind); DUMP (BlockParams::dump_a set) selects the step check's form of the same kernel.
template <bool DUMP>
static hipError_t launch_bottleneck_form(const BlockParams& p, int precision, int grid, hipStream_t s)
{
    const int slot = (precision == kF16 ? 0 : 1) + (p.proj ? 2 : 0);
    auto go = [&](auto kernel, int lds, int threads, bool (&done)[64]) -> hipError_t {
        const hipError_t e = dynamic_lds_once((const void*)kernel, lds, done);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, p);
        return hipGetLastError();
    };
    if (p.pq) {
        static bool attr_done8[4][64] = {};
        bool (&done)[64] = attr_done8[slot];
        if (p.proj) return precision == kF16 ? go(bottleneck_fused_pq<true, 64, true, DUMP>, block_pq_lds_bytes(64, true), 512, done) : go(bottleneck_fused_pq<false, 64, true, DUMP>, block_pq_lds_bytes(64, true), 512, done);
        return precision == kF16 ? go(bottleneck_fused_pq<true, 256, false, DUMP>, block_pq_lds_bytes(256, false), 512, done) : go(bottleneck_fused_pq<false, 256, false, DUMP>, block_pq_lds_bytes(256, false), 512, done);
    }
    static bool attr_done[4][64] = {};
    bool (&done)[64] = attr_done[slot];
    if (p.proj) return precision == kF16 ? go(bottleneck_fused<true, 64, true, DUMP>, block_lds_bytes(64, true), 256, done) : go(bottleneck_fused<false, 64, true, DUMP>, block_lds_bytes(64, true), 256, done);
    return precision == kF16 ? go(bottleneck_fused<true, 256, false, DUMP>, block_lds_bytes(256, false), 256, done) : go(bottleneck_fused<false, 256, false, DUMP>, block_lds_bytes(256, false), 256, done);
}

hipError_t launch_bottleneck(const BlockParams& p, int precision, int num_cus, hipStream_t s, LaunchRec* rec)
{
    const int n_tiles = p.n * ((p.H + 7) / 8) * ((p.W + 15) / 16);
    const int grid = xcd_grid(n_tiles, num_cus);
    launch_rec(rec, p.pq ? SBBSEG_LAUNCH_BOTTLENECK_PQ : SBBSEG_LAUNCH_BOTTLENECK, 8 * 16, 256, 1, n_tiles, grid, 1, 0, !p.proj);
    if (p.dump_a || p.dump_b) {
        if (!p.dump_a || !p.dump_b) return hipErrorInvalidValue;
        return launch_bottleneck_form<true>(p, precision, grid, s);
    }
    return launch_bottleneck_form<false>(p, precision, grid, s);
}

}  // namespace sbbseg
