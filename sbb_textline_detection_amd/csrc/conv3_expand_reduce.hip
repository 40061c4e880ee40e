// conv3_expand_reduce.hip -- an identity bottleneck block's 3x3 conv, its last 1x1 conv and the NEXT block's first 1x1 conv in one launch
// (round 6; encoder stage 3 at 56 x 56, C = 128):
//
//   b  = ReLU(s2 * (W2 * a) + h2)              a, b: [n][H][W][C], 3x3 / stride 1 / zero padding 1        ("GEMM 0", new here)
//   y  = ReLU(s3 * (W3 . b) + h3 + x)          x, y: [n][H][W][4C]                                         (expand_reduce's GEMM 1)
//   a' = ReLU(s1 * (W1 . y) + h1)              a': [n][H][W][C]                                            (expand_reduce's GEMM 2)
//
// As two launches (conv_igemm_mfma for the 3x3, expand_reduce for the pair) b makes a round trip through HBM, the 3x3 is MFMA-bound
// with the memory system idle and the pair is HBM-bound with the matrix pipe 25 % busy.  Here a block of eight waves owns an 8 x 8
// pixel tile: the 10 x 10 halo of `a` is copied to LDS (LDS-DMA, in pieces of 256 bytes per pixel, rotated as in dec_halo_*: tile_walk.h), GEMM 0
// contracts it tap by tap into b, which goes from the epilogue registers straight into the LDS image expand_reduce's GEMM 1 reads; the
// halo of the NEXT tile is fetched while GEMM 1 / GEMM 2 of this one run, and the x / y streams of the pair run under GEMM 0 of the next.
// From GEMM 1 on this IS expand_reduce (same K-steps, same order, same MFMA triple, same epilogue arithmetic: the same functions, pair_steps.h,
// with this kernel's pixel-block offsets), and GEMM 0 walks the
// K-steps of the conv it replaces in that conv's order (taken from its K-step records) with its epilogue arithmetic: b, y and a' are
// bit-identical to the three launches (tests/test_gpu_parity.py).  b itself is never written to HBM.
// Every vector-memory operation of the loop is issued from inline asm and waited for by a hand-counted vmcnt (see dec_halo_x3.hip).
// One count is deliberately NOT the tight steady-state one: GEMM 0's first two steps wait `vmcnt(weights of the next step)` although the
// previous tile's a' stores (epilogue 2) are younger than their own weight request and could be left in flight.  The tight count
// `next step + 4 stores` is only right from a block's second tile on: its FIRST tile has no epilogue in front of it, the count is then
// looser than what is in flight, and steps 0 / 1 multiplied weight registers whose loads had not landed whenever those loads missed L2 --
// one tile in ~10^5 in the plain fp16 mode (tools/first_run_probe.py: a whole patch's labels, run to run; with the first tile drained in
// the prologue and the stores allowed for again: 0 of 144, profiles/r06_experiments.md section 7).  `vmcnt(next step)` is right for every
// tile and costs nothing measurable (the stores are acknowledged by then).  expand_reduce had the same tile top since round 4.  And the
// wait is one statement, not an `if (first tile) ... else ...` pair: the `"+v"` ties of two asm statements in two branches make the
// compiler copy the weight registers in front of one of them -- a copy of registers whose loads are still in flight.
#include "pair_steps.h"
#include "tile_walk.h"

namespace sbbseg {

namespace {

constexpr int kPieceBytes = kHalo10Bytes;    // one 256-byte piece of every pixel of the 10 x 10 halo (tile_walk.h)

}  // namespace

// C = channels of a, b and a' (128); x and y have 4 C.  X3: split mode (hi | lo planes, K-steps of 32 channels, three MFMAs per product);
// else plain fp16 (K-steps of 64 channels as two k-halves).  Tiles are 8 x 8 pixels: pixel block ni (16 pixels) = tile rows 2 ni, 2 ni + 1;
// lane frow of a fragment = pixel (2 ni + (frow >> 3), frow & 7) -- the index ni * 16 + frow is what expand_reduce calls the tile's pixel.
template <int C, bool X3>
__global__ __launch_bounds__(512, 2) void conv3_expand_reduce(const C3ERParams p)
{
    static_assert(C == 128, "stage 3 only (LDS: the split mode's halo + b + y chunk fill it at C = 128)");
    using S = PairShape<C, X3>;                                 // the pair's shape (pair_steps.h), under the names the schedule below uses
    constexpr int EB = S::EB, KS1 = S::KS1, G2S = S::G2S, NCH = S::NCH, MI2 = S::MI2, LG2 = S::LG2, PB = S::PB, PY = S::PY, PA = S::PA, YROW = S::YROW;
    constexpr int SLB = S::SLB, SLY = S::SLY, kEpi1 = S::kEpi1;
    constexpr int KS0 = 9 * C / S::KCH;                         // K-steps of GEMM 0 (LG2 weight loads each, as GEMM 2)
    constexpr int NP = PB / 256;                                // 256-byte pieces of a halo pixel
    constexpr int kHaloBytes = NP * kPieceBytes, kBBytes = 64 * PB, kYBytes = 64 * YROW;
    constexpr int PER = KS1 + G2S;                              // K-steps of one chunk
    constexpr int STEPS = KS0 + NCH * PER;                      // K-steps per tile, all three GEMMs (even)
    constexpr int kDma = kHalo10PerWave * NP;                   // halo DMA instructions per wave and tile
    static_assert(STEPS % 2 == 0 && KS0 % 2 == 0, "the weight ring alternates two register sets");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const lds_a = smem;                                   // NP pieces of [100 px][256 B]
    char* const lds_b = smem + kHaloBytes;
    char* const lds_y = lds_b + kBBytes;
    float* const cst = (float*)(lds_y + kYBytes);               // s3 * wmul3 [4C] | h3 [4C] | s1 * wmul1 [C] | h1 [C] | s2 * wmul2 [C] | h2 [C]
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LDS_AS char*)smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fg = lane >> 4;
    const int tiles_x = p.W >> 3, tiles_y = p.H >> 3;
    const int tpp = tiles_x * tiles_y;
    const int n_tiles = p.n * tpp;
    const XcdWalk walk = xcd_walk(n_tiles, blockIdx, gridDim);      // (neighbouring tiles share halo lines in one L2)
    const int my_tiles = walk.my_tiles;
    if (my_tiles <= 0) return;
    // tile -> patch, first pixel row / column
    auto tile_coords = [&](int tile, int& n, int& y0, int& x0) __attribute__((always_inline)) {
        n = tile / tpp;
        const int rem = tile - n * tpp;
        const int ty = rem / tiles_x;
        y0 = ty * 8;
        x0 = (rem - ty * tiles_x) * 8;
    };

    for (int i = tid; i < 4 * C; i += 512) { cst[i] = p.s3[i] * p.wmul3; cst[4 * C + i] = p.h3[i]; }
    for (int i = tid; i < C; i += 512) {
        cst[8 * C + i] = p.s1[i] * p.wmul1; cst[9 * C + i] = p.h1[i];
        cst[10 * C + i] = p.s2[i] * p.wmul2; cst[11 * C + i] = p.h2[i];
    }

    // ---- halo DMA (tile_walk.h: halo10_*): NP pieces, kHalo10PerWave loads per wave each
    int halo_e[kHalo10PerWave];
#pragma unroll
    for (int m = 0; m < kHalo10PerWave; ++m) halo_e[m] = halo10_desc(wave, lane, m);
    auto issue_halo = [&](int tile) __attribute__((always_inline)) {
        int n, y0, x0;
        tile_coords(tile, n, y0, x0);
        // (halo10_issue's loop, written out: through the shared function one addition of the prologue's burst comes out with its operands
        //  swapped -- profiles/kernel_share.md)
#pragma unroll
        for (int pc = 0; pc < NP; ++pc)
#pragma unroll
            for (int m = 0; m < kHalo10PerWave; ++m) {
                const int e = halo_e[m];
                const int Y = y0 - 1 + (e & 255), X = x0 - 1 + ((e >> 8) & 255);
                const bool ok = (unsigned)Y < (unsigned)p.H && (unsigned)X < (unsigned)p.W;
                const uint32_t off = ok ? (uint32_t)((n * p.H + Y) * p.W + X) * (uint32_t)PB + (uint32_t)(pc * 256 + ((e >> 16) & 15) * 16 + kZeroHeaderBytes) : 0u;
                const uint32_t dst = lds0 + (uint32_t)(pc * kPieceBytes) + (uint32_t)__builtin_amdgcn_readfirstlane(e >> 24) * 1024u;
                glds16_hidden(p.a + off, dst);
            }
    };

    const uint32_t npix = (uint32_t)p.n * (uint32_t)p.H * (uint32_t)p.W;
    const u4_t xrsrc = make_rsrc(p.x + kZeroHeaderBytes, npix * (uint32_t)PY);
    const u4_t yrsrc = make_rsrc(p.y + kZeroHeaderBytes, npix * (uint32_t)PY);
    const u4_t arsrc = make_rsrc(p.a2 + kZeroHeaderBytes, npix * (uint32_t)PA);
    // weights: w2frag = [K-step][wave][mi][hi | lo][64 lanes x 16 B], w3frag = [chunk][K-step][wave][m][hi | lo][..] (4 KB per wave and step),
    // w1frag = [chunk][K-step][wave][mi2][hi | lo][..]
    const u4_t w2rsrc = make_rsrc((const char*)p.w2frag + wave * (LG2 * 1024), (uint32_t)(KS0 * 8 * LG2 * 1024));
    const u4_t w3rsrc = make_rsrc((const char*)p.w3frag + wave * 4096, (uint32_t)(NCH * KS1 * 8 * 4096));
    const u4_t w1rsrc = make_rsrc((const char*)p.w1frag + wave * (LG2 * 1024), (uint32_t)(NCH * G2S * 8 * LG2 * 1024));
    uint32_t wlane = (uint32_t)lane * 16u;
    int frv = frow, fgv = fg;

    // lane-constant pieces of the addresses.  A tile's pixel (ni, frow) is image pixel (y0 + 2 ni + (frow >> 3), x0 + (frow & 7))
    int rot = fg + 2 * frow;                                    // b / y images: slot of granule fg of this lane's pixel row, before the K-step's 8 k
    const int i0 = frow >> 3, j0 = frow & 7;
    uint32_t xlane = (uint32_t)((i0 * p.W + j0) * PY + wave * (32 * EB) + fg * 16);
    uint32_t alane = MI2 == 2 ? (uint32_t)((i0 * p.W + j0) * PA + wave * (32 * EB) + fg * 16)
                              : (uint32_t)((i0 * p.W + j0) * PA + (wave >> 1) * (32 * EB) + fg * 16 + (wave & 1) * 8);
    const uint32_t ni_y = (uint32_t)(2 * p.W) * (uint32_t)PY, ni_a = (uint32_t)(2 * p.W) * (uint32_t)PA;      // pixel block ni + 1 = two image rows down
    int a0 = (i0 + 1) * 10 + j0 + 1, r0 = fg + 2 * (j0 + 1);    // halo: pixel index / slot of this lane's centre tap
    // GEMM 0's K-steps (the conv's own order): (dy & 255) | (dx & 255) << 8 | channel group << 16, wave-uniform
    int k0[KS0];
    {
        const __attribute__((address_space(4))) int* kp = (const __attribute__((address_space(4))) int*)(uintptr_t)p.k0;
#pragma unroll
        for (int t = 0; t < KS0; ++t) k0[t] = kp[t];
    }

    u4_t w[2][4];                                               // weight ring: step u in set u & 1
    h8_t bh[2][4], bl[2][4];                                    // pixel fragments of step u in set u & 1
    u4_t xh[4], xl[4];                                          // the residual of the chunk ahead: [pixel block]
    auto issue_w = [&](int u, u4_t (&d)[4]) __attribute__((always_inline)) {             // u in [0, STEPS)
        if (u < KS0) {
            if constexpr (MI2 == 2) wload4(d[0], d[1], d[2], d[3], wlane + (uint32_t)(u * 8 * 4096), w2rsrc);
            else wload2(d[0], d[1], wlane + (uint32_t)(u * 8 * 2048), w2rsrc);
            return;
        }
        const int v = u - KS0;
        pair_issue_w<S>(v / PER, v % PER, d, wlane, 1u, w3rsrc, w1rsrc);
    };
    auto issue_x = [&](uint32_t pix0, int j) __attribute__((always_inline)) {             // kEpi1 / 2 loads
        pair_issue_x<X3>(xh, xl, xrsrc, [&](int ni) __attribute__((always_inline)) -> uint32_t {
            return xlane + pix0 * (uint32_t)PY + (uint32_t)ni * ni_y + (uint32_t)(j * YROW);
        });
    };
    auto load_frags = [&](const char* base, int row_bytes, int slots, int k, h8_t (&dh)[4], h8_t (&dl)[4]) __attribute__((always_inline)) {
        pair_load_frags(base, row_bytes, slots, k, rot, frv, dh, dl);
    };
    // GEMM 0, K-step t: tap (dy, dx) of channel group cg: piece cg >> 1, granules 8 (cg & 1) + fg (first fragment) and + 4 (second) of halo pixel
    // (2 ni + i0 + dy + 1, j0 + dx + 1); slot = (granule + 2 hx) & 15
    auto load_halo = [&](int t, h8_t (&dh)[4], h8_t (&dl)[4]) __attribute__((always_inline)) {
        const int rec = k0[t];
        const int dy = (rec << 24) >> 24, dx = (rec << 16) >> 24, cg = rec >> 16;
        const int hp = a0 + dy * 10 + dx;
        const int sh = (r0 + 2 * dx + 8 * (cg & 1)) & 15;
        const char* base = lds_a + (cg >> 1) * kPieceBytes + hp * 256;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            dh[ni] = *(const h8_t*)(base + ni * (20 * 256) + (sh << 4));
            dl[ni] = *(const h8_t*)(base + ni * (20 * 256) + (((sh + 4) & 15) << 4));
        }
    };

    // ---- prologue: the first tile's halo and its first chunk of x
    int cn, cy0, cx0;
    tile_coords(walk.tile_at_clamped(0), cn, cy0, cx0);
    uint32_t pix0 = (uint32_t)((cn * p.H + cy0) * p.W + cx0);
    issue_halo(walk.tile_at_clamped(0));
    issue_x(pix0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        asm volatile("" : "+v"(xh[ni]));
        if constexpr (X3) asm volatile("" : "+v"(xl[ni]));
    }
    __syncthreads();                                            // halo, constants visible
    issue_w(0, w[0]);
    issue_w(1, w[1]);

    for (int it = 0; it < my_tiles; ++it) {
        int nn, ny0, nx0;
        tile_coords(walk.tile_at_clamped(it + 1), nn, ny0, nx0);
        const uint32_t pix_next = (uint32_t)((nn * p.H + ny0) * p.W + nx0);
        asm volatile("" : "+v"(rot), "+v"(xlane), "+v"(alane), "+v"(wlane), "+v"(frv), "+v"(fgv), "+v"(a0), "+v"(r0));
#pragma unroll
        for (int t = 0; t < KS0; ++t) asm volatile("" : "+s"(k0[t]));
        f4_t acc2[MI2][4];
        f4_t acc1[2][4];
        static_for<0, STEPS>([&](auto uc) __attribute__((always_inline)) {
            constexpr int u = decltype(uc)::value;
            constexpr bool g0 = u < KS0;
            constexpr int v = g0 ? 0 : u - KS0;
            constexpr int j = v / PER, r = v % PER;
            constexpr bool g1 = !g0 && r < KS1;
            constexpr int k = g0 ? u : (g1 ? r : r - KS1);
            constexpr int set = u & 1;
            // loads of the weight request of the step after this one (the only request younger than this step's, but for the bursts below)
            constexpr int un = (u + 1) % STEPS;
            constexpr int Lnext = un < KS0 ? LG2 : (((un - KS0) % PER) < KS1 ? 4 : LG2);
            // vector-memory operations issued between this step's weight request (end of step u - 2) and here, beside that one request:
            //   GEMM 0 steps 0, 1: the previous tile's epilogue 2 (a' stores)      GEMM 1 steps 0, 1 of chunk 0: the next tile's halo DMA
            //   GEMM 2 steps 0, 1: epilogue 1 (y stores + x loads)
            constexpr int extra = (!g0 && !g1 && k < 2) ? kEpi1 : ((g1 && j == 0 && k < 2) ? kDma : 0);
            if constexpr (g0 && k == 0) {
#pragma unroll
                for (int m = 0; m < MI2; ++m)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc2[m][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};      // (GEMM 0's accumulators live in acc2: same shape)
                load_halo(0, bh[set], bl[set]);
            }
            if constexpr (g1 && k == 0) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc1[m][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};
                load_frags(lds_b, PB, SLB, 0, bh[set], bl[set]);
            }
            if constexpr (!g0 && !g1 && k == 0) load_frags(lds_y, YROW, SLY, 0, bh[set], bl[set]);
            // the next step's pixel fragments, inside a phase
            if constexpr (g0 && k + 1 < KS0) load_halo(k + 1, bh[set ^ 1], bl[set ^ 1]);
            if constexpr (g1 && k + 1 < KS1) load_frags(lds_b, PB, SLB, k + 1, bh[set ^ 1], bl[set ^ 1]);
            if constexpr (!g0 && !g1 && k + 1 < G2S) load_frags(lds_y, YROW, SLY, k + 1, bh[set ^ 1], bl[set ^ 1]);
            u4_t (&cw)[4] = w[set];
            if constexpr (g0 && k < 2) {
                // (the a' stores of the previous tile's epilogue 2 sit between this step's weight request and here -- but not on a block's
                //  first tile: they are NOT allowed for in the count, see the header)
                wait4<Lnext>(cw[0], cw[1], cw[2], cw[3]);
            } else {
                wait4<Lnext + extra>(cw[0], cw[1], cw[2], cw[3]);
            }
            const h8_t (&ph)[4] = bh[set];
            const h8_t (&pl)[4] = bl[set];
            if constexpr (g1) {
                const h8_t ah[2] = {__builtin_bit_cast(h8_t, cw[0]), __builtin_bit_cast(h8_t, cw[2])};       // (plain mode: k-half 0)
                const h8_t al[2] = {__builtin_bit_cast(h8_t, cw[1]), __builtin_bit_cast(h8_t, cw[3])};       // (             k-half 1)
                mma_step<X3, 2>(acc1, ah, al, ph, pl);
            } else {
                // GEMM 0 and GEMM 2: C / 8 output channels x 64 pixels per wave
                h8_t ah[MI2], al[MI2];
#pragma unroll
                for (int m = 0; m < MI2; ++m) { ah[m] = __builtin_bit_cast(h8_t, cw[2 * m]); al[m] = __builtin_bit_cast(h8_t, cw[2 * m + 1]); }
                mma_step<X3, MI2>(acc2, ah, al, ph, pl);
            }
            // this set's weights are spent: step u + 2 (of the next tile behind the last two; always issued: the counts stay constant)
            issue_w((u + 2) % STEPS, cw);
            __builtin_amdgcn_sched_barrier(0);

            if constexpr (g0 && k == KS0 - 1) {
                // ---- epilogue 0: b = ReLU(s2 * acc + h2) -> the LDS image GEMM 1 reads (granule G of pixel p at slot (G + 2 (p & 15)) mod SLB).
                // No vector-memory operation here: the hand-counted queue is untouched
                const int c0 = MI2 == 2 ? wave * 32 + fgv * 8 : (wave >> 1) * 32 + fgv * 8 + (wave & 1) * 4;      // (= pair_c0)
                float sc[4 * MI2], sh[4 * MI2];
                *(float4*)&sc[0] = *(const float4*)(cst + 10 * C + c0);
                *(float4*)&sh[0] = *(const float4*)(cst + 11 * C + c0);
                if constexpr (MI2 == 2) {
                    *(float4*)&sc[4] = *(const float4*)(cst + 10 * C + c0 + 4);
                    *(float4*)&sh[4] = *(const float4*)(cst + 11 * C + c0 + 4);
                }
                // byte offset of channel c0 inside the stored pixel: split mode = groups of 32 channels [32 hi][32 lo]
                const int boff = X3 ? (c0 >> 5) * 128 + (c0 & 31) * 2 : c0 * 2;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    float y[4 * MI2];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        y[q] = fmaxf(__builtin_fmaf(acc2[0][ni][q], sc[q], sh[q]), 0.f);
                        if constexpr (MI2 == 2) y[4 + q] = fmaxf(__builtin_fmaf(acc2[MI2 - 1][ni][q], sc[4 * (MI2 - 1) + q], sh[4 * (MI2 - 1) + q]), 0.f);
                    }
                    char* row = lds_b + (ni * 16 + frv) * PB;
                    const int s_hi = ((boff >> 4) + 2 * frv) & (SLB - 1), s_lo = (((boff + 64) >> 4) + 2 * frv) & (SLB - 1);
                    // (epilogue 2's packing; to LDS where that stores.  MI2 == 1: 8 bytes, the half of the granule boff points into)
                    using V = typename PairPack<X3, MI2>::V;
                    V vh, vl;
                    PairPack<X3, MI2>::pack(y, vh, vl);
                    *(V*)(row + (s_hi << 4) + (MI2 == 2 ? 0 : boff & 8)) = vh;
                    if constexpr (X3) *(V*)(row + (s_lo << 4) + (MI2 == 2 ? 0 : boff & 8)) = vl;
                }
#pragma unroll
                for (int m = 0; m < MI2; ++m)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc2[m][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};      // GEMM 2 accumulates across the chunks from here
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // b is complete; every wave has taken its last fragment from the halo
                asm volatile("" ::: "memory");
                issue_halo(walk.tile_at_clamped(it + 1));                    // the next tile's halo lands under GEMM 1 / GEMM 2 (kDma loads per wave)
            }
            if constexpr (g1 && k == KS1 - 1) {
                // ---- epilogue 1 (expand_reduce's): y = ReLU(s3 * acc + h3 + x) -> hi | lo: to HBM and into the LDS image of the chunk
                pair_wait_x<X3, 2 * LG2>(xh, xl);
                const int c0 = j * 256 + wave * 32 + fgv * 8;
                float sc[8], sh[8];                             // (loaded here, where `cst` is a constant address: profiles/kernel_share.md)
                *(float4*)&sc[0] = *(const float4*)(cst + c0); *(float4*)&sc[4] = *(const float4*)(cst + c0 + 4);
                *(float4*)&sh[0] = *(const float4*)(cst + 4 * C + c0); *(float4*)&sh[4] = *(const float4*)(cst + 4 * C + c0 + 4);
                pair_epilogue1<S, X3>(
                    acc1, xh, xl, sc, sh, wave, rot, yrsrc,
                    [&](int ni) __attribute__((always_inline)) -> uint32_t { return xlane + pix0 * (uint32_t)PY + (uint32_t)ni * ni_y + (uint32_t)(j * YROW); },
                    [&](int ni) __attribute__((always_inline)) -> char* { return lds_y + (ni * 16 + frv) * YROW; });
                // the residual of the chunk after this one (the next tile's first behind the last)
                if constexpr (j + 1 < NCH) issue_x(pix0, j + 1);
                else issue_x(pix_next, 0);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // the y chunk is complete
                asm volatile("" ::: "memory");
            }
            if constexpr (!g0 && !g1 && k == G2S - 1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // every wave has taken its last fragment of this y chunk (and, past GEMM 1's first steps
                asm volatile("" ::: "memory");                  // of chunk 0, has waited for its share of the next tile's halo)
            }
        });

        // ---- epilogue 2: a' = ReLU(s1 * acc + h1) -> hi | lo.  EXACTLY kEpi2 stores per wave.
        {
            float sc[4 * MI2], sh[4 * MI2];
            pair_bn_consts<MI2>(cst + 8 * C, cst + 9 * C, pair_c0<MI2>(wave, fgv), sc, sh);
#pragma unroll
            for (int ni = 0; ni < S::kNI; ++ni) {
                const uint32_t off = alane + pix0 * (uint32_t)PA + (uint32_t)ni * ni_a;
                float y[4 * MI2];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    y[q] = fmaxf(__builtin_fmaf(acc2[0][ni][q], sc[q], sh[q]), 0.f);
                    if constexpr (MI2 == 2) y[4 + q] = fmaxf(__builtin_fmaf(acc2[MI2 - 1][ni][q], sc[4 * (MI2 - 1) + q], sh[4 * (MI2 - 1) + q]), 0.f);
                }
                pair_pack_store<X3, MI2>(y, off, arsrc);
            }
        }
        pix0 = pix_next;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int C, bool X3> static hipError_t launch_one(const C3ERParams& p, int num_cus, hipStream_t s, LaunchRec* rec)
{
    constexpr int EB = X3 ? 4 : 2;
    constexpr int lds = (C * EB / 256) * kPieceBytes + 64 * C * EB + 64 * 256 * EB + 12 * C * 4;
    static_assert(lds <= 160 * 1024, "conv3_expand_reduce: LDS");
    static bool attr_done[64] = {};
    const hipError_t e = dynamic_lds_once((const void*)conv3_expand_reduce<C, X3>, lds, attr_done);
    if (e != hipSuccess) return e;
    const int n_tiles = p.n * (p.H / 8) * (p.W / 8);
    if (n_tiles <= 0) return hipSuccess;
    const int grid = xcd_grid(n_tiles, num_cus);
    launch_rec(rec, SBBSEG_LAUNCH_CONV3_EXPAND_REDUCE, 8 * 8, 4 * C, 1, n_tiles, grid, 1, 0, 1);
    hipLaunchKernelGGL((conv3_expand_reduce<C, X3>), dim3(grid), dim3(512), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_conv3_expand_reduce(const C3ERParams& p, int num_cus, hipStream_t s, LaunchRec* rec)
{
    if (p.C == 128) return p.x3 ? launch_one<128, true>(p, num_cus, s, rec) : launch_one<128, false>(p, num_cus, s, rec);
    return hipErrorInvalidValue;
}

}  // namespace sbbseg
