// expand_reduce_x3.hip -- stages 3 and 4 of the ResNet-50 encoder in the split-fp16 mode (kF16X3): the LAST 1x1 conv of an identity
// bottleneck block ("expand": C -> 4C channels, BN, + residual x, ReLU) and the FIRST 1x1 conv of the next block ("reduce": 4C -> C,
// BN, ReLU) in one launch, round 4.
//
//   y  = ReLU(s3 * (W3 . b) + h3 + x)          b: [M][C], x, y: [M][4C]   (y is still written: the next block's residual)
//   a' = ReLU(s1 * (W1 . y) + h1)              a': [M][C]
//
// As two launches of conv_igemm_mfma these layers are HBM-bound (3.1 - 4.5 TB/s): the expand reads b and x and writes y (4.5 C' bytes
// ... 9 KB per pixel in stage 4), the reduce reads y back (4 KB) and writes a'.  Fused, y goes from the expand's epilogue registers
// into LDS and is contracted there: 5 KB per pixel in place of 7 (stage 3), 10 in place of 14 (stage 4).
//
// A block of eight waves owns 64 consecutive pixels (the convs are pointwise: any 64) and walks the 4C channels of y in chunks of 256:
//   GEMM 1  y chunk [256 ch x 64 px] = W3 rows . b:  wave w owns 32 channels (2 row blocks) x 64 pixels, K = C in steps of 32 channels;
//           b (64 px x C, hi + lo) is resident in LDS for the whole tile (LDS-DMA, refilled for the next tile once the last chunk's GEMM 1
//           is through), W3 is streamed as A fragments straight into registers, two K-steps ahead
//   epilogue 1  BN, + x (loaded a chunk ahead into registers, fragment-shaped), ReLU, hi | lo split: 16-byte stores of y AND the same
//           registers into the LDS image of the chunk (64 px x 256 ch)
//   GEMM 2  a' [C ch x 64 px] += W1[:, chunk] . y chunk:  wave w owns C / 8 output channels x 64 pixels, accumulators live across chunks,
//           8 K-steps per chunk, W1 streamed like W3
//   epilogue 2  BN, ReLU, split, stores of a'
// Both contractions walk the K-steps in the order of the convs they replace, three MFMAs per product (lo*hi, hi*lo, hi*hi), one
// accumulator per output, and state the same epilogue arithmetic: y and a' are bit-identical to the two launches (tests/test_gpu_parity.py).
// (Every asm store ends in `s_nop 1`: the hazard recognizer does not see a store inside inline asm, so it does not insert the wait state the
// ISA wants between a store of more than 64 bits and a VALU write of its data registers -- lanes 12-15 of the first data register came out
// as the NEXT pixel block's values in the plain mode, where the compiler reuses the registers at once.)
// The steps named above -- fragment loads, x / weight requests, the epilogues' arithmetic and stores -- are pair_steps.h's, shared with
// conv3_expand_reduce.hip; this unit holds the schedule: which step requests what, and the terms of every wait count.
// Every vector-memory operation of the loop is issued from inline asm and waited for by a hand-counted vmcnt (retirement is in issue
// order): see dec_halo_x3.hip for why.  Pixel rows in LDS are C * 4 bytes (b) / 1 KB (y chunk); 16-byte slot s of pixel p sits at slot
// (s + 2 (p & 15)) mod row: conflict-free for the 16-lane groups of ds_read_b128 (64 banks); the epilogue's ds_write_b128 (32 banks, 8-lane
// groups) lands two lanes on a bank -- PMC: 13-17 % of the LDS-busy cycles are conflict cycles, all from those 16 writes per chunk.
#include "pair_steps.h"

namespace sbbseg {

// C = channels of b and a' (128: stage 3, 256: stage 4); y and x have 4 C.  X3: split mode (hi | lo planes, K-steps of 32 channels, three
// MFMAs per product); else plain fp16 (K-steps of 64 channels = two k-halves: the fragment pair (hi, lo) of the text above reads (kk = 0,
// kk = 1), one MFMA each, half the bytes everywhere) -- the same K-steps / accumulation order / epilogue arithmetic as conv_igemm_mfma's
// plain mode: bit-identical there too.
template <int C, bool X3>
__global__ __launch_bounds__(512, 2) void expand_reduce(const ExpRedParams p)
{
    using S = PairShape<C, X3>;                                 // the pair's shape (pair_steps.h), under the names the schedule below uses
    constexpr int EB = S::EB, KS1 = S::KS1, G2S = S::G2S, NCH = S::NCH, MI2 = S::MI2, LG2 = S::LG2, PB = S::PB, PY = S::PY, PA = S::PA, YROW = S::YROW;
    constexpr int SLB = S::SLB, SLY = S::SLY, kEpi1 = S::kEpi1;
    constexpr int kBBytes = 64 * PB, kYBytes = 64 * YROW;
    constexpr int STEPS = NCH * (KS1 + G2S);                    // K-steps per tile, both GEMMs (even)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const lds_b = smem;
    char* const lds_y = smem + kBBytes;
    float* const cst = (float*)(smem + kBBytes + kYBytes);      // s3 * wmul3 [4C] | h3 [4C] | s1 * wmul1 [C] | h1 [C]
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LDS_AS char*)smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fg = lane >> 4;
    const int n_tiles = (p.M + 63) >> 6;
    const int G = gridDim.x;
    const int my_tiles = (n_tiles - (int)blockIdx.x + G - 1) / G;
    if (my_tiles <= 0) return;
    auto tile_at = [&](int it) __attribute__((always_inline)) -> int { return (int)blockIdx.x + (it < my_tiles ? it : my_tiles - 1) * G; };

    for (int i = tid; i < 4 * C; i += 512) { cst[i] = p.s3[i] * p.wmul3; cst[4 * C + i] = p.h3[i]; }
    for (int i = tid; i < C; i += 512) { cst[8 * C + i] = p.s1[i] * p.wmul1; cst[9 * C + i] = p.h1[i]; }

    // ---- b tile DMA: instruction i fills bytes [1024 i, 1024 i + 1024) of the LDS image (64 rows of PB bytes); wave w issues i = w + 8 k.
    // (pixel / source granule of a lane are recomputed per tile from `dlane`: 2 x KS1 registers the loop has no room for)
    int dlane = lane;
    auto issue_b = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < KS1; ++k) {
            const int byte = (wave + 8 * k) * 1024 + dlane * 16;
            const int px = byte / PB, slot = (byte - px * PB) >> 4;
            const int go = ((slot - 2 * (px & 15)) & (SLB - 1)) * 16;          // byte offset of the source granule inside the stored pixel
            const int m = tile * 64 + px;
            const uint32_t off = m < p.M ? (uint32_t)m * (uint32_t)PB + (uint32_t)(go + kZeroHeaderBytes) : 0u;
            glds16_hidden(p.b + off, lds0 + (uint32_t)((wave + 8 * k) * 1024));
        }
    };

    // ---- buffers: x (read), y, a' (written); an offset past the end reads zero / is dropped (the last tile of a ragged M)
    const u4_t xrsrc = make_rsrc(p.x + kZeroHeaderBytes, (uint32_t)p.M * (uint32_t)PY);
    const u4_t yrsrc = make_rsrc(p.y + kZeroHeaderBytes, (uint32_t)p.M * (uint32_t)PY);
    const u4_t arsrc = make_rsrc(p.a2 + kZeroHeaderBytes, (uint32_t)p.M * (uint32_t)PA);
    // weights: w3frag = [chunk][K-step][wave][m][hi | lo][64 lanes x 16 B] (4 KB per wave and step), w1frag = [chunk][K-step][wave][mi2][hi | lo][..]
    const u4_t w3rsrc = make_rsrc((const char*)p.w3frag + wave * 4096, (uint32_t)(NCH * KS1 * 8 * 4096));
    const u4_t w1rsrc = make_rsrc((const char*)p.w1frag + wave * (LG2 * 1024), (uint32_t)(NCH * G2S * 8 * LG2 * 1024));
    uint32_t wlane = (uint32_t)lane * 16u;
    int frv = frow, fgv = fg;                                   // (copies the tile loop re-derives its addresses from: see the asm at its top)

    // lane-constant pieces of the addresses
    int rot = fg + 2 * frow;                                    // slot of granule fg of this lane's pixel row, before the K-step's 8 k
    uint32_t xlane = (uint32_t)(frow * PY + wave * (32 * EB) + fg * 16);      // x / y: pixel frow of a 16-pixel block, the wave's 32 channels of a chunk
    uint32_t alane = MI2 == 2 ? (uint32_t)(frow * PA + wave * (32 * EB) + fg * 16)
                              : (uint32_t)(frow * PA + (wave >> 1) * (32 * EB) + fg * 16 + (wave & 1) * 8);

    // step u of a tile: chunk j, GEMM 1 K-step k (u % (KS1 + 8) < KS1) or GEMM 2 K-step k
    u4_t w[2][4];                                               // weight ring: step u in set u & 1
    h8_t bh[2][4], bl[2][4];                                    // pixel fragments of step u in set u & 1
    u4_t xh[4], xl[4];                                          // the residual of the chunk ahead: [pixel block]
    auto issue_w = [&](int u, u4_t (&d)[4]) __attribute__((always_inline)) {             // u in [0, STEPS)
        const int j = u / (KS1 + G2S), r = u % (KS1 + G2S);
        const uint32_t wm = SBBSEG_PROBE(p.dbg & 1) ? 0u : 1u;                 // (timing probe: every request reads the first step's fragments)
        pair_issue_w<S>(j, r, d, wlane, wm, w3rsrc, w1rsrc);
    };
    auto issue_x = [&](int tile, int j) __attribute__((always_inline)) {                  // kEpi1 / 2 loads
        pair_issue_x<X3>(xh, xl, xrsrc, [&](int ni) __attribute__((always_inline)) -> uint32_t {
            return (SBBSEG_PROBE(p.dbg & 4) ? 0xf0000000u : 0u) + xlane + (uint32_t)(tile * 64 + ni * 16) * (uint32_t)PY + (uint32_t)(j * YROW);
        });
    };
    auto load_frags = [&](const char* base, int row_bytes, int slots, int k, h8_t (&dh)[4], h8_t (&dl)[4]) __attribute__((always_inline)) {
        pair_load_frags(base, row_bytes, slots, k, rot, frv, dh, dl);
    };

    // ---- prologue: the first tile's b and its first chunk of x
    issue_b(tile_at(0));
    issue_x(tile_at(0), 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        asm volatile("" : "+v"(xh[ni]));
        if constexpr (X3) asm volatile("" : "+v"(xl[ni]));
    }
    __syncthreads();                                            // b, constants visible
    issue_w(0, w[0]);
    issue_w(1, w[1]);

    for (int it = 0; it < my_tiles; ++it) {
        const int tile = tile_at(it), tile_next = tile_at(it + 1);
        asm volatile("" : "+v"(rot), "+v"(xlane), "+v"(alane), "+v"(wlane), "+v"(dlane), "+v"(frv), "+v"(fgv));
        f4_t acc2[MI2][4];
#pragma unroll
        for (int m = 0; m < MI2; ++m)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc2[m][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};
        f4_t acc1[2][4];
        static_for<0, STEPS>([&](auto uc) __attribute__((always_inline)) {
            constexpr int u = decltype(uc)::value;
            constexpr int j = u / (KS1 + G2S), r = u % (KS1 + G2S);
            constexpr bool g1 = r < KS1;
            constexpr int k = g1 ? r : r - KS1;
            constexpr int set = u & 1;
            // loads per weight request of the step after this one (its request is the only one younger than this step's, but for the
            // epilogues in between)
            constexpr int un = (u + 1) % STEPS;
            constexpr int Lnext = (un % (KS1 + G2S)) < KS1 ? 4 : LG2;
            // vector-memory operations issued between this step's weight request (end of step u - 2) and here, beside that one request:
            //   GEMM 2 steps 0, 1: epilogue 1 (+ the b DMA behind the last chunk's)     GEMM 1 steps 0, 1 of chunk 0: the previous tile's epilogue 2
            constexpr int extra = (!g1 && k < 2) ? kEpi1 + (j == NCH - 1 ? KS1 : 0) : 0;
            if constexpr (g1 && k == 0) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc1[m][ni] = (f4_t){0.f, 0.f, 0.f, 0.f};
                load_frags(lds_b, PB, SLB, 0, bh[set], bl[set]);                 // (not requested ahead across the barrier in front of this phase)
            }
            if constexpr (!g1 && k == 0) load_frags(lds_y, YROW, SLY, 0, bh[set], bl[set]);
            // the next step's pixel fragments, inside a phase
            if constexpr (g1 && k + 1 < KS1) load_frags(lds_b, PB, SLB, k + 1, bh[set ^ 1], bl[set ^ 1]);
            if constexpr (!g1 && k + 1 < G2S) load_frags(lds_y, YROW, SLY, k + 1, bh[set ^ 1], bl[set ^ 1]);
            u4_t (&cw)[4] = w[set];
            if constexpr (g1 && j == 0 && k < 2) {
                // (round 6: the previous tile's a' stores are younger than this step's weight request but are NOT allowed for in the count:
                //  a block's FIRST tile has no epilogue in front of it, the count with the stores in was looser than what is in flight there, and
                //  steps 0 / 1 could multiply weights still on their way.  conv3_expand_reduce, which has the same tile top, lost that race once in
                //  ~1e5 tiles when its weight loads missed L2: profiles/r06_experiments.md section 7.  One statement, not an if / else pair of
                //  two asm waits: see there too)
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
                h8_t ah[MI2], al[MI2];
#pragma unroll
                for (int m = 0; m < MI2; ++m) { ah[m] = __builtin_bit_cast(h8_t, cw[2 * m]); al[m] = __builtin_bit_cast(h8_t, cw[2 * m + 1]); }
                mma_step<X3, MI2>(acc2, ah, al, ph, pl);
            }
            // this set's weights are spent: step u + 2 (of the next tile behind the last two; always issued: the counts stay constant)
            issue_w((u + 2) % STEPS, cw);
            __builtin_amdgcn_sched_barrier(0);

            if constexpr (g1 && k == KS1 - 1) {
                // ---- epilogue 1: y = ReLU(s3 * acc + h3 + x) -> hi | lo: to HBM and into the LDS image of the chunk.  x of this chunk was requested
                // an epilogue ago: older than every weight request already waited for (the wait below only ties the registers to that fact)
                pair_wait_x<X3, 2 * LG2>(xh, xl);
                const int c0 = j * 256 + wave * 32 + fgv * 8;
                float sc[8], sh[8];                             // (loaded here, where `cst` is a constant address: profiles/kernel_share.md)
                *(float4*)&sc[0] = *(const float4*)(cst + c0); *(float4*)&sc[4] = *(const float4*)(cst + c0 + 4);
                *(float4*)&sh[0] = *(const float4*)(cst + 4 * C + c0); *(float4*)&sh[4] = *(const float4*)(cst + 4 * C + c0 + 4);
                pair_epilogue1<S, X3>(
                    acc1, xh, xl, sc, sh, wave, rot, yrsrc,
                    [&](int ni) __attribute__((always_inline)) -> uint32_t {
                        return (SBBSEG_PROBE(p.dbg & 2) ? 0xf0000000u : 0u) + xlane + (uint32_t)(tile * 64 + ni * 16) * (uint32_t)PY + (uint32_t)(j * YROW);
                    },
                    [&](int ni) __attribute__((always_inline)) -> char* { return lds_y + (ni * 16 + frv) * YROW; });
                // the residual of the chunk after this one (the next tile's first behind the last)
                if constexpr (j + 1 < NCH) issue_x(tile, j + 1);
                else issue_x(tile_next, 0);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // the y chunk is complete; (last chunk) every wave is through with b
                asm volatile("" ::: "memory");
                if constexpr (j == NCH - 1) issue_b(tile_next);
            }
            if constexpr (!g1 && k == G2S - 1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // every wave has taken its last fragment of this y chunk (last chunk: and has waited
                asm volatile("" ::: "memory");                  // for its share of the next tile's b: steps >= 2 of this GEMM)
            }
        });

        // ---- epilogue 2: a' = ReLU(s1 * acc + h1) -> hi | lo.  EXACTLY kEpi2 stores per wave.
        {
            float sc[4 * MI2], sh[4 * MI2];
            pair_bn_consts<MI2>(cst + 8 * C, cst + 9 * C, pair_c0<MI2>(wave, fgv), sc, sh);
#pragma unroll
            for (int ni = 0; ni < S::kNI; ++ni) {
                const uint32_t off = alane + (uint32_t)(tile * 64 + ni * 16) * (uint32_t)PA;
                float y[4 * MI2];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    y[q] = fmaxf(__builtin_fmaf(acc2[0][ni][q], sc[q], sh[q]), 0.f);
                    if constexpr (MI2 == 2) y[4 + q] = fmaxf(__builtin_fmaf(acc2[MI2 - 1][ni][q], sc[4 * (MI2 - 1) + q], sh[4 * (MI2 - 1) + q]), 0.f);
                }
                pair_pack_store<X3, MI2>(y, off, arsrc);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int C, bool X3> static hipError_t launch_one(const ExpRedParams& p, int num_cus, hipStream_t s, LaunchRec* rec)
{
    constexpr int EB = X3 ? 4 : 2;
    constexpr int lds = 64 * C * EB + 64 * 256 * EB + 10 * C * 4;
    static bool attr_done[64] = {};
    const hipError_t e = dynamic_lds_once((const void*)expand_reduce<C, X3>, lds, attr_done);
    if (e != hipSuccess) return e;
    const int n_tiles = (p.M + 63) / 64;
    const int grid = n_tiles < num_cus ? n_tiles : num_cus;
    launch_rec(rec, SBBSEG_LAUNCH_EXPAND_REDUCE, 64, 4 * C, 1, n_tiles, grid, 1, 0, 1);
    hipLaunchKernelGGL((expand_reduce<C, X3>), dim3(grid), dim3(512), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_expand_reduce_x3(const ExpRedParams& p, int num_cus, hipStream_t s, LaunchRec* rec)
{
    if (p.C == 128) return p.x3 ? launch_one<128, true>(p, num_cus, s, rec) : launch_one<128, false>(p, num_cus, s, rec);
    if (p.C == 256) return p.x3 ? launch_one<256, true>(p, num_cus, s, rec) : launch_one<256, false>(p, num_cus, s, rec);
    return hipErrorInvalidValue;
}

}  // namespace sbbseg
