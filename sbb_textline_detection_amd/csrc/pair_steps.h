// pair_steps.h -- the steps of the fused 1x1 pair, "expand" (C -> 4C channels, BN, + residual x, ReLU) and the next block's "reduce" (4C -> C, BN,
// ReLU), that expand_reduce_x3.hip and conv3_expand_reduce.hip both run: the shape constants, the fragment loader, the x / weight requests, the
// wait that ties the x registers, and the epilogues.  Each exists ONCE, here (device_prims.h's rule, one level up: a wait or a store that is audited
// or fixed is audited or fixed for both kernels -- the round-6 race of the tile top had to be found twice).  What the kernels do NOT share stays
// with them: the per-step schedule (which step requests what, the wait counts' terms) and how a pixel block's byte offset is formed -- the steps
// take that as a callable `off_of(ni)`.  The layouts, the K-step order and the reasons are told in expand_reduce_x3.hip's header.
#pragma once
#include <type_traits>

#include "device_prims.h"

namespace sbbseg {

// C = channels of b and a' (128: stage 3, 256: stage 4); y and x have 4 C.  X3: split mode (hi | lo planes, K-steps of 32 channels, three MFMAs
// per product); else plain fp16 (K-steps of 64 channels = two k-halves, half the bytes everywhere).  A block of eight waves owns 64 pixels =
// kNI pixel blocks of 16 and walks the 4C channels of y in chunks of 256.
constexpr int kPairNI = 4;            // pixel blocks of 16 of a tile: the bound of every request / store loop below
template <int C, bool X3> struct PairShape {
    static constexpr int EB = X3 ? 4 : 2;                              // stored bytes per channel
    static constexpr int KCH = X3 ? 32 : 64;                           // channels per K-step
    static constexpr int KS1 = C / KCH;                                // K-steps of GEMM 1
    static constexpr int G2S = 256 / KCH;                              // K-steps of GEMM 2 per chunk
    static constexpr int NCH = C / 64;                                 // 256-channel chunks of y
    static constexpr int MI2 = C / 128;                                // row blocks of a' (and of conv3_expand_reduce's b) per wave
    static constexpr int LG2 = 2 * MI2;                                // weight loads per K-step of GEMM 2
    static constexpr int PB = C * EB, PY = 4 * C * EB, PA = C * EB;    // bytes per stored pixel: b, y / x, a'
    static constexpr int YROW = 256 * EB;                              // bytes per pixel of the y chunk's LDS image
    static constexpr int SLB = PB / 16, SLY = YROW / 16;               // 16-byte slots per LDS row
    static constexpr int kNI = kPairNI;
    static constexpr int kPlanes = X3 ? 2 : 1;                         // vector-memory operations per pixel block and 8-channel group: hi | lo
    // vector-memory operations of the epilogues per wave, the terms of the kernels' wait counts: y stores + x loads; a' stores
    static constexpr int kEpi1 = kNI * 2 * kPlanes, kEpi2 = kNI * kPlanes;
};

// the four pixel fragments (hi, lo / k-half 0, 1) of K-step k from an LDS image of `slots` 16-byte slots per pixel row: slot s of pixel p sits at
// slot (s + 2 (p & 15)) mod slots.  rot = fg + 2 frow, frv = frow (the lane's copies: see the asm at the kernels' tile top)
__device__ __attribute__((always_inline)) inline void pair_load_frags(const char* base, int row_bytes, int slots, int k, int rot, int frv,
                                                                      h8_t (&dh)[4], h8_t (&dl)[4])
{
    const int sh = (rot + 8 * k) & (slots - 1), sl = (rot + 8 * k + 4) & (slots - 1);
    const char* a = base + frv * row_bytes;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        dh[ni] = *(const h8_t*)(a + ni * 16 * row_bytes + (sh << 4));
        dl[ni] = *(const h8_t*)(a + ni * 16 * row_bytes + (sl << 4));
    }
}

// request the residual of one chunk, fragment-shaped: kNI * kPlanes loads (split mode: 8, plain: 4); off_of(ni) = byte offset of this lane's
// granule of pixel block ni in x
template <bool X3, class OffOf>
__device__ __attribute__((always_inline)) inline void pair_issue_x(u4_t (&xh)[4], u4_t (&xl)[4], u4_t xrsrc, OffOf&& off_of)
{
#pragma unroll
    for (int ni = 0; ni < kPairNI; ++ni) {
        const uint32_t off = off_of(ni);
        if constexpr (X3) xload2(xh[ni], xl[ni], off, xrsrc);
        else asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=&v"(xh[ni]) : "v"(off), "s"(xrsrc) : "memory");
    }
}
// all but the youngest N vector-memory operations are done, tied to the x registers.  x was requested an epilogue ago: older than every weight
// request already waited for -- the wait only ties the registers to that fact
template <bool X3, int N> __device__ __attribute__((always_inline)) inline void pair_wait_x(u4_t (&xh)[4], u4_t (&xl)[4])
{
    if constexpr (X3)
        asm volatile("s_waitcnt vmcnt(%8)" : "+v"(xh[0]), "+v"(xh[1]), "+v"(xh[2]), "+v"(xh[3]), "+v"(xl[0]), "+v"(xl[1]), "+v"(xl[2]), "+v"(xl[3])
                     : "n"(N) : "memory");
    else
        asm volatile("s_waitcnt vmcnt(%4)" : "+v"(xh[0]), "+v"(xh[1]), "+v"(xh[2]), "+v"(xh[3]) : "n"(N) : "memory");
}

// the weight request of step r of chunk j (r < KS1: GEMM 1, 4 loads; else GEMM 2's step r - KS1, LG2 loads).  w3frag =
// [chunk][K-step][wave][m][hi | lo][64 lanes x 16 B] (4 KB per wave and step), w1frag = [chunk][K-step][wave][mi2][hi | lo][..]; the resources
// start at the wave's fragments.  `wm` scales the step's offset: 1 (expand_reduce's timing probe: 0, every request reads the first step)
template <class S>
__device__ __attribute__((always_inline)) inline void pair_issue_w(int j, int r, u4_t (&d)[4], uint32_t wlane, uint32_t wm, u4_t w3rsrc, u4_t w1rsrc)
{
    if (r < S::KS1) wload4(d[0], d[1], d[2], d[3], wlane + wm * (uint32_t)((j * S::KS1 + r) * 8 * 4096), w3rsrc);
    else if constexpr (S::MI2 == 2) wload4(d[0], d[1], d[2], d[3], wlane + wm * (uint32_t)((j * S::G2S + r - S::KS1) * 8 * 4096), w1rsrc);
    else wload2(d[0], d[1], wlane + wm * (uint32_t)((j * S::G2S + r - S::KS1) * 8 * 2048), w1rsrc);
}

// ---- 8 (MI == 2) or 4 (MI == 1) consecutive output channels of one pixel block: what the epilogues share
// the stored form: split mode hi | lo halves, plain fp16 packed pairs (`lo` unused)
template <bool X3, int MI> struct PairPack {
    using V = std::conditional_t<X3, std::conditional_t<MI == 2, h8_t, h4_t>, std::conditional_t<MI == 2, u4_t, u2_t>>;
    __device__ __attribute__((always_inline)) static void pack(const float (&y)[4 * MI], V& hi, V& lo)
    {
        if constexpr (X3) {
            split_n<4 * MI>(y, hi, lo);
        } else {
            hi[0] = pack_h2(y[0], y[1]); hi[1] = pack_h2(y[2], y[3]);
            if constexpr (MI == 2) { hi[2] = pack_h2(y[4], y[5]); hi[3] = pack_h2(y[6], y[7]); }
        }
    }
};
// kPlanes stores of 16 / 8 bytes, the lo half 64 bytes behind.  (Every asm store ends in `s_nop 1`: the hazard recognizer does not see a store
// inside inline asm, so it does not insert the wait state the ISA wants between a store of more than 64 bits and a VALU write of its data registers
// -- lanes 12-15 of the first data register came out as the NEXT pixel block's values in the plain mode, where the compiler reuses the registers
// at once.)
template <bool X3, class V> __device__ __attribute__((always_inline)) inline void pair_store(uint32_t off, const V& hi, const V& lo, u4_t rsrc)
{
    if constexpr (X3 && sizeof(V) == 16)
        asm volatile("buffer_store_dwordx4 %1, %0, %3, 0 offen\n\tbuffer_store_dwordx4 %2, %0, %3, 0 offen offset:64\n\ts_nop 1"
                     :: "v"(off), "v"(hi), "v"(lo), "s"(rsrc) : "memory");
    else if constexpr (X3)
        asm volatile("buffer_store_dwordx2 %1, %0, %3, 0 offen\n\tbuffer_store_dwordx2 %2, %0, %3, 0 offen offset:64\n\ts_nop 1"
                     :: "v"(off), "v"(hi), "v"(lo), "s"(rsrc) : "memory");
    else if constexpr (sizeof(V) == 16)
        asm volatile("buffer_store_dwordx4 %1, %0, %2, 0 offen\n\ts_nop 1" :: "v"(off), "v"(hi), "s"(rsrc) : "memory");
    else
        asm volatile("buffer_store_dwordx2 %1, %0, %2, 0 offen\n\ts_nop 1" :: "v"(off), "v"(hi), "s"(rsrc) : "memory");
}
// first channel of this lane's 4 MI outputs of a [C / 8 channels x 64 px] wave tile (GEMM 2; conv3_expand_reduce's GEMM 0)
template <int MI> __device__ __attribute__((always_inline)) inline int pair_c0(int wave, int fgv)
{
    return MI == 2 ? wave * 32 + fgv * 8 : (wave >> 1) * 32 + fgv * 8 + (wave & 1) * 4;
}
template <int MI> __device__ __attribute__((always_inline)) inline void pair_bn_consts(const float* s, const float* h, int c0, float (&sc)[4 * MI],
                                                                                       float (&sh)[4 * MI])
{
    *(float4*)&sc[0] = *(const float4*)(s + c0);
    *(float4*)&sh[0] = *(const float4*)(h + c0);
    if constexpr (MI == 2) {
        *(float4*)&sc[4] = *(const float4*)(s + c0 + 4);
        *(float4*)&sh[4] = *(const float4*)(h + c0 + 4);
    }
}
// pack and store: kPlanes stores at byte offset `off`
template <bool X3, int MI>
__device__ __attribute__((always_inline)) inline void pair_pack_store(const float (&y)[4 * MI], uint32_t off, u4_t rsrc)
{
    typename PairPack<X3, MI>::V vh, vl;
    PairPack<X3, MI>::pack(y, vh, vl);
    pair_store<X3>(off, vh, vl, rsrc);
}
// (The BN + ReLU loop in front of it, y[q] = max(fma(acc, sc, sh), 0), stays written out in the kernels' epilogues 0 and 2: as a function of its
// own it changes nothing but the order in which the compiler meets the instructions, and expand_reduce<256, true> then pairs the split's
// subtractions differently -- profiles/kernel_share.md.)

// ---- epilogue 1 of a chunk: y = ReLU(s3 * acc + h3 + x) -> hi | lo: to HBM (kNI * kPlanes stores) and into the LDS image of the chunk.
// sc, sh = s3 * wmul3, h3 of this lane's 8 channels (the kernel loads them: its `cst` is a constant address there); off_of(ni) = byte offset of
// this lane's granule of pixel block ni in y, row_of(ni) = the LDS row of this lane's pixel of block ni.  The wave's 32 channels = granules
// wave * 4 + fg of the chunk (split mode: group `wave`, hi granules fg, lo granules 4 + fg); rot = fg + 2 frow.
// (round 5 timed the LDS writes with a conflict-free rotation -- one slot per pixel, results then wrong -- and found no difference:
//  profiles/r05_experiments.md section 6; the probe itself made the compiler add a vmcnt wait to the loop and is not kept)
template <class S, bool X3, class OffOf, class RowOf>
__device__ __attribute__((always_inline)) inline void pair_epilogue1(const f4_t (&acc1)[2][4], const u4_t (&xh)[4], const u4_t (&xl)[4], const float (&sc)[8],
                                                                     const float (&sh)[8], int wave, int rot, u4_t yrsrc, OffOf&& off_of, RowOf&& row_of)
{
    const int s_hi = (wave * (X3 ? 8 : 4) + rot) & (S::SLY - 1), s_lo = (wave * 8 + 4 + rot) & (S::SLY - 1);
#pragma unroll
    for (int ni = 0; ni < S::kNI; ++ni) {
        float y[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            y[q] = __builtin_fmaf(acc1[0][ni][q], sc[q], sh[q]);
            y[4 + q] = __builtin_fmaf(acc1[1][ni][q], sc[4 + q], sh[4 + q]);
        }
        const uint32_t off = off_of(ni);
        char* row = row_of(ni);
        typename PairPack<X3, 2>::V vh, vl;
        if constexpr (X3) {
            const h8_t rh = __builtin_bit_cast(h8_t, xh[ni]), rl = __builtin_bit_cast(h8_t, xl[ni]);
#pragma unroll
            for (int q = 0; q < 8; ++q) y[q] = fmaxf(__fadd_rn(y[q], __fadd_rn((float)rh[q], (float)rl[q])), 0.f);      // (= add_split8 + ReLU, kernels.hip)
        } else {
            const h8_t rr = __builtin_bit_cast(h8_t, xh[ni]);
#pragma unroll
            for (int q = 0; q < 8; ++q) y[q] = fmaxf(__fadd_rn(y[q], (float)rr[q]), 0.f);
        }
        PairPack<X3, 2>::pack(y, vh, vl);
        pair_store<X3>(off, vh, vl, yrsrc);
        *(typename PairPack<X3, 2>::V*)(row + (s_hi << 4)) = vh;
        if constexpr (X3) *(h8_t*)(row + (s_lo << 4)) = vl;
    }
}

}  // namespace sbbseg
