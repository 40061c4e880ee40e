// device_prims.h -- the low-level device primitives the gfx950 kernel units of libsbbseg share: vector types, 16-bit packing, the
// hi | lo split of the label-exact mode, MFMA wrappers and the K-step built from them, and the inline-asm loads / waits whose counts the kernels
// keep by hand.  (The steps built from these that several units run: tile_walk.h, pair_steps.h.)
// Each exists ONCE, here: a wait or an M0 save that is audited or fixed is audited or fixed for every kernel.  A unit keeps a private
// variant only where the instructions differ (stem_pool_x3.hip: split1).
#pragma once
#include "internal.h"

namespace sbbseg {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;   // 8 bf16 = one 16-byte granule
typedef __attribute__((ext_vector_type(8))) _Float16 h8_t;    // 8 fp16
typedef __attribute__((ext_vector_type(4))) _Float16 h4_t;
typedef __attribute__((ext_vector_type(2))) _Float16 h2_t;
typedef __attribute__((ext_vector_type(4))) float f4_t;
typedef __attribute__((ext_vector_type(4))) unsigned u4_t;
typedef __attribute__((ext_vector_type(2))) unsigned u2_t;

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

template <int N> struct IC { static constexpr int value = N; };
// f(IC<B>{}), f(IC<B + 1>{}), ... f(IC<E - 1>{}): the index is a compile-time constant in every copy (register sets are selected by
// it; `#pragma unroll` left dec_halo_x3's 34-step loop rolled and the sets in scratch memory)
template <int B, int E, class F> __device__ __attribute__((always_inline)) inline void static_for(F&& f)
{
    if constexpr (B < E) {
        f(IC<B>{});
        static_for<B + 1, E>(f);
    }
}

// ---- 16-bit elements
__host__ __device__ inline uint16_t bf16_bits_rne(float f)
{
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ inline float bf16_lo(uint32_t v) { return __builtin_bit_cast(float, v << 16); }
__device__ inline float bf16_hi(uint32_t v) { return __builtin_bit_cast(float, v & 0xffff0000u); }
__device__ inline uint32_t pack_bf16x2(float a, float b)
{
    uint32_t r;                                   // gfx950 packed RNE convert (no builtin)
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// fp16 twins (SBBSEG_PREC_F16): saturate instead of overflowing to inf, round to nearest even
__device__ inline uint32_t pack_h2(float a, float b)
{
    a = fminf(fmaxf(a, -65504.f), 65504.f);
    b = fminf(fmaxf(b, -65504.f), 65504.f);
    h2_t v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ inline float f16_lo(uint32_t v) { return (float)__builtin_bit_cast(h2_t, v)[0]; }
__device__ inline float f16_hi(uint32_t v) { return (float)__builtin_bit_cast(h2_t, v)[1]; }

template <bool F16> __device__ inline uint32_t pack2(float a, float b) { return F16 ? pack_h2(a, b) : pack_bf16x2(a, b); }
template <bool F16> __device__ inline float unpack_lo(uint32_t v) { return F16 ? f16_lo(v) : bf16_lo(v); }
template <bool F16> __device__ inline float unpack_hi(uint32_t v) { return F16 ? f16_hi(v) : bf16_hi(v); }

// ---- MFMA
__device__ inline f4_t mma(h8_t a, h8_t b, f4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
// w * x with both operands split: small terms first
__device__ inline f4_t mma3(h8_t wh, h8_t wl, h8_t xh, h8_t xl, f4_t c) { return mma(wh, xh, mma(wh, xl, mma(wl, xh, c))); }
// One K-step on a wave tile of M row blocks x 4 pixel blocks, one accumulator per output.  Split mode (X3): (ah, al) / (ph, pl) are the hi and lo
// halves of the weights / pixels, three sweeps, small terms first -- al . ph, ah . pl, ah . ph, the order conv_igemm_mfma's split loop uses per
// accumulator.  Plain fp16: (ah, al) / (ph, pl) are the two k-halves of a 64-channel step, k-half 0 before k-half 1.
template <bool X3, int M>
__device__ __attribute__((always_inline)) inline void mma_step(f4_t (&acc)[M][4], const h8_t (&ah)[M], const h8_t (&al)[M], const h8_t (&ph)[4],
                                                               const h8_t (&pl)[4])
{
    if constexpr (X3) {
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[m][ni] = mma(al[m], ph[ni], acc[m][ni]);
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[m][ni] = mma(ah[m], pl[ni], acc[m][ni]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[m][ni] = mma(ah[m], ph[ni], acc[m][ni]);
    if constexpr (!X3) {
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[m][ni] = mma(al[m], pl[ni], acc[m][ni]);
    }
}
template <bool F16> __device__ inline f4_t mfma16(bf16x8_t a, bf16x8_t b, f4_t c)
{
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, a), __builtin_bit_cast(h8_t, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ---- split mode (kF16X3) element helpers: v = hi + lo, hi = fp16(v) (saturating), lo = fp16(v - hi)
__device__ inline void split_f32(float v, _Float16& hi, _Float16& lo)
{
    v = fminf(fmaxf(v, -65504.f), 65504.f);
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);               // exact difference (Sterbenz-like: |v - hi| <= ulp(hi)/2), then one rounding
}
template <int N, class V> __device__ inline void split_n(const float (&y)[N], V& hi, V& lo)
{
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float v = fminf(fmaxf(y[q], -65504.f), 65504.f);
        const _Float16 h = (_Float16)v;
        hi[q] = h;
        lo[q] = (_Float16)(v - (float)h);
    }
}
__device__ inline void split8(const float (&y)[8], h8_t& hi, h8_t& lo) { split_n(y, hi, lo); }
// 8 consecutive channels of one pixel: hi halves at dst, lo halves `plane` elements behind
__device__ inline void store_split8(uint16_t* dst, int plane, const float (&y)[8])
{
    h8_t h, l;
#pragma unroll
    for (int q = 0; q < 8; ++q) { _Float16 a, b; split_f32(y[q], a, b); h[q] = a; l[q] = b; }
    *(h8_t*)dst = h;
    *(h8_t*)(dst + plane) = l;
}

// value of lane (l ^ 8) inside each row of 16 lanes (DPP row_ror:8)
__device__ inline uint32_t row_ror8(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
}

// ---- wave-wide (64 lanes) reductions and scans of integers: every lane returns the result of the whole wave (reductions) or of lanes
// 0 .. its own (inclusive scans).  Integer sums are exact in any order, so these never decide a bit.
__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ inline int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ inline long long wave_scan_sum(long long v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long below = __shfl_up(v, off, 64);
        if (lane >= off) v += below;
    }
    return v;
}

// ---- vector memory.  The wload / xload / glds16_hidden loads are invisible to the compiler's own wait insertion: a kernel that issues
// them counts its vmcnt by hand (retirement is in issue order) and ties the destination registers to the wait (wait4).
// buffer resource over [base, base + bytes): wave-uniform words, out-of-range lanes read zeros
__device__ inline u4_t make_rsrc(const void* base, uint32_t bytes)
{
    u4_t r;
    const uint64_t b = (uint64_t)(uintptr_t)base;
    r[0] = __builtin_amdgcn_readfirstlane((uint32_t)b);
    r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32) & 0xffffu);
    r[2] = __builtin_amdgcn_readfirstlane(bytes);
    r[3] = 0x00020000u;
    return r;
}
// four weight fragments (1 KB apart) of one K-step: 16 bytes per lane each, destination registers valid after wait4
__device__ __attribute__((always_inline)) inline void wload4(u4_t& a, u4_t& b, u4_t& c, u4_t& d, uint32_t voff, u4_t rsrc)
{
    asm volatile("buffer_load_dwordx4 %0, %4, %5, 0 offen\n\t"
                 "buffer_load_dwordx4 %1, %4, %5, 0 offen offset:1024\n\t"
                 "buffer_load_dwordx4 %2, %4, %5, 0 offen offset:2048\n\t"
                 "buffer_load_dwordx4 %3, %4, %5, 0 offen offset:3072"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d) : "v"(voff), "s"(rsrc) : "memory");
}
__device__ __attribute__((always_inline)) inline void wload2(u4_t& a, u4_t& b, uint32_t voff, u4_t rsrc)
{
    asm volatile("buffer_load_dwordx4 %0, %2, %3, 0 offen\n\t"
                 "buffer_load_dwordx4 %1, %2, %3, 0 offen offset:1024"
                 : "=&v"(a), "=&v"(b) : "v"(voff), "s"(rsrc) : "memory");
}
// a pixel's hi and lo granule (64 bytes apart)
__device__ __attribute__((always_inline)) inline void xload2(u4_t& h, u4_t& l, uint32_t voff, u4_t rsrc)
{
    asm volatile("buffer_load_dwordx4 %0, %2, %3, 0 offen\n\t"
                 "buffer_load_dwordx4 %1, %2, %3, 0 offen offset:64"
                 : "=&v"(h), "=&v"(l) : "v"(voff), "s"(rsrc) : "memory");
}
// all but the youngest N vector-memory operations of this wave have completed; ties the four registers to the wait
template <int N> __device__ __attribute__((always_inline)) inline void wait4(u4_t& a, u4_t& b, u4_t& c, u4_t& d)
{
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
template <int N> __device__ inline void wait_vmcnt()
{
    // (the counter field holds 0..63: a larger count cannot be expressed -> drain)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N > 63 ? 0 : N) : "memory");
}

// One LDS-DMA wave-instruction the compiler does not see: lane l's 16 bytes at gsrc(l) land at LDS byte address lds_dst + 16 l
// (wave-uniform; M0 is written in the statement that reads it, and restored).  After the BUILTIN hipcc waits vmcnt(0) in front of the
// next LDS access it cannot tell apart from the DMA's destination, whatever that access touches -- in stem_conv_pairs the
// epilogue-constant read in the middle of a tile, i.e. the NEXT tile's halo, just requested, had to land there (0.260 -> 0.252 ms per
// 140 patches; the same change measured nothing on dec_tail_fused, two blocks per CU, which keeps the builtin).  A kernel that uses
// this waits for its DMA by hand (a counted s_waitcnt at the top of a tile or in front of a K-step).
__device__ __attribute__((always_inline)) inline void glds16_hidden(const void* gsrc, uint32_t lds_dst)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// ... with the destination as a generic pointer into LDS
__device__ __attribute__((always_inline)) inline void glds16_hidden(const void* gsrc, const char* lds_dst)
{
    glds16_hidden(gsrc, (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(const LDS_AS char*)lds_dst));
}

// one `buffer_load_dwordx4 ... offen lds`: lane l's 16 bytes at base + voff(l) + soff land at lds + 16 * l; a lane whose
// voff + soff reaches past nrec gets zeros (the resource words are wave-uniform and hoisted out of the loops)
__device__ inline void buffer_load_lds16(const void* base, uint32_t nrec, LDS_AS void* lds, uint32_t voff, uint32_t soff)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)nrec, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, lds, 16, voff, soff, 0, 0);
}

}  // namespace sbbseg
