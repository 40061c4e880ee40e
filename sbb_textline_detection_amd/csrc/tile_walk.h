// tile_walk.h -- how the persistent kernels of libsbbseg find their tiles, stated once for the device side AND the host side that sizes the grid:
// the XCD-contiguous walk (block_x3, bottleneck, direct64, dec_tail, dec_halo_*, conv3_expand_reduce), the owned-region table lookup of the
// dec_halo_* pair and the 10 x 10 halo DMA (dec_halo_* src0; conv3_expand_reduce: the descriptor and the counts, its issue loop is written out
// there).  The walk is plain arithmetic: tests/test_xcd_walk_cpu.py runs it on the CPU.  (expand_reduce, the stem kernels and conv_igemm_mfma
// walk differently and keep their walks.)  What is shaped oddly here -- blockIdx handed over whole, parameters by address -- is shaped so that
// every kernel compiles to the instructions it had with the text in place: profiles/kernel_share.md.
#pragma once
#include "device_prims.h"

namespace sbbseg {

// ---- XCD-contiguous walk.  Consecutive blocks land on consecutive XCDs (block b on XCD b % 8), and neighbouring tiles share halo lines, so XCD x
// owns the contiguous tiles [x * per_xcd, (x + 1) * per_xcd): its grid / 8 blocks walk that range with stride grid / 8 and the shared lines meet
// in one L2.  The grid must be a multiple of 8 (xcd_grid): with a ragged grid some XCD's range would have no block to walk it.
struct XcdWalk {
    int xcd_lo, slot, GX, my_tiles;      // first tile of this block's XCD, the block's place among the XCD's GX blocks, tiles this block owns
    __host__ __device__ int tile_at(int it) const { return xcd_lo + slot + it * GX; }      // it in [0, my_tiles)
    // ... for kernels that request "the tile after this one" unconditionally: past the end, the block's last tile again
    __host__ __device__ int tile_at_clamped(int it) const { return xcd_lo + slot + (it < my_tiles ? it : my_tiles - 1) * GX; }
};
// block, grid: blockIdx and gridDim (on the host: anything with an unsigned `x`).  They are read here, in this order -- handed over as two
// loaded values the sums below come out associated differently in conv3x3_c64_direct_x3
template <class B, class G> __host__ __device__ inline XcdWalk xcd_walk(int n_tiles, const B& block, const G& grid)
{
    const int xcd = block.x & 7, slot = block.x >> 3, GX = grid.x >> 3;
    const int per_xcd = (n_tiles + 7) >> 3;
    const int xcd_lo = xcd * per_xcd, xcd_hi = n_tiles < xcd_lo + per_xcd ? n_tiles : xcd_lo + per_xcd;
    const int my_tiles = xcd_lo + slot < xcd_hi ? (xcd_hi - xcd_lo - slot + GX - 1) / GX : 0;
    return XcdWalk{xcd_lo, slot, GX, my_tiles};
}
// blocks to launch for a walk over n_tiles with room for `resident` blocks at once (the CU count, or twice it): a multiple of 8
inline int xcd_grid(int n_tiles, int resident) { return ((n_tiles < resident ? n_tiles : resident) + 7) & ~7; }

// ---- tile -> patch and output origin of the dec_halo_* kernels (16 x 16 outputs; wave-uniform).  With an owned-region table
// (DecHaloParams::ttab, region.h) the tiles are the table's entries -- patch << 22 | (y0 / 2) << 11 | x0 / 2, any even origin; tiles of one patch
// may overlap at its far edge (same values twice), the entry comes through the scalar cache -- instead of the grid of every patch.
__device__ __attribute__((always_inline)) inline void dec_tile_coords(const __attribute__((address_space(4))) uint32_t* ttab, int tile,
                                                                      int tiles_per_patch, int tiles_x, int& n, int& y0, int& x0)
{
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
}

// ---- 10 x 10 halo of an 8 x 8 pixel tile as one LDS piece of [100 px][256 B], by LDS-DMA.  Instruction k of a piece fills halo pixels
// 4 k .. 4 k + 3; lane l writes slot l & 15 of pixel 4 k + (l >> 4) and fetches granule (slot - 2 hx) & 15 of the pixel's 256 bytes: granule G of
// halo pixel (hy, hx) sits at slot (G + 2 hx) & 15, conflict-free for the 16-lane groups of ds_read_b128.  Wave w of eight issues k = w, w + 8,
// w + 16, w + 24 (past 24: k - 25 again, same bytes to the same place): every wave issues kHalo10PerWave loads per piece, a constant the
// kernels' hand-counted waits are built from.
constexpr int kHalo10Instr = 25;                 // wave-instructions of 4 pixels x 256 B per piece
constexpr int kHalo10Bytes = kHalo10Instr * 1024;
constexpr int kHalo10PerWave = 4;
// tile-invariant part of this lane's load m of kHalo10PerWave: hy | hx << 8 | source granule << 16 | instruction << 24
__device__ __attribute__((always_inline)) inline int halo10_desc(int wave, int lane, int m)
{
    int k = wave + 8 * m;
    k = k < kHalo10Instr ? k : k - kHalo10Instr;
    const int hp = 4 * k + (lane >> 4);
    const int hy = hp / 10, hx = hp - hy * 10;
    return hy | (hx << 8) | ((((lane & 15) - 2 * hx) & 15) << 16) | (k << 24);
}
// one piece: halo pixel (hy, hx) is pixel (Y0 + hy, X0 + hx) of patch n of a [n][H][W] image of pix_bytes per stored pixel behind the zero
// header (outside the image: the header's zeros), its 256 bytes start at `byte0` of the pixel; `dst` is the piece's LDS byte address.
// src, H and W are the ADDRESSES of the kernel's parameters: each is then loaded where the kernels' own loops loaded it (W behind the
// comparison with H, src behind the offset).  Handed over by value the three loads are hoisted in front of the burst, the two comparisons merge
// into one, and dec_halo_x3 is scheduled into four more registers.
__device__ __attribute__((always_inline)) inline void halo10_issue(const int (&e)[kHalo10PerWave], const char* const* src, int n, int Y0, int X0,
                                                                   const int* H, const int* W, uint32_t pix_bytes, int byte0, uint32_t dst)
{
#pragma unroll
    for (int m = 0; m < kHalo10PerWave; ++m) {
        const int d = e[m];
        const int Y = Y0 + (d & 255), X = X0 + ((d >> 8) & 255);
        const bool ok = (unsigned)Y < (unsigned)*H && (unsigned)X < (unsigned)*W;
        const uint32_t off = ok ? (uint32_t)((n * *H + Y) * *W + X) * pix_bytes + (uint32_t)(byte0 + ((d >> 16) & 15) * 16 + kZeroHeaderBytes) : 0u;
        const uint32_t to = dst + (uint32_t)__builtin_amdgcn_readfirstlane(d >> 24) * 1024u;
        glds16_hidden(*src + off, to);
    }
}

}  // namespace sbbseg
