// region.h -- owned-region launches of the decoder (round 6).
//
// do_prediction pastes only a part of every tile's label map into the page (main.py:294-364): the 10 % margin is cropped on every side
// that is not a page edge, and where the inward-clamped last tile of an axis overlaps its neighbour the later tile wins (main.py:276-281 +
// the paste order).  What survives of tile t along one axis -- its OWNED range -- is a closed form of the page geometry (region_own below:
// the per-axis rule `stitch_kernel`'s owner tables are built from).  A 3500 x 2500 page keeps 8.75 of the 14.05 Mpx its 70 tiles produce.
//
// The decoder is local: a level is a 3x3 conv over [nearest-x2 upsampling of the level below, skip from the encoder], followed by
// pointwise work.  So the rows a level must produce are the owned rows dilated by one pixel per 3x3 conv above it and halved per
// upsampling (region_down) -- the encoder, whose receptive field spans the tile, is computed whole.  The fused page paths launch the
// decoder convs and the tail over these regions only:
//   * conv_igemm_mfma (the parity-split decoder convs): a per-launch table maps the compact pixel index of a class grid to
//     (patch, y, x) -- kind 1 below;
//   * dec_halo_* and dec_tail_fused* (16 x 16 output tiles): a per-launch table of tile origins -- kind 0.
// Every computed pixel goes through exactly the arithmetic of the full launch (same K order, same epilogue), so the label map the stitch
// assembles is bit-identical; pixels outside a tile's region are simply never written (and never read: region_down covers every tap).
// The tables are built on the device per launch chunk (region.hip) from the closed forms below; the host evaluates the same closed forms
// for the entry counts (grid sizes, executed-work accounting).
#pragma once
#include "internal.h"

namespace sbbseg {

constexpr int kRegionMaxLevels = 8;

// one axis of the page's tile grid (main.py:246-281): n tiles of `tile` pixels, origin(t) = min(t * mid, extent - tile)
struct RegionAxis {
    int extent, tile, margin, mid, n;
};

struct RegionGeom {
    RegionAxis ax, ay;            // x axis (outer loop of the reference, index i), y axis (inner, index j)
    int tpp, ny;                  // tiles per page (ax.n * ay.n), tiles per column: grid index g -> i = g / ny, j = g % ny
    int n_levels;                 // level 0 = the network output (tail), level k = the decoder conv k steps below it
    int kind[kRegionMaxLevels];   // 0: table of 16 x 16 output tiles; 1: table of class-grid pixels (four output-parity classes)
    int Rh[kRegionMaxLevels], Rw[kRegionMaxLevels];      // output size of the level
    int align_x[kRegionMaxLevels];                        // kind 0: tile origins in x are multiples of this (16-byte label rows: 16; else 2)
};

SBBSEG_HD inline int region_origin(const RegionAxis& a, int t) { return t * a.mid + a.tile > a.extent ? a.extent - a.tile : t * a.mid; }

// [lo, hi) in TILE coordinates of what the stitch keeps of tile t (empty: lo == hi): the margin crop of main.py:294-364, minus
// everything a later tile of the axis writes -- later ranges chain up without a gap, so only the next tile's first pixel matters
SBBSEG_HD inline void region_own(const RegionAxis& a, int t, int& lo, int& hi)
{
    const int o = region_origin(a, t);
    lo = t == 0 ? 0 : a.margin;
    hi = t == a.n - 1 ? a.tile : a.tile - a.margin;
    if (t + 1 < a.n) {
        const int cut = region_origin(a, t + 1) + a.margin - o;
        if (cut < hi) hi = cut;
    }
    if (hi < lo) hi = lo;
}

// rows of the level below (half the resolution, R_below rows) that rows [lo, hi) of a level read: output row Y takes rows Y - 1 .. Y + 1 of
// the nearest-x2 upsampling = rows (Y - 1) >> 1 .. (Y + 1) >> 1 below (outside the tensor: zero padding)
SBBSEG_HD inline void region_down(int& lo, int& hi, int R_below)
{
    if (hi <= lo) { lo = hi = 0; return; }
    lo = lo > 0 ? (lo - 1) >> 1 : 0;
    hi = (hi >> 1) + 1;
    if (hi > R_below) hi = R_below;
}

// The owner of coordinate q of an axis: the last tile in paste order whose kept range [origin + lo, origin + hi) (region_own before its
// cut) contains q, as (tile << 16) | (q - origin) -- the value stitch_kernel's uploaded tables hold.  Tiles 0 .. n - 2 sit on unclamped
// origins (a clamped tile n - 2 repeats tile n - 1's origin and is overwritten by it wherever they differ), so their kept ranges
// [t * mid + margin, (t + 1) * mid + margin) tile the axis; the last tile takes everything from its own margin on.
SBBSEG_HD inline int region_owner(const RegionAxis& a, int q)
{
    int t = a.n - 1;
    if (a.n > 1 && q < region_origin(a, a.n - 1) + a.margin) t = q < a.margin ? 0 : (q - a.margin) / a.mid;
    return (t << 16) | (q - region_origin(a, t));
}

// rows [lo, hi) / columns of level `level` that patch (i, j) of the grid ax x ay must produce (before the level's own rounding below)
SBBSEG_HD inline void region_needed(const RegionGeom& g, const RegionAxis& ax, const RegionAxis& ay, int i, int j, int level, int& ylo, int& yhi,
                                    int& xlo, int& xhi)
{
    region_own(ay, j, ylo, yhi);
    region_own(ax, i, xlo, xhi);
    if (yhi <= ylo || xhi <= xlo) { ylo = yhi = xlo = xhi = 0; return; }
    for (int k = 1; k <= level; ++k) {
        region_down(ylo, yhi, g.Rh[k]);
        region_down(xlo, xhi, g.Rw[k]);
    }
}
SBBSEG_HD inline void region_needed(const RegionGeom& g, int i, int j, int level, int& ylo, int& yhi, int& xlo, int& xhi)
{
    region_needed(g, g.ax, g.ay, i, j, level, ylo, yhi, xlo, xhi);
}

// kind 1: the range grows to an even length, so that the two parities of an axis have the same number of class rows
SBBSEG_HD inline void region_even(int& lo, int& hi, int R)
{
    if ((hi - lo) & 1) {
        if (hi < R) ++hi; else --lo;
    }
}
// kind 0: 16-pixel tiles from `lo` rounded down to `align`: their number, and the origin of tile k (the last one is pulled inside the tensor)
SBBSEG_HD inline int region_tiles16(int lo, int hi, int align) { return hi > lo ? (hi - (lo & ~(align - 1)) + 15) >> 4 : 0; }
SBBSEG_HD inline int region_tile_origin(int lo, int align, int k, int R)
{
    const int o = (lo & ~(align - 1)) + 16 * k;
    return o + 16 > R ? R - 16 : o;
}

// table entries of patch (i, j) at `level`: kind 0 = tiles, kind 1 = pixels PER CLASS
SBBSEG_HD inline int region_entries(const RegionGeom& g, const RegionAxis& ax, const RegionAxis& ay, int i, int j, int level)
{
    int ylo, yhi, xlo, xhi;
    region_needed(g, ax, ay, i, j, level, ylo, yhi, xlo, xhi);
    if (yhi <= ylo) return 0;
    if (g.kind[level] == 0) return region_tiles16(ylo, yhi, 2) * region_tiles16(xlo, xhi, g.align_x[level]);
    region_even(ylo, yhi, g.Rh[level]);
    region_even(xlo, xhi, g.Rw[level]);
    return ((yhi - ylo) >> 1) * ((xhi - xlo) >> 1);
}
SBBSEG_HD inline int region_entries(const RegionGeom& g, int i, int j, int level) { return region_entries(g, g.ax, g.ay, i, j, level); }

// table entry: patch (10 bits) | y (11 bits) | x (11 bits).  kind 0: tile origin / 2; kind 1: class-grid pixel
SBBSEG_HD inline uint32_t region_code(int n, int y, int x) { return ((uint32_t)n << 22) | ((uint32_t)y << 11) | (uint32_t)x; }
SBBSEG_HD inline int region_code_n(uint32_t c) { return (int)(c >> 22); }
SBBSEG_HD inline int region_code_y(uint32_t c) { return (int)((c >> 11) & 2047u); }
SBBSEG_HD inline int region_code_x(uint32_t c) { return (int)(c & 2047u); }
constexpr int kRegionMaxPatches = 1023, kRegionMaxCoord = 2047;

// device tables of one launch chunk: patch p of the chunk is tile g0 + p of the pooled tile list (page-major, grid index = tile % tpp)
struct RegionBuildParams {
    RegionGeom g;
    int g0, nb;
    uint32_t* out[kRegionMaxLevels];      // kind 0: [entries]; kind 1: [4 classes][entries] (class q = parity (q >> 1, q & 1))
    int total[kRegionMaxLevels];          // entries (per class) of the whole chunk, as the host counted them
};
hipError_t launch_region_build(const RegionBuildParams& p, hipStream_t s);

// One view of sbbseg_segment_views_dev, as the device sees it: a crop cw x ch of a (virtually upscaled) stored page with its own tile grid.
// The views of a GROUP pool their tiles into one list, view-major; within a view tile i * ny + j as everywhere (x outer, y inner).
struct ViewRec {
    const uint8_t* page;          // stored page [Hs][Ws][3]
    uint8_t* labels;              // [ch][cw] out
    const int* thr;               // binarised view: its Otsu threshold (device int); else null
    int src_Wp;                   // Ws
    int cw, ch;                   // the page the tile grid lives on
    int nx, ny;                   // tiles per axis, after the dedupe rule
    int first, n_tiles;           // first pooled tile of the view in its group; nx * ny
    int mapped;                   // 1: crop row r reads stored row maps[my + r] (column alike); 0: stored row my + r (no rescale: my = cy, mx = cx)
    int my, mx;
    unsigned blk_first;           // stitch: first 256-pixel block of the view's plane among its group's (every plane starts a new block)
};
SBBSEG_HD inline RegionAxis view_axis_x(const ViewRec& v, int tile, int margin) { return {v.cw, tile, margin, tile - 2 * margin, v.nx}; }
SBBSEG_HD inline RegionAxis view_axis_y(const ViewRec& v, int tile, int margin) { return {v.ch, tile, margin, tile - 2 * margin, v.ny}; }
// index of the view that holds element `key` of a prefix taken from the views (first pooled tile, first stitch block): the last v with prefix(v) <= key
template <typename F>
SBBSEG_HD inline int view_find(int n_views, unsigned key, F prefix)
{
    int lo = 0, hi = n_views - 1;
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (prefix(m) <= key) lo = m; else hi = m - 1;
    }
    return lo;
}

// the tables of a chunk whose patches come from several views: patch p is pooled tile g0 + p of the group; g.ax / g.ay / g.tpp / g.ny are not read
struct RegionViewsBuildParams {
    RegionGeom g;
    const ViewRec* views;
    int n_views, g0, nb, tile_h, tile_w, margin;
    uint32_t* out[kRegionMaxLevels];
    int total[kRegionMaxLevels];
};
hipError_t launch_region_build_views(const RegionViewsBuildParams& p, hipStream_t s);

}  // namespace sbbseg
