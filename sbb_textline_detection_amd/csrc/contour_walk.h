// contour_walk.h -- the outer border of ONE 8-connected component as cv2.findContours(..., CHAIN_APPROX_SIMPLE) lists it [EXT, restated
// from OpenCV's border follower, unpinned like the rest of cv2], as plain integer C++ for host and device code.  contours.hip runs it on a
// bit map in LDS or on the label plane; sbbseg_mask_contours_host runs it on the host's label plane.  Integer topology only: the three
// callers give the same points, the same doubled area and the same box, bit for bit.
//
// The walk.  The start pixel is the component's first pixel in raster order (its W, NW, N and NE neighbours are background).  Its
// PREDECESSOR is the first component pixel of a CLOCKWISE search of its neighbours that begins after the west one; a start pixel without
// one is a one-point contour.  From then on the next pixel is the first component pixel of a COUNTER-CLOCKWISE search (on the screen, y
// pointing down) that begins after the pixel the walk came from.  The walk ends when the start pixel is entered from the predecessor
// again.  A point is KEPT when the step that leaves it differs from the step that entered it (the start pixel: entered from the
// predecessor).  The doubled shoelace sum runs over every step, kept or not: dropping collinear points does not change it.
//
// Bounds.  A (pixel, leaving direction) pair occurs at most once, so a walk over a component whose box holds `box_pixels` pixels takes at
// most 8 * box_pixels steps; contour_step_bound adds 8.  A walk that reaches the bound, or that finds no neighbour where one must be,
// ends with a status: a damaged label plane cannot spin the walker.
#ifndef SBBSEG_CONTOUR_WALK_H
#define SBBSEG_CONTOUR_WALK_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBB_CW_HD __host__ __device__ __forceinline__
#else
#define SBB_CW_HD inline
#endif

namespace sbbseg {

constexpr int kContourLdsBytes = 64 * 1024;         // largest bit map (box + ring) the LDS form of the tracer takes: 524 288 pixels
constexpr int kContourStage = 64;                   // kept points staged in LDS before the wave stores them
enum { kContourOk = 0, kContourStepBound = 1, kContourBroken = 2, kContourBadBox = 3 };

// direction d: E, SE, S, SW, W, NW, N, NE -- clockwise on the screen; d + 1 turns clockwise, d - 1 counter-clockwise
// (two tiny tables kept in a register each: 2 bits per direction, step + 1)
SBB_CW_HD int contour_step_x(int d) { return (int)((0x901au >> (2 * d)) & 3u) - 1; }      // 1, 1, 0, -1, -1, -1, 0, 1
SBB_CW_HD int contour_step_y(int d) { return (int)((0x01a9u >> (2 * d)) & 3u) - 1; }      // 0, 1, 1, 1, 0, -1, -1, -1

SBB_CW_HD long long contour_step_bound(long long box_pixels) { return 8 * box_pixels + 8; }

// row stride in 32-bit words and bytes of the bit map of a w x h box with its one-pixel ring (one spare word behind the last row: a
// three-bit field that ends a row is read as two words)
SBB_CW_HD int contour_bitmap_stride(int w) { return (w + 2 + 31) >> 5; }
SBB_CW_HD long long contour_bitmap_bytes(int w, int h) { return ((long long)contour_bitmap_stride(w) * (h + 2) + 1) * 4; }

// which form of the tracer takes a candidate {root, box}: decided the same way by the host (which launches) and the device (which skips)
enum { kContourFormLds = 0, kContourFormGlobal = 1, kContourFormBad = 2 };
SBB_CW_HD int contour_form(int root, int x0, int y0, int x1, int y1, int H, int W, int lds_limit)
{
    if (x0 < 0 || y0 < 0 || x1 >= W || y1 >= H || x1 < x0 || y1 < y0 || root < 0 || (long long)root >= (long long)H * W) return kContourFormBad;
    const int sx = root % W, sy = root / W;
    if (sx < x0 || sx > x1 || sy < y0 || sy > y1) return kContourFormBad;
    return contour_bitmap_bytes(x1 - x0 + 1, y1 - y0 + 1) <= lds_limit ? kContourFormLds : kContourFormGlobal;
}

struct ContourResult {
    long long area2;          // |doubled shoelace sum| of the closed chain
    long long steps;          // chain length (CHAIN_APPROX_NONE points)
    int n_points;             // kept points (CHAIN_APPROX_SIMPLE)
    int status;
    int x0, y0, x1, y1;       // extent of the chain = of the component
};

// nb(x, y): bit d set <=> the neighbour of (x, y) in direction d belongs to the component.  emit(k, x, y): kept point k.
//
// contour_walk_from is the same walk with two more parameters, for the callers that follow EVERY border of a mask (line_extent.h):
//   * first: the direction after which the clockwise search for the predecessor begins -- 4 (west) for an outer border, 0 (east) for the
//     border of a hole, whose start pixel is the pixel WEST of the hole's first background pixel;
//   * mark(x, y, right): called once per step with the pixel the step leaves; right = the pixel's east neighbour was examined during this
//     step's search and was background (OpenCV writes -nbd there, nbd otherwise).  A one-pixel border is marked right.
// contour_walk is contour_walk_from(first = 4, no marks): the outer-border callers' results do not change.
struct ContourNoMark {
    SBB_CW_HD void operator()(int, int, bool) const {}
};

template <typename Nb, typename Emit, typename Mark>
SBB_CW_HD ContourResult contour_walk_from(Nb nb, int sx, int sy, int first, long long max_steps, Emit emit, Mark mark)
{
    ContourResult r;
    r.area2 = 0; r.steps = 1; r.n_points = 0; r.status = kContourOk;
    r.x0 = r.x1 = sx; r.y0 = r.y1 = sy;
    unsigned m = nb(sx, sy);
    m = (((m | (m << 8)) >> first) & 0xfeu);                 // bit j = the neighbour in direction first + j: clockwise from `first`, itself left out
    if (!m) {                                                // a one-pixel component
        emit(0, sx, sy);
        mark(sx, sy, true);
        r.n_points = 1;
        return r;
    }
    const int to_pred = (first + __builtin_ctz(m)) & 7;          // from the start pixel to its predecessor
    const int px = sx + contour_step_x(to_pred), py = sy + contour_step_y(to_pred);
    int cx = sx, cy = sy, back = to_pred, entered = to_pred ^ 4;
    long long sum = 0, steps = 0;
    for (;;) {
        if (steps >= max_steps) { r.status = kContourStepBound; break; }
        m = nb(cx, cy);
        m = ((m | (m << 8)) >> back) & 0xffu;                // bit j = direction back + j; counter-clockwise from `back`: j = 7, 6, ..., 0
        if (!m) { r.status = kContourBroken; break; }        // (the pixel the walk came from has gone: the plane is damaged)
        const int found = 31 - __builtin_clz(m);
        const int d = (back + found) & 7;
        mark(cx, cy, ((8 - back) & 7) > found);              // east = direction back + ((8 - back) & 7): examined iff that offset lies above `found`
        if (d != entered) { emit(r.n_points, cx, cy); ++r.n_points; }
        const int nx = cx + contour_step_x(d), ny = cy + contour_step_y(d);
        sum += (long long)cx * ny - (long long)nx * cy;
        ++steps;
        const bool closed = nx == sx && ny == sy && cx == px && cy == py;
        cx = nx; cy = ny;
        if (closed) break;
        r.x0 = cx < r.x0 ? cx : r.x0; r.x1 = cx > r.x1 ? cx : r.x1;
        r.y0 = cy < r.y0 ? cy : r.y0; r.y1 = cy > r.y1 ? cy : r.y1;
        entered = d;
        back = d ^ 4;
    }
    r.area2 = sum < 0 ? -sum : sum;
    r.steps = steps;
    return r;
}

template <typename Nb, typename Emit>
SBB_CW_HD ContourResult contour_walk(Nb nb, int sx, int sy, long long max_steps, Emit emit)
{
    return contour_walk_from(nb, sx, sy, 4, max_steps, emit, ContourNoMark{});
}

}  // namespace sbbseg

#endif
