// line_extent.h -- the x extent of every text line of ONE region from the region's filled, rotated contour: the contour half of
// textline_contours_postprocessing (main.py:1492-1511) and its only consumer, cv2.pointPolygonTest inside seperate_lines (main.py:780-791,
// 878-889, 945-956), as plain integer / float64 C++ for host and device code.  line_extent.hip deals these statements out to waves,
// sbbseg_region_line_extents_host runs them serially.  Every cv2 rule below is [EXT]: restated from the OpenCV 4.5.1 text, unpinned (there
// is no cv2 to hold it against); each is reduced to integer predicates so that "bit for bit" is checkable, and tests/line_extent_ref.py
// restates each one independently in Python.
//
// R1 fill (cv2.fillPoly, colour 255, on zeros).  Scope: rings whose edges between consecutive points -- the closing edge from the last point
//   to the first included; a repeated closing point is a zero-length edge -- are horizontal, vertical or exact diagonals, and whose points
//   lie in [0, w) x [0, h) after the box origin is subtracted: what CHAIN_APPROX_SIMPLE lists of a traced border are.  Anything else is
//   kExtentBadRing.  For such edges cv2's drawn outline is exactly the lattice points of the segment, and a pixel is set when it lies on an
//   edge or when the number of edges crossing its row strictly left of it is odd (an edge crosses row py when min(y0, y1) <= py <
//   max(y0, y1), at the integer x0 + (py - y0) * sign(dx) * sign(dy)).  Row by row: extent_edge_row gives the edge's pixels and its crossing
//   on a row; the row is edges | prefix-xor(crossings).  (Inclusive or exclusive prefix: they differ only AT a crossing, an edge pixel.)
//
// R2 rotate (rotate_image on float64: getRotationMatrix2D((w // 2, h // 2), slope, 1.0), warpAffine(INTER_CUBIC, BORDER_REPLICATE), the
//   FLOAT path).  Source coordinates and the 5-bit table indices are line_mask.h's (the same matrix and inverse map per box as the line
//   masks).  The 2-D weight of tap (r, c) is the float32 product tab[ay][r] * tab[ax][c]; all 32 x 32 x 16 of them are multiples of 2^-34
//   (extent_weight_table verifies it while building, a CPU test enumerates it), and with a 0 / 255 source 255 * sum |weights| < 483, so
//   every partial sum is exact in float64 whatever the order of the taps: v = 255 * S / 2^34 with the integer S = sum of weight * 2^34
//   over the taps that fall on set pixels.
//
// R3 cast and threshold (.astype(np.uint8), BGR2GRAY of three equal channels, threshold(., 0, 255, 0)).  numpy's float64 -> uint8 cast on
//   x86-64 truncates toward zero and keeps the low 8 bits: a pixel of threshrot is set iff (trunc(v) & 255) != 0.  With v in [-113.6, 368.6]:
//   not set for |v| < 1 and for 256 <= v < 257; the ring of negative overshoot outside the outline IS set.
//
// R4 borders (cv2.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE), then np.argmax of the point counts).  The image is treated as padded by one
//   pixel of zeros; the raster scan visits the real pixels only.  At position x of a row, with p the pixel there and q its west neighbour
//   (marks as they are at that moment):
//     * p unmarked and set, q background: an OUTER border starts at x; its first search goes clockwise from west;
//     * p background, q set and not marked "right": a HOLE border starts at x - 1; its first search goes clockwise from east;
//   after the start the walk is contour_walk.h's.  A step marks the pixel it leaves "right" when that pixel's east neighbour was examined as
//   background during the step's search, "visited" otherwise; a one-pixel border is marked right.  ALL borders compete.  The count is the
//   number of kept points; among equal counts the list order decides, which is assumed to be reverse discovery order as everywhere else in
//   the project [EXT, unpinned]: the LAST discovered of the maxima wins, and `tie` says there was more than one.  No border: np.argmax([])
//   raises and the function's bare except returns [] -- kExtentNone.
//
// R5 inside test (horizontal splitter only).  xv = np.linspace(0, w, 1000): k * (w / 999) in float64, the last sample exactly w.  Sample k
//   of a line is inside iff cv2.pointPolygonTest(winner, (float32(xv[k]), float32(peak)), True) >= 0, i.e. iff some edge's dist_num is 0 or
//   the crossing counter is odd (-0.0 >= 0 holds).  dx1 = pt.x - v0.x and dx2 = pt.x - v.x are FLOAT32 subtractions; everything after them
//   is float64 and only signs and zero tests of sums of two exact products are used, which no rounding, contraction or evaluation order can
//   change.  x_min = int(min xv inside), x_max = int(max xv inside) truncate the float64 xv; no sample inside: 0 and w.
//
// R6 corners: line_box_with_extent (line_split.h) for branches 0, 3, 4 of the horizontal splitter; branch 2 keeps 0 .. w; the vertical
//   splitter never uses the extent.
#ifndef SBBSEG_LINE_EXTENT_H
#define SBBSEG_LINE_EXTENT_H

#include "contour_walk.h"
#include "line_mask.h"

#define SBB_LE_HD SBB_CW_HD

namespace sbbseg {

constexpr int kExtentSamples = 1000;                // np.linspace(0, w, 1000)
constexpr int kExtentTabEntries = 32 * 32 * 16;     // int64 [ay][ax][r][c]: weight * 2^34
constexpr int kExtentWeightShift = 34;
constexpr int kExtentRows = 8;                      // rows of a work item of the fill and warp kernels
// Largest sum of the THREE bit maps (pixels, visited, right; box + ring each) the LDS form of the border scan takes; larger regions scan on
// a workspace in global memory.  Chosen, not measured.
constexpr int kExtentLdsBytes = 60 * 1024;
enum { kExtentOk = 0, kExtentNone = 1, kExtentBadRing = 2, kExtentBroken = 3 };
// the record of a region: status, borders found (outer + hole), the winner's kept points, 1 = the winner is a hole border, 1 = more than
// one border had that many points, the winner's start pixel, hole borders found
enum { kExtentRecStatus = 0, kExtentRecBorders = 1, kExtentRecPoints = 2, kExtentRecHole = 3, kExtentRecTie = 4, kExtentRecStartX = 5,
       kExtentRecStartY = 6, kExtentRecHoles = 7, kExtentRecInts = 8 };

SBB_LE_HD int extent_src_stride(int w) { return (w + 31) >> 5; }      // the filled source: no ring, taps are clamped

// ---- R1
SBB_LE_HD bool extent_edge_ok(int x0, int y0, int x1, int y1, int w, int h)
{
    const int dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
    return x0 >= 0 && x0 < w && x1 >= 0 && x1 < w && y0 >= 0 && y0 < h && y1 >= 0 && y1 < h && (dx == 0 || dy == 0 || dx == dy);
}

struct ExtentEdgeRow {
    int lo, hi;               // the edge's pixels on the row: columns lo .. hi (lo > hi: none)
    int cross;                // the column at which the edge crosses the row, or -1
};
SBB_LE_HD ExtentEdgeRow extent_edge_row(int x0, int y0, int x1, int y1, int py)
{
    ExtentEdgeRow e;
    e.lo = 0; e.hi = -1; e.cross = -1;
    if (y0 == y1) {
        if (y0 == py) { e.lo = x0 < x1 ? x0 : x1; e.hi = x0 < x1 ? x1 : x0; }
        return e;
    }
    const int ylo = y0 < y1 ? y0 : y1, yhi = y0 < y1 ? y1 : y0;
    if (py < ylo || py > yhi) return e;
    const int sx = (x1 > x0) - (x1 < x0), sy = y1 > y0 ? 1 : -1;
    e.lo = e.hi = x0 + (py - y0) * sx * sy;
    if (py < yhi) e.cross = e.lo;
    return e;
}

// bits lo .. hi (clipped to 0 .. 31) of the word that holds columns c0 .. c0 + 31
SBB_LE_HD uint32_t extent_span_bits(int lo, int hi, int c0)
{
    lo -= c0; hi -= c0;
    if (hi < 0 || lo > 31 || lo > hi) return 0u;
    lo = lo < 0 ? 0 : lo; hi = hi > 31 ? 31 : hi;
    return (hi == 31 ? ~0u : ((2u << hi) - 1u)) & ~((1u << lo) - 1u);
}

// inclusive prefix xor over the bits of a word, bit 0 first
SBB_LE_HD uint32_t extent_prefix_xor(uint32_t t)
{
    t ^= t << 1; t ^= t << 2; t ^= t << 4; t ^= t << 8; t ^= t << 16;
    return t;
}

// one region, serially: pts = n ring points in page coordinates, (ox, oy) the box origin; src = h rows of extent_src_stride(w) words.
// false: a bad ring (nothing useful is written)
inline bool extent_fill_serial(const int32_t* pts, int n, int ox, int oy, int w, int h, uint32_t* src)
{
    const int stride = extent_src_stride(w);
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        if (!extent_edge_ok(pts[2 * i] - ox, pts[2 * i + 1] - oy, pts[2 * j] - ox, pts[2 * j + 1] - oy, w, h)) return false;
    }
    for (int py = 0; py < h; ++py) {
        uint32_t carry = 0;
        for (int wi = 0; wi < stride; ++wi) {
            uint32_t edge = 0, toggles = 0;
            for (int i = 0; i < n; ++i) {
                const int j = i + 1 < n ? i + 1 : 0;
                const ExtentEdgeRow e = extent_edge_row(pts[2 * i] - ox, pts[2 * i + 1] - oy, pts[2 * j] - ox, pts[2 * j + 1] - oy, py);
                edge |= extent_span_bits(e.lo, e.hi, 32 * wi);
                if (e.cross >= 0) toggles ^= extent_span_bits(e.cross, e.cross, 32 * wi);
            }
            const uint32_t par = extent_prefix_xor(toggles) ^ carry;
            carry = (par >> 31) ? ~0u : 0u;
            src[(size_t)py * stride + wi] = (edge | par) & extent_span_bits(0, w - 1, 32 * wi);
        }
    }
    return true;
}

// ---- R2 / R3
// the int64 table from the float bicubic table [32][4]; false: a weight is no multiple of 2^-34 (the step's premise does not hold)
inline bool extent_weight_table(const float* tab, int64_t* wtab)
{
#pragma clang fp contract(off)
    bool exact = true;
    for (int ay = 0; ay < 32; ++ay)
        for (int ax = 0; ax < 32; ++ax)
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) {
                    const float v = tab[ay * 4 + r] * tab[ax * 4 + c];
                    const double s = (double)v * 17179869184.0;         // 2^34: exact
                    const long long q = (long long)s;
                    exact = exact && (double)q == s;
                    wtab[(((size_t)ay * 32 + ax) << 4) + r * 4 + c] = q;
                }
    return exact;
}

SBB_LE_HD bool extent_threshold(long long S)
{
    const long long T = (255 * S) / (1ll << kExtentWeightShift);        // trunc(v): C++ integer division truncates toward zero
    return (T & 255) != 0;
}

// pixel x of destination row (X0, Y0) of threshrot; src: the filled h x w bit map
SBB_LE_HD bool extent_pixel(const uint32_t* src, int w, int h, double m0, double m3, long long X0, long long Y0, int x, const int64_t* wtab)
{
#pragma clang fp contract(off)
    const long long X = (X0 + llrint(m0 * (double)x * 1024.0)) >> 5;
    const long long Y = (Y0 + llrint(m3 * (double)x * 1024.0)) >> 5;
    long long sxl = X >> 5, syl = Y >> 5;
    sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl);
    syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
    const int sx = (int)sxl, sy = (int)syl, stride = extent_src_stride(w);
    const int64_t* wt = wtab + ((((int)(Y & 31) << 5) + (int)(X & 31)) << 4);
    int xs[4];
    for (int c = 0; c < 4; ++c) {
        const int xx = sx - 1 + c;
        xs[c] = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
    }
    long long S = 0;
    for (int r = 0; r < 4; ++r) {
        int yy = sy - 1 + r;
        yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
        const uint32_t* row = src + (size_t)yy * stride;
        for (int c = 0; c < 4; ++c)
            if ((row[xs[c] >> 5] >> (xs[c] & 31)) & 1u) S += wt[r * 4 + c];
    }
    return extent_threshold(S);
}

// ---- R4: threshrot and the two mark planes as bit maps of the box with its one-pixel ring (contour_bitmap_stride / _bytes): pixel (x, y)
// is bit (x + 1) & 31 of word (y + 1) * stride + ((x + 1) >> 5)
struct ExtentMap {
    const uint32_t* pix;
    uint32_t* vis;
    uint32_t* right;
    int stride, w, h;
};

struct ExtentNb {
    const uint32_t* bits;
    int stride;
    SBB_LE_HD unsigned three(const uint32_t* p, int sh) const
    {
        return (unsigned)((((unsigned long long)p[1] << 32) | p[0]) >> sh) & 7u;      // columns x - 1, x, x + 1
    }
    SBB_LE_HD unsigned operator()(int x, int y) const
    {
        const uint32_t* p = bits + y * stride + (x >> 5);                               // the field's first column, the row above
        const int sh = x & 31;
        const unsigned a = three(p, sh), b = three(p + stride, sh), c = three(p + 2 * stride, sh);
        // E, SE, S, SW, W, NW, N, NE
        return ((b >> 2) & 1u) | (((c >> 2) & 1u) << 1) | (((c >> 1) & 1u) << 2) | ((c & 1u) << 3) | ((b & 1u) << 4) | ((a & 1u) << 5) |
               (((a >> 1) & 1u) << 6) | (((a >> 2) & 1u) << 7);
    }
};

struct ExtentMark {
    uint32_t* vis;
    uint32_t* right;
    int stride;
    SBB_LE_HD void operator()(int x, int y, bool r) const
    {
        uint32_t* p = (r ? right : vis) + (y + 1) * stride + ((x + 1) >> 5);
        *p |= 1u << ((x + 1) & 31);
    }
};

struct ExtentNoEmit {
    SBB_LE_HD void operator()(int, int, int) const {}
};

// the scan positions of word wi of row y at which a border starts, as the marks stand now (bit b = bit-map column 32 wi + b = pixel
// column 32 wi + b - 1; an outer border starts AT the position, a hole border at the pixel west of it)
SBB_LE_HD uint32_t extent_events(const ExtentMap& m, int y, int wi)
{
    const int at = (y + 1) * m.stride + wi;
    const uint32_t P = m.pix[at], R = m.right[at], V = m.vis[at];
    const uint32_t Pp = wi ? m.pix[at - 1] : 0u, Rp = wi ? m.right[at - 1] : 0u;
    const uint32_t Pw = (P << 1) | (Pp >> 31), Rw = (R << 1) | (Rp >> 31);
    const uint32_t E = (P & ~Pw & ~V & ~R) | (~P & Pw & ~Rw);
    return E & extent_span_bits(1, m.w, 32 * wi);                   // the real pixels: bit-map columns 1 .. w
}

struct ExtentWinner {
    int status, borders, holes, n_points, is_hole, tie, sx, sy;
};

// Every border of the map in OpenCV's discovery order; the marks must be zero on entry.  next_word(y, from): the first word >= from of
// row y whose extent_events is not zero, or m.stride -- the serial form tries every word, a wave looks at 64 words at a time.
template <typename NextWord>
SBB_LE_HD ExtentWinner extent_scan(const ExtentMap& m, NextWord next_word)
{
    ExtentWinner win;
    win.status = kExtentNone; win.borders = 0; win.holes = 0; win.n_points = 0; win.is_hole = 0; win.tie = 0; win.sx = 0; win.sy = 0;
    const long long bound = contour_step_bound((long long)m.w * m.h);
    const ExtentNb nb{m.pix, m.stride};
    const ExtentMark mark{m.vis, m.right, m.stride};
    for (int y = 0; y < m.h; ++y)
        for (int wi = next_word(y, 0); wi < m.stride; wi = next_word(y, wi + 1)) {
            uint32_t done = 0;                                      // positions of this word the scan has passed
            for (;;) {
                const uint32_t E = extent_events(m, y, wi) & ~done;
                if (!E) break;
                const int b = __builtin_ctz(E);
                done |= (2u << b) - 1u;
                const int hole = ((m.pix[(y + 1) * m.stride + wi] >> b) & 1u) ? 0 : 1;
                const int sx = 32 * wi + b - 1 - hole;
                const ContourResult r = contour_walk_from(nb, sx, y, hole ? 0 : 4, bound, ExtentNoEmit{}, mark);
                if (r.status != kContourOk) { win.status = kExtentBroken; return win; }
                ++win.borders;
                win.holes += hole;
                if (r.n_points >= win.n_points) {                   // the last discovered of the maxima
                    win.tie = r.n_points == win.n_points && win.borders > 1 ? 1 : 0;
                    win.n_points = r.n_points; win.is_hole = hole; win.sx = sx; win.sy = y;
                }
            }
        }
    if (win.borders) win.status = kExtentOk;
    return win;
}

struct ExtentSerialNext {
    const ExtentMap* m;
    int operator()(int y, int from) const
    {
        while (from < m->stride && !extent_events(*m, y, from)) ++from;
        return from;
    }
};

// ---- R5
SBB_LE_HD double extent_sample(int k, double step, int w) { return k == kExtentSamples - 1 ? (double)w : (double)k * step; }

// cv2.pointPolygonTest(pts, (ptx, pty), True) >= 0 for int points
SBB_LE_HD bool extent_inside(const int32_t* pts, int n, float ptx, float pty)
{
#pragma clang fp contract(off)
    if (n <= 0) return false;
    int counter = 0;
    float vx = (float)pts[2 * (size_t)(n - 1)], vy = (float)pts[2 * (size_t)(n - 1) + 1];
    for (int i = 0; i < n; ++i) {
        const float v0x = vx, v0y = vy;
        vx = (float)pts[2 * (size_t)i]; vy = (float)pts[2 * (size_t)i + 1];
        const double dx = (double)(vx - v0x), dy = (double)(vy - v0y);
        const double dx1 = (double)(ptx - v0x), dy1 = (double)(pty - v0y), dx2 = (double)(ptx - vx), dy2 = (double)(pty - vy);
        double dist_num;
        if (dx1 * dx + dy1 * dy <= 0) dist_num = dx1 * dx1 + dy1 * dy1;
        else if (dx2 * dx + dy2 * dy >= 0) dist_num = dx2 * dx2 + dy2 * dy2;
        else { dist_num = dy1 * dx - dx1 * dy; dist_num *= dist_num; }
        if (dist_num == 0) return true;                             // the minimum becomes 0 and the loop ends: +-0.0 >= 0
        if ((v0y <= pty && vy <= pty) || (v0y > pty && vy > pty)) continue;
        double side = dy1 * dx - dx1 * dy;
        if (dy < 0) side = -side;
        counter += side > 0 ? 1 : 0;
    }
    return (counter & 1) != 0;
}

// one line, serially: the first and last inside sample as x_min / x_max, or 0 / w
inline void extent_line_serial(const int32_t* pts, int n, int w, int peak, int32_t* extent)
{
    const double step = (double)w / (double)(kExtentSamples - 1);
    int kmin = -1, kmax = -1;
    for (int k = 0; k < kExtentSamples; ++k)
        if (extent_inside(pts, n, (float)extent_sample(k, step, w), (float)peak)) { kmin = kmin < 0 ? k : kmin; kmax = k; }
    extent[0] = kmin < 0 ? 0 : (int)extent_sample(kmin, step, w);
    extent[1] = kmin < 0 ? w : (int)extent_sample(kmax, step, w);
}

}  // namespace sbbseg

#endif  // SBBSEG_LINE_EXTENT_H
