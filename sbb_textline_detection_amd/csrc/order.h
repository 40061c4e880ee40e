// order.h -- the reading order of the text regions of ONE page: everything order_of_regions (main.py:1802-1889) computes from the row sums of
// the textline plane and the region contours, as plain float64 C++ for host and device code.  moments_serial(), order_edges_serial() and order_rank_serial() are what the
// CPU entry points run; order.hip deals the same pieces out to waves and blocks.  Built on profile_stat.h and held to the same rule: every float64 result is
// scipy's / numpy's bit for bit (no FMA contraction, soft_div), so find_peaks' exact comparisons and the band tests decide the same.
//
//   * band edges: [0] + (find_peaks(gaussian_filter1d(zneg, 8), height=0) - 40) + [H], zneg = the array `b` of seperate_lines
//     (line_split.h: FlippedSamplesP with pad 20).  Edges below 0 and at or above H occur and are NOT clamped.  peaks_real, z and peaks
//     (main.py:1811, 1816, 1824) are read by nothing: dead and non-raising, not computed.
//   * moments: OpenCV's contourMoments for integer points [EXT, restated, unpinned: cv2 is not installable] -- float64, serial, starting
//     from the last point, every multiply and add rounded on its own.
//   * order: per pair of consecutive edges [top, down), in edge order, the regions with top <= cy < down by ascending cx; ties [EXT:
//     np.argsort's default sort is unstable] by ascending region index.  Edges are 0, an ascending run, H: the bands are disjoint, so a
//     region lies in at most one -- exactly one whenever 0 <= cy < H.  A region in none (band -1) is left out of the list, as the
//     reference's masks leave it out.
#ifndef SBBSEG_ORDER_H
#define SBBSEG_ORDER_H

#include "profile_stat.h"

namespace sbbseg {

constexpr int kOrderPad = 20;                       // zeros either side of y, and again either side of max - padded (main.py:1806-1820)
constexpr int kOrderSigma = 8;                      // main.py:1814
constexpr int kOrderRadius = 4 * kOrderSigma;       // scipy's truncate = 4: 33 weights
constexpr int kOrderCoordLimit = 32768;             // |x|, |y| below this: every term of the moment sums is an exact integer below 2^47
constexpr long long kOrderExactLimit = 1ll << 53;   // an integer prefix below this in magnitude is the float64 prefix

// find_peaks gives at most (H + 80 - 1) / 2 maxima of the H + 80 samples; 0 in front and H behind them
SBB_HD constexpr int order_edge_capacity(int H) { return (H + 4 * kOrderPad) / 2 + 2; }

struct OrderMoments {
    double m00, m10, m01, cx, cy;
};

// one step of contourMoments' loop: (xp, yp) the point before (x, y)
SBB_HD void moments_step(double xp, double yp, double x, double y, double* a00, double* a10, double* a01)
{
#pragma clang fp contract(off)
    const double p = xp * y, q = x * yp;
    const double dxy = p - q;
    const double sx = xp + x, sy = yp + y;
    const double tx = dxy * sx, ty = dxy * sy;
    *a00 = *a00 + dxy;
    *a10 = *a10 + tx;
    *a01 = *a01 + ty;
}

// the same step's three terms as integers (exact for coordinates below kOrderCoordLimit in magnitude)
SBB_HD void moments_terms(int xp, int yp, int x, int y, long long* d, long long* tx, long long* ty)
{
    const long long dxy = (long long)xp * y - (long long)x * yp;
    *d = dxy;
    *tx = dxy * ((long long)xp + x);
    *ty = dxy * ((long long)yp + y);
}

SBB_HD bool order_coord_small(int v) { return v > -kOrderCoordLimit && v < kOrderCoordLimit; }
SBB_HD bool order_prefix_exact(long long v) { return v > -kOrderExactLimit && v < kOrderExactLimit; }

// cv::moments' completion for a contour (fabs(a00) > FLT_EPSILON, the sign of a00 folded into the two factors) and the centroid of
// main.py:1835-1836
SBB_HD OrderMoments moments_finish(double a00, double a10, double a01)
{
#pragma clang fp contract(off)
    OrderMoments m;
    m.m00 = 0.0; m.m10 = 0.0; m.m01 = 0.0;
    const double mag = a00 < 0.0 ? -a00 : a00;
    if (mag > 1.1920928955078125e-07) {
        const double half = a00 > 0.0 ? 0.5 : -0.5, sixth = a00 > 0.0 ? 0.16666666666666666 : -0.16666666666666666;
        m.m00 = a00 * half;
        m.m10 = a10 * sixth;
        m.m01 = a01 * sixth;
    }
    const double den = m.m00 + 1e-32;
    m.cx = soft_div(m.m10, den);
    m.cy = soft_div(m.m01, den);
    return m;
}

// The literal loop over the n points pts[0 .. n) (x, y interleaved).  *exact (optional): every coordinate is small and every prefix of the
// three integer sums stays below 2^53 -- the case in which the integer sums ARE these float64 sums (what the device's wave scan relies on).
SBB_HD OrderMoments moments_serial(const int32_t* pts, long long n, bool* exact)
{
    double a00 = 0.0, a10 = 0.0, a01 = 0.0;
    long long i00 = 0, i10 = 0, i01 = 0;
    bool ok = true;
    if (n > 0) {
        int xp = pts[2 * (n - 1)], yp = pts[2 * (n - 1) + 1];
        for (long long i = 0; i < n; ++i) {
            const int x = pts[2 * i], y = pts[2 * i + 1];
            moments_step((double)xp, (double)yp, (double)x, (double)y, &a00, &a10, &a01);
            if (exact && ok) {
                ok = order_coord_small(x) && order_coord_small(y) && order_coord_small(xp) && order_coord_small(yp);
                if (ok) {
                    long long d, tx, ty;
                    moments_terms(xp, yp, x, y, &d, &tx, &ty);
                    i00 += d; i10 += tx; i01 += ty;
                    ok = order_prefix_exact(i00) && order_prefix_exact(i10) && order_prefix_exact(i01);
                }
            }
            xp = x; yp = y;
        }
    }
    if (exact) *exact = ok;
    return moments_finish(a00, a10, a01);
}

// the band of a centroid: the first pair of consecutive edges with top <= cy < down, or -1
SBB_HD int order_band(const int32_t* edges, int n_edges, double cy)
{
    for (int i = 0; i + 1 < n_edges; ++i)
        if (cy >= (double)edges[i] && cy < (double)edges[i + 1]) return i;
    return -1;
}

// (band, cx, index) of region a sorts before that of region b; band -1 sorts behind every band
SBB_HD bool order_key_less(int band_a, double cx_a, int a, int band_b, double cx_b, int b)
{
    const unsigned ua = (unsigned)band_a, ub = (unsigned)band_b;
    if (ua != ub) return ua < ub;
    if (cx_a < cx_b) return true;
    if (cx_b < cx_a) return false;
    return a < b;
}

// one sample of the smoothed zneg (H + 80 samples) from the int32 row sums; top = max(0, max(y)).  radius = kOrderRadius (the kernel
// hands it in as a run-time value: a loop the compiler unrolls 32 times keeps every pair in flight, 204 vector registers)
SBB_HD double order_smooth_sample(const int32_t* y, int H, int top, const double* w, int radius, int k)
{
    const FlippedSamplesP fs{y, H, kOrderPad, (double)top};
    return smooth_sample(fs, H + 4 * kOrderPad, w, radius, k);
}

// find_peaks(z, height=0) asked about sample i of z[0 .. n): the edge it gives
template <class Ptr>
SBB_HD bool order_edge_at(Ptr z, int n, int i, int32_t* edge)
{
    int mid;
    if (!peak_starts_at(z, n, i, &mid) || !(z[mid] >= 0.0)) return false;
    *edge = mid - 2 * kOrderPad;
    return true;
}

// The band edges, serially.  z: H + 80 doubles of workspace; edges: order_edge_capacity(H) ints.  Returns their number.
inline int order_edges_serial(const int32_t* y, int H, const double* w, double* z, int32_t* edges)
{
    const int n = H + 4 * kOrderPad;
    int top = 0, ne = 0;
    for (int i = 0; i < H; ++i) top = y[i] > top ? y[i] : top;
    for (int k = 0; k < n; ++k) z[k] = order_smooth_sample(y, H, top, w, kOrderRadius, k);
    edges[ne++] = 0;
    for (int i = 1; i < n - 1; ++i) {
        int32_t e;
        if (order_edge_at(z, n, i, &e)) edges[ne++] = e;
    }
    edges[ne++] = H;
    return ne;
}

// bands and ranks of n regions from their centroids ([n][2] cx, cy), serially: sorted_index[rank] = region, order[region] = rank (-1 for
// a region in no band: those stand behind all others in sorted_index)
inline void order_rank_serial(const int32_t* edges, int n_edges, const double* centroids, int n, int32_t* sorted_index, int32_t* order, int32_t* band)
{
    for (int m = 0; m < n; ++m) band[m] = order_band(edges, n_edges, centroids[2 * m + 1]);
    for (int m = 0; m < n; ++m) {
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += order_key_less(band[j], centroids[2 * j], j, band[m], centroids[2 * m], m) ? 1 : 0;
        sorted_index[rank] = m;
        order[m] = band[m] >= 0 ? rank : -1;
    }
}

}  // namespace sbbseg

#endif  // SBBSEG_ORDER_H
