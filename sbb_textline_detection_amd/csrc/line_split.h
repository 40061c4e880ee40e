// line_split.h -- the text lines of ONE region from the projection of its deskewed mask `dst`: everything seperate_lines (main.py:516-991)
// and seperate_lines_vertical (main.py:993-1457) compute after `img_patch.sum(axis=...)`, as plain float64 C++ for host and device code.
// line_split_serial() is the CPU entry point; line_split.hip deals the same pieces out to the lanes of a wave.  Built on profile_stat.h
// and held to the same rule: every float64 result is scipy's / numpy's bit for bit (no FMA contraction, numpy's pairwise sums,
// soft_div / soft_sqrt), so find_peaks' exact comparisons, the ratio tests and the int() truncations decide the same.
//
// Scope.  The contour the reference passes in enters only through cv2.pointPolygonTest (x_min / x_max of the horizontal splitter; computed
// and never used by the vertical one).  It is not part of this file: every line gets the reference's own fallback extent x_min_cont = 0,
// x_max_cont = w (main.py:786-788, the `len(xvinside) == 0` case); line_extent.h computes x_min / x_max from the region's filled, rotated
// contour and rewrites the corners through line_box_with_extent below.  return_contours_of_image / filter_contours_area_of_image inside the first `try`
// (main.py:608-609) produce values nobody reads; they are treated as dead and non-raising [EXT] unpinned.  point_down_narrow
// (main.py:759-778) is computed by the reference and read by nothing; it is not computed here.
//
// Weights.  The sigma of the second pass is only known after the first, so the caller hands in a table of half kernels
// (scipy's _gaussian_kernel1d(sigma, 0, 4 * sigma)[4 * sigma:]) for sigma = 2 .. sigma_max with a prefix-offset array, and optionally ONE
// further half kernel (`extra`, for `extra_sigma`).  A region whose sigma is in neither gets kLineSigmaTooLarge and its sigma; the caller
// finishes it by calling again with that sigma's kernel as `extra`.  The device gets the table up to kLineSigmaMax only.
#ifndef SBBSEG_LINE_SPLIT_H
#define SBBSEG_LINE_SPLIT_H

#include "profile_stat.h"

namespace sbbseg {

constexpr int kLinePad = 20;                        // zeros either side of y, and again either side of max - padded (main.py:544-556)
constexpr int kLineSigmaMin = 2;                    // the first estimate's sigma (main.py:553)
constexpr int kLineSigmaMax = 128;                  // largest sigma of the device's table: a mean line distance of 731 samples
constexpr int kLineSigmaRaised = 12;                // main.py:615
enum { kLineOk = 0, kLineNoLines = 1, kLineSigmaTooLarge = 2 };
// main.py:744 / 822 / 825 / 864 / 919, in the reference's order; kLineBranchNotReached: the region ended before the branches
enum { kLineBranchBetween = 0, kLineBranchNoPeak = 1, kLineBranchOnePeak = 2, kLineBranchTwoPeaks = 3, kLineBranchOther = 4, kLineBranchNotReached = -1 };
enum { kLineInfoStatus = 0, kLineInfoSigma = 1, kLineInfoRaised = 2, kLineInfoBranch = 3, kLineInfoCount = 4, kLineInfoInts = 5 };

// lines a region of `n` profile samples can have: find_peaks gives at most (n + 40 - 1) / 2 maxima of y_padded_smoothed, and the merged
// list is never longer (every cluster removes at least one peak of its own and adds one)
SBB_HD constexpr int line_capacity(int n) { return (n + 2 * kLinePad) / 2; }
SBB_HD constexpr int line_neg_capacity(int n) { return (n + 4 * kLinePad) / 2; }

struct LineGeom {
    int n;                                          // samples of the profile: h of dst (rows), or w for the vertical splitter (columns)
    int other;                                      // the other extent of dst
    int vertical;                                   // 1: seperate_lines_vertical
    double r00, r01, r10, r11, xd, yd;              // rotation_matrix (main.py:524) and M[0, 2], M[1, 2] (main.py:519-521)
};

struct LineWeights {
    const double* table;                            // half kernels of sigma = kLineSigmaMin .. sigma_max, one after the other
    const int64_t* off;                             // [sigma_max - kLineSigmaMin + 2] first double of each
    int sigma_max;
    const double* extra;                            // or nullptr
    int extra_sigma;
    SBB_HD const double* half(int sigma) const
    {
        if (sigma >= kLineSigmaMin && sigma <= sigma_max) return table + off[sigma - kLineSigmaMin];
        return (extra && sigma == extra_sigma) ? extra : nullptr;
    }
};

// working arrays of one region in one allocation of line_work_bytes(n) bytes (the arrays are addressed from the base on every use: nine
// pointers held at once cost the device more scalar registers than it has)
struct LineWork {
    unsigned char* base;
    int n;
    PairwiseStack* st;
    SBB_HD double* a() const { return (double*)base; }                                          // [n + 40] y_padded_smoothed
    SBB_HD double* b() const { return a() + n + 2 * kLinePad; }                                 // [n + 80] y_padded_up_to_down_padded (smoothed)
    SBB_HD int32_t* peaks() const { return (int32_t*)(b() + n + 4 * kLinePad); }                // [line_capacity] find_peaks(a), positions in a
    SBB_HD int32_t* merged() const { return peaks() + line_capacity(n); }                       // [line_capacity] peaks_new_tot
    SBB_HD int32_t* negs() const { return merged() + line_capacity(n); }                        // [line_neg_capacity] find_peaks(b); peaks_neg_new after line_merge
    SBB_HD int32_t* arg() const { return negs() + line_neg_capacity(n); }                       // [line_neg_capacity] arg_neg_must_be_deleted
    SBB_HD int32_t* extra() const { return arg() + line_neg_capacity(n); }                      // [line_neg_capacity] peaks_new_extra
    SBB_HD uint8_t* drop_p() const { return (uint8_t*)(extra() + line_neg_capacity(n)); }       // [line_capacity]
    SBB_HD uint8_t* drop_n() const { return drop_p() + line_capacity(n); }                      // [line_neg_capacity]
};

SBB_HD constexpr size_t line_work_bytes(int n)
{
    const size_t cp = (size_t)line_capacity(n), cq = (size_t)line_neg_capacity(n);
    return ((size_t)(2 * n + 6 * kLinePad) * sizeof(double) + (2 * cp + 3 * cq) * sizeof(int32_t) + cp + cq + 15) & ~(size_t)15;
}

// find_peaks(x, height=0), asked about one sample: a peak starts at i and its value is >= 0
template <class Ptr>
SBB_HD bool line_peak_at(Ptr x, int n, int i, int* mid)
{
    return peak_starts_at(x, n, i, mid) && x[*mid] >= 0.0;
}

// The cluster bookkeeping of either pass (first: main.py:562-605, second: main.py:646-721) on the P maxima `peaks` of a and the Q maxima
// `negs` of b.  Returns 1 where the reference raises: np.max of an empty array, or a cluster position that is no index of `peaks`
// (the positions were enumerated over peaks_neg, main.py:564 / 649).  Otherwise k.merged()[0 .. *P2) is peaks_new_tot, k.negs()[0 .. *Q2)
// peaks_neg_new and *clusters the number of clusters merged.
SBB_HD int line_merge(const LineWork& k, int P, int Q, bool first, bool vertical, int* P2, int* Q2, int* clusters)
{
    const double threshold = first ? 0.3 : 0.42;
    double top;
    if (first || vertical) {                        // main.py:562, 1127: np.max(b[peaks_neg])
        if (Q == 0) return 1;
        top = k.b()[k.negs()[0]];
        for (int i = 1; i < Q; ++i) top = k.b()[k.negs()[i]] > top ? k.b()[k.negs()[i]] : top;
    } else {                                        // main.py:646: np.max(a[peaks])
        if (P == 0) return 1;
        top = k.a()[k.peaks()[0]];
        for (int i = 1; i < P; ++i) top = k.a()[k.peaks()[i]] > top ? k.a()[k.peaks()[i]] : top;
    }
    int na = 0, breaks = 0;
    for (int i = 0; i < Q; ++i)
        if (soft_div(k.b()[k.negs()[i]], top) < threshold) k.arg()[na++] = i;
    for (int j = 0; j + 1 < na; ++j) breaks += k.arg()[j + 1] - k.arg()[j] > 1;
    // first pass (main.py:577): clusters only where there is a break.  Second pass (main.py:665-677): >= 2 breaks split; no break and
    // >= 2 entries, or exactly one entry, make one cluster; ONE break makes none.
    const bool split = first ? breaks > 0 : breaks >= 2;
    const bool whole = !first && breaks == 0 && na >= 1;
    *clusters = 0;
    if (!split && !whole) {
        for (int i = 0; i < P; ++i) k.merged()[i] = k.peaks()[i];
        *P2 = P; *Q2 = Q;
        return 0;
    }
    for (int i = 0; i < P; ++i) k.drop_p()[i] = 0;
    for (int i = 0; i < Q; ++i) k.drop_n()[i] = 0;
    int nc = 0, s = 0;
    for (int j = 0; j < na; ++j) {
        if (j + 1 < na && !(split && k.arg()[j + 1] - k.arg()[j] > 1)) continue;
        const int lo = k.arg()[s], hi = k.arg()[j];     // cluster arg[s .. j], ascending; peaks ascending: min = peaks[lo], max = peaks[hi]
        if (hi >= P) return 1;                      // IndexError (main.py:588 / 683)
        k.extra()[nc++] = (k.peaks()[lo] + k.peaks()[hi]) / 2;            // int((min + max) / 2.0), both >= 0
        for (int t = s; t <= j; ++t) {
            const int c = k.arg()[t];
            k.drop_p()[c == 0 ? P - 1 : c - 1] = 1;   // peaks[c - 1]: numpy wraps -1 to the last peak (no exception)
            k.drop_p()[c] = 1;
            k.drop_n()[c] = 1;
        }
        s = j + 1;
    }
    // np.sort(kept peaks ++ extras): both ascending, one merge
    int m = 0, e = 0;
    for (int i = 0; i < P; ++i) {
        if (k.drop_p()[i]) continue;
        while (e < nc && k.extra()[e] < k.peaks()[i]) k.merged()[m++] = k.extra()[e++];
        k.merged()[m++] = k.peaks()[i];
    }
    while (e < nc) k.merged()[m++] = k.extra()[e++];
    int q = 0;
    for (int i = 0; i < Q; ++i)
        if (!k.drop_n()[i]) k.negs()[q++] = k.negs()[i];
    *P2 = m; *Q2 = q; *clusters = nc;
    return 0;
}

// main.py:551-617 after the two smoothings and scans with sigma 2: sigma_gaus, *raised = 1 where the `try` block raised
SBB_HD int line_first_sigma(const LineWork& k, int P, int Q, int* raised)
{
#pragma clang fp contract(off)
    int P2 = 0, Q2 = 0, clusters = 0, sigma = kLineSigmaRaised;
    *raised = 1;
    // fewer than two peaks: np.mean of an empty np.diff is nan and int(nan) raises (main.py:610-612)
    if (!line_merge(k, P, Q, true, false, &P2, &Q2, &clusters) && P2 >= 2) {
        // np.mean(np.diff(peaks_new_tot)): the sum of the int64 differences is exact in any order, last - first
        const double y_diff_mean = soft_div((double)(k.merged()[P2 - 1] - k.merged()[0]), (double)(P2 - 1));
        const double scaled = y_diff_mean * (7. / 40.0);
        sigma = (int)scaled;
        *raised = 0;
    }
    return sigma < 3 ? 3 : sigma;                   // main.py:616-617
}

template <class Ptr>
struct GatheredValues {
    Ptr a;
    const int32_t* at;
    SBB_HD double operator[](int i) const { return a[at[i]]; }
};

struct LineSummary {
    int status, branch, count, P, Q, clusters;
    double level;                                   // mean_value_of_peaks - std_value_of_peaks / 2. (branch 0)
};

// main.py:646-744 after the two smoothings and scans with sigma_gaus: the merged peaks, their statistics and the branch
SBB_HD LineSummary line_second(const LineWork& k, const LineGeom& g, int P, int Q)
{
#pragma clang fp contract(off)
    LineSummary s;
    s.status = kLineNoLines; s.branch = kLineBranchNotReached; s.count = 0; s.P = 0; s.Q = 0; s.clusters = 0; s.level = 0.0;
    // an exception here is not caught in the function: textline_contours_postprocessing's bare except makes the region [] (main.py:1520)
    if (line_merge(k, P, Q, false, g.vertical != 0, &s.P, &s.Q, &s.clusters)) return s;
    if (s.Q == s.P + 1 && s.P >= 3) {
        const GatheredValues<const double*> v{k.a(), k.merged()};
        const double mean = mean_of(v, s.P, k.st), std = std_of(v, s.P, k.st);      // main.py:723-724
        s.level = mean - soft_div(std, 2.0);
        s.branch = kLineBranchBetween;
    } else if (s.P < 1) {
        s.branch = kLineBranchNoPeak;
    } else if (s.P == 1) {
        s.branch = kLineBranchOnePeak;
        if (g.vertical) return s;                   // main.py:1298 reads point_up before any assignment: NameError, the region is []
    } else {
        s.branch = s.P == 2 ? kLineBranchTwoPeaks : kLineBranchOther;
    }
    s.status = kLineOk;
    s.count = s.P;
    return s;
}

// main.py:728-737: peaks - 20 and peaks_neg - 40, clamped to len(x) - 1; negative values are left alone
SBB_HD int line_peak(const LineWork& k, const LineGeom& g, int j) { const int v = k.merged()[j] - kLinePad; return v > g.n - 1 ? g.n - 1 : v; }
SBB_HD int line_neg(const LineWork& k, const LineGeom& g, int j) { const int v = k.negs()[j] - 2 * kLinePad; return v > g.n - 1 ? g.n - 1 : v; }
SBB_HD int line_abs(int v) { return v < 0 ? -v : v; }
// int(factor * d) as Python forms it: one float64 multiply, truncation toward zero
SBB_HD int line_scaled(double factor, int d)
{
#pragma clang fp contract(off)
    const double t = factor * (double)d;
    return (int)t;
}

// int(a * x + b * y + d) with the reference's `< 0` clamp where it has one (main.py:793-815)
SBB_HD int line_rot(double a, double b, double d, int x, int y, bool clamp)
{
#pragma clang fp contract(off)
    const double ax = a * (double)x, by = b * (double)y;
    double v = ax + by;
    v = v + d;
    if (clamp && v < 0.0) v = 0.0;
    return (int)v;
}

// the four rotated corners (main.py:793-815): p1 and p4 clamp x, p1 and p2 clamp y
SBB_HD void line_rot_corners(const LineGeom& g, const int* px, const int* py, int32_t* rot)
{
    rot[0] = line_rot(g.r00, g.r01, g.xd, px[0], py[0], true);      // x_min_rot1
    rot[1] = line_rot(g.r10, g.r11, g.yd, px[0], py[0], true);      // point_up_rot1
    rot[2] = line_rot(g.r00, g.r01, g.xd, px[1], py[1], false);
    rot[3] = line_rot(g.r10, g.r11, g.yd, px[1], py[1], true);      // point_up_rot2
    rot[4] = line_rot(g.r00, g.r01, g.xd, px[2], py[2], false);
    rot[5] = line_rot(g.r10, g.r11, g.yd, px[2], py[2], false);
    rot[6] = line_rot(g.r00, g.r01, g.xd, px[3], py[3], true);      // x_min_rot4
    rot[7] = line_rot(g.r10, g.r11, g.yd, px[3], py[3], false);
}

// line jj of a region (main.py:744-988): pts ={peak, point_up, point_down}, box = the unrotated corners [4][2] (main.py:817-820), rot =
// the rotated corners [4][2]
SBB_HD void line_box(const LineWork& k, const LineGeom& g, const LineSummary& s, int jj, int32_t* pts, int32_t* box, int32_t* rot)
{
    const int rows = g.vertical ? g.other : g.n;    // img_patch.shape[0] = y_max_cont
    const int x_max = g.vertical ? g.n : g.other;   // img_patch.shape[1] = x_max_cont
    const int pk = line_peak(k, g, jj), last = s.P - 1;
    int up, down;
    if (s.branch == kLineBranchBetween) {
        const int d_up = line_abs(pk - line_neg(k, g, jj)), d_down = line_abs(pk - line_neg(k, g, jj + 1));
        const bool high = k.a()[k.merged()[jj]] > s.level;              // main.py:752 / 765
        if (jj == last) {
            up = pk - line_scaled(high ? 1.3 : 1.4, d_up);
            down = g.n - 1;                         // y_max_cont - 1 (main.py:754); x_max_cont - 1 in the vertical splitter (main.py:1220)
        } else {
            up = pk - line_scaled(high ? 1.1 : 1.23, d_up);
            down = pk + line_scaled(high ? 1.1 : 1.33, d_down);
        }
    } else if (s.branch == kLineBranchOnePeak) {
        up = 0; down = rows;                        // y_min_cont, y_max_cont (main.py:829-860)
    } else if (s.branch == kLineBranchTwoPeaks) {
        const int step = line_scaled(1. / 1.8, line_abs(line_peak(k, g, 1) - line_peak(k, g, 0)));
        if (jj == 0) {
            up = 0; down = pk + step;               // main.py:868-871 (`point_up < 0` cannot hold)
        } else {
            down = pk + step;
            if (down >= rows) down = rows - 2;
            up = pk - step;
        }
    } else {
        if (jj == 0) {
            const int step = line_scaled(1. / 1.9, line_peak(k, g, 1) - pk);
            up = pk - step;
            if (up < 0) up = 1;
            down = pk + step;
        } else if (jj == last) {
            const int dis = pk - line_peak(k, g, jj - 1);
            down = pk + line_scaled(1. / 1.7, dis);
            if (down >= rows) down = rows - 2;
            up = pk - line_scaled(1. / 1.9, dis);
        } else {
            up = pk - line_scaled(1. / 1.9, pk - line_peak(k, g, jj - 1));
            down = pk + line_scaled(1. / 1.9, line_peak(k, g, jj + 1) - pk);
        }
    }
    pts[0] = pk; pts[1] = up; pts[2] = down;
    box[0] = 0; box[1] = up; box[2] = x_max; box[3] = up; box[4] = x_max; box[5] = down; box[6] = 0; box[7] = down;
    // the four points that are rotated: the box itself, or (point_up | point_down, y_min_cont | y_max_cont) in the vertical splitter
    // (main.py:1259-1262)
    int px[4], py[4];
    if (g.vertical) {
        px[0] = up; py[0] = 0; px[1] = down; py[1] = 0; px[2] = down; py[2] = rows; px[3] = up; py[3] = rows;
    } else {
        px[0] = 0; py[0] = up; px[1] = x_max; py[1] = up; px[2] = x_max; py[2] = down; px[3] = 0; py[3] = down;
    }
    line_rot_corners(g, px, py, rot);
}

// The corners of a line of the HORIZONTAL splitter for an x extent other than 0 .. x_max_cont (line_extent.h: x_min / x_max from
// cv2.pointPolygonTest, main.py:780-820): box and rot as line_box writes them, with x_min / x_max in place of 0 / x_max_cont.
SBB_HD void line_box_with_extent(const LineGeom& g, int x_min, int x_max, int up, int down, int32_t* box, int32_t* rot)
{
    box[0] = x_min; box[1] = up; box[2] = x_max; box[3] = up; box[4] = x_max; box[5] = down; box[6] = x_min; box[7] = down;
    const int px[4] = {x_min, x_max, x_max, x_min}, py[4] = {up, up, down, down};
    line_rot_corners(g, px, py, rot);
}

// both smoothings and both scans of one pass, serially; returns through *P, *Q
inline void line_pass_serial(const int32_t* y, int n, double top, const double* w, int sigma, const LineWork& k, int* P, int* Q)
{
    const int na = n + 2 * kLinePad, nb = n + 4 * kLinePad, radius = 4 * sigma;
    const PaddedSamplesP ys{y, n, kLinePad};
    const FlippedSamplesP fs{y, n, kLinePad, top};
    for (int i = 0; i < na; ++i) k.a()[i] = smooth_sample(ys, na, w, radius, i);
    for (int i = 0; i < nb; ++i) k.b()[i] = smooth_sample(fs, nb, w, radius, i);
    int p = 0, q = 0, mid;
    for (int i = 1; i < na - 1; ++i)
        if (line_peak_at(k.a(), na, i, &mid)) k.peaks()[p++] = mid;
    for (int i = 1; i < nb - 1; ++i)
        if (line_peak_at(k.b(), nb, i, &mid)) k.negs()[q++] = mid;
    *P = p; *Q = q;
}

// One region, serially.  info: kLineInfoInts ints; pts / box / rot: room for line_capacity(g.n) lines of 3 / 8 / 8 ints, the first
// info[kLineInfoCount] of which are written.
inline void line_split_serial(const int32_t* y, const LineGeom& g, const LineWeights& weights, const LineWork& k, int32_t* info, int32_t* pts,
                              int32_t* box, int32_t* rot)
{
    int top = 0, P = 0, Q = 0, raised = 0;
    for (int i = 0; i < g.n; ++i) top = y[i] > top ? y[i] : top;
    line_pass_serial(y, g.n, (double)top, weights.half(kLineSigmaMin), kLineSigmaMin, k, &P, &Q);
    const int sigma = line_first_sigma(k, P, Q, &raised);
    info[kLineInfoSigma] = sigma; info[kLineInfoRaised] = raised; info[kLineInfoBranch] = kLineBranchNotReached; info[kLineInfoCount] = 0;
    const double* w = weights.half(sigma);
    if (!w) { info[kLineInfoStatus] = kLineSigmaTooLarge; return; }
    line_pass_serial(y, g.n, (double)top, w, sigma, k, &P, &Q);
    const LineSummary s = line_second(k, g, P, Q);
    info[kLineInfoStatus] = s.status; info[kLineInfoBranch] = s.branch; info[kLineInfoCount] = s.count;
    for (int jj = 0; jj < s.count; ++jj) line_box(k, g, s, jj, pts + 3 * jj, box + 8 * jj, rot + 8 * jj);
}

}  // namespace sbbseg

#endif  // SBBSEG_LINE_SPLIT_H
