// contour_glue.hip -- host side of libsbbseg's component and contour stages: the C ABI entry points (include/sbbseg.h) of the page box, the
// text-region presence gate, boxes and contour polygons, and the host twins of the tracer.  One front end serves them all: class mask + OPEN +
// CLOSE (open_close_class), labelling (label_components), the root records (fetch_roots), and -- where the device's bounds leave a ranking
// or a filter open -- one host fallback on the downloaded label plane (trace_on_host).  The host twins run on contour_host.h.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "ctx.h"
#include "contour_host.h"

using namespace sbbseg;

static const char* contour_status_text(int status)
{
    return status == kContourStepBound ? "the walk did not close within its step bound"
                                       : status == kContourBroken ? "the walk lost its component" : "the component's box does not hold its first pixel";
}

// The five int planes launch_largest_contour leaves per root in c->cc_aux: a lower bound of the doubled contour area, and the box.
struct CcPlanes {
    int *lower2, *x0, *y0, *x1, *y1;
};

// The labelling step: the 8-connected components of the 0 / 255 plane d_mask into c->cc_parent.p (parent[i] = root = the component's first
// pixel in raster order, -1 for background), pixel counts into c->cc_count.p, the per-root planes into *pl, the ranking's result record
// into c->d_cc_list and its best key into c->d_cc_small.
static int label_components(sbbseg_ctx* c, const uint8_t* d_mask, int H, int W, CcPlanes* pl)
{
    const size_t pix = (size_t)H * W;
    if (ensure(c, c->cc_parent, pix * sizeof(int)) || ensure(c, c->cc_count, pix * sizeof(int))) return 1;
    if (ensure(c, c->cc_aux, 5 * pix * sizeof(int))) return 1;
    if (!c->d_cc_small && dmalloc(c, (void**)&c->d_cc_small, 4 * sizeof(unsigned long long))) return 1;
    if (!c->d_cc_list && dmalloc(c, (void**)&c->d_cc_list, (6 + kCcMaxRivals) * sizeof(int))) return 1;
    int* aux = c->cc_aux.p;
    *pl = CcPlanes{aux, aux + pix, aux + 2 * pix, aux + 3 * pix, aux + 4 * pix};
    HIPCHK(launch_largest_contour(d_mask, H, W, c->cc_parent.p, c->cc_count.p, pl->lower2, pl->x0, pl->y0, pl->x1, pl->y1, c->d_cc_small, c->d_cc_list,
                                  c->stream));
    return 0;
}

// get_text_region_contours_and_boxes' front end (main.py:456-480): class mask (all channels == label -> 255), MORPH_OPEN, MORPH_CLOSE with the
// 5x5 kernel, into c->morph_b.p.  OPEN = erode, dilate; CLOSE = dilate, erode (cv2.morphologyEx, one iteration each, default border: outside
// pixels never win); the two dilations in a row are one clipped 9x9 maximum.
static int open_close_class(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label)
{
    const size_t pix = (size_t)H * W;
    if (ensure(c, c->morph_a, pix) || ensure(c, c->morph_b, pix)) return 1;
    HIPCHK(launch_morph((const uint8_t*)d_regions_hw, c->morph_a.p, c->morph_b.p, H, W, 2, 0, 0x100 | label, c->stream));
    HIPCHK(launch_morph(c->morph_b.p, c->morph_a.p, c->morph_b.p, H, W, 4, 1, 0, c->stream));
    HIPCHK(launch_morph(c->morph_b.p, c->morph_a.p, c->morph_b.p, H, W, 2, 0, 0, c->stream));
    return 0;
}

// The root records a kernel listed in c->cc_roots.p (their number in *d_n), sorted by DESCENDING root -- the reverse discovery order that
// OpenCV's contour list is assumed to have (contour_host.h: host_largest_contour).
static int fetch_roots(sbbseg_ctx* c, const int* d_n, size_t list_cap, const char* what, std::vector<ContourCand>& roots)
{
    int found = 0;
    HIPCHK(hipMemcpyAsync(&found, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    REQUIRE(found >= 0 && (size_t)found <= list_cap, "internal error: %d %s, room for %zu", found, what, list_cap);
    alloc_check();
    roots.resize((size_t)found);
    if (found) HIPCHK(hipMemcpy(roots.data(), c->cc_roots.p, (size_t)found * sizeof(ContourCand), hipMemcpyDeviceToHost));
    std::sort(roots.begin(), roots.end(), [](const ContourCand& a, const ContourCand& b) { return a.root > b.root; });
    return 0;
}

// Doubled shoelace area of the outer border of the component `inside` describes, walked from its first pixel in raster order
// (sy, sx) -- whose west / north neighbours are background -- by Moore neighbour tracing, clockwise with y pointing down; stops
// when the start pixel is left again in the first direction.  box = {x0, y0, x1, y1} of the border (= of the component).
// The same closed chain as contour_walk's, reversed (tests/test_contours_cpu.py), so the same area and box.  It stays for the host fallback
// alone because it is the faster of the two there: it stops at the first neighbour it finds where walk_label_contour reads all eight per
// step (profiles/contour_glue.md: 10 against 15.6 ms for the page box of a 3600 x 2600 notched lattice).
static const int dx8[8] = {1, 1, 0, -1, -1, -1, 0, 1}, dy8[8] = {0, 1, 1, 1, 0, -1, -1, -1};      // E, SE, S, SW, W, NW, N, NE
template <typename Inside>
static long long trace_outer_area2(Inside inside, int sy, int sx, long n_pixels, int (&box)[4])
{
    long long area2 = 0;
    int cy = sy, cx = sx, back = 4, first_dir = -1;              // back: direction of the background pixel the search resumes after (W)
    box[0] = box[2] = sx; box[1] = box[3] = sy;
    for (long guard = 0; guard < 4 * n_pixels + 8; ++guard) {
        int d = -1;
        for (int k = 1; k <= 8; ++k) {                           // clockwise from the backtrack direction
            const int dd = (back + k) & 7;
            if (inside(cy + dy8[dd], cx + dx8[dd])) { d = dd; break; }
        }
        if (d < 0) break;                                        // isolated pixel: area 0
        if (cy == sy && cx == sx) {
            if (first_dir < 0) first_dir = d;
            else if (d == first_dir) break;                      // back at the start, leaving the same way: closed
        }
        const int ny = cy + dy8[d], nx = cx + dx8[d];
        area2 += (long long)cx * ny - (long long)nx * cy;
        cy = ny; cx = nx;
        box[0] = cx < box[0] ? cx : box[0]; box[2] = cx > box[2] ? cx : box[2];
        box[1] = cy < box[1] ? cy : box[1]; box[3] = cy > box[3] ? cy : box[3];
        // the neighbour examined just before (direction d - 1 from the old pixel) is background; seen from the new pixel it
        // lies in direction d + 6 (axis step) or d + 5 (diagonal step): the next search resumes right after it
        back = (d + ((d & 1) ? 5 : 6)) & 7;
    }
    return area2 < 0 ? -area2 : area2;
}

// The host fallback: the exact outer contours of components of the device's label plane (c->cc_parent.p), for the callers whose bounds
// leave a decision open: 4 bytes per pixel of D2H, once per call, + the listed perimeters.  every_root: t is filled with every root of the
// plane instead.  Counts as ONE host ranking (host_contour_calls) however many roots it traces.
struct HostTrace {
    int root;
    long long area2;
    int box[4];             // x0, y0, x1, y1
};
static int trace_on_host(sbbseg_ctx* c, int H, int W, std::vector<HostTrace>& t, bool every_root = false)
{
    const size_t pix = (size_t)H * W;
    alloc_check();
    std::vector<int> lab(pix);
    HIPCHK(hipMemcpy(lab.data(), c->cc_parent.p, pix * sizeof(int), hipMemcpyDeviceToHost));
    if (every_root) {
        t.clear();
        for (size_t i = 0; i < pix; ++i)
            if (lab[i] == (int)i) t.push_back(HostTrace{(int)i, 0, {}});
    }
    for (HostTrace& k : t) {
        const int root = k.root;
        auto inside = [&](int y, int x) { return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && lab[(size_t)y * W + x] == root; };
        int tb[4];                                           // (a local: the tracer keeps it in registers)
        k.area2 = trace_outer_area2(inside, root / W, root % W, (long)pix, tb);
        for (int q = 0; q < 4; ++q) k.box[q] = tb[q];
    }
    c->host_contour_calls += 1;
    return 0;
}

// The contour ranking behind sbbseg_page_box_dev and sbbseg_text_regions_present_dev: 8-connected components of the 0 / 255 plane in
// c->morph_b.p, ranked by the area of their outer contour (cv2.contourArea of cv2.findContours' outer borders).  The device ranks by a
// lower bound of that area and checks the winner against every other component's bounding-box bound (launch_largest_contour); when
// that leaves the ranking open the host walks the outer borders of the candidates on the device's label plane (trace_on_host).
// box = {x0, y0, x1, y1, pixels} of the winner; *any = false for an empty plane; *area2 = twice the winner's contour area (exact when
// traced, else the device's lower bound).
// exact_below2: trace on the host (exact area) also when the device's lower bound of TWICE the winner's area is below this -- the caller's
// threshold: one labelling pass and one copy of the label plane decide "too small", not two
static int rank_contours(sbbseg_ctx* c, int H, int W, int (&box)[5], bool* any, long long* area2, double exact_below2 = -1.0)
{
    CcPlanes pl;
    if (label_components(c, c->morph_b.p, H, W, &pl)) return 1;
    int out[6 + kCcMaxRivals];
    unsigned long long key = 0;
    HIPCHK(hipMemcpyAsync(out, c->d_cc_list, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&key, c->d_cc_small, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int q = 0; q < 5; ++q) box[q] = out[q];
    *any = out[2] >= 0;
    *area2 = (long long)(key >> 32);
    if (!*any || !(out[5] > 0 || c->force_host_contours || (double)*area2 < exact_below2)) return 0;
    // the device's winner and the rivals it listed; every root when it found more than it lists (or the test hook asks)
    const bool every_root = out[5] > kCcMaxRivals || c->force_host_contours;
    std::vector<HostTrace> t(1, HostTrace{(int)((unsigned)(key & 0xffffffffu) - 1u), 0, {}});
    for (int k = 0; k < out[5] && !every_root; ++k) t.push_back(HostTrace{out[6 + k], 0, {}});
    if (trace_on_host(c, H, W, t, every_root)) return 1;
    const HostTrace* best = nullptr;
    for (const HostTrace& k : t)
        if (!best || k.area2 > best->area2 || (k.area2 == best->area2 && k.root > best->root)) best = &k;      // ties: the later root
    REQUIRE(best, "internal error: a plane with a winner has no root");
    for (int q = 0; q < 4; ++q) box[q] = best->box[q];
    HIPCHK(hipMemcpy(&box[4], c->cc_count.p + best->root, sizeof(int), hipMemcpyDeviceToHost));
    *area2 = best->area2;
    return 0;
}

extern "C" {

int sbbseg_page_box_dev(sbbseg_ctx* c, const void* d_mask_hw, int H, int W, int32_t* box_xywh, int64_t* pixels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_mask_hw && box_xywh && H > 0 && W > 0, "bad arguments");
    REQUIRE((size_t)H * W < ((size_t)1 << 31), "mask too large for 32-bit pixel indices");
    const size_t pix = (size_t)H * W;
    if (ensure(c, c->morph_a, pix) || ensure(c, c->morph_b, pix)) return 1;
    // main.py:394-398: gray > 0 -> 255, dilate with the 5x5 kernel of ones, 6 iterations (= one clipped 25x25 maximum)
    HIPCHK(launch_morph((const uint8_t*)d_mask_hw, c->morph_a.p, c->morph_b.p, H, W, 12, 1, 1, c->stream));
    // main.py:398-404: the contour with the largest cv2.contourArea
    int box[5];
    bool any = false;
    long long area2 = 0;
    if (rank_contours(c, H, W, box, &any, &area2)) return 1;
    if (pixels) *pixels = any ? (int64_t)box[4] : 0;
    if (!any) {                                        // empty mask: the reference's np.argmax of an empty list raises (main.py:399-401)
        box_xywh[0] = box_xywh[1] = box_xywh[2] = box_xywh[3] = 0;
        return 0;
    }
    box_xywh[0] = box[0]; box_xywh[1] = box[1]; box_xywh[2] = box[2] - box[0] + 1; box_xywh[3] = box[3] - box[1] + 1;   // cv2.boundingRect
    return 0;
    API_END
}

// What the region entry points share: a label plane and filter_contours_area_of_image's window, as fractions of the plane.  (The
// presence gate has no upper end -- its max_area is the reference's fixed 1 -- and any min_area >= 0 is valid for it: it omits max_area.)
static int check_region_args(const void* d_regions_hw, int H, int W, int label, double min_area, double max_area = HUGE_VAL)
{
    REQUIRE(d_regions_hw && H > 0 && W > 0 && label >= 0 && label <= 255 && min_area >= 0.0 && max_area >= min_area, "bad arguments");
    return 0;
}

// get_text_region_contours_and_boxes' EXISTENCE test (main.py:456-480, the `if len(contours) > 0` that gates the textline model,
// main.py:2083-2096): open_close_class, findContours(RETR_TREE), keep the contours without a parent whose polygon area lies in
// [min_area, max_area = 1] x H x W.  After OPEN and CLOSE every component and every hole is a union of 5x5 squares, so no contour has
// fewer than three points (the `jv` bookkeeping of filter_contours_area_of_image, main.py:81-91, never drifts), and the largest outer
// contour of the plane is always a parentless one (a component nested in a hole is smaller than the component around it): contours
// exist <=> the largest outer-contour area reaches min_area * H * W.
int sbbseg_text_regions_present_dev(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label, double min_area, int* present)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(present, "bad arguments");
    if (check_region_args(d_regions_hw, H, W, label, min_area)) return 1;
    REQUIRE((size_t)H * W < ((size_t)1 << 31), "plane too large for 32-bit pixel indices");
    if (open_close_class(c, d_regions_hw, H, W, label)) return 1;
    const double need = min_area * (double)((long long)H * W);            // main.py:87: area >= min_area * np.prod(image.shape[:2])
    int box[5];
    bool any = false;
    long long area2 = 0;
    // the device's figure is a lower bound (holes not filled): only the exact area can say "too small" -- traced in the same pass
    if (rank_contours(c, H, W, box, &any, &area2, 2.0 * need)) return 1;
    *present = (any && (double)area2 * 0.5 >= need) ? 1 : 0;
    return 0;
    API_END
}

// The front end the boxes and the contours share: open_close_class (into c->morph_b.p), labelling (c->cc_parent.p), and the records of the
// components without a parent (launch_parentless_roots), sorted by DESCENDING root.
static int parentless_roots(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label, std::vector<ContourCand>& roots)
{
    const size_t pix = (size_t)H * W;
    CcPlanes pl;
    if (open_close_class(c, d_regions_hw, H, W, label) || label_components(c, c->morph_b.p, H, W, &pl)) return 1;
    // after OPEN + CLOSE a component holds a whole 5x5 square (planes narrower than the kernel: no such bound)
    const size_t list_cap = (H >= 5 && W >= 5) ? pix / 25 + 16 : pix;
    if (ensure(c, c->cc_bg, 2 * pix * sizeof(int)) || ensure(c, c->cc_roots, list_cap * sizeof(ContourCand))) return 1;
    int* d_n = (int*)(c->d_cc_small + 2);
    HIPCHK(launch_parentless_roots(c->morph_b.p, c->morph_a.p, H, W, c->cc_parent.p, c->cc_bg.p, c->cc_count.p, pl.lower2, pl.x0, pl.y0, pl.x1, pl.y1,
                                   d_n, c->cc_roots.p, (int)list_cap, c->stream));
    return fetch_roots(c, d_n, list_cap, "parentless components", roots);
}

// get_text_region_contours_and_boxes' BOXES (main.py:456-480, `self.boxes`): parentless_roots, then cv2.boundingRect of every contour that
// filter_contours_area_of_image keeps -- a component without a parent whose outer-contour area lies in [min_area, max_area] x H x W.  The
// device has a lower bound of that area per root (cells of the component as it is) and the bounding-box upper bound (w - 1)(h - 1); only
// a component the two bounds leave undecided is traced on the host (trace_on_host).  Order [EXT, unpinned]: the component's first pixel in
// raster order, DESCENDING (fetch_roots).  Nothing downstream of the boxes depends on it: slopes are per box.
int sbbseg_text_region_boxes_dev(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label, double min_area, double max_area,
                                 int32_t* boxes_xywh, int cap, int* n_boxes)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_boxes && cap >= 0 && (boxes_xywh || cap == 0), "bad arguments");
    if (check_region_args(d_regions_hw, H, W, label, min_area, max_area)) return 1;
    REQUIRE((size_t)H * W < ((size_t)1 << 31), "plane too large for 32-bit pixel indices");
    std::vector<ContourCand> roots;
    if (parentless_roots(c, d_regions_hw, H, W, label, roots)) return 1;
    const int found = (int)roots.size();
    // main.py:87: area >= min_area * np.prod(image.shape[:2]) and area <= max_area * np.prod(image.shape[:2])
    const double lo = min_area * (double)((long long)H * W), hi = max_area * (double)((long long)H * W);
    std::vector<int> state((size_t)found);                     // 1 keep, 0 drop, >= 2 undecided: 2 + its place among the traced
    std::vector<HostTrace> t;
    for (int k = 0; k < found; ++k) {
        const ContourCand& r = roots[k];
        const double lower = (double)r.lower2 * 0.5, upper = (double)(r.x1 - r.x0) * (double)(r.y1 - r.y0);
        if (!c->force_host_contours && (upper < lo || lower > hi)) state[k] = 0;
        else if (!c->force_host_contours && lower >= lo && upper <= hi) state[k] = 1;
        else {
            state[k] = 2 + (int)t.size();
            t.push_back(HostTrace{r.root, 0, {}});
        }
    }
    if (!t.empty() && trace_on_host(c, H, W, t)) return 1;
    int kept = 0;
    for (int k = 0; k < found; ++k) {
        if (state[k] >= 2) {
            const double area = (double)t[(size_t)state[k] - 2].area2 * 0.5;
            state[k] = (area >= lo && area <= hi) ? 1 : 0;
        }
        if (state[k] != 1) continue;
        if (kept < cap) {
            const ContourCand& r = roots[k];
            int32_t* o = boxes_xywh + (size_t)kept * 4;
            o[0] = r.x0; o[1] = r.y0; o[2] = r.x1 - r.x0 + 1; o[3] = r.y1 - r.y0 + 1;                  // cv2.boundingRect
        }
        ++kept;
    }
    *n_boxes = kept;
    return 0;
    API_END
}

int sbbseg_text_region_boxes(sbbseg_ctx* c, const uint8_t* regions_hw, int H, int W, int label, double min_area, double max_area,
                             int32_t* boxes_xywh, int cap, int* n_boxes)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    const void* d_plane;
    if (stage_plane(c, regions_hw, H, W, true, &d_plane)) return 1;
    return sbbseg_text_region_boxes_dev(c, d_plane, H, W, label, min_area, max_area, boxes_xywh, cap, n_boxes);
    API_END
}

// ---- get_text_region_contours_and_boxes' CONTOURS (main.py:471-481): the outer border of every kept component as
// cv2.findContours(CHAIN_APPROX_SIMPLE) lists it (contour_walk.h), traced on the device (contours.hip) on the label plane in
// c->cc_parent.p.  cand: the candidates in the order of the result.  filter: filter_contours_area_of_image's test on the EXACT area of the
// traced chain (no bounds, no host tracing).  The tables stay in c->contour_tab / c->contour_pts until the next call.
static int trace_contours(sbbseg_ctx* c, int H, int W, const std::vector<ContourCand>& cand, bool filter, double lo, double hi, int* n_contours,
                          int64_t* n_points)
{
    c->contour_n = -1;
    c->contour_np = 0;
    const size_t n = cand.size();
    *n_contours = 0;
    *n_points = 0;
    if (n == 0) {
        c->contour_n = 0;
        return 0;
    }
    const size_t rec_at = align16(n * sizeof(ContourCand)), slot_at = rec_at + align16(n * sizeof(ContourRec));
    const size_t boxes_at = slot_at + align16(n * sizeof(int)), area2_at = boxes_at + align16(n * 4 * sizeof(int32_t));
    const size_t off_at = area2_at + align16(n * sizeof(long long)), totals_at = off_at + align16((n + 1) * sizeof(long long));
    if (ensure(c, c->contour_tab, totals_at + 4 * sizeof(long long))) return 1;
    unsigned char* d = (unsigned char*)c->contour_tab.p;
    bool any_lds = false, any_global = false;
    for (const ContourCand& k : cand) {
        const bool lds = contour_form(k.root, k.x0, k.y0, k.x1, k.y1, H, W, c->contour_lds_limit) == kContourFormLds;
        any_lds = any_lds || lds;
        any_global = any_global || !lds;
    }
    ContourParams p;
    p.parent = c->cc_parent.p; p.H = H; p.W = W;
    p.cand = (const ContourCand*)d; p.n_cand = (int)n; p.lds_limit = c->contour_lds_limit;
    p.rec = (ContourRec*)(d + rec_at); p.slot = (const int*)(d + slot_at); p.point_off = (const long long*)(d + off_at); p.points = nullptr;
    ContourPackParams q;
    q.rec = p.rec; q.n_cand = (int)n; q.filter = filter ? 1 : 0; q.lo = lo; q.hi = hi;
    q.slot = (int*)(d + slot_at); q.boxes = (int32_t*)(d + boxes_at); q.area2 = (long long*)(d + area2_at);
    q.point_off = (long long*)(d + off_at); q.totals = (long long*)(d + totals_at);
    long long totals[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(d, cand.data(), n * sizeof(ContourCand), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_contour_trace(p, any_lds, any_global, c->stream));
    HIPCHK(launch_contour_pack(q, c->stream));
    HIPCHK(hipMemcpyAsync(totals, q.totals, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the caller's candidate list lives until here)
    c->contour_launches += (any_lds ? 1 : 0) + (any_global ? 1 : 0) + 1;
    REQUIRE(totals[2] == 0, "contour tracing failed for %lld of %zu components (%s): the label plane is damaged", totals[2], n,
            totals[3] == kContourStepBound ? "the walk did not close within 8 x box pixels + 8 steps" : contour_status_text((int)totals[3]));
    REQUIRE(totals[0] >= 0 && (size_t)totals[0] <= n && totals[1] >= 0, "internal error: %lld contours of %zu candidates", totals[0], n);
    if (totals[1] > 0) {
        if (ensure(c, c->contour_pts, (size_t)totals[1] * 2 * sizeof(int32_t))) return 1;
        p.points = c->contour_pts.p;
        HIPCHK(launch_contour_trace(p, any_lds, any_global, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->contour_launches += (any_lds ? 1 : 0) + (any_global ? 1 : 0);
    }
    c->contour_boxes_at = boxes_at; c->contour_area2_at = area2_at; c->contour_off_at = off_at;
    c->contour_n = (int)totals[0];
    c->contour_np = totals[1];
    *n_contours = c->contour_n;
    *n_points = (int64_t)c->contour_np;
    return 0;
}

int sbbseg_text_region_contours_dev(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label, double min_area, double max_area,
                                    int* n_contours, int64_t* n_points)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_contours && n_points, "bad arguments");
    if (check_region_args(d_regions_hw, H, W, label, min_area, max_area)) return 1;
    REQUIRE((size_t)H * W < ((size_t)1 << 28), "plane too large: a contour's point count must fit 32 bits");
    c->contour_n = -1;
    std::vector<ContourCand> roots;
    if (parentless_roots(c, d_regions_hw, H, W, label, roots)) return 1;
    // main.py:87: area >= min_area * np.prod(image.shape[:2]) and area <= max_area * np.prod(image.shape[:2])
    const double lo = min_area * (double)((long long)H * W), hi = max_area * (double)((long long)H * W);
    return trace_contours(c, H, W, roots, true, lo, hi, n_contours, n_points);
    API_END
}

int sbbseg_text_region_contours(sbbseg_ctx* c, const uint8_t* regions_hw, int H, int W, int label, double min_area, double max_area,
                                int* n_contours, int64_t* n_points)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    const void* d_plane;
    if (stage_plane(c, regions_hw, H, W, true, &d_plane)) return 1;
    return sbbseg_text_region_contours_dev(c, d_plane, H, W, label, min_area, max_area, n_contours, n_points);
    API_END
}

int sbbseg_debug_mask_contours_dev(sbbseg_ctx* c, const void* d_mask_hw, int H, int W, int* n_contours, int64_t* n_points)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_mask_hw && n_contours && n_points && H > 0 && W > 0, "bad arguments");
    REQUIRE((size_t)H * W < ((size_t)1 << 28), "plane too large: a contour's point count must fit 32 bits");
    c->contour_n = -1;
    const size_t pix = (size_t)H * W;
    const size_t list_cap = (size_t)((H + 1) / 2) * (size_t)((W + 1) / 2);         // 8-connected components of an H x W plane, at most
    CcPlanes pl;
    if (ensure(c, c->cc_roots, list_cap * sizeof(ContourCand)) || label_components(c, (const uint8_t*)d_mask_hw, H, W, &pl)) return 1;
    int* d_n = (int*)(c->d_cc_small + 2);
    HIPCHK(launch_contour_all_roots(c->cc_parent.p, pl.x0, pl.y0, pl.x1, pl.y1, (long)pix, d_n, (ContourCand*)c->cc_roots.p, (int)list_cap, c->stream));
    std::vector<ContourCand> roots;
    if (fetch_roots(c, d_n, list_cap, "components", roots)) return 1;
    return trace_contours(c, H, W, roots, false, 0.0, 0.0, n_contours, n_points);
    API_END
}

int sbbseg_text_region_contours_read(sbbseg_ctx* c, int32_t* boxes_xywh, int64_t* area2, int64_t* point_off, int cap_contours, int32_t* points_xy,
                                     int64_t cap_points)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(c->contour_n >= 0, "no contours on this handle: the last contour call failed, or there was none");
    REQUIRE(cap_contours >= 0 && cap_points >= 0 && point_off && (boxes_xywh || cap_contours == 0) && (area2 || cap_contours == 0) &&
                (points_xy || cap_points == 0), "bad arguments");
    const int n = c->contour_n;
    const long long np = c->contour_np;
    REQUIRE(cap_contours >= n && cap_points >= np, "room for %d contours and %lld points, the handle holds %d and %lld", cap_contours,
            (long long)cap_points, n, np);
    if (n == 0) {
        point_off[0] = 0;
        return 0;
    }
    static_assert(sizeof(int64_t) == sizeof(long long), "the tables are copied out as they are");
    const unsigned char* d = (const unsigned char*)c->contour_tab.p;
    HIPCHK(hipMemcpyAsync(boxes_xywh, d + c->contour_boxes_at, (size_t)n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(area2, d + c->contour_area2_at, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(point_off, d + c->contour_off_at, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (np) HIPCHK(hipMemcpyAsync(points_xy, c->contour_pts.p, (size_t)np * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_debug_set_contour_lds_limit(sbbseg_ctx* c, int bytes)
{
    API_BEGIN
    REQUIRE(c && bytes >= 0 && bytes <= kContourLdsBytes, "contour LDS limit: 0 .. %d bytes", kContourLdsBytes);
    c->contour_lds_limit = bytes;
    return 0;
    API_END
}

int sbbseg_debug_contour_launches(sbbseg_ctx* c, int64_t* value)
{
    API_BEGIN
    REQUIRE(c && value, "bad arguments");
    *value = (int64_t)c->contour_launches;
    return 0;
    API_END
}

// The host twin: every 8-connected component of mask != 0 (no morphology, no filter), by descending first pixel, through the same walk.
static long long g_contour_host_step_bound = 0;          // test hook: > 0 replaces contour_step_bound (sbbseg_debug_set_contour_host_step_bound)

int sbbseg_debug_set_contour_host_step_bound(int64_t steps)
{
    API_BEGIN
    REQUIRE(steps >= 0, "steps must be >= 0 (0 restores the bound of 8 x box pixels + 8)");
    g_contour_host_step_bound = steps;
    return 0;
    API_END
}

int sbbseg_mask_contours_host(const uint8_t* mask_hw, int H, int W, int32_t* boxes_xywh, int64_t* area2, int64_t* point_off, int cap_contours,
                              int32_t* points_xy, int64_t cap_points, int* n_contours, int64_t* n_points)
{
    API_BEGIN
    REQUIRE(mask_hw && H > 0 && W > 0 && n_contours && n_points && cap_contours >= 0 && cap_points >= 0, "bad arguments");
    REQUIRE((size_t)H * W < ((size_t)1 << 28), "plane too large: a contour's point count must fit 32 bits");
    const bool count_only = !boxes_xywh && !area2 && !point_off && !points_xy;
    REQUIRE(count_only || (boxes_xywh && area2 && point_off && points_xy), "give every output table, or none (to get the counts)");
    alloc_check();
    std::vector<int> lab;
    std::vector<LabelComp> comps;
    label_mask(mask_hw, H, W, lab, comps);
    std::vector<int32_t> boxes, pts;
    std::vector<int64_t> areas, offs(1, 0);
    for (size_t q = comps.size(); q-- > 0;) {                      // descending first pixel
        const int root = comps[q].root;
        auto emit = [&](int, int x, int y) { pts.push_back(x); pts.push_back(y); };
        const long long bound = g_contour_host_step_bound > 0 ? g_contour_host_step_bound : label_comp_step_bound(comps[q]);
        const ContourResult r = walk_label_contour(lab.data(), H, W, root, bound, emit);
        REQUIRE(r.status == kContourOk, "the contour of the component at (%d, %d) did not close within %lld steps", root % W, root / W, bound);
        const int32_t b[4] = {r.x0, r.y0, r.x1 - r.x0 + 1, r.y1 - r.y0 + 1};
        boxes.insert(boxes.end(), b, b + 4);
        areas.push_back((int64_t)r.area2);
        offs.push_back((int64_t)(pts.size() / 2));
    }
    *n_contours = (int)comps.size();
    *n_points = offs.back();
    if (count_only) return 0;
    REQUIRE((size_t)cap_contours >= comps.size() && cap_points >= offs.back(), "room for %d contours and %lld points, the mask has %zu and %lld",
            cap_contours, (long long)cap_points, comps.size(), (long long)offs.back());
    if (!boxes.empty()) memcpy(boxes_xywh, boxes.data(), boxes.size() * sizeof(int32_t));
    if (!areas.empty()) memcpy(area2, areas.data(), areas.size() * sizeof(int64_t));
    memcpy(point_off, offs.data(), offs.size() * sizeof(int64_t));
    if (!pts.empty()) memcpy(points_xy, pts.data(), pts.size() * sizeof(int32_t));
    return 0;
    API_END
}

// The host ranking (contour_host.h: host_largest_contour) of a u8 mask: box + pixels, and the doubled area, of its largest outer contour.
static int largest_contour_of(const uint8_t* mask_hw, int H, int W, LargestContour* best)
{
    REQUIRE(mask_hw && H > 0 && W > 0 && (size_t)H * W < ((size_t)1 << 31), "bad arguments");
    alloc_check();
    *best = host_largest_contour(mask_hw, H, W);
    REQUIRE(best->status == kContourOk, "contour tracing failed for the component at (%d, %d) (%s)", best->bad_root % W, best->bad_root / W,
            contour_status_text(best->status));
    return 0;
}

int sbbseg_debug_largest_contour(const uint8_t* mask_hw, int H, int W, int32_t* box_xywh, int64_t* pixels)
{
    API_BEGIN
    REQUIRE(box_xywh, "bad arguments");
    LargestContour best;
    if (largest_contour_of(mask_hw, H, W, &best)) return 1;
    const LabelComp& k = best.comp;
    if (pixels) *pixels = best.any ? k.pixels : 0;
    box_xywh[0] = best.any ? k.x0 : 0; box_xywh[1] = best.any ? k.y0 : 0;
    box_xywh[2] = best.any ? k.x1 - k.x0 + 1 : 0; box_xywh[3] = best.any ? k.y1 - k.y0 + 1 : 0;
    return 0;
    API_END
}

int sbbseg_debug_largest_contour_area2(const uint8_t* mask_hw, int H, int W, int64_t* area2)
{
    API_BEGIN
    REQUIRE(area2, "bad arguments");
    LargestContour best;
    if (largest_contour_of(mask_hw, H, W, &best)) return 1;
    *area2 = (int64_t)best.area2;
    return 0;
    API_END
}

}  // extern "C"
