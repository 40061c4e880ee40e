// line_extent_glue.hip -- host side of the text-line x extents (the contour half of textline_contours_postprocessing, main.py:1492-1511, and
// cv2.pointPolygonTest inside seperate_lines): the C ABI entry points (include/sbbseg.h) of the device step (line_extent.hip), its serial
// host twin, and the debug entries of the border scan.  The arithmetic is line_extent.h's.  The rings are either the resident result of the
// handle's last contour call (contour_glue.hip: c->contour_tab, c->contour_pts), read in place, or a list the caller passes in.
#include <math.h>
#include <string.h>

#include "ctx.h"
#include "line_extent.h"
#include "line_split.h"

using namespace sbbseg;

static int extent_weights(std::vector<int64_t>& wtab)
{
    float tab[128];
    cubic_table(tab);
    wtab.resize((size_t)kExtentTabEntries);
    REQUIRE(extent_weight_table(tab, wtab.data()), "internal error: a bicubic weight is no multiple of 2^-34");
    return 0;
}

static int check_extent_box(const int32_t* b, int r)
{
    REQUIRE(b[2] >= 1 && b[3] >= 1 && b[2] <= 32767 && b[3] <= 32767 && b[0] >= 0 && b[1] >= 0 && b[0] <= (1 << 24) && b[1] <= (1 << 24),
            "region %d: box x %d, y %d, width %d, height %d (x, y >= 0; width and height 1 .. 32767)", r, b[0], b[1], b[2], b[3]);
    return 0;
}

static LineGeom extent_line_geom(int w, int h, const double* rot)
{
    LineGeom g;
    g.n = h; g.other = w; g.vertical = 0;
    g.r00 = rot[0]; g.r01 = rot[1]; g.r10 = rot[2]; g.r11 = rot[3]; g.xd = rot[4]; g.yd = rot[5];
    return g;
}

static void write_rec(const ExtentWinner& win, int32_t* rec)
{
    rec[kExtentRecStatus] = win.status; rec[kExtentRecBorders] = win.borders; rec[kExtentRecPoints] = win.n_points; rec[kExtentRecHole] = win.is_hole;
    rec[kExtentRecTie] = win.tie; rec[kExtentRecStartX] = win.sx; rec[kExtentRecStartY] = win.sy; rec[kExtentRecHoles] = win.holes;
}

struct HostEmit {
    int32_t* out;
    void operator()(int k, int x, int y) const { out[2 * (size_t)k] = x; out[2 * (size_t)k + 1] = y; }
};

// the serial scan of one bit map (box + ring) and the winner's points
static int host_border_winner(const std::vector<uint32_t>& pix, int w, int h, int32_t* rec, std::vector<int32_t>& winner)
{
    std::vector<uint32_t> vis(pix.size(), 0u), right(pix.size(), 0u);
    ExtentMap m;
    m.pix = pix.data(); m.vis = vis.data(); m.right = right.data(); m.stride = contour_bitmap_stride(w); m.w = w; m.h = h;
    const ExtentWinner win = extent_scan(m, ExtentSerialNext{&m});
    write_rec(win, rec);
    REQUIRE(win.status != kExtentBroken, "internal error: a border walk of a %d x %d mask did not close", w, h);
    winner.assign((size_t)win.n_points * 2, 0);
    if (win.status == kExtentOk) {
        const ContourResult res = contour_walk_from(ExtentNb{m.pix, m.stride}, win.sx, win.sy, win.is_hole ? 0 : 4, contour_step_bound((long long)w * h),
                                                    HostEmit{winner.data()}, ContourNoMark{});
        REQUIRE(res.status == kContourOk && res.n_points == win.n_points, "internal error: the winner's second walk differs from its first");
    }
    return 0;
}

static void pack_mask(const uint8_t* mask, int w, int h, uint32_t* pix)
{
    const int stride = contour_bitmap_stride(w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            if (mask[(size_t)y * w + x]) pix[(size_t)(y + 1) * stride + ((x + 1) >> 5)] |= 1u << ((x + 1) & 31);
}

static void unpack_mask(const uint32_t* pix, int w, int h, uint8_t* mask)
{
    const int stride = contour_bitmap_stride(w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) mask[(size_t)y * w + x] = ((pix[(size_t)(y + 1) * stride + ((x + 1) >> 5)] >> ((x + 1) & 31)) & 1u) ? 255 : 0;
}

// where the pieces of c->extent_tab lie for n regions and `lines` line slots
struct ExtentLayout {
    size_t off_at, rec_at, info_at, lines_at, extent_at, box_at, rot_at, total;
};
static ExtentLayout extent_layout(int n, size_t lines)
{
    ExtentLayout l;
    l.off_at = align16((size_t)n * sizeof(ExtentRegion));
    l.rec_at = l.off_at + align16(((size_t)n + 1) * sizeof(long long));
    l.info_at = l.rec_at + align16((size_t)n * kExtentRecInts * sizeof(int32_t));
    l.lines_at = l.info_at + align16((size_t)n * kLineInfoInts * sizeof(int32_t));
    l.extent_at = l.lines_at + align16(lines * 3 * sizeof(int32_t));
    l.box_at = l.extent_at + align16(lines * 2 * sizeof(int32_t));
    l.rot_at = l.box_at + align16(lines * 8 * sizeof(int32_t));
    l.total = l.rot_at + align16(lines * 8 * sizeof(int32_t));
    return l;
}

// The offsets of the bit maps, work items and mark planes of regions whose ox, oy, w, h are set; *any_lds / *any_global: which forms of the
// scan the call needs.
static int extent_place(sbbseg_ctx* c, std::vector<ExtentRegion>& regs, long long* bit_words, long long* mark_words, int* blocks, bool* any_lds,
                        bool* any_global)
{
    long long words = 0, marks = 0, nblocks = 0;
    *any_lds = *any_global = false;
    for (size_t r = 0; r < regs.size(); ++r) {
        ExtentRegion& g = regs[r];
        const long long map_words = contour_bitmap_bytes(g.w, g.h) / 4;
        g.src_off = (int)words;
        words += (long long)extent_src_stride(g.w) * g.h;
        g.dst_off = (int)words;
        words += map_words;
        g.block0 = (int)nblocks;
        nblocks += (g.h + kExtentRows - 1) / kExtentRows;
        g.mark_off = marks;
        g.win_off = 0;
        if (3 * map_words * 4 <= (long long)c->extent_lds_limit) *any_lds = true;
        else { *any_global = true; marks += 2 * map_words; }
        REQUIRE(words < (1ll << 30) && nblocks < (1ll << 30), "too much work for one call (%d regions): split the regions", (int)regs.size());
    }
    *bit_words = words; *mark_words = marks; *blocks = (int)nblocks;
    return 0;
}

// the two passes of the scan on bit maps that are in c->extent_bits: records to the host, winners' offsets, winners' points on the device
static int extent_scan_passes(sbbseg_ctx* c, ExtentParams& p, std::vector<ExtentRegion>& regs, long long mark_words, bool any_lds, bool any_global,
                              int32_t* rec)
{
    const int n = p.n_regions;
    if (mark_words) {
        if (ensure(c, c->extent_marks, (size_t)mark_words * 4)) return 1;
        HIPCHK(hipMemsetAsync(c->extent_marks.p, 0, (size_t)mark_words * 4, c->stream));
    }
    p.marks = c->extent_marks.p;
    p.winner = nullptr;
    HIPCHK(launch_extent_scan(p, any_lds, any_global, c->stream));
    HIPCHK(hipMemcpyAsync(rec, p.rec, (size_t)n * kExtentRecInts * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    long long pts = 0;
    c->extent_geom.assign((size_t)n * 5, 0);
    for (int r = 0; r < n; ++r) {
        int32_t* q = rec + (size_t)r * kExtentRecInts;
        REQUIRE(q[kExtentRecStatus] != kExtentBadRing,
                "region %d: its ring has an edge that is not horizontal, vertical or an exact diagonal, or a point outside its box", r);
        REQUIRE(q[kExtentRecStatus] == kExtentOk || q[kExtentRecStatus] == kExtentNone, "internal error: region %d: a border walk did not close", r);
        if (q[kExtentRecStatus] == kExtentNone)
            for (int i = 1; i < kExtentRecInts; ++i) q[i] = 0;
        regs[r].win_off = pts;
        int32_t* geo = c->extent_geom.data() + (size_t)r * 5;
        geo[0] = regs[r].w; geo[1] = regs[r].h; geo[2] = regs[r].dst_off; geo[3] = (int32_t)pts; geo[4] = q[kExtentRecPoints];
        pts += q[kExtentRecPoints];
        REQUIRE(pts < (1ll << 30), "too much work for one call (%d regions): split the regions", n);
    }
    if (ensure(c, c->extent_win, (size_t)(pts ? pts : 2) * 2 * sizeof(int32_t))) return 1;
    HIPCHK(hipMemcpyAsync((void*)p.regions, regs.data(), (size_t)n * sizeof(ExtentRegion), hipMemcpyHostToDevice, c->stream));
    p.winner = c->extent_win.p;
    HIPCHK(launch_extent_scan(p, any_lds, any_global, c->stream));
    c->extent_launches += 2 * ((any_lds ? 1 : 0) + (any_global ? 1 : 0));
    return 0;
}

extern "C" {

int sbbseg_region_line_extents_host(const int32_t* ring_xy, int n_points, const int32_t* box_xywh, double slope, const double* rot, int branch,
                                    const int32_t* lines, int n_lines, int32_t* extent, int32_t* corners, int32_t* corners_rot, int32_t* rec,
                                    uint8_t* threshrot, int32_t* winner_xy, int winner_cap)
{
    API_BEGIN
    REQUIRE(ring_xy && n_points >= 1 && box_xywh && rot && rec && n_lines >= 0 && (n_lines == 0 || (lines && extent && corners && corners_rot)),
            "bad arguments");
    if (check_extent_box(box_xywh, 0)) return 1;
    alloc_check();
    const int ox = box_xywh[0], oy = box_xywh[1], w = box_xywh[2], h = box_xywh[3];
    std::vector<int64_t> wtab;
    if (extent_weights(wtab)) return 1;
    std::vector<uint32_t> src((size_t)extent_src_stride(w) * h, 0u);
    REQUIRE(extent_fill_serial(ring_xy, n_points, ox, oy, w, h, src.data()),
            "region 0: its ring has an edge that is not horizontal, vertical or an exact diagonal, or a point outside its box");
    double m[6];
    if (line_inverse_map(h, w, slope, m)) return 1;
    const int stride = contour_bitmap_stride(w);
    std::vector<uint32_t> pix((size_t)(contour_bitmap_bytes(w, h) / 4), 0u);
    for (int y = 0; y < h; ++y) {
        long long X0, Y0;
        line_mask_row_origin(m, y, &X0, &Y0);
        for (int x = 0; x < w; ++x)
            if (extent_pixel(src.data(), w, h, m[0], m[3], X0, Y0, x, wtab.data()))
                pix[(size_t)(y + 1) * stride + ((x + 1) >> 5)] |= 1u << ((x + 1) & 31);
    }
    if (threshrot) unpack_mask(pix.data(), w, h, threshrot);
    std::vector<int32_t> winner;
    if (host_border_winner(pix, w, h, rec, winner)) return 1;
    if (winner_xy) {
        REQUIRE(winner_cap >= rec[kExtentRecPoints], "room for %d points, the winner has %d", winner_cap, rec[kExtentRecPoints]);
        memcpy(winner_xy, winner.data(), winner.size() * sizeof(int32_t));
    }
    const bool rewrite = !(fabs(slope) > 45.0) && rec[kExtentRecStatus] == kExtentOk && branch != kLineBranchOnePeak;
    const LineGeom g = extent_line_geom(w, h, rot);
    for (int j = 0; j < n_lines; ++j) {
        extent[2 * j] = 0; extent[2 * j + 1] = w;
        if (!rewrite) continue;
        extent_line_serial(winner.data(), rec[kExtentRecPoints], w, lines[3 * j], extent + 2 * j);
        line_box_with_extent(g, extent[2 * j], extent[2 * j + 1], lines[3 * j + 1], lines[3 * j + 2], corners + 8 * j, corners_rot + 8 * j);
    }
    return 0;
    API_END
}

int sbbseg_region_line_extents_dev(sbbseg_ctx* c, const int32_t* points_xy, const int64_t* point_off, int n, const int32_t* boxes_xywh,
                                   const double* slopes, const double* rot, const int32_t* info, const int64_t* line_off, const int32_t* lines,
                                   int32_t* extent, int32_t* corners, int32_t* corners_rot, int32_t* rec)
{
    API_BEGIN
    REQUIRE(n >= 0 && n <= (1 << 20), "bad arguments");
    if (n == 0) return 0;
    REQUIRE(boxes_xywh && slopes && rot && info && line_off && lines && extent && corners && corners_rot && rec, "bad arguments");
    if (check_ready(c)) return 1;
    alloc_check();
    std::vector<ExtentRegion> regs((size_t)n);
    REQUIRE(line_off[0] == 0, "line offsets start at 0");
    for (int r = 0; r < n; ++r) {
        const int32_t* b = boxes_xywh + (size_t)r * 4;
        if (check_extent_box(b, r)) return 1;
        ExtentRegion& g = regs[r];
        memset(&g, 0, sizeof(g));
        g.ox = b[0]; g.oy = b[1]; g.w = b[2]; g.h = b[3];
        g.vertical = fabs(slopes[r]) > 45.0 ? 1 : 0;
        REQUIRE(line_off[r + 1] - line_off[r] == line_capacity(g.vertical ? g.w : g.h) && line_off[r + 1] < (1ll << 27),
                "region %d: line offsets %lld .. %lld are not sbbseg_region_line_boxes' for its box", r, (long long)line_off[r], (long long)line_off[r + 1]);
        const int32_t* f = info + (size_t)r * kLineInfoInts;
        REQUIRE(f[kLineInfoStatus] != kLineOk || (f[kLineInfoCount] >= 0 && f[kLineInfoCount] <= line_off[r + 1] - line_off[r]), "region %d: %d lines", r,
                f[kLineInfoCount]);
        g.line_off = (int)line_off[r];
        if (line_inverse_map(g.h, g.w, slopes[r], g.minv)) return 1;
        memcpy(g.rot, rot + (size_t)r * 6, 6 * sizeof(double));
        g.step = (double)g.w / (double)(kExtentSamples - 1);
    }
    if (points_xy) {
        REQUIRE(point_off && point_off[0] == 0, "point offsets start at 0");
        for (int r = 0; r < n; ++r)
            REQUIRE(point_off[r + 1] > point_off[r] && point_off[r + 1] < (1ll << 30), "region %d: ring offsets %lld .. %lld (a ring has at least one point)", r,
                    (long long)point_off[r], (long long)point_off[r + 1]);
    } else {
        REQUIRE(c->contour_n >= 0, "no contours on this handle: the last contour call failed, or there was none");
        REQUIRE(n == c->contour_n, "the handle holds %d contours, the call names %d", c->contour_n, n);
    }
    long long bit_words = 0, mark_words = 0;
    int blocks = 0;
    bool any_lds = false, any_global = false;
    c->extent_n = -1;
    if (extent_place(c, regs, &bit_words, &mark_words, &blocks, &any_lds, &any_global)) return 1;
    const size_t total = (size_t)line_off[n];
    const ExtentLayout l = extent_layout(n, total);
    if (ensure(c, c->extent_tab, l.total) || ensure(c, c->extent_bits, (size_t)bit_words * 4)) return 1;
    if (!c->d_extent_wtab) {
        std::vector<int64_t> wtab;
        if (extent_weights(wtab)) return 1;
        if (upload(c, &c->d_extent_wtab, wtab.data(), wtab.size())) return 1;
    }
    unsigned char* d = (unsigned char*)c->extent_tab.p;
    ExtentParams p;
    memset(&p, 0, sizeof(p));
    p.regions = (const ExtentRegion*)d; p.n_regions = n; p.total_blocks = blocks; p.total_lines = (int)total; p.lds_limit = c->extent_lds_limit;
    p.bits = c->extent_bits.p; p.wtab = c->d_extent_wtab; p.rec = (int32_t*)(d + l.rec_at);
    p.info = (const int32_t*)(d + l.info_at); p.lines = (const int32_t*)(d + l.lines_at); p.extent = (int32_t*)(d + l.extent_at);
    p.box = (int32_t*)(d + l.box_at); p.rot = (int32_t*)(d + l.rot_at);
    if (points_xy) {
        static_assert(sizeof(int64_t) == sizeof(long long), "the offsets are uploaded as they are");
        if (ensure(c, c->extent_pts, (size_t)point_off[n] * 2 * sizeof(int32_t))) return 1;
        HIPCHK(hipMemcpyAsync(d + l.off_at, point_off, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->extent_pts.p, points_xy, (size_t)point_off[n] * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        p.points = c->extent_pts.p; p.point_off = (const long long*)(d + l.off_at);
    } else {
        p.points = c->contour_pts.p;
        p.point_off = (const long long*)((const unsigned char*)c->contour_tab.p + c->contour_off_at);
    }
    HIPCHK(hipMemcpyAsync(d, regs.data(), (size_t)n * sizeof(ExtentRegion), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d + l.info_at, info, (size_t)n * kLineInfoInts * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d + l.lines_at, lines, total * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->extent_bits.p, 0, (size_t)bit_words * 4, c->stream));          // (the rings of zeros round threshrot)
    HIPCHK(launch_extent_masks(p, c->stream));
    c->extent_launches += 2;
    if (extent_scan_passes(c, p, regs, mark_words, any_lds, any_global, rec)) return 1;
    HIPCHK(launch_extent_lines(p, c->stream));
    c->extent_launches += 1;
    std::vector<int32_t> stage(total * 18);
    HIPCHK(hipMemcpyAsync(stage.data(), p.extent, total * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stage.data() + total * 2, p.box, total * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stage.data() + total * 10, p.rot, total * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the host staging buffers live until here)
    // per region its first `count` lines: nothing beyond a count is written on the host, and corners only where the step rewrites them
    for (int r = 0; r < n; ++r) {
        const int32_t* f = info + (size_t)r * kLineInfoInts;
        if (f[kLineInfoStatus] != kLineOk) continue;
        const size_t at = (size_t)line_off[r], cnt = (size_t)f[kLineInfoCount];
        memcpy(extent + at * 2, stage.data() + at * 2, cnt * 2 * sizeof(int32_t));
        if (regs[r].vertical || rec[(size_t)r * kExtentRecInts + kExtentRecStatus] != kExtentOk || f[kLineInfoBranch] == kLineBranchOnePeak) continue;
        memcpy(corners + at * 8, stage.data() + total * 2 + at * 8, cnt * 8 * sizeof(int32_t));
        memcpy(corners_rot + at * 8, stage.data() + total * 10 + at * 8, cnt * 8 * sizeof(int32_t));
    }
    c->extent_n = n;
    return 0;
    API_END
}

int sbbseg_region_line_extents_read(sbbseg_ctx* c, int region, uint8_t* threshrot_hw, int32_t* winner_xy, int cap)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(c->extent_n >= 0, "no extents on this handle: the last extent call failed, or there was none");
    REQUIRE(region >= 0 && region < c->extent_n, "region %d: the handle holds %d", region, c->extent_n);
    alloc_check();
    const int32_t* geo = c->extent_geom.data() + (size_t)region * 5;
    if (threshrot_hw) {
        std::vector<uint32_t> pix((size_t)(contour_bitmap_bytes(geo[0], geo[1]) / 4));
        HIPCHK(hipMemcpy(pix.data(), c->extent_bits.p + geo[2], pix.size() * 4, hipMemcpyDeviceToHost));
        unpack_mask(pix.data(), geo[0], geo[1], threshrot_hw);
    }
    if (winner_xy) {
        REQUIRE(cap >= geo[4], "room for %d points, the winner has %d", cap, geo[4]);
        if (geo[4]) HIPCHK(hipMemcpy(winner_xy, c->extent_win.p + 2 * (size_t)geo[3], (size_t)geo[4] * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return 0;
    API_END
}

int sbbseg_debug_mask_border_winner_dev(sbbseg_ctx* c, const uint8_t* masks, const int32_t* wh, int n, int32_t* rec)
{
    API_BEGIN
    REQUIRE(n >= 0 && n <= (1 << 20) && (n == 0 || (masks && wh && rec)), "bad arguments");
    if (n == 0) return 0;
    if (check_ready(c)) return 1;
    alloc_check();
    std::vector<ExtentRegion> regs((size_t)n);
    for (int r = 0; r < n; ++r) {
        const int32_t b[4] = {0, 0, wh[2 * r], wh[2 * r + 1]};
        if (check_extent_box(b, r)) return 1;
        memset(&regs[r], 0, sizeof(ExtentRegion));
        regs[r].w = b[2]; regs[r].h = b[3];
    }
    long long bit_words = 0, mark_words = 0;
    int blocks = 0;
    bool any_lds = false, any_global = false;
    c->extent_n = -1;
    if (extent_place(c, regs, &bit_words, &mark_words, &blocks, &any_lds, &any_global)) return 1;
    const ExtentLayout l = extent_layout(n, 0);
    if (ensure(c, c->extent_tab, l.total) || ensure(c, c->extent_bits, (size_t)bit_words * 4)) return 1;
    std::vector<uint32_t> bits((size_t)bit_words, 0u);
    std::vector<int32_t> rec0((size_t)n * kExtentRecInts, 0);       // (status kExtentOk: there is no ring to be bad)
    size_t at = 0;
    for (int r = 0; r < n; ++r) {
        pack_mask(masks + at, regs[r].w, regs[r].h, bits.data() + regs[r].dst_off);
        at += (size_t)regs[r].w * regs[r].h;
    }
    unsigned char* d = (unsigned char*)c->extent_tab.p;
    ExtentParams p;
    memset(&p, 0, sizeof(p));
    p.regions = (const ExtentRegion*)d; p.n_regions = n; p.lds_limit = c->extent_lds_limit; p.bits = c->extent_bits.p; p.rec = (int32_t*)(d + l.rec_at);
    HIPCHK(hipMemcpyAsync(d, regs.data(), (size_t)n * sizeof(ExtentRegion), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(p.rec, rec0.data(), rec0.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(p.bits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (extent_scan_passes(c, p, regs, mark_words, any_lds, any_global, rec)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->extent_n = n;
    return 0;
    API_END
}

int sbbseg_debug_mask_border_winner_host(const uint8_t* mask, int w, int h, int32_t* rec, int32_t* winner_xy, int cap)
{
    API_BEGIN
    REQUIRE(mask && rec, "bad arguments");
    const int32_t b[4] = {0, 0, w, h};
    if (check_extent_box(b, 0)) return 1;
    alloc_check();
    std::vector<uint32_t> pix((size_t)(contour_bitmap_bytes(w, h) / 4), 0u);
    pack_mask(mask, w, h, pix.data());
    std::vector<int32_t> winner;
    if (host_border_winner(pix, w, h, rec, winner)) return 1;
    if (winner_xy) {
        REQUIRE(cap >= rec[kExtentRecPoints], "room for %d points, the winner has %d", cap, rec[kExtentRecPoints]);
        memcpy(winner_xy, winner.data(), winner.size() * sizeof(int32_t));
    }
    return 0;
    API_END
}

int sbbseg_region_line_extent_weights(int64_t* wtab, int capacity)
{
    API_BEGIN
    REQUIRE(wtab && capacity >= kExtentTabEntries, "room for %d weights, the table has %d", capacity, kExtentTabEntries);
    alloc_check();
    std::vector<int64_t> t;
    if (extent_weights(t)) return 1;
    memcpy(wtab, t.data(), t.size() * sizeof(int64_t));
    return 0;
    API_END
}

int sbbseg_debug_set_extent_lds_limit(sbbseg_ctx* c, int bytes)
{
    API_BEGIN
    REQUIRE(c && bytes >= 0 && bytes <= kExtentLdsBytes, "the limit is 0 .. %d bytes", kExtentLdsBytes);
    c->extent_lds_limit = bytes;
    return 0;
    API_END
}

int sbbseg_debug_extent_launches(sbbseg_ctx* c, int64_t* value)
{
    API_BEGIN
    REQUIRE(c && value, "bad arguments");
    *value = (int64_t)c->extent_launches;
    return 0;
    API_END
}

}  // extern "C"
