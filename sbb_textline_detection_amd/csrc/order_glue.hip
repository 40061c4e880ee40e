// order_glue.hip -- host side of the reading order of a page's text regions (order_of_regions, main.py:1802-1889): the C ABI entry points
// (include/sbbseg.h) of the contour moments and the region order on the device (order.hip), and their serial host twins (order.h).  The
// contours are either the resident result of the handle's last contour call (contour_glue.hip: c->contour_tab, c->contour_pts), read in
// place, or a list the caller passes in.
#include <string.h>

#include "ctx.h"
#include "order.h"

using namespace sbbseg;

// a contour list of the caller's: n >= 0 contours, contour r = points point_off[r] .. point_off[r + 1] of points_xy
static int check_point_list(const int32_t* points_xy, const int64_t* point_off, int n)
{
    REQUIRE(n >= 0 && n <= (1 << 20) && (point_off || n == 0), "bad arguments");
    if (n == 0) return 0;
    REQUIRE(point_off[0] == 0, "point offsets start at 0");
    for (int r = 0; r < n; ++r)
        REQUIRE(point_off[r + 1] >= point_off[r] && point_off[r + 1] - point_off[r] < (1ll << 31), "contour %d: offsets %lld .. %lld", r,
                (long long)point_off[r], (long long)point_off[r + 1]);
    REQUIRE(points_xy || point_off[n] == 0, "bad arguments");
    return 0;
}

// where the pieces of c->order_buf lie for a plane of H rows and n contours
struct OrderLayout {
    size_t off_at, n_edges_at, edges_at, sorted_at, order_at, band_at, serial_at, cent_at, mom_at, sums_at, smooth_at, w_at, total;
};
static OrderLayout order_layout(int H, int n)
{
    OrderLayout l;
    const size_t cap = (size_t)order_edge_capacity(H), nn = (size_t)n;
    l.off_at = 0;
    l.n_edges_at = align16((nn + 1) * sizeof(long long));
    l.edges_at = l.n_edges_at + 16;
    l.sorted_at = l.edges_at + align16(cap * sizeof(int32_t));
    l.order_at = l.sorted_at + align16(nn * sizeof(int32_t));
    l.band_at = l.order_at + align16(nn * sizeof(int32_t));
    l.serial_at = l.band_at + align16(nn * sizeof(int32_t));
    l.cent_at = l.serial_at + align16(nn * sizeof(int32_t));
    l.mom_at = l.cent_at + nn * 2 * sizeof(double);
    l.sums_at = l.mom_at + align16(nn * 3 * sizeof(double));
    l.smooth_at = l.sums_at + align16((size_t)H * sizeof(int32_t));
    l.w_at = l.smooth_at + align16(((size_t)H + 4 * kOrderPad) * sizeof(double));
    l.total = l.w_at + align16((kOrderRadius + 1) * sizeof(double));
    return l;
}

// c->order_buf for (H, n) and the contours in *p: the resident result (points_xy == nullptr) in place, or the caller's list uploaded
static int order_prepare(sbbseg_ctx* c, int H, const int32_t* points_xy, const int64_t* point_off, int n, OrderParams* p, OrderLayout* l)
{
    *l = order_layout(H, n);
    if (ensure(c, c->order_buf, l->total)) return 1;
    unsigned char* d = (unsigned char*)c->order_buf.p;
    memset(p, 0, sizeof(*p));
    p->H = H; p->n = n; p->radius = kOrderRadius;
    p->n_edges = (int32_t*)(d + l->n_edges_at); p->edges = (int32_t*)(d + l->edges_at);
    p->sorted_index = (int32_t*)(d + l->sorted_at); p->order = (int32_t*)(d + l->order_at); p->band = (int32_t*)(d + l->band_at);
    p->serial = (int32_t*)(d + l->serial_at); p->centroids = (double*)(d + l->cent_at); p->moments = (double*)(d + l->mom_at);
    p->row_sums = (int32_t*)(d + l->sums_at); p->smooth = (double*)(d + l->smooth_at); p->weights = (const double*)(d + l->w_at);
    if (n == 0) return 0;
    if (!points_xy) {
        REQUIRE(c->contour_n >= 0, "no contours on this handle: the last contour call failed, or there was none");
        REQUIRE(n == c->contour_n, "the handle holds %d contours, the call names %d", c->contour_n, n);
        p->points = c->contour_pts.p;
        p->point_off = (const long long*)((const unsigned char*)c->contour_tab.p + c->contour_off_at);
        return 0;
    }
    static_assert(sizeof(int64_t) == sizeof(long long), "the offsets are uploaded as they are");
    const size_t np = (size_t)point_off[n];
    if (np && ensure(c, c->order_pts, np * 2 * sizeof(int32_t))) return 1;
    HIPCHK(hipMemcpyAsync(d + l->off_at, point_off, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (np) HIPCHK(hipMemcpyAsync(c->order_pts.p, points_xy, np * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    p->points = c->order_pts.p;
    p->point_off = (const long long*)(d + l->off_at);
    return 0;
}

static int region_order_dev(sbbseg_ctx* c, const void* d_plane_hw, int H, int W, const double* weights, const int32_t* points_xy,
                            const int64_t* point_off, int n, int32_t* sorted_index, int32_t* order, int32_t* band, double* centroids, int32_t* edges,
                            int cap, int* n_edges)
{
    REQUIRE(d_plane_hw && weights && edges && n_edges && H > 0 && W > 0, "bad arguments");
    REQUIRE(H <= (1 << 24) && W <= (1 << 23), "plane of %d x %d: at most 2^24 rows of 2^23 bytes (a row sum must fit 32 bits)", H, W);
    REQUIRE(cap >= order_edge_capacity(H), "room for %d edges, a plane of %d rows can have %d", cap, H, order_edge_capacity(H));
    REQUIRE(n == 0 || (sorted_index && order && band && centroids), "bad arguments");
    if (points_xy || n == 0) {
        if (check_point_list(points_xy, point_off, n)) return 1;
    } else {
        REQUIRE(n > 0, "bad arguments");
    }
    OrderParams p;
    OrderLayout l;
    if (order_prepare(c, H, points_xy, point_off, n, &p, &l)) return 1;
    p.plane = (const uint8_t*)d_plane_hw; p.W = W;
    HIPCHK(hipMemcpyAsync((void*)p.weights, weights, (kOrderRadius + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_row_sums(p, c->stream));
    HIPCHK(launch_order_edges(p, c->stream));
    c->order_launches += 2;
    if (n) {
        HIPCHK(launch_contour_moments(p, c->stream));
        HIPCHK(launch_order_rank(p, c->stream));
        c->order_launches += 2;
        HIPCHK(hipMemcpyAsync(sorted_index, p.sorted_index, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(order, p.order, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(band, p.band, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(centroids, p.centroids, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    int32_t ne = 0;
    HIPCHK(hipMemcpyAsync(&ne, p.n_edges, sizeof(ne), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the caller's tables live until here)
    REQUIRE(ne >= 2 && ne <= order_edge_capacity(H), "internal error: %d edges, room for %d", ne, order_edge_capacity(H));
    HIPCHK(hipMemcpy(edges, p.edges, (size_t)ne * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_edges = ne;
    return 0;
}

extern "C" {

int sbbseg_contour_moments_dev(sbbseg_ctx* c, const int32_t* points_xy, const int64_t* point_off, int n, double* moments, double* centroids,
                               int32_t* serial)
{
    API_BEGIN
    REQUIRE(n >= 0 && ((moments && centroids) || n == 0), "bad arguments");
    if (points_xy || n == 0) {
        if (check_point_list(points_xy, point_off, n)) return 1;
    }
    if (n == 0) return 0;
    if (check_ready(c)) return 1;
    OrderParams p;
    OrderLayout l;
    if (order_prepare(c, 1, points_xy, point_off, n, &p, &l)) return 1;
    HIPCHK(launch_contour_moments(p, c->stream));
    c->order_launches += 1;
    HIPCHK(hipMemcpyAsync(moments, p.moments, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(centroids, p.centroids, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (serial) HIPCHK(hipMemcpyAsync(serial, p.serial, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_contour_moments_host(const int32_t* points_xy, const int64_t* point_off, int n, double* moments, double* centroids, int32_t* serial)
{
    API_BEGIN
    REQUIRE(n >= 0 && ((moments && centroids) || n == 0), "bad arguments");
    if (check_point_list(points_xy, point_off, n)) return 1;
    for (int r = 0; r < n; ++r) {
        bool exact = true;
        const OrderMoments m = moments_serial(points_xy + 2 * point_off[r], (long long)(point_off[r + 1] - point_off[r]), &exact);
        moments[3 * (size_t)r] = m.m00; moments[3 * (size_t)r + 1] = m.m10; moments[3 * (size_t)r + 2] = m.m01;
        centroids[2 * (size_t)r] = m.cx; centroids[2 * (size_t)r + 1] = m.cy;
        if (serial) serial[r] = exact ? 0 : 1;
    }
    return 0;
    API_END
}

int sbbseg_region_order_dev(sbbseg_ctx* c, const void* d_plane_hw, int H, int W, const double* weights, const int32_t* points_xy,
                            const int64_t* point_off, int n, int32_t* sorted_index, int32_t* order, int32_t* band, double* centroids, int32_t* edges,
                            int cap, int* n_edges)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return region_order_dev(c, d_plane_hw, H, W, weights, points_xy, point_off, n, sorted_index, order, band, centroids, edges, cap, n_edges);
    API_END
}

int sbbseg_region_order(sbbseg_ctx* c, const uint8_t* plane_hw, int H, int W, const double* weights, const int32_t* points_xy,
                        const int64_t* point_off, int n, int32_t* sorted_index, int32_t* order, int32_t* band, double* centroids, int32_t* edges,
                        int cap, int* n_edges)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    const void* d_plane;
    if (stage_plane(c, plane_hw, H, W, true, &d_plane)) return 1;
    return region_order_dev(c, d_plane, H, W, weights, points_xy, point_off, n, sorted_index, order, band, centroids, edges, cap, n_edges);
    API_END
}

int sbbseg_region_order_host(const int32_t* row_sums, int H, const double* weights, const int32_t* points_xy, const int64_t* point_off, int n,
                             int32_t* sorted_index, int32_t* order, int32_t* band, double* centroids, int32_t* edges, int cap, int* n_edges)
{
    API_BEGIN
    REQUIRE(row_sums && weights && edges && n_edges && H > 0 && H <= (1 << 24), "bad arguments");
    REQUIRE(cap >= order_edge_capacity(H), "room for %d edges, a plane of %d rows can have %d", cap, H, order_edge_capacity(H));
    REQUIRE(n == 0 || (sorted_index && order && band && centroids), "bad arguments");
    if (check_point_list(points_xy, point_off, n)) return 1;
    alloc_check();
    std::vector<double> z((size_t)H + 4 * kOrderPad);
    const int ne = order_edges_serial(row_sums, H, weights, z.data(), edges);
    *n_edges = ne;
    for (int r = 0; r < n; ++r) {
        const OrderMoments m = moments_serial(points_xy + 2 * point_off[r], (long long)(point_off[r + 1] - point_off[r]), nullptr);
        centroids[2 * (size_t)r] = m.cx; centroids[2 * (size_t)r + 1] = m.cy;
    }
    order_rank_serial(edges, ne, centroids, n, sorted_index, order, band);
    return 0;
    API_END
}

int sbbseg_debug_row_sums(sbbseg_ctx* c, const uint8_t* plane_hw, int H, int W, int32_t* row_sums)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(row_sums && H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 23), "bad arguments");
    const void* d_plane;
    if (stage_plane(c, plane_hw, H, W, true, &d_plane)) return 1;
    OrderParams p;
    OrderLayout l;
    if (order_prepare(c, H, nullptr, nullptr, 0, &p, &l)) return 1;
    p.plane = (const uint8_t*)d_plane; p.W = W;
    HIPCHK(launch_row_sums(p, c->stream));
    c->order_launches += 1;
    HIPCHK(hipMemcpyAsync(row_sums, p.row_sums, (size_t)H * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_debug_order_launches(sbbseg_ctx* c, int64_t* value)
{
    API_BEGIN
    REQUIRE(c && value, "bad arguments");
    *value = (int64_t)c->order_launches;
    return 0;
    API_END
}

}  // extern "C"
