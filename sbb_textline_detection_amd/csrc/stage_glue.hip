// stage_glue.hip -- host side of libsbbseg's stage glue: the C ABI entry points (include/sbbseg.h) of what the reference does between
// and after its models -- morphology, the deskew sweeps and their statistic, deskewed line masks, the line split (components, boxes and
// contours: contour_glue.hip).  Each stage checks its arguments, lays its tables out in one staging buffer and queues its kernels on the
// handle (ctx.h).
#include <string.h>
#include <algorithm>
#include <cmath>

#include "ctx.h"
#include "profile_stat.h"
#include "line_mask.h"
#include "line_split.h"

using namespace sbbseg;

extern "C" {

// ------------------------------------------------------------------------------ stage glue (8f-3)
int sbbseg_morph_dev(sbbseg_ctx* c, const void* d_src_hw, int H, int W, int op, int ksize, int iterations, void* d_dst_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_src_hw && d_dst_hw && H > 0 && W > 0, "bad arguments");
    REQUIRE((op == SBBSEG_MORPH_ERODE || op == SBBSEG_MORPH_DILATE) && ksize >= 1 && (ksize & 1) && iterations >= 1, "morph: op 0|1, odd kernel, iterations >= 1");
    const size_t pix = (size_t)H * W;
    if (ensure(c, c->morph_a, pix)) return 1;
    HIPCHK(launch_morph((const uint8_t*)d_src_hw, c->morph_a.p, (uint8_t*)d_dst_hw, H, W, (ksize - 1) / 2 * iterations, op == SBBSEG_MORPH_DILATE, 0, c->stream));
    return 0;
    API_END
}

int sbbseg_morph(sbbseg_ctx* c, const uint8_t* src_hw, int H, int W, int op, int ksize, int iterations, uint8_t* dst_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(dst_hw, "bad arguments");
    const void* d_plane;
    if (stage_plane(c, src_hw, H, W, true, &d_plane)) return 1;
    if (sbbseg_morph_dev(c, d_plane, H, W, op, ksize, iterations, c->morph_b.p)) return 1;          // in place
    HIPCHK(hipMemcpyAsync(dst_hw, c->morph_b.p, (size_t)H * W, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

// ---- stage glue: the rotate-and-project of the deskew search (main.py:1601-1718) ----------------------------------
int sbbseg_deskew_side(int H, int W, int* side)
{
    API_BEGIN
    REQUIRE(side && H > 0 && W > 0, "bad arguments");
    *side = (int)((double)(H > W ? H : W) * 1.4);              // main.py:1613  int(max_x_y * (1.4))
    return 0;
    API_END
}

// cv2.getRotationMatrix2D(center, angle, 1.0) [EXT OpenCV 4.5.1]: positive angle = counter-clockwise
int sbbseg_rotation_matrix(double cx, double cy, double angle_deg, double* m6)
{
    API_BEGIN
    REQUIRE(m6, "bad arguments");
    const double a = angle_deg * 3.14159265358979323846 / 180.0;
    const double alpha = std::cos(a), beta = std::sin(a);
    m6[0] = alpha; m6[1] = beta; m6[2] = (1 - alpha) * cx - beta * cy;
    m6[3] = -beta; m6[4] = alpha; m6[5] = beta * cx + (1 - alpha) * cy;
    return 0;
    API_END
}

static void invert_affine(const double* M, double* o)
{
#pragma clang fp contract(off)
    // the in-place inversion of cv::warpAffine (no WARP_INVERSE_MAP), same operation order
    double m[6] = {M[0], M[1], M[2], M[3], M[4], M[5]};
    double D = m[0] * m[4] - m[1] * m[3];
    D = D != 0 ? 1.0 / D : 0.0;
    const double A11 = m[4] * D, A22 = m[0] * D;
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22;
    const double b1 = -m[0] * m[2] - m[1] * m[5];
    const double b2 = -m[3] * m[2] - m[4] * m[5];
    m[2] = b1; m[5] = b2;
    for (int i = 0; i < 6; ++i) o[i] = m[i];
}

extern "C++" {
namespace sbbseg {
void cubic_table(float* tab)
{
#pragma clang fp contract(off)
    // interpolateCubic of imgwarp.cpp, A = -0.75, float arithmetic
    const float A = -0.75f;
    for (int i = 0; i < 32; ++i) {
        const float x = (float)i * (1.0f / 32);
        float* c = tab + i * 4;
        c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
        c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
        c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
        c[3] = 1.f - c[0] - c[1] - c[2];
    }
}
}  // namespace sbbseg
}  // extern "C++"

int sbbseg_deskew_profiles_dev(sbbseg_ctx* c, const void* d_mask_hw, int H, int W, const double* matrices, const double* angles_deg,
                               int n_angles, int32_t* counts)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_mask_hw && counts && H > 0 && W > 0 && n_angles >= 1 && n_angles <= 4096 && (matrices || angles_deg), "bad arguments");
    const int S = (int)((double)(H > W ? H : W) * 1.4);
    REQUIRE(S >= 1 && S <= 32767, "deskew square side %d out of range", S);
    const int cp = (int)(S / 2.0), top = cp - (int)(H / 2.0), left = cp - (int)(W / 2.0);      // main.py:1615-1619
    alloc_check();
    std::vector<double> minv((size_t)n_angles * 6);
    for (int a = 0; a < n_angles; ++a) {
        double M[6];
        if (matrices) memcpy(M, matrices + (size_t)a * 6, sizeof(M));
        else if (sbbseg_rotation_matrix((double)(S / 2), (double)(S / 2), angles_deg[a], M)) return 1;     // main.py:161  center = (w // 2, h // 2)
        invert_affine(M, &minv[(size_t)a * 6]);
    }
    float tab[128];
    cubic_table(tab);
    const size_t need = (size_t)n_angles * 6 * sizeof(double) + sizeof(tab) + (size_t)n_angles * S * sizeof(int);
    if (ensure(c, c->deskew, need)) return 1;
    double* d_minv = (double*)c->deskew.p;
    float* d_tab = (float*)(d_minv + (size_t)n_angles * 6);
    int* d_counts = (int*)(d_tab + 128);
    HIPCHK(hipMemcpyAsync(d_minv, minv.data(), minv.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_tab, tab, sizeof(tab), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (pageable host staging buffers die with this frame)
    HIPCHK(launch_deskew_profiles((const uint8_t*)d_mask_hw, H, W, S, top, left, d_minv, d_tab, n_angles, d_counts, c->stream));
    HIPCHK(hipMemcpyAsync(counts, d_counts, (size_t)n_angles * S * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_deskew_profiles(sbbseg_ctx* c, const uint8_t* mask_hw, int H, int W, const double* matrices, const double* angles_deg, int n_angles,
                           int32_t* counts)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    const void* d_plane;
    if (stage_plane(c, mask_hw, H, W, true, &d_plane)) return 1;
    return sbbseg_deskew_profiles_dev(c, d_plane, H, W, matrices, angles_deg, n_angles, counts);
    API_END
}

// Where the boxes of a per-box call lie: box r on planes[box_plane[r]] (pooled), or every box on planes[0] -- the one-plane entry points'
// form, a table of one plane.
struct PlaneSet {
    const sbbseg_plane* planes;
    int n_planes;
    const int32_t* box_plane;
    bool pooled;
};
static PlaneSet one_plane(sbbseg_plane* pl, const void* d_hw, int H, int W)
{
    pl->d_hw = d_hw; pl->H = H; pl->W = W;
    return PlaneSet{pl, 1, nullptr, false};
}

static int check_plane_set(const PlaneSet& ps, int n_boxes)
{
    if (!ps.pooled) {
        REQUIRE(ps.planes[0].H > 0 && ps.planes[0].W > 0, "bad arguments");
        return 0;
    }
    REQUIRE(n_boxes <= 0 || (ps.planes && ps.box_plane), "bad arguments");
    REQUIRE(n_boxes <= 0 || ps.n_planes >= 1, "%d boxes but %d planes (at least one plane is needed)", n_boxes, ps.n_planes);
    return 0;
}

// The checks every per-box entry point makes on box r, the crop part of its DeskewRegion (what launch_region_deskew_crops reads;
// crop_image_inside_box; the rest of *g is zeroed) and the record of the plane it is cropped from.
static int crop_region(const PlaneSet& ps, const int32_t* boxes_xywh, int r, long long crop_off, DeskewRegion* g, DeskewPlane* src)
{
    const int32_t* b = boxes_xywh + (size_t)r * 4;
    const int k = ps.pooled ? ps.box_plane[r] : 0;
    REQUIRE(k >= 0 && k < ps.n_planes, "box %d: plane %d out of range (0 .. %d)", r, k, ps.n_planes - 1);
    const sbbseg_plane& pl = ps.planes[k];
    REQUIRE(b[2] >= 1 && b[3] >= 1, "box %d: width %d, height %d (both must be at least 1)", r, b[2], b[3]);
    const bool inside = b[0] >= 0 && b[1] >= 0 && (long long)b[0] + b[2] <= pl.W && (long long)b[1] + b[3] <= pl.H;
    if (ps.pooled) {
        REQUIRE(inside, "box %d (%d, %d, %d, %d) leaves the %d x %d plane %d", r, b[0], b[1], b[2], b[3], pl.W, pl.H, k);
        REQUIRE(pl.d_hw, "box %d: plane %d has no device pointer", r, k);
    } else {
        REQUIRE(inside, "box %d (%d, %d, %d, %d) leaves the %d x %d plane", r, b[0], b[1], b[2], b[3], pl.W, pl.H);
    }
    memset(g, 0, sizeof(*g));
    g->x = b[0]; g->y = b[1]; g->w = b[2]; g->h = b[3]; g->crop_off = crop_off;
    src->base = (const uint8_t*)pl.d_hw; src->W = pl.W; src->H = pl.H;
    return 0;
}

// The same sweep for every text-region box of a page (do_work_of_slopes, main.py:1728-1738): crop_image_inside_box, cv2.erode(crop, 5x5,
// iterations) on the CROP, return_deskew_slope's square and rotations.  offsets[r] = first int of region r in the packed counts
// ([n_angles][S_r]), offsets[n_boxes] = the total.  size_only: only the offsets are computed (needs no handle).  Otherwise the sweep is
// queued on the stream and *d_counts points at the packed counts in the handle's buffer: they STAY on the device.  `head` is the host
// staging buffer of the tables: the caller keeps it alive until it has synchronised the stream.
static int region_sweep(sbbseg_ctx* c, const PlaneSet& ps, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                        const double* angles_deg, int n_angles, int64_t* offsets, bool size_only, std::vector<unsigned char>& head,
                        const int32_t** d_counts)
{
    *d_counts = nullptr;
    REQUIRE(n_boxes >= 0 && n_boxes <= (1 << 20) && (boxes_xywh || n_boxes == 0) && offsets && n_angles >= 1 && n_angles <= 4096 &&
                erode_iterations >= 0 && erode_iterations <= 64, "bad arguments");
    if (check_plane_set(ps, n_boxes)) return 1;
    alloc_check();
    std::vector<DeskewRegion> geom((size_t)n_boxes);
    std::vector<DeskewPlane> src((size_t)n_boxes);
    long long total_pix = 0, total_counts = 0, total_blocks = 0;
    for (int r = 0; r < n_boxes; ++r) {
        DeskewRegion& g = geom[r];
        if (crop_region(ps, boxes_xywh, r, total_pix, &g, &src[r])) return 1;
        g.S = (int)((double)(g.h > g.w ? g.h : g.w) * 1.4);                               // main.py:1613
        REQUIRE(g.S >= 1 && g.S <= 32767, "box %d: deskew square side %d out of range", r, g.S);
        const int cp = (int)(g.S / 2.0);
        g.top = cp - (int)(g.h / 2.0); g.left = cp - (int)(g.w / 2.0);                    // main.py:1615-1619
        g.clip = (g.top >= 1 && g.left >= 1 && g.top + g.h <= g.S - 1 && g.left + g.w <= g.S - 1) ? 1 : 0;
        g.count_off = total_counts;
        g.row_groups = (g.S + kRegionDeskewRows - 1) / kRegionDeskewRows;
        g.block0 = (int)total_blocks;
        offsets[r] = total_counts;
        total_pix += (long long)g.w * g.h;
        total_counts += (long long)n_angles * g.S;
        total_blocks += (long long)n_angles * g.row_groups;
        REQUIRE(total_counts < (1ll << 31) && total_blocks < (1ll << 31), "too much work for one sweep (%d boxes, %d angles): split the boxes", n_boxes, n_angles);
    }
    offsets[n_boxes] = total_counts;
    if (size_only || n_boxes == 0) return 0;                       // (the size query needs no handle)
    if (check_ready(c)) return 1;
    REQUIRE((ps.pooled || ps.planes[0].d_hw) && angles_deg, "bad arguments");
    // head of the device buffer, built on the host and copied in one piece: inverse maps | bicubic table | geometry | planes
    const size_t minv_bytes = (size_t)n_boxes * n_angles * 6 * sizeof(double), tab_bytes = 128 * sizeof(float);
    const size_t geom_off = minv_bytes + tab_bytes, src_off = geom_off + (size_t)n_boxes * sizeof(DeskewRegion);
    const size_t head_bytes = align16(src_off + (size_t)n_boxes * sizeof(DeskewPlane));
    const size_t pix_bytes = align16((size_t)total_pix);
    head.assign(head_bytes, 0);
    double* minv = (double*)head.data();
    for (int r = 0; r < n_boxes; ++r)
        for (int a = 0; a < n_angles; ++a) {
            double M[6];
            if (sbbseg_rotation_matrix((double)(geom[r].S / 2), (double)(geom[r].S / 2), angles_deg[a], M)) return 1;     // main.py:161
            invert_affine(M, minv + ((size_t)r * n_angles + a) * 6);
        }
    cubic_table((float*)(head.data() + minv_bytes));
    memcpy(head.data() + geom_off, geom.data(), (size_t)n_boxes * sizeof(DeskewRegion));
    memcpy(head.data() + src_off, src.data(), (size_t)n_boxes * sizeof(DeskewPlane));
    if (ensure(c, c->rdk, head_bytes + 2 * pix_bytes + (size_t)total_counts * sizeof(int))) return 1;
    unsigned char* d = (unsigned char*)c->rdk.p;
    RegionDeskewParams p;
    p.planes = (const DeskewPlane*)(d + src_off);
    p.geom = (const DeskewRegion*)(d + geom_off); p.n_regions = n_boxes; p.n_angles = n_angles; p.radius = 2 * erode_iterations;
    p.total_pix = total_pix;
    p.minv = (const double*)d; p.cubic = (const float*)(d + minv_bytes);
    p.tmp = d + head_bytes; p.crops = d + head_bytes + pix_bytes; p.counts = (int*)(d + head_bytes + 2 * pix_bytes);
    p.total_blocks = (int)total_blocks;
    HIPCHK(hipMemcpyAsync(d, head.data(), head_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_region_deskew_crops(p, c->stream));
    HIPCHK(launch_region_deskew_profiles(p, c->stream));
    c->slope_launches += 3;
    *d_counts = p.counts;
    return 0;
}

// counts == NULL: only the offsets are computed (to size the buffer).
int sbbseg_region_deskew_profiles_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                      int erode_iterations, const double* angles_deg, int n_angles, int32_t* counts, int64_t* offsets)
{
    API_BEGIN
    std::vector<unsigned char> head;
    const int32_t* d_counts = nullptr;
    sbbseg_plane pl;
    if (region_sweep(c, one_plane(&pl, d_textline_hw, H, W), boxes_xywh, n_boxes, erode_iterations, angles_deg, n_angles, offsets, !counts, head, &d_counts)) return 1;
    if (!d_counts) return 0;
    HIPCHK(hipMemcpyAsync(counts, d_counts, (size_t)offsets[n_boxes] * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the host staging buffer lives until here)
    return 0;
    API_END
}

int sbbseg_region_deskew_profiles(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                  int erode_iterations, const double* angles_deg, int n_angles, int32_t* counts, int64_t* offsets)
{
    API_BEGIN
    const void* d_plane;
    if (stage_plane(c, textline_hw, H, W, counts && n_boxes > 0, &d_plane)) return 1;
    return sbbseg_region_deskew_profiles_dev(c, d_plane, H, W, boxes_xywh, n_boxes, erode_iterations, angles_deg, n_angles, counts, offsets);
    API_END
}

// ---- stage glue: the 1-D statistic of the deskew search and the angle selection (main.py:1545-1599, 1630-1716; profile_stat.h) ----
static const double kSigma2Weights[kSigma2Radius + 1] = SBBSEG_SIGMA2_WEIGHTS;

// np.linspace(start, stop, num) bit for bit: i * ((stop - start) / (num - 1)) + start, the last one = stop
static void linspace(double start, double stop, int num, double* out)
{
#pragma clang fp contract(off)
    const double step = (stop - start) / (double)(num - 1);
    for (int i = 0; i < num; ++i) {
        const double t = (double)i * step;
        out[i] = t + start;
    }
    out[num - 1] = stop;
}

// the two sweeps of return_deskew_slope: np.linspace(-25, 25, 80) (main.py:1622) and, for a steep winner, np.linspace(-90, -50, 30) (main.py:1670)
static constexpr struct { double start, stop; int n; } kSweeps[2] = {{-25.0, 25.0, 80}, {-90.0, -50.0, 30}};
static void sweep_angles(int sweep, double* out) { linspace(kSweeps[sweep].start, kSweeps[sweep].stop, kSweeps[sweep].n, out); }

int sbbseg_deskew_sweep_angles(int sweep, double* angles_deg, int capacity, int* n_angles)
{
    API_BEGIN
    REQUIRE((sweep == 0 || sweep == 1) && n_angles && (angles_deg || capacity == 0) && capacity >= 0, "bad arguments");
    const int n = kSweeps[sweep].n;
    *n_angles = n;
    if (capacity == 0) return 0;
    REQUIRE(capacity >= n, "room for %d angles, the sweep has %d", capacity, n);
    sweep_angles(sweep, angles_deg);
    return 0;
    API_END
}

static int check_profile_tables(const int64_t* offsets, int n_regions, int n_angles, int radius)
{
    REQUIRE(n_regions >= 0 && n_regions <= (1 << 20) && (offsets || n_regions == 0), "bad arguments");
    REQUIRE(n_angles >= 1 && n_angles <= 4096, "n_angles %d out of range (1 .. 4096)", n_angles);
    REQUIRE(radius >= 0 && radius <= (1 << 16), "radius %d out of range (0 .. 65536)", radius);
    for (int r = 0; r < n_regions; ++r) {
        const int64_t len = offsets[r + 1] - offsets[r];
        REQUIRE(offsets[r] >= 0 && len >= n_angles && len % n_angles == 0 && len / n_angles <= 32767 && offsets[r + 1] < (1ll << 31),
                "region %d: offsets %lld .. %lld do not hold %d profiles of 1 .. 32767 samples", r, (long long)offsets[r], (long long)offsets[r + 1], n_angles);
    }
    return 0;
}

// the serial host twin on every profile of a sweep (checked arguments); smooth and below are optional
static void profile_stats_serial(const int32_t* counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights, int radius,
                                 double multiplier, double* spread, uint8_t* state, int32_t* winner, double* smooth, double* below)
{
    if (!weights) { weights = kSigma2Weights; radius = kSigma2Radius; }
    std::vector<double> z, g;
    PairwiseStack stack;
    for (int r = 0; r < n_regions; ++r) {
        const int S = (int)((offsets[r + 1] - offsets[r]) / n_angles);
        z.resize((size_t)S); g.resize((size_t)S + kProfileFlipExtra);
        for (int a = 0; a < n_angles; ++a) {
            const size_t k = (size_t)r * n_angles + a;
            const size_t at = (size_t)offsets[r] + (size_t)a * S;
            state[k] = (uint8_t)profile_statistic_serial(counts + at, S, weights, radius, multiplier, z.data(), g.data(), &stack, &spread[k],
                                                         smooth ? smooth + at : nullptr, below ? below + k : nullptr);
        }
        winner[r] = sweep_winner(spread + (size_t)r * n_angles, state + (size_t)r * n_angles, n_angles);
    }
}

int sbbseg_profile_statistics_host(const int32_t* counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights, int radius,
                                   double multiplier, double* spread, uint8_t* state, int32_t* winner, double* smooth)
{
    API_BEGIN
    if (check_profile_tables(offsets, n_regions, n_angles, radius)) return 1;
    REQUIRE((counts && spread && state && winner) || n_regions == 0, "bad arguments");
    alloc_check();
    profile_stats_serial(counts, offsets, n_regions, n_angles, weights, radius, multiplier, spread, state, winner, smooth, nullptr);
    return 0;
    API_END
}

// queues the statistic of a sweep whose counts are in device memory; *out holds the device pointers of the results (in c->pstat.p)
static int profile_stats_queue(sbbseg_ctx* c, const int32_t* d_counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights,
                               int radius, double multiplier, std::vector<unsigned char>& head, ProfileStatParams* out, double* d_smooth = nullptr,
                               double* d_below = nullptr)
{
    if (!weights) { weights = kSigma2Weights; radius = kSigma2Radius; }
    const size_t np = (size_t)n_regions * n_angles;
    const size_t w_bytes = (size_t)(radius + 1) * sizeof(double), head_bytes = w_bytes + (size_t)n_regions * sizeof(ProfileRegion);
    head.assign(head_bytes, 0);
    memcpy(head.data(), weights, w_bytes);
    ProfileRegion* reg = (ProfileRegion*)(head.data() + w_bytes);
    long long ws_doubles = 0;
    for (int r = 0; r < n_regions; ++r) {
        reg[r].count_off = offsets[r];
        reg[r].S = (int)((offsets[r + 1] - offsets[r]) / n_angles);
        reg[r].ws_off = ws_doubles;
        if (reg[r].S > kProfileLdsSamples) ws_doubles += (long long)n_angles * (2ll * reg[r].S + kProfileFlipExtra);
    }
    const size_t spread_off = head_bytes, winner_off = spread_off + np * sizeof(double), state_off = winner_off + (size_t)n_regions * sizeof(int32_t);
    const size_t ws_off = align16(state_off + np);
    if (ensure(c, c->pstat, ws_off + (size_t)ws_doubles * sizeof(double))) return 1;
    unsigned char* d = (unsigned char*)c->pstat.p;
    ProfileStatParams p;
    p.counts = d_counts; p.regions = (const ProfileRegion*)(d + w_bytes); p.n_regions = n_regions; p.n_angles = n_angles;
    p.weights = (const double*)d; p.radius = radius; p.multiplier = multiplier;
    p.workspace = (double*)(d + ws_off); p.spread = (double*)(d + spread_off); p.state = d + state_off; p.winner = (int32_t*)(d + winner_off);
    p.smooth = d_smooth; p.below = d_below;                         // (null in the product's calls)
    HIPCHK(hipMemcpyAsync(d, head.data(), head_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_profile_statistics(p, ws_doubles > 0, c->stream));
    c->slope_launches += ws_doubles > 0 ? 3 : 2;
    *out = p;
    return 0;
}

int sbbseg_profile_statistics_dev(sbbseg_ctx* c, const void* d_counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights,
                                  int radius, double multiplier, double* spread, uint8_t* state, int32_t* winner)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    if (check_profile_tables(offsets, n_regions, n_angles, radius)) return 1;
    if (n_regions == 0) return 0;
    REQUIRE(d_counts, "bad arguments");
    alloc_check();
    std::vector<unsigned char> head;
    ProfileStatParams p;
    if (profile_stats_queue(c, (const int32_t*)d_counts, offsets, n_regions, n_angles, weights, radius, multiplier, head, &p)) return 1;
    const size_t np = (size_t)n_regions * n_angles;
    if (spread) HIPCHK(hipMemcpyAsync(spread, p.spread, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (state) HIPCHK(hipMemcpyAsync(state, p.state, np, hipMemcpyDeviceToHost, c->stream));
    if (winner) HIPCHK(hipMemcpyAsync(winner, p.winner, (size_t)n_regions * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the host staging buffer lives until here)
    return 0;
    API_END
}

int sbbseg_debug_profile_statistics(sbbseg_ctx* c, const int32_t* counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights,
                                    int radius, double multiplier, double* spread, uint8_t* state, int32_t* winner, double* smooth, double* below)
{
    API_BEGIN
    if (c && check_ready(c)) return 1;
    if (check_profile_tables(offsets, n_regions, n_angles, radius)) return 1;
    REQUIRE((counts && spread && state && winner) || n_regions == 0, "bad arguments");
    if (n_regions == 0) return 0;
    alloc_check();
    if (!c) {
        profile_stats_serial(counts, offsets, n_regions, n_angles, weights, radius, multiplier, spread, state, winner, smooth, below);
        return 0;
    }
    const size_t np = (size_t)n_regions * n_angles, total = (size_t)offsets[n_regions];
    ScopedBlock<int32_t> d_counts(c->mem);
    ScopedBlock<double> d_smooth(c->mem), d_below(c->mem);
    if (d_counts.alloc(total) || (smooth && d_smooth.alloc(total)) || (below && d_below.alloc(np))) return 1;
    HIPCHK(hipMemcpyAsync(d_counts.p, counts, total * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    std::vector<unsigned char> head;
    ProfileStatParams p;
    if (profile_stats_queue(c, d_counts.p, offsets, n_regions, n_angles, weights, radius, multiplier, head, &p, d_smooth.p, d_below.p)) return 1;
    HIPCHK(hipMemcpyAsync(spread, p.spread, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(state, p.state, np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(winner, p.winner, (size_t)n_regions * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (smooth) HIPCHK(hipMemcpyAsync(smooth, p.smooth, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (below) HIPCHK(hipMemcpyAsync(below, p.below, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_debug_soft_arith(sbbseg_ctx* c, int op, const double* a, const double* b, int64_t n, double* out)
{
    API_BEGIN
    if (c && check_ready(c)) return 1;
    REQUIRE((op == 0 || op == 1) && n >= 0 && n <= (1ll << 24) && ((a && out && (b || op == 1)) || n == 0), "bad arguments");
    if (n == 0) return 0;
    if (!c) {
        for (int64_t i = 0; i < n; ++i) out[i] = op == 0 ? soft_div(a[i], b[i]) : soft_sqrt(a[i]);
        return 0;
    }
    alloc_check();
    ScopedBlock<double> d_a(c->mem), d_b(c->mem), d_out(c->mem);
    if (d_a.alloc((size_t)n) || (op == 0 && d_b.alloc((size_t)n)) || d_out.alloc((size_t)n)) return 1;
    HIPCHK(hipMemcpyAsync(d_a.p, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (op == 0) HIPCHK(hipMemcpyAsync(d_b.p, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_soft_arith(op, d_a.p, d_b.p, n, d_out.p, c->stream));
    HIPCHK(hipMemcpyAsync(out, d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

// one sweep of all `boxes`: rotate-and-project, statistic, selection; the winners come back, the counts do not
static int slopes_sweep(sbbseg_ctx* c, const PlaneSet& ps, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                        const double* angles, int n_angles, const double* weights, int radius, std::vector<int32_t>& winner)
{
    std::vector<int64_t> offsets((size_t)n_boxes + 1);
    std::vector<unsigned char> head_sweep, head_stat;
    const int32_t* d_counts = nullptr;
    if (region_sweep(c, ps, boxes_xywh, n_boxes, erode_iterations, angles, n_angles, offsets.data(), false, head_sweep, &d_counts)) return 1;
    ProfileStatParams p;
    if (profile_stats_queue(c, d_counts, offsets.data(), n_boxes, n_angles, weights, radius, 20.3, head_stat, &p)) return 1;      // main.py:1644
    winner.resize((size_t)n_boxes);
    HIPCHK(hipMemcpyAsync(winner.data(), p.winner, (size_t)n_boxes * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the host staging buffers live until here)
    return 0;
}

static int region_slopes(sbbseg_ctx* c, const PlaneSet& ps, const int32_t* boxes_xywh, int n_boxes, int erode_iterations, const double* weights,
                         int radius, double* slopes)
{
    if (check_ready(c)) return 1;
    REQUIRE(n_boxes >= 0 && n_boxes <= (1 << 20) && (boxes_xywh || n_boxes == 0) && (slopes || n_boxes == 0), "bad arguments");
    if (check_plane_set(ps, n_boxes)) return 1;
    REQUIRE(radius >= 0 && radius <= (1 << 16), "radius %d out of range (0 .. 65536)", radius);
    if (n_boxes == 0) return 0;
    REQUIRE(ps.pooled || ps.planes[0].d_hw, "bad arguments");
    alloc_check();
    double first[kSweeps[0].n], second[kSweeps[1].n];
    sweep_angles(0, first); sweep_angles(1, second);
    std::vector<int32_t> winner;
    if (slopes_sweep(c, ps, boxes_xywh, n_boxes, erode_iterations, first, kSweeps[0].n, weights, radius, winner)) return 1;
    std::vector<int32_t> steep, steep_boxes, steep_plane;              // the steep boxes are cropped again: their planes travel with them
    for (int r = 0; r < n_boxes; ++r) {
        slopes[r] = winner[r] < 0 ? 0.0 : first[winner[r]];
        if (std::fabs(slopes[r]) > 15.0) {                          // main.py:1669-1670
            steep.push_back(r);
            steep_boxes.insert(steep_boxes.end(), boxes_xywh + (size_t)r * 4, boxes_xywh + (size_t)r * 4 + 4);
            if (ps.pooled) steep_plane.push_back(ps.box_plane[r]);
        }
    }
    if (!steep.empty()) {
        const PlaneSet again{ps.planes, ps.n_planes, ps.pooled ? steep_plane.data() : nullptr, ps.pooled};
        if (slopes_sweep(c, again, steep_boxes.data(), (int)steep.size(), erode_iterations, second, kSweeps[1].n, weights, radius, winner)) return 1;
        for (size_t k = 0; k < steep.size(); ++k) slopes[steep[k]] = winner[k] < 0 ? 0.0 : second[winner[k]];
    }
    for (int r = 0; r < n_boxes; ++r)
        if (std::fabs(slopes[r]) > 120.5) slopes[r] = 0.0;          // main.py:1746-1747
    return 0;
}

int sbbseg_region_deskew_slopes_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                    int erode_iterations, const double* weights, int radius, double* slopes)
{
    API_BEGIN
    sbbseg_plane pl;
    return region_slopes(c, one_plane(&pl, d_textline_hw, H, W), boxes_xywh, n_boxes, erode_iterations, weights, radius, slopes);
    API_END
}

int sbbseg_planes_deskew_slopes_dev(sbbseg_ctx* c, const sbbseg_plane* planes, int n_planes, const int32_t* boxes_xywh, const int32_t* box_plane,
                                    int n_boxes, int erode_iterations, const double* weights, int radius, double* slopes)
{
    API_BEGIN
    return region_slopes(c, PlaneSet{planes, n_planes, box_plane, true}, boxes_xywh, n_boxes, erode_iterations, weights, radius, slopes);
    API_END
}

int sbbseg_region_deskew_slopes(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                int erode_iterations, const double* weights, int radius, double* slopes)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    const void* d_plane;
    if (stage_plane(c, textline_hw, H, W, n_boxes > 0, &d_plane)) return 1;
    return sbbseg_region_deskew_slopes_dev(c, d_plane, H, W, boxes_xywh, n_boxes, erode_iterations, weights, radius, slopes);
    API_END
}

// ---- stage glue: deskewed text-line masks and line profiles per region (textline_contours_postprocessing, main.py:1472-1487; line_mask.h) ----
static void line_table(std::vector<int16_t>& itab)
{
    float tab[128];
    cubic_table(tab);
    itab.resize((size_t)kLineTabEntries);
    for (int ay = 0; ay < 32; ++ay)
        for (int ax = 0; ax < 32; ++ax) line_mask_weights(tab, ay, ax, itab.data() + (size_t)(ay * 32 + ax) * 16);
}

// rotate_image's inverse map for an h x w crop (main.py:159-163: center = (w // 2, h // 2))
extern "C++" {
namespace sbbseg {
int line_inverse_map(int h, int w, double slope, double* minv6)
{
    double M[6];
    if (sbbseg_rotation_matrix((double)(w / 2), (double)(h / 2), slope, M)) return 1;
    invert_affine(M, minv6);
    return 0;
}
}  // namespace sbbseg
}  // extern "C++"

int sbbseg_region_line_table(int16_t* itab, int capacity)
{
    API_BEGIN
    REQUIRE(itab && capacity >= kLineTabEntries, "room for %d weights, the table has %d", capacity, kLineTabEntries);
    alloc_check();
    std::vector<int16_t> t;
    line_table(t);
    memcpy(itab, t.data(), t.size() * sizeof(int16_t));
    return 0;
    API_END
}

// one clipped separable min / max of the given radius, in place (tmp: h * w bytes)
static void host_line_morph(uint8_t* img, uint8_t* tmp, int h, int w, int radius, int is_max, int scale)
{
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) tmp[(size_t)y * w + x] = (uint8_t)line_mask_morph_1d(img + (size_t)y * w, 1, x, w, radius, is_max, scale);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) img[(size_t)y * w + x] = (uint8_t)line_mask_morph_1d(tmp + x, (size_t)w, y, h, radius, is_max, 1);
}

int sbbseg_region_line_masks_host(const uint8_t* crop_hw, int h, int w, int erode_iterations, double slope, uint8_t* mask, int32_t* rows, int32_t* cols)
{
    API_BEGIN
    REQUIRE(crop_hw && rows && cols && erode_iterations >= 0 && erode_iterations <= 64, "bad arguments");
    REQUIRE(h >= 1 && w >= 1, "crop: width %d, height %d (both must be at least 1)", w, h);
    REQUIRE((long long)h * w < (1ll << 31), "crop of %d x %d is too large", w, h);
    alloc_check();
    const size_t pix = (size_t)h * w;
    std::vector<uint8_t> img(crop_hw, crop_hw + pix), tmp(pix);
    std::vector<int16_t> itab;
    line_table(itab);
    host_line_morph(img.data(), tmp.data(), h, w, 2 * erode_iterations, 0, 1);        // cv2.erode(crop, 5x5, iterations) (main.py:1734)
    host_line_morph(img.data(), tmp.data(), h, w, 2, 0, 255);                         // * 255, then OPEN's erode ...
    host_line_morph(img.data(), tmp.data(), h, w, 4, 1, 1);                           // ... OPEN's dilate + CLOSE's dilate ...
    host_line_morph(img.data(), tmp.data(), h, w, 2, 0, 1);                           // ... and CLOSE's erode
    double m[6];
    if (line_inverse_map(h, w, slope, m)) return 1;
    for (int x = 0; x < w; ++x) cols[x] = 0;
    for (int y = 0; y < h; ++y) {
        long long X0, Y0;
        line_mask_row_origin(m, y, &X0, &Y0);
        int cnt = 0;
        for (int x = 0; x < w; ++x) {
            const int d = line_mask_pixel(img.data(), w, h, m[0], m[3], X0, Y0, x, itab.data()) != 0;
            if (mask) mask[(size_t)y * w + x] = (uint8_t)d;
            cnt += d;
            cols[x] += d;
        }
        rows[y] = cnt;
    }
    return 0;
    API_END
}

// queues crop / erode / OPEN / CLOSE / warp / sums of all boxes; *out holds the device pointers of the results (in c->rdk.p), out->n_regions
// == 0 when there is nothing to do.  `need_sums`: what a caller that downloads rows and cols must have passed.
static int region_line_masks_queue(sbbseg_ctx* c, const PlaneSet& ps, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                                   const double* slopes, bool need_sums, int64_t* mask_off, int64_t* row_off, int64_t* col_off,
                                   std::vector<unsigned char>& head, RegionLinesParams* out, long long* rows_total)
{
    out->n_regions = 0;
    REQUIRE(n_boxes >= 0 && n_boxes <= (1 << 20) && (boxes_xywh || n_boxes == 0) && mask_off && row_off && col_off &&
                erode_iterations >= 0 && erode_iterations <= 64, "bad arguments");
    if (check_plane_set(ps, n_boxes)) return 1;
    alloc_check();
    std::vector<DeskewRegion> crop_geom((size_t)n_boxes);
    std::vector<DeskewPlane> src((size_t)n_boxes);
    std::vector<LineRegion> geom((size_t)n_boxes);
    long long total_pix = 0, total_rows = 0, total_cols = 0, total_blocks = 0;
    for (int r = 0; r < n_boxes; ++r) {
        DeskewRegion& cg = crop_geom[r];
        if (crop_region(ps, boxes_xywh, r, total_pix, &cg, &src[r])) return 1;
        LineRegion& g = geom[r];
        g.w = cg.w; g.h = cg.h; g.crop_off = total_pix; g.row_off = (int)total_rows; g.col_off = (int)total_cols; g.block0 = (int)total_blocks; g.pad = 0;
        mask_off[r] = total_pix; row_off[r] = total_rows; col_off[r] = total_cols;
        total_pix += (long long)g.w * g.h;
        total_rows += g.h;
        total_cols += g.w;
        total_blocks += (g.h + kRegionLineRows - 1) / kRegionLineRows;
        REQUIRE(total_pix < (1ll << 31) && total_rows < (1ll << 30) && total_cols < (1ll << 30), "too much work for one call (%d boxes): split the boxes", n_boxes);
    }
    mask_off[n_boxes] = total_pix; row_off[n_boxes] = total_rows; col_off[n_boxes] = total_cols;
    if (n_boxes == 0) return 0;
    if (check_ready(c)) return 1;
    REQUIRE((ps.pooled || ps.planes[0].d_hw) && slopes && need_sums, "bad arguments");
    if (!c->d_line_tab) {
        std::vector<int16_t> itab;
        line_table(itab);
        if (upload(c, &c->d_line_tab, itab.data(), itab.size())) return 1;
    }
    // head of the device buffer, built on the host and copied in one piece: inverse maps | crop geometry | line geometry | planes
    const size_t minv_bytes = (size_t)n_boxes * 6 * sizeof(double), cgeom_bytes = (size_t)n_boxes * sizeof(DeskewRegion);
    const size_t lgeom_off = minv_bytes + cgeom_bytes, src_off = lgeom_off + (size_t)n_boxes * sizeof(LineRegion);
    const size_t head_bytes = align16(src_off + (size_t)n_boxes * sizeof(DeskewPlane));
    const size_t pix_bytes = align16((size_t)total_pix);
    head.assign(head_bytes, 0);
    for (int r = 0; r < n_boxes; ++r)
        if (line_inverse_map(geom[r].h, geom[r].w, slopes[r], (double*)head.data() + (size_t)r * 6)) return 1;
    memcpy(head.data() + minv_bytes, crop_geom.data(), cgeom_bytes);
    memcpy(head.data() + lgeom_off, geom.data(), (size_t)n_boxes * sizeof(LineRegion));
    memcpy(head.data() + src_off, src.data(), (size_t)n_boxes * sizeof(DeskewPlane));
    if (ensure(c, c->rdk, head_bytes + 3 * pix_bytes + (size_t)(total_rows + total_cols) * sizeof(int))) return 1;
    unsigned char* d = (unsigned char*)c->rdk.p;
    RegionDeskewParams cp;
    memset(&cp, 0, sizeof(cp));
    cp.planes = (const DeskewPlane*)(d + src_off);
    cp.geom = (const DeskewRegion*)(d + minv_bytes); cp.n_regions = n_boxes; cp.radius = 2 * erode_iterations; cp.total_pix = total_pix;
    cp.tmp = d + head_bytes; cp.crops = d + head_bytes + pix_bytes;
    RegionLinesParams p;
    p.geom = (const LineRegion*)(d + lgeom_off); p.n_regions = n_boxes; p.total_pix = total_pix; p.total_cols = (int)total_cols;
    p.total_blocks = (int)total_blocks; p.minv = (const double*)d; p.itab = c->d_line_tab;
    p.a = cp.tmp; p.b = cp.crops; p.mask = d + head_bytes + 2 * pix_bytes;
    p.rows = (int*)(d + head_bytes + 3 * pix_bytes); p.cols = p.rows + total_rows;
    HIPCHK(hipMemcpyAsync(d, head.data(), head_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_region_deskew_crops(cp, c->stream));
    HIPCHK(launch_region_line_morph(p, c->stream));
    HIPCHK(launch_region_line_masks(p, c->stream));
    c->line_launches += 2 + kRegionLineLaunches;
    *out = p;
    *rows_total = total_rows;
    return 0;
}

static int region_line_masks(sbbseg_ctx* c, const PlaneSet& ps, const int32_t* boxes_xywh, int n_boxes, int erode_iterations, const double* slopes,
                             uint8_t* masks, int32_t* rows, int32_t* cols, int64_t* mask_off, int64_t* row_off, int64_t* col_off)
{
    std::vector<unsigned char> head;
    RegionLinesParams p;
    long long total_rows = 0;
    if (region_line_masks_queue(c, ps, boxes_xywh, n_boxes, erode_iterations, slopes, rows && cols, mask_off, row_off, col_off, head, &p, &total_rows)) return 1;
    if (p.n_regions == 0) return 0;
    if (masks) HIPCHK(hipMemcpyAsync(masks, p.mask, (size_t)p.total_pix, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rows, p.rows, (size_t)total_rows * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cols, p.cols, (size_t)p.total_cols * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the host staging buffer lives until here)
    return 0;
}

int sbbseg_region_line_masks_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                                 const double* slopes, uint8_t* masks, int32_t* rows, int32_t* cols, int64_t* mask_off, int64_t* row_off, int64_t* col_off)
{
    API_BEGIN
    sbbseg_plane pl;
    return region_line_masks(c, one_plane(&pl, d_textline_hw, H, W), boxes_xywh, n_boxes, erode_iterations, slopes, masks, rows, cols, mask_off, row_off, col_off);
    API_END
}

int sbbseg_planes_line_masks_dev(sbbseg_ctx* c, const sbbseg_plane* planes, int n_planes, const int32_t* boxes_xywh, const int32_t* box_plane, int n_boxes,
                                 int erode_iterations, const double* slopes, uint8_t* masks, int32_t* rows, int32_t* cols, int64_t* mask_off,
                                 int64_t* row_off, int64_t* col_off)
{
    API_BEGIN
    return region_line_masks(c, PlaneSet{planes, n_planes, box_plane, true}, boxes_xywh, n_boxes, erode_iterations, slopes, masks, rows, cols, mask_off, row_off,
                             col_off);
    API_END
}

int sbbseg_region_line_masks(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                             const double* slopes, uint8_t* masks, int32_t* rows, int32_t* cols, int64_t* mask_off, int64_t* row_off, int64_t* col_off)
{
    API_BEGIN
    const void* d_plane;
    if (stage_plane(c, textline_hw, H, W, n_boxes > 0, &d_plane)) return 1;
    return sbbseg_region_line_masks_dev(c, d_plane, H, W, boxes_xywh, n_boxes, erode_iterations, slopes, masks, rows, cols,
                                        mask_off, row_off, col_off);
    API_END
}

// ---- stage glue: text-line peaks and line boxes per region (seperate_lines / seperate_lines_vertical after the projection; line_split.h) ----
static int check_line_split_tables(const int64_t* offsets, int n_regions, const int32_t* geom, const double* rot, const double* weights,
                                   const int64_t* weight_off, int sigma_max, int64_t* line_off)
{
    REQUIRE(n_regions >= 0 && n_regions <= (1 << 20) && line_off && ((offsets && geom && rot) || n_regions == 0), "bad arguments");
    REQUIRE(weights && weight_off && sigma_max >= kLineSigmaRaised && sigma_max <= 4096, "the weight table must hold sigma = 2 .. sigma_max, sigma_max in 12 .. 4096");
    for (int s = kLineSigmaMin; s <= sigma_max; ++s)
        REQUIRE(weight_off[s - kLineSigmaMin] >= 0 && weight_off[s - kLineSigmaMin + 1] - weight_off[s - kLineSigmaMin] == 4 * s + 1,
                "weight table: sigma %d does not have 4 * sigma + 1 weights", s);
    long long lines = 0;
    for (int r = 0; r < n_regions; ++r) {
        const int32_t* g = geom + (size_t)r * 3;
        REQUIRE(g[0] >= 1 && g[0] <= 32767 && g[1] >= 1 && g[1] <= (1 << 24) && (g[2] == 0 || g[2] == 1),
                "region %d: length %d (1 .. 32767), other extent %d (1 .. 2^24), vertical %d (0, 1)", r, g[0], g[1], g[2]);
        REQUIRE(offsets[r] >= 0 && offsets[r + 1] - offsets[r] == g[0] && offsets[r + 1] < (1ll << 31), "region %d: offsets %lld .. %lld do not hold %d samples", r,
                (long long)offsets[r], (long long)offsets[r + 1], g[0]);
        line_off[r] = lines;
        lines += line_capacity(g[0]);
    }
    line_off[n_regions] = lines;
    REQUIRE(lines < (1ll << 27), "too much work for one call (%d regions): split the regions", n_regions);
    return 0;
}

static LineGeom line_geom(const int32_t* g, const double* rot)
{
    LineGeom out;
    out.n = g[0]; out.other = g[1]; out.vertical = g[2];
    out.r00 = rot[0]; out.r01 = rot[1]; out.r10 = rot[2]; out.r11 = rot[3]; out.xd = rot[4]; out.yd = rot[5];
    return out;
}

int sbbseg_line_split_host(const int32_t* profiles, const int64_t* offsets, int n_regions, const int32_t* geom, const double* rot, const double* weights,
                           const int64_t* weight_off, int sigma_max, const double* extra_weights, int extra_sigma, int32_t* info, int64_t* line_off,
                           int32_t* lines, int32_t* corners, int32_t* corners_rot)
{
    API_BEGIN
    if (check_line_split_tables(offsets, n_regions, geom, rot, weights, weight_off, sigma_max, line_off)) return 1;
    REQUIRE((profiles && info && lines && corners && corners_rot) || n_regions == 0, "bad arguments");
    REQUIRE(!extra_weights || extra_sigma >= 1, "extra_sigma %d", extra_sigma);
    alloc_check();
    const LineWeights w{weights, weight_off, sigma_max, extra_weights, extra_sigma};
    std::vector<unsigned char> work;
    PairwiseStack stack;
    for (int r = 0; r < n_regions; ++r) {
        const LineGeom g = line_geom(geom + (size_t)r * 3, rot + (size_t)r * 6);
        work.resize(line_work_bytes(g.n));
        const size_t at = (size_t)line_off[r];
        line_split_serial(profiles + offsets[r], g, w, LineWork{work.data(), g.n, &stack}, info + (size_t)r * kLineInfoInts, lines + at * 3, corners + at * 8,
                          corners_rot + at * 8);
    }
    return 0;
    API_END
}

// queues the split of regions whose profiles are in device memory (region r: n ints from d_profiles + prof_off[r]); *out holds the device
// pointers of the results (in c->lsplit.p)
static int line_split_queue(sbbseg_ctx* c, const int32_t* d_profiles, const int64_t* prof_off, int n_regions, const int32_t* geom, const double* rot,
                            const double* weights, const int64_t* weight_off, int sigma_max, const int64_t* line_off, std::vector<unsigned char>& head,
                            LineSplitParams* out)
{
    if (sigma_max > kLineSigmaMax) sigma_max = kLineSigmaMax;      // the device's table ends there; larger sigmas are reported, not computed
    const size_t n_off = (size_t)(sigma_max - kLineSigmaMin + 2), n_w = (size_t)weight_off[n_off - 1];
    const size_t off_bytes = align16(n_off * sizeof(long long));
    if (c->line_w_host.size() != n_w || !c->line_w.p || memcmp(c->line_w_host.data(), weights, n_w * sizeof(double)) != 0) {
        std::vector<unsigned char> tab(off_bytes + n_w * sizeof(double));
        for (size_t i = 0; i < n_off; ++i) ((long long*)tab.data())[i] = (long long)weight_off[i];
        memcpy(tab.data() + off_bytes, weights, n_w * sizeof(double));
        c->line_w_host.clear();
        if (ensure(c, c->line_w, tab.size())) return 1;
        HIPCHK(hipMemcpyAsync(c->line_w.p, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->line_w_host.assign(weights, weights + n_w);
    }
    const size_t lines = (size_t)line_off[n_regions];
    const size_t info_off = align16((size_t)n_regions * sizeof(LineSplitRegion));
    const size_t pts_off = align16(info_off + (size_t)n_regions * kLineInfoInts * sizeof(int32_t));
    const size_t box_off = align16(pts_off + lines * 3 * sizeof(int32_t)), rot_off = box_off + lines * 8 * sizeof(int32_t);
    const size_t ws_off = rot_off + lines * 8 * sizeof(int32_t);
    head.assign(info_off, 0);
    LineSplitRegion* reg = (LineSplitRegion*)head.data();
    size_t ws_bytes = 0;
    for (int r = 0; r < n_regions; ++r) {
        const int32_t* g = geom + (size_t)r * 3;
        reg[r].prof_off = prof_off[r]; reg[r].ws_off = (long long)ws_bytes;
        reg[r].n = g[0]; reg[r].other = g[1]; reg[r].vertical = g[2]; reg[r].line_off = (int)line_off[r];
        memcpy(reg[r].rot, rot + (size_t)r * 6, 6 * sizeof(double));
        if (g[0] > kProfileLdsSamples) ws_bytes += line_work_bytes(g[0]);
    }
    if (ensure(c, c->lsplit, ws_off + ws_bytes)) return 1;
    unsigned char* d = (unsigned char*)c->lsplit.p;
    LineSplitParams p;
    p.profiles = d_profiles; p.regions = (const LineSplitRegion*)d; p.n_regions = n_regions; p.sigma_max = sigma_max;
    p.weights = (const double*)((unsigned char*)c->line_w.p + off_bytes); p.weight_off = (const long long*)c->line_w.p;
    p.workspace = d + ws_off; p.info = (int32_t*)(d + info_off); p.pts = (int32_t*)(d + pts_off); p.box = (int32_t*)(d + box_off);
    p.rot = (int32_t*)(d + rot_off);
    HIPCHK(hipMemcpyAsync(d, head.data(), info_off, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_line_split(p, ws_bytes > 0, c->stream));
    c->line_launches += ws_bytes > 0 ? 2 : 1;
    *out = p;
    return 0;
}

// copies info and, per region, its first `count` lines back: nothing beyond a region's count is written on the host
static int line_split_download(sbbseg_ctx* c, const LineSplitParams& p, const int64_t* line_off, int32_t* info, int32_t* lines, int32_t* corners,
                               int32_t* corners_rot)
{
    const size_t total = (size_t)line_off[p.n_regions];
    std::vector<int32_t> stage(total * 19);
    HIPCHK(hipMemcpyAsync(info, p.info, (size_t)p.n_regions * kLineInfoInts * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stage.data(), p.pts, total * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stage.data() + total * 3, p.box, total * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stage.data() + total * 11, p.rot, total * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the host staging buffers live until here)
    for (int r = 0; r < p.n_regions; ++r) {
        const size_t at = (size_t)line_off[r], n = (size_t)info[(size_t)r * kLineInfoInts + kLineInfoCount];
        memcpy(lines + at * 3, stage.data() + at * 3, n * 3 * sizeof(int32_t));
        memcpy(corners + at * 8, stage.data() + total * 3 + at * 8, n * 8 * sizeof(int32_t));
        memcpy(corners_rot + at * 8, stage.data() + total * 11 + at * 8, n * 8 * sizeof(int32_t));
    }
    return 0;
}

int sbbseg_line_split_dev(sbbseg_ctx* c, const void* d_profiles, const int64_t* offsets, int n_regions, const int32_t* geom, const double* rot,
                          const double* weights, const int64_t* weight_off, int sigma_max, int32_t* info, int64_t* line_off, int32_t* lines,
                          int32_t* corners, int32_t* corners_rot)
{
    API_BEGIN
    if (check_line_split_tables(offsets, n_regions, geom, rot, weights, weight_off, sigma_max, line_off)) return 1;
    if (n_regions == 0) return 0;
    if (check_ready(c)) return 1;
    REQUIRE(d_profiles && info && lines && corners && corners_rot, "bad arguments");
    alloc_check();
    std::vector<unsigned char> head;
    LineSplitParams p;
    if (line_split_queue(c, (const int32_t*)d_profiles, offsets, n_regions, geom, rot, weights, weight_off, sigma_max, line_off, head, &p)) return 1;
    return line_split_download(c, p, line_off, info, lines, corners, corners_rot);
    API_END
}

static int region_line_boxes(sbbseg_ctx* c, const PlaneSet& ps, const int32_t* boxes_xywh, int n_boxes, int erode_iterations, const double* slopes,
                             const double* rot, const double* weights, const int64_t* weight_off, int sigma_max, int32_t* info, int64_t* line_off,
                             int32_t* lines, int32_t* corners, int32_t* corners_rot)
{
    REQUIRE(n_boxes >= 0 && n_boxes <= (1 << 20) && line_off && ((boxes_xywh && slopes && rot) || n_boxes == 0), "bad arguments");
    alloc_check();
    std::vector<int64_t> mask_off((size_t)n_boxes + 1), row_off((size_t)n_boxes + 1), col_off((size_t)n_boxes + 1), prof_off((size_t)n_boxes + 1);
    std::vector<int32_t> geom((size_t)n_boxes * 3);
    std::vector<unsigned char> head_masks, head_split;
    RegionLinesParams lp;
    long long total_rows = 0;
    if (region_line_masks_queue(c, ps, boxes_xywh, n_boxes, erode_iterations, slopes, true, mask_off.data(), row_off.data(), col_off.data(),
                                head_masks, &lp, &total_rows)) return 1;
    // rows and cols are one device array (cols behind rows): a region's profile is its row sums, or its column sums beyond 45 degrees
    // (main.py:1514)
    int64_t at = 0;
    for (int r = 0; r < n_boxes; ++r) {
        const int w = boxes_xywh[(size_t)r * 4 + 2], h = boxes_xywh[(size_t)r * 4 + 3], vertical = std::fabs(slopes[r]) > 45.0;
        geom[(size_t)r * 3] = vertical ? w : h; geom[(size_t)r * 3 + 1] = vertical ? h : w; geom[(size_t)r * 3 + 2] = vertical;
        prof_off[r] = at;
        at += geom[(size_t)r * 3];
    }
    prof_off[n_boxes] = at;
    if (check_line_split_tables(prof_off.data(), n_boxes, geom.data(), rot, weights, weight_off, sigma_max, line_off)) return 1;
    if (n_boxes == 0) return 0;
    REQUIRE(info && lines && corners && corners_rot, "bad arguments");
    for (int r = 0; r < n_boxes; ++r) prof_off[r] = geom[(size_t)r * 3 + 2] ? total_rows + col_off[r] : row_off[r];
    LineSplitParams p;
    if (line_split_queue(c, lp.rows, prof_off.data(), n_boxes, geom.data(), rot, weights, weight_off, sigma_max, line_off, head_split, &p)) return 1;
    return line_split_download(c, p, line_off, info, lines, corners, corners_rot);
}

int sbbseg_region_line_boxes_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                                 const double* slopes, const double* rot, const double* weights, const int64_t* weight_off, int sigma_max, int32_t* info,
                                 int64_t* line_off, int32_t* lines, int32_t* corners, int32_t* corners_rot)
{
    API_BEGIN
    sbbseg_plane pl;
    return region_line_boxes(c, one_plane(&pl, d_textline_hw, H, W), boxes_xywh, n_boxes, erode_iterations, slopes, rot, weights, weight_off, sigma_max, info,
                             line_off, lines, corners, corners_rot);
    API_END
}

int sbbseg_planes_line_boxes_dev(sbbseg_ctx* c, const sbbseg_plane* planes, int n_planes, const int32_t* boxes_xywh, const int32_t* box_plane, int n_boxes,
                                 int erode_iterations, const double* slopes, const double* rot, const double* weights, const int64_t* weight_off,
                                 int sigma_max, int32_t* info, int64_t* line_off, int32_t* lines, int32_t* corners, int32_t* corners_rot)
{
    API_BEGIN
    return region_line_boxes(c, PlaneSet{planes, n_planes, box_plane, true}, boxes_xywh, n_boxes, erode_iterations, slopes, rot, weights, weight_off, sigma_max, info,
                             line_off, lines, corners, corners_rot);
    API_END
}

int sbbseg_region_line_boxes(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                             const double* slopes, const double* rot, const double* weights, const int64_t* weight_off, int sigma_max, int32_t* info,
                             int64_t* line_off, int32_t* lines, int32_t* corners, int32_t* corners_rot)
{
    API_BEGIN
    const void* d_plane;
    if (stage_plane(c, textline_hw, H, W, n_boxes > 0, &d_plane)) return 1;
    return sbbseg_region_line_boxes_dev(c, d_plane, H, W, boxes_xywh, n_boxes, erode_iterations, slopes, rot, weights,
                                        weight_off, sigma_max, info, line_off, lines, corners, corners_rot);
    API_END
}

}  // extern "C"
