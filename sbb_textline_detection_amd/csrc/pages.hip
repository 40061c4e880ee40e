// pages.hip -- do_prediction(patches=True) (main.py:225-380) without the per-patch Python loop: the tile grid, the pooled tile ranges of equally
// sized pages and of views of any size, the stitch, and the page, crop and view entry points on top of them
//   ingest (u8 -> LUT -> bf16 tiles)  ->  fused conv plan (forward.hip)  ->  head (softmax/argmax)  ->  stitch
#include <string.h>

#include <cmath>

#include "exec.h"
#include "route.h"

using namespace sbbseg;

namespace {

int margin_of(int W) { return (int)(0.1 * (double)W); }   // main.py:233  int(0.1 * img_width_model)

// per-axis tiles exactly as main.py:246-281: count = ceil(extent/mid); origin t*mid clamped inward
int axis_tiles(int extent, int tile, int margin, std::vector<int>& origin)
{
    const int mid = tile - 2 * margin;
    if (mid <= 0 || extent < tile) return -1;
    const int n = (extent + mid - 1) / mid;
    origin.resize(n);
    for (int t = 0; t < n; ++t) {
        int d = t * mid;
        if (d + tile > extent) d = extent - tile;
        origin[t] = d;
    }
    return n;
}

// owner table of one axis (closed form of the crop + overwrite order, main.py:294-364)
void axis_owner(int extent, int tile, int margin, const std::vector<int>& origin, std::vector<int>& own)
{
    own.assign(extent, 0);
    const int n = (int)origin.size();
    for (int t = 0; t < n; ++t) {
        const int lo = origin[t] + (t == 0 ? 0 : margin);
        const int hi = origin[t] + (t == n - 1 ? tile : tile - margin);
        for (int q = lo; q < hi; ++q) own[q] = (t << 16) | (q - origin[t]);
    }
}

}  // namespace

namespace sbbseg {

// cv2.resize(..., INTER_NEAREST) index rule [EXT OpenCV resizeNN]: min(floor(dst * (1/(dst_len/src_len))), src_len-1)
void nearest_map(int src_len, int dst_len, std::vector<int>& m)
{
    m.resize(dst_len);
    const double inv = 1.0 / ((double)dst_len / (double)src_len);
    for (int i = 0; i < dst_len; ++i) {
        int s = (int)std::floor(i * inv);
        m[i] = s < src_len - 1 ? s : src_len - 1;
    }
}

// The per-call tables of the many-view entry points (sbbseg_segment_views_dev, sbbseg_segment_whole_views_dev): c->h_views (pinned) and
// c->views hold at least `bytes`, and the staging may be rewritten (the previous call's upload has read it).
int views_staging(sbbseg_ctx* c, size_t bytes)
{
    if (c->views_copy_pending) {                               // (the previous call's upload still reads the staging)
        HIPCHK(hipEventSynchronize(c->ev_views));
        c->views_copy_pending = false;
    }
    if (!c->ev_views) HIPCHK(hipEventCreateWithFlags(&c->ev_views, hipEventDisableTiming));
    if (c->h_views.cap < bytes && ensure(c->pinned, c->h_views, bytes + bytes / 2)) return 1;       // (half as much again: view counts creep up)
    if (c->views.cap < bytes && ensure(c, c->views, bytes + bytes / 2)) return 1;
    return 0;
}

}  // namespace sbbseg

extern "C" {

int sbbseg_debug_owned_range(int extent, int tile, int margin, int n_tiles, int t, int* lo, int* hi)
{
    API_BEGIN
    REQUIRE(lo && hi && tile > 2 * margin && margin >= 0 && extent >= tile && n_tiles >= 1 && t >= 0 && t < n_tiles, "bad arguments");
    const RegionAxis a = {extent, tile, margin, tile - 2 * margin, n_tiles};
    region_own(a, t, *lo, *hi);
    return 0;
    API_END
}

int sbbseg_debug_region_rows(int extent, int tile, int margin, int n_tiles, int t, int levels, const int32_t* level_size, int32_t* lo_hi)
{
    API_BEGIN
    REQUIRE(lo_hi && level_size && levels >= 1 && levels <= kRegionMaxLevels && tile > 2 * margin && margin >= 0 && extent >= tile && n_tiles >= 1 &&
            t >= 0 && t < n_tiles, "bad arguments");
    const RegionAxis a = {extent, tile, margin, tile - 2 * margin, n_tiles};
    int lo, hi;
    region_own(a, t, lo, hi);
    lo_hi[0] = lo; lo_hi[1] = hi;
    for (int k = 1; k < levels; ++k) {
        region_down(lo, hi, level_size[k]);
        lo_hi[2 * k] = lo; lo_hi[2 * k + 1] = hi;
    }
    return 0;
    API_END
}

// -------------------------------------------------------------------------------------- seam 1
int sbbseg_tile_grid(int Hp, int Wp, int H, int W, int32_t* tile_xy, int capacity, int* nxf, int* nyf)
{
    API_BEGIN
    alloc_check();
    std::vector<int> ox, oy;
    const int margin = margin_of(W);
    const int nx = axis_tiles(Wp, W, margin, ox), ny = axis_tiles(Hp, H, margin, oy);
    REQUIRE_GEOMETRY(nx > 0 && ny > 0, "page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)", Hp, Wp, H, W);
    if (nxf) *nxf = nx;
    if (nyf) *nyf = ny;
    if (tile_xy) {
        REQUIRE(capacity >= nx * ny, "tile_xy capacity %d < %d tiles", capacity, nx * ny);
        for (int i = 0; i < nx; ++i)               // x outer, y inner: main.py:259-260
            for (int j = 0; j < ny; ++j) {
                tile_xy[2 * (i * ny + j)] = ox[i];
                tile_xy[2 * (i * ny + j) + 1] = oy[j];
            }
    }
    return 0;
    API_END
}

int sbbseg_nearest_map(int src_len, int dst_len, int32_t* map)
{
    API_BEGIN
    REQUIRE(src_len > 0 && dst_len > 0 && map, "bad arguments");
    alloc_check();
    std::vector<int> m;
    nearest_map(src_len, dst_len, m);
    for (int i = 0; i < dst_len; ++i) map[i] = m[i];
    return 0;
    API_END
}

int sbbseg_segment_tiles_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, const int32_t* tile_xy, int n_tiles,
                             void* d_tile_labels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && tile_xy && d_tile_labels && n_tiles >= 0, "bad arguments");
    for (int t = 0; t < n_tiles; ++t)
        REQUIRE(tile_xy[2 * t] >= 0 && tile_xy[2 * t] + c->in_W <= Wp && tile_xy[2 * t + 1] >= 0 && tile_xy[2 * t + 1] + c->in_H <= Hp,
                "tile %d at (%d,%d) leaves the %dx%d page", t, tile_xy[2 * t], tile_xy[2 * t + 1], Hp, Wp);
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = (const uint8_t*)d_page_hwc; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = Hp; ip.src_Wp = Wp; ip.tile_xy = c->d_tile_xy;
    const size_t per = (size_t)c->in_H * c->in_W;
    for (int done = 0; done < n_tiles; done += c->max_batch) {
        const int nb = n_tiles - done < c->max_batch ? n_tiles - done : c->max_batch;
        // explicit origin lists are the slow, general form: the table is re-used per chunk, so wait
        // for the previous chunk's ingest before overwriting it (the grid form below needs no table)
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(c->d_tile_xy, tile_xy + 2 * done, sizeof(int) * 2 * nb, hipMemcpyHostToDevice));
        ip.n_tiles = nb;
        HIPCHK(launch_ingest_u8(ip, c->precision, c->stream));
        if (run_plan(c, nb, (uint8_t*)d_tile_labels + done * per, nullptr)) return 1;
    }
    return 0;
    API_END
}

// Tile grid of the FUSED page paths: the reference's grid (sbbseg_tile_grid) minus the repeated last tile of an axis whose last two
// origins coincide (at most the last two can: three equal origins would need 2 * mid < tile - mid).  Origins are still
// min(t * mid, extent - tile) for t < n', so the ingest kernel's closed form holds on the smaller grid; the dropped tile's pixels
// [origin + margin, origin + tile) are exactly what tile n' - 1 pastes as the new last tile (axis_owner with dedupe).
static int fused_grid(const sbbseg_ctx* c, int Hp, int Wp, bool dedupe, int* nx, int* ny)
{
    if (sbbseg_tile_grid(Hp, Wp, c->in_H, c->in_W, nullptr, 0, nx, ny)) return 1;
    if (!dedupe) return 0;
    const int margin = margin_of(c->in_W);
    std::vector<int> o;
    if (axis_tiles(Wp, c->in_W, margin, o) >= 2 && o[o.size() - 1] == o[o.size() - 2]) --*nx;
    if (axis_tiles(Hp, c->in_H, margin, o) >= 2 && o[o.size() - 1] == o[o.size() - 2]) --*ny;
    return 0;
}

// ---- what the pooled tile paths share (tile_range_impl: pages of one size; sbbseg_segment_views_dev: views of any size) ----
// the plan's side of the owned-region geometry: levels, table kinds, output sizes (the page's side -- axes, grid -- is the caller's)
static void region_plan_levels(const sbbseg_ctx* c, RegionGeom& rg)
{
    rg.n_levels = c->region_levels;
    for (int L = 0; L < c->region_levels; ++L) {
        const Op& lop = c->ops[c->region_op[L]];
        if (L == 0) { rg.kind[L] = 0; rg.Rh[L] = c->in_H; rg.Rw[L] = c->in_W; rg.align_x[L] = 16; }
        else {
            const Tensor& to = c->tensors[lop.conv.d.out_tensor];
            rg.kind[L] = route_of(c, lop) == kRouteDecHalo ? 0 : 1;        // tile origins for dec_halo_*, class-grid pixels for conv_igemm_mfma
            rg.Rh[L] = to.H; rg.Rw[L] = to.W; rg.align_x[L] = 2;
        }
    }
}

// level L's table of the chunk of nb patches lane `lane` is about to run: `total` entries as the host counted them -> c->rr; the lane's buffer
// holds the largest table a full batch can need
static int region_level_table(sbbseg_ctx* c, int lane, const RegionGeom& rg, int L, int nb, long total)
{
    const size_t batch_cap = (size_t)(lane == 0 ? c->max_batch : c->lane1_batch);
    const size_t need = 4 * (rg.kind[L] ? 4 * batch_cap * (size_t)(rg.Rh[L] / 2) * (size_t)(rg.Rw[L] / 2)
                                         : batch_cap * (size_t)(rg.Rh[L] / 16 + 1) * (size_t)(rg.Rw[L] / 16 + 1));
    if (c->rtab[lane][L].cap < need) {
        HIPCHK(hipDeviceSynchronize());                  // (first use / a kind switched by an A/B knob: rare)
        if (ensure(c, c->rtab[lane][L], need)) return 1;
    }
    RegionRun& rr = c->rr;
    rr.kind[L] = rg.kind[L]; rr.total[L] = (int)total; rr.tab[L] = c->rtab[lane][L].p;
    rr.frac[L] = (double)total * (rg.kind[L] ? 4.0 : 256.0) / ((double)nb * rg.Rh[L] * rg.Rw[L]);
    return 0;
}

// Tiles [first_tile, first_tile + n_tiles) of the tile list of `n_pages` equally sized pages (page-major: tile g = page g / tpp,
// grid index g % tpp) -> d_tile_labels[g - first_tile].  Chunks of <= max_batch tiles may span pages: big launches fill the chip's
// persistent grids better than one page's 70 tiles (profiles/r02_experiments.md).
// `owned`: the decoder of every tile is launched over the region the page stitch keeps of it (+ the halo the levels above need) only
// (region.h) -- d_tile_labels is then defined on the owned regions, which is all stitch_impl reads.
static int tile_range_impl(sbbseg_ctx* c, const void* const* d_pages, int n_pages, int src_Hp, int src_Wp, const int* d_map_y, const int* d_map_x,
                           int Hp, int Wp, int first_tile, int n_tiles, void* d_tile_labels, const int* d_bin_thr = nullptr, bool dedupe = false,
                           bool owned = false)
{
    REQUIRE(d_pages && n_pages >= 1 && d_tile_labels && first_tile >= 0 && n_tiles >= 0, "bad arguments");
    for (int k = 0; k < n_pages; ++k) REQUIRE(d_pages[k], "null page pointer (page %d)", k);
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, dedupe, &nx, &ny)) return 1;
    const int tpp = nx * ny;
    REQUIRE((long)first_tile + n_tiles <= (long)tpp * n_pages, "tile range [%d,%d) exceeds the %d tiles of the %d page(s)", first_tile,
            first_tile + n_tiles, tpp * n_pages, n_pages);
    const int margin = margin_of(c->in_W);
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = (const uint8_t*)d_pages[0]; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = src_Hp; ip.src_Wp = src_Wp; ip.tile_xy = nullptr;
    ip.map_y = d_map_y; ip.map_x = d_map_x; ip.bin_thr = d_bin_thr;
    ip.grid_nyf = ny; ip.grid_mid_x = c->in_W - 2 * margin; ip.grid_mid_y = c->in_H - 2 * margin;
    const size_t per = (size_t)c->in_H * c->in_W;
    const size_t act = (size_t)c->elem * c->planes;          // bytes per stored element
    // owned-region launches: the page geometry in closed form; the tables of a chunk are built on its lane's stream in front of its forward
    const bool regions = owned && c->region_levels > 0 && c->max_batch <= kRegionMaxPatches;
    RegionGeom rg;
    memset(&rg, 0, sizeof(rg));
    if (regions) {
        rg.ax = {Wp, c->in_W, margin, c->in_W - 2 * margin, nx};
        rg.ay = {Hp, c->in_H, margin, c->in_H - 2 * margin, ny};
        rg.tpp = tpp; rg.ny = ny;
        region_plan_levels(c, rg);
    }
    auto setup_regions = [&](int lane, int g_first, int nb) -> int {       // (inside the lane's scope: c->stream is the lane's stream)
        RegionBuildParams bp;
        memset(&bp, 0, sizeof(bp));
        bp.g = rg; bp.g0 = g_first; bp.nb = nb;
        for (int L = 0; L < rg.n_levels; ++L) {
            long total = 0;
            for (int q = 0; q < nb; ++q) {
                const int local = (g_first + q) % tpp, i = local / ny, j = local - i * ny;
                total += region_entries(rg, i, j, L);
            }
            if (region_level_table(c, lane, rg, L, nb, total)) return 1;
            bp.out[L] = c->rtab[lane][L].p; bp.total[L] = (int)total;
        }
        HIPCHK(launch_region_build(bp, c->stream));
        c->rr.on = true;
        return 0;
    };
    auto run_chunk = [&](int lane, int first, int nb) -> int {
        LaneScope scope(c, lane);
        RegionOff roff{c};
        if (regions && setup_regions(lane, first_tile + first, nb)) return 1;
        IngestParams lp = ip;
        if (fill_ingest(c, lp)) return 1;          // (input-form pointers of this lane)
        char* const c8_base = (char*)lp.c8;
        char* const pairs_base = (char*)lp.pairs;
        const size_t c8_tile = per * 8 * act, pairs_tile = lp.pairs ? (size_t)(c->in_H + 2 * lp.pad) * lp.pairs_w * 8 * act : 0;
        lp.Hp = ip.Hp; lp.Wp = ip.Wp; lp.src_Hp = ip.src_Hp; lp.src_Wp = ip.src_Wp; lp.tile_xy = nullptr;
        lp.map_y = ip.map_y; lp.map_x = ip.map_x; lp.bin_thr = ip.bin_thr;
        lp.grid_nyf = ip.grid_nyf; lp.grid_mid_x = ip.grid_mid_x; lp.grid_mid_y = ip.grid_mid_y;
        for (int done = 0; done < nb;) {            // one ingest launch per page the chunk touches
            const int g = first_tile + first + done, pg = g / tpp, local = g - pg * tpp;
            const int run = nb - done < tpp - local ? nb - done : tpp - local;
            lp.page = (const uint8_t*)d_pages[pg];
            lp.grid_first = local;
            lp.n_tiles = run;
            lp.c8 = c8_base + (size_t)done * c8_tile;
            lp.pairs = pairs_base ? pairs_base + (size_t)done * pairs_tile : nullptr;
            HIPCHK(launch_ingest_u8(lp, c->precision, c->stream));
            done += run;
        }
        return run_plan(c, nb, (uint8_t*)d_tile_labels + first * per, nullptr);
    };
    return run_chunked(c, n_tiles, run_chunk);
}

int sbbseg_segment_tile_range_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int first_tile, int n_tiles,
                                  void* d_tile_labels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return tile_range_impl(c, &d_page_hwc, 1, Hp, Wp, nullptr, nullptr, Hp, Wp, first_tile, n_tiles, d_tile_labels, nullptr, false, c->owned_mode >= 2);
    API_END
}

static int prepare_owner(sbbseg_ctx* c, int Hp, int Wp, bool dedupe)
{
    if (c->own_Hp == Hp && c->own_Wp == Wp && c->own_dedupe == dedupe) return 0;
    alloc_check();
    std::vector<int> ox, oy, own_x, own_y;
    const int margin = margin_of(c->in_W);
    int nx = axis_tiles(Wp, c->in_W, margin, ox), ny = axis_tiles(Hp, c->in_H, margin, oy);
    REQUIRE_GEOMETRY(nx > 0 && ny > 0, "page %dx%d is smaller than the model input", Hp, Wp);
    if (dedupe) {                              // (fused_grid: the repeated last tile of an axis is not computed)
        if (nx >= 2 && ox[nx - 1] == ox[nx - 2]) ox.resize(--nx);
        if (ny >= 2 && oy[ny - 1] == oy[ny - 2]) oy.resize(--ny);
    }
    axis_owner(Wp, c->in_W, margin, ox, own_x);
    axis_owner(Hp, c->in_H, margin, oy, own_y);
    const size_t need = sizeof(int) * (size_t)(Hp > Wp ? Hp : Wp);
    if (ensure(c, c->own_x, need) || ensure(c, c->own_y, need)) return 1;      // (waits for the stream before it frees a table)
    HIPCHK(hipStreamSynchronize(c->stream));   // tables may still be in use by an earlier stitch
    HIPCHK(hipMemcpy(c->own_x.p, own_x.data(), sizeof(int) * Wp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->own_y.p, own_y.data(), sizeof(int) * Hp, hipMemcpyHostToDevice));
    c->own_Hp = Hp; c->own_Wp = Wp; c->own_nyf = ny; c->own_dedupe = dedupe;
    return 0;
}

static int stitch_impl(sbbseg_ctx* c, const void* d_tile_labels, int Hp, int Wp, void* d_labels_hw, bool dedupe)
{
    REQUIRE(d_tile_labels && d_labels_hw, "bad arguments");
    if (prepare_owner(c, Hp, Wp, dedupe)) return 1;
    HIPCHK(launch_stitch((const uint8_t*)d_tile_labels, c->in_H, c->in_W, c->own_x.p, c->own_y.p, c->own_nyf, Hp, Wp,
                         (uint8_t*)d_labels_hw, c->stream));
    return 0;
}

int sbbseg_stitch_dev(sbbseg_ctx* c, const void* d_tile_labels, int Hp, int Wp, void* d_labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return stitch_impl(c, d_tile_labels, Hp, Wp, d_labels_hw, false);      // tile labels in the reference's call order
    API_END
}

// The nearest maps "row / column of the Hs x Ws stored image shown at Hp x Wp -> stored row / column" (main.py:214 -> 112-113; the identity
// where the sizes agree), in c->map: built and uploaded once per geometry (map_key).
static int page_maps(sbbseg_ctx* c, int Hs, int Ws, int Hp, int Wp, const int** d_my, const int** d_mx)
{
    if (c->map_key[0] != Hs || c->map_key[1] != Ws || c->map_key[2] != Hp || c->map_key[3] != Wp || !c->map.p) {
        std::vector<int> my, mx;
        nearest_map(Hs, Hp, my);
        nearest_map(Ws, Wp, mx);
        if (ensure(c, c->map, sizeof(int) * (size_t)(Hp + Wp))) return 1;
        HIPCHK(hipStreamSynchronize(c->stream));   // the maps may still be in use by an earlier call
        HIPCHK(hipMemcpy(c->map.p, my.data(), sizeof(int) * Hp, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->map.p + Hp, mx.data(), sizeof(int) * Wp, hipMemcpyHostToDevice));
        c->map_key[0] = Hs; c->map_key[1] = Ws; c->map_key[2] = Hp; c->map_key[3] = Wp;
    }
    *d_my = c->map.p;
    *d_mx = c->map.p + Hp;
    return 0;
}

// One view through the fused page path: the box {cx, cy, cw, ch} of the Hs x Ws stored page at d_page as shown at Hp x Wp -> its label plane
// d_labels [ch][cw].  `mapped`: rows and columns are gathered through page_maps; without it the view is the whole page as stored (no box,
// Hs x Ws = Hp x Wp) and the ingest kernel reads it directly.  d_thr: otsu_copy first -- the threshold of exactly the view's pixels
// (channel 0) lands there and the tiles are binarised at it.  Then grid, tile-label scratch, the tiles, the stitch.
static int fused_view(sbbseg_ctx* c, const void* d_page, int Hs, int Ws, int Hp, int Wp, bool mapped, int cx, int cy, int cw, int ch, int* d_thr,
                      void* d_labels)
{
    const int *d_my = nullptr, *d_mx = nullptr;
    if (mapped) {
        if (page_maps(c, Hs, Ws, Hp, Wp, &d_my, &d_mx)) return 1;
        d_my += cy; d_mx += cx;
    }
    if (d_thr) HIPCHK(launch_otsu((const uint8_t*)d_page, Ws, ch, cw, d_my, d_mx, c->d_hist, d_thr, c->num_cus, c->stream));
    int nx = 0, ny = 0;
    if (fused_grid(c, ch, cw, c->dedupe, &nx, &ny)) return 1;
    if (ensure(c, c->tile_labels, (size_t)nx * ny * c->in_H * c->in_W)) return 1;
    if (tile_range_impl(c, &d_page, 1, Hs, Ws, d_my, d_mx, ch, cw, 0, nx * ny, c->tile_labels.p, d_thr, c->dedupe, c->owned_mode >= 1)) return 1;
    return stitch_impl(c, c->tile_labels.p, ch, cw, d_labels, c->dedupe);
}

// ... for a page in host memory: up into c->page, fused_view into c->page_labels, the labels (label_channels of them) and, with `binarise`,
// the Otsu threshold back; returns when both have arrived.
static int host_view(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, bool mapped, int cx, int cy, int cw, int ch, bool binarise,
                     uint8_t* labels_hw, int* threshold)
{
    const size_t spix = (size_t)Hs * Ws, pix = (size_t)ch * cw;
    if (ensure(c, c->page, spix * 3)) return 1;
    if (ensure(c, c->page_labels, pix + 4)) return 1;
    HIPCHK(hipMemcpyAsync(c->page.p, page_hwc, spix * 3, hipMemcpyHostToDevice, c->stream));
    int* d_thr = binarise ? (int*)(c->d_hist + 256) : nullptr;
    if (fused_view(c, c->page.p, Hs, Ws, Hp, Wp, mapped, cx, cy, cw, ch, d_thr, c->page_labels.p)) return 1;
    if (labels_to_host(c, c->page_labels.p, labels_hw, pix, c->label_channels)) return 1;
    int thr = 0;
    if (d_thr) HIPCHK(hipMemcpyAsync(&thr, d_thr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (threshold) *threshold = thr;
    return 0;
}

int sbbseg_segment_page_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, void* d_labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return fused_view(c, d_page_hwc, Hp, Wp, Hp, Wp, false, 0, 0, Wp, Hp, nullptr, d_labels_hw);
    API_END
}

int sbbseg_segment_pages_dev(sbbseg_ctx* c, int n_pages, const void* const* d_pages_hwc, int Hp, int Wp, void* const* d_labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_pages >= 1 && d_pages_hwc && d_labels_hw, "bad arguments");
    for (int k = 0; k < n_pages; ++k) REQUIRE(d_pages_hwc[k] && d_labels_hw[k], "null page / label pointer (page %d)", k);
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, c->dedupe, &nx, &ny)) return 1;
    const size_t per = (size_t)c->in_H * c->in_W, tpp = (size_t)nx * ny;
    // Pages are pooled in GROUPS whose tile count is a whole number of chunks where that is possible with few pages
    // (lcm(tiles per page, max_batch)), else about eight chunks: the tile-label scratch stays bounded by the group, not
    // by the caller's page count (64 pages of 4000x3000 would otherwise hold 1.4 GB of tile labels at once), and no
    // chunk is cut short except the very last.  Groups run back to back on the handle's stream (stream order protects the
    // scratch buffer that every group reuses).
    size_t a = tpp, b = (size_t)c->max_batch;
    while (b) { const size_t t = a % b; a = b; b = t; }                 // a = gcd
    size_t G = (size_t)c->max_batch / a;                                 // pages per group with G * tpp = lcm
    if (G > 32) G = (8 * (size_t)c->max_batch + tpp - 1) / tpp;
    if (G < 1) G = 1;
    if (G > (size_t)n_pages) G = (size_t)n_pages;
    REQUIRE(tpp * G < (size_t)1 << 30, "page group of %zu tiles is too large", tpp * G);
    if (ensure(c, c->tile_labels, tpp * G * per)) return 1;
    for (size_t g0 = 0; g0 < (size_t)n_pages; g0 += G) {
        const size_t np = g0 + G <= (size_t)n_pages ? G : (size_t)n_pages - g0;
        if (tile_range_impl(c, d_pages_hwc + g0, (int)np, Hp, Wp, nullptr, nullptr, Hp, Wp, 0, (int)(tpp * np), c->tile_labels.p, nullptr, c->dedupe, c->owned_mode >= 1)) return 1;
        for (size_t k = 0; k < np; ++k)
            if (stitch_impl(c, c->tile_labels.p + k * tpp * per, Hp, Wp, d_labels_hw[g0 + k], c->dedupe)) return 1;
    }
    return 0;
    API_END
}

// do_prediction(patches=True) for several HOST pages of one size, pipelined in groups of as many pages as fill a chunk:
// while group g runs on the handle's stream, the caller's thread stages group g+1 into pinned memory and starts its upload on
// a copy stream, and the label planes of group g-1 come back on another.  Results equal n_pages sbbseg_segment_page calls.
int sbbseg_segment_pages(sbbseg_ctx* c, int n_pages, const uint8_t* const* pages_hwc, int Hp, int Wp, uint8_t* const* labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_pages >= 1 && pages_hwc && labels_hw, "bad arguments");
    for (int k = 0; k < n_pages; ++k) REQUIRE(pages_hwc[k] && labels_hw[k], "null page / label pointer (page %d)", k);
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)", Hp, Wp, c->in_H, c->in_W);
    int nx = 0, ny = 0;
    if (fused_grid(c, Hp, Wp, c->dedupe, &nx, &ny)) return 1;
    const size_t pix = (size_t)Hp * Wp, in_b = pix * 3, ch = c->label_channels == 3 ? 3 : 1, out_b = pix * ch;
    const size_t out3_b = (pix + 3) / 4 * 12;                          // launch_replicate3 writes whole 12-byte groups
    int G = c->max_batch / (nx * ny);
    G = G < 1 ? 1 : (G > n_pages ? n_pages : G);
    if (!c->pp_ready) {                                                   // set LAST: a failed creation is retried by the next call
        if (!c->copy_in) HIPCHK(hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
        if (!c->copy_out) HIPCHK(hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            if (!c->pp_in[k]) HIPCHK(hipEventCreateWithFlags(&c->pp_in[k], hipEventDisableTiming));
            if (!c->pp_comp[k]) HIPCHK(hipEventCreateWithFlags(&c->pp_comp[k], hipEventDisableTiming));
            if (!c->pp_out[k]) HIPCHK(hipEventCreateWithFlags(&c->pp_out[k], hipEventDisableTiming));
        }
        c->pp_ready = true;
    }
    HIPCHK(hipStreamSynchronize(c->stream));                            // (buffers below may be re-allocated)
    // Every slot has its own capacity, and a pair serves only when BOTH slots hold `bytes`: a failed allocation leaves its slot "nothing
    // allocated" (devmem.h), which the next call sees and fills.
    auto pair = [&](DeviceMem& mem, DevBuf<uint8_t> (&b)[2], size_t bytes) -> int { return ensure(mem, b[0], bytes) || ensure(mem, b[1], bytes); };
    if (pair(c->pinned, c->pp_h_in, G * in_b)) return 1;
    if (pair(c->mem, c->pp_d_in, G * in_b)) return 1;
    if (pair(c->pinned, c->pp_h_out, G * out_b)) return 1;
    if (pair(c->mem, c->pp_d_out, G * (pix + 4))) return 1;               // one u8 plane (+4 bytes slack) per page, whatever label_channels is
    if (ch == 3 && pair(c->mem, c->pp_d_out3, G * out3_b)) return 1;
    const int n_groups = (n_pages + G - 1) / G;
    auto group_pages = [&](int g) { return g * G + G <= n_pages ? G : n_pages - g * G; };
    auto drain = [&](int g) -> int {                                      // labels of group g: staging -> caller
        const int slot = g & 1;
        HIPCHK(hipEventSynchronize(c->pp_out[slot]));
        for (int k = 0; k < group_pages(g); ++k) memcpy(labels_hw[g * G + k], c->pp_h_out[slot].p + (size_t)k * out_b, out_b);
        return 0;
    };
    alloc_check();
    std::vector<const void*> d_pages(G);
    std::vector<void*> d_labels(G);
    for (int g = 0; g < n_groups; ++g) {
        const int slot = g & 1, np = group_pages(g);
        if (g >= 2 && drain(g - 2)) return 1;                             // frees this slot's staging and device buffers
        for (int k = 0; k < np; ++k) memcpy(c->pp_h_in[slot].p + (size_t)k * in_b, pages_hwc[g * G + k], in_b);
        HIPCHK(hipMemcpyAsync(c->pp_d_in[slot].p, c->pp_h_in[slot].p, (size_t)np * in_b, hipMemcpyHostToDevice, c->copy_in));
        HIPCHK(hipEventRecord(c->pp_in[slot], c->copy_in));
        HIPCHK(hipStreamWaitEvent(c->stream, c->pp_in[slot], 0));
        for (int k = 0; k < np; ++k) {
            d_pages[k] = c->pp_d_in[slot].p + (size_t)k * in_b;
            d_labels[k] = c->pp_d_out[slot].p + (size_t)k * (pix + 4);
        }
        if (sbbseg_segment_pages_dev(c, np, d_pages.data(), Hp, Wp, d_labels.data())) return 1;
        const uint8_t* d_src = c->pp_d_out[slot].p;
        size_t d_stride = pix + 4;
        if (ch == 3) {
            for (int k = 0; k < np; ++k)
                HIPCHK(launch_replicate3(c->pp_d_out[slot].p + (size_t)k * (pix + 4), c->pp_d_out3[slot].p + (size_t)k * out3_b, pix, c->stream));
            d_src = c->pp_d_out3[slot].p;
            d_stride = out3_b;
        }
        HIPCHK(hipEventRecord(c->pp_comp[slot], c->stream));
        HIPCHK(hipStreamWaitEvent(c->copy_out, c->pp_comp[slot], 0));
        for (int k = 0; k < np; ++k)
            HIPCHK(hipMemcpyAsync(c->pp_h_out[slot].p + (size_t)k * out_b, d_src + (size_t)k * d_stride, out_b, hipMemcpyDeviceToHost, c->copy_out));
        HIPCHK(hipEventRecord(c->pp_out[slot], c->copy_out));
    }
    for (int g = n_groups >= 2 ? n_groups - 2 : 0; g < n_groups; ++g)
        if (drain(g)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_segment_page(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, uint8_t* labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw, "bad arguments");
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)", Hp, Wp, c->in_H, c->in_W);
    return host_view(c, page_hwc, Hp, Wp, Hp, Wp, false, 0, 0, Wp, Hp, false, labels_hw, nullptr);
    API_END
}

int sbbseg_segment_page_scaled(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, uint8_t* labels_hw)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw && Hs > 0 && Ws > 0, "bad arguments");
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "scaled page %dx%d is smaller than the model input %dx%d", Hp, Wp, c->in_H, c->in_W);
    return host_view(c, page_hwc, Hs, Ws, Hp, Wp, true, 0, 0, Wp, Hp, false, labels_hw, nullptr);
    API_END
}

int sbbseg_otsu_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int* d_threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && d_threshold && Hp > 0 && Wp > 0, "bad arguments");
    HIPCHK(launch_otsu((const uint8_t*)d_page_hwc, Wp, Hp, Wp, nullptr, nullptr, c->d_hist, d_threshold, c->num_cus, c->stream));
    return 0;
    API_END
}

int sbbseg_segment_tile_range_bin_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int first_tile, int n_tiles,
                                      const int* d_threshold, void* d_tile_labels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_threshold, "bad arguments");
    return tile_range_impl(c, &d_page_hwc, 1, Hp, Wp, nullptr, nullptr, Hp, Wp, first_tile, n_tiles, d_tile_labels, d_threshold, false, c->owned_mode >= 2);
    API_END
}

int sbbseg_segment_page_otsu(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, uint8_t* labels_hw,
                             int* threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw && Hs > 0 && Ws > 0, "bad arguments");
    REQUIRE_GEOMETRY(Hp >= c->in_H && Wp >= c->in_W, "page %dx%d is smaller than the model input %dx%d", Hp, Wp, c->in_H, c->in_W);
    return host_view(c, page_hwc, Hs, Ws, Hp, Wp, Hs != Hp || Ws != Wp, 0, 0, Wp, Hp, true, labels_hw, threshold);
    API_END
}

// The patch stages of run() on the CROPPED page (main.py:2061-2102: extract_page's croped_page goes to extract_text_regions and
// textline_contours): the crop box lives in the coordinates of the page as upscaled to Hp x Wp, the stored image is Hs x Ws.
// Rescale, crop and (binarise != 0) otsu_copy are all index arithmetic in the tile gather: row r / column q of the crop read
// stored row map_y[cy + r] / column map_x[cx + q]; the Otsu histogram is taken over exactly those pixels (channel 0).
static int check_crop(const sbbseg_ctx* c, int Hs, int Ws, int Hp, int Wp, int cx, int cy, int cw, int ch)
{
    REQUIRE(Hs > 0 && Ws > 0 && Hp > 0 && Wp > 0, "bad arguments");
    REQUIRE(cx >= 0 && cy >= 0 && cw > 0 && ch > 0 && cx + cw <= Wp && cy + ch <= Hp, "crop box {%d,%d,%d,%d} leaves the %dx%d page", cx, cy, cw, ch, Hp, Wp);
    REQUIRE_GEOMETRY(ch >= c->in_H && cw >= c->in_W, "cropped page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)",
            ch, cw, c->in_H, c->in_W);
    return 0;
}

int sbbseg_segment_crop_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hs, int Ws, int Hp, int Wp, int cx, int cy, int cw, int ch,
                            int binarise, void* d_labels_hw, int* d_threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && d_labels_hw, "bad arguments");
    if (check_crop(c, Hs, Ws, Hp, Wp, cx, cy, cw, ch)) return 1;
    int* d_thr = !binarise ? nullptr : d_threshold ? d_threshold : (int*)(c->d_hist + 256);
    return fused_view(c, d_page_hwc, Hs, Ws, Hp, Wp, true, cx, cy, cw, ch, d_thr, d_labels_hw);     // (the identity maps when Hs x Ws = Hp x Wp)
    API_END
}

int sbbseg_segment_crop(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, int cx, int cy, int cw, int ch,
                        int binarise, uint8_t* labels_hw, int* threshold)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_hw && Hs > 0 && Ws > 0 && cw > 0 && ch > 0, "bad arguments");
    if (check_crop(c, Hs, Ws, Hp, Wp, cx, cy, cw, ch)) return 1;
    return host_view(c, page_hwc, Hs, Ws, Hp, Wp, true, cx, cy, cw, ch, binarise != 0, labels_hw, threshold);
    API_END
}

// ---- many views in one call: tiles of differently sized pages and crops share launches (include/sbbseg.h) ----
// Per call: the view table (region.h ViewRec), a fallback threshold int per view and the nearest maps of the rescaled views are laid out in
// pinned staging and go up in one asynchronous copy; per group of views (about eight chunks of tiles, which bounds the tile-label scratch):
// the pooled tile list through run_chunked -- one ingest and one region-table launch per lane-chunk -- and one stitch launch.
int sbbseg_segment_views_dev(sbbseg_ctx* c, int n_views, const sbbseg_view* views)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_views >= 1, "n_views %d < 1", n_views);
    REQUIRE(views, "null view array");
    alloc_check();
    const int margin = margin_of(c->in_W);
    const size_t per = (size_t)c->in_H * c->in_W;
    struct Group { int v0, v1, tiles; unsigned blocks; };
    struct MapAt { int src, dst, off; };
    std::vector<ViewRec> recs(n_views);
    std::vector<Group> groups;
    std::vector<MapAt> map_at;
    std::vector<int> maps, one;
    auto map_offset = [&](int src, int dst) -> int {          // (the views of one document share their maps)
        for (const MapAt& m : map_at)
            if (m.src == src && m.dst == dst) return m.off;
        nearest_map(src, dst, one);        // scaled row -> stored row   (main.py:214 -> 112-113)
        map_at.push_back({src, dst, (int)maps.size()});
        maps.insert(maps.end(), one.begin(), one.end());
        return map_at.back().off;
    };
    const int group_cap = 8 * c->max_batch;
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_view& v = views[k];
        REQUIRE(v.d_page_hwc && v.d_labels_hw, "view %d: null page / label pointer", k);
        REQUIRE(v.Hs > 0 && v.Ws > 0 && v.Hp > 0 && v.Wp > 0, "view %d: bad page size %dx%d (stored %dx%d)", k, v.Hp, v.Wp, v.Hs, v.Ws);
        REQUIRE(v.cx >= 0 && v.cy >= 0 && v.cw > 0 && v.ch > 0 && (long)v.cx + v.cw <= v.Wp && (long)v.cy + v.ch <= v.Hp,
                "view %d: crop box {%d,%d,%d,%d} leaves the %dx%d page", k, v.cx, v.cy, v.cw, v.ch, v.Hp, v.Wp);
        REQUIRE_GEOMETRY(v.ch >= c->in_H && v.cw >= c->in_W, "view %d: cropped page %dx%d is smaller than the model input %dx%d (unsupported by the reference too, main.py:278-281)",
                k, v.ch, v.cw, c->in_H, c->in_W);
        ViewRec& r = recs[k];
        memset(&r, 0, sizeof(r));
        if (fused_grid(c, v.ch, v.cw, c->dedupe, &r.nx, &r.ny)) return 1;
        r.page = (const uint8_t*)v.d_page_hwc; r.labels = (uint8_t*)v.d_labels_hw; r.src_Wp = v.Ws; r.cw = v.cw; r.ch = v.ch;
        r.n_tiles = r.nx * r.ny;
        REQUIRE(r.n_tiles < 1 << 30, "view %d: %d x %d tiles are too many", k, r.nx, r.ny);
        r.mapped = v.Hs != v.Hp || v.Ws != v.Wp;
        r.my = r.mapped ? map_offset(v.Hs, v.Hp) + v.cy : v.cy;
        r.mx = r.mapped ? map_offset(v.Ws, v.Wp) + v.cx : v.cx;
        if (groups.empty() || groups.back().tiles + r.n_tiles > group_cap) groups.push_back({k, k, 0, 0u});
        Group& g = groups.back();
        r.first = g.tiles; r.blk_first = g.blocks;
        const size_t blocks = ((size_t)v.ch * v.cw + 255) / 256;
        REQUIRE(g.blocks + blocks < (size_t)1 << 31, "view %d: the group's label planes are too large for one stitch launch", k);
        g.v1 = k + 1; g.tiles += r.n_tiles; g.blocks += (unsigned)blocks;
    }
    size_t most = 0;
    for (const Group& g : groups) most = most > (size_t)g.tiles ? most : (size_t)g.tiles;
    // one buffer: [n_views] ViewRec | [n_views] int thresholds (views that bring no device int of their own) | maps
    const size_t thr_at = sizeof(ViewRec) * (size_t)n_views, maps_at = thr_at + sizeof(int) * (size_t)n_views;
    const size_t bytes = maps_at + sizeof(int) * maps.size();
    if (views_staging(c, bytes)) return 1;
    if (ensure(c, c->tile_labels, most * per)) return 1;
    const ViewRec* d_recs = (const ViewRec*)c->views.p;
    int* d_thr = (int*)((char*)c->views.p + thr_at);
    const int* d_maps = (const int*)((char*)c->views.p + maps_at);
    for (int k = 0; k < n_views; ++k) recs[k].thr = views[k].binarise ? (views[k].d_threshold ? views[k].d_threshold : d_thr + k) : nullptr;
    memcpy(c->h_views.p, recs.data(), thr_at);
    memset((char*)c->h_views.p + thr_at, 0, maps_at - thr_at);
    if (!maps.empty()) memcpy((char*)c->h_views.p + maps_at, maps.data(), sizeof(int) * maps.size());
    HIPCHK(hipMemcpyAsync(c->views.p, c->h_views.p, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_views, c->stream));
    c->views_copy_pending = true;
    c->d_views_thr = d_thr;
    for (int k = 0; k < n_views; ++k) {                        // otsu_copy over exactly the crop's pixels (channel 0), view by view
        const ViewRec& r = recs[k];
        if (!r.thr) continue;
        const uint8_t* pg = r.mapped ? r.page : r.page + ((size_t)r.my * r.src_Wp + r.mx) * 3;
        HIPCHK(launch_otsu(pg, r.src_Wp, r.ch, r.cw, r.mapped ? d_maps + r.my : nullptr, r.mapped ? d_maps + r.mx : nullptr, c->d_hist,
                           (int*)r.thr, c->num_cus, c->stream));
    }
    const bool regions = c->owned_mode >= 1 && c->region_levels > 0 && c->max_batch <= kRegionMaxPatches;
    RegionViewsBuildParams bp;
    memset(&bp, 0, sizeof(bp));
    if (regions) region_plan_levels(c, bp.g);
    bp.tile_h = c->in_H; bp.tile_w = c->in_W; bp.margin = margin;
    for (const Group& g : groups) {
        const ViewRec* gv = recs.data() + g.v0;
        const int nv = g.v1 - g.v0;
        auto run_chunk = [&](int lane, int first, int nb) -> int {
            LaneScope scope(c, lane);
            RegionOff roff{c};
            if (regions) {                                     // the chunk's tables, on the lane's stream in front of its forward
                RegionViewsBuildParams lp = bp;
                lp.views = d_recs + g.v0; lp.n_views = nv; lp.g0 = first; lp.nb = nb;
                for (int L = 0; L < lp.g.n_levels; ++L) {
                    long total = 0;
                    for (int q = 0, w = view_find(nv, (unsigned)first, [&](int m) { return (unsigned)gv[m].first; }); q < nb; ++q) {
                        while (first + q >= gv[w].first + gv[w].n_tiles) ++w;
                        const int local = first + q - gv[w].first, i = local / gv[w].ny, j = local - i * gv[w].ny;
                        total += region_entries(lp.g, view_axis_x(gv[w], c->in_W, margin), view_axis_y(gv[w], c->in_H, margin), i, j, L);
                    }
                    if (region_level_table(c, lane, lp.g, L, nb, total)) return 1;
                    lp.out[L] = c->rtab[lane][L].p; lp.total[L] = (int)total;
                }
                HIPCHK(launch_region_build_views(lp, c->stream));
                c->views_launches += 1;
                c->rr.on = true;
            }
            IngestParams fp;
            if (fill_ingest(c, fp)) return 1;                  // (input-form pointers of this lane)
            IngestViewsParams ip;
            memset(&ip, 0, sizeof(ip));
            ip.views = d_recs + g.v0; ip.maps = d_maps; ip.n_views = nv; ip.g0 = first; ip.n_tiles = nb;
            ip.H = c->in_H; ip.W = c->in_W; ip.margin = margin; ip.lut = fp.lut; ip.c8 = fp.c8; ip.pairs = fp.pairs; ip.pad = fp.pad; ip.pairs_w = fp.pairs_w;
            HIPCHK(launch_ingest_views(ip, c->precision, c->stream));
            c->views_launches += 1;
            return run_plan(c, nb, c->tile_labels.p + (size_t)first * per, nullptr);
        };
        if (run_chunked(c, g.tiles, run_chunk)) return 1;
        HIPCHK(launch_stitch_views(c->tile_labels.p, c->in_H, c->in_W, margin, d_recs + g.v0, nv, g.blocks, c->stream));
        c->views_launches += 1;
    }
    return 0;
    API_END
}

int sbbseg_segment_views(sbbseg_ctx* c, int n_views, const sbbseg_view* views_host_pointers, int* thresholds)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(n_views >= 1, "n_views %d < 1", n_views);
    REQUIRE(views_host_pointers, "null view array");
    alloc_check();
    std::vector<sbbseg_view> dv(views_host_pointers, views_host_pointers + n_views);
    std::vector<size_t> page_at(n_views), plane_at(n_views);
    size_t page_bytes = 0, plane_bytes = 0, most_pix = 0;
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_view& v = dv[k];
        REQUIRE(v.d_page_hwc && v.d_labels_hw, "view %d: null page / label pointer", k);
        REQUIRE(v.Hs > 0 && v.Ws > 0 && v.cw > 0 && v.ch > 0, "view %d: bad page or crop size", k);
        int same = 0;
        while (same < k && dv[same].d_page_hwc != v.d_page_hwc) ++same;
        if (same < k) {
            REQUIRE(dv[same].Hs == v.Hs && dv[same].Ws == v.Ws, "view %d: the page of view %d with another stored size", k, same);
            page_at[k] = page_at[same];
        } else {
            page_at[k] = page_bytes;
            page_bytes += ((size_t)v.Hs * v.Ws * 3 + 15) & ~(size_t)15;
        }
        const size_t pix = (size_t)v.ch * v.cw;
        plane_at[k] = plane_bytes;
        plane_bytes += (pix + 4 + 15) & ~(size_t)15;
        most_pix = most_pix > pix ? most_pix : pix;
    }
    if (ensure(c, c->page, page_bytes)) return 1;
    if (ensure(c, c->page_labels, plane_bytes)) return 1;
    if (c->label_channels == 3 && ensure(c, c->page_labels3, (most_pix + 3) / 4 * 12)) return 1;
    for (int k = 0; k < n_views; ++k) {
        int same = 0;
        while (dv[same].d_page_hwc != dv[k].d_page_hwc) ++same;
        if (same == k)
            HIPCHK(hipMemcpyAsync(c->page.p + page_at[k], views_host_pointers[k].d_page_hwc, (size_t)dv[k].Hs * dv[k].Ws * 3, hipMemcpyHostToDevice, c->stream));
    }
    for (int k = 0; k < n_views; ++k) {                        // (after the search above: it compares the caller's host pointers)
        dv[k].d_page_hwc = c->page.p + page_at[k];
        dv[k].d_labels_hw = c->page_labels.p + plane_at[k];
        dv[k].d_threshold = nullptr;
    }
    if (sbbseg_segment_views_dev(c, n_views, dv.data())) {
        (void)hipStreamSynchronize(c->stream);                 // (the uploads read the caller's pages)
        return 1;
    }
    for (int k = 0; k < n_views; ++k)
        if (labels_to_host(c, c->page_labels.p + plane_at[k], views_host_pointers[k].d_labels_hw, (size_t)dv[k].ch * dv[k].cw, c->label_channels)) return 1;
    std::vector<int> thr(n_views, 0);
    HIPCHK(hipMemcpyAsync(thr.data(), c->d_views_thr, sizeof(int) * (size_t)n_views, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (thresholds)
        for (int k = 0; k < n_views; ++k) thresholds[k] = dv[k].binarise ? thr[k] : 0;
    return 0;
    API_END
}

int sbbseg_debug_axis_owner(int extent, int tile, int margin, int n_tiles, int32_t* own)
{
    API_BEGIN
    REQUIRE(own && tile > 2 * margin && margin >= 0 && extent >= tile && n_tiles >= 1, "bad arguments");
    const RegionAxis a = {extent, tile, margin, tile - 2 * margin, n_tiles};
    for (int q = 0; q < extent; ++q) own[q] = region_owner(a, q);
    return 0;
    API_END
}

}  // extern "C"
