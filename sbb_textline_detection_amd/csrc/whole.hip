// whole.hip -- do_prediction(patches=False) (main.py:368-380), the whole-image branch, for one page and for many; extract_page's box on top of it;
// and the model-running part of run() for one page and for many (sbbseg_run_page, sbbseg_run_pages).
#include <string.h>

#include "exec.h"

using namespace sbbseg;

extern "C" {

int sbbseg_segment_whole(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int out_h, int out_w, uint8_t* labels_out)
{
    API_BEGIN
    return sbbseg_segment_whole_scaled(c, page_hwc, Hp, Wp, Hp, Wp, out_h, out_w, labels_out);
    API_END
}

// One gather map of the whole-image branch.  page > 0: model index -> index into the stored image, through the page do_prediction was handed
// (main.py:371), which is itself the nearest-upscaled stored image where the two sizes differ (main.py:214: composed).  page == 0: index of
// an output axis of length `stored` -> model index (main.py:378).
static void whole_map(int stored, int page, int model, std::vector<int>& m)
{
    if (page == 0) { nearest_map(model, stored, m); return; }
    nearest_map(page, model, m);
    if (page != stored) {
        std::vector<int> s;
        nearest_map(stored, page, s);
        for (auto& q : m) q = s[q];
    }
}

// do_prediction(patches=False) on the page as upscaled to Hs x Ws: the page comes from host memory (page_hwc) or is already on the
// device (d_page_in); the label plane lands in c->page_labels and, if labels_out is given, in host memory too -- or, with d_dst, in that
// device buffer alone (labels_out is then NULL).
static int whole_scaled_impl(sbbseg_ctx* c, const uint8_t* page_hwc, const void* d_page_in, int Hp, int Wp, int Hs, int Ws, int out_h, int out_w,
                             uint8_t* labels_out, void* d_dst = nullptr)
{
    const size_t pix = (size_t)Hp * Wp, opix = (size_t)out_h * out_w;
    if (!d_page_in && ensure(c, c->page, pix * 3)) return 1;
    if (!d_dst && ensure(c, c->page_labels, opix + 4)) return 1;
    const size_t need = sizeof(int) * (size_t)(c->in_H + c->in_W + out_h + out_w);
    const bool cached = c->wmap.p && c->wmap.cap >= need && c->wmap_key[0] == Hp && c->wmap_key[1] == Wp && c->wmap_key[2] == Hs &&
                        c->wmap_key[3] == Ws && c->wmap_key[4] == out_h && c->wmap_key[5] == out_w;
    if (!cached) {                         // the four gather tables depend on the sizes only: built and uploaded once per geometry
        std::vector<int> my, mx, oy, ox;
        whole_map(Hp, Hs, c->in_H, my);
        whole_map(Wp, Ws, c->in_W, mx);
        whole_map(out_h, 0, c->in_H, oy);
        whole_map(out_w, 0, c->in_W, ox);
        if (ensure(c, c->wmap, need)) return 1;
        memset(c->wmap_key, 0, sizeof(c->wmap_key));      // (none while the tables are rewritten: a failed copy must not leave the old key)
        int* d_my = c->wmap.p; int* d_mx = d_my + c->in_H; int* d_oy = d_mx + c->in_W; int* d_ox = d_oy + out_h;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(d_my, my.data(), sizeof(int) * c->in_H, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_mx, mx.data(), sizeof(int) * c->in_W, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_oy, oy.data(), sizeof(int) * out_h, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ox, ox.data(), sizeof(int) * out_w, hipMemcpyHostToDevice));
        c->wmap_key[0] = Hp; c->wmap_key[1] = Wp; c->wmap_key[2] = Hs; c->wmap_key[3] = Ws; c->wmap_key[4] = out_h; c->wmap_key[5] = out_w;
    }
    int* d_my = c->wmap.p; int* d_mx = d_my + c->in_H; int* d_oy = d_mx + c->in_W; int* d_ox = d_oy + out_h;
    if (!d_page_in) HIPCHK(hipMemcpyAsync(c->page.p, page_hwc, pix * 3, hipMemcpyHostToDevice, c->stream));
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = d_page_in ? (const uint8_t*)d_page_in : c->page.p; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = Hp; ip.src_Wp = Wp; ip.tile_xy = nullptr; ip.n_tiles = 1;
    ip.whole = 1; ip.map_y = d_my; ip.map_x = d_mx;
    HIPCHK(launch_ingest_u8(ip, c->precision, c->stream));
    {
        KsplitScope scope(c);
        if (run_plan(c, 1, c->d_batch_labels, nullptr)) return 1;
    }
    HIPCHK(launch_resize_labels(c->d_batch_labels, c->in_H, c->in_W, d_oy, d_ox, out_h, out_w, d_dst ? (uint8_t*)d_dst : c->page_labels.p, c->stream));
    if (labels_out) {
        if (labels_to_host(c, c->page_labels.p, labels_out, opix, c->label_channels)) return 1;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int sbbseg_segment_whole_scaled(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws, int out_h, int out_w,
                                uint8_t* labels_out)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && labels_out && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0 && out_h > 0 && out_w > 0, "bad arguments");
    return whole_scaled_impl(c, page_hwc, nullptr, Hp, Wp, Hs, Ws, out_h, out_w, labels_out);
    API_END
}

// ---- the whole-image branch for many pages in shared launches (include/sbbseg.h): one patch per view, chunks of <= max_batch patches one
// after the other on the handle's stream.  Per call the view table (internal.h WholeViewRec) and every view's four nearest maps -- the
// composed model -> page -> stored maps and the output -> model maps of whole_scaled_impl, shared between views of equal geometry -- go up
// in one asynchronous copy; per chunk one ingest and one label-resize launch.  n_views == 1 is whole_scaled_impl itself (split-K as the
// handle has it); from two views on nothing splits: ksplit_now is only ever set inside whole_scaled_impl.
static int check_whole_views(int n_views, const sbbseg_whole_view* views, bool planes_required)
{
    REQUIRE(n_views >= 1, "n_views %d < 1", n_views);
    REQUIRE(views, "null view array");
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_whole_view& v = views[k];
        REQUIRE(v.d_page_hwc && (v.d_labels_out || !planes_required), "view %d: null page / label pointer", k);
        REQUIRE(v.stored_h > 0 && v.stored_w > 0 && v.page_h > 0 && v.page_w > 0 && v.out_h > 0 && v.out_w > 0,
                "view %d: bad size (stored %dx%d, page %dx%d, labels %dx%d)", k, v.stored_h, v.stored_w, v.page_h, v.page_w, v.out_h, v.out_w);
    }
    return 0;
}

static int whole_views_impl(sbbseg_ctx* c, int n_views, const sbbseg_whole_view* views)
{
    if (check_whole_views(n_views, views, true)) return 1;
    if (n_views == 1) {
        const sbbseg_whole_view& v = views[0];
        if (whole_scaled_impl(c, nullptr, v.d_page_hwc, v.stored_h, v.stored_w, v.page_h, v.page_w, v.out_h, v.out_w, nullptr, v.d_labels_out)) return 1;
        c->whole_launches += 2;
        return 0;
    }
    alloc_check();
    // chunks of equal size, as run_chunked cuts a tile list (9 views at max_batch 4: 3 + 3 + 3)
    const int n_chunks = (n_views + c->max_batch - 1) / c->max_batch, chunk = (n_views + n_chunks - 1) / n_chunks;
    struct MapAt { int a, b, m, off; };
    std::vector<MapAt> map_at;
    std::vector<int> maps, one;
    auto map_offset = [&](int stored, int page, int model) -> int {       // (whole_map's arguments; views of equal geometry share their maps)
        for (const MapAt& m : map_at)
            if (m.a == stored && m.b == page && m.m == model) return m.off;
        whole_map(stored, page, model, one);
        map_at.push_back({stored, page, model, (int)maps.size()});
        maps.insert(maps.end(), one.begin(), one.end());
        return map_at.back().off;
    };
    std::vector<WholeViewRec> recs(n_views);
    std::vector<unsigned> chunk_blocks(n_chunks, 0u);
    for (int k = 0; k < n_views; ++k) {
        const sbbseg_whole_view& v = views[k];
        WholeViewRec& r = recs[k];
        memset(&r, 0, sizeof(r));
        r.page = (const uint8_t*)v.d_page_hwc; r.out = (uint8_t*)v.d_labels_out; r.stored_w = v.stored_w; r.out_h = v.out_h; r.out_w = v.out_w;
        r.my = map_offset(v.stored_h, v.page_h, c->in_H); r.mx = map_offset(v.stored_w, v.page_w, c->in_W);
        r.oy = map_offset(v.out_h, 0, c->in_H); r.ox = map_offset(v.out_w, 0, c->in_W);
        r.lead = (unsigned)((uintptr_t)v.d_labels_out & 15);
        unsigned& blocks = chunk_blocks[k / chunk];
        r.blk_first = blocks;
        const size_t nb = ((size_t)r.lead + (size_t)v.out_h * v.out_w + kResizeViewsBlockBytes - 1) / kResizeViewsBlockBytes;
        REQUIRE(blocks + nb < (size_t)1 << 31, "view %d: the chunk's label planes are too large for one resize launch", k);
        blocks += (unsigned)nb;
    }
    const size_t maps_at = sizeof(WholeViewRec) * (size_t)n_views, bytes = maps_at + sizeof(int) * maps.size();
    if (views_staging(c, bytes)) return 1;
    memcpy(c->h_views.p, recs.data(), maps_at);
    memcpy((char*)c->h_views.p + maps_at, maps.data(), sizeof(int) * maps.size());
    HIPCHK(hipMemcpyAsync(c->views.p, c->h_views.p, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_views, c->stream));
    c->views_copy_pending = true;
    const WholeViewRec* d_recs = (const WholeViewRec*)c->views.p;
    const int* d_maps = (const int*)((char*)c->views.p + maps_at);
    for (int q = 0, first = 0; first < n_views; ++q, first += chunk) {
        const int nb = n_views - first < chunk ? n_views - first : chunk;
        IngestParams fp;
        if (fill_ingest(c, fp)) return 1;
        IngestWholeViewsParams ip;
        memset(&ip, 0, sizeof(ip));
        ip.views = d_recs + first; ip.maps = d_maps; ip.n_views = nb; ip.H = c->in_H; ip.W = c->in_W;
        ip.lut = fp.lut; ip.c8 = fp.c8; ip.pairs = fp.pairs; ip.pad = fp.pad; ip.pairs_w = fp.pairs_w;
        HIPCHK(launch_ingest_whole_views(ip, c->precision, c->stream));
        if (run_plan(c, nb, c->d_batch_labels, nullptr)) return 1;              // (ksplit_now is false: no launch splits, whatever nb is)
        HIPCHK(launch_resize_labels_views(c->d_batch_labels, c->in_H, c->in_W, d_recs + first, d_maps, nb, chunk_blocks[q], c->stream));
        c->whole_launches += 2;
    }
    return 0;
}

int sbbseg_segment_whole_views_dev(sbbseg_ctx* c, int n_views, const sbbseg_whole_view* views)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    return whole_views_impl(c, n_views, views);
    API_END
}

int sbbseg_extract_page_box(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws, uint8_t* mask_out, int32_t* box_xywh,
                            int64_t* pixels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && box_xywh && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0, "bad arguments");
    // border model on the (virtually) upscaled page, result at the upscaled size (main.py:384-392) ...  (mask_out == NULL: the mask --
    // a local of extract_page in the reference -- stays on the device)
    if (whole_scaled_impl(c, page_hwc, nullptr, Hp, Wp, Hs, Ws, Hs, Ws, mask_out)) return 1;
    // ... whose label plane is still in c->page_labels: threshold, dilate x 6, largest component, bounding box (main.py:394-404)
    return sbbseg_page_box_dev(c, c->page_labels.p, Hs, Ws, box_xywh, pixels);
    API_END
}

int sbbseg_extract_page_box_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int Hs, int Ws, void* d_mask_out, int32_t* box_xywh,
                                int64_t* pixels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(d_page_hwc && box_xywh && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0, "bad arguments");
    if (whole_scaled_impl(c, nullptr, d_page_hwc, Hp, Wp, Hs, Ws, Hs, Ws, nullptr)) return 1;
    if (d_mask_out) HIPCHK(hipMemcpyAsync(d_mask_out, c->page_labels.p, (size_t)Hs * Ws, hipMemcpyDeviceToDevice, c->stream));
    return sbbseg_page_box_dev(c, c->page_labels.p, Hs, Ws, box_xywh, pixels);
    API_END
}

// extract_page's model + glue for many pages: the border forwards at batch width (whole_views_impl), then the box search plane by plane.
int sbbseg_extract_page_boxes_dev(sbbseg_ctx* c, int n_pages, const sbbseg_whole_view* views, int32_t* boxes_xywh, int64_t* pixels)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(boxes_xywh, "bad arguments");
    if (check_whole_views(n_pages, views, false)) return 1;
    alloc_check();
    std::vector<sbbseg_whole_view> v(views, views + n_pages);
    std::vector<size_t> at(n_pages, 0);
    size_t scratch = 0;
    for (int k = 0; k < n_pages; ++k) {
        REQUIRE(v[k].out_h == v[k].page_h && v[k].out_w == v[k].page_w, "view %d: the mask %dx%d must have the page's size %dx%d", k, v[k].out_h, v[k].out_w,
                v[k].page_h, v[k].page_w);
        REQUIRE((size_t)v[k].page_h * v[k].page_w < ((size_t)1 << 31), "view %d: mask too large for 32-bit pixel indices", k);
        if (v[k].d_labels_out) continue;
        at[k] = scratch;
        scratch += ((size_t)v[k].page_h * v[k].page_w + 15) & ~(size_t)15;
    }
    if (scratch && ensure(c, c->page_labels, scratch + 16)) return 1;      // (the masks nobody asked for)
    for (int k = 0; k < n_pages; ++k)
        if (!v[k].d_labels_out) v[k].d_labels_out = c->page_labels.p + at[k];
    if (whole_views_impl(c, n_pages, v.data())) return 1;
    for (int k = 0; k < n_pages; ++k) {                        // main.py:394-404 per plane; an empty mask: {0, 0, 0, 0} / 0
        int64_t px = 0;
        if (sbbseg_page_box_dev(c, v[k].d_labels_out, v[k].page_h, v[k].page_w, boxes_xywh + 4 * k, &px)) return 1;
        if (pixels) pixels[k] = px;
    }
    return 0;
    API_END
}

// A stage of sbbseg_run_page(s) failed on handle h: wait for whatever it had queued on either lane, with the failure's message and kind kept
// for the caller.  Returns 1, the failed call's status.
static int drain_after_failure(sbbseg_ctx* h)
{
    const std::string msg = g_err;
    const int kind = g_err_kind;
    (void)hipStreamSynchronize(h->stream);
    if (h->lane_stream) (void)hipStreamSynchronize(h->lane_stream);
    (void)hipGetLastError();
    g_err = msg; g_err_kind = kind;
    return 1;
}

// ---- the model-running part of run() (main.py:2056-2107) in ONE call: the stored page is uploaded once and stays in device memory for
// all three stages, the border mask and the region map never leave the device between their model and their glue.
//   extract_page (main.py:2061, 384-437)            border model on the page as upscaled to Hs x Ws, dilate x 6, largest contour, box;
//                                                   outside the reference's try: an error here is the call's error
//   extract_text_regions (2072, 439-454)            layout model on the Otsu'd CROP, erode x 3 / dilate x 4 (2074-2075); a failure --
//                                                   e.g. a crop smaller than the model input, main.py:278-285 -- is "no regions" (2089-2091)
//   get_text_region_contours_and_boxes (2083, 2096) existence only: the textline model runs when a contour would be kept
//   textline_contours (2102, 490-503)               textline model on the crop
int sbbseg_run_page(sbbseg_ctx* border, sbbseg_ctx* layout, sbbseg_ctx* textline, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws,
                    int channels, uint8_t* page_mask_out, uint8_t* regions_out, uint8_t* textlines_out, sbbseg_run_info* info)
{
    API_BEGIN
    if (check_ready(border) || check_ready(layout) || check_ready(textline)) return 1;
    REQUIRE(page_hwc && info && regions_out && textlines_out && Hp > 0 && Wp > 0 && Hs > 0 && Ws > 0 && (channels == 1 || channels == 3), "bad arguments");
    REQUIRE(border->device == layout->device && border->device == textline->device, "the three handles must live on one device");
    border->run_planes_valid = layout->run_planes_valid = textline->run_planes_valid = false;      // (the call rewrites the resident planes)
    memset(info, 0, sizeof(*info));
    const size_t spix = (size_t)Hp * Wp, pix = (size_t)Hs * Ws;
    if (ensure(border, border->run_page, spix * 3)) return 1;
    if (page_mask_out && ensure(border, border->run_mask, pix)) return 1;
    HIPCHK(hipMemcpyAsync(border->run_page.p, page_hwc, spix * 3, hipMemcpyHostToDevice, border->stream));      // the one upload of the page
    int64_t pixels = 0;
    if (sbbseg_extract_page_box_dev(border, border->run_page.p, Hp, Wp, Hs, Ws, page_mask_out ? border->run_mask.p : nullptr, info->box_xywh, &pixels)) return 1;
    info->box_pixels = pixels;                                  // (extract_page_box_dev has synchronised the border handle's stream)
    REQUIRE(pixels > 0, "attempt to get argmax of an empty sequence (the border model found no page: main.py:399-401 raises here)");
    if (page_mask_out && sbbseg_download_labels(border, page_mask_out, border->run_mask.p, pix, channels)) return 1;
    const int x = info->box_xywh[0], y = info->box_xywh[1], w = info->box_xywh[2], h = info->box_xywh[3];
    const size_t cpix = (size_t)w * h;
    // A failed stage: wait for whatever it had queued (its kernels read border->run_page and the handle's run_a / run_b, which the next
    // call overwrites / may reallocate), then decide what the failure is.  Only a crop that cannot hold one model input -- what makes the
    // reference's own loop raise inside its bare try / except (main.py:278-281 under 2069-2091 / 2152-2157) -- degrades to "no regions" /
    // "no lines"; a device or allocation error fails the call with its message in sbbseg_last_error(): a fault must not look like an empty page.
    // layout stage + its post-processing: the reference's bare try / except (main.py:2069-2091)
    int present = 0;
    bool ok = false;
    do {
        if (ensure(layout, layout->run_a, cpix + 4) || ensure(layout, layout->run_b, cpix + 4)) break;
        int* d_thr = (int*)(layout->d_hist + 256);
        if (sbbseg_segment_crop_dev(layout, border->run_page.p, Hp, Wp, Hs, Ws, x, y, w, h, 1, layout->run_a.p, d_thr)) break;
        if (sbbseg_morph_dev(layout, layout->run_a.p, h, w, SBBSEG_MORPH_ERODE, 5, 3, layout->run_b.p)) break;          // main.py:2074
        if (sbbseg_morph_dev(layout, layout->run_b.p, h, w, SBBSEG_MORPH_DILATE, 5, 4, layout->run_b.p)) break;         // main.py:2075
        if (sbbseg_text_regions_present_dev(layout, layout->run_b.p, h, w, 1, 0.00001, &present)) break;                 // main.py:2083, 2096
        if (sbbseg_download(layout, &info->otsu_threshold, d_thr, sizeof(int))) break;
        if (sbbseg_download_labels(layout, regions_out, layout->run_b.p, cpix, channels)) break;
        info->regions_ok = 1;
        ok = true;
    } while (0);
    if (!ok && drain_after_failure(layout) && g_err_kind != kErrGeometry) return 1;
    info->text_present = info->regions_ok ? present : 0;
    if (info->text_present) {                                  // main.py:2096-2107; a failure = the outer except (2152-2157): no lines
        ok = false;
        do {
            if (ensure(textline, textline->run_a, cpix + 4)) break;
            if (sbbseg_segment_crop_dev(textline, border->run_page.p, Hp, Wp, Hs, Ws, x, y, w, h, 0, textline->run_a.p, nullptr)) break;
            if (sbbseg_download_labels(textline, textlines_out, textline->run_a.p, cpix, 1)) break;
            info->textlines_ok = 1;
            ok = true;
        } while (0);
        if (!ok && drain_after_failure(textline) && g_err_kind != kErrGeometry) return 1;
    }
    return 0;
    API_END
}

// ---- sbbseg_run_page for many pages: the stored pages go up once, the border forwards run at batch width, the layout and textline models
// take all pages' crops in one sbbseg_segment_views_dev call each; masks, region maps and textline maps stay on the device between their
// model and their glue.  What run() swallows for a page -- a crop that cannot hold a model input -- is decided by geometry before the
// pooled call; any failure of a library call is a device or allocation error and fails the whole call.
static int run_pages_impl(sbbseg_ctx* border, sbbseg_ctx* layout, sbbseg_ctx* textline, int n_pages, sbbseg_run_page_io* pages, int channels,
                          std::vector<size_t>& crop_at)
{
    std::vector<size_t> page_at(n_pages), mask_at(n_pages);
    crop_at.assign(n_pages, 0);
    size_t page_bytes = 0, mask_bytes = 0, crop_bytes = 0;
    for (int k = 0; k < n_pages; ++k) {
        sbbseg_run_page_io& pg = pages[k];
        REQUIRE(pg.page_hwc && pg.regions_out && pg.textlines_out && pg.Hp > 0 && pg.Wp > 0 && pg.Hs > 0 && pg.Ws > 0, "page %d: bad arguments", k);
        memset(&pg.info, 0, sizeof(pg.info));
        pg.status = 0;
        page_at[k] = page_bytes; page_bytes += ((size_t)pg.Hp * pg.Wp * 3 + 15) & ~(size_t)15;
        mask_at[k] = mask_bytes; mask_bytes += ((size_t)pg.Hs * pg.Ws + 15) & ~(size_t)15;
    }
    if (ensure(border, border->run_page, page_bytes)) return 1;
    if (ensure(border, border->run_mask, mask_bytes)) return 1;
    // (a failed step: drain_after_failure -- the uploads read the caller's pages, kernels read buffers the next call may reallocate)
    std::vector<sbbseg_whole_view> wv(n_pages);
    std::vector<int32_t> boxes(4 * (size_t)n_pages);
    std::vector<int64_t> px(n_pages);
    for (int k = 0; k < n_pages; ++k) {
        const sbbseg_run_page_io& pg = pages[k];
        if (hipMemcpyAsync(border->run_page.p + page_at[k], pg.page_hwc, (size_t)pg.Hp * pg.Wp * 3, hipMemcpyHostToDevice, border->stream) != hipSuccess) {
            set_error("upload of page %d failed", k);
            return drain_after_failure(border);
        }
        wv[k] = {border->run_page.p + page_at[k], pg.Hp, pg.Wp, pg.Hs, pg.Ws, pg.Hs, pg.Ws, border->run_mask.p + mask_at[k]};
    }
    if (sbbseg_extract_page_boxes_dev(border, n_pages, wv.data(), boxes.data(), px.data())) return drain_after_failure(border);
    HIPCHK(hipStreamSynchronize(border->stream));              // the hand-over: the other two handles read the pages from here on
    for (int k = 0; k < n_pages; ++k) {
        sbbseg_run_page_io& pg = pages[k];
        memcpy(pg.info.box_xywh, &boxes[4 * (size_t)k], sizeof(pg.info.box_xywh));
        pg.info.box_pixels = px[k];
        if (px[k] <= 0) { pg.status = 1; continue; }            // main.py:399-401 raises for this page: nothing else of it is written
        if (pg.page_mask_out && sbbseg_download_labels(border, pg.page_mask_out, border->run_mask.p + mask_at[k], (size_t)pg.Hs * pg.Ws, channels)) return drain_after_failure(border);
        crop_at[k] = crop_bytes;
        crop_bytes += ((size_t)pg.info.box_xywh[2] * pg.info.box_xywh[3] + 4 + 15) & ~(size_t)15;
    }
    auto fits = [](const sbbseg_ctx* h, const sbbseg_run_page_io& pg) { return pg.info.box_xywh[3] >= h->in_H && pg.info.box_xywh[2] >= h->in_W; };
    auto crop_view = [&](const sbbseg_run_page_io& pg, int k, int binarise) -> sbbseg_view {
        const int32_t* b = pg.info.box_xywh;
        return {border->run_page.p + page_at[k], pg.Hp, pg.Wp, pg.Hs, pg.Ws, b[0], b[1], b[2], b[3], binarise, layout->run_a.p + crop_at[k], nullptr};
    };
    // layout stage (main.py:2069-2091): every page that has a box and whose crop holds one input of the layout model
    std::vector<int> todo;
    std::vector<sbbseg_view> lv;
    for (int k = 0; k < n_pages; ++k)
        if (pages[k].status == 0 && fits(layout, pages[k])) todo.push_back(k);
    if (todo.empty()) return 0;
    if (ensure(layout, layout->run_a, crop_bytes) || ensure(layout, layout->run_b, crop_bytes)) return 1;
    for (int k : todo) lv.push_back(crop_view(pages[k], k, 1));
    if (sbbseg_segment_views_dev(layout, (int)lv.size(), lv.data())) return drain_after_failure(layout);
    std::vector<int> thr(lv.size(), 0);
    if (sbbseg_download(layout, thr.data(), layout->d_views_thr, sizeof(int) * lv.size())) return drain_after_failure(layout);
    for (size_t q = 0; q < todo.size(); ++q) {
        const int k = todo[q];
        sbbseg_run_page_io& pg = pages[k];
        const int w = pg.info.box_xywh[2], h = pg.info.box_xywh[3];
        uint8_t* raw = layout->run_a.p + crop_at[k];
        uint8_t* clean = layout->run_b.p + crop_at[k];
        int present = 0;
        if (sbbseg_morph_dev(layout, raw, h, w, SBBSEG_MORPH_ERODE, 5, 3, clean) ||                                         // main.py:2074
            sbbseg_morph_dev(layout, clean, h, w, SBBSEG_MORPH_DILATE, 5, 4, clean) ||                                      // main.py:2075
            sbbseg_text_regions_present_dev(layout, clean, h, w, 1, 0.00001, &present) ||                                   // main.py:2083, 2096
            sbbseg_download_labels(layout, pg.regions_out, clean, (size_t)w * h, channels)) return drain_after_failure(layout);
        pg.info.otsu_threshold = thr[q];
        pg.info.regions_ok = 1;
        pg.info.text_present = present;
    }
    // textline stage (main.py:2096-2107), on the pages the gate let through.  Its planes take the place of the raw layout maps: every
    // download above has waited for the layout handle's stream, nothing reads them any more.
    todo.clear(); lv.clear();
    for (int k = 0; k < n_pages; ++k)
        if (pages[k].info.text_present && fits(textline, pages[k])) todo.push_back(k);
    if (todo.empty()) return 0;
    for (int k : todo) lv.push_back(crop_view(pages[k], k, 0));
    if (sbbseg_segment_views_dev(textline, (int)lv.size(), lv.data())) return drain_after_failure(textline);
    for (int k : todo) {
        sbbseg_run_page_io& pg = pages[k];
        if (sbbseg_download_labels(textline, pg.textlines_out, layout->run_a.p + crop_at[k], (size_t)pg.info.box_xywh[2] * pg.info.box_xywh[3], 1)) return drain_after_failure(textline);
        pg.info.textlines_ok = 1;
    }
    return 0;
}

// STREAMS: when the call returns 0 the streams of all three handles have been synchronised behind everything it queued -- the border
// handle's at the hand-over, the other two by the download of every plane they wrote (the textline planes lie in the LAYOUT handle's buffer
// but are written on the textline handle's stream: their downloads wait for that stream).  So any handle may read the resident planes
// (sbbseg_run_pages_planes) without a further synchronisation.
int sbbseg_run_pages(sbbseg_ctx* border, sbbseg_ctx* layout, sbbseg_ctx* textline, int n_pages, sbbseg_run_page_io* pages, int channels)
{
    API_BEGIN
    if (check_ready(border) || check_ready(layout) || check_ready(textline)) return 1;
    border->run_planes_valid = layout->run_planes_valid = textline->run_planes_valid = false;
    REQUIRE(n_pages >= 1 && pages && (channels == 1 || channels == 3), "bad arguments");
    REQUIRE(border->device == layout->device && border->device == textline->device, "the three handles must live on one device");
    alloc_check();
    std::vector<size_t> crop_at;
    if (run_pages_impl(border, layout, textline, n_pages, pages, channels, crop_at)) return 1;
    layout->run_planes.resize((size_t)n_pages);
    for (int k = 0; k < n_pages; ++k) {
        const sbbseg_run_info& i = pages[k].info;
        layout->run_planes[k] = {crop_at[k], i.box_xywh[2], i.box_xywh[3], pages[k].status == 0 && i.regions_ok, pages[k].status == 0 && i.textlines_ok};
    }
    layout->run_planes_valid = true;
    return 0;
    API_END
}

int sbbseg_run_pages_planes(sbbseg_ctx* layout, int n_pages, sbbseg_plane* regions, sbbseg_plane* textlines)
{
    API_BEGIN
    if (check_ready(layout)) return 1;
    REQUIRE(regions && textlines && n_pages >= 1, "bad arguments");
    REQUIRE(layout->run_planes_valid, "no resident planes: the last sbbseg_run_pages on this layout handle failed, was overwritten by a later sbbseg_run_page, or never ran");
    REQUIRE((size_t)n_pages == layout->run_planes.size(), "%d pages asked for, the last sbbseg_run_pages ran %d", n_pages, (int)layout->run_planes.size());
    for (int k = 0; k < n_pages; ++k) {
        const sbbseg_ctx::RunPlanes& rp = layout->run_planes[k];
        regions[k] = {rp.regions_ok ? layout->run_b.p + rp.at : nullptr, rp.h, rp.w};
        textlines[k] = {rp.textlines_ok ? layout->run_a.p + rp.at : nullptr, rp.h, rp.w};
    }
    return 0;
    API_END
}

}  // extern "C"
