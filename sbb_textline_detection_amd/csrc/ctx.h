// ctx.h -- private, host only: what the translation units behind the C ABI (api.hip, forward.hip, pages.hip, whole.hip, comm.hip -- these five
// through exec.h, forward.hip and pages.hip through route.h too -- plan_build.hip, stage_glue.hip, contour_glue.hip, order_glue.hip, line_extent_glue.hip) share: the error and exception plumbing, the allocation helpers, and the handle
// (struct sbbseg_ctx) with the plan structs it embeds.  Device and pinned memory belong to the handle's two registries (devmem.h: `mem`, `pinned`);
// every device pointer below, in the handle and in the plan structs, points at a block one of them owns and sbbseg_destroy frees with the registry.
#pragma once

#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sbbseg.h"
#include "devmem.h"
#include "internal.h"
#include "region.h"

#define HIPCHK(expr)                                                                                                 \
    do {                                                                                                             \
        hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess)                                                                                        \
            return sbbseg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);     \
    } while (0)

#define REQUIRE(cond, ...) do { if (!(cond)) return sbbseg::set_error(__VA_ARGS__); } while (0)
// ... for the one failure the reference's run() swallows: a page or crop that cannot hold one model input (main.py:278-285 under the bare
// try / except of 2069-2091 and 2152-2157).  Callers that mirror run() branch on g_err_kind, not on the message's wording.
#define REQUIRE_GEOMETRY(cond, ...) do { if (!(cond)) { sbbseg::set_error(__VA_ARGS__); sbbseg::g_err_kind = sbbseg::kErrGeometry; return 1; } } while (0)

// Every extern "C" body runs inside API_BEGIN / API_END: a C++ exception (std::bad_alloc from a std::vector, ...)
// becomes a non-zero status + sbbseg_last_error() instead of terminating the caller's process -- the reference's
// callers rely on ordinary Python exceptions (main.py:2061-2157).
#define API_BEGIN try {
#define API_END                                                                                               \
    }                                                                                                         \
    catch (const std::bad_alloc&) { return sbbseg::set_error("out of host memory (std::bad_alloc)"); }        \
    catch (const std::exception& e_) { return sbbseg::set_error("internal error: %s", e_.what()); }           \
    catch (...) { return sbbseg::set_error("unknown internal error"); }

namespace sbbseg {

// Defined once in the library (api.hip): sbbseg_last_error() and sbbseg_debug_inject_alloc_failure() serve every unit.
extern thread_local std::string g_err;          // written by set_error() (internal.h)
enum ErrKind { kErrOther = 0, kErrGeometry = 1 };
extern thread_local int g_err_kind;             // kind of the error in g_err: set_error() says kErrOther, REQUIRE_GEOMETRY kErrGeometry
extern int g_alloc_fail_countdown;              // test hook (sbbseg_debug_inject_alloc_failure): the n-th next alloc_check() throws std::bad_alloc
inline void alloc_check() { if (g_alloc_fail_countdown > 0 && --g_alloc_fail_countdown == 0) throw std::bad_alloc(); }

int dmalloc(sbbseg_ctx* c, void** p, size_t bytes);                    // a block of c->mem
int check_ready(sbbseg_ctx* c);                                        // a finalized handle; makes its device current

template <typename T>
int ensure(sbbseg_ctx* c, DevBuf<T>& b, size_t bytes);                 // grows b to `bytes` in c->mem (defined below the handle)

template <typename T>
int upload(sbbseg_ctx* c, T** dptr, const T* host, size_t n)
{
    if (dmalloc(c, (void**)dptr, n * sizeof(T))) return 1;
    HIPCHK(hipMemcpy(*dptr, host, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
template <typename T>
int upload(sbbseg_ctx* c, T** dptr, const std::vector<T>& host) { return upload(c, dptr, host.data(), host.size()); }

struct Tensor {
    int H = 0, W = 0, C = 0;
    size_t elems_per_patch = 0;
    char* buf = nullptr;          // zero header + data (of the lane in use)
    char* lane_buf[2] = {nullptr, nullptr};
    bool is_input_form = false;
    int form = -1, pad = 0;
    char* data() const { return buf + kZeroHeaderBytes; }
};

enum OpType { kConv = 0, kPool = 1, kHead = 2, kTail = 3, kBlock = 4 };

struct ConvOp {
    sbbseg_conv_desc d;
    int Ho = 0, Wo = 0, TH = 0, TW = 0;
    int cout_pad = 0, Ktot = 0, total_ksteps = 0, ksteps[2] = {0, 0};
    KTabEntry* d_ktab = nullptr;
    KStepRec* d_kstep = nullptr;
    void* d_w = nullptr;
    float *d_scale = nullptr, *d_shift = nullptr, *d_rscale = nullptr, *d_rshift = nullptr;
    float *d_head_w = nullptr, *d_head_scale = nullptr, *d_head_shift = nullptr;
    // further placement classes merged into this op (parity siblings); class 0 = the fields above
    int n_cls = 1;
    void* d_w_cls[4] = {nullptr, nullptr, nullptr, nullptr};
    KStepRec* d_kstep_cls[4] = {nullptr, nullptr, nullptr, nullptr};
    KTabEntry* d_ktab_cls[4] = {nullptr, nullptr, nullptr, nullptr};
    int ooy_cls[4] = {0, 0, 0, 0}, oox_cls[4] = {0, 0, 0, 0};
    float wmul_cls[4] = {1.f, 1.f, 1.f, 1.f};   // split mode: 2^-s of the class's power-of-two weight pre-scale
    std::vector<float> h_epi;             // host copy of scale | shift | head_w | head_scale | head_shift: parity siblings are
                                          // only merged into one launch when these are identical (they share class 0's)
    uint16_t* d_stem_wfrag = nullptr;     // non-null: the op is the network stem and runs stem_conv_pairs
    int fused_pool = -1;                  // split mode: index of the max-pool op this stem also computes (sbbseg_finalize), or -1
    uint16_t* d_halo_wfrag = nullptr;     // split mode, the 224 x 224 decoder conv: the four classes' weights as MFMA A fragments (dec_halo_x3.hip)
    int* d_halo_taps = nullptr;           //   ... and their taps in K-step order (sbbseg_finalize)
    uint16_t* d_d64_wfrag = nullptr;      // non-null: 3x3 s1 64->64 conv, runs conv3x3_c64_direct
    int fused_reduce = -1;                // split mode: index of the NEXT block's first 1x1 conv, computed by this (expand) conv's launch too
                                          // (expand_reduce_x3.hip; sbbseg_finalize), or -1
    uint16_t *d_er_w3 = nullptr, *d_er_w1 = nullptr;      //   ... the two convs' packed rows as MFMA A fragments
    int fused_conv3 = -1;                 // on an expand conv with fused_reduce: index of the block's 3x3 conv, which the same launch computes too
                                          // (conv3_expand_reduce.hip; sbbseg_finalize), or -1
    uint16_t* d_c3_w2 = nullptr;          //   ... the 3x3 conv's packed rows as MFMA A fragments, and its K-steps (taps / channel groups) in order
    int* d_c3_k0 = nullptr;
                                          // (that conv's output tensor then lives in LDS only)
    std::vector<float> h_w[2];            // host copy of a small 1x1 conv's weights ([cin][cout] per source): bottleneck fusion
                                          // (sbbseg_finalize) repacks them as MFMA A fragments
    bool fg_ok = true;                    // every K-step (of every class) regular: the fast gather of conv_igemm_mfma applies
                                          // (ConvParams::fast_gather) if each source's taps also span at most 4 x 4 offsets
    int tap_lo[2][2] = {{127, 127}, {127, 127}}, tap_hi[2][2] = {{-127, -127}, {-127, -127}};   // [source][y|x] over all classes
    std::vector<KStepRec> h_ksteps_cls[4];   // host copies: sbbseg_finalize builds the fast gather's tables from them
    FgStepRec* d_fgstep_cls[4] = {nullptr, nullptr, nullptr, nullptr};
    bool fg_pointwise = false;            // all taps (0, 0) in bounds: ConvParams::fast_gather = 2 (no masks)
};

struct PoolOp {
    int src, dst, k, stride, Ho, Wo; float *d_pre_scale = nullptr, *d_pre_shift = nullptr; int pre_relu = 0;
};

struct HeadOp {
    int src, cin, classes;
    float *d_w = nullptr, *d_scale = nullptr, *d_shift = nullptr;
};

struct TailOp {
    int src0 = -1, img = -1, classes = 0;
    void* d_wfrag = nullptr;
    float *d_scale = nullptr, *d_shift = nullptr, *d_head_w = nullptr, *d_head_scale = nullptr, *d_head_shift = nullptr;
};

// a fused ResNet bottleneck block (bottleneck_fused): the three convs it replaces stay alive as `parts` of the op
// (they own the scale / shift arrays and the 3x3 fragments the fused kernel reads, and they are what runs when the
// fusion is switched off at run time, conv variant bit 18)
struct BlockOp {
    int x_tensor = -1, out_tensor = -1, cin = 0, proj = 0, H = 0, W = 0;
    uint16_t *d_w1 = nullptr, *d_w3 = nullptr;
    float wmul[3] = {1.f, 1.f, 1.f};      // split mode: 2^-s of the three convs' weight pre-scales
};

struct Op {
    OpType type;
    std::string name;
    double flops = 0, min_bytes = 0;
    double issued_flops = 0;      // MFMA work the kernel really issues per patch (K padding, pre-summed taps, 3x in split mode)
    ConvOp conv;
    PoolOp pool;
    HeadOp head;
    TailOp tail;
    BlockOp block;
    std::vector<Op> parts;        // kBlock: the convs it fuses
    double prof_ms = 0;
    int64_t prof_launches = 0, prof_patches = 0;
    int absorbed_by = -1;         // >= 0: index of the op whose launch can write this op's output too -- the stem of a max-pool (fused_pool), the
                                  // expand conv of a reduce conv (fused_reduce) or of a 3x3 conv (fused_conv3); sbbseg_finalize.  The op launches
                                  // nothing when that op takes the fused route (route.h)
    int region_level = -1;        // >= 0: a decoder level of the owned-region chain (sbbseg_finalize: region_chain; region.h)
    double exec_patches = 0;      // work executed since sbbseg_profile_reset, in whole-patch equivalents: a launch of n patches adds n, an
                                  // owned-region launch n x (pixels walked / pixels of the whole grid)
    double prof_exec_patches = 0; // the same, over the launches the profiling events timed (prof_ms)
    LaunchRec last;               // what the op's last launch used (sbbseg_debug_op_launch): written by launch_op and the launcher it calls
};

constexpr int kMinLaneTiles = 8;      // a lane gets at least this many tiles, else the chunk runs whole on lane 0

struct PendingEvent { int op; hipEvent_t a, b; int patches; double exec; };

// owned-region launches (region.h): tables of the chunk a lane is running
struct RegionRun {
    bool on = false;
    int kind[kRegionMaxLevels] = {0};            // 0 = tile table, 1 = pixel map (what the level's kernel takes: dec_halo_* / tail vs conv_igemm_mfma)
    int total[kRegionMaxLevels] = {0};           // entries (per class)
    double frac[kRegionMaxLevels] = {0};         // pixels walked / pixels of the whole grid, over the chunk
    uint32_t* tab[kRegionMaxLevels] = {nullptr};
};

}  // namespace sbbseg

struct sbbseg_ctx {
    int device = 0;
    int precision = sbbseg::kBF16;
    int elem = 2;                 // bytes per stored half-element (weights, one activation plane)
    int planes = 1;               // 16-bit planes per activation element: 2 in the split mode (hi, lo), else 1
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // second lane: its own activation buffers and stream; a chunk of tiles is split over the two lanes so
    // that one half's launch tails (few tiles left, most CUs idle) are filled by the other half's kernels
    hipStream_t lane_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int lanes = 2, lane1_batch = 0;
    int lane_prio = 0, prio_least = 0, prio_greatest = 0;      // priority class of lane_stream (never the own stream's class: see sbbseg_create)
    int in_H = 0, in_W = 0, in_C = 0;
    std::vector<sbbseg::Tensor> tensors;
    std::vector<sbbseg::Op> ops;
    int form_tensor[2] = {-1, -1};
    int classes = 0, max_batch = 0;
    bool finalized = false;
    // who owns the handle's memory (devmem.h).  A new buffer: declare a DevBuf here and call ensure() where it is used -- nothing else.
    // sbbseg_create gives the registries their allocators (api.hip); a handle built without them (the host-only tests) can allocate nothing
    sbbseg::DeviceMem mem;                        // device memory; sbbseg_device_bytes is its total
    sbbseg::DeviceMem pinned;                     // pinned host staging
    typedef sbbseg::DeviceMem::AllocFn AllocFn;
    typedef sbbseg::DeviceMem::FreeFn FreeFn;
    explicit sbbseg_ctx(AllocFn dev_alloc = nullptr, FreeFn dev_free = nullptr, AllocFn pin_alloc = nullptr, FreeFn pin_free = nullptr)
        : mem(dev_alloc, dev_free), pinned(pin_alloc, pin_free) {}
    // run-time buffers
    float* d_lut = nullptr;
    unsigned* d_hist = nullptr;   // [256] channel-0 histogram + [1] Otsu threshold (int) behind it
    int* d_tile_xy = nullptr;          // [max_batch][2]
    uint8_t* d_batch_labels = nullptr; // [max_batch][H][W] (predict / whole-image path)
    float* d_probs = nullptr;          // [max_batch][H][W][classes], lazily allocated
    float* d_xin = nullptr;            // predict(): staged float input, lazily allocated
    sbbseg::DevBuf<float> ks_ws;                         // split-K partial sums (whole-image branch)
    bool ksplit = true, ksplit_now = false;              // SBBSEG_KSPLIT=0 switches it off; _now: inside the whole-image branch's run_plan
    sbbseg::DevBuf<uint8_t> page, page_labels;
    sbbseg::DevBuf<uint8_t> page_labels3;                             // 3-channel copy for label_channels == 3
    int label_channels = 1;
    sbbseg::DevBuf<uint8_t> tile_labels;
    sbbseg::DevBuf<int> own_x, own_y;
    int own_Hp = -1, own_Wp = -1, own_nyf = 0;
    bool own_dedupe = false;          // the cached owner tables index the deduplicated grid (see fused_grid)
    // Duplicate clamped tiles: when extent % mid lies in (0, tile - mid] the inward clamp (main.py:276-281) gives the LAST
    // TWO tiles of an axis the same origin -- the reference runs the same forward twice and pastes the same labels twice.  The fused
    // page paths skip the repeat (same label map, 1 / n of the forwards of that axis saved); the tile-indexed entry points
    // (sbbseg_tile_grid, _segment_tile_range_dev, _stitch_dev: the multi-rank protocol) keep the reference's call list.
    bool dedupe = true;               // sbbseg_set_dedupe / SBBSEG_DEDUPE=0
    int64_t forwards = 0;             // patches run through the plan so far (sbbseg_debug_counter 1)
    sbbseg::DevBuf<int> map;
    sbbseg::DevBuf<int> wmap;                        // gather tables of the whole-image branch, cached per geometry
    int wmap_key[6] = {0, 0, 0, 0, 0, 0};            // {Hp, Wp, Hs, Ws, out_h, out_w} (0 = none)
    int map_key[4] = {0, 0, 0, 0};     // {Hs, Ws, Hp, Wp} the nearest maps in `map` were built for (sbbseg_segment_crop_dev; 0 = none)
    // sbbseg_segment_views_dev: the call's view table | fallback threshold ints | nearest maps, staged in pinned memory and uploaded in one
    // asynchronous copy; ev_views marks that copy done (the staging may then be rewritten by the next call)
    sbbseg::DevBuf<void> views;
    sbbseg::DevBuf<void> h_views;                                     // (pinned)
    hipEvent_t ev_views = nullptr; bool views_copy_pending = false;
    int* d_views_thr = nullptr;       // the last call's threshold ints inside `views`, one per view (sbbseg_segment_views reads them back)
    int64_t views_launches = 0;       // ingest + region-build + stitch kernels sbbseg_segment_views_dev has queued (sbbseg_debug_counter 3)
    int64_t whole_launches = 0;       // ingest + label-resize kernels the whole-views calls have queued (sbbseg_debug_counter 4)
    // stage glue scratch (morphology planes, union-find arrays, result words)
    sbbseg::DevBuf<uint8_t> morph_a, morph_b;
    // pipelined multi-page host path (sbbseg_segment_pages): copy streams, two slots of pinned staging + device buffers
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    hipEvent_t pp_in[2] = {nullptr, nullptr}, pp_comp[2] = {nullptr, nullptr}, pp_out[2] = {nullptr, nullptr};
    sbbseg::DevBuf<uint8_t> pp_h_in[2], pp_h_out[2];              // pinned host staging
    sbbseg::DevBuf<uint8_t> pp_d_in[2], pp_d_out[2], pp_d_out3[2];      // device buffers
    bool pp_ready = false;                                        // streams + events of the page pipeline exist
    // RCCL communicator of the sharded path (sbbseg_comm_init; librccl is dlopen'ed on first use)
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    sbbseg::DevBuf<void> deskew;                          // inverse maps | bicubic table | row counts of sbbseg_deskew_profiles
    // sbbseg_run_page's / sbbseg_run_pages' resident buffers (owned by the handle passed as `border` / `layout` / `textline` respectively;
    // sbbseg_run_pages: all pages' planes one after the other, and the textline planes in the layout handle's run_a)
    sbbseg::DevBuf<uint8_t> run_page, run_mask, run_a, run_b;
    // what the last sbbseg_run_pages left resident in this (layout) handle's run_b / run_a, page by page (sbbseg_run_pages_planes); no
    // device memory of its own.  Emptied by a failed call and by the next sbbseg_run_page(s) that names the handle.
    struct RunPlanes { size_t at; int w, h, regions_ok, textlines_ok; };
    std::vector<RunPlanes> run_planes;
    bool run_planes_valid = false;
    sbbseg::DevBuf<int> cc_parent, cc_count;
    bool force_host_contours = false;     // test hook (conv variant bit 21): always take the exact host ranking
    int host_contour_calls = 0;           // how often the exact host ranking ran (sbbseg_debug_counter)
    int* d_cc_list = nullptr;             // [6 + kCcMaxRivals]: launch_largest_contour's result record
    sbbseg::DevBuf<int> cc_aux;                          // five int planes: doubled cell area + bounding boxes per root (sbbseg_page_box_dev)
    unsigned long long* d_cc_small = nullptr;      // [0] best key, [1..2] box (4 ints)
    sbbseg::DevBuf<int> cc_bg;                           // two int planes: labels of the complement, border flags (sbbseg_text_region_boxes_dev)
    sbbseg::DevBuf<int> cc_roots;                        // parentless roots (or all roots), 6 ints each: sbbseg::ContourCand
    // sbbseg_text_region_contours_dev / sbbseg_debug_mask_contours_dev: the last call's result stays here until the next one
    // (sbbseg_text_region_contours_read; the next device steps read it in place)
    sbbseg::DevBuf<void> contour_tab;                    // candidates | records | slots | boxes | doubled areas | point offsets | totals
    sbbseg::DevBuf<int32_t> contour_pts;                 // [points][2] x, y, packed in contour order
    int contour_n = -1;                                  // contours of the resident result (-1: none)
    long long contour_np = 0;                            // ... and its points
    size_t contour_boxes_at = 0, contour_area2_at = 0, contour_off_at = 0;      // byte offsets of the result tables inside contour_tab
    int contour_lds_limit = 64 * 1024;                   // kContourLdsBytes, or less (sbbseg_debug_set_contour_lds_limit)
    long long contour_launches = 0;                      // tracer and packing kernels queued so far (sbbseg_debug_contour_launches)
    sbbseg::DevBuf<void> rdk;                            // sbbseg_region_deskew_profiles_dev: maps | table | geometry | crops | counts
    sbbseg::DevBuf<void> pstat;                          // sbbseg_profile_statistics_dev: weights | regions | spread | winner | state | workspace
    long long line_launches = 0;                         // kernels queued by sbbseg_region_line_masks_dev (sbbseg_debug_counter 2)
    long long slope_launches = 0;                        // kernels queued by the slope sweeps: crop, profile, statistic, winner (sbbseg_debug_counter 5)
    sbbseg::DevBuf<void> lsplit;                         // sbbseg_line_split_dev: regions | info | lines | corners | rotated corners | workspace
    sbbseg::DevBuf<void> line_w;                         // ... its table of half Gaussian kernels: offsets | weights, uploaded when it differs from
    std::vector<double> line_w_host;                     // ... this copy of the last one
    int16_t* d_line_tab = nullptr;                       // sbbseg_region_line_masks_dev: the fixed-point bicubic table, built on first use
    // sbbseg_region_order_dev / sbbseg_contour_moments_dev (order_glue.hip): point offsets | edges | ranks | bands | flags | centroids | moments |
    // row sums | smoothed profile | weights, and the points of a contour list the caller passed in
    sbbseg::DevBuf<void> order_buf;
    sbbseg::DevBuf<int32_t> order_pts;
    long long order_launches = 0;                        // kernels queued by the two calls above (sbbseg_debug_order_launches)
    // sbbseg_region_line_extents_dev / sbbseg_debug_mask_border_winner_dev (line_extent_glue.hip); the last call's bit maps, records and
    // winners stay here until the next one (sbbseg_region_line_extents_read)
    sbbseg::DevBuf<void> extent_tab;                     // regions | point offsets | records | line tables
    sbbseg::DevBuf<uint32_t> extent_bits, extent_marks;  // filled + threshrot bit maps; mark planes of the scan's global form
    sbbseg::DevBuf<int32_t> extent_pts, extent_win;      // a ring list the caller passed in; the winners' points
    int64_t* d_extent_wtab = nullptr;                    // float32 bicubic products * 2^34, built on first use
    int extent_lds_limit = 60 * 1024;                    // kExtentLdsBytes, or less (sbbseg_debug_set_extent_lds_limit)
    long long extent_launches = 0;                       // kernels queued by the two calls (sbbseg_debug_extent_launches)
    std::vector<int32_t> extent_geom;                    // per region of the resident result: w, h, first word of threshrot, winner offset, points
    int extent_n = -1;                                   // regions of the resident result (-1: none)
    // profiling
    bool profiling = false;
    int conv_variant = 0;
    bool ph8 = false;            // 8-phase schedule on the 256x256 tile (opt-in, conv variant bit 16)
    int fg_min_ksteps = 9;             // convs with real taps take the fast gather from this many K-steps on (SBBSEG_FG_MIN)
    int fg_pointwise_min_ksteps = 4;   // pointwise convs take the fast gather from this many K-steps on (SBBSEG_FG_POINTWISE_MIN)
    bool ranged_walk = false;    // A/B: grouped launches walk XCD-contiguous tile ranges (conv variant bit 19)
    bool block_pq = true;        // fused bottleneck blocks run the producer / consumer form (conv variant bit 20: the one-group form)
    bool unfuse_blocks = false;  // A/B: run a fused bottleneck block as its three convs (conv variant bit 18)
    bool dump_blocks = false;    // step check: the fused 16-bit bottleneck blocks also store a and b to their plan tensors (conv variant bit 26;
                                 // nothing in the split mode, whose block_x3 is held bit-identical to its three convs)
    bool unfuse_stem_pool = false;    // A/B: stem and max-pool as two launches (conv variant bit 22)
    bool no_dec_halo = false;          // A/B: the 224 x 224 decoder conv on the generic kernel (conv variant bit 23)
    bool no_expand_reduce = false;     // A/B: expand + next reduce 1x1 convs as two launches (conv variant bit 24)
    bool no_c3er = false;              // A/B: the 3x3 conv of a stage-3 identity block as its own launch in front of expand_reduce (conv variant bit 25)
    bool plain_gather = false;   // A/B: per-load address arithmetic instead of the fast gather (conv variant bit 17)
    int contig_max_k = 0;        // short-K layers up to this K walk their tiles in per-block contiguous runs (tile map 2)
    int fused_heads = 0;
    int num_cus = 256;
    std::vector<sbbseg::PendingEvent> pending;
    std::vector<hipEvent_t> free_events;
    // owned-region launches of the decoder (region.h; sbbseg_set_owned_regions): 0 = off, 1 = the fused page paths (default), 2 = the
    // tile-range entry points of the multi-rank protocol too (their tile labels are then defined on the owned regions only)
    int owned_mode = 1;
    int region_levels = 0;                        // decoder levels of the chain found by sbbseg_finalize (0: the plan has none)
    int region_op[sbbseg::kRegionMaxLevels] = {0};        // op index per level (level 0 = the tail)
    sbbseg::DevBuf<uint32_t> rtab[2][sbbseg::kRegionMaxLevels];                 // per lane and level: the chunk's table (allocated on first use)
    sbbseg::RegionRun rr;                                 // the chunk run_plan is launching (set by tile_range_impl around run_plan)
    double last_exec_frac = 1.0;                  // share of its output grid the op being launched walks (run_plan's accounting; launch_op resets
                                                  // it to 1 when an A/B knob takes a level off its owned-region form)
};

namespace sbbseg {

// The one way a run-time buffer of the handle grows.  The handle's stream may still be using the block about to be freed: wait for it first.
template <typename T>
int ensure(sbbseg_ctx* c, DevBuf<T>& b, size_t bytes)
{
    if (b.cap >= bytes) return 0;
    if (b.p) HIPCHK(hipStreamSynchronize(c->stream));
    return ensure(c->mem, b, bytes);
}

// ---- what the stage-glue units (stage_glue.hip, contour_glue.hip, order_glue.hip, line_extent_glue.hip) share
inline size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
// (stage_glue.hip) the float bicubic table [32][4] of cv2.warpAffine, and rotate_image's inverse map for an h x w crop
void cubic_table(float* tab);
int line_inverse_map(int h, int w, double slope, double* minv6);

// The host-plane form of an entry point: the caller's H x W plane goes into c->morph_b.p and the `_dev` twin runs on *d_plane (in place
// where the twin writes there too).  needed == false -- a size query, or no boxes -- needs no handle and uploads nothing.
inline int stage_plane(sbbseg_ctx* c, const uint8_t* host_hw, int H, int W, bool needed, const void** d_plane)
{
    *d_plane = nullptr;
    REQUIRE(H > 0 && W > 0, "bad arguments");
    if (!needed) return 0;
    if (check_ready(c)) return 1;
    REQUIRE(host_hw, "bad arguments");
    if (ensure(c, c->morph_b, (size_t)H * W)) return 1;
    HIPCHK(hipMemcpyAsync(c->morph_b.p, host_hw, (size_t)H * W, hipMemcpyHostToDevice, c->stream));
    *d_plane = c->morph_b.p;
    return 0;
}

}  // namespace sbbseg
