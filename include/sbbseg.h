/* sbbseg.h -- C ABI of libsbbseg.so: MI355X (gfx950) patch-wise pixel-segmentation inference.
 *
 * This is the drop-in boundary for ONE path of qurator-spk/sbb_textline_detection:
 * `textline_detector.do_prediction()` and the `model.predict()` it calls per 448x448 patch
 * (reference: qurator/sbb_textline_detector/main.py:225-380).  The reference is Python; its
 * "FFI" for this path is the Keras model duck type.  A maintainer binds these entry points
 * with ctypes (the shipped binding is sbb_textline_detection_amd/_capi.py).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is in
 *     sbbseg_last_error() (thread-local).  Nothing aborts: the reference's callers rely on
 *     ordinary Python exceptions (main.py:2061-2157), which the Python shim raises from this.
 *   - plain pointers and sizes only; host buffers are caller-owned; the library owns only device
 *     memory behind the opaque handle.  A handle is not thread-safe; distinct handles may be used
 *     from distinct threads / processes (one process per GPU).
 *   - "*_dev" variants take device pointers (HBM-resident inputs/outputs, used by bench.py and
 *     the multi-GPU path); all work is enqueued on the handle's stream (sbbseg_set_stream).
 */
#ifndef SBBSEG_H
#define SBBSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBBSEG_ABI_VERSION 5

typedef struct sbbseg_ctx sbbseg_ctx;

/* arithmetic mode of a handle */
#define SBBSEG_PREC_BF16 0   /* bf16 operands, fp32 MFMA accumulate, fp32 epilogue.  Fast, coarse: 8-bit significands
                                through ~60 layers move near-tie labels (kept for A/B only) */
#define SBBSEG_PREC_F32  1   /* fp32 everything, plain FMA kernels: slow, used to separate plumbing
                                errors from 16-bit rounding in the parity tests */
#define SBBSEG_PREC_F16  2   /* fp16 operands (11-bit significand, saturating stores), same MFMA rate as
                                bf16, fp32 accumulate/epilogue: 8x finer rounding, range +-65504.  The FAST mode:
                                labels can differ from an fp32 run where the top-2 softmax margin is small */
#define SBBSEG_PREC_F16X3 3  /* error-compensated fp16 ("split") mode, the LABEL-EXACT mode and the default of the
                                Python seams: every activation and weight is carried as hi + lo fp16 halves (~22
                                significant bits), each product is three MFMAs (hi*hi + hi*lo + lo*hi) accumulated
                                in fp32.  Same MFMA kernels, ~1/3 of the fp16 mode's arithmetic rate; label maps
                                equal an fp32 evaluation except at exact ties (main.py:290 "argmax bit-exact") */

/* ---- lifecycle: replaces start_new_session_and_model / session.close (main.py:216-223, 428) */
const char* sbbseg_last_error(void);
int sbbseg_abi_version(void);
int sbbseg_device_count(int* count);
int sbbseg_create(int device, int precision, sbbseg_ctx** out);
int sbbseg_destroy(sbbseg_ctx* c);                       /* frees all device memory; NULL ok */
/* ONE-CALL model load: what keras.models.load_model(path, compile=False) + the first predict do in the reference
 * (main.py:216-223).  Takes the .sbbw container (magic "SBBW0001", JSON header = the Keras-2.3 model_config of the .h5 plus a
 * tensor table, little-endian fp32 weights; written offline by tools/h5_to_sbbw.py), reads the layer graph, lowers it to the fused
 * plan (BN folding, parity split of the decoder convs, shortcut merge, fused head / tail -- the planner of planner.py restated in
 * C++, same algebra in the same precision) and returns a finalized handle: no Python needed on the consumer's side.
 * flags: SBBSEG_LOAD_* switches (0 = all lowerings on).  The step-by-step plan API below stays available. */
#define SBBSEG_LOAD_NO_PARITY_SPLIT   1
#define SBBSEG_LOAD_NO_SHORTCUT_MERGE 2
#define SBBSEG_LOAD_NO_FUSED_HEAD     4
#define SBBSEG_LOAD_NO_FUSED_TAIL     8
int sbbseg_model_load(const void* sbbw_bytes, size_t n_bytes, int device, int precision, int max_batch, int flags, sbbseg_ctx** out);
int sbbseg_model_load_file(const char* sbbw_path, int device, int precision, int max_batch, int flags, sbbseg_ctx** out);
/* Test hook (no GPU needed): the plan sbbseg_model_load would build, as text -- one line per tensor / step with the CRC32 of every
 * weight plane, scale and shift vector -- so the library's planner can be compared with planner.py value for value. */
int sbbseg_debug_plan_summary(const void* sbbw_bytes, size_t n_bytes, int precision, int flags, char* out, size_t capacity, size_t* needed);
/* run on the caller's HIP stream (NULL = the legacy default stream, e.g. torch's current stream when
 * no stream context is active); SBBSEG_OWN_STREAM returns to the handle's private non-blocking stream */
#define SBBSEG_OWN_STREAM ((void*)(intptr_t)-1)
int sbbseg_set_stream(sbbseg_ctx* c, void* hip_stream);
int sbbseg_synchronize(sbbseg_ctx* c);
/* Lanes (default 2): the grid-form page entry points split every chunk of >= 16 tiles into two halves
 * that run concurrently -- the second on a private stream with its own activation buffers -- so the
 * launch tails of one half are filled by the other's kernels (measured +6-7 % on a 70-tile page).
 * All work stays ordered on the handle's stream (fork/join events); results do not depend on it.
 * Call before sbbseg_finalize to skip the second set of buffers (lanes = 1), or any time to switch. */
int sbbseg_set_lanes(sbbseg_ctx* c, int lanes);
/* Layout of the HOST label outputs of sbbseg_segment_page / _scaled / _otsu / _whole: 1 (default) = one
 * uint8 plane [H][W]; 3 = the reference's own return layout, uint8 [H][W][3] with three identical channels
 * (main.py:366, 380) -- replicated on the device, the host buffer must hold 3 x H x W bytes. */
int sbbseg_set_label_channels(sbbseg_ctx* c, int channels);
/* Duplicate clamped tiles (default on; SBBSEG_DEDUPE=0 or on = 0 switches it off): when (extent % mid) lies in (0, tile - mid]
 * -- mid = tile - 2 * margin = 360 for the 448-pixel models, so 88 of every 360 page extents -- the inward clamp of main.py:276-281
 * gives the LAST TWO tiles of that axis the same origin: the reference runs the same forward twice and pastes the same labels
 * twice (a 448 x 448 page: four identical forwards).  The fused page entry points (sbbseg_segment_page[_dev / _scaled / _otsu],
 * _segment_pages[_dev], _segment_crop[_dev]) compute each distinct tile once; the label map is the same byte for byte.  The
 * tile-indexed entry points (sbbseg_tile_grid, _segment_tiles_dev, _segment_tile_range[_bin]_dev, _stitch_dev -- the multi-rank
 * protocol) always keep the reference's call list. */
int sbbseg_set_dedupe(sbbseg_ctx* c, int on);
/* Split-K in the whole-image branch (sbbseg_segment_whole[_scaled], sbbseg_extract_page_box[_dev]; every mode but fp32; default on, SBBSEG_KSPLIT=0 or
 * on = 0 switches it off): one patch through a long-K conv occupies 2-32 CUs for 100-400 K-steps, so the K range of such a launch is
 * split over up to 16 blocks per tile and the fp32 partial sums are added in split order by a second launch -- 3.4 -> 1.9 ms per
 * whole-image forward of the 448 model in the split mode, 2.1 -> 1.5 ms in plain fp16.  Deterministic, but the last bits differ from the unsplit launches (summation order): the
 * patch paths and sbbseg_predict never split, their results do not depend on the batch size. */
int sbbseg_set_ksplit(sbbseg_ctx* c, int on);
/* Owned-region launches of the decoder (round 6; default mode 1, SBBSEG_OWNED_REGIONS=0|1|2 overrides the default at creation).
 * do_prediction pastes only part of every tile's label map into the page: the 10 % margin is cropped on every side that is not a page
 * edge (main.py:294-364) and where the inward-clamped last tile of an axis overlaps its neighbour the later tile wins (main.py:276-281
 * + the paste order) -- a 3500 x 2500 page keeps 8.75 of the 14.05 Mpx its 70 tiles produce.  The decoder is local (3x3 convs over
 * nearest-x2 upsamplings, pointwise epilogues), so each decoder level is launched only over the rows / columns the kept pixels depend
 * on: the owned rectangle dilated by one pixel per 3x3 conv above the level and halved per upsampling.  The encoder (receptive field
 * = the tile) runs whole.  Every computed pixel goes through the arithmetic of the full launch: the stitched label map is the same
 * byte for byte.
 *   mode 0: off.  mode 1: the fused page entry points (sbbseg_segment_page[_dev / _scaled / _otsu], _segment_pages[_dev],
 *   _segment_crop[_dev], sbbseg_run_page).  mode 2: also sbbseg_segment_tile_range[_bin]_dev -- the tile labels they return are then
 *   DEFINED ONLY ON EACH TILE'S OWNED REGION (everything sbbseg_stitch_dev reads); a repeated clamped tile owns nothing.
 * sbbseg_predict, sbbseg_segment_tiles_dev and the whole-image branch always compute whole patches. */
int sbbseg_set_owned_regions(sbbseg_ctx* c, int mode);
/* the mode in force, and the decoder levels (the fused tail + the parity-split decoder convs below it) the handle's plan runs as
 * owned-region launches; 0 levels = none (fp32 handles, unfused heads, decoders of another shape: everything is computed whole) */
int sbbseg_owned_region_info(sbbseg_ctx* c, int* mode, int* levels);

/* ---- plan building: the host-side planner (planner.py) lowers the Keras model_config that the
 * reference would have handed to keras.models.load_model (main.py:221) into these calls, in
 * execution order.  Tensors are per-patch NHWC activations; the batch dimension is runtime. */

/* Forms of the network input the kernels consume (both are filled by the ingest kernels):
 *   SBBSEG_INPUT_C8     [H][W][8]            pixel (y,x) channel c at [y][x][c], channels 3..7 zero
 *   SBBSEG_INPUT_PAIRS  [H+2p][ceil((W+2p)/2)][8]  zero-padded by p on every side, two horizontal
 *                       neighbours x 4 channels per 16-byte granule: [y+p][(x+p)>>1][((x+p)&1)*4+c]
 *                       (lets the 7x7 stride-2 stem run as a 7x4 stride-(2,1) conv over 8 channels) */
#define SBBSEG_INPUT_C8    0
#define SBBSEG_INPUT_PAIRS 1
int sbbseg_set_input(sbbseg_ctx* c, int H, int W, int channels);
int sbbseg_input_form(sbbseg_ctx* c, int form, int pad, int* tensor_id);
int sbbseg_add_tensor(sbbseg_ctx* c, int H, int W, int C, int* tensor_id);

typedef struct {
    int32_t tensor;      /* source tensor id */
    int32_t channels;    /* channels taken from it (from channel 0), contraction order */
    int32_t kh, kw;      /* taps of THIS source */
    int32_t stride_y, stride_x;   /* input step per output step, 1 or 2 (in the source's logical coordinates) */
    int32_t pad_top, pad_left;    /* logical input row = oy*stride_y - pad_top + ky  (zero outside) */
    int32_t up_shift;    /* 0, or 1 = nearest-neighbour x2 upsampling (UpSampling2D) fused into the gather */
    int32_t off_y;       /* placement offset of the stored tensor inside the logical one: */
    int32_t off_x;       /*   logical[y][x] = stored[y-off_y][x-off_x] (zero outside); one_side_pad = (1,1) */
} sbbseg_conv_src;

typedef struct {
    int32_t n_src;               /* 1 or 2.  2 = channel concat [src0, src1] (Concatenate fused); the two
                                    sources may have different taps/strides: the planner rewrites a 3x3 conv
                                    over [UpSampling2D(x), skip] as four output-parity classes, each a 2x2 conv
                                    over x at its own resolution (taps that hit the same source pixel are
                                    pre-summed) plus the 3x3 stride-2 conv over the skip */
    sbbseg_conv_src src[2];
    int32_t cout;
    int32_t out_h, out_w;        /* output grid of this op */
    int32_t out_stride_y, out_stride_x, out_off_y, out_off_x;
                                 /* placement in the output tensor(s): tensor[y*stride+off] = result[y] */
    int32_t out_tensor;          /* y = act(scale*conv + shift [+ residual]);  -1 = none */
    int32_t relu;
    int32_t residual_tensor;     /* -1 = none (Add fused into the epilogue) */
    int32_t raw_out_tensor;      /* -1 = none; second output raw_scale*conv + raw_shift, no activation
                                    (the stem's pre-BN skip f1) */
    int32_t head_classes;        /* > 0: fuse the network head (1x1 conv + BN + softmax + argmax, main.py:290)
                                    into this conv's epilogue (needs cout == 32, <= 4 classes, 16-bit mode);
                                    labels/probabilities are the plan's outputs, out_tensor may be -1 */
    double algorithmic_macs;     /* MACs per patch of the reference's formulation of this op (for reporting);
                                    0 = derive from the geometry given here */
} sbbseg_conv_desc;

/* w_src0 / w_src1: float32 [kh][kw][channels][cout] per source (Keras kernel layout); scale/shift:
 * float32 [cout] (BatchNorm and bias folded by the caller); raw_*: only if raw_out_tensor >= 0;
 * head_w [cout][classes], head_scale/head_shift [classes]: only if head_classes > 0. */
int sbbseg_add_conv(sbbseg_ctx* c, const sbbseg_conv_desc* d, const float* w_src0, const float* w_src1,
                    const float* scale, const float* shift,
                    const float* raw_scale, const float* raw_shift,
                    const float* head_w, const float* head_scale, const float* head_shift);
/* k x k max-pool, 'valid'.  pre_scale/pre_shift [C] (or NULL) + pre_relu: per-channel affine and ReLU
 * applied to every input element before the max (a BatchNormalization + relu fused into the pool). */
int sbbseg_add_maxpool(sbbseg_ctx* c, int src_tensor, int dst_tensor, int k, int stride,
                       const float* pre_scale, const float* pre_shift, int pre_relu);
/* Fused network tail (16-bit modes): ReLU(BN(conv3x3 'same' over [UpSampling2D(2)(src0: 64 channels),
 * network input (3 channels, C8 form)])) -> 32 channels -> 1x1 conv + BN + softmax + argmax, in one
 * launch that writes only labels (and probabilities on request).  w_src0 [3][3][64][32], w_img
 * [3][3][3][32] (Keras layout, original 3x3 taps: the library pre-sums them per output parity);
 * scale/shift [32]; head_w [32][classes], head_scale/head_shift [classes], classes <= 4. */
int sbbseg_add_tail(sbbseg_ctx* c, int src0_tensor, int img_c8_tensor, const float* w_src0, const float* w_img,
                    const float* scale, const float* shift, int classes,
                    const float* head_w, const float* head_scale, const float* head_shift,
                    double algorithmic_macs);
/* Final 1x1 conv + BN + softmax + argmax (main.py:290) over src_tensor's channels:
 * w [cin][classes], scale/shift [classes].  Produces u8 labels and (on request) f32 probabilities. */
int sbbseg_add_head(sbbseg_ctx* c, int src_tensor, int cin, int classes,
                    const float* w, const float* scale, const float* shift);
int sbbseg_finalize(sbbseg_ctx* c, int max_batch);

/* ---- queries */
int sbbseg_model_info(sbbseg_ctx* c, int* H, int* W, int* classes, int* max_batch);
int sbbseg_num_ops(sbbseg_ctx* c, int* n);
int sbbseg_op_info(sbbseg_ctx* c, int op, char* name, int name_len, double* flops_per_patch,
                   double* min_bytes_per_patch);
/* MFMA FLOPs op `op` really issues per patch (contraction axis padded to whole K-steps, parity-split decoder convs
 * with pre-summed taps, three MFMAs per product in the split mode): the numerator of bench.py's `frac_issued`;
 * sbbseg_op_info's flops are the ALGORITHMIC ones (reference formulation). */
int sbbseg_op_issued_flops(sbbseg_ctx* c, int op, double* issued_flops_per_patch);
int sbbseg_device_bytes(sbbseg_ctx* c, size_t* bytes);

/* ---- seam 2: model.predict (main.py:287-288, 373-374).
 * x: host float32 [n][H][W][3] already scaled to [0,1]; probs: host float32 [n][H][W][classes]. */
int sbbseg_predict(sbbseg_ctx* c, const float* x_nhwc, int n, float* probs_nhwc);

/* ---- seam 1, patches=True (main.py:231-366), fused: u8/255 LUT normalise, tile with 10 % margin,
 * forward, argmax, margin-crop + last-writer-wins stitch.  page: uint8 [Hp][Wp][3];
 * labels: uint8 [Hp][Wp] (the reference returns this plane replicated x3). */
int sbbseg_segment_page(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, uint8_t* labels_hw);
/* do_prediction(patches=True) for n_pages HOST pages of one size (uint8 [Hp][Wp][3] each; pages_hwc / labels_hw are arrays of
 * n_pages pointers; labels as in sbbseg_segment_page, x3 with sbbseg_set_label_channels(3)).  Pipelined in groups of as many
 * pages as fill a chunk: while one group runs, the next is staged into pinned memory and uploaded on a copy stream and the
 * previous group's label planes come back on another -- page-at-a-time callers (main.py:490-503 per page) pay the PCIe
 * copies serially.  Results equal n_pages sbbseg_segment_page calls. */
int sbbseg_segment_pages(sbbseg_ctx* c, int n_pages, const uint8_t* const* pages_hwc, int Hp, int Wp, uint8_t* const* labels_hw);
/* Many equally sized pages in one call (the reference walks them one by one: ocrd_cli.py:51 -> main.py:2056 per page): their
 * tiles are pooled into chunks of up to max_batch tiles, so launches stay large when a page has few tiles (a 3500x2500 page has
 * 70; the persistent conv grids want a few hundred).  d_pages_hwc / d_labels_hw: HOST arrays of n_pages DEVICE pointers
 * (uint8 [Hp][Wp][3] in, uint8 [Hp][Wp] out).  Result per page == sbbseg_segment_page_dev. */
int sbbseg_segment_pages_dev(sbbseg_ctx* c, int n_pages, const void* const* d_pages_hwc, int Hp, int Wp, void* const* d_labels_hw);
int sbbseg_segment_page_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, void* d_labels_hw);

/* Same, with the page rescale of get_image_and_scales (main.py:196-214: cv2.resize INTER_NEAREST to Hp x Wp)
 * fused into the tile gather: page is the STORED image [Hs][Ws][3], labels are [Hp][Wp]; the rescaled
 * page is never materialised.  Identical to sbbseg_segment_page on the nearest-resized page. */
int sbbseg_segment_page_scaled(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp,
                               uint8_t* labels_hw);

/* The layout stage's caller fused in: extract_text_regions (main.py:439-447) = otsu_copy (main.py:178-194:
 * cv2.threshold(channel 0, THRESH_BINARY + THRESH_OTSU), the channel-0 result written to all three
 * channels) + astype(uint8) + do_prediction(patches=True), on the page rescaled to Hp x Wp as above
 * (Hs == Hp and Ws == Wp: no rescale).  Histogram and threshold run on the device; the binarised page
 * is never materialised (the tile gather compares channel 0 with the threshold).  *threshold (may be
 * NULL) receives the Otsu threshold. */
int sbbseg_segment_page_otsu(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp,
                             uint8_t* labels_hw, int* threshold);
/* building blocks of the same for sharded runs: threshold of a device page into a device int, and a
 * tile range gathered through that threshold */
int sbbseg_otsu_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int* d_threshold);
int sbbseg_segment_tile_range_bin_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int first_tile,
                                      int n_tiles, const int* d_threshold, void* d_tile_labels);

/* The two patch stages as textline_detector.run() really calls them (main.py:2061, 2072, 2102): on extract_page's CROPPED page.
 * page = the STORED image [Hs][Ws][3]; Hp x Wp = its size after get_image_and_scales (main.py:196-214); {cx, cy, cw, ch} =
 * extract_page's box on the upscaled page (cv2.boundingRect convention, main.py:404-409); labels = [ch][cw] (x3 with
 * sbbseg_set_label_channels(3)).  binarise != 0: otsu_copy of the CROPPED page first (extract_text_regions, main.py:443: the
 * threshold is the Otsu threshold of the crop's channel 0; *threshold receives it), binarise == 0: textline_contours
 * (main.py:494).  Upscale, crop and binarisation are index arithmetic in the tile gather: neither the upscaled page nor the
 * crop is materialised.  Equal to sbbseg_segment_page[_otsu] on the materialised crop of the nearest-resized page.
 * _dev: page / labels / threshold (may be NULL) are device pointers, work is enqueued on the handle's stream. */
int sbbseg_segment_crop(sbbseg_ctx* c, const uint8_t* page_hwc, int Hs, int Ws, int Hp, int Wp, int cx, int cy, int cw, int ch,
                        int binarise, uint8_t* labels_hw, int* threshold);
int sbbseg_segment_crop_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hs, int Ws, int Hp, int Wp, int cx, int cy, int cw, int ch,
                            int binarise, void* d_labels_hw, int* d_threshold);

/* Many crops in one call: the tiles of differently sized pages and crops share launches.  A VIEW is what sbbseg_segment_crop_dev takes --
 * the stored page [Hs][Ws][3], its size Hp x Wp after get_image_and_scales, the crop box on the upscaled page (the full page:
 * {0, 0, Wp, Hp}), binarise, the label plane [ch][cw] to write and (optional, binarised views) a device int that receives the crop's Otsu
 * threshold.  The result of view k equals sbbseg_segment_crop_dev on that view alone with the same handle settings, byte for byte.
 * The tiles of all views form one list, view-major (within a view in the reference's call order, less the repeated clamped tile under
 * sbbseg_set_dedupe), cut into chunks of <= max_batch tiles exactly as sbbseg_segment_pages_dev cuts its list; views are taken in groups
 * of about eight chunks, which bounds the tile-label scratch whatever n_views is.  Per call ONE asynchronous upload carries the view
 * table and the nearest maps of the rescaled views; per lane-chunk there is one ingest and one region-table launch however many views
 * the chunk spans, per group one stitch launch (every pixel's owner tile in closed form); nothing in the call waits for the device unless a
 * buffer has to grow.  A bad view (null pointer, box leaving the page, crop smaller than the model input) fails the call before anything is
 * launched; sbbseg_last_error() names its index.
 * sbbseg_segment_views: the same from and to host memory -- pages (views with equal d_page_hwc are uploaded once), label planes ([ch][cw],
 * x3 with sbbseg_set_label_channels(3)) and thresholds[n_views] (0 for a view that is not binarised; may be NULL); d_threshold is ignored. */
typedef struct sbbseg_view {
    const void* d_page_hwc;
    int Hs, Ws, Hp, Wp, cx, cy, cw, ch, binarise;
    void* d_labels_hw;
    int* d_threshold;
} sbbseg_view;
int sbbseg_segment_views_dev(sbbseg_ctx* c, int n_views, const sbbseg_view* views);
int sbbseg_segment_views(sbbseg_ctx* c, int n_views, const sbbseg_view* views_host_pointers, int* thresholds);

/* ---- seam 1, patches=False (main.py:368-380): nearest-resize page to the model size, one forward,
 * argmax, nearest-resize labels to out_h x out_w (cv2.INTER_NEAREST index rule). */
int sbbseg_segment_whole(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp,
                         int out_h, int out_w, uint8_t* labels_out);
/* Same for the border stage's actual input: the page do_prediction receives there is the stored image
 * [Hp][Wp] nearest-upscaled to Hs x Ws by get_image_and_scales (main.py:196-214, 387-392).  The two
 * nearest-neighbour index maps are composed, the upscaled page is never built. */
int sbbseg_segment_whole_scaled(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws,
                                int out_h, int out_w, uint8_t* labels_out);

/* The same branch for MANY pages in shared launches: one patch per view, the list cut into chunks of <= max_batch patches exactly as
 * sbbseg_segment_pages_dev cuts its tile list (9 views at max_batch 4: 3 + 3 + 3), the chunks one after the other on the handle's stream.
 * View k's plane equals sbbseg_segment_whole_scaled on that page alone on the same handle with split-K off, byte for byte: the network
 * kernels give a patch the same bits whatever else is in the batch.  SPLIT-K RULE: n_views == 1 takes exactly the one-page route, split-K
 * included when the handle has it on (sbbseg_set_ksplit); n_views >= 2 never splits, not even in a chunk that ends up holding one page.
 * Per call ONE asynchronous upload carries the view table and all nearest maps (the composed model row -> page row -> stored row maps and
 * the output row -> model row maps, shared between views of equal geometry); per chunk there is one ingest launch and one label-resize
 * launch however many views the chunk holds; nothing in the call waits for the device unless a buffer has to grow.  The label planes may
 * start at any address and have any width.  A bad view (null pointer, non-positive size) fails the call before anything is launched;
 * sbbseg_last_error() names its index. */
typedef struct sbbseg_whole_view {
    const void* d_page_hwc;        /* stored page, uint8 [stored_h][stored_w][3], device */
    int stored_h, stored_w;        /* its size */
    int page_h, page_w;            /* size after get_image_and_scales (== stored: no rescale) */
    int out_h, out_w;              /* size of the label plane (main.py:378) */
    void* d_labels_out;            /* uint8 [out_h][out_w], device */
} sbbseg_whole_view;
int sbbseg_segment_whole_views_dev(sbbseg_ctx* c, int n_views, const sbbseg_whole_view* views);

/* ---- stage glue either side of the models, on u8 label planes [H][W]:
 * cv2.erode / cv2.dilate with a ksize x ksize kernel of ones (the reference's self.kernel is 5x5, main.py:57), `iterations` times,
 * OpenCV's default border (outside pixels never win): text_regions erode x 3 / dilate x 4 (main.py:2074-2075), border mask
 * dilate x 6 (main.py:397).  Integer-exact: n iterations of a k x k flat kernel == one (n(k-1)+1)-wide clipped min / max.
 * src may equal dst.  _dev: device pointers, enqueued on the handle's stream. */
#define SBBSEG_MORPH_ERODE  0
#define SBBSEG_MORPH_DILATE 1
int sbbseg_morph_dev(sbbseg_ctx* c, const void* d_src_hw, int H, int W, int op, int ksize, int iterations, void* d_dst_hw);
int sbbseg_morph(sbbseg_ctx* c, const uint8_t* src_hw, int H, int W, int op, int ksize, int iterations, uint8_t* dst_hw);
/* extract_page's box (main.py:394-404): mask > 0 -> dilate 5x5 x 6 -> the component whose OUTER CONTOUR has the largest
 * cv2.contourArea (contours[np.argmax([cv2.contourArea(c) ...])]; a hole's contour lies inside its component's and never wins)
 * -> its bounding box {x, y, w, h} (cv2.boundingRect convention) and pixel count; {0,0,0,0} / 0 when the mask is empty.
 * The contour area of a component = area of the polygon through its boundary pixels' centres = (2x2 pixel cells fully inside)
 * + (cells with three pixels inside) / 2, counted over the component with its holes filled.  The device ranks the components
 * by that sum over the component as it is (a lower bound) and checks the winner against every other component's bounding-box
 * bound; a ring- or frame-shaped blob beside a solid one can leave that undecided, and only then the dilated mask is copied
 * back and the contours are traced on the host (Moore border following + shoelace: exact).  Equal areas: the component whose
 * first pixel comes LAST in raster order wins -- in the reference np.argmax keeps the first maximum of cv2.findContours' list,
 * which runs in reverse discovery order (OpenCV contours.cpp links every new contour in at the head of its parent's child
 * list) [EXT, restated, unpinned: no cv2 build exists here to confirm it on two equal rectangles]. */
int sbbseg_page_box_dev(sbbseg_ctx* c, const void* d_mask_hw, int H, int W, int32_t* box_xywh, int64_t* pixels);
/* extract_page's model + glue in one call: border model on the page as upscaled to Hs x Ws (sbbseg_segment_whole_scaled),
 * then sbbseg_page_box_dev on the label plane while it is still on the device.  mask_out: Hs x Ws labels (x3 with
 * sbbseg_set_label_channels(3)) or NULL. */
int sbbseg_extract_page_box(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws, uint8_t* mask_out,
                            int32_t* box_xywh, int64_t* pixels);
/* the same with the stored page already on the device (run() hands the SAME page to all three stages, main.py:2061-2102: uploaded
 * once, it stays resident for the two patch stages): d_mask_out = device buffer of Hs x Ws labels, or NULL -- the border mask is a
 * local of extract_page (main.py:392-404), only its box leaves the function.  Synchronises the handle's stream (the box is a host
 * result). */
int sbbseg_extract_page_box_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp, int Hs, int Ws, void* d_mask_out,
                                int32_t* box_xywh, int64_t* pixels);

/* extract_page's model + glue for MANY pages: sbbseg_segment_whole_views_dev on all of them (the border forwards at batch width; the
 * split-K rule above applies), then sbbseg_page_box_dev plane by plane -- the component labelling itself is not batched.  Every view's
 * out_h x out_w must equal its page_h x page_w; d_labels_out may be NULL, that page's mask then lives in library scratch.  boxes_xywh
 * [n_pages][4] and pixels [n_pages] (may be NULL) are host arrays; an empty mask gives {0,0,0,0} / 0 for that page and is not an error
 * here.  Per page the results equal sbbseg_extract_page_box_dev with split-K off.  Synchronises the handle's stream. */
int sbbseg_extract_page_boxes_dev(sbbseg_ctx* c, int n_pages, const sbbseg_whole_view* views, int32_t* boxes_xywh, int64_t* pixels);

/* get_text_region_contours_and_boxes' existence test (main.py:456-480), the `if len(contours) > 0` that decides whether run() calls
 * the textline model at all (main.py:2083-2096): pixels == label -> 255, cv2.morphologyEx MORPH_OPEN then MORPH_CLOSE with the 5x5
 * kernel, cv2.findContours(RETR_TREE), keep parentless contours whose polygon area >= min_area * H * W (the reference: min_area =
 * 0.00001, max_area = 1).  *present = 1 when at least one contour is kept.  Decided from the largest outer-contour area of the
 * opened / closed plane (the ranking of sbbseg_page_box_dev); the polygons: sbbseg_text_region_contours_dev below.  Synchronises the stream. */
int sbbseg_text_regions_present_dev(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label, double min_area, int* present);

/* The boxes of those contours (main.py:474-478, `self.boxes`): the same class mask, MORPH_OPEN and MORPH_CLOSE, then cv2.boundingRect
 * {x, y, w, h} of every component that has no parent (it is 4-adjacent to the background connected to the frame: an island inside
 * another component's hole is dropped) and whose outer-contour area lies in [min_area, max_area] x H x W (the reference: 0.00001, 1).
 * *n_boxes = the number found; at most `cap` boxes are written (cap = 0 and boxes_xywh = NULL: count only, then call again).
 * Order [EXT, unpinned]: the component's first pixel in raster order, DESCENDING -- the reverse discovery order assumed for
 * cv2.findContours' list; slopes are per box, nothing downstream depends on it.  The polygons: sbbseg_text_region_contours_dev.
 * Synchronises the stream.  The second form takes a HOST plane. */
int sbbseg_text_region_boxes_dev(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label, double min_area, double max_area,
                                 int32_t* boxes_xywh, int cap, int* n_boxes);
int sbbseg_text_region_boxes(sbbseg_ctx* c, const uint8_t* regions_hw, int H, int W, int label, double min_area, double max_area,
                             int32_t* boxes_xywh, int cap, int* n_boxes);

/* The CONTOURS themselves (main.py:471-481, what get_text_region_contours_and_boxes returns), traced on the device: the same front end,
 * then the outer border of every parentless component as cv2.findContours(CHAIN_APPROX_SIMPLE) lists it [EXT, restated from OpenCV's
 * border follower, unpinned] -- first point = the component's first pixel in raster order, counter-clockwise on the screen, a point
 * kept where the direction changes.  A contour is kept when it has at least three points (main.py:82-83) and its polygon area -- the
 * exact doubled shoelace sum of the traced chain; no bounds, no host tracing -- lies in [min_area, max_area] x H x W.  Order as the boxes
 * call: descending first pixel.  *n_contours / *n_points = contours kept and their points in all.  The result -- boxes {x, y, w, h},
 * doubled areas, point offsets, points -- stays in device memory the handle owns until the next contour call on the handle; read it with
 * sbbseg_text_region_contours_read.  No label plane leaves the device.  A walk that does not close within 8 x (box pixels) + 8 steps (a
 * damaged label plane) is an error.  Synchronises the stream.  The second form takes a HOST plane. */
int sbbseg_text_region_contours_dev(sbbseg_ctx* c, const void* d_regions_hw, int H, int W, int label, double min_area, double max_area,
                                    int* n_contours, int64_t* n_points);
int sbbseg_text_region_contours(sbbseg_ctx* c, const uint8_t* regions_hw, int H, int W, int label, double min_area, double max_area,
                                int* n_contours, int64_t* n_points);
/* Copies the handle's last contour result out: boxes_xywh [n][4], area2 [n] (TWICE cv2.contourArea), point_off [n + 1] (contour k owns
 * points point_off[k] .. point_off[k + 1]), points_xy [points][2].  cap_contours / cap_points: room in the caller's arrays; too little of
 * either is an error that writes nothing.  Synchronises the stream. */
int sbbseg_text_region_contours_read(sbbseg_ctx* c, int32_t* boxes_xywh, int64_t* area2, int64_t* point_off, int cap_contours, int32_t* points_xy,
                                     int64_t cap_points);
/* The host twin of the tracer (no GPU, no handle): the contour of EVERY 8-connected component of mask != 0 -- no morphology, no filter --
 * by descending first pixel, in the same tables.  All four tables NULL: only *n_contours / *n_points are set (call again with room). */
int sbbseg_mask_contours_host(const uint8_t* mask_hw, int H, int W, int32_t* boxes_xywh, int64_t* area2, int64_t* point_off, int cap_contours,
                              int32_t* points_xy, int64_t cap_points, int* n_contours, int64_t* n_points);

/* ---- device buffers for callers without a device runtime of their own.  The reference's environment is Keras/TF (requirements.txt),
 * not PyTorch: what run() keeps resident across its three stages (main.py:2056-2107: the stored page, the border mask, the region
 * map, the textline map) lives in buffers the library hands out, and every `_dev` entry point above accepts them.  A buffer belongs
 * to the handle that allocated it (sbbseg_destroy frees what is left); any handle on the same device may use it.  upload / download
 * return when the copy is complete.  sbbseg_download_labels: a u8 label plane [pixels] as 1 channel or as the 3 identical channels
 * do_prediction returns (main.py:366), replicated on the device. */
int sbbseg_device_alloc(sbbseg_ctx* c, size_t bytes, void** d_ptr);
int sbbseg_device_free(sbbseg_ctx* c, void* d_ptr);                       /* NULL ok; a pointer of another handle is an error */
int sbbseg_upload(sbbseg_ctx* c, void* d_dst, const void* src, size_t bytes);
int sbbseg_download(sbbseg_ctx* c, void* dst, const void* d_src, size_t bytes);
int sbbseg_download_labels(sbbseg_ctx* c, uint8_t* dst, const void* d_labels_hw, size_t pixels, int channels);

/* ---- the model-running part of textline_detector.run() (main.py:2056-2107) in ONE call, for callers that want neither Python glue
 * nor device pointers: three finalized handles on one device (border, layout, textline model), the stored page in host memory, the
 * upscaled size Hs x Ws (get_image_and_scales, main.py:196-214).  The page is uploaded once and stays on the device for all three
 * stages.  Error behaviour mirrors run(): extract_page sits outside the reference's try (main.py:2061) -- its failures, an empty
 * border mask included, fail the call; the layout stage and its glue sit in a bare try / except (2069-2091) -- a failure there (a
 * crop smaller than the model input) leaves info->regions_ok = 0 and skips the textline model; the textline model runs only when
 * get_text_region_contours_and_boxes would return a contour (2083, 2096: info->text_present) and a failure there is "no lines"
 * (2152-2157: info->textlines_ok = 0).  Outputs, caller-allocated for the WORST case (the box may be the whole page):
 *   page_mask_out   Hs x Ws x channels bytes or NULL   border labels at the upscaled size
 *   regions_out     Hs x Ws x channels bytes            cleaned layout labels of the box, h x w x channels, densely packed
 *   textlines_out   Hs x Ws bytes                       textline labels of the box, h x w
 * channels = 1 or 3 (the reference's three identical channels, main.py:366). */
typedef struct sbbseg_run_info {
    int32_t box_xywh[4];      /* extract_page's box on the upscaled page (cv2.boundingRect convention) */
    int64_t box_pixels;       /* pixels of the winning component of the dilated border mask */
    int32_t otsu_threshold;   /* otsu_copy's threshold on the crop's channel 0 (main.py:178-194) */
    int32_t regions_ok;       /* 1: regions_out holds the cleaned layout map */
    int32_t text_present;     /* 1: a text-region contour would be kept (the textline model ran) */
    int32_t textlines_ok;     /* 1: textlines_out holds the textline map */
} sbbseg_run_info;
int sbbseg_run_page(sbbseg_ctx* border, sbbseg_ctx* layout, sbbseg_ctx* textline, const uint8_t* page_hwc, int Hp, int Wp, int Hs, int Ws,
                    int channels, uint8_t* page_mask_out, uint8_t* regions_out, uint8_t* textlines_out, sbbseg_run_info* info);

/* The same for MANY pages in one resident, pooled call (the reference walks a directory one run() at a time, ocrd_cli.py:51 ->
 * main.py:2056).  All stored pages are uploaded once into buffers of the border handle; sbbseg_extract_page_boxes_dev runs for all of
 * them; the layout model takes the crops of all pages that have a box and can hold one model input in ONE sbbseg_segment_views_dev call
 * (binarised); erode x 3 / dilate x 4 and the text-region gate run per page on the device; the textline model takes the crops of the pages
 * that passed the gate and fit in one more sbbseg_segment_views_dev call; then the results come back.  Per page the fields are those of
 * sbbseg_run_page (Hp x Wp = the stored size, Hs x Ws = the upscaled size; outputs sized for the worst case, page_mask_out may be NULL).
 * A page whose crop cannot hold a model input is kept out of that model's call by a geometry test and gets regions_ok = 0 /
 * textlines_ok = 0 exactly as sbbseg_run_page gives it; an empty border mask sets that page's status to 1 and leaves its other outputs
 * untouched, the call still returns 0; a device or allocation error fails the whole call.  With sbbseg_set_ksplit off on the border handle
 * every output byte, info field and status of page k equals one sbbseg_run_page call for that page on the same handles; with split-K on
 * (the default) only the border mask may differ, at near-ties of the split and unsplit forwards (n_pages >= 2 never splits).
 * DEVICE MEMORY, all of it held at once (the caller chooses n_pages), growing only when a call needs more than the last:
 *   border handle:  sum over pages of (3 x Hp x Wp + Hs x Ws) bytes  -- the stored pages and one mask plane per page
 *   layout handle:  2 x sum over pages with a box of (w x h) bytes    -- two crop planes per page (raw / textline map, cleaned layout map)
 * each plane rounded up to 16 bytes, beside what the per-page calls use (the component labelling works on one plane at a time). */
typedef struct sbbseg_run_page_io {
    const uint8_t* page_hwc; int Hp, Wp, Hs, Ws;          /* as sbbseg_run_page */
    uint8_t *page_mask_out, *regions_out, *textlines_out; /* as sbbseg_run_page, worst-case sized; mask may be NULL */
    sbbseg_run_info info;
    int32_t status;   /* 0 ok; 1 = extract_page failed for THIS page (empty border mask, main.py:399-401): its other outputs are untouched */
} sbbseg_run_page_io;
int sbbseg_run_pages(sbbseg_ctx* border, sbbseg_ctx* layout, sbbseg_ctx* textline, int n_pages, sbbseg_run_page_io* pages, int channels);

/* What sbbseg_run_pages leaves on the device.  regions[k] / textlines[k] (n_pages entries each, written by the call): the cleaned layout
 * plane and the textline plane of page k of the LAST successful sbbseg_run_pages that had this handle as `layout`, both h x w of that
 * page's box (info.box_xywh), one byte per pixel; d_hw = NULL where that page's regions_ok / textlines_ok is 0 (and for a page of status
 * 1).  The pointers lead into buffers of the layout handle: they stay valid until the next sbbseg_run_page or sbbseg_run_pages that names
 * one of the three handles, or until sbbseg_destroy, and must not be freed or written.  Status + sbbseg_last_error() when the last
 * sbbseg_run_pages on the handle failed, when there was none, when an sbbseg_run_page came after it, or when n_pages differs from that
 * call's.  The handle keeps only the per-page offsets and flags for this; no device memory is added.
 * STREAMS: when sbbseg_run_pages returns 0, the streams of all three handles have been synchronised behind everything the call queued
 * (the border handle's at the hand-over to the other two; the layout and textline handles' by the download of every plane they wrote --
 * the textline planes lie in the layout handle's buffer but are written on the TEXTLINE handle's stream, and their downloads wait for
 * it).  Any handle of the device may therefore read the planes, e.g. with the sbbseg_planes_* calls below, without synchronising. */
typedef struct sbbseg_plane { const void* d_hw; int32_t H, W; } sbbseg_plane;   /* dense u8 [H][W] in device memory */
int sbbseg_run_pages_planes(sbbseg_ctx* layout, int n_pages, sbbseg_plane* regions, sbbseg_plane* textlines);

/* ---- stage glue: the rotate-and-project of the deskew search (return_deskew_slope, main.py:1601-1718; per text region,
 * 80 angles in [-25, 25] and 30 more in [-90, -50] -- the reference spreads the regions over cpu_count() processes,
 * main.py:1760-1799).  The H x W u8 region mask is centred on a zero square of side S = (int)(1.4 * max(H, W))
 * (sbbseg_deskew_side; main.py:1613-1621), rotated by every angle exactly as rotate_image does (main.py:159-163:
 * cv2.getRotationMatrix2D((S/2, S/2), angle, 1.0) + cv2.warpAffine INTER_CUBIC / BORDER_REPLICATE), binarised (!= 0,
 * main.py:1642) and summed along its rows (main.py:1546).  counts: host int32 [n_angles][S].  One launch for the sweep.
 * matrices (optional, [n_angles][6] forward 2 x 3 maps) overrides angles_deg; otherwise sbbseg_rotation_matrix is used.
 * The 1-D peak logic on the profiles (scipy gaussian_filter1d / find_peaks, main.py:1545-1599) of this ONE-region call stays on the
 * host (stages.return_deskew_slope); for all boxes of a page it runs on the device (sbbseg_profile_statistics_dev,
 * sbbseg_region_deskew_slopes below).  [EXT, unpinned]: OpenCV 4.5.1's warpAffine arithmetic is restated (fixed-point source
 * coordinates with 5 fractional bits, float bicubic table with A = -0.75, replicated borders); cv2 is not available to
 * pin it against. */
int sbbseg_deskew_side(int H, int W, int* side);
int sbbseg_rotation_matrix(double cx, double cy, double angle_deg, double* m6);
int sbbseg_deskew_profiles_dev(sbbseg_ctx* c, const void* d_mask_hw, int H, int W, const double* matrices, const double* angles_deg,
                               int n_angles, int32_t* counts);
int sbbseg_deskew_profiles(sbbseg_ctx* c, const uint8_t* mask_hw, int H, int W, const double* matrices, const double* angles_deg,
                           int n_angles, int32_t* counts);

/* The same rotate-and-project for ALL text-region boxes of a page in one call (do_work_of_slopes, main.py:1728-1738).  textline_hw: the
 * u8 textline label plane [H][W]; boxes_xywh: n_boxes x {x, y, w, h} inside it.  Per box: crop (crop_image_inside_box), cv2.erode with
 * the 5x5 kernel `erode_iterations` times ON THE CROP (the reference: 2; 0 = none), centre on the zero square of side
 * S_r = int(1.4 * max(h_r, w_r)), rotate by every angle, binarise (!= 0), sum the rows -- bit for bit what sbbseg_deskew_profiles gives
 * for the eroded crop.  counts is packed: region r starts at offsets[r] and holds [n_angles][S_r] int32; offsets has n_boxes + 1
 * entries, the last one is the total.  counts = NULL: only offsets is filled (to size counts; needs no handle).  All regions and
 * angles run in three launches whatever n_boxes is; one device-to-host copy.  A box that leaves the plane, w or h < 1, or
 * S_r > 32767 is an error (status + sbbseg_last_error()).  Synchronises the stream. */
int sbbseg_region_deskew_profiles_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                      int erode_iterations, const double* angles_deg, int n_angles, int32_t* counts, int64_t* offsets);
int sbbseg_region_deskew_profiles(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                  int erode_iterations, const double* angles_deg, int n_angles, int32_t* counts, int64_t* offsets);

/* ---- stage glue: the 1-D statistic of the deskew search and the angle selection (get_standard_deviation_of_summed_textline_patch_along_width,
 * main.py:1545-1599; the angle loops of return_deskew_slope, main.py:1630-1716).  Per row profile y (n samples): z = gaussian_filter1d(y),
 * the maxima of z and the minima of the padded, flipped profile (y between 10 zeros, max - that between 10 more zeros, smoothed,
 * find_peaks(height = 0), positions - 20 with numpy's indexing: a negative one wraps, one >= n is the reference's IndexError), the "deep"
 * minima z < L - L / multiplier with L = mean(maxima > 10), and np.std(z).  Every float64 value equals scipy's / numpy's BIT FOR BIT
 * (multiplies and adds rounded one by one in correlate1d's order, numpy's pairwise sums, correctly rounded divide and sqrt), because the
 * winner is an arg max in which equal maxima occur and find_peaks compares exactly.
 *   counts / offsets    packed as sbbseg_region_deskew_profiles packs them: region r holds [n_angles][S_r] int32 from offsets[r]; offsets
 *                       has n_regions + 1 entries; S_r = 1 .. 32767
 *   weights, radius     the half Gaussian kernel weights[0 .. radius], weights[j] = normalised weight at distance j, computed by the CALLER
 *                       as scipy.ndimage does (numpy's exp: libm's differs in the last bit for some sigma).  weights = NULL: the built-in
 *                       table of sigma = 2 (radius 8), the only sigma the reference uses (main.py:1737); `radius` is then ignored
 *   multiplier          the reference passes 20.3 (main.py:1644)
 *   spread  [n_regions][n_angles]   np.std(z) where state is 0, else 0
 *   state   [n_regions][n_angles]   0 appended; 1 skipped (no deep minimum: NOT appended); 2 exception (the IndexError: appended, spread 0)
 *   winner  [n_regions]             index into the angle array: the first maximum of the appended spreads, whose POSITION in the shortened
 *                                   list indexes the full angle array (main.py:1655-1665); -1: nothing appended (the slope is then 0)
 *   smooth  (host entry, optional)  z of every profile, packed like counts
 * sbbseg_profile_statistics_host runs serially on the CPU and needs no handle (it is what holds the arithmetic to scipy on a machine
 * without a GPU); sbbseg_profile_statistics_dev takes the counts in DEVICE memory (offsets, weights and the outputs are host arrays; NULL
 * outputs are skipped) and runs all profiles in one launch (a second one for S_r > 2048, whose smoothed profiles do not fit in LDS) plus the
 * selection.  Both give the same bits.  n_angles < 1, radius < 0, bad offsets, a null handle: status + sbbseg_last_error(). */
int sbbseg_profile_statistics_host(const int32_t* counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights, int radius,
                                   double multiplier, double* spread, uint8_t* state, int32_t* winner, double* smooth);
int sbbseg_profile_statistics_dev(sbbseg_ctx* c, const void* d_counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights,
                                  int radius, double multiplier, double* spread, uint8_t* state, int32_t* winner);
/* The angles of return_deskew_slope's two sweeps, bit for bit numpy's: sweep 0 = np.linspace(-25, 25, 80) (main.py:1622), sweep 1 =
 * np.linspace(-90, -50, 30) (main.py:1670).  capacity = 0: only *n_angles is set.  Host only. */
int sbbseg_deskew_sweep_angles(int sweep, double* angles_deg, int capacity, int* n_angles);
/* The whole slope half of do_work_of_slopes (main.py:1728-1748) for a page: crop, erode and the sweep of 80 angles for every box
 * (sbbseg_region_deskew_profiles' launches), statistic and selection on the device, ONE small copy of the winners; then the same with the 30
 * angles of the second sweep for the boxes whose first answer is steeper than 15 degrees only (main.py:1669-1670); then the reference's
 * clean-up (|slope| > 120.5 -> 0; nothing appended -> 0).  slopes: host double [n_boxes].  The row counts never leave the device.
 * weights / radius as above (NULL: sigma = 2).  Errors as sbbseg_region_deskew_profiles (the message names the box); n_boxes = 0 is
 * success.  Synchronises the stream. */
int sbbseg_region_deskew_slopes_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                    int erode_iterations, const double* weights, int radius, double* slopes);
int sbbseg_region_deskew_slopes(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes,
                                int erode_iterations, const double* weights, int radius, double* slopes);

/* ---- stage glue: the deskewed text-line mask of every text region and the two projections the line splitters open on
 * (textline_contours_postprocessing, main.py:1472-1487, called by do_work_of_slopes at main.py:1750 with the ERODED crop and the region's
 * cleaned slope; seperate_lines' row sums, main.py:539; seperate_lines_vertical's column sums, main.py:1020).  Per box [x, y, w, h] of
 * the u8 textline plane, with slopes[r] in degrees (as sbbseg_region_deskew_slopes returns them):
 *   a. crop, cv2.erode with the 5x5 kernel `erode_iterations` times on the crop (the reference: 2) -- sbbseg_region_deskew_profiles' crops;
 *   b. * 255 in uint8, MORPH_OPEN then MORPH_CLOSE with the 5x5 kernel on the crop (erode, dilate, dilate, erode; default border: outside
 *      pixels never win), computed as one clipped separable min(5) / max(9) / min(5);
 *   c. rotate_image(mask, slope) (main.py:159-163): getRotationMatrix2D((w / 2, h / 2), slope, 1.0) (integer halves), warpAffine onto the
 *      crop's own (w, h), INTER_CUBIC, BORDER_REPLICATE.  The source is uint8, so this is OpenCV's FIXED-POINT bicubic path, not the float
 *      path of the deskew sweep above.  [EXT, unpinned: OpenCV 4.5.1 imgwarp.cpp (initInterTab2D, remapBicubic) restated from memory; cv2 is
 *      not available to pin it against.]  Source coordinates and table indices: as the deskew sweep (5 fractional bits).  Weights: for every
 *      (ay, ax) the 16 entries i[r][c] = saturate_cast<short>(float(tab[ay][r] * tab[ax][c]) * 32768), tab = the float bicubic table
 *      (A = -0.75), rounded to nearest even, clamped to int16; if they do not sum to 32768 the difference is removed from one entry of the
 *      2 x 2 block at rows / columns {2, 3}: scanned row-major with both candidates starting at (2, 2), a strictly smaller entry replaces
 *      the minimum candidate, otherwise a strictly larger entry replaces the maximum candidate; a negative difference raises the maximum, a
 *      positive one lowers the minimum.  Pixel: v = clamp((sum over the 16 taps of src * i + 16384) >> 15, 0, 255) in int32 (arithmetic
 *      shift), the taps clamped to the crop.  The builder knows of no difference between this and the OpenCV text;
 *   d. dst = (v != 0) as 0 / 1; rows = dst.sum(axis = 1); cols = dst.sum(axis = 0).  Both projections are returned: the caller picks by
 *      |slope| > 45 as main.py:1514 does.
 * Outputs are HOST buffers packed in box order: masks u8 (region r from mask_off[r], h_r x w_r; NULL: the masks stay on the device),
 * rows int32 (from row_off[r], h_r values), cols int32 (from col_off[r], w_r values).  The three offset arrays have n_boxes + 1 entries
 * (prefix sums of w * h, h and w; the last entry is the total); the caller sizes the buffers from the same sums.  All boxes run in ten launches whatever n_boxes is (crop + erode 2, morphology
 * 6, warp + row sums 1, column sums 1).  n_boxes = 0 is success.  A box that leaves the plane, w or h < 1: status + sbbseg_last_error()
 * (the message names the box).  Shares the deskew sweep's workspace: call order with sbbseg_region_deskew_slopes does not matter.
 * Synchronises the stream.
 * sbbseg_region_line_masks_host: no GPU, no handle -- ONE crop (the textline plane cut to the box, h x w), the same statements on the
 * CPU (csrc/line_mask.h is shared by both); mask may be NULL.  sbbseg_region_line_table: the int16 [32][32][16] weights (host only). */
int sbbseg_region_line_masks_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                                 const double* slopes, uint8_t* masks, int32_t* rows, int32_t* cols, int64_t* mask_off, int64_t* row_off,
                                 int64_t* col_off);
int sbbseg_region_line_masks(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                             const double* slopes, uint8_t* masks, int32_t* rows, int32_t* cols, int64_t* mask_off, int64_t* row_off, int64_t* col_off);
int sbbseg_region_line_masks_host(const uint8_t* crop_hw, int h, int w, int erode_iterations, double slope, uint8_t* mask, int32_t* rows,
                                  int32_t* cols);
int sbbseg_region_line_table(int16_t* itab, int capacity);

/* ---- stage glue: text-line peaks and line boxes per region.  Everything seperate_lines (main.py:516-991) and seperate_lines_vertical
 * (main.py:993-1457) compute from the projection of dst (the row sums, or the column sums for |slope| > 45, main.py:1514): the sigma
 * estimate of the first `try` block (12 where it raises, at least 3), the second pass with that sigma, the merged peaks, their mean / std,
 * the five branches and the corners of every line, unrotated and rotated.  One wave per region on the device, one launch for all regions
 * (a second one when a profile is longer than 2048 samples), the profiles never leave the device between sbbseg_region_line_masks_dev's
 * kernels and this step.  Every float64 result equals scipy's gaussian_filter1d / find_peaks and numpy's mean / std bit for bit, on the
 * device and in the serial host twin (csrc/line_split.h is shared by both).
 *   SCOPE: the contour enters the reference only through cv2.pointPolygonTest (x_min / x_max of the horizontal splitter; the vertical
 *   splitter computes it and never uses it).  These calls do not take it: every line gets the reference's own fallback extent
 *   x_min_cont = 0, x_max_cont = w (main.py:786-788), and sbbseg_region_line_extents_dev (below) then cuts the lines to the region's filled,
 *   rotated contour (main.py:1492-1511) and rewrites the corners.  return_contours_of_image /
 *   filter_contours_area_of_image inside the first `try` (main.py:608-609) are treated as dead and non-raising [EXT] unpinned.
 * Inputs per region r: geom[r] = {length of the profile, the other extent of dst, vertical (0 / 1)}; rot[r] = {cos, -sin, sin, cos, x_d,
 * y_d}: numpy's cos / sin of thetha / 180. * np.pi (thetha = slope, + 90 first for the vertical splitter) and M[0, 2], M[1, 2] of
 * getRotationMatrix2D((w // 2, h // 2), -thetha, 1.0) (sbbseg_rotation_matrix); libm is not reproduced by the library, so the caller
 * passes them.  profiles: packed int32, region r from offsets[r] (n_regions + 1 entries, offsets[r + 1] - offsets[r] = length).
 * weights / weight_off: the half kernels of gaussian_filter1d for sigma = 2 .. sigma_max one after the other (sigma s: 4 s + 1 doubles
 * from weight_off[s - 2]; sigma_max - 2 + 2 offsets; sigma_max >= 12).  The device uses the table up to sigma 128.
 * Outputs (host buffers).  info[r] = {status, sigma_gaus, 1 if the first estimate raised, branch, line count}; status SBBSEG_LINES_OK,
 * SBBSEG_LINES_NONE (the second pass raised: textline_contours_postprocessing's bare except returns [], main.py:1520) or
 * SBBSEG_LINES_SIGMA_TOO_LARGE (sigma_gaus is in neither table: nothing else was computed; finish the region with
 * sbbseg_line_split_host and that sigma's half kernel as extra_weights / extra_sigma); branch 0 .. 4 = main.py:744, 822, 825, 864, 919
 * in that order, -1 = not reached.  Lines are packed by CAPACITY: region r owns lines line_off[r] .. line_off[r + 1] with
 * line_off[r + 1] - line_off[r] = (length + 40) / 2 (the maxima of the padded profile bound the peaks, and the merged list is never longer);
 * line_off has n_regions + 1 entries and is written by the call, the caller sizes lines [total][3] = {peak, point_up, point_down},
 * corners [total][4][2] (main.py:817-820) and corners_rot [total][4][2] (int(a * x + b * y + d), every operation rounded on its own,
 * with the reference's four `< 0` clamps) from the same sums.  Only the first `count` lines of a region are written; the buffers need no
 * fill.  sbbseg_line_split_host: serial, no handle, no GPU.  sbbseg_region_line_boxes(_dev): sbbseg_region_line_masks' steps a .. d on
 * all boxes and then the split of each box's own profile, boxes and slopes in, line boxes out; rot as above with (w, h) of the box.
 * Synchronise the stream. */
#define SBBSEG_LINES_OK 0
#define SBBSEG_LINES_NONE 1
#define SBBSEG_LINES_SIGMA_TOO_LARGE 2
int sbbseg_line_split_host(const int32_t* profiles, const int64_t* offsets, int n_regions, const int32_t* geom, const double* rot, const double* weights,
                           const int64_t* weight_off, int sigma_max, const double* extra_weights, int extra_sigma, int32_t* info, int64_t* line_off,
                           int32_t* lines, int32_t* corners, int32_t* corners_rot);
int sbbseg_line_split_dev(sbbseg_ctx* c, const void* d_profiles, const int64_t* offsets, int n_regions, const int32_t* geom, const double* rot,
                          const double* weights, const int64_t* weight_off, int sigma_max, int32_t* info, int64_t* line_off, int32_t* lines,
                          int32_t* corners, int32_t* corners_rot);
int sbbseg_region_line_boxes_dev(sbbseg_ctx* c, const void* d_textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                                 const double* slopes, const double* rot, const double* weights, const int64_t* weight_off, int sigma_max, int32_t* info,
                                 int64_t* line_off, int32_t* lines, int32_t* corners, int32_t* corners_rot);
int sbbseg_region_line_boxes(sbbseg_ctx* c, const uint8_t* textline_hw, int H, int W, const int32_t* boxes_xywh, int n_boxes, int erode_iterations,
                             const double* slopes, const double* rot, const double* weights, const int64_t* weight_off, int sigma_max, int32_t* info,
                             int64_t* line_off, int32_t* lines, int32_t* corners, int32_t* corners_rot);

/* ---- the three per-box calls above for boxes that lie on MANY planes (the textline planes of many pages: sbbseg_run_pages_planes), the
 * boxes of all planes sharing the launches.  planes: n_planes records; box r = boxes_xywh[4 r ..] lies on planes[box_plane[r]].  Boxes come
 * in any order; a plane may have no box (its d_hw may then be NULL) or be named by many.  Every per-box result -- slopes; masks, row and
 * column sums; every field of the line records -- equals bit for bit what the one-plane `_dev` call gives for that box on that plane, and
 * the outputs are packed in BOX order exactly as there (offsets, capacities, buffers: see the one-plane calls).  Only the row pass of the
 * crops reads the planes, through one (pointer, width) record per box; every later kernel works on the packed crops.  The number of
 * launches does not depend on n_planes or n_boxes: per slope sweep 3 + the statistic's 2 or 3 (the second sweep re-crops only the boxes
 * steeper than 15 degrees, with their planes); line masks 10; line boxes 11 or 12.  Nothing is uploaded but the small tables.
 * Errors (status + sbbseg_last_error(); checked on the host before anything is queued, the message names the box): box_plane[r] outside
 * 0 .. n_planes - 1; a box that leaves ITS OWN plane, w or h < 1; a plane named by a box whose d_hw is NULL; n_planes < 1 with n_boxes > 0.
 * n_boxes = 0 is success.  The limits of the one-plane calls ("too much work for one call ... split the boxes") apply to the totals over
 * all planes.  Each call synchronises the handle's stream; the planes must be complete when it is called (see sbbseg_run_pages_planes). */
int sbbseg_planes_deskew_slopes_dev(sbbseg_ctx* c, const sbbseg_plane* planes, int n_planes, const int32_t* boxes_xywh, const int32_t* box_plane,
                                    int n_boxes, int erode_iterations, const double* weights, int radius, double* slopes);
int sbbseg_planes_line_masks_dev(sbbseg_ctx* c, const sbbseg_plane* planes, int n_planes, const int32_t* boxes_xywh, const int32_t* box_plane, int n_boxes,
                                 int erode_iterations, const double* slopes, uint8_t* masks, int32_t* rows, int32_t* cols, int64_t* mask_off,
                                 int64_t* row_off, int64_t* col_off);
int sbbseg_planes_line_boxes_dev(sbbseg_ctx* c, const sbbseg_plane* planes, int n_planes, const int32_t* boxes_xywh, const int32_t* box_plane, int n_boxes,
                                 int erode_iterations, const double* slopes, const double* rot, const double* weights, const int64_t* weight_off,
                                 int sigma_max, int32_t* info, int64_t* line_off, int32_t* lines, int32_t* corners, int32_t* corners_rot);

/* ---- stage glue: the x extent of every text line from its region's filled, rotated contour -- the contour half of
 * textline_contours_postprocessing (main.py:1492-1511) and cv2.pointPolygonTest inside seperate_lines (main.py:780-791, 878-889, 945-956);
 * csrc/line_extent.h is shared by the device step and the serial host twin.  Every cv2 rule is [EXT]: restated from the OpenCV 4.5.1
 * text, unpinned (no cv2 to hold it against), reduced to integer predicates:
 *   R1 cv2.fillPoly(zeros (h, w), ring - (x, y), 255).  Scope: rings whose edges between consecutive points (the closing edge included; a
 *      repeated closing point is a zero-length edge) are horizontal, vertical or exact diagonals and whose points lie inside the box --
 *      what CHAIN_APPROX_SIMPLE lists are.  A pixel is set when it lies on an edge, or when an odd number of edges cross its row strictly
 *      left of it (an edge crosses row py when min(y0, y1) <= py < max(y0, y1)).  Any other ring is an error that names the region.
 *   R2 rotate_image on float64: the matrix, inverse map and 5-bit table indices of sbbseg_region_line_masks_dev, the FLOAT bicubic path:
 *      the weight of a tap is the float32 product tab[ay][r] * tab[ax][c]; all of them are multiples of 2^-34, so with a 0 / 255 source
 *      the float64 sum is exact in any order: v = 255 * S / 2^34, S = the integer sum of weight * 2^34 over the taps on set pixels.
 *   R3 .astype(np.uint8) truncates toward zero and keeps the low 8 bits (numpy on x86-64); BGR2GRAY of equal channels is the value;
 *      threshold(., 0, 255, 0): a pixel of threshrot is set iff (trunc(v) & 255) != 0 -- the negative overshoot outside the outline IS set,
 *      |v| < 1 and 256 <= v < 257 are holes.
 *   R4 cv2.findContours(threshrot, RETR_TREE, CHAIN_APPROX_SIMPLE) and np.argmax of the point counts: ALL borders compete, outer borders
 *      and hole borders.  Raster scan over the image padded with zeros; at a position with pixel p and west neighbour q: p set and
 *      unmarked, q background -- an outer border starts there, first search clockwise from west; p background, q set and not marked
 *      "right" -- a hole border starts at q, first search clockwise from east; then the walk of sbbseg_mask_contours_host.  A step marks
 *      the pixel it leaves "right" if its east neighbour was examined as background during the step, "visited" otherwise.  The winner has
 *      the most kept points; among equals the LAST discovered (OpenCV lists borders in reverse discovery order: assumed, as everywhere
 *      in this library) -- `tie` reports that there were equals.  No border: np.argmax([]) raises, the region's lines are [] (status NONE).
 *   R5 per line of the HORIZONTAL splitter (|slope| <= 45): xv = np.linspace(0, w, 1000) (k * (w / 999), the last exactly w); sample k is
 *      inside iff pointPolygonTest(winner, (float32(xv[k]), float32(peak)), True) >= 0: some edge's dist_num is 0, or the crossing
 *      counter is odd; pt.x - v.x is a float32 subtraction, all else float64 signs of sums of two exact products.  x_min = int(min inside
 *      xv), x_max = int(max inside xv); none inside: 0, w.
 *   R6 branches 0, 3 and 4 of the line record take x_min / x_max: corners and corners_rot are rewritten through the writer of
 *      sbbseg_line_split_dev.  Branch 2 and the vertical splitter keep 0 .. w and their corners.
 * sbbseg_region_line_extents_dev: n regions.  Rings: packed int (x, y) points in page coordinates, region r = points point_off[r] ..
 * point_off[r + 1] (closed or not); points_xy = NULL names the handle's resident contour result (sbbseg_text_region_contours_dev), read in
 * place: n must be its contour count.  boxes_xywh [n][4], slopes [n], rot [n][6], info [n][5], line_off [n + 1], lines [total][3]: as
 * passed to and written by sbbseg_region_line_boxes_dev.  Outputs (host): extent [total][2] = x_min, x_max for the first `count` lines of
 * every region with status SBBSEG_LINES_OK (0, w where the step does not apply); corners / corners_rot [total][4][2]: IN / OUT, only the
 * lines R6 names are rewritten; rec [n][8] = {status (SBBSEG_EXTENT_OK, SBBSEG_EXTENT_NONE: the region has no lines), borders found,
 * the winner's points, 1 = the winner is a hole border, 1 = tie, the winner's start pixel x, y, hole borders found}.  The step reads no
 * label plane: the boxes of many pages share one call.  Launches, whatever n is: fill 1, warp + threshold 1, border scan 2 per form in use
 * (bit maps + marks within 60 KB of LDS: the LDS form, else a global workspace -- chosen, not measured; so is one wave per region), extents
 * 1.  No atomics: the results are bit-identical from run to run.  n = 0 is success.  Synchronises the stream.
 * sbbseg_region_line_extents_read: threshrot (uint8 [h][w], 0 / 255) and the winner's points of region `region` of the handle's last
 * extent (or debug mask) call; either may be NULL.  sbbseg_region_line_extents_host: ONE region, serial, no GPU, no handle: the same
 * statements; lines [n_lines][3], branch = info[3]; threshrot / winner_xy optional.  sbbseg_region_line_extent_weights: the int64
 * [32][32][16] table of R2 (host only). */
#define SBBSEG_EXTENT_OK 0
#define SBBSEG_EXTENT_NONE 1
#define SBBSEG_EXTENT_REC_INTS 8
int sbbseg_region_line_extents_dev(sbbseg_ctx* c, const int32_t* points_xy, const int64_t* point_off, int n, const int32_t* boxes_xywh,
                                   const double* slopes, const double* rot, const int32_t* info, const int64_t* line_off, const int32_t* lines,
                                   int32_t* extent, int32_t* corners, int32_t* corners_rot, int32_t* rec);
int sbbseg_region_line_extents_read(sbbseg_ctx* c, int region, uint8_t* threshrot_hw, int32_t* winner_xy, int cap);
int sbbseg_region_line_extents_host(const int32_t* ring_xy, int n_points, const int32_t* box_xywh, double slope, const double* rot, int branch,
                                    const int32_t* lines, int n_lines, int32_t* extent, int32_t* corners, int32_t* corners_rot, int32_t* rec,
                                    uint8_t* threshrot, int32_t* winner_xy, int winner_cap);
int sbbseg_region_line_extent_weights(int64_t* wtab, int capacity);
/* the border scan of R4 alone on raw masks (!= 0; tests): n masks packed one after the other, mask r = wh[2 r] x wh[2 r + 1] bytes; rec as
 * above; winners through sbbseg_region_line_extents_read.  _host: one mask, serially, no GPU. */
int sbbseg_debug_mask_border_winner_dev(sbbseg_ctx* c, const uint8_t* masks, const int32_t* wh, int n, int32_t* rec);
int sbbseg_debug_mask_border_winner_host(const uint8_t* mask, int w, int h, int32_t* rec, int32_t* winner_xy, int cap);
/* a region whose three bit maps (box + ring, 32-bit words) exceed `bytes` is scanned on a global workspace instead of LDS (0 .. 61440, the
 * default; tests lower it so that small shapes reach the global form) */
int sbbseg_debug_set_extent_lds_limit(sbbseg_ctx* c, int bytes);
/* kernels the extent calls have queued on this handle so far */
int sbbseg_debug_extent_launches(sbbseg_ctx* c, int64_t* value);

/* ---- multi-GPU: one process per GPU, one handle per process; tiles (sbbseg_segment_tile_range_dev) or whole
 * pages (sbbseg_segment_pages_dev) are sharded by the caller, and the ONE data-path collective -- the all-gather of the u8
 * label maps -- runs on RCCL inside the library, on the handle's stream, so an integrator needs neither PyTorch nor an MPI:
 *   rank 0:     sbbseg_comm_unique_id(id)  -> ship the 128 bytes to every rank by any means (file, socket, env)
 *   every rank: sbbseg_comm_init(ctx, rank, world, id)            (collective: returns when all ranks have joined)
 *               ... sbbseg_segment_tile_range_dev(...) into my slice ...
 *               sbbseg_allgather_labels_dev(ctx, d_my_slice, bytes_per_rank, d_all)      (d_all = world x bytes_per_rank)
 *               sbbseg_stitch_dev(ctx, d_all, Hp, Wp, d_page_mask)
 * librccl is loaded with dlopen on first use (no link-time dependency: the library loads on machines without it).
 * The reference has no counterpart: main.py:259-288 is a serial loop; tiles and pages are independent there. */
int sbbseg_comm_unique_id(char* id128);
int sbbseg_comm_init(sbbseg_ctx* c, int rank, int world, const char* id128);
int sbbseg_comm_info(sbbseg_ctx* c, int* rank, int* world);       /* world = 0: no communicator */
int sbbseg_comm_destroy(sbbseg_ctx* c);
int sbbseg_allgather_labels_dev(sbbseg_ctx* c, const void* d_send, size_t bytes_per_rank, void* d_recv);

/* ---- building blocks (multi-GPU sharding, tests).  tile_xy: host int32 [n][2] = (x0, y0) origins.
 * d_tile_labels: device uint8 [n][H][W]. */
int sbbseg_tile_grid(int Hp, int Wp, int H, int W, int32_t* tile_xy, int capacity, int* nxf, int* nyf);
/* The index rule every nearest-neighbour rescale of this library uses (page upscale of get_image_and_scales, main.py:214;
 * both resizes of the whole-image branch, main.py:371, 378): map[i] = source index of destination index i for
 * cv2.resize(..., interpolation=cv2.INTER_NEAREST) = min(floor(i * (1 / (dst_len / src_len))), src_len - 1).  Host only. */
int sbbseg_nearest_map(int src_len, int dst_len, int32_t* map);
int sbbseg_segment_tiles_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp,
                             const int32_t* tile_xy, int n_tiles, void* d_tile_labels);
/* same, for the contiguous range [first_tile, first_tile+n_tiles) of the page's own tile grid in the
 * reference's call order (x outer, y inner) -- origins come from the closed form, no table upload.
 * This is the unit of work the multi-GPU path shards. */
int sbbseg_segment_tile_range_dev(sbbseg_ctx* c, const void* d_page_hwc, int Hp, int Wp,
                                  int first_tile, int n_tiles, void* d_tile_labels);
int sbbseg_stitch_dev(sbbseg_ctx* c, const void* d_tile_labels, int Hp, int Wp, void* d_labels_hw);
/* ingest only (tests): fills both input forms for n tiles and copies form `form` back as float32 */
int sbbseg_debug_ingest(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, const int32_t* tile_xy,
                        int n_tiles, int form, float* out, size_t out_floats);
/* copy an activation tensor of the last run back as float32 [n][H][W][C] (tests) */
int sbbseg_debug_read_tensor(sbbseg_ctx* c, int tensor_id, int n, float* out, size_t out_floats);

/* A/B knobs of the conv kernel (benchmarking, tests; results never depend on them).  bits 0-1: tile
 * family (0 auto, 1 = 4 waves / 2 LDS stages, 2 = 8 waves / 3 stages, 3 = big 8-wave tiles);
 * bit 2 = one block per tile instead of persistent blocks; bit 3 = no XCD-grouped tile walk;
 * bit 4 = half-K-step stages in a 4-deep ring; bit 5 = XCD-grouped tile walk on single-class layers too;
 * bit 6 = drain the epilogue stores before the next barrier; bit 7 = half-line (64-byte) epilogue stores; bits 8-15 = with bit 5: K limit (units of
 * 64) up to which every block walks a contiguous run of tiles (0 = keep the current limit);
 * bit 16 = 8-phase schedule on the 256x256 tile (half-tile restaging, staggered wave groups);
 * bit 17 = plain gather (per-load address arithmetic) instead of the fast gather on every layer;
 * bit 18 = fused bottleneck blocks run as the three convs they replace; bit 19 = grouped (parity-class) launches walk
 * XCD-contiguous tile ranges; bit 20 = fused bottleneck blocks run bottleneck_fused (one group of four waves per tile)
 * instead of bottleneck_fused_pq (producer / consumer wave groups) -- split mode: block_x3 prefetches the next tile's inner x in
 * place (inside phase C) instead of into its own registers a tile ahead; bit 21 = sbbseg_page_box_dev always ranks on the host;
 * bit 22 = split mode: stem and max-pool as two launches (stem_conv_pairs_x3 + maxpool_kernel) instead of stem_pool_x3;
 * bit 23 = the 224 x 224 decoder conv on conv_igemm_mfma instead of dec_halo_x3 / dec_halo_f16 (LDS-resident halos);
 * bit 24 = split mode: an identity block's last 1x1 conv and the next block's first 1x1 conv (encoder stages 3 / 4) as two
 * conv_igemm_mfma launches instead of expand_reduce_x3; bit 25 = the 3x3 conv of a stage-3 identity block as its own launch in front
 * of expand_reduce instead of inside conv3_expand_reduce; bit 26 = f16 / bf16 modes: the fused bottleneck blocks also store their
 * intermediates a and b to the plan tensors the three-conv route (bit 18) writes, same bytes otherwise (the per-phase step check of
 * tests/test_gpu_steps_blocks.py) -- nothing in the split mode, whose block_x3 is held bit-identical to its three convs */
int sbbseg_debug_set_conv_variant(sbbseg_ctx* c, int variant);
/* the exact host-side contour ranking of sbbseg_page_box_dev on a host mask that is ALREADY dilated (no GPU needed; tests) */
int sbbseg_debug_largest_contour(const uint8_t* mask_hw, int H, int W, int32_t* box_xywh, int64_t* pixels);
/* ... and TWICE the largest outer-contour area itself (host mirror of sbbseg_text_regions_present_dev's ranking; 0 for an empty mask) */
int sbbseg_debug_largest_contour_area2(const uint8_t* mask_hw, int H, int W, int64_t* area2);
/* closed forms of the owned-region launches (no GPU needed; tests): [lo, hi) in tile coordinates of what the stitch keeps of tile t of an
 * axis of n_tiles tiles (origin(t) = min(t * (tile - 2 margin), extent - tile)), and the rows every decoder level below must produce for
 * it: lo_hi[2 k], lo_hi[2 k + 1] for level k = 0 .. levels - 1, level_size[k] = rows of level k (level 0 = the network output) */
int sbbseg_debug_owned_range(int extent, int tile, int margin, int n_tiles, int t, int* lo, int* hi);
int sbbseg_debug_region_rows(int extent, int tile, int margin, int n_tiles, int t, int levels, const int32_t* level_size, int32_t* lo_hi);
/* ... and the owner of every coordinate of such an axis as the stitch of sbbseg_segment_views_dev computes it (the same closed form, on
 * the host): own[q] = (t << 16) | (q - origin(t)) for the last tile t in paste order that keeps q; own = [extent] */
int sbbseg_debug_axis_owner(int extent, int tile, int margin, int n_tiles, int32_t* own);
/* fill every activation buffer (both lanes), the tile-label scratch and -- once the whole-image branch has allocated it -- the split-K
 * workspace of fp32 partial sums with `byte_value` (tests: a launch that reads what an owned-region launch did not write, or a split whose
 * partial sums were never written, then shows; 0xFF = NaN in every 16-bit format and in fp32) */
int sbbseg_debug_poison_activations(sbbseg_ctx* c, int byte_value);
/* What the LAST launch of plan op `op` used (tests: which kernel route a launch size takes; written by the host where the launch is sized,
 * nothing is read from the device).  out[0 .. min(cap, SBBSEG_LAUNCH_INTS)) =
 *   [0] kernel family, SBBSEG_LAUNCH_* below; NONE: the op has launched nothing (it is fused into another op's launch, or has not run)
 *   [1] BP, [2] BC, [3] LDS stages: pixels x channels of a work item (tile), stages of the staging ring (1 where there is none)
 *   [4] fast_gather (0 plain, 1 masked, 2 pointwise), [5] tile_map (0 .. 3), [6] cls_minor: the generic conv only
 *   [7] 1 = an owned-region table was passed
 *   [8] work items of the launch, [9] blocks launched
 *   [10] generic conv with a residual: 1 = the residual is read in the epilogue, 0 = prefetched with the tile's last K-step
 *   [11] 1 = persistent blocks (grid sized by the CU count, every block loops over work items), 0 = one block per slice of the output
 *   [12] 1 = the launch adds a stored residual
 * A fused bottleneck block that runs as its three convs (conv variant bit 18) reports the last of them. */
#define SBBSEG_LAUNCH_INTS 13
#define SBBSEG_LAUNCH_NONE 0
#define SBBSEG_LAUNCH_CONV_IGEMM 1
#define SBBSEG_LAUNCH_CONV_NAIVE_F32 2
#define SBBSEG_LAUNCH_CONV_SPLITK 3
#define SBBSEG_LAUNCH_STEM 4
#define SBBSEG_LAUNCH_STEM_POOL 5
#define SBBSEG_LAUNCH_DIRECT64 6
#define SBBSEG_LAUNCH_BOTTLENECK 7
#define SBBSEG_LAUNCH_BOTTLENECK_PQ 8
#define SBBSEG_LAUNCH_BLOCK_X3 9
#define SBBSEG_LAUNCH_EXPAND_REDUCE 10
#define SBBSEG_LAUNCH_CONV3_EXPAND_REDUCE 11
#define SBBSEG_LAUNCH_DEC_HALO 12
#define SBBSEG_LAUNCH_TAIL 13
#define SBBSEG_LAUNCH_MAXPOOL 14
#define SBBSEG_LAUNCH_HEAD 15
int sbbseg_debug_op_launch(sbbseg_ctx* c, int op, int32_t* out, int cap);
/* Bytes of activation tensor `tensor_id` in which patch i differs from patch i - period, over period <= i < n and the whole patch stride as
 * stored (every plane, padding included): *count = differing bytes, *first = offset of the first one from the start of patch `period`
 * (-1: none).  One kernel on the handle's stream, waited for (tests: a batch of cyclically repeated patches must come out periodic). */
int sbbseg_debug_tensor_period_mismatches(sbbseg_ctx* c, int tensor_id, int n, int period, int64_t* count, int64_t* first);
/* the device tracer on a raw device mask (!= 0): labels it and traces EVERY root, no morphology and no filter -- shapes OPEN and CLOSE can
 * never leave behind (tests).  The result is read with sbbseg_text_region_contours_read. */
int sbbseg_debug_mask_contours_dev(sbbseg_ctx* c, const void* d_mask_hw, int H, int W, int* n_contours, int64_t* n_points);
/* a contour whose bit map (box + ring, 32-bit words) exceeds `bytes` is traced on the label plane in global memory instead of LDS
 * (0 .. 65536, the default; tests lower it so that small planes reach the global form) */
int sbbseg_debug_set_contour_lds_limit(sbbseg_ctx* c, int bytes);
/* tracer + packing kernels the contour calls have queued on this handle so far */
int sbbseg_debug_contour_launches(sbbseg_ctx* c, int64_t* value);
/* sbbseg_mask_contours_host gives up after `steps` steps per contour instead of 8 x (box pixels) + 8 (0 restores that).  Process-global;
 * tests of the failure path only. */
int sbbseg_debug_set_contour_host_step_bound(int64_t steps);

/* ---- reading order of the text regions (order_of_regions / order_and_id_of_texts, main.py:1802-1906; csrc/order.h) ----
 * Contours: n lists of int (x, y) points, contour r = points point_off[r] .. point_off[r + 1] of points_xy (point_off[0] = 0).  The
 * repeated closing point of a ring adds zero terms: closed and unclosed lists give the same bits.  In the `_dev` calls points_xy = NULL
 * names the handle's resident contour result (sbbseg_text_region_contours_dev / sbbseg_debug_mask_contours_dev), read in place: n must
 * be its contour count and point_off is ignored.
 *
 * Moments: OpenCV's contourMoments for integer points [EXT: restated, unpinned] -- float64, serial, starting from the last point:
 * dxy = x' y - x y', a00 += dxy, a10 += dxy (x' + x), a01 += dxy (y' + y), every multiply and add rounded on its own; if
 * fabs(a00) > FLT_EPSILON, m00 = a00 * (s / 2), m10 = a10 * (s * 0.16666666666666666), m01 likewise (s = sign of a00), else all 0;
 * cx = m10 / (m00 + 1e-32), cy likewise.  moments [n][3] = m00, m10, m01; centroids [n][2] = cx, cy.  The device sums exact integers
 * with a wave scan where that is the float64 sum (coordinates below 32768 in magnitude, every prefix below 2^53) and redoes any other
 * contour serially in float64: serial [n] (optional) = 1 for those.  The host twin is the serial loop and reports the same flags.
 * n = 0 is success and needs no handle. */
int sbbseg_contour_moments_dev(sbbseg_ctx* c, const int32_t* points_xy, const int64_t* point_off, int n, double* moments, double* centroids,
                               int32_t* serial);
int sbbseg_contour_moments_host(const int32_t* points_xy, const int64_t* point_off, int n, double* moments, double* centroids, int32_t* serial);
/* The order.  plane: the textline plane, uint8 [H][W]; its rows are summed as stored (not `!= 0`).  weights: the 33 doubles of
 * scipy's half Gaussian kernel of sigma 8 (_gaussian_kernel1d(8, 0, 32)[32:]); the library does not reproduce libm.
 *   edges [cap], *n_edges: [0] + (find_peaks(gaussian_filter1d(zneg, 8), height=0) - 40) + [H]; cap >= (H + 80) / 2 + 2.  Edges below 0
 *     and at or above H occur and are not clamped.
 *   centroids [n][2]: cx, cy as above.  band [n]: the i with edges[i] <= cy < edges[i + 1] (at most one; exactly one for 0 <= cy < H), or -1.
 *   sorted_index [n]: the regions by (band, cx, index) -- the reference's list; cx ties [EXT: np.argsort's default sort is unstable] by
 *     ascending index; regions of band -1, which the reference leaves out, stand behind all others.  order [n]: the region's position in
 *     that list, -1 for band -1.
 * The region order is that of the contour list.  The plane may belong to another handle on the same device.  n = 0 is success (the edges
 * are still computed).  sbbseg_region_order_host takes the int32 row sums instead of the plane and needs no GPU. */
int sbbseg_region_order_dev(sbbseg_ctx* c, const void* d_plane_hw, int H, int W, const double* weights, const int32_t* points_xy,
                            const int64_t* point_off, int n, int32_t* sorted_index, int32_t* order, int32_t* band, double* centroids, int32_t* edges,
                            int cap, int* n_edges);
int sbbseg_region_order(sbbseg_ctx* c, const uint8_t* plane_hw, int H, int W, const double* weights, const int32_t* points_xy,
                        const int64_t* point_off, int n, int32_t* sorted_index, int32_t* order, int32_t* band, double* centroids, int32_t* edges,
                        int cap, int* n_edges);
int sbbseg_region_order_host(const int32_t* row_sums, int H, const double* weights, const int32_t* points_xy, const int64_t* point_off, int n,
                             int32_t* sorted_index, int32_t* order, int32_t* band, double* centroids, int32_t* edges, int cap, int* n_edges);
/* the row-sum kernel alone on a host plane (tests): row_sums int32 [H] */
int sbbseg_debug_row_sums(sbbseg_ctx* c, const uint8_t* plane_hw, int H, int W, int32_t* row_sums);
/* kernels the reading-order calls have queued on this handle so far (4 per order call with regions, 2 without) */
int sbbseg_debug_order_launches(sbbseg_ctx* c, int64_t* value);
/* sbbseg_profile_statistics_host / _dev behind one signature, with two more outputs (tests).  counts is a HOST array.  c = NULL: the serial
 * host twin.  A handle: the counts are uploaded and the product's kernels run through the product's launch.  Optional outputs: smooth = z of
 * every profile, packed like counts; below [n_regions][n_angles] = the level a deep minimum must lie below, mean(maxima > 10) * (1 - 1 /
 * multiplier) as the reference writes it, NaN without such maxima -- the only place where the ORDER of the compacted maxima shows. */
int sbbseg_debug_profile_statistics(sbbseg_ctx* c, const int32_t* counts, const int64_t* offsets, int n_regions, int n_angles, const double* weights,
                                    int radius, double multiplier, double* spread, uint8_t* state, int32_t* winner, double* smooth, double* below);
/* The statistic's own float64 divide (op 0: out[i] = a[i] / b[i]) and square root (op 1: out[i] = sqrt(a[i]), b unused), which claim IEEE
 * round-to-nearest-even for every class of operand (tests).  Host arrays of n <= 2^24 doubles.  c = NULL: on the host; a handle: one kernel. */
int sbbseg_debug_soft_arith(sbbseg_ctx* c, int op, const double* a, const double* b, int64_t n, double* out);
/* counters: which 0 = how often sbbseg_page_box_dev had to fall back to the host ranking on this handle */
int sbbseg_debug_counter(sbbseg_ctx* c, int which, int64_t* value);      /* which: 0 = exact host contour rankings, 1 = patches run through the plan, 2 = kernels queued by sbbseg_region_line_masks(_dev), sbbseg_region_line_boxes(_dev) and their sbbseg_planes_* forms, 3 = ingest + region-table + stitch kernels queued by sbbseg_segment_views_dev, 4 = ingest + label-resize kernels queued by the whole-views calls (sbbseg_segment_whole_views_dev, sbbseg_extract_page_boxes_dev, sbbseg_run_pages: 2 per chunk), 5 = kernels queued by the deskew slope sweeps (crop 2, profiles 1, statistic 1 or 2, winner 1 per sweep) */
/* Test hook for the no-abort guarantee: the nth_check-th next internal host-allocation checkpoint throws
 * std::bad_alloc, which every entry point turns into a non-zero status + sbbseg_last_error() instead of
 * terminating the process (main.py:2061-2157 relies on ordinary exceptions).  0 disarms.  Process-global. */
int sbbseg_debug_inject_alloc_failure(int nth_check);

/* ---- per-op timing with HIP events on the handle's stream (bench.py roofline) */
int sbbseg_profile_enable(sbbseg_ctx* c, int enable);
int sbbseg_profile_reset(sbbseg_ctx* c);
/* accumulated since reset: total ms and number of launches for op `op` */
int sbbseg_profile_get(sbbseg_ctx* c, int op, double* total_ms, int64_t* launches, int64_t* patches);
/* Work op `op` EXECUTED since sbbseg_profile_reset, in whole-patch equivalents: a launch over n patches counts n, an owned-region
 * launch n x (output pixels walked / output pixels of the whole grid).  exec_patches: every launch; timed_exec_patches: the launches
 * the profiling events timed (the denominator's counterpart of sbbseg_profile_get's total_ms).  Executed FLOPs of an op =
 * sbbseg_op_info's flops_per_patch x these. */
int sbbseg_op_executed(sbbseg_ctx* c, int op, double* exec_patches, double* timed_exec_patches);

#ifdef __cplusplus
}
#endif
#endif /* SBBSEG_H */
