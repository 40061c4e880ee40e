// api.hip -- host side of libsbbseg: the error and allocation plumbing every host unit uses (ctx.h), the handle's life cycle, setters and queries,
// seam 2 (sbbseg_predict), the device buffers handed to callers, and the debug entry points.  The rest of the C ABI declared in include/sbbseg.h:
// forward.hip (the forward pass over a plan), pages.hip (the tile and page paths), whole.hip (the whole-image branch, sbbseg_run_page(s)), comm.hip
// (the RCCL collective), plan_build.hip (plan building), stage_glue.hip (the stage glue) and contour_glue.hip (components and contours).  All of them sit on ctx.h; those that run a plan share exec.h.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "exec.h"

using namespace sbbseg;

namespace sbbseg {

thread_local std::string g_err;
thread_local int g_err_kind = kErrOther;
int g_alloc_fail_countdown = 0;

int set_error(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    g_err_kind = kErrOther;
    return 1;
}

// The two allocators behind a handle's registries (ctx.h: mem, pinned).  Nothing else in the library allocates or frees device or pinned memory.
static int hip_device_alloc(void** p, size_t bytes) { HIPCHK(hipMalloc(p, bytes)); return 0; }
static int hip_device_free(void* p) { HIPCHK(hipFree(p)); return 0; }
static int hip_pinned_alloc(void** p, size_t bytes) { HIPCHK(hipHostMalloc(p, bytes, hipHostMallocDefault)); return 0; }
static int hip_pinned_free(void* p) { HIPCHK(hipHostFree(p)); return 0; }

int dmalloc(sbbseg_ctx* c, void** p, size_t bytes) { return c->mem.alloc(p, bytes); }

int check_ready(sbbseg_ctx* c)
{
    REQUIRE(c != nullptr, "null handle");
    REQUIRE(c->finalized, "plan not finalized");
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

// a u8 label plane [pixels] on the device -> host memory, as one plane or as the three identical channels do_prediction returns
// (main.py:366; replicated on the device); queued on the handle's stream, the caller synchronises
int labels_to_host(sbbseg_ctx* c, const void* d_plane, void* host, size_t pixels, int channels)
{
    if (channels == 3) {
        if (ensure(c, c->page_labels3, (pixels + 3) / 4 * 12)) return 1;
        HIPCHK(launch_replicate3((const uint8_t*)d_plane, c->page_labels3.p, pixels, c->stream));
        HIPCHK(hipMemcpyAsync(host, c->page_labels3.p, pixels * 3, hipMemcpyDeviceToHost, c->stream));
    } else {
        HIPCHK(hipMemcpyAsync(host, d_plane, pixels, hipMemcpyDeviceToHost, c->stream));
    }
    return 0;
}

}  // namespace sbbseg

extern "C" {

const char* sbbseg_last_error(void) { return g_err.c_str(); }
int sbbseg_abi_version(void) { return SBBSEG_ABI_VERSION; }

int sbbseg_device_count(int* count)
{
    API_BEGIN
    REQUIRE(count, "null count");
    HIPCHK(hipGetDeviceCount(count));
    return 0;
    API_END
}

int sbbseg_create(int device, int precision, sbbseg_ctx** out)
{
    API_BEGIN
    REQUIRE(out, "null out");
    REQUIRE(precision == SBBSEG_PREC_BF16 || precision == SBBSEG_PREC_F32 || precision == SBBSEG_PREC_F16 || precision == SBBSEG_PREC_F16X3,
            "bad precision %d", precision);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    REQUIRE(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
            "libsbbseg is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
    sbbseg_ctx* c = new sbbseg_ctx(hip_device_alloc, hip_device_free, hip_pinned_alloc, hip_pinned_free);
    c->device = device;
    c->precision = precision;
    c->elem = precision == SBBSEG_PREC_F32 ? 4 : 2;
    c->planes = is_split(precision) ? 2 : 1;
    c->num_cus = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    // The second lane's stream is created in ANOTHER PRIORITY CLASS than the handle's own stream.  HIP multiplexes streams onto a few
    // hardware queues per priority class (GPU_MAX_HW_QUEUES, default 4, dealt round robin): when a handle's two streams land on the
    // same queue its lanes serialise behind each other's barrier packets -- measured 26.4 ms instead of 22.9 ms per 108-tile page on the
    // SECOND handle of a process (the fourth with 8 queues, none of five with 16: tools/handle_order_probe.py, profiles/r04_experiments.md
    // section 10); configs[2]'s layout stage was that handle.  Queues of different priority classes are never shared.
    // SBBSEG_LANE_PRIORITY: -1 (default) = the device's highest priority, 0 = same class as the own stream (the old behaviour), 1 = lowest
    {
        int least = 0, greatest = 0, want = -1;
        if (const char* v = getenv("SBBSEG_LANE_PRIORITY")) want = atoi(v);
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        const int prio = want < 0 ? greatest : want > 0 ? least : 0;
        e = prio != 0 ? hipStreamCreateWithPriority(&c->lane_stream, hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(&c->lane_stream, hipStreamNonBlocking);
        c->lane_prio = prio; c->prio_least = least; c->prio_greatest = greatest;
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) {
        sbbseg_destroy(c);
        return set_error("lane stream/event creation failed: %s", hipGetErrorString(e));
    }
    if (const char* v = getenv("SBBSEG_DEDUPE")) c->dedupe = v[0] != '0';
    if (const char* v = getenv("SBBSEG_KSPLIT")) c->ksplit = v[0] != '0';
    if (const char* v = getenv("SBBSEG_OWNED_REGIONS")) c->owned_mode = v[0] == '0' ? 0 : (v[0] == '2' ? 2 : 1);
    *out = c;
    return 0;
    API_END
}

int sbbseg_destroy(sbbseg_ctx* c)
{
    API_BEGIN
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->lane_stream) (void)hipStreamSynchronize(c->lane_stream);
    (void)c->mem.release_all();
    (void)c->pinned.release_all();
    if (c->ev_views) (void)hipEventDestroy(c->ev_views);
    for (int k = 0; k < 2; ++k) {
        if (c->pp_in[k]) (void)hipEventDestroy(c->pp_in[k]);
        if (c->pp_comp[k]) (void)hipEventDestroy(c->pp_comp[k]);
        if (c->pp_out[k]) (void)hipEventDestroy(c->pp_out[k]);
    }
    comm_release(c);
    if (c->copy_in) (void)hipStreamDestroy(c->copy_in);
    if (c->copy_out) (void)hipStreamDestroy(c->copy_out);
    for (auto& pe : c->pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto e : c->free_events) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->lane_stream) (void)hipStreamDestroy(c->lane_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    delete c;
    return 0;
    API_END
}

int sbbseg_set_stream(sbbseg_ctx* c, void* hip_stream)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (resolve_pending(c)) return 1;
    // NULL is a real stream (the legacy default stream torch uses unless told otherwise)
    c->stream = hip_stream == SBBSEG_OWN_STREAM ? c->own_stream : (hipStream_t)hip_stream;
    // a caller's stream of the lane stream's own priority class could share its hardware queue (see sbbseg_create): move the lane
    // stream to the other end of the range
    int up = 0;
    if (hip_stream != SBBSEG_OWN_STREAM && hip_stream && c->lane_prio != 0 && c->prio_least != c->prio_greatest &&
        hipStreamGetPriority((hipStream_t)hip_stream, &up) == hipSuccess && up == c->lane_prio) {
        const int other = c->lane_prio == c->prio_greatest ? c->prio_least : c->prio_greatest;
        hipStream_t ns = nullptr;
        if (other != 0 && hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, other) == hipSuccess) {
            HIPCHK(hipStreamSynchronize(c->lane_stream));
            HIPCHK(hipStreamDestroy(c->lane_stream));
            c->lane_stream = ns;
            c->lane_prio = other;
        } else (void)hipGetLastError();
    }
    return 0;
    API_END
}

int sbbseg_set_lanes(sbbseg_ctx* c, int lanes)
{
    API_BEGIN
    REQUIRE(c && (lanes == 1 || lanes == 2), "lanes must be 1 or 2");
    REQUIRE(!(c->finalized && lanes == 2 && c->lane1_batch == 0), "the second lane was not allocated at finalize (lanes was 1 or max_batch < 16)");
    c->lanes = lanes;
    return 0;
    API_END
}

int sbbseg_set_label_channels(sbbseg_ctx* c, int channels)
{
    API_BEGIN
    REQUIRE(c && (channels == 1 || channels == 3), "label channels must be 1 or 3");
    c->label_channels = channels;
    return 0;
    API_END
}

int sbbseg_set_dedupe(sbbseg_ctx* c, int on)
{
    API_BEGIN
    REQUIRE(c && (on == 0 || on == 1), "dedupe must be 0 or 1");
    c->dedupe = on != 0;
    return 0;
    API_END
}

int sbbseg_set_owned_regions(sbbseg_ctx* c, int mode)
{
    API_BEGIN
    REQUIRE(c && mode >= 0 && mode <= 2, "mode: 0 = off, 1 = fused page paths, 2 = tile-range entry points too");
    c->owned_mode = mode;
    return 0;
    API_END
}

int sbbseg_owned_region_info(sbbseg_ctx* c, int* mode, int* levels)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (mode) *mode = c->owned_mode;
    if (levels) *levels = c->finalized ? c->region_levels : 0;
    return 0;
    API_END
}

int sbbseg_debug_poison_activations(sbbseg_ctx* c, int byte_value)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    HIPCHK(hipDeviceSynchronize());
    for (auto& t : c->tensors) {
        if (t.is_input_form) continue;                     // (their zero borders are part of the form)
        for (int lane = 0; lane < 2; ++lane) {
            if (!t.lane_buf[lane]) continue;
            const size_t n = t.elems_per_patch * (size_t)(lane == 0 ? c->max_batch : c->lane1_batch) * c->elem * c->planes;
            HIPCHK(hipMemset(t.lane_buf[lane] + kZeroHeaderBytes, byte_value & 255, n));
        }
    }
    if (c->tile_labels.p) HIPCHK(hipMemset(c->tile_labels.p, byte_value & 255, c->tile_labels.cap));
    // the split-K partial sums too: a split that a later pass does not write must not find the last pass's (equal) value there
    if (c->ks_ws.p) HIPCHK(hipMemset(c->ks_ws.p, byte_value & 255, c->ks_ws.cap));
    HIPCHK(hipDeviceSynchronize());
    return 0;
    API_END
}

int sbbseg_set_ksplit(sbbseg_ctx* c, int on)
{
    API_BEGIN
    REQUIRE(c && (on == 0 || on == 1), "ksplit must be 0 or 1");
    c->ksplit = on != 0;
    return 0;
    API_END
}

int sbbseg_synchronize(sbbseg_ctx* c)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

// ----------------------------------------------------------------------------------------- queries
int sbbseg_model_info(sbbseg_ctx* c, int* H, int* W, int* classes, int* max_batch)
{
    API_BEGIN
    REQUIRE(c, "null handle");
    if (H) *H = c->in_H;
    if (W) *W = c->in_W;
    if (classes) *classes = c->classes;
    if (max_batch) *max_batch = c->max_batch;
    return 0;
    API_END
}

int sbbseg_num_ops(sbbseg_ctx* c, int* n)
{
    API_BEGIN
    REQUIRE(c && n, "bad arguments");
    *n = (int)c->ops.size();
    return 0;
    API_END
}

int sbbseg_op_info(sbbseg_ctx* c, int op, char* name, int name_len, double* flops_per_patch, double* min_bytes_per_patch)
{
    API_BEGIN
    REQUIRE(c && op >= 0 && op < (int)c->ops.size(), "op index out of range");
    if (name && name_len > 0) snprintf(name, name_len, "%s", c->ops[op].name.c_str());
    if (flops_per_patch) *flops_per_patch = c->ops[op].flops;
    if (min_bytes_per_patch) *min_bytes_per_patch = c->ops[op].min_bytes;
    return 0;
    API_END
}

int sbbseg_op_issued_flops(sbbseg_ctx* c, int op, double* issued_flops_per_patch)
{
    API_BEGIN
    REQUIRE(c && op >= 0 && op < (int)c->ops.size() && issued_flops_per_patch, "op index out of range");
    *issued_flops_per_patch = c->ops[op].issued_flops;
    return 0;
    API_END
}

int sbbseg_device_bytes(sbbseg_ctx* c, size_t* bytes)
{
    API_BEGIN
    REQUIRE(c && bytes, "bad arguments");
    *bytes = c->mem.bytes();
    return 0;
    API_END
}

// -------------------------------------------------------------------------------------- seam 2
int sbbseg_predict(sbbseg_ctx* c, const float* x_nhwc, int n, float* probs_nhwc)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(x_nhwc && probs_nhwc && n >= 0, "bad arguments");
    const size_t per_in = (size_t)c->in_H * c->in_W * 3, per_out = (size_t)c->in_H * c->in_W * c->classes;
    if (!c->d_xin && dmalloc(c, (void**)&c->d_xin, per_in * c->max_batch * sizeof(float))) return 1;
    if (!c->d_probs && dmalloc(c, (void**)&c->d_probs, per_out * c->max_batch * sizeof(float))) return 1;
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    for (int done = 0; done < n; done += c->max_batch) {
        const int nb = n - done < c->max_batch ? n - done : c->max_batch;
        HIPCHK(hipMemcpyAsync(c->d_xin, x_nhwc + done * per_in, per_in * nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_ingest_f32(c->d_xin, nb, c->in_H, c->in_W, ip.c8, ip.pairs, ip.pad, ip.pairs_w, c->precision, c->stream));
        if (run_plan(c, nb, c->d_batch_labels, c->d_probs)) return 1;
        HIPCHK(hipMemcpyAsync(probs_nhwc + done * per_out, c->d_probs, per_out * nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
    API_END
}

// ---- device buffers for callers that have no device runtime of their own (the reference's environment is Keras/TF, not PyTorch):
// what run() keeps resident across its three stages -- the stored page, the border mask, the region map, the textline map -- lives in
// buffers the library hands out.  They belong to the handle that allocated them (sbbseg_destroy frees what is left) but any handle of
// the same device may read and write them.
int sbbseg_device_alloc(sbbseg_ctx* c, size_t bytes, void** d_ptr)
{
    API_BEGIN
    REQUIRE(c != nullptr && d_ptr != nullptr && bytes > 0, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    alloc_check();
    return c->mem.alloc(d_ptr, bytes, /*user=*/true);
    API_END
}

int sbbseg_device_free(sbbseg_ctx* c, void* d_ptr)
{
    API_BEGIN
    REQUIRE(c != nullptr, "null handle");
    if (!d_ptr) return 0;
    const DeviceMem::Block* b = c->mem.find(d_ptr);
    REQUIRE(b && b->user, "sbbseg_device_free: %p was not allocated by this handle", d_ptr);      // (its own blocks are not the caller's to free)
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());                    // DEVICE-wide on purpose: any handle on the device may use the buffer (sbbseg.h), so
                                                       // other handles' streams may still be reading it; a free is not a hot-path call
    return c->mem.release(d_ptr) ? 1 : 0;
    API_END
}

// host -> device / device -> host on the handle's stream; both return when the copy is complete, so the buffer may be handed to
// another handle (another stream) right away.
int sbbseg_upload(sbbseg_ctx* c, void* d_dst, const void* src, size_t bytes)
{
    API_BEGIN
    REQUIRE(c != nullptr && d_dst && src, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

int sbbseg_download(sbbseg_ctx* c, void* dst, const void* d_src, size_t bytes)
{
    API_BEGIN
    REQUIRE(c != nullptr && dst && d_src, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

// labels_to_host for the caller's buffers (sbbseg_set_label_channels is not consulted); returns when the labels have arrived
int sbbseg_download_labels(sbbseg_ctx* c, uint8_t* dst, const void* d_labels_hw, size_t pixels, int channels)
{
    API_BEGIN
    REQUIRE(c != nullptr && dst && d_labels_hw && pixels > 0 && (channels == 1 || channels == 3), "bad arguments (channels: 1 or 3)");
    HIPCHK(hipSetDevice(c->device));
    if (labels_to_host(c, d_labels_hw, dst, pixels, channels)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
    API_END
}

// ----------------------------------------------------------------------------------------- debug
// n stored elements of tensor t (of the lane in use) -> n floats in host memory, through a temporary of the handle; returns when they are there
static int tensor_to_host_f32(sbbseg_ctx* c, const Tensor& t, size_t n, float* out)
{
    ScopedBlock<float> tmp(c->mem);
    if (tmp.alloc(n)) return 1;
    HIPCHK(c->planes == 2 ? launch_split_to_f32(t.data(), tmp.p, n / t.C, t.C, c->stream) : launch_to_f32(t.data(), tmp.p, n, c->precision, c->stream));
    HIPCHK(hipMemcpyAsync(out, tmp.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->planes == 2 && t.is_input_form && t.form == SBBSEG_INPUT_C8)      // (the hi plane's slots 4..6 repeat lo(ch 0..2) for the fused tail: not channels)
        for (size_t i = 0; i < n; i += 8)
            for (int ch = 3; ch < 8; ++ch) out[i + ch] = 0.f;
    return 0;
}

int sbbseg_debug_ingest(sbbseg_ctx* c, const uint8_t* page_hwc, int Hp, int Wp, const int32_t* tile_xy, int n_tiles,
                        int form, float* out, size_t out_floats)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(page_hwc && tile_xy && out && n_tiles >= 1 && n_tiles <= c->max_batch, "bad arguments (n_tiles <= max_batch)");
    REQUIRE(form == SBBSEG_INPUT_C8 || form == SBBSEG_INPUT_PAIRS, "unknown form");
    REQUIRE(c->form_tensor[form] >= 0, "plan does not use input form %d", form);
    const Tensor& t = c->tensors[c->form_tensor[form]];
    const size_t n = t.elems_per_patch * n_tiles;
    REQUIRE(out_floats >= n, "output buffer too small (%zu < %zu)", out_floats, n);
    const size_t pix = (size_t)Hp * Wp;
    if (ensure(c, c->page, pix * 3)) return 1;
    HIPCHK(hipMemcpyAsync(c->page.p, page_hwc, pix * 3, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(c->d_tile_xy, tile_xy, sizeof(int) * 2 * n_tiles, hipMemcpyHostToDevice));
    IngestParams ip;
    if (fill_ingest(c, ip)) return 1;
    ip.page = c->page.p; ip.Hp = Hp; ip.Wp = Wp; ip.src_Hp = Hp; ip.src_Wp = Wp; ip.tile_xy = c->d_tile_xy; ip.n_tiles = n_tiles;
    HIPCHK(launch_ingest_u8(ip, c->precision, c->stream));
    return tensor_to_host_f32(c, t, n, out);
    API_END
}

int sbbseg_debug_read_tensor(sbbseg_ctx* c, int tensor_id, int n, float* out, size_t out_floats)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(tensor_id >= 0 && tensor_id < (int)c->tensors.size() && out && n >= 1 && n <= c->max_batch, "bad arguments");
    const Tensor& t = c->tensors[tensor_id];
    const size_t cnt = t.elems_per_patch * n;
    REQUIRE(out_floats >= cnt, "output buffer too small (%zu < %zu)", out_floats, cnt);
    return tensor_to_host_f32(c, t, cnt, out);
    API_END
}

int sbbseg_debug_op_launch(sbbseg_ctx* c, int op, int32_t* out, int cap)
{
    API_BEGIN
    REQUIRE(c && out && cap >= 0 && op >= 0 && op < (int)c->ops.size(), "op index out of range");
    const LaunchRec& r = c->ops[op].last;
    const int rec[kLaunchRecInts] = {r.family, r.bp, r.bc, r.stages, r.fast_gather, r.tile_map, r.cls_minor, r.table, r.n_tiles, r.grid,
                                     r.res_epilogue, r.persistent, r.residual};
    static_assert(kLaunchRecInts == SBBSEG_LAUNCH_INTS, "sbbseg.h documents the record");
    for (int i = 0; i < cap && i < kLaunchRecInts; ++i) out[i] = rec[i];
    return 0;
    API_END
}

int sbbseg_debug_tensor_period_mismatches(sbbseg_ctx* c, int tensor_id, int n, int period, int64_t* count, int64_t* first)
{
    API_BEGIN
    if (check_ready(c)) return 1;
    REQUIRE(tensor_id >= 0 && tensor_id < (int)c->tensors.size() && count && first && period >= 1 && n >= period && n <= c->max_batch, "bad arguments");
    const Tensor& t = c->tensors[tensor_id];
    const size_t stride = t.elems_per_patch * (size_t)c->elem * c->planes;          // bytes of one stored patch
    REQUIRE(stride % 16 == 0, "patch stride %zu is not a multiple of 16 bytes", stride);
    unsigned long long h_res[2] = {0ull, ~0ull};
    ScopedBlock<unsigned long long> res(c->mem);
    if (res.alloc(2)) return 1;
    HIPCHK(hipMemcpyAsync(res.p, h_res, sizeof(h_res), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_period_mismatches(t.data(), stride * period, stride * (size_t)(n - period), res.p, c->num_cus, c->stream));
    HIPCHK(hipMemcpyAsync(h_res, res.p, sizeof(h_res), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *count = (int64_t)h_res[0];
    *first = h_res[0] ? (int64_t)h_res[1] : -1;
    return 0;
    API_END
}

int sbbseg_debug_inject_alloc_failure(int nth_check)
{
    API_BEGIN
    REQUIRE(nth_check >= 0, "nth_check must be >= 0 (0 disarms)");
    g_alloc_fail_countdown = nth_check;
    return 0;
    API_END
}

int sbbseg_debug_counter(sbbseg_ctx* c, int which, int64_t* value)
{
    API_BEGIN
    REQUIRE(c && value && which >= 0 && which <= 5, "unknown counter %d (0 = exact host contour rankings, 1 = patches run through the plan, 2 = kernels queued by the line-mask calls, 3 = ingest / region-table / stitch kernels queued by sbbseg_segment_views_dev, 4 = ingest / label-resize kernels queued by the whole-views calls, 5 = kernels queued by the deskew slope sweeps)", which);
    *value = which == 0 ? (int64_t)c->host_contour_calls : which == 1 ? (int64_t)c->forwards : which == 2 ? (int64_t)c->line_launches : which == 3 ? c->views_launches : which == 4 ? c->whole_launches : (int64_t)c->slope_launches;
    return 0;
    API_END
}

int sbbseg_debug_set_conv_variant(sbbseg_ctx* c, int variant)
{
    API_BEGIN
    REQUIRE(c && variant >= 0 && variant <= 0x7ffffff, "variant: bits 0-1 = 0 auto | 1 4-wave/2-stage | 2 8-wave/3-stage; bit 2 = one block per tile (non-persistent); bit 3 = no XCD-grouped tile walk; bit 4 = half-K-step stages; bit 5 = XCD-grouped walk on single-class layers; bit 6 = drain epilogue stores; bit 7 = half-line epilogue stores; bits 8-15 = contiguous-run K limit / 64; bit 16 = 8-phase schedule on the 256x256 tile; bit 17 = plain gather everywhere; bit 18 = fused bottleneck blocks run as their three convs; bit 19 = XCD-contiguous walk for grouped launches; bit 20 = one-group form of the fused block kernel; bit 21 = extract_page ranks contours on the host always; bit 22 = stem and max-pool as two launches; bit 23 = the 224 x 224 decoder conv on the generic kernel; bit 24 = expand + next reduce 1x1 convs as two launches; bit 25 = the 3x3 conv of a stage-3 identity block as its own launch; bit 26 = fused 16-bit bottleneck blocks also store a and b (nothing in the split mode: block_x3 stays held by bit-identity to its three convs)");
    c->conv_variant = variant & 0xff;
    c->ph8 = (variant >> 16) & 1;
    c->plain_gather = (variant >> 17) & 1;
    c->unfuse_blocks = (variant >> 18) & 1;
    c->ranged_walk = (variant >> 19) & 1;
    c->block_pq = !((variant >> 20) & 1);
    c->force_host_contours = (variant >> 21) & 1;
    c->unfuse_stem_pool = (variant >> 22) & 1;
    c->no_dec_halo = (variant >> 23) & 1;
    c->no_expand_reduce = (variant >> 24) & 1;
    c->no_c3er = (variant >> 25) & 1;
    c->dump_blocks = (variant >> 26) & 1;
    if ((variant >> 8) & 0xff) c->contig_max_k = ((variant >> 8) & 0xff) * 64;
    return 0;
    API_END
}

}  // extern "C"
