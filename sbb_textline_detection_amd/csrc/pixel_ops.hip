// pixel_ops.hip -- the HBM-bound per-pixel kernels around the convs: ingest (u8 page / f32 batch -> both network-input forms), max-pool,
// the 1x1 head, the page stitch, label resize, and the conversions of stored tensors back to f32 / three channels.
#include "device_prims.h"
#include "region.h"

namespace sbbseg {

// ------------------------------------------------------------------------------------------------
// element helpers for the HBM-bound kernels (E = uint16_t bf16 bits | float)
// ------------------------------------------------------------------------------------------------
template <typename E> __device__ inline E to_elem(float v);
template <> __device__ inline uint16_t to_elem<uint16_t>(float v) { return bf16_bits_rne(v); }
template <> __device__ inline float to_elem<float>(float v) { return v; }
template <> __device__ inline _Float16 to_elem<_Float16>(float v) { return (_Float16)fminf(fmaxf(v, -65504.f), 65504.f); }
template <typename E> __device__ inline float from_elem(E v);
template <> __device__ inline float from_elem<uint16_t>(uint16_t v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }
template <> __device__ inline float from_elem<float>(float v) { return v; }
template <> __device__ inline float from_elem<_Float16>(_Float16 v) { return (float)v; }

template <typename E> struct alignas(16) Vec8 { E v[8]; };
template <typename E> struct alignas(sizeof(E) * 4) Vec4 { E v[4]; };

// split-mode writer of one network-input pixel into both input forms (see ingest_u8_kernel)
template <typename E>
__device__ inline void write_split_input(const float (&f)[3], void* c8, void* pairs, long idx, int t, int y, int x,
                                         int H, int pad, int pairs_w)
{
    _Float16 hi[3], lo[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) split_f32(f[i], hi[i], lo[i]);
    const _Float16 z = (_Float16)0.f;
    Vec8<_Float16> oh, ol;
#pragma unroll
    for (int i = 0; i < 8; ++i) { oh.v[i] = i < 3 ? hi[i] : z; ol.v[i] = i < 3 ? lo[i] : z; }
    // The channel slots 4..6 of the hi plane repeat lo(ch 0..2): every kernel that treats the form as an 8-channel tensor multiplies
    // them by zero weights (channels 3..7 do not exist), dec_tail_fused_x3ps reads the first granule as [h0 h1 h2 0 | l0 l1 l2 0]
#pragma unroll
    for (int i = 0; i < 3; ++i) oh.v[4 + i] = lo[i];
    ((Vec8<_Float16>*)c8)[2 * idx] = oh;
    ((Vec8<_Float16>*)c8)[2 * idx + 1] = ol;
    if (pairs) {
        const int PH = H + 2 * pad;
        const int xp = x + pad;
        _Float16* dst = (_Float16*)pairs + (((size_t)t * PH + (y + pad)) * pairs_w + (xp >> 1)) * 16 + (xp & 1) * 4;
        Vec4<_Float16> qh, ql;
        qh.v[0] = hi[0]; qh.v[1] = hi[1]; qh.v[2] = hi[2]; qh.v[3] = z;
        ql.v[0] = lo[0]; ql.v[1] = lo[1]; ql.v[2] = lo[2]; ql.v[3] = z;
        *(Vec4<_Float16>*)dst = qh;
        *(Vec4<_Float16>*)(dst + 8) = ql;
    }
}

// ------------------------------------------------------------------------------------------------
// ingest: u8 page -> normalised network input in both forms (main.py:239 `img / 255.0`, 285 slice)
// one thread per (tile, y, x)
// ------------------------------------------------------------------------------------------------
// SPLIT (kF16X3): every stored element is an fp16 (hi, lo) pair -- C8 pixel = [8 hi][8 lo] (32 bytes; hi slots 4..6 = lo 0..2), PAIRS
// granule = [2 px x 4 hi][2 px x 4 lo] (32 bytes); f32(v / 255.0) is carried to ~22 bits
template <typename E, bool SPLIT = false>
__global__ __launch_bounds__(256) void ingest_u8_kernel(const IngestParams p)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)p.H * p.W;
    if (idx >= per * p.n_tiles) return;
    const int t = (int)(idx / per);
    const int rem = (int)(idx - t * per);
    const int y = rem / p.W, x = rem - y * p.W;
    int vy, vx;                                   // position on the (virtual) page
    if (p.whole) { vy = y; vx = x; }
    else if (p.tile_xy) { vx = p.tile_xy[2 * t] + x; vy = p.tile_xy[2 * t + 1] + y; }
    else {
        const int gt = p.grid_first + t;
        const int gi = gt / p.grid_nyf, gj = gt - gi * p.grid_nyf;
        vx = min(gi * p.grid_mid_x, p.Wp - p.W) + x;
        vy = min(gj * p.grid_mid_y, p.Hp - p.H) + y;
    }
    // optional nearest-neighbour rescale (cv2.INTER_NEAREST index tables): the rescaled page of
    // get_image_and_scales (main.py:196-214) / the resize of the whole-image branch (main.py:371)
    // is never materialised, the tiles are gathered straight from the stored page
    const int sy = p.map_y ? p.map_y[vy] : vy, sx = p.map_x ? p.map_x[vx] : vx;
    const uint8_t* px = p.page + ((size_t)sy * p.src_Wp + sx) * 3;
    E v0, v1, v2;
    if (p.bin_thr) {
        // otsu_copy + astype(uint8) + /255 (main.py:178-194, 443-444, 239): channel 0 binarised at the
        // page's Otsu threshold lands in all three channels (reference quirk, lines 191-193): 0.0 or 1.0
        v0 = v1 = v2 = to_elem<E>((int)px[0] > *p.bin_thr ? 1.f : 0.f);
    } else {
        v0 = to_elem<E>(p.lut[px[0]]); v1 = to_elem<E>(p.lut[px[1]]); v2 = to_elem<E>(p.lut[px[2]]);
    }
    const E z = to_elem<E>(0.f);
    if constexpr (SPLIT) {
        float f[3];
        if (p.bin_thr) f[0] = f[1] = f[2] = (int)px[0] > *p.bin_thr ? 1.f : 0.f;
        else { f[0] = p.lut[px[0]]; f[1] = p.lut[px[1]]; f[2] = p.lut[px[2]]; }
        write_split_input<E>(f, p.c8, p.pairs, idx, t, y, x, p.H, p.pad, p.pairs_w);
        return;
    }
    Vec8<E> o;
    o.v[0] = v0; o.v[1] = v1; o.v[2] = v2;
#pragma unroll
    for (int i = 3; i < 8; ++i) o.v[i] = z;
    ((Vec8<E>*)p.c8)[idx] = o;
    if (p.pairs) {
        const int PH = p.H + 2 * p.pad;
        const int xp = x + p.pad;
        E* dst = (E*)p.pairs + (((size_t)t * PH + (y + p.pad)) * p.pairs_w + (xp >> 1)) * 8 + (xp & 1) * 4;
        Vec4<E> q; q.v[0] = v0; q.v[1] = v1; q.v[2] = v2; q.v[3] = z;
        *(Vec4<E>*)dst = q;
    }
}

template <typename E, bool SPLIT = false>
__global__ __launch_bounds__(256) void ingest_f32_kernel(const float* x, int n, int H, int W, void* c8,
                                                         void* pairs, int pad, int pairs_w)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)H * W;
    if (idx >= per * n) return;
    const int t = (int)(idx / per);
    const int rem = (int)(idx - t * per);
    const int y = rem / W, xx = rem - y * W;
    const float* px = x + idx * 3;
    if constexpr (SPLIT) {
        const float f[3] = {px[0], px[1], px[2]};
        write_split_input<E>(f, c8, pairs, idx, t, y, xx, H, pad, pairs_w);
        return;
    }
    const E v0 = to_elem<E>(px[0]), v1 = to_elem<E>(px[1]), v2 = to_elem<E>(px[2]);
    const E z = to_elem<E>(0.f);
    Vec8<E> o;
    o.v[0] = v0; o.v[1] = v1; o.v[2] = v2;
#pragma unroll
    for (int i = 3; i < 8; ++i) o.v[i] = z;
    ((Vec8<E>*)c8)[idx] = o;
    if (pairs) {
        const int PH = H + 2 * pad;
        const int xp = xx + pad;
        E* dst = (E*)pairs + (((size_t)t * PH + (y + pad)) * pairs_w + (xp >> 1)) * 8 + (xp & 1) * 4;
        Vec4<E> q; q.v[0] = v0; q.v[1] = v1; q.v[2] = v2; q.v[3] = z;
        *(Vec4<E>*)dst = q;
    }
}

hipError_t launch_ingest_u8(const IngestParams& p, int precision, hipStream_t s)
{
    const long total = (long)p.H * p.W * p.n_tiles;
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (precision == kF32) hipLaunchKernelGGL(ingest_u8_kernel<float>, dim3(grid), dim3(256), 0, s, p);
    else if (precision == kF16X3) hipLaunchKernelGGL((ingest_u8_kernel<_Float16, true>), dim3(grid), dim3(256), 0, s, p);
    else if (precision == kF16) hipLaunchKernelGGL(ingest_u8_kernel<_Float16>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(ingest_u8_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// ingest of a chunk that pools tiles of several views (sbbseg_segment_views_dev): blockIdx.y = tile of the chunk, so the view
// (binary search of the pooled tile index in the views' first tiles) and the tile origin are uniform over the block; the pixel then goes
// through exactly what ingest_u8_kernel does in grid mode -- nearest maps, the LUT or the binarise rule, both input forms.
// ------------------------------------------------------------------------------------------------
template <typename E, bool SPLIT = false>
__global__ __launch_bounds__(256) void ingest_views_kernel(const IngestViewsParams p)
{
    const int t = blockIdx.y;
    const int rem = blockIdx.x * 256 + threadIdx.x;
    if (rem >= p.H * p.W) return;
    const unsigned gt = (unsigned)(p.g0 + t);
    const ViewRec& v = p.views[view_find(p.n_views, gt, [&](int m) { return (unsigned)p.views[m].first; })];
    const int local = (int)gt - v.first;
    const int gi = local / v.ny, gj = local - gi * v.ny;
    const int y = rem / p.W, x = rem - y * p.W;
    const int vx = min(gi * (p.W - 2 * p.margin), v.cw - p.W) + x;
    const int vy = min(gj * (p.H - 2 * p.margin), v.ch - p.H) + y;
    const int sy = v.mapped ? p.maps[v.my + vy] : v.my + vy, sx = v.mapped ? p.maps[v.mx + vx] : v.mx + vx;
    const uint8_t* px = v.page + ((size_t)sy * v.src_Wp + sx) * 3;
    const long idx = (long)t * (p.H * p.W) + rem;
    float f[3];
    if (v.thr) f[0] = f[1] = f[2] = (int)px[0] > *v.thr ? 1.f : 0.f;      // (otsu_copy: channel 0 into all three, see ingest_u8_kernel)
    else { f[0] = p.lut[px[0]]; f[1] = p.lut[px[1]]; f[2] = p.lut[px[2]]; }
    if constexpr (SPLIT) {
        write_split_input<E>(f, p.c8, p.pairs, idx, t, y, x, p.H, p.pad, p.pairs_w);
        return;
    }
    const E v0 = to_elem<E>(f[0]), v1 = to_elem<E>(f[1]), v2 = to_elem<E>(f[2]), z = to_elem<E>(0.f);
    Vec8<E> o;
    o.v[0] = v0; o.v[1] = v1; o.v[2] = v2;
#pragma unroll
    for (int i = 3; i < 8; ++i) o.v[i] = z;
    ((Vec8<E>*)p.c8)[idx] = o;
    if (p.pairs) {
        const int PH = p.H + 2 * p.pad;
        const int xp = x + p.pad;
        E* dst = (E*)p.pairs + (((size_t)t * PH + (y + p.pad)) * p.pairs_w + (xp >> 1)) * 8 + (xp & 1) * 4;
        Vec4<E> q; q.v[0] = v0; q.v[1] = v1; q.v[2] = v2; q.v[3] = z;
        *(Vec4<E>*)dst = q;
    }
}

hipError_t launch_ingest_views(const IngestViewsParams& p, int precision, hipStream_t s)
{
    if (p.n_tiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.H * p.W + 255) / 256), (unsigned)p.n_tiles);
    if (precision == kF32) hipLaunchKernelGGL(ingest_views_kernel<float>, grid, dim3(256), 0, s, p);
    else if (precision == kF16X3) hipLaunchKernelGGL((ingest_views_kernel<_Float16, true>), grid, dim3(256), 0, s, p);
    else if (precision == kF16) hipLaunchKernelGGL(ingest_views_kernel<_Float16>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(ingest_views_kernel<uint16_t>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// ingest of a chunk of the whole-image branch for many pages (sbbseg_segment_whole_views_dev): blockIdx.y = patch of the chunk = one view,
// so the view's record is uniform over the block (the compiler fetches it through the scalar cache); the pixel goes through the view's two
// composed nearest maps (model row -> page row -> stored row), then through what ingest_u8_kernel does in whole mode -- the LUT, both forms.
// ------------------------------------------------------------------------------------------------
template <typename E, bool SPLIT = false>
__global__ __launch_bounds__(256) void ingest_whole_views_kernel(const IngestWholeViewsParams p)
{
    const int t = blockIdx.y;
    const int rem = blockIdx.x * 256 + threadIdx.x;
    if (rem >= p.H * p.W) return;
    const WholeViewRec& v = p.views[t];
    const int y = rem / p.W, x = rem - y * p.W;
    const int sy = p.maps[v.my + y], sx = p.maps[v.mx + x];
    const uint8_t* px = v.page + ((size_t)sy * v.stored_w + sx) * 3;
    const long idx = (long)t * (p.H * p.W) + rem;
    const float f[3] = {p.lut[px[0]], p.lut[px[1]], p.lut[px[2]]};
    if constexpr (SPLIT) {
        write_split_input<E>(f, p.c8, p.pairs, idx, t, y, x, p.H, p.pad, p.pairs_w);
        return;
    }
    const E v0 = to_elem<E>(f[0]), v1 = to_elem<E>(f[1]), v2 = to_elem<E>(f[2]), z = to_elem<E>(0.f);
    Vec8<E> o;
    o.v[0] = v0; o.v[1] = v1; o.v[2] = v2;
#pragma unroll
    for (int i = 3; i < 8; ++i) o.v[i] = z;
    ((Vec8<E>*)p.c8)[idx] = o;
    if (p.pairs) {
        const int PH = p.H + 2 * p.pad;
        const int xp = x + p.pad;
        E* dst = (E*)p.pairs + (((size_t)t * PH + (y + p.pad)) * p.pairs_w + (xp >> 1)) * 8 + (xp & 1) * 4;
        Vec4<E> q; q.v[0] = v0; q.v[1] = v1; q.v[2] = v2; q.v[3] = z;
        *(Vec4<E>*)dst = q;
    }
}

hipError_t launch_ingest_whole_views(const IngestWholeViewsParams& p, int precision, hipStream_t s)
{
    if (p.n_views <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.H * p.W + 255) / 256), (unsigned)p.n_views);
    if (precision == kF32) hipLaunchKernelGGL(ingest_whole_views_kernel<float>, grid, dim3(256), 0, s, p);
    else if (precision == kF16X3) hipLaunchKernelGGL((ingest_whole_views_kernel<_Float16, true>), grid, dim3(256), 0, s, p);
    else if (precision == kF16) hipLaunchKernelGGL(ingest_whole_views_kernel<_Float16>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(ingest_whole_views_kernel<uint16_t>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ingest_f32(const float* x, int n, int H, int W, void* c8, void* pairs, int pad,
                             int pairs_w, int precision, hipStream_t s)
{
    const long total = (long)H * W * n;
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (precision == kF32)
        hipLaunchKernelGGL(ingest_f32_kernel<float>, dim3(grid), dim3(256), 0, s, x, n, H, W, c8, pairs, pad, pairs_w);
    else if (precision == kF16X3)
        hipLaunchKernelGGL((ingest_f32_kernel<_Float16, true>), dim3(grid), dim3(256), 0, s, x, n, H, W, c8, pairs, pad, pairs_w);
    else if (precision == kF16)
        hipLaunchKernelGGL(ingest_f32_kernel<_Float16>, dim3(grid), dim3(256), 0, s, x, n, H, W, c8, pairs, pad, pairs_w);
    else
        hipLaunchKernelGGL(ingest_f32_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, x, n, H, W, c8, pairs, pad, pairs_w);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// max-pool (valid), NHWC, one thread per (pixel, 8-channel granule)
// ------------------------------------------------------------------------------------------------
// optional per-channel affine + ReLU applied to every input element before the max: lets the stem
// write only its pre-BN tensor (the f1 skip) and the pool apply bn_conv1 + relu on the fly
// SPLIT (kF16X3): pixels are channel groups [G hi][G lo] (internal.h); values are re-assembled in fp32 (exact), the maximum is split again
template <typename E, bool SPLIT = false>
__global__ __launch_bounds__(256) void maxpool_kernel(const E* src, E* dst, int n, int H, int W, int C,
                                                      int k, int stride, int Ho, int Wo,
                                                      const float* pre_scale, const float* pre_shift, int pre_relu)
{
    // one thread = 8 channels x up to 4 horizontally adjacent outputs: the windows of neighbours overlap
    // (k - stride shared columns), so the strip is read once -- (3*stride + k) columns instead of 4*k
    constexpr int OX = 4;
    const int cg = C / 8;
    const int wq = (Wo + OX - 1) / OX;
    // Blocks are dealt round-robin to the 8 XCDs; give every XCD one CONTIGUOUS eighth of the output
    // raster, so the input rows shared by vertically adjacent windows (blocks a few indices apart)
    // meet in ONE L2 instead of being fetched by two (PMC: fetch was 1.43x the input tensor).
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const unsigned wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
    const unsigned idx = wg * 256u + threadIdx.x;
    const unsigned total = (unsigned)n * Ho * wq * cg;
    if (idx >= total) return;
    const int g = (int)(idx % cg);
    unsigned pix = idx / cg;
    const int oq = (int)(pix % wq); pix /= wq;
    const int oy = (int)(pix % Ho);
    const int b = (int)(pix / Ho);
    const int ox0 = oq * OX;
    const int nout = min(OX, Wo - ox0);
    float m[OX][8], ps[8], pb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ps[i] = pre_scale ? pre_scale[g * 8 + i] : 1.f;
        pb[i] = pre_scale ? pre_shift[g * 8 + i] : 0.f;
#pragma unroll
        for (int o = 0; o < OX; ++o) m[o][i] = -3.0e38f;
    }
    const int ncol = (nout - 1) * stride + k;                   // input columns of the strip
    const int CS = SPLIT ? 2 * C : C;                           // elements per stored pixel
    if (k == 3 && stride == 2 && nout == OX) {
        // the ResNet stem pool, full strip: all 27 loads are independent -> issue them back to back
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const E* row = src + (((size_t)b * H + oy * 2 + ky) * W + ox0 * 2) * CS + (SPLIT ? split_hi_elem(C, g * 8) : g * 8);
            Vec8<E> v[9], vl[SPLIT ? 9 : 1];
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                v[c] = *(const Vec8<E>*)(row + (size_t)c * CS);
                if constexpr (SPLIT) vl[c] = *(const Vec8<E>*)(row + (size_t)c * CS + split_group(C));
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                float x[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float xv = from_elem<E>(v[c].v[i]);
                    if constexpr (SPLIT) xv = __fadd_rn(xv, from_elem<E>(vl[c].v[i]));       // hi + lo: exact in fp32
                    x[i] = __builtin_fmaf(xv, ps[i], pb[i]);                                  // (stem_pool_x3 states the same arithmetic)
                    if (pre_relu) x[i] = fmaxf(x[i], 0.f);
                }
#pragma unroll
                for (int o = 0; o < OX; ++o) {
                    if (c >= 2 * o && c < 2 * o + 3) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) m[o][i] = fmaxf(m[o][i], x[i]);
                    }
                }
            }
        }
    } else
    for (int ky = 0; ky < k; ++ky) {
        const E* row = src + (((size_t)b * H + oy * stride + ky) * W + ox0 * stride) * CS + (SPLIT ? split_hi_elem(C, g * 8) : g * 8);
        for (int c = 0; c < ncol; ++c) {
            const Vec8<E> v = *(const Vec8<E>*)(row + (size_t)c * CS);
            float x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float xv = from_elem<E>(v.v[i]);
                if constexpr (SPLIT) xv = __fadd_rn(xv, from_elem<E>((*(const Vec8<E>*)(row + (size_t)c * CS + split_group(C))).v[i]));
                x[i] = __builtin_fmaf(xv, ps[i], pb[i]);
                if (pre_relu) x[i] = fmaxf(x[i], 0.f);
            }
#pragma unroll
            for (int o = 0; o < OX; ++o) {
                const int kx = c - o * stride;                     // column c inside output o's window?
                if (o < nout && kx >= 0 && kx < k) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) m[o][i] = fmaxf(m[o][i], x[i]);
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < OX; ++o) {
        if (o < nout) {
            E* dp = dst + (((size_t)b * Ho + oy) * Wo + ox0 + o) * CS + (SPLIT ? split_hi_elem(C, g * 8) : g * 8);
            if constexpr (SPLIT) store_split8((uint16_t*)dp, split_group(C), m[o]);
            else {
                Vec8<E> r;
#pragma unroll
                for (int i = 0; i < 8; ++i) r.v[i] = to_elem<E>(m[o][i]);
                *(Vec8<E>*)dp = r;
            }
        }
    }
}

hipError_t launch_maxpool(const void* src, void* dst, int n, int H, int W, int C, int k, int stride,
                          int Ho, int Wo, const float* pre_scale, const float* pre_shift, int pre_relu,
                          int precision, hipStream_t s, LaunchRec* rec)
{
    const long total = (long)n * Ho * ((Wo + 3) / 4) * (C / 8);
    const unsigned grid = (unsigned)((total + 255) / 256);
    launch_rec(rec, SBBSEG_LAUNCH_MAXPOOL, 256 * 4, 8, 1, (int)grid, (int)grid, 0);
    if (precision == kF32)
        hipLaunchKernelGGL(maxpool_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)src, (float*)dst, n, H, W, C, k, stride, Ho, Wo, pre_scale, pre_shift, pre_relu);
    else if (precision == kF16X3)
        hipLaunchKernelGGL((maxpool_kernel<_Float16, true>), dim3(grid), dim3(256), 0, s, (const _Float16*)src, (_Float16*)dst, n, H, W, C, k, stride, Ho, Wo, pre_scale, pre_shift, pre_relu);
    else if (precision == kF16)
        hipLaunchKernelGGL(maxpool_kernel<_Float16>, dim3(grid), dim3(256), 0, s, (const _Float16*)src, (_Float16*)dst, n, H, W, C, k, stride, Ho, Wo, pre_scale, pre_shift, pre_relu);
    else
        hipLaunchKernelGGL(maxpool_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, (const uint16_t*)src, (uint16_t*)dst, n, H, W, C, k, stride, Ho, Wo, pre_scale, pre_shift, pre_relu);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// head: 1x1 conv + BN + softmax + argmax (main.py:290: np.argmax over the softmax output, first
// maximum wins).  One thread per pixel; weights broadcast from LDS.
// ------------------------------------------------------------------------------------------------
template <typename E, bool SPLIT = false>
__global__ __launch_bounds__(256) void head_kernel(const HeadParams p)
{
    __shared__ float sw[64 * 8];
    __shared__ float ss[16];
    for (int i = threadIdx.x; i < p.cin * p.classes; i += 256) sw[i] = p.w[i];
    if (threadIdx.x < p.classes) { ss[threadIdx.x] = p.scale[threadIdx.x]; ss[8 + threadIdx.x] = p.shift[threadIdx.x]; }
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= p.M) return;
    float logit[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) logit[c] = 0.f;
    const E* src = (const E*)p.src + (size_t)m * p.cin * (SPLIT ? 2 : 1);
    for (int g = 0; g < p.cin / 8; ++g) {
        const int e0 = SPLIT ? split_hi_elem(p.cin, g * 8) : g * 8;
        const Vec8<E> v = *(const Vec8<E>*)(src + e0);
        Vec8<E> vl;
        if constexpr (SPLIT) vl = *(const Vec8<E>*)(src + e0 + split_group(p.cin));
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float xv = from_elem<E>(v.v[i]);
            if constexpr (SPLIT) xv += from_elem<E>(vl.v[i]);
            const float* wr = sw + (g * 8 + i) * p.classes;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < p.classes) logit[c] = fmaf(xv, wr[c], logit[c]);
        }
    }
    float mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < p.classes) { logit[c] = logit[c] * ss[c] + ss[8 + c]; mx = fmaxf(mx, logit[c]); }
    float pr[8], sum = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < p.classes) { pr[c] = expf(logit[c] - mx); sum += pr[c]; }
    int best = 0;
    float bestp = -1.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < p.classes) {
            pr[c] = pr[c] / sum;
            if (pr[c] > bestp) { bestp = pr[c]; best = c; }
            if (p.probs) p.probs[(size_t)m * p.classes + c] = pr[c];
        }
    p.labels[m] = (uint8_t)best;
}

hipError_t launch_head(const HeadParams& p, int precision, hipStream_t s, LaunchRec* rec)
{
    const unsigned grid = (unsigned)((p.M + 255) / 256);
    launch_rec(rec, SBBSEG_LAUNCH_HEAD, 256, p.classes, 1, (int)grid, (int)grid, 0);
    if (precision == kF32) hipLaunchKernelGGL(head_kernel<float>, dim3(grid), dim3(256), 0, s, p);
    else if (precision == kF16X3) hipLaunchKernelGGL((head_kernel<_Float16, true>), dim3(grid), dim3(256), 0, s, p);
    else if (precision == kF16) hipLaunchKernelGGL(head_kernel<_Float16>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(head_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// stitch: page pixel (y,x) takes the label of its owner tile (closed form of the reference's
// crop-and-overwrite, main.py:294-364).  own_x[x] = (tile column i << 16) | x-inside-tile, own_y alike.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stitch_kernel(const uint8_t* tile_labels, int H, int W, const int* own_x,
                                                     const int* own_y, int nyf, int Hp, int Wp, uint8_t* out)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Hp * Wp) return;
    const int y = (int)(idx / Wp), x = (int)(idx - (long)y * Wp);
    const int ex = own_x[x], ey = own_y[y];
    const int t = (ex >> 16) * nyf + (ey >> 16);
    out[idx] = tile_labels[((size_t)t * H + (ey & 0xffff)) * W + (ex & 0xffff)];
}

hipError_t launch_stitch(const uint8_t* tile_labels, int H, int W, const int* own_x, const int* own_y,
                         int nyf, int Hp, int Wp, uint8_t* out, hipStream_t s)
{
    const long total = (long)Hp * Wp;
    hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, tile_labels, H, W,
                       own_x, own_y, nyf, Hp, Wp, out);
    return hipGetLastError();
}

// the stitch of a group of views in one launch: block b serves 256 pixels of the plane of the view whose block range holds b (every plane
// starts a new block); the owner of a pixel is region_owner's closed form on the view's two axes -- the value stitch_kernel reads from
// its uploaded tables
__global__ __launch_bounds__(256) void stitch_views_kernel(const uint8_t* tile_labels, int H, int W, int margin, const ViewRec* views, int n_views)
{
    const ViewRec& v = views[view_find(n_views, blockIdx.x, [&](int m) { return views[m].blk_first; })];
    const long idx = (long)(blockIdx.x - v.blk_first) * 256 + threadIdx.x;
    if (idx >= (long)v.ch * v.cw) return;
    const int y = (int)(idx / v.cw), x = (int)(idx - (long)y * v.cw);
    const int ex = region_owner(view_axis_x(v, W, margin), x), ey = region_owner(view_axis_y(v, H, margin), y);
    const int t = v.first + (ex >> 16) * v.ny + (ey >> 16);
    v.labels[idx] = tile_labels[((size_t)t * H + (ey & 0xffff)) * W + (ex & 0xffff)];
}

hipError_t launch_stitch_views(const uint8_t* tile_labels, int H, int W, int margin, const ViewRec* views, int n_views, unsigned n_blocks, hipStream_t s)
{
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(stitch_views_kernel, dim3(n_blocks), dim3(256), 0, s, tile_labels, H, W, margin, views, n_views);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void resize_labels_kernel(const uint8_t* labels, int H, int W, const int* map_y,
                                                            const int* map_x, int out_h, int out_w, uint8_t* out)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)out_h * out_w) return;
    const int y = (int)(idx / out_w), x = (int)(idx - (long)y * out_w);
    out[idx] = labels[(size_t)map_y[y] * W + map_x[x]];
}

hipError_t launch_resize_labels(const uint8_t* labels, int H, int W, const int* map_y, const int* map_x,
                                int out_h, int out_w, uint8_t* out, hipStream_t s)
{
    const long total = (long)out_h * out_w;
    hipLaunchKernelGGL(resize_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, labels, H, W,
                       map_y, map_x, out_h, out_w, out);
    return hipGetLastError();
}

// The label resize of a chunk of views in one launch: patch p's 1 x H x W label map -> view p's out_h x out_w plane (main.py:378, the index
// rule of resize_labels_kernel).  A plane is walked as the run of bytes it is, in the 16-byte lines of its address: a lane owns one line
// and stores it as one 16-byte word -- a border mask is 12.6 MB per page, a byte store per lane issues sixteen times the stores -- except
// the line the plane starts in and the one it ends in, which belong to it only in part and are stored byte by byte (planes start anywhere,
// rows have any width: a line may hold the end of one row and the start of the next).  Block b serves lines of the view whose block range
// holds b (prefix sums, every plane starts a new block); the view's record depends on blockIdx only and comes through the scalar cache.
__global__ __launch_bounds__(256) void resize_labels_views_kernel(const uint8_t* labels, int H, int W, const WholeViewRec* views, const int* maps,
                                                                  int n_views)
{
    const int p = view_find(n_views, blockIdx.x, [&](int m) { return views[m].blk_first; });
    const WholeViewRec& v = views[p];
    const long total = (long)v.out_h * v.out_w;
    const long first = ((long)(blockIdx.x - v.blk_first) * 256 + threadIdx.x) * 16 - (long)v.lead;      // plane byte of the line's byte 0
    if (first >= total) return;
    const uint8_t* src = labels + (size_t)p * H * W;
    const int* map_y = maps + v.oy;
    const int* map_x = maps + v.ox;
    const long i0 = first < 0 ? 0 : first;
    int y = (int)(i0 / v.out_w), x = (int)(i0 - (long)y * v.out_w);
    const uint8_t* row = src + (size_t)map_y[y] * W;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const long i = first + k;
        if (i >= 0 && i < total) {
            w[k >> 2] |= (uint32_t)row[map_x[x]] << (8 * (k & 3));
            if (++x == v.out_w) {
                x = 0; ++y;
                if (i + 1 < total) row = src + (size_t)map_y[y] * W;
            }
        }
    }
    if (first >= 0 && first + 16 <= total) {
        *(uint4*)(v.out + first) = make_uint4(w[0], w[1], w[2], w[3]);      // (out - lead is a multiple of 16, and so is first + lead)
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (first + k >= 0 && first + k < total) v.out[first + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

hipError_t launch_resize_labels_views(const uint8_t* labels, int H, int W, const WholeViewRec* views, const int* maps, int n_views, unsigned n_blocks,
                                      hipStream_t s)
{
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(resize_labels_views_kernel, dim3(n_blocks), dim3(256), 0, s, labels, H, W, views, maps, n_views);
    return hipGetLastError();
}

template <typename E>
__global__ __launch_bounds__(256) void to_f32_kernel(const E* src, float* dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = from_elem<E>(src[i]);
}

__global__ __launch_bounds__(256) void split_to_f32_kernel(const _Float16* src, float* dst, size_t n, int C)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;         // i = pixel * C + channel
    if (i >= n) return;
    const size_t pix = i / C;
    const int ch = (int)(i - pix * C);
    const size_t e0 = pix * 2 * C + split_hi_elem(C, ch);           // channel groups [G hi][G lo] (internal.h)
    dst[i] = (float)src[e0] + (float)src[e0 + split_group(C)];
}

hipError_t launch_split_to_f32(const void* src, float* dst, size_t npix, int C, hipStream_t s)
{
    const size_t n = npix * C;
    hipLaunchKernelGGL(split_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const _Float16*)src, dst, n, C);
    return hipGetLastError();
}

// u8 label plane -> the reference's return layout: three identical channels (main.py:366, 380)
__global__ __launch_bounds__(256) void replicate3_kernel(const uint8_t* src, uint8_t* dst, size_t n4)
{
    // 4 labels -> 12 bytes per thread
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const uint32_t v = ((const uint32_t*)src)[i];
    const uint32_t a = v & 0xff, b = (v >> 8) & 0xff, c = (v >> 16) & 0xff, d = v >> 24;
    uint32_t* o = (uint32_t*)dst + i * 3;
    o[0] = a | (a << 8) | (a << 16) | (b << 24);
    o[1] = b | (b << 8) | (c << 16) | (c << 24);
    o[2] = c | (d << 8) | (d << 16) | (d << 24);
}

hipError_t launch_replicate3(const uint8_t* src, uint8_t* dst, size_t n, hipStream_t s)
{
    const size_t n4 = (n + 3) / 4;                   // buffers are padded to a multiple of 4 labels by the caller
    hipLaunchKernelGGL(replicate3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, src, dst, n4);
    return hipGetLastError();
}

// sbbseg_debug_tensor_period_mismatches: 16-byte word i of the tail [shift_words, shift_words + n_words) of a buffer against word i - shift_words
// (patch q against patch q - period: shift = period patches).  res[0] += differing bytes, res[1] = min(first differing byte offset into the tail);
// a grid-stride loop, a block reduction in LDS, then one atomic pair per block that found something.
__global__ __launch_bounds__(256) void period_mismatch_kernel(const uint4* __restrict__ base, size_t shift_words, size_t n_words,
                                                               unsigned long long* __restrict__ res)
{
    __shared__ unsigned long long s_cnt[256], s_first[256];
    unsigned long long cnt = 0, first = ~0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (size_t)gridDim.x * 256) {
        const uint4 a = base[i], b = base[i + shift_words];
        const uint32_t d[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
        if ((d[0] | d[1] | d[2] | d[3]) == 0) continue;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((d[w] >> (8 * k)) & 255u) {
                    ++cnt;
                    const unsigned long long off = (unsigned long long)i * 16 + w * 4 + k;
                    if (off < first) first = off;
                }
    }
    s_cnt[threadIdx.x] = cnt; s_first[threadIdx.x] = first;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
            if (s_first[threadIdx.x + h] < s_first[threadIdx.x]) s_first[threadIdx.x] = s_first[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_cnt[0]) {
        atomicAdd(&res[0], s_cnt[0]);
        atomicMin(&res[1], s_first[0]);
    }
}

hipError_t launch_period_mismatches(const void* data, size_t shift_bytes, size_t tail_bytes, unsigned long long* res, int num_cus, hipStream_t s)
{
    if ((shift_bytes | tail_bytes | (size_t)(uintptr_t)data) & 15) return hipErrorInvalidValue;
    const size_t n_words = tail_bytes / 16;
    if (n_words == 0) return hipSuccess;
    const size_t want = (n_words + 255) / 256, cap = (size_t)(num_cus > 0 ? num_cus : 256) * 8;
    hipLaunchKernelGGL(period_mismatch_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, s, (const uint4*)data, shift_bytes / 16, n_words, res);
    return hipGetLastError();
}

hipError_t launch_to_f32(const void* src, float* dst, size_t n, int precision, hipStream_t s)
{
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (precision == kF32) hipLaunchKernelGGL(to_f32_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)src, dst, n);
    else if (precision == kF16) hipLaunchKernelGGL(to_f32_kernel<_Float16>, dim3(grid), dim3(256), 0, s, (const _Float16*)src, dst, n);
    else hipLaunchKernelGGL(to_f32_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, (const uint16_t*)src, dst, n);
    return hipGetLastError();
}

}  // namespace sbbseg
