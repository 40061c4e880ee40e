// region_lines.hip -- the deskewed text-line mask of ALL text-region boxes of a page at once (textline_contours_postprocessing,
// main.py:1472-1487, as do_work_of_slopes calls it at main.py:1750 with the eroded crop and the region's slope): crop * 255,
// MORPH_OPEN, MORPH_CLOSE, rotate_image by the slope onto the crop's own h x w, != 0; and the two projections the line splitters
// open on (row sums, main.py:539; column sums, main.py:1020).
//
// The crops arrive packed one after the other from region_deskew.hip's crop / erode kernels.  Eight launches whatever the number of
// boxes: six 1-D passes of the morphology on the packed crops (erode, dilate, dilate, erode with the 5 x 5 kernel on the CROP == a
// clipped separable min(5) / max(9) / min(5)), the warp with the row sums, the column sums.  The per-pixel arithmetic is line_mask.h's,
// shared with the host twin.  The warp follows region_deskew_profile_kernel: a work list of (region, group of kRegionLineRows rows)
// from prefix sums, a wave per destination row, geometry and inverse map wave-uniform through the scalar cache (loads only), the row
// sum a wave reduction and one plain store.  The column sums are a second small pass over the stored mask (a thread per column):
// integer sums, no atomics, no zero-fill.
#include "internal.h"
#include "line_mask.h"

namespace sbbseg {

namespace {

// largest r with geom[r].crop_off <= idx (crop_off is strictly increasing: every box holds at least one pixel)
__device__ __forceinline__ int line_region_of_pixel(const LineRegion* geom, int n, long long idx)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (geom[mid].crop_off <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void region_line_morph_kernel(const RegionLinesParams p, const uint8_t* src, uint8_t* dst, int radius,
                                                                int is_max, int vertical, int scale)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total_pix) return;
    const LineRegion& g = p.geom[line_region_of_pixel(p.geom, p.n_regions, idx)];
    const int local = (int)(idx - g.crop_off);
    const int yy = local / g.w, xx = local - yy * g.w;
    const uint8_t* base = src + g.crop_off;
    const int v = vertical ? line_mask_morph_1d(base + xx, (size_t)g.w, yy, g.h, radius, is_max, scale)
                           : line_mask_morph_1d(base + (size_t)yy * g.w, 1, xx, g.w, radius, is_max, scale);
    dst[idx] = (uint8_t)v;
}

__global__ __launch_bounds__(256) void region_line_warp_kernel(const RegionLinesParams p)
{
    const int tid = threadIdx.x, lane = tid & 63;
    // the block's region: the last one whose first block is not behind this block (block-uniform)
    const int b = blockIdx.x;
    int rlo = 0, rhi = p.n_regions - 1;
    while (rlo < rhi) {
        const int mid = (rlo + rhi + 1) >> 1;
        if (p.geom[mid].block0 <= b) rlo = mid;
        else rhi = mid - 1;
    }
    const LineRegion& g = p.geom[rlo];
    const int H = g.h, W = g.w;
    const int grp = b - g.block0;
    const double* m = p.minv + (size_t)rlo * 6;
    const double m0 = m[0], m3 = m[3];
    const uint8_t* src = p.b + g.crop_off;
    uint8_t* dst = p.mask + g.crop_off;
    int* rows = p.rows + g.row_off;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = 0; k < kRegionLineRows / 4; ++k) {
        const int y = grp * kRegionLineRows + k * 4 + wave;
        if (y >= H) break;                                      // wave-uniform
        long long X0, Y0;
        line_mask_row_origin(m, y, &X0, &Y0);
        int cnt = 0;
        for (int x = lane; x < W; x += 64) {
            const int d = line_mask_pixel(src, W, H, m0, m3, X0, Y0, x, p.itab) != 0;
            dst[(size_t)y * W + x] = (uint8_t)d;
            cnt += d;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (lane == 0) rows[y] = cnt;
    }
}

__global__ __launch_bounds__(256) void region_line_cols_kernel(const RegionLinesParams p)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total_cols) return;
    int lo = 0, hi = p.n_regions - 1;                           // largest r with col_off <= idx (strictly increasing: w >= 1)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.geom[mid].col_off <= idx) lo = mid;
        else hi = mid - 1;
    }
    const LineRegion& g = p.geom[lo];
    const uint8_t* col = p.mask + g.crop_off + (idx - g.col_off);
    int cnt = 0;
    for (int y = 0; y < g.h; ++y) cnt += col[(size_t)y * g.w];
    p.cols[idx] = cnt;
}

}  // namespace

hipError_t launch_region_line_morph(const RegionLinesParams& p, hipStream_t s)
{
    const unsigned grid = (unsigned)((p.total_pix + 255) / 256);
    // MORPH_OPEN = erode, dilate; MORPH_CLOSE = dilate, erode (main.py:1478-1479): min over 5, max over 9, min over 5, x then y each
    const int radius[3] = {2, 4, 2}, is_max[3] = {0, 1, 0};
    for (int k = 0; k < 3; ++k) {
        hipLaunchKernelGGL(region_line_morph_kernel, dim3(grid), dim3(256), 0, s, p, (const uint8_t*)p.b, p.a, radius[k], is_max[k], 0, k == 0 ? 255 : 1);
        hipLaunchKernelGGL(region_line_morph_kernel, dim3(grid), dim3(256), 0, s, p, (const uint8_t*)p.a, p.b, radius[k], is_max[k], 1, 1);
    }
    return hipGetLastError();
}

hipError_t launch_region_line_masks(const RegionLinesParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(region_line_warp_kernel, dim3((unsigned)p.total_blocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(region_line_cols_kernel, dim3((unsigned)((p.total_cols + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace sbbseg
