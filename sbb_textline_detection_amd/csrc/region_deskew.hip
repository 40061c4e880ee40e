// region_deskew.hip -- the rotate-and-project of the deskew search for ALL text-region boxes of a page at once (do_work_of_slopes,
// main.py:1721-1748: crop the textline map to the box, cv2.erode(crop, 5x5, iterations = 2), return_deskew_slope on the eroded crop).
//
// Two small kernels build the eroded crops of every box, packed one after the other; one kernel then computes the row profile of
// every (region, angle, destination row) of a sweep.  The arithmetic of a destination pixel is that of deskew_profile_kernel
// (page_glue.hip), statement for statement: fixed-point source coordinates, the float bicubic table, 16 taps added one by one in
// float64, no contraction, mask values as stored.  What differs is how the work is dealt out:
//   * the grid is a work list of (region, angle, group of kRegionDeskewRows rows) built from prefix sums on the host -- a small
//     region launches few blocks, not one 256-thread block per row;
//   * a WAVE owns a destination row; the region's geometry and the inverse map are wave-uniform and are read through the scalar
//     cache (loads only);
//   * the span of x whose 4 x 4 window can meet the crop is bounded analytically per row, so lanes never visit the columns (and
//     whole rows) that the old kernel's `continue` skipped one by one; inside the span the exact test still decides;
//   * the row's count is a wave reduction and one plain store.
#include "internal.h"

namespace sbbseg {

namespace {

// largest r with geom[r].crop_off <= idx (crop_off is strictly increasing: every box holds at least one pixel)
__device__ __forceinline__ int region_of_pixel(const DeskewRegion* geom, int n, long long idx)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (geom[mid].crop_off <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// cv2.erode with the 5x5 kernel, n iterations, on the CROP (default border: outside pixels never win) == one (4n+1)-wide minimum over
// the window clipped to the crop, separable (as launch_morph): pass 0 along x from the region's plane, pass 1 along y from tmp.
// Pass 0 is the only kernel that sees a plane: every region brings its own (pointer, width) in p.planes, so the boxes of one call may
// lie on any number of planes; everything after it works on the packed crops.  Regions are packed one after the other, so a wave
// usually lies inside one region: its plane record then comes through the scalar cache (loads only), per lane where a wave straddles
// regions.
__global__ __launch_bounds__(256) void region_crop_erode_kernel(const RegionDeskewParams p, int vertical)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total_pix) return;
    const int r = region_of_pixel(p.geom, p.n_regions, idx);
    const DeskewRegion& g = p.geom[r];
    const int local = (int)(idx - g.crop_off);
    const int yy = local / g.w, xx = local - yy * g.w;
    int v = 255;
    if (!vertical) {
        // the record of the first lane's region through the scalar cache (a wave-uniform index; the values are pinned to scalar registers,
        // or the compiler folds this load and the per-lane one below into one vector load) ...
        const int r0 = __builtin_amdgcn_readfirstlane(r);
        const uint64_t b0 = (uint64_t)(uintptr_t)p.planes[r0].base;
        const uint8_t* base = (const uint8_t*)(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(b0 >> 32)) << 32) |
                                                           (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b0));
        int W = __builtin_amdgcn_readfirstlane(p.planes[r0].W);
        if (r != r0) { base = p.planes[r].base; W = p.planes[r].W; }      // ... the lanes of a wave that straddles regions read their own
        const uint8_t* row = base + (size_t)(g.y + yy) * W + g.x;
        const int lo = max(xx - p.radius, 0), hi = min(xx + p.radius, g.w - 1);
        for (int q = lo; q <= hi; ++q) v = min(v, (int)row[q]);
        p.tmp[idx] = (uint8_t)v;
    } else {
        const uint8_t* col = p.tmp + g.crop_off + xx;
        const int lo = max(yy - p.radius, 0), hi = min(yy + p.radius, g.h - 1);
        for (int q = lo; q <= hi; ++q) v = min(v, (int)col[(size_t)q * g.w]);
        p.crops[idx] = (uint8_t)v;
    }
}

// x in [lo, hi] for which c * x + b can lie in [L, R] (a superset: one pixel of slack on either side); c ~ 0: all x or none
__device__ __forceinline__ void clip_span(double c, double b, double L, double R, int S, int& lo, int& hi)
{
    if (fabs(c) < 1e-7) {                                       // |c * x| < 0.004 for x < 32768
        if (b < L - 1.0 || b > R + 1.0) hi = -1;
        return;
    }
    double t0 = (L - b) / c, t1 = (R - b) / c;
    if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
    t0 = fmin(fmax(t0, -2.0), (double)S + 2.0);                 // (kept inside int range before the conversions)
    t1 = fmin(fmax(t1, -2.0), (double)S + 2.0);
    lo = max(lo, (int)floor(t0) - 1);
    hi = min(hi, (int)ceil(t1) + 1);
}

__global__ __launch_bounds__(256) void region_deskew_profile_kernel(const RegionDeskewParams p)
{
#pragma clang fp contract(off)
    __shared__ float tab[32 * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 128) tab[tid] = p.cubic[tid];
    __syncthreads();
    // the block's region: the last one whose first block is not behind this block (block-uniform)
    const int b = blockIdx.x;
    int rlo = 0, rhi = p.n_regions - 1;
    while (rlo < rhi) {
        const int mid = (rlo + rhi + 1) >> 1;
        if (p.geom[mid].block0 <= b) rlo = mid;
        else rhi = mid - 1;
    }
    const DeskewRegion& g = p.geom[rlo];
    const int S = g.S, top = g.top, left = g.left, H = g.h, W = g.w;
    const int local = b - g.block0;
    const int a = local / g.row_groups, grp = local - a * g.row_groups;
    const double* m = p.minv + ((size_t)rlo * p.n_angles + a) * 6;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const uint8_t* mask = p.crops + g.crop_off;
    int* counts = p.counts + g.count_off + (size_t)a * S;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = 0; k < kRegionDeskewRows / 4; ++k) {
        const int y = grp * kRegionDeskewRows + k * 4 + wave;
        if (y >= S) break;                                      // wave-uniform
        const long long X0 = __double2ll_rn((m1 * (double)y + m2) * 1024.0) + 16;
        const long long Y0 = __double2ll_rn((m4 * (double)y + m5) * 1024.0) + 16;
        // A pixel can only count when some tap lies inside the crop: sx in [left - 2, left + W], sy in [top - 2, top + H] (with a margin
        // of one pixel between crop and square no clamped tap is inside the crop).  sx is floor(m0 x + m1 y + m2 + 1/64 +- 1/1024): the
        // real-valued coordinate lies within (-0.02, 1] of it, the bounds below allow two whole pixels.
        int x_lo = 0, x_hi = S - 1;
        if (g.clip) {
            clip_span(m0, m1 * (double)y + m2, (double)(left - 4), (double)(left + W + 3), S, x_lo, x_hi);
            clip_span(m3, m4 * (double)y + m5, (double)(top - 4), (double)(top + H + 3), S, x_lo, x_hi);
        }
        int cnt = 0;
        for (int x = x_lo + lane; x <= x_hi; x += 64) {
            const long long X = (X0 + __double2ll_rn(m0 * (double)x * 1024.0)) >> 5;
            const long long Y = (Y0 + __double2ll_rn(m3 * (double)x * 1024.0)) >> 5;
            long long sx = X >> 5, sy = Y >> 5;
            sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
            sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
            const int ax = (int)(X & 31), ay = (int)(Y & 31);
            // window rows sy-1 .. sy+2, columns sx-1 .. sx+2, clamped to the square; non-zero source pixels only inside the crop
            const int wx_lo = (int)min(max(sx - 1, 0LL), (long long)S - 1), wx_hi = (int)min(max(sx + 2, 0LL), (long long)S - 1);
            const int wy_lo = (int)min(max(sy - 1, 0LL), (long long)S - 1), wy_hi = (int)min(max(sy + 2, 0LL), (long long)S - 1);
            if (wx_hi < left || wx_lo >= left + W || wy_hi < top || wy_lo >= top + H) continue;
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int yy = (int)min(max(sy - 1 + r, 0LL), (long long)S - 1) - top;
                const float wy = tab[ay * 4 + r];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const int xx = (int)min(max(sx - 1 + cc, 0LL), (long long)S - 1) - left;
                    const float w2 = wy * tab[ax * 4 + cc];                          // the 2-D table entry: a float product
                    const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                    const double v = in ? (double)mask[(size_t)yy * W + xx] : 0.0;
                    sum = sum + v * (double)w2;
                }
            }
            cnt += sum != 0.0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (lane == 0) counts[y] = cnt;
    }
}

}  // namespace

hipError_t launch_region_deskew_crops(const RegionDeskewParams& p, hipStream_t s)
{
    const unsigned grid = (unsigned)((p.total_pix + 255) / 256);
    hipLaunchKernelGGL(region_crop_erode_kernel, dim3(grid), dim3(256), 0, s, p, 0);
    hipLaunchKernelGGL(region_crop_erode_kernel, dim3(grid), dim3(256), 0, s, p, 1);
    return hipGetLastError();
}

hipError_t launch_region_deskew_profiles(const RegionDeskewParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(region_deskew_profile_kernel, dim3((unsigned)p.total_blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace sbbseg
