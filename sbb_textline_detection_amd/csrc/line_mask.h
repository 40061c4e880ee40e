// line_mask.h -- the per-pixel arithmetic of the deskewed text-line mask of ONE text region (textline_contours_postprocessing,
// main.py:1472-1487: crop * 255, MORPH_OPEN, MORPH_CLOSE, rotate_image by the region's slope, != 0), as plain integer C++ for host and
// device code.  region_lines.hip runs these statements on the device, sbbseg_region_line_masks_host on the CPU.
//
// The rotation is cv2.warpAffine(INTER_CUBIC, BORDER_REPLICATE) of a uint8 image [EXT, unpinned: OpenCV 4.5.1 imgwarp.cpp restated]:
//   * source coordinates in fixed point with 5 fractional bits, as the float path of the deskew sweep (page_glue.hip) computes them;
//   * the FIXED-POINT bicubic table (initInterTab2D): per (ay, ax) sixteen int16 i[r][c] = saturate_cast<short>(float(tab[ay][r] *
//     tab[ax][c]) * 32768), rounded to nearest even; when they do not sum to 32768 the difference is taken from one entry of the 2 x 2
//     block at rows / columns {2, 3}: the block is scanned row-major with both candidates starting at (2, 2), a strictly smaller entry
//     replaces the minimum candidate, otherwise a strictly larger one replaces the maximum candidate; a negative difference raises the
//     maximum, a positive one lowers the minimum;
//   * pixel = saturate_cast<uchar>((sum of 16 taps src * i + 16384) >> 15) in int32 (remapBicubic, FixedPtCast<int, uchar, 15>), the
//     taps clamped to the image.
#ifndef SBBSEG_LINE_MASK_H
#define SBBSEG_LINE_MASK_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBB_LM_HD __host__ __device__ __forceinline__
#else
#define SBB_LM_HD inline
#endif

namespace sbbseg {

constexpr int kLineTabEntries = 32 * 32 * 16;      // int16 [ay][ax][r][c]

// the sixteen integer weights of sub-pixel position (ay, ax); tab = the float bicubic table [32][4]
SBB_LM_HD void line_mask_weights(const float* tab, int ay, int ax, int16_t* w16)
{
#pragma clang fp contract(off)
    int isum = 0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            const float v = tab[ay * 4 + r] * tab[ax * 4 + c];
            float s = rintf(v * 32768.0f);                              // cvRound: to nearest even
            s = s < -32768.0f ? -32768.0f : (s > 32767.0f ? 32767.0f : s);
            w16[r * 4 + c] = (int16_t)(int)s;
            isum += (int)s;
        }
    if (isum != 32768) {
        const int diff = isum - 32768;
        int lo = 2 * 4 + 2, hi = 2 * 4 + 2;
        for (int r = 2; r < 4; ++r)
            for (int c = 2; c < 4; ++c) {
                const int k = r * 4 + c;
                if (w16[k] < w16[lo]) lo = k;
                else if (w16[k] > w16[hi]) hi = k;
            }
        if (diff < 0) w16[hi] = (int16_t)(w16[hi] - diff);
        else w16[lo] = (int16_t)(w16[lo] - diff);
    }
}

// fixed-point source coordinate of column 0 of destination row y (WarpAffineInvoker: X0 / Y0 with the rounding delta)
SBB_LM_HD void line_mask_row_origin(const double* m, int y, long long* X0, long long* Y0)
{
#pragma clang fp contract(off)
    *X0 = llrint((m[1] * (double)y + m[2]) * 1024.0) + 16;
    *Y0 = llrint((m[4] * (double)y + m[5]) * 1024.0) + 16;
}

// the rotated uint8 value of destination pixel x of that row; src: the h x w image, itab: int16 [32][32][16]
SBB_LM_HD int line_mask_pixel(const uint8_t* src, int w, int h, double m0, double m3, long long X0, long long Y0, int x, const int16_t* itab)
{
#pragma clang fp contract(off)
    const long long X = (X0 + llrint(m0 * (double)x * 1024.0)) >> 5;
    const long long Y = (Y0 + llrint(m3 * (double)x * 1024.0)) >> 5;
    long long sxl = X >> 5, syl = Y >> 5;
    sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl);
    syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
    const int sx = (int)sxl, sy = (int)syl;
    const int16_t* wt = itab + ((((int)(Y & 31) << 5) + (int)(X & 31)) << 4);
    int xs[4];
    for (int c = 0; c < 4; ++c) {
        const int xx = sx - 1 + c;
        xs[c] = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
    }
    int sum = 0;
    for (int r = 0; r < 4; ++r) {
        int yy = sy - 1 + r;
        yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
        const uint8_t* row = src + (size_t)yy * w;
        for (int c = 0; c < 4; ++c) sum += (int)row[xs[c]] * (int)wt[r * 4 + c];
    }
    const int v = (sum + 16384) >> 15;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one output sample of a 1-D pass of cv2.erode / cv2.dilate on the crop: min (is_max = 0) or max over [pos - radius, pos + radius]
// clipped to [0, len) -- outside pixels never win; `scale`: every sample read is multiplied by it in uint8 (the crop * 255 of
// main.py:1475-1476 rides on the first pass)
SBB_LM_HD int line_mask_morph_1d(const uint8_t* p, size_t stride, int pos, int len, int radius, int is_max, int scale)
{
    const int lo = pos - radius < 0 ? 0 : pos - radius, hi = pos + radius > len - 1 ? len - 1 : pos + radius;
    int v = is_max ? 0 : 255;
    for (int q = lo; q <= hi; ++q) {
        const int s = (int)(uint8_t)(p[(size_t)q * stride] * scale);
        v = is_max ? (s > v ? s : v) : (s < v ? s : v);
    }
    return v;
}

}  // namespace sbbseg

#endif /* SBBSEG_LINE_MASK_H */
