// page_glue.hip -- byte and integer work on whole page planes: Otsu threshold, morphology, the union-find component labelling with its
// contour ranking, and the rotate-and-project of the deskew sweep.
#include "device_prims.h"

namespace sbbseg {

// ------------------------------------------------------------------------------------------------
// Otsu threshold of channel 0 of the (virtually rescaled) page -- cv2.threshold(img[:,:,0], 0, 255,
// THRESH_BINARY + THRESH_OTSU) of otsu_copy (main.py:178-194).  Pass 1: 256-bin histogram, an HBM-bound
// scan (runs of equal bytes are counted in registers first: document pages are mostly one value, and
// same-address LDS atomics serialise).  Pass 2: one thread walks the 256 bins in the order and
// precision OpenCV's getThreshVal_Otsu_8u does [EXT], fp64, no FMA contraction.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hist_u8_kernel(const uint8_t* page, int src_Wp, int Hp, int Wp,
                                                      const int* map_y, const int* map_x, unsigned* hist)
{
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    constexpr int RUN = 16;
    const long total = (long)Hp * Wp;
    for (long base = ((long)blockIdx.x * 256 + threadIdx.x) * RUN; base < total; base += (long)gridDim.x * 256 * RUN) {
        int y = (int)(base / Wp), x = (int)(base - (long)y * Wp);
        const uint8_t* row = page + (size_t)(map_y ? map_y[y] : y) * src_Wp * 3;
        int prev = -1;
        unsigned cnt = 0;
        for (int i = 0; i < RUN && base + i < total; ++i) {
            const int v = row[(size_t)(map_x ? map_x[x] : x) * 3];
            if (v != prev) {
                if (cnt) atomicAdd(&h[prev], cnt);
                prev = v;
                cnt = 0;
            }
            ++cnt;
            if (++x == Wp) {
                x = 0;
                if (++y < Hp) row = page + (size_t)(map_y ? map_y[y] : y) * src_Wp * 3;
            }
        }
        if (cnt) atomicAdd(&h[prev], cnt);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

__global__ void otsu_threshold_kernel(const unsigned* hist, long n_pixels, int* thr)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double scale = 1.0 / (double)n_pixels;
    double mu = 0.0;
    for (int i = 0; i < 256; ++i) mu += (double)i * (double)hist[i];
    mu *= scale;
    const double eps = (double)1.1920928955078125e-07f;      // FLT_EPSILON
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int max_val = 0;
    for (int i = 0; i < 256; ++i) {
        const double p_i = (double)hist[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        if (fmin(q1, q2) < eps || fmax(q1, q2) > 1.0 - eps) continue;
        mu1 = (mu1 + (double)i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double d = mu1 - mu2;
        const double sigma = q1 * q2 * d * d;
        if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
    }
    *thr = max_val;
}

hipError_t launch_otsu(const uint8_t* page, int src_Wp, int Hp, int Wp, const int* map_y, const int* map_x,
                       unsigned* hist, int* thr, int num_cus, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(hist, 0, 256 * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const long total = (long)Hp * Wp;
    long blocks = (total + 256 * 16 - 1) / (256 * 16);
    if (blocks > 8L * num_cus) blocks = 8L * num_cus;
    hipLaunchKernelGGL(hist_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, page, src_Wp, Hp, Wp, map_y, map_x, hist);
    hipLaunchKernelGGL(otsu_threshold_kernel, dim3(1), dim3(64), 0, s, hist, total, thr);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Stage glue around the border / layout models: cv2.erode / cv2.dilate with the reference's
// 5x5 kernel of ones (main.py:57) and the largest connected component of the border mask (main.py:394-404).
// ------------------------------------------------------------------------------------------------
// n iterations of a k x k min (erode) / max (dilate) filter with cv2's default border (the outside never wins:
// BORDER_CONSTANT with +inf / -inf) == ONE (n(k-1)+1)-wide filter over the window clipped to the image, separable.
// pass 0: along x, pass 1: along y.
// binarize: 0 = the plane as it is; 1 = t > 0 ? 255 : 0 (cv2.threshold(gray, 0, 255, THRESH_BINARY), main.py:395); 0x100 | label =
// t == label ? 255 : 0 (the class mask of get_text_region_contours_and_boxes, main.py:457-461)
__device__ __forceinline__ int morph_binarize(int t, int binarize)
{
    if (binarize & 0x100) return t == (binarize & 0xff) ? 255 : 0;
    return binarize ? (t > 0 ? 255 : 0) : t;
}
__global__ __launch_bounds__(256) void morph_pass_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int radius, int is_max,
                                                         int vertical, int binarize)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
    int v = is_max ? 0 : 255;
    if (!vertical) {
        const int lo = max(x - radius, 0), hi = min(x + radius, W - 1);
        const uint8_t* row = src + (size_t)y * W;
        for (int q = lo; q <= hi; ++q) {
            int t = row[q];
            t = morph_binarize(t, binarize);
            v = is_max ? max(v, t) : min(v, t);
        }
    } else {
        const int lo = max(y - radius, 0), hi = min(y + radius, H - 1);
        for (int q = lo; q <= hi; ++q) {
            const int t = src[(size_t)q * W + x];
            v = is_max ? max(v, t) : min(v, t);
        }
    }
    dst[idx] = (uint8_t)v;
}

// The same pass, FOUR horizontally adjacent output pixels per thread (W % 4 == 0: every row starts on a 4-byte boundary): the row pass reads
// the 4 + 2 radius window bytes once for its four outputs, the column pass reads one 32-bit word per row.  A thread per pixel issued
// 2 radius + 1 byte loads per output: 147 us per pass on a 4200 x 3000 mask at radius 12 (extract_page's six dilations).
template <int IS_MAX>
__global__ __launch_bounds__(256) void morph_pass4_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int radius, int vertical, int binarize)
{
    const int W4 = W >> 2;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)H * W4) return;
    const int y = (int)(g / W4), x0 = (int)(g - (long)y * W4) * 4;
    constexpr int ID = IS_MAX ? 0 : 255;
    auto op = [](int a, int b) __attribute__((always_inline)) { return IS_MAX ? max(a, b) : min(a, b); };
    int o0 = ID, o1 = ID, o2 = ID, o3 = ID;
    if (!vertical) {
        const uint8_t* row = src + (size_t)y * W;
        // window of output j = [x0 + j - radius, x0 + j + radius]: bytes x0 - radius + 3 .. x0 + radius are common to all four
        int mid = ID;
        for (int q = x0 - radius + 3; q <= x0 + radius; ++q) {
            if ((unsigned)q < (unsigned)W) { const int t = morph_binarize(row[q], binarize); mid = op(mid, t); }
        }
        int e[6];                                           // the three bytes on either side of the common part
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ql = x0 - radius + j, qr = x0 + radius + 1 + j;
            int tl = ID, tr = ID;
            if ((unsigned)ql < (unsigned)W) tl = morph_binarize(row[ql], binarize);
            if ((unsigned)qr < (unsigned)W) tr = morph_binarize(row[qr], binarize);
            e[j] = tl; e[3 + j] = tr;
        }
        o0 = op(mid, op(e[0], op(e[1], e[2])));
        o1 = op(mid, op(e[1], op(e[2], e[3])));
        o2 = op(mid, op(e[2], op(e[3], e[4])));
        o3 = op(mid, op(e[3], op(e[4], e[5])));
    } else {
        const int lo = max(y - radius, 0), hi = min(y + radius, H - 1);
        for (int q = lo; q <= hi; ++q) {
            const uint32_t t = *(const uint32_t*)(src + (size_t)q * W + x0);
            o0 = op(o0, (int)(t & 255u)); o1 = op(o1, (int)((t >> 8) & 255u)); o2 = op(o2, (int)((t >> 16) & 255u)); o3 = op(o3, (int)(t >> 24));
        }
    }
    *(uint32_t*)(dst + (size_t)y * W + x0) = (uint32_t)o0 | ((uint32_t)o1 << 8) | ((uint32_t)o2 << 16) | ((uint32_t)o3 << 24);
}

hipError_t launch_morph(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int H, int W, int radius, int is_max, int binarize, hipStream_t s)
{
    if ((W & 3) == 0 && radius >= 2 && (((uintptr_t)src | (uintptr_t)tmp | (uintptr_t)dst) & 3) == 0) {
        const unsigned grid4 = (unsigned)(((long)H * (W >> 2) + 255) / 256);
        if (is_max) {
            hipLaunchKernelGGL(morph_pass4_kernel<1>, dim3(grid4), dim3(256), 0, s, src, tmp, H, W, radius, 0, binarize);
            hipLaunchKernelGGL(morph_pass4_kernel<1>, dim3(grid4), dim3(256), 0, s, (const uint8_t*)tmp, dst, H, W, radius, 1, 0);
        } else {
            hipLaunchKernelGGL(morph_pass4_kernel<0>, dim3(grid4), dim3(256), 0, s, src, tmp, H, W, radius, 0, binarize);
            hipLaunchKernelGGL(morph_pass4_kernel<0>, dim3(grid4), dim3(256), 0, s, (const uint8_t*)tmp, dst, H, W, radius, 1, 0);
        }
        return hipGetLastError();
    }
    const unsigned grid = (unsigned)(((long)H * W + 255) / 256);
    hipLaunchKernelGGL(morph_pass_kernel, dim3(grid), dim3(256), 0, s, src, tmp, H, W, radius, is_max, 0, binarize);
    hipLaunchKernelGGL(morph_pass_kernel, dim3(grid), dim3(256), 0, s, (const uint8_t*)tmp, dst, H, W, radius, is_max, 1, 0);
    return hipGetLastError();
}

// 8-connected components of mask > 0 by union-find on pixel indices (roots = smallest index of a component = its first
// pixel in raster order).  parent values only ever decrease and every value ever stored is an ancestor, so a stale read
// (another CU's update not yet visible) costs a retry, never a wrong merge: links are made by atomicMin, whose RETURN
// value is what decides.
__device__ inline int cc_find(int* parent, int i)
{
    int p = parent[i];
    while (p != i) {
        const int g = parent[p];
        if (g != p) parent[i] = g;                          // path halving (any ancestor is a valid parent)
        i = p;
        p = g;
    }
    return i;
}
__device__ inline void cc_union(int* parent, int a, int b)
{
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[b], a);           // hang the larger root under the smaller one
        if (old == b) return;
        b = old;                                            // b had been linked meanwhile: go on from its parent
    }
}
// Wave-aggregated atomics: a page mask is mostly ONE component, so nearly every lane of a wave targets the same root -- 11 M
// single-address atomics took 125 ms before the lanes of a wave were combined (one atomic per wave and distinct root).
__device__ inline void wave_add_by_root(int* dst, int root, int val)
{
    bool pending = root >= 0 && val != 0;
    while (__builtin_amdgcn_ballot_w64(pending)) {
        const unsigned long long live = __builtin_amdgcn_ballot_w64(pending);
        const int leader = __builtin_ctzll(live);
        const int r = __builtin_amdgcn_readlane(root, leader);
        const bool mine = pending && root == r;
        int v = mine ? val : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&dst[r], v);
        pending = pending && !mine;
    }
}
__device__ inline void wave_minmax_by_root(int* dmin, int* dmax, int root, int lo, int hi)
{
    bool pending = root >= 0;
    while (__builtin_amdgcn_ballot_w64(pending)) {
        const unsigned long long live = __builtin_amdgcn_ballot_w64(pending);
        const int leader = __builtin_ctzll(live);
        const int r = __builtin_amdgcn_readlane(root, leader);
        const bool mine = pending && root == r;
        int a = mine ? lo : (1 << 30), b = mine ? hi : -1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { a = min(a, __shfl_xor(a, off)); b = max(b, __shfl_xor(b, off)); }
        if ((int)(threadIdx.x & 63) == leader) { atomicMin(&dmin[r], a); atomicMax(&dmax[r], b); }
        pending = pending && !mine;
    }
}
// parent = first pixel of the horizontal run (keeps the union-find trees flat).  One WAVE per row, 64 pixels per step: the run
// starts of a chunk come from the lanes' mask ballot (highest clear bit below the lane), a run that crosses into the next chunk
// is carried in a scalar.  (Round 3 walked a row per THREAD -- 3 000 dependent, uncoalesced steps: 0.70 ms at 4200 x 3000.)
__global__ __launch_bounds__(64) void cc_rows_kernel(const uint8_t* mask, int* parent, int* count, int H, int W)
{
    const int y = blockIdx.x, lane = threadIdx.x;
    if (y >= H) return;
    const long row = (long)y * W;
    int carry = -1;                                         // start of the run that reaches the left edge of the chunk, or -1
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool m = x < W && mask[row + x] != 0;
        const unsigned long long bits = __builtin_amdgcn_ballot_w64(m);
        const unsigned long long below = lane ? (~bits & ((1ull << lane) - 1ull)) : 0ull;      // clear bits under this lane
        int start = below ? (int)(row + x0 + (64 - __builtin_clzll(below))) : (carry >= 0 ? carry : (int)(row + x0));
        if (x < W) {
            parent[row + x] = m ? start : -1;
            count[row + x] = 0;
        }
        const int last = __builtin_amdgcn_readlane(m ? start : -1, 63);
        carry = last;                                       // lane 63 set: its run goes on (x0 + 64 <= W there, or the loop ends)
    }
}
__global__ __launch_bounds__(256) void cc_link_kernel(const uint8_t* mask, int* parent, int H, int W)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
    if (y == 0 || !mask[idx]) return;
    const long up = idx - W;
    // Only the LEFT END of a contact between two row runs makes the union: a pixel whose left neighbour is set (same run) and whose
    // upper-left pixel is set too (same upper run as `up`) repeats a union its left neighbour is responsible for -- inside a blob
    // that is every pixel but one per run pair (12.6 M root walks on a page mask: 1.5 ms; now ~ the number of runs).  Same for the
    // diagonal links: through a set left / right neighbour the link exists already (that neighbour sees the pixel as its N).
    const bool left = x > 0 && mask[idx - 1];
    if (mask[up]) {
        if (!(left && mask[up - 1])) cc_union(parent, (int)idx, (int)up);      // N set: NW / NE are joined to it through their row runs
        return;
    }
    if (x > 0 && mask[up - 1] && !left) cc_union(parent, (int)idx, (int)(up - 1));
    if (x + 1 < W && mask[up + 1] && !mask[idx + 1]) cc_union(parent, (int)idx, (int)(up + 1));
}
// flatten + pixel count per root (a lane merges its pixels while their root stays the same, equal roots across the lanes of a wave are
// merged by wave_add_by_root: one atomic per wave and distinct root)
__global__ __launch_bounds__(256) void cc_count_kernel(int* parent, int* count, long n)
{
    // A WAVE per 4 096 consecutive pixels, 64 consecutive pixels per step (coalesced); each lane merges the pixels of its own column of the
    // 64 x 64 block while their root stays the same.  (Up to round 4 a THREAD walked 64 consecutive pixels: every load of the wave touched
    // 64 lines, 0.65 ms at 4200 x 3000; sums do not care how the pixels are dealt to the lanes.)
    const long wave_base = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4096;
    const int lane = threadIdx.x & 63;
    int cur = -1, run = 0;
    for (int k = 0; k < 64; ++k) {
        const long i = wave_base + k * 64 + lane;
        int r = -1;
        if (i < n && parent[i] >= 0) { r = cc_find(parent, (int)i); parent[i] = r; }
        if (__builtin_amdgcn_ballot_w64(r >= 0 && r != cur)) {     // wave-uniform branch: some lane meets another root (background pixels end nothing)
            const bool flush = r >= 0 && r != cur;
            wave_add_by_root(count, flush ? cur : -1, run);
            if (flush) { cur = r; run = 0; }
        }
        run += r >= 0;
    }
    wave_add_by_root(count, cur, run);
}
// cc_count_kernel's `parent[i] = root` races with the path halving of OTHER threads' walks through i (cc_find stores an ancestor it read
// before the root was written): a few pixels per million were left pointing at a non-root ancestor, and the kernels below, which take
// parent[] for the root, credited their cells / extents to that ancestor -- the lower-bound area of a blob came out a little short in
// some runs, so equal-area blobs were ranked at random (round 5: tools/border_repeat_probe.py, three 31 x 33 blobs).  This pass runs
// with no halving writer active: every store is a root, a reader sees an ancestor or the root, the walk ends at the root either way.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* parent, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int p = parent[i];
    if (p < 0) return;
    int q = parent[p];
    if (q == p) return;                                     // already at its root (nearly every pixel)
    while (q != p) { p = q; q = parent[p]; }                // read-only walk
    parent[i] = p;
}
// ---- ranking by cv2.contourArea (main.py:399-401).  The outer contour cv2.findContours traces runs through the centres of the
// component's boundary pixels (8-connected steps); its polygon area is, for the component with its holes filled, the number of
// 2 x 2 pixel cells that are completely inside plus half the number of cells with exactly three pixels inside (a diagonal
// step cuts such a cell in half).  Counted over the component AS IT IS (holes not filled) that sum is a LOWER bound of the
// contour area, and (w - 1)(h - 1) of the bounding box an UPPER bound: the device picks the component with the largest lower
// bound and reports whether any other component's upper bound could beat it; only then does the host trace contours.
// Areas are kept doubled (integers).  Two set pixels of one 2 x 2 cell are 8-neighbours, i.e. of one component.
__global__ __launch_bounds__(256) void cc_cell_area_kernel(const int* parent, int* area2, int H, int W)
{
    // a WAVE per 64 strips of 64 cells (strips in row-major order of the cell rows): step k = strip k of the wave, a cell per lane
    // (coalesced); a lane sums its cells while their root stays the same and flushes through wave_add_by_root (one atomic per wave and
    // distinct root).  A thread per CELL sent 197 k atomics to the one root of a page mask: 2.2 ms.
    const long strips_per_row = (W - 1 + 63) / 64, n_strips = strips_per_row * (H - 1);
    const long first = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    const int lane = threadIdx.x & 63;
    int cur = -1, sum = 0;
    for (int k = 0; k < 64; ++k) {
        const long sidx = first + k;
        const bool live = sidx < n_strips;
        const int y = live ? (int)(sidx / strips_per_row) : 0;
        const int x = live ? (int)(sidx - (long)y * strips_per_row) * 64 + lane : 0;
        int root = -1, val = 0;
        if (live && x < W - 1) {
            const long i = (long)y * W + x;
            const int a = parent[i], b = parent[i + 1], c2 = parent[i + W], d = parent[i + W + 1];
            const int n = (a >= 0) + (b >= 0) + (c2 >= 0) + (d >= 0);
            if (n >= 3) { root = a >= 0 ? a : b; val = n == 4 ? 2 : 1; }      // (parent[] is flat after cc_count_kernel)
        }
        if (__builtin_amdgcn_ballot_w64(root != cur && val != 0)) {          // some lane's run of one root ends (wave-uniform branch)
            const bool flush = root != cur && val != 0;
            wave_add_by_root(area2, flush ? cur : -1, sum);
            if (flush) { cur = root; sum = 0; }
        }
        sum += val;
    }
    wave_add_by_root(area2, cur, sum);
}
// bounding box per root: {min x, min y, max x, max y} in four arrays indexed by root (initialised by cc_box_init_kernel)
__global__ __launch_bounds__(256) void cc_box_init_kernel(const int* parent, int* area2, int* bx0, int* by0, int* bx1, int* by1, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    area2[i] = 0;
    if (parent[i] == (int)i) { bx0[i] = 1 << 30; by0[i] = 1 << 30; bx1[i] = -1; by1[i] = -1; }
}
__global__ __launch_bounds__(256) void cc_box_kernel(const int* parent, int* bx0, int* by0, int* bx1, int* by1, int H, int W)
{
    // a WAVE per 64 strips of 64 pixels (row-major strips), a pixel per lane per step (coalesced); a lane keeps the x / y extent of its
    // pixels while their root stays the same, equal roots across the lanes are merged by wave_minmax_by_root
    const long strips_per_row = (W + 63) / 64, n_strips = strips_per_row * H;
    const long first = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    const int lane = threadIdx.x & 63;
    int cur = -1, lox = 0, hix = 0, loy = 0, hiy = 0;
    for (int k = 0; k < 64; ++k) {
        const long sidx = first + k;
        const bool live = sidx < n_strips;
        const int y = live ? (int)(sidx / strips_per_row) : 0;
        const int x = live ? (int)(sidx - (long)y * strips_per_row) * 64 + lane : 0;
        const int r = (live && x < W) ? parent[(long)y * W + x] : -1;
        if (__builtin_amdgcn_ballot_w64(r >= 0 && r != cur)) {     // some lane meets another root: flush its extent (wave-uniform branch;
            const bool flush = r >= 0 && r != cur;                 // background pixels and the padding of a row's last strip end nothing)
            wave_minmax_by_root(bx0, bx1, flush ? cur : -1, lox, hix);
            wave_minmax_by_root(by0, by1, flush ? cur : -1, loy, hiy);
            if (flush) { cur = r; lox = x; hix = x; loy = y; hiy = y; }
        }
        if (r >= 0) { lox = min(lox, x); hix = max(hix, x); loy = min(loy, y); hiy = max(hiy, y); }
    }
    wave_minmax_by_root(bx0, bx1, cur, lox, hix);
    wave_minmax_by_root(by0, by1, cur, loy, hiy);
}
// best = max over roots of (area2 lower bound, then LARGEST root index: the reference's np.argmax over OpenCV's contour list, which
// runs in reverse discovery order, keeps the last-discovered of equal areas -- contour_host.h host_largest_contour); key = area2 << 32 | root + 1
__global__ __launch_bounds__(256) void cc_best_area_kernel(const int* parent, const int* area2, long n, unsigned long long* best)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long key = 0;
    if (i < n && parent[i] == (int)i) key = ((unsigned long long)(unsigned)area2[i] << 32) | ((unsigned)i + 1u);
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}
// out[0..3] = bounding box of the best root, out[4] = its pixel count, out[5] = number of RIVALS -- other roots whose upper bound
// 2 (w - 1)(h - 1) exceeds the best lower bound (or ties it with a larger index) -- and out[6..] the first kCcMaxRivals of them:
// with rivals the ranking is not decided here
__global__ __launch_bounds__(256) void cc_decide_kernel(const int* parent, const int* count, const int* bx0, const int* by0, const int* bx1,
                                                        const int* by1, long n, const unsigned long long* best, int* out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long key = *best;
    if (!key || i >= n || parent[i] != (int)i) return;
    const int root = (int)((unsigned)(key & 0xffffffffu) - 1u);
    const long long best_lo = (long long)(key >> 32);
    if ((int)i == root) {
        out[0] = bx0[i]; out[1] = by0[i]; out[2] = bx1[i]; out[3] = by1[i]; out[4] = count[i];
        return;
    }
    const long long hi2 = 2ll * (bx1[i] - bx0[i]) * (by1[i] - by0[i]);
    if (hi2 > best_lo || (hi2 == best_lo && (int)i > root)) {
        const int k = atomicAdd(&out[5], 1);                     // out[5] = number of undecided rivals, out[6 + k] = their roots
        if (k < kCcMaxRivals) out[6 + k] = (int)i;
    }
}

// d_out: int[6 + kCcMaxRivals] = {min x, min y, max x, max y, pixels, rivals, rival roots...} of the component with the largest
// contour-area lower bound ({2^30, 2^30, -1, -1, 0, 0} if the mask is empty); d_best: its (area2 << 32 | root + 1) key.  scratch: five int arrays of H * W.
hipError_t launch_largest_contour(const uint8_t* mask, int H, int W, int* parent, int* count, int* area2, int* bx0, int* by0, int* bx1,
                                  int* by1, unsigned long long* d_best, int* d_out, hipStream_t s)
{
    const long n = (long)H * W;
    static const int init_out[6] = {1 << 30, 1 << 30, -1, -1, 0, 0};
    hipError_t e = hipMemsetAsync(d_best, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(d_out, init_out, sizeof(init_out), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cc_rows_kernel, dim3((unsigned)H), dim3(64), 0, s, mask, parent, count, H, W);
    hipLaunchKernelGGL(cc_link_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mask, parent, H, W);
    hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)((n + 256 * 64 - 1) / (256 * 64))), dim3(256), 0, s, parent, count, n);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, parent, n);
    hipLaunchKernelGGL(cc_box_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int*)parent, area2, bx0, by0, bx1, by1, n);
    if (H > 1 && W > 1) {
        const long cell_strips = (long)((W - 1 + 63) / 64) * (H - 1);
        hipLaunchKernelGGL(cc_cell_area_kernel, dim3((unsigned)((cell_strips + 255) / 256)), dim3(256), 0, s, (const int*)parent, area2, H, W);
    }
    const long strips = (long)((W + 63) / 64) * H;
    hipLaunchKernelGGL(cc_box_kernel, dim3((unsigned)((strips + 255) / 256)), dim3(256), 0, s, (const int*)parent, bx0, by0, bx1, by1, H, W);
    hipLaunchKernelGGL(cc_best_area_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int*)parent, (const int*)area2, n, d_best);
    hipLaunchKernelGGL(cc_decide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int*)parent, (const int*)count, (const int*)bx0,
                       (const int*)by0, (const int*)bx1, (const int*)by1, n, (const unsigned long long*)d_best, d_out);
    return hipGetLastError();
}

// ---- the PARENTLESS components of a labelled plane (cv2.findContours(RETR_TREE): hierarchy[..][3] == -1, main.py:88).  An
// 8-connected component has no parent when it is 4-adjacent to the background that is 4-connected to the frame around the image;
// an island inside another component's hole is not.  So: label the COMPLEMENT with 4-connectivity (the same union-find), flag the
// background components that reach the image border, and mark every foreground root one of whose pixels lies on the border or
// next to flagged background.  The marked roots are then compacted into a list of {root, x0, y0, x1, y1, area2 lower bound}.
__global__ __launch_bounds__(256) void cc_invert_kernel(const uint8_t* mask, uint8_t* inv, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) inv[i] = mask[i] ? 0 : 255;
}
__global__ __launch_bounds__(256) void cc_link4_kernel(const uint8_t* mask, int* parent, int H, int W)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
    if (y == 0 || !mask[idx] || !mask[idx - W]) return;
    // only the left end of a contact between two row runs makes the union (see cc_link_kernel)
    if (x > 0 && mask[idx - 1] && mask[idx - W - 1]) return;
    cc_union(parent, (int)idx, (int)(idx - W));
}
// flag[root] = 1 for every background component with a pixel on the image border (flag[] is zero on entry)
__global__ __launch_bounds__(256) void cc_frame_flag_kernel(const int* bg_parent, int* flag, int H, int W)
{
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    long i;
    if (k < W) i = k;                                                  // top row
    else if (k < 2L * W) i = (long)(H - 1) * W + (k - W);              // bottom row
    else if (k < 2L * W + H) i = (k - 2L * W) * W;                     // left column
    else if (k < 2L * W + 2L * H) i = (k - 2L * W - H) * W + (W - 1);  // right column
    else return;
    const int r = bg_parent[i];
    if (r >= 0) flag[r] = 1;
}
// touch[root] = 1 for every foreground component that is 4-adjacent to the frame or to flagged background (touch[] is zero on entry;
// all writers store the same value)
__global__ __launch_bounds__(256) void cc_touch_kernel(const int* parent, const int* bg_parent, const int* flag, int* touch, int H, int W)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)H * W) return;
    const int r = parent[i];
    if (r < 0) return;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    bool t = x == 0 || y == 0 || x == W - 1 || y == H - 1;
    if (!t) {
        const long nb[4] = {i - 1, i + 1, i - W, i + W};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int b = bg_parent[nb[q]];
            if (b >= 0 && flag[b]) t = true;
        }
    }
    if (t) touch[r] = 1;
}
__global__ __launch_bounds__(256) void cc_collect_roots_kernel(const int* parent, const int* touch, const int* area2, const int* bx0, const int* by0,
                                                               const int* bx1, const int* by1, long n, int* n_found, int* list, int cap)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || parent[i] != (int)i || !touch[i]) return;
    const int k = atomicAdd(n_found, 1);                       // the list's order is arbitrary: the host sorts it by root
    if (k >= cap) return;
    int* rec = list + (size_t)k * 6;
    rec[0] = (int)i; rec[1] = bx0[i]; rec[2] = by0[i]; rec[3] = bx1[i]; rec[4] = by1[i]; rec[5] = area2[i];
}

// After launch_largest_contour on the same plane (parent flat; area2 / boxes per root in place).  inv: u8 scratch plane; bg: two int
// planes of H * W (labels of the complement, border flags); touch: an int plane of H * W (launch_largest_contour's `count` may be
// given: the pixel counts are lost).  d_n: the number of parentless roots, list: the first `cap` of them, 6 ints each.
hipError_t launch_parentless_roots(const uint8_t* mask, uint8_t* inv, int H, int W, const int* parent, int* bg, int* touch, const int* area2,
                                   const int* bx0, const int* by0, const int* bx1, const int* by1, int* d_n, int* list, int cap, hipStream_t s)
{
    const long n = (long)H * W;
    const unsigned grid = (unsigned)((n + 255) / 256);
    int* bg_parent = bg;
    int* flag = bg + n;
    hipError_t e = hipMemsetAsync(d_n, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(touch, 0, (size_t)n * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cc_invert_kernel, dim3(grid), dim3(256), 0, s, mask, inv, n);
    hipLaunchKernelGGL(cc_rows_kernel, dim3((unsigned)H), dim3(64), 0, s, (const uint8_t*)inv, bg_parent, flag, H, W);      // (zeroes flag[])
    hipLaunchKernelGGL(cc_link4_kernel, dim3(grid), dim3(256), 0, s, (const uint8_t*)inv, bg_parent, H, W);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid), dim3(256), 0, s, bg_parent, n);
    hipLaunchKernelGGL(cc_frame_flag_kernel, dim3((unsigned)((2L * W + 2L * H + 255) / 256)), dim3(256), 0, s, (const int*)bg_parent, flag, H, W);
    hipLaunchKernelGGL(cc_touch_kernel, dim3(grid), dim3(256), 0, s, parent, (const int*)bg_parent, (const int*)flag, touch, H, W);
    hipLaunchKernelGGL(cc_collect_roots_kernel, dim3(grid), dim3(256), 0, s, parent, (const int*)touch, area2, bx0, by0, bx1, by1, n, d_n, list, cap);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// deskew_profile_kernel -- the rotate-and-project of the deskew search (main.py:1601-1718): for every angle of a sweep,
// the region mask (centred on a zero square of side S, main.py:1613-1621) is rotated as rotate_image does (main.py:159-163:
// cv2.warpAffine, INTER_CUBIC, BORDER_REPLICATE), binarised (!= 0, main.py:1642) and summed along its rows (main.py:1546).
// One block per (row, angle).  OpenCV's arithmetic [EXT, 4.5.1 imgwarp.cpp]: source coordinates in fixed point with 5
// fractional bits (AB_BITS = 10, round-half-even), 4 x 4 taps with the float bicubic table (A = -0.75), taps accumulated
// one by one in float64.  Floating-point contraction is off: the integer coordinates must come out of the same roundings
// as on the host.  HBM-trivial (the mask is L2-resident); 16 taps are only evaluated where the 4 x 4 window meets the patch.
// ------------------------------------------------------------------------------------------------
struct DeskewParams {
    const uint8_t* mask;      // [H][W] region mask (device)
    int H, W, S, top, left;   // square side, placement of the patch inside the square
    const double* minv;       // [n_angles][6] inverse affine maps (destination -> source), row-major 2 x 3
    const float* cubic;       // [32][4]
    int* counts;              // [n_angles][S]
};

__global__ __launch_bounds__(256) void deskew_profile_kernel(const DeskewParams p)
{
#pragma clang fp contract(off)
    __shared__ float tab[32 * 4];
    __shared__ int total;
    const int y = blockIdx.x, a = blockIdx.y, tid = threadIdx.x;
    if (tid < 128) tab[tid] = p.cubic[tid];
    if (tid == 0) total = 0;
    __syncthreads();
    const double* m = p.minv + (size_t)a * 6;
    const long long X0 = __double2ll_rn((m[1] * (double)y + m[2]) * 1024.0) + 16;
    const long long Y0 = __double2ll_rn((m[4] * (double)y + m[5]) * 1024.0) + 16;
    int cnt = 0;
    for (int x = tid; x < p.S; x += 256) {
        const long long X = (X0 + __double2ll_rn(m[0] * (double)x * 1024.0)) >> 5;
        const long long Y = (Y0 + __double2ll_rn(m[3] * (double)x * 1024.0)) >> 5;
        long long sx = X >> 5, sy = Y >> 5;
        sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
        sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
        const int ax = (int)(X & 31), ay = (int)(Y & 31);
        // window rows sy-1 .. sy+2, columns sx-1 .. sx+2, clamped to the square; non-zero source pixels only inside the patch
        const int x_lo = (int)min(max(sx - 1, 0LL), (long long)p.S - 1), x_hi = (int)min(max(sx + 2, 0LL), (long long)p.S - 1);
        const int y_lo = (int)min(max(sy - 1, 0LL), (long long)p.S - 1), y_hi = (int)min(max(sy + 2, 0LL), (long long)p.S - 1);
        if (x_hi < p.left || x_lo >= p.left + p.W || y_hi < p.top || y_lo >= p.top + p.H) continue;
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int yy = (int)min(max(sy - 1 + r, 0LL), (long long)p.S - 1) - p.top;
            const float wy = tab[ay * 4 + r];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int xx = (int)min(max(sx - 1 + cc, 0LL), (long long)p.S - 1) - p.left;
                const float w2 = wy * tab[ax * 4 + cc];                          // the 2-D table entry: a float product
                const bool in = (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
                const double v = in ? (double)p.mask[(size_t)yy * p.W + xx] : 0.0;
                sum = sum + v * (double)w2;
            }
        }
        cnt += sum != 0.0;
    }
    // wave reduction, then one atomic per wave
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) p.counts[(size_t)a * p.S + y] = total;
}

hipError_t launch_deskew_profiles(const uint8_t* mask, int H, int W, int S, int top, int left, const double* minv, const float* cubic,
                                  int n_angles, int* counts, hipStream_t s)
{
    DeskewParams p;
    p.mask = mask; p.H = H; p.W = W; p.S = S; p.top = top; p.left = left; p.minv = minv; p.cubic = cubic; p.counts = counts;
    hipLaunchKernelGGL(deskew_profile_kernel, dim3(S, n_angles), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace sbbseg
