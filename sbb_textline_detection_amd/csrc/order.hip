// order.hip -- the reading order of a page's text regions (order_of_regions, main.py:1802-1889) from the textline plane and the traced
// contours, both in device memory.  The arithmetic is order.h's, shared with the CPU entry points and bit for bit scipy's / numpy's float64
// results; this file only deals it out:
//   * row sums: one wave per row of the u8 plane, 16 bytes per lane and load between an unaligned head and tail (rows start anywhere when W
//     is odd), four bytes per v_sad_u8; the stored values are summed, not `!= 0`;
//   * band edges: one block takes the maximum, smooths the H + 80 flipped samples (radius 32, the weights wave-uniform through the scalar
//     cache) and compacts find_peaks' maxima in ascending order with a ballot per wave and the waves' counts in LDS;
//   * moments: one wave per contour.  The three terms of a point are exact integers for coordinates below 32768; the wave scans them as
//     int64, 64 points at a time in point order, carrying the totals.  While every prefix stays below 2^53 in magnitude the integer sum is
//     the reference's serial float64 sum; a contour where one does not is redone by lane 0 in the literal float64 order and flagged;
//   * rank: one block counts, per region, the (band, cx, index) keys below its own -- n^2 comparisons, 256 keys at a time through LDS.
// Every output is a plain vector store: no atomics, no scratch, no FMA contraction and no float64 divide sequence (a build test holds the
// kernels to that).
#include "device_prims.h"
#include "order.h"

namespace sbbseg {

namespace {

constexpr int kOrderBlock = 256;

__global__ __launch_bounds__(kOrderBlock) void row_sums_kernel(const uint8_t* __restrict__ plane, int H, int W, int32_t* __restrict__ sums)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * (kOrderBlock / 64) + (threadIdx.x >> 6);
    if (row >= H) return;                                           // (wave-uniform)
    const uint8_t* p = plane + (size_t)row * W;
    const uint8_t* end = p + W;
    const uint8_t* body = (const uint8_t*)(((uintptr_t)p + 15) & ~(uintptr_t)15);
    if (body > end) body = end;
    const long nvec = (long)(end - body) >> 4;
    const uint8_t* tail = body + nvec * 16;
    unsigned acc = 0;
    if (lane < (int)(body - p)) acc += p[lane];                     // fewer than 16 bytes
    const u4_t* v = (const u4_t*)body;
    for (long i = lane; i < nvec; i += 64) {
        const u4_t q = v[i];
        acc = __builtin_amdgcn_sad_u8(q[0], 0u, acc);
        acc = __builtin_amdgcn_sad_u8(q[1], 0u, acc);
        acc = __builtin_amdgcn_sad_u8(q[2], 0u, acc);
        acc = __builtin_amdgcn_sad_u8(q[3], 0u, acc);
    }
    if (lane < (int)(end - tail)) acc += tail[lane];                // fewer than 16 bytes
    const int total = wave_sum((int)acc);
    if (lane == 0) sums[row] = total;
}

__global__ __launch_bounds__(kOrderBlock) void order_edges_kernel(const OrderParams p)
{
#pragma clang fp contract(off)
    __shared__ int wave_val[kOrderBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, n = H + 4 * kOrderPad;
    const int32_t* y = p.row_sums;

    int top = 0;                                                    // max(y_padded) = max(0, max(y))
    for (int i = tid; i < H; i += kOrderBlock) top = max(top, y[i]);
    top = wave_max(top);
    if (lane == 0) wave_val[wave] = top;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kOrderBlock / 64; ++w) top = max(top, wave_val[w]);
    __syncthreads();

    for (int k = tid; k < n; k += kOrderBlock) p.smooth[k] = order_smooth_sample(y, H, top, p.weights, p.radius, k);
    __syncthreads();

    int ne = 1;                                                     // edges[0] = 0
    for (int base = 1; base < n - 1; base += kOrderBlock) {
        const int i = base + tid;
        int32_t e = 0;
        const bool keep = i < n - 1 && order_edge_at((const double*)p.smooth, n, i, &e);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_val[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kOrderBlock / 64; ++w) {
            const int cnt = wave_val[w];
            before += w < wave ? cnt : 0;
            total += cnt;
        }
        if (keep) p.edges[ne + before + __popcll(mask & ((1ull << lane) - 1ull))] = e;
        ne += total;
        __syncthreads();
    }
    if (tid == 0) {
        p.edges[0] = 0;
        p.edges[ne] = H;
        *p.n_edges = ne + 1;
    }
}

__global__ __launch_bounds__(64) void contour_moments_kernel(const OrderParams p)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, r = blockIdx.x;
    const long long first = p.point_off[r], cnt = p.point_off[r + 1] - first;       // block-uniform
    const int32_t* pts = p.points + 2 * first;
    long long c00 = 0, c10 = 0, c01 = 0;
    bool bad = false;
    for (long long base = 0; base < cnt && !bad; base += 64) {
        const long long k = base + lane;
        long long d = 0, tx = 0, ty = 0;
        bool ok = true;
        if (k < cnt) {
            const long long kp = k == 0 ? cnt - 1 : k - 1;
            const int x = pts[2 * k], yy = pts[2 * k + 1], xp = pts[2 * kp], yp = pts[2 * kp + 1];
            ok = order_coord_small(x) && order_coord_small(yy) && order_coord_small(xp) && order_coord_small(yp);
            if (ok) moments_terms(xp, yp, x, yy, &d, &tx, &ty);
        }
        d = wave_scan_sum(d, lane) + c00;
        tx = wave_scan_sum(tx, lane) + c10;
        ty = wave_scan_sum(ty, lane) + c01;
        ok = ok && order_prefix_exact(d) && order_prefix_exact(tx) && order_prefix_exact(ty);
        bad = __ballot(!ok) != 0ull;
        c00 = __shfl(d, 63, 64);
        c10 = __shfl(tx, 63, 64);
        c01 = __shfl(ty, 63, 64);
    }
    if (lane != 0) return;
    const OrderMoments m = bad ? moments_serial(pts, cnt, nullptr) : moments_finish((double)c00, (double)c10, (double)c01);
    p.moments[3 * (size_t)r] = m.m00; p.moments[3 * (size_t)r + 1] = m.m10; p.moments[3 * (size_t)r + 2] = m.m01;
    p.centroids[2 * (size_t)r] = m.cx; p.centroids[2 * (size_t)r + 1] = m.cy;
    p.serial[r] = bad ? 1 : 0;
}

__global__ __launch_bounds__(kOrderBlock) void order_rank_kernel(const OrderParams p)
{
    __shared__ int s_band[kOrderBlock];
    __shared__ double s_cx[kOrderBlock];
    const int tid = threadIdx.x, n = p.n, ne = *p.n_edges;
    for (int m = tid; m < n; m += kOrderBlock) p.band[m] = order_band(p.edges, ne, p.centroids[2 * (size_t)m + 1]);
    __syncthreads();
    for (int m0 = 0; m0 < n; m0 += kOrderBlock) {
        const int m = m0 + tid;
        const int bm = m < n ? p.band[m] : 0;
        const double cxm = m < n ? p.centroids[2 * (size_t)m] : 0.0;
        int rank = 0;
        for (int j0 = 0; j0 < n; j0 += kOrderBlock) {
            __syncthreads();
            if (j0 + tid < n) { s_band[tid] = p.band[j0 + tid]; s_cx[tid] = p.centroids[2 * (size_t)(j0 + tid)]; }
            __syncthreads();
            const int cnt = min(kOrderBlock, n - j0);
            if (m < n)
                for (int t = 0; t < cnt; ++t) rank += order_key_less(s_band[t], s_cx[t], j0 + t, bm, cxm, m) ? 1 : 0;
        }
        if (m < n) {
            p.sorted_index[rank] = m;
            p.order[m] = bm >= 0 ? rank : -1;
        }
    }
}

}  // namespace

hipError_t launch_row_sums(const OrderParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(row_sums_kernel, dim3((unsigned)((p.H + kOrderBlock / 64 - 1) / (kOrderBlock / 64))), dim3(kOrderBlock), 0, s, p.plane, p.H, p.W,
                       p.row_sums);
    return hipGetLastError();
}

hipError_t launch_order_edges(const OrderParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(order_edges_kernel, dim3(1), dim3(kOrderBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_contour_moments(const OrderParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(contour_moments_kernel, dim3((unsigned)p.n), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_order_rank(const OrderParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(order_rank_kernel, dim3(1), dim3(kOrderBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace sbbseg
